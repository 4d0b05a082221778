// pt_filter_tile.h -- what the three filter units (pt_denoise.hip and so pt_denoise_batch.hip, pt_denoise_var.hip, pt_upsample.hip) share
// on the device beside the per-pixel definitions of pt_filter_math.h: one pixel per lane, a wave = 64 consecutive pixels of one
// framebuffer row, a workgroup = 4 such rows (a 64 x 4 tile), no LDS; frames of a batch in blockIdx.z.
#pragma once
#include "pt_instance.h"

constexpr int PT_FILTER_TILE_W = 64, PT_FILTER_TILE_H = 4; // a wave per row of the tile
constexpr int PT_FILTER_BLOCK = PT_FILTER_TILE_W * PT_FILTER_TILE_H;

// The lane's pixel (x, row) of a W x H frame; false: the lane has none.
__device__ __forceinline__ bool pt_filter_pixel(int W, int H, int& x, int& row)
{
    x = (int)blockIdx.x * PT_FILTER_TILE_W + (int)threadIdx.x;
    row = (int)blockIdx.y * PT_FILTER_TILE_H + (int)threadIdx.y;
    return x < W && row < H;
}

inline dim3 pt_filter_block() { return dim3(PT_FILTER_TILE_W, PT_FILTER_TILE_H); }
inline dim3 pt_filter_grid(int W, int H, int frames = 1) { return dim3((W + PT_FILTER_TILE_W - 1) / PT_FILTER_TILE_W, (H + PT_FILTER_TILE_H - 1) / PT_FILTER_TILE_H, frames); }

// Geometry of the filter kernel fn over `frames` frames of W x H (block, *grid = the workgroups of all of them, vgprs, lds_bytes = 0);
// hipErrorInvalidConfiguration if fn needs scratch in this build.
inline hipError_t pt_filter_geometry(int W, int H, int frames, PtGeometry* g, int* grid, const void* fn)
{
    g->block = PT_FILTER_BLOCK;
    g->ns = PT_FILTER_BLOCK;
    g->lds_bytes = 0;
    g->lds_levels = 0;
    g->state_words = 0;
    const dim3 d = pt_filter_grid(W, H, frames);
    *grid = (int)(d.x * d.y * d.z);
    return pt_complete_geometry(g, fn);
}
