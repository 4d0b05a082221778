// pt_accum.hip -- the progressive accumulation's two streaming kernels (pt_accum_*; include/mi355pt.h, "progressive accumulation"), gfx950.
// The per-pixel definition is pt_accum_math.h, which the CPU twins of pt_accum_host.cpp compile as well; tests/accum_ref.py restates it
// in numpy and the tests hold the three to each other bit for bit.  Arithmetic: the contract of pt_device.h (binary32,
// -ffp-contract=off, correctly rounded division and square root).
//
// One pixel per lane, no LDS, no scratch:
//   resolve   over the W x H pixels of the frame in launch order (id = x + W * y, the index of the render kernel's rng_state / accum):
//             updates seen / half / n / n_half / passes of the pixels that were active in this add, writes noise (by id) and the image
//             (framebuffer order x + W * (H - 1 - y)): 50 B read and up to 56 B written per owned pixel, all dword streams.
//   select    over the entries of the shard's pixel queue: the active flag by id, and the active ids compacted into the render's pixel
//             queue - one ballot and ONE device-scope atomic per wave on a counter that has its cache line to itself.  The order of the
//             compacted list follows the order in which waves arrive; the image does not depend on it.
#include <hip/hip_runtime.h>

#include "../../include/mi355pt.h"
#include "pt_accum_math.h"
#include "pt_instance.h"

using namespace ptd;

namespace {

constexpr int ACC_BLOCK = 256; // four waves

__global__ __launch_bounds__(ACC_BLOCK) void pt_accum_resolve_kernel(PtAccumArgs A)
{
    const uint32_t id = blockIdx.x * (uint32_t)ACC_BLOCK + threadIdx.x;
    if (id >= A.n_frame) return;
    const uint32_t x = id % (uint32_t)A.width, y = id / (uint32_t)A.width;
    const size_t ofs = (size_t)x + (size_t)A.width * (size_t)((uint32_t)A.height - 1u - y); // device.cu:251
    if (!A.owned[id]) { // +0 in every output; the state of such a pixel is never read
        A.out_rgb[3 * ofs] = 0.0f;
        A.out_rgb[3 * ofs + 1] = 0.0f;
        A.out_rgb[3 * ofs + 2] = 0.0f;
        A.out_rgba8[ofs] = 0u;
        return;
    }
    const bool active = A.all_active || A.active[id] != 0;
    AccumPixel s;
    for (int k = 0; k < 3; ++k) {
        s.sum[k] = A.sum[3 * (size_t)id + k];
        s.seen[k] = A.seen[3 * (size_t)id + k];
        s.half[k] = A.half[3 * (size_t)id + k];
    }
    s.n = A.n[id];
    s.n_half = A.n_half[id];
    s.passes = A.passes[id];
    AccumResolved o;
    accum_resolve_pixel(s, active, (uint32_t)A.n_samples, o);
    if (active) {
        for (int k = 0; k < 3; ++k) {
            A.seen[3 * (size_t)id + k] = s.seen[k];
            A.half[3 * (size_t)id + k] = s.half[k];
        }
        A.n[id] = s.n;
        A.n_half[id] = s.n_half;
        A.passes[id] = s.passes;
    }
    A.noise[id] = o.noise;
    A.out_rgb[3 * ofs] = o.rgb[0];
    A.out_rgb[3 * ofs + 1] = o.rgb[1];
    A.out_rgb[3 * ofs + 2] = o.rgb[2];
    A.out_rgba8[ofs] = o.rgba8;
}

__global__ __launch_bounds__(ACC_BLOCK) void pt_accum_select_kernel(PtAccumSelectArgs A)
{
    const uint32_t i = blockIdx.x * (uint32_t)ACC_BLOCK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u; // (the block is a multiple of the wave: every wave is whole, lanes past the queue vote no)
    uint32_t id = 0;
    bool act = false;
    if (i < A.n_queue) {
        id = A.queue[i];
        act = accum_select_pixel(A.noise[id], A.n[id], A.cap, A.threshold);
        A.active[id] = act ? 1 : 0;
    }
    const unsigned long long votes = __ballot(act);
    if (votes == 0ull) return; // (wave-uniform)
    uint32_t base = 0;
    if (lane == 0u) base = atomicAdd(A.count, (uint32_t)__popcll(votes));
    base = (uint32_t)__shfl((int)base, 0);
    if (act) A.ids_out[base + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull))] = id;
}

} // namespace

extern "C" hipError_t pt_accum_geometry(PtGeometry* g)
{
    const hipError_t e = pt_refuse_scratch({(const void*)pt_accum_select_kernel});
    if (e != hipSuccess) return e;
    g->block = ACC_BLOCK;
    g->ns = ACC_BLOCK;
    g->lds_bytes = 0;
    g->lds_levels = 0;
    g->state_words = 0;
    return pt_complete_geometry(g, (const void*)pt_accum_resolve_kernel);
}

extern "C" hipError_t pt_launch_accum_resolve(const PtAccumArgs* a, hipStream_t stream)
{
    if (a->n_frame == 0) return hipSuccess;
    hipLaunchKernelGGL(pt_accum_resolve_kernel, dim3((a->n_frame + ACC_BLOCK - 1) / ACC_BLOCK), dim3(ACC_BLOCK), 0, stream, *a);
    return hipGetLastError();
}

// *a->count must be 0 when the kernel starts (the caller clears it on `stream`).
extern "C" hipError_t pt_launch_accum_select(const PtAccumSelectArgs* a, hipStream_t stream)
{
    if (a->n_queue == 0) return hipSuccess;
    hipLaunchKernelGGL(pt_accum_select_kernel, dim3((a->n_queue + ACC_BLOCK - 1) / ACC_BLOCK), dim3(ACC_BLOCK), 0, stream, *a);
    return hipGetLastError();
}
