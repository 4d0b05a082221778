// pt_nogpu_stubs.cpp -- the kernel launchers of pt_kernel.hip / pt_lbvh.hip as stubs that fail: ONLY for the host-side sanitizer build
// (make -C csrc asan: libmi355pt_asan.so).  That build compiles the host sources (HOST_SRCS of the Makefile) with g++ -fsanitize=address,
// undefined so that the CPU tests and the garbled-input tests run the host paths of the library (scene flattening, BVH build and
// collapse, sharding, validation hooks) under ASan/UBSan; device code cannot be sanitized on this pool and a host-only context never
// reaches these functions (every render path refuses first: "no CPU fallback").  Not part of libmi355pt.so.
#include <hip/hip_runtime.h>

#include "pt_launch.h"

extern "C" {
hipError_t pt_launch_render(const PtKernelParams*, const PtKernelParams*, int, int, size_t, hipStream_t, int) { return hipErrorNotSupported; }
hipError_t pt_launch_debug(const PtKernelParams*, int, const float*, int, float*, int, long long, size_t, hipStream_t) { return hipErrorNotSupported; }
size_t pt_sort_scratch_bytes(uint32_t) { return 16; }
hipError_t pt_launch_plan_tiers(const uint32_t*, uint32_t, int, int, int, uint32_t*, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_launch_sort_pixels(const uint8_t*, int, int, int, const uint32_t*, uint32_t*, uint32_t, uint32_t, uint32_t*, uint8_t*, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_kernel_geometry(int, int, int, int, int, int, PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_render_batch(const PtKernelParams*, const PtKernelParams*, int, int, size_t, hipStream_t, int) { return hipErrorNotSupported; }
hipError_t pt_batch_kernel_geometry(int, int, int, int, int, int, PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_render_rayimage(const PtKernelParams*, const PtKernelParams*, int, int, size_t, hipStream_t, int) { return hipErrorNotSupported; }
hipError_t pt_rayimage_kernel_geometry(int, int, int, int, int, int, PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_render_wt(const PtKernelParams*, const PtKernelParams*, int, int, size_t, hipStream_t, int) { return hipErrorNotSupported; }
hipError_t pt_wt_kernel_geometry(int, int, int, int, int, int, PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_probe_wt(const PtKernelParams*, int, const float*, int, float*, int, long long, int, size_t, uint32_t*, hipStream_t) { return hipErrorNotSupported; }
int pt_debug_block(void) { return 256; }
hipError_t pt_launch_aov(const PtKernelParams*, const PtAovArgs*, int, int, size_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_aov_geometry(int, int, int, PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_aov_wt(const PtKernelParams*, const PtAovArgs*, int, int, size_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_aov_geometry_wt(int, int, int, PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_aov_follow(const PtKernelParams*, const PtAovFollowArgs*, int, int, size_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_aov_follow_geometry(int, int, int, PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_aov_follow_wt(const PtKernelParams*, const PtAovFollowArgs*, int, int, size_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_aov_follow_geometry_wt(int, int, int, PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_aov_follow_batch(const PtKernelParams*, const PtAovFollowArgs*, int, int, size_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_aov_follow_batch_geometry(int, int, int, PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_aov_rays(const PtKernelParams*, const PtAovFollowArgs*, int, int, size_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_aov_rays_geometry(int, int, int, PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_aov_rays_wt(const PtKernelParams*, const PtAovFollowArgs*, int, int, size_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_aov_rays_geometry_wt(int, int, int, PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_rays(const PtKernelParams*, const PtRaysArgs*, int, int, size_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_rays_geometry(int, int, PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_rays_wt(const PtKernelParams*, const PtRaysArgs*, int, int, size_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_rays_geometry_wt(int, int, PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_rays_surface(const PtKernelParams*, const PtRaysArgs*, int, int, size_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_rays_surface_geometry(int, int, PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_rays_surface_wt(const PtKernelParams*, const PtRaysArgs*, int, int, size_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_rays_surface_geometry_wt(int, int, PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_rays_ao(const PtKernelParams*, const PtAoArgs*, int, size_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_rays_ao_geometry(int, PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_rays_ao_wt(const PtKernelParams*, const PtAoArgs*, int, size_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_rays_ao_geometry_wt(int, PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_rays_hits(const PtKernelParams*, const PtHitsArgs*, int, size_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_rays_hits_geometry(int, int, PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_rays_hits_wt(const PtKernelParams*, const PtHitsArgs*, int, size_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_rays_hits_geometry_wt(int, int, PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_points(const PtKernelParams*, const PtRaysArgs*, int, size_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_points_geometry(PtGeometry*) { return hipErrorNotSupported; }
int pt_points_entry_words(void) { return 1; }
size_t pt_denoise_workspace_bytes(int, int) { return 16; }
hipError_t pt_denoise_geometry(int, int, PtGeometry*, int*) { return hipErrorNotSupported; }
hipError_t pt_launch_denoise(const PtDenoiseArgs*, hipStream_t) { return hipErrorNotSupported; }
size_t pt_denoise_batch_workspace_bytes(int, int, int) { return 16; }
hipError_t pt_denoise_batch_geometry(int, int, int, PtGeometry*, int*) { return hipErrorNotSupported; }
hipError_t pt_launch_denoise_batch(const PtDenoiseArgs*, int, hipStream_t) { return hipErrorNotSupported; }
size_t pt_denoise_var_workspace_bytes(int, int) { return 16; }
hipError_t pt_denoise_var_geometry(int, int, PtGeometry*, int*) { return hipErrorNotSupported; }
hipError_t pt_launch_denoise_var(const PtDenoiseVarArgs*, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_launch_accum_variance(const PtAccumVarArgs*, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_accum_geometry(PtGeometry*) { return hipErrorNotSupported; }
hipError_t pt_launch_accum_resolve(const PtAccumArgs*, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_launch_accum_select(const PtAccumSelectArgs*, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_accum_reproject_geometry(int, int, PtGeometry*, int*) { return hipErrorNotSupported; }
hipError_t pt_launch_accum_reproject(const PtAccumReprojectArgs*, hipStream_t) { return hipErrorNotSupported; }
size_t pt_upsample_workspace_bytes(int, int) { return 16; }
hipError_t pt_upsample_geometry(int, int, PtGeometry*, int*) { return hipErrorNotSupported; }
hipError_t pt_launch_upsample(const PtUpsampleArgs*, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_launch_probe(const PtKernelParams*, int, const float*, int, float*, int, long long, int, size_t, uint32_t*, hipStream_t) { return hipErrorNotSupported; }
int pt_probe_lds_stack(void) { return 12; }
size_t pt_probe_group_lds_bytes(int, int) { return 16; }
size_t pt_probe_group_state_words(void) { return 16; }
size_t pt_lbvh_workspace_bytes(int) { return 16; }
hipError_t pt_lbvh_build_device(const float*, int, int, void*, size_t, PtNode*, uint32_t*, int32_t*, int32_t*, int32_t*, int32_t*, float*, hipStream_t) { return hipErrorNotSupported; }
size_t pt_ploc_workspace_bytes(int) { return 16; }
hipError_t pt_ploc_build_device(const float*, int, int, void*, size_t, int*, float*, int*, uint32_t*, int32_t*, int32_t*, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_launch_store_params(const PtKernelParams*, PtKernelParams*, hipStream_t) { return hipErrorNotSupported; }
size_t pt_refit_workspace_bytes(void) { return 16; }
hipError_t pt_launch_refit(const PtRefitArgs*, hipEvent_t, hipEvent_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t pt_launch_pack_rgba8(const float*, uint32_t*, long long, hipStream_t) { return hipErrorNotSupported; }
}
