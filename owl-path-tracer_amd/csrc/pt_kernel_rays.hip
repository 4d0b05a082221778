// pt_kernel_rays.hip -- the ray kernels of pt_trace_closest / pt_trace_occluded (closest hit and occlusion for the caller's rays):
// pt_rays_kernels.h around the device functions of pt_trace.h (node4_step, ray_inv, leaf_test, stack_pop), and none of the render,
// probe or guide kernels.  Moeller-Trumbore; the watertight instances are pt_kernel_rays_wt.hip.
#include "pt_rays_kernels.h"
