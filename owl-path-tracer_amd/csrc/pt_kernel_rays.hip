// pt_kernel_rays.hip -- the ray kernels of pt_trace_closest / pt_trace_occluded (closest hit and occlusion for the caller's rays):
// pt_kernel.hip with PT_AOV = 3, i.e. its device functions (node4_step, and through pt_trace.h ray_inv, leaf_test, stack_pop) around
// pt_rays_kernel and its launcher, and none of the render, probe or guide kernels.  Moeller-Trumbore; the watertight instances are
// pt_kernel_rays_wt.hip.
#define PT_AOV 3
#include "pt_kernel.hip"
