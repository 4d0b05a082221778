// pt_kernel_rays_surface.hip -- the surface instances of the ray kernels (pt_trace_surface: closest hit with the surface record at the
// hit): pt_rays_kernels.h with PT_RAYS_SURFACE = 1, which retires a lane through pt_surface.h.  Moeller-Trumbore; the watertight
// instances are pt_kernel_rays_surface_wt.hip.
#define PT_RAYS_SURFACE 1
#include "pt_rays_kernels.h"
