// pt_kernel_rayimage.hip -- the ray-image instances of the wavefront render kernel: every pixel starts its paths on a ray record of the
// caller's instead of a pinhole camera's ray (pt_render_rays; DESIGN.md 4, "Ray images").
//
// The body is pt_kernel.hip itself, compiled once more with PT_RAYGEN = 1: same scheduler, same walks, same shading code, as
// pt_render_rayimage_kernel<COUNT, WAVES, EXACT> with the launchers pt_launch_render_rayimage / pt_rayimage_kernel_geometry; the one
// difference is the ray generator (gen_ray_from, pt_trace.h).  A translation unit of its own, so that the instances of the other units
// are compiled from exactly the tokens they were compiled from before (same registers, same code size: `make asm` / `make asm-rayimage`
// print both reports).
#define PT_RAYGEN 1
#include "pt_kernel.hip"
