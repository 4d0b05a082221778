// pt_kernel_batch.hip -- the batch instances of the wavefront render kernel: K frames of one scene, each with its own camera and
// material table, in one launch sequence (pt_render_batch; DESIGN.md 4, "Batches").
//
// The body is pt_kernel.hip itself, compiled a second time with PT_BATCH = 1: same scheduler, same walks, same shading code, as
// pt_render_batch_kernel<COUNT, WAVES, EXACT> with the launchers pt_launch_render_batch / pt_batch_kernel_geometry.  A translation unit
// of its own, so that the five single-frame instances of pt_render_wave_kernel are compiled from exactly the tokens they were compiled
// from before batches existed (same registers, same code size: `make asm` / `make asm-batch` print both reports).
#define PT_BATCH 1
#include "pt_kernel.hip"
