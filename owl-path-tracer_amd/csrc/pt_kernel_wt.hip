// pt_kernel_wt.hip -- the watertight instances of the wavefront render kernel and of the ray probes (option "watertight" = 1; DESIGN.md
// 2.1 and 4, "Watertight instances").
//
// The body is pt_kernel.hip itself, compiled a third time with PT_WATERTIGHT = 1: same scheduler, same walks, same shading code; every
// triangle test - the quad walk's leaf_test pairs, the group walk's lane-per-triangle leaf, under both slab forms - is the test of Woop,
// Benthin and Wald in the fixed float32 sequence of pt_trace.h ("WATERTIGHT BUILD").  Instances: pt_render_wt_kernel<COUNT, WAVES, EXACT>
// (product budget, fallback budget and instrumented, each with its subtracting-slab twin where the single-frame build has one) behind
// pt_launch_render_wt / pt_wt_kernel_geometry, and the probe kernels behind pt_launch_probe_wt.  A translation unit of its own, so that
// the instances of pt_render_wave_kernel and pt_render_batch_kernel are compiled from exactly the tokens they were compiled from before
// (`make asm` / `make asm-batch` / `make asm-wt` print the three reports).
// Resource report of this file (VGPRs / scratch bytes per lane / code bytes): instrumented 194 / 0 / 71 012, fallback 140 / 0 / 54 168
// (subtracting slabs 54 400), product 128 / 0 / 54 272 (54 504): +3.4 KB over the Moeller-Trumbore instances, same register budgets.
// Closed meshes, 2 000 rays aimed at shared edges and vertices: 176 / 240 / 293 / 323 leaks with watertight = 0, none with 1.  The cost per
// frame has not been measured yet (tools/ab_bench.py toggle=watertight measures it); profiles/r09_watertight.json.
#define PT_WATERTIGHT 1
#include "pt_kernel.hip"
