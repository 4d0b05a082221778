// pt_kernel_aov_follow_batch.hip -- the batch instances of the follow kernels (pt_render_aov_batch: the guide buffers of K frames of one
// scene, each with its own camera and material table, in one launch): pt_aov_follow.h with PT_BATCH = 1, i.e. the three
// instances of pt_aov_follow_batch_kernel (binary walk, quad walk with either slab form) behind pt_launch_aov_follow_batch /
// pt_aov_follow_batch_geometry, and no other kernel.  Moeller-Trumbore: batches have no watertight instances.  First-hit guides are
// max_follow = 0 of the same kernels.  A translation unit of its own, so that the single-frame follow instances are compiled from the
// tokens they were compiled from before (`make asm-aov-follow` / `make asm-aov-follow-batch` print both reports).
#define PT_BATCH 1
#include "pt_aov_follow.h"
