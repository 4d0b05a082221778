// pt_denoise_batch.hip -- the batch instances of the denoiser's kernels (pt_denoise_batch: K frames of one size, each filtered by its own
// guides, in L + 2 launches): pt_denoise.hip with PT_DENOISE_BATCH = 1, i.e. pt_denoise_batch_{prepare,iter,finish}_kernel with the frame
// in blockIdx.z behind pt_launch_denoise_batch / pt_denoise_batch_geometry / pt_denoise_batch_workspace_bytes.  A translation unit of
// its own, so that pt_denoise.hip holds the three kernels it held (`make asm-denoise` / `make asm-denoise-batch` print both reports).
#define PT_DENOISE_BATCH 1
#include "pt_denoise.hip"
