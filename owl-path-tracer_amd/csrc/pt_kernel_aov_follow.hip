// pt_kernel_aov_follow.hip -- the follow kernels of pt_render_aov_follow (the guide ray passes mirrors and glass): pt_kernel.hip with
// PT_AOV = 2, i.e. the device functions the first-hit guide kernels take (pt_kernel_aov.hip) around pt_aov_follow_kernel and its
// launcher, and no other kernel.  Moeller-Trumbore; the watertight instances are pt_kernel_aov_follow_wt.hip.
#define PT_AOV 2
#include "pt_kernel.hip"
