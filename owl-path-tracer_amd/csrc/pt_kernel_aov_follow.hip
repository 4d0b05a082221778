// pt_kernel_aov_follow.hip -- the follow kernels of pt_render_aov_follow (the guide ray passes mirrors and glass): pt_aov_follow.h around
// the device functions the first-hit guide kernels take (pt_kernel_aov.hip), and no other kernel.  Moeller-Trumbore; the watertight
// instances are pt_kernel_aov_follow_wt.hip.
#include "pt_aov_follow.h"
