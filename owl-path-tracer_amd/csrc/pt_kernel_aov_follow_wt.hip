// pt_kernel_aov_follow_wt.hip -- the watertight instances of the follow kernels (option "watertight" = 1): pt_aov_follow.h with
// PT_WATERTIGHT = 1 (pt_aov_follow_wt_kernel behind pt_launch_aov_follow_wt / pt_aov_follow_geometry_wt; no binary-walk instance:
// that walk has no watertight test).
#define PT_WATERTIGHT 1
#include "pt_aov_follow.h"
