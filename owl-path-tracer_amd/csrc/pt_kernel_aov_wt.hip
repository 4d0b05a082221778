// pt_kernel_aov_wt.hip -- the watertight instances of the guide kernels (option "watertight" = 1): pt_aov_first.h with PT_WATERTIGHT = 1
// (pt_aov_wt_kernel behind pt_launch_aov_wt / pt_aov_geometry_wt; no binary-walk instance: that walk has no watertight test).
#define PT_WATERTIGHT 1
#include "pt_aov_first.h"
