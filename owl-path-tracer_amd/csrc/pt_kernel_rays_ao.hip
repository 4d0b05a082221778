// pt_kernel_rays_ao.hip -- the fused ambient-occlusion kernel of pt_trace_ao (include/mi355pt.h, "ray queries: ambient occlusion"):
// pt_ao.h with the Moeller-Trumbore test, two instances (the slab forms).
#include "pt_ao.h"
