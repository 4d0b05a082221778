// pt_kernel_rays_hits.hip -- the first-K-hits kernel of pt_trace_hits (include/mi355pt.h, "ray queries: the first K hits"):
// pt_hits.h with the Moeller-Trumbore test, two instances (the slab forms).
#include "pt_hits.h"
