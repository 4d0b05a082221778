/* stand-in header: the whole CUDA / OptiX / OWL surface the reference device code uses is in ref_shim.h */
#include "ref_shim.h"
