// pt_device_host.h -- pt_device.h for a host source: the device arithmetic as plain CPU functions, which is what makes a CPU twin the
// very text its kernel compiles.  pt_device.h and the per-element definitions built on it (pt_filter_math.h, pt_accum_math.h,
// pt_ao_math.h, pt_points_math.h) spell every function PTD.  A kernel unit leaves PTD alone and gets __device__ __forceinline__; a host
// source includes THIS header first, which sets PTD = static inline, and then its *_math.h: the same functions, run by the CPU under the
// same contract (binary32, -ffp-contract=off, fma only where spelled, correctly rounded division and sqrt).
// The two bit casts pt_device.h uses are device functions of the HIP headers, so they get host forms under the same names while
// pt_device.h is read; no *_math.h uses them.  Works under hipcc's host pass and under plain g++ (the sanitizer build) alike.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

static inline uint32_t pt_host_float_as_uint(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static inline float pt_host_uint_as_float(uint32_t u) { float x; std::memcpy(&x, &u, 4); return x; }
#define __float_as_uint pt_host_float_as_uint
#define __uint_as_float pt_host_uint_as_float
#define PTD static inline
#include "pt_device.h"
#undef __float_as_uint
#undef __uint_as_float
