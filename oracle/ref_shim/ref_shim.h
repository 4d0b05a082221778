/*
 * ref_shim.h -- stand-ins for the CUDA / OptiX / OWL surface that the reference's device code uses, so that its own
 * random.hpp, math.hpp, sample_methods.hpp, the disney/ headers and device.cu compile for the CPU (oracle/Makefile, target
 * `ref`; driver oracle/ref_device.cpp).  TEST INFRASTRUCTURE ONLY.  Nothing here is taken from OWL, OptiX or CUDA: the
 * declarations are written from the call sites in the reference.
 *
 * What the stand-ins define (and so what a comparison through them does NOT check):
 *   - OptiX traversal (owl::traceRay, optixGet*): closest hit over the flattened triangle soup, answered by
 *     orc_intersect through the oracle's BVH (equal to brute force: tests/test_oracle_render.py).  The closest-hit
 *     and miss programs that run are the reference's own.
 *   - texture filtering (tex2D): orc_tex_nearest, the oracle's reading of OWL_TEXTURE_NEAREST + CLAMP on RGBA8.
 *   - owl::make_rgba: orc_make_rgba (UNVERIFIED); the float colour is also kept for the driver.
 *   - the vector library: owl::dot = fma(z, z', fma(y, y', x x')), owl::cross as fma pairs, owl::normalize =
 *     v * (1/sqrt(dot(v,v))) -- the oracle's model of nvcc's code for OWL's vec.h.
 *   - float transcendentals (sin cos tan atan atan2 asin logf powf pow): the oracle's deterministic routines
 *     (orc_dm_*, tested against high precision in tests/test_oracle_libm.py), so both twins share one libm and differ
 *     only where their formulas or control flow differ.  sqrt, division, fmin/fmax are IEEE.
 * Everything else -- every formula, constant, branch, RNG draw and the path loop -- is the reference's text.
 *
 * No <cmath>/<math.h>/<cstdlib> here: the float overloads below must be the only candidates for the reference's
 * unqualified sin(float), abs(float), pow(float, float) ... (as CUDA's headers make them), and <stdlib.h> would
 * declare ::random(), which hides the reference's `struct random`.
 */
#ifndef REF_SHIM_H
#define REF_SHIM_H

#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "pt_oracle.h"

#define __device__
#define __host__
#define __both__
#define __constant__
#define __forceinline__ inline

/* macros.hpp traps with PTX `asm("trap;")` */
#define asm(x) __builtin_trap()

/* ---- CUDA vector types and runtime handles ---- */
struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
typedef unsigned long long cudaTextureObject_t;
typedef unsigned long long OptixTraversableHandle;

enum OptixRayFlags : unsigned {
    OPTIX_RAY_FLAG_NONE = 0u,
    OPTIX_RAY_FLAG_DISABLE_ANYHIT = 1u << 0,
    OPTIX_RAY_FLAG_ENFORCE_ANYHIT = 1u << 1,
    OPTIX_RAY_FLAG_TERMINATE_ON_FIRST_HIT = 1u << 2,
};

/* ---- CUDA float math, global scope (as the reference calls it unqualified) ---- */
inline float fmaxf_ieee(float a, float b) { return (b != b || a > b) ? a : b; } /* fmaxf: a NaN operand is ignored */
inline float fminf_ieee(float a, float b) { return (b != b || a < b) ? a : b; }
inline float fmax(float a, float b) { return fmaxf_ieee(a, b); }
inline float fmin(float a, float b) { return fminf_ieee(a, b); }
inline float max(float a, float b) { return fmaxf_ieee(a, b); }
inline float min(float a, float b) { return fminf_ieee(a, b); }
inline float abs(float x) { return __builtin_fabsf(x); }
inline float sqrt(float x) { return __builtin_sqrtf(x); }
inline bool isinf(float x) { return __builtin_fabsf(x) == __builtin_inff(); }
inline bool isnan(float x) { return x != x; }
inline float ldexpf(float x, int e) { return __builtin_ldexpf(x, e); }
inline float sin(float x) { return orc_dm_sin(x); }
inline float cos(float x) { return orc_dm_cos(x); }
inline float tan(float x) { return orc_dm_tan(x); }
inline float atan(float x) { return orc_dm_atan(x); }
inline float atan2(float y, float x) { return orc_dm_atan2(y, x); }
inline float asin(float x) { return orc_dm_asin(x); }
inline float logf(float x) { return orc_dm_log(x); }
inline float powf(float x, float y) { return orc_dm_pow(x, y); }
inline float pow(float x, float y) { return orc_dm_pow(x, y); }

/* ---- owl/common/math/vec.h ---- */
namespace owl {

template <typename T> struct vec4_t;

template <typename T> struct vec2_t {
    union { T x; T u; };
    union { T y; T v; };
    vec2_t() : x(0), y(0) {}
    vec2_t(T s) : x(s), y(s) {}
    vec2_t(T a, T b) : x(a), y(b) {}
    template <typename U> explicit vec2_t(const vec2_t<U>& o) : x(T(o.x)), y(T(o.y)) {}
    vec2_t(const float2& f) : x(f.x), y(f.y) {}
    T& operator[](int i) { return i ? y : x; }
    const T& operator[](int i) const { return i ? y : x; }
};

template <typename T> struct vec3_t {
    T x, y, z;
    vec3_t() : x(0), y(0), z(0) {}
    vec3_t(T s) : x(s), y(s), z(s) {}
    vec3_t(T a, T b, T c) : x(a), y(b), z(c) {}
    template <typename U> explicit vec3_t(const vec3_t<U>& o) : x(T(o.x)), y(T(o.y)), z(T(o.z)) {}
    explicit vec3_t(const vec4_t<T>& o) : x(o.x), y(o.y), z(o.z) {}
    vec3_t(const float3& f) : x(f.x), y(f.y), z(f.z) {}
    T& operator[](int i) { return i == 0 ? x : (i == 1 ? y : z); }
    const T& operator[](int i) const { return i == 0 ? x : (i == 1 ? y : z); }
};

template <typename T> struct vec4_t {
    T x, y, z, w;
    vec4_t() : x(0), y(0), z(0), w(0) {}
    vec4_t(T s) : x(s), y(s), z(s), w(s) {}
    vec4_t(T a, T b, T c, T d) : x(a), y(b), z(c), w(d) {}
    vec4_t(const float4& f) : x(f.x), y(f.y), z(f.z), w(f.w) {}
};

typedef vec2_t<float> vec2f;
typedef vec2_t<int32_t> vec2i;
typedef vec2_t<uint32_t> vec2ui;
typedef vec3_t<float> vec3f;
typedef vec3_t<int32_t> vec3i;
typedef vec3_t<uint32_t> vec3ui;
typedef vec4_t<float> vec4f;

#define REF_SHIM_BINOP(op)                                                                                                   \
    template <typename T> inline vec2_t<T> operator op(const vec2_t<T>& a, const vec2_t<T>& b) { return {a.x op b.x, a.y op b.y}; } \
    template <typename T> inline vec2_t<T> operator op(const vec2_t<T>& a, T s) { return {a.x op s, a.y op s}; }                \
    template <typename T> inline vec2_t<T> operator op(T s, const vec2_t<T>& a) { return {s op a.x, s op a.y}; }                \
    template <typename T> inline vec3_t<T> operator op(const vec3_t<T>& a, const vec3_t<T>& b)                                   \
    {                                                                                                                        \
        return {a.x op b.x, a.y op b.y, a.z op b.z};                                                                         \
    }                                                                                                                        \
    template <typename T> inline vec3_t<T> operator op(const vec3_t<T>& a, T s) { return {a.x op s, a.y op s, a.z op s}; }      \
    template <typename T> inline vec3_t<T> operator op(T s, const vec3_t<T>& a) { return {s op a.x, s op a.y, s op a.z}; }      \
    template <typename T> inline vec3_t<T>& operator op##=(vec3_t<T>& a, const vec3_t<T>& b) { return a = a op b; }             \
    template <typename T> inline vec3_t<T>& operator op##=(vec3_t<T>& a, T s) { return a = a op s; }
REF_SHIM_BINOP(+)
REF_SHIM_BINOP(-)
REF_SHIM_BINOP(*)
REF_SHIM_BINOP(/)
#undef REF_SHIM_BINOP

template <typename T> inline vec3_t<T> operator-(const vec3_t<T>& a) { return {-a.x, -a.y, -a.z}; }

inline float dot(const vec3f& a, const vec3f& b) { return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x)); }
inline vec3f cross(const vec3f& a, const vec3f& b)
{
    return {__builtin_fmaf(a.y, b.z, -(a.z * b.y)), __builtin_fmaf(a.z, b.x, -(a.x * b.z)), __builtin_fmaf(a.x, b.y, -(a.y * b.x))};
}
inline vec3f normalize(const vec3f& v) { return v * (1.0f / __builtin_sqrtf(dot(v, v))); }

inline float sqrt(float x) { return __builtin_sqrtf(x); }
inline vec3f sqrt(const vec3f& v) { return {sqrt(v.x), sqrt(v.y), sqrt(v.z)}; }
inline float abs(float x) { return __builtin_fabsf(x); }
inline float max(float a, float b) { return fmaxf_ieee(a, b); }
inline float min(float a, float b) { return fminf_ieee(a, b); }
inline float clamp(float x, float lo, float hi) { return min(max(x, lo), hi); }
inline vec3f clamp(const vec3f& x, const vec3f& lo, const vec3f& hi)
{
    return {clamp(x.x, lo.x, hi.x), clamp(x.y, lo.y, hi.y), clamp(x.z, lo.z, hi.z)};
}
inline float sin(float x) { return orc_dm_sin(x); }
inline float cos(float x) { return orc_dm_cos(x); }

/* ---- owl/owl_device.h ---- */
namespace device {
struct Buffer {
    size_t count;
    void* data;
};
} // namespace device

template <int RAY_TYPE, int NUM_RAY_TYPES> struct RayT {
    enum { rayType = RAY_TYPE, numRayTypes = NUM_RAY_TYPES };
    RayT() = default;
    RayT(const vec3f& o, const vec3f& d, float t0, float t1) : origin(o), direction(d), tmin(t0), tmax(t1) {}
    vec3f origin, direction;
    float tmin = 0.0f, tmax = 1e30f;
};

} // namespace owl

/* the launch state the stand-ins answer from; set by oracle/ref_device.cpp */
struct ref_shim_state {
    const void* program_data;
    owl::vec2i launch_index;
    void* prd;
    float2 bary;
    float t;
    float3 direction;
    unsigned primitive;
    owl::vec3f last_rgba_color; /* float colour of the last make_rgba call */
};
extern thread_local ref_shim_state g_ref_shim;

/* closest hit over the scene `world` (ray type 0: closest-hit program, ray type 1: shadow), defined by the driver */
void ref_shim_trace(OptixTraversableHandle world, int ray_type, const owl::vec3f& org, const owl::vec3f& dir, float tmin, float tmax,
                    void* prd);
float4 ref_shim_tex2d(cudaTextureObject_t tex, float u, float v);

namespace owl {
template <typename T> inline const T& getProgramData() { return *static_cast<const T*>(g_ref_shim.program_data); }
template <typename T> inline T& getPRD() { return *static_cast<T*>(g_ref_shim.prd); }
inline vec2i getLaunchIndex() { return g_ref_shim.launch_index; }

template <typename RAY, typename PRD> inline void traceRay(OptixTraversableHandle world, const RAY& ray, PRD& prd, uint32_t flags = 0)
{
    (void)flags;
    ref_shim_trace(world, RAY::rayType, ray.origin, ray.direction, ray.tmin, ray.tmax, &prd);
}

inline uint32_t make_rgba(const vec3f& c)
{
    g_ref_shim.last_rgba_color = c;
    const float a[3] = {c.x, c.y, c.z};
    return orc_make_rgba(a);
}
} // namespace owl

inline float2 optixGetTriangleBarycentrics() { return g_ref_shim.bary; }
inline float optixGetRayTmax() { return g_ref_shim.t; }
inline float3 optixGetWorldRayDirection() { return g_ref_shim.direction; }
inline unsigned optixGetPrimitiveIndex() { return g_ref_shim.primitive; }

template <typename T> T tex2D(cudaTextureObject_t tex, float u, float v);
template <> inline float4 tex2D<float4>(cudaTextureObject_t tex, float u, float v) { return ref_shim_tex2d(tex, u, v); }

/* program entry points become plain functions the driver calls */
#define OPTIX_RAYGEN_PROGRAM(name) void ref_raygen_##name
#define OPTIX_CLOSEST_HIT_PROGRAM(name) void ref_closest_hit_##name
#define OPTIX_MISS_PROGRAM(name) void ref_miss_##name

/* ---- fmt/color.h (types.hpp names a few terminal colours) ---- */
namespace fmt {
enum class terminal_color { red, green, yellow, magenta, bright_cyan, bright_magenta };
}

#endif
