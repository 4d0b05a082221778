// pt_probes.h -- ray probes (tests only: pt_debug_eval ops PT_PROBE_*, pt_launch.h; tests/test_gpu_ray_probes.py)
//
// Caller-chosen rays through the walks of pt_render_wave_kernel: the kernels below own no traversal arithmetic, they call ray_inv,
// node4_step and leaf_test (through quad_walk_step, pt_trace.h) and traverse_groups (pt_kernel.hip) the way the render kernel does, and write the closest hit out
// per ray.  The group probe runs the render kernel's own WaveCtx, pick_pass and traverse_groups, which sit in the anonymous namespace
// of pt_kernel.hip: that file includes this header at its end, in the single-frame and the watertight build, and nothing else does.
// They are separate kernels, so the product instances' code does not change with them.
#pragma once
#if PT_WATERTIGHT // the watertight build's twins (pt_kernel_wt.hip)
#define PT_PROBE_QUAD_KERNEL pt_probe_quad_wt_kernel
#define PT_PROBE_GROUP_KERNEL pt_probe_group_wt_kernel
#define PT_PROBE_LAUNCH pt_launch_probe_wt
#define PT_PROBE_LDS_STACK pt_probe_lds_stack_wt
#define PT_PROBE_GROUP_LDS_BYTES pt_probe_group_lds_bytes_wt
#define PT_PROBE_GROUP_STATE_WORDS pt_probe_group_state_words_wt
#else
#define PT_PROBE_QUAD_KERNEL pt_probe_quad_kernel
#define PT_PROBE_GROUP_KERNEL pt_probe_group_kernel
#define PT_PROBE_LAUNCH pt_launch_probe
#define PT_PROBE_LDS_STACK pt_probe_lds_stack
#define PT_PROBE_GROUP_LDS_BYTES pt_probe_group_lds_bytes
#define PT_PROBE_GROUP_STATE_WORDS pt_probe_group_state_words
#endif

namespace {
__device__ __forceinline__ void probe_store(float* y, bool hit, float t, float u, float v, int id, float aux)
{
    y[0] = hit ? 1.0f : 0.0f; y[1] = t; y[2] = u; y[3] = v; y[4] = __int_as_float(hit ? id : -1); y[5] = aux;
}
} // namespace

// Quad walk, one ray per lane, one wave per workgroup (stack[level * 64 + lane] as in the render kernel).  LDS_ENTRIES = 0x7fffffff: the common
// instance of the step (whole stack in LDS; `cap` levels are allocated: the stack bound + the three stores above the top);
// LDS_ENTRIES = PT_LDS_STACK: the overflow-aware instance, levels >= PT_LDS_STACK in the wave's HBM columns.  EXACT as in the render kernel.
template <int LDS_ENTRIES, bool EXACT>
__global__ void __launch_bounds__(PT_WAVE) PT_PROBE_QUAD_KERNEL(const PtKernelParams P, const float* __restrict__ in, int in_stride, float* __restrict__ out, int out_stride,
                                                                long long n, uint32_t* ovf_area, int cap)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int lane = threadIdx.x;
    uint32_t* stack = lds + lane;
    const int ovf_levels = cap > P.lds_levels ? cap - P.lds_levels : 0;
    uint32_t PT_AS1* ovf = gp(ovf_area) + (size_t)blockIdx.x * ((size_t)ovf_levels * PT_WAVE) + lane;
    const PtNode4* __restrict__ nodes4 = P.nodes4;
    const PtTri* __restrict__ tris = P.tris;
    for (long long i = (long long)blockIdx.x * PT_WAVE + lane; i < n; i += (long long)gridDim.x * PT_WAVE) {
        const float* x = in + i * in_stride;
        const v3 o = V(x[0], x[1], x[2]), d = V(x[3], x[4], x[5]);
        const v3 inv = ray_inv(d);
        Hit h;
        hit_reset(h, kTMax);
        int cur = P.root, sp = 0, max_sp = 0, steps = 0;
        while (cur != PT_DONE) { // (a walk out of its bounds ends here too, with the best hit so far: quad_walk_step)
            quad_walk_step<LDS_ENTRIES>(P, nodes4, tris, stack, ovf, cap, o, d, inv, h, cur, sp, steps, EXACT, false);
            max_sp = sp > max_sp ? sp : max_sp; // sp falls only on a pop: the maximum is the one over the node steps
        }
        probe_store(out + i * out_stride, h.slot >= 0, h.t, h.u, h.v, h.id, (float)max_sp);
    }
}

// Group walk: a minimal wave context around traverse_groups.  The wave owns rays [first, first + per_wave) and ns path slots; its
// "shading pass" writes the queued hits and misses out and gives each of those slots the wave's next ray, exactly where shade_pass would
// emit the continuation ray.  The batch thresholds are small (8 / 4 / 4), so pick_pass ends most group phases with groups still walking:
// they are parked in HBM and resumed by the next phase.  lstate is one word per slot here: the ray the slot carries (PT_FRESH: none).
__global__ void __launch_bounds__(PT_WAVE) PT_PROBE_GROUP_KERNEL(const PtKernelParams P, const float* __restrict__ in, int in_stride, float* __restrict__ out,
                                                                 int out_stride, long long n, int per_wave, uint32_t* park_area)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int lane = threadIdx.x;
    const int ns = P.ns;
    uint32_t* lray = lds + P.lds_levels * PT_WAVE;
    uint32_t* lidx = lray + L_NFIELDS * ns;
    uint32_t PT_AS1* park = gp(park_area) + (size_t)blockIdx.x * (K_NFIELDS * PT_WAVE) + lane;
    WaveCtx w;
    w.lray = lray;
    w.lstate = lidx;
    w.ns = ns;
    w.rayq = reinterpret_cast<uint8_t*>(lidx + ns);
    w.hitq = w.rayq + ns;
    w.missq = w.hitq + ns;
    w.tier.counter = nullptr; w.tier.q0 = w.tier.count = 0u; w.tier.express = false;
    w.miss_blocked = false;
    w.topup_min = 0; w.topup = false;
    w.min_batch = 4; w.ray_low = 4; w.full_batch = 8;
    w.adapt = 0;
    w.n_run = 0;
    for (int i = lane; i < ns; i += PT_WAVE) {
        w.missq[i] = (uint8_t)i; // as in the render kernel: every slot starts fresh, in the miss queue
        lidx[i] = PT_FRESH;
    }
    w.ray_head = 0; w.ray_count = 0; w.hit_head = 0; w.hit_count = 0; w.miss_head = 0; w.miss_count = ns; w.n_dead = 0;
    const long long first = (long long)blockIdx.x * per_wave;
    const long long end = first + per_wave < n ? first + per_wave : n;
    long long next = first;
    int n_parked = 0, n_park_phases = 0, rounds = 0;
    Counters cn;
#define LF(f, s) lray[(f) * ns + (s)]
#define LFF(f, s) __uint_as_float(lray[(f) * ns + (s)])
    while (w.n_dead < ns) {
        if (++rounds > (1 << 20)) { // every round retires or walks at least one ray
            if (lane == 0) gp(P.error_flag)[0] = 1u;
            break;
        }
        // ---- "shading pass": all queued hits, then all queued misses (ns <= 64: one pass takes both queues whole) ----
        const int n1 = w.hit_count, n2 = w.miss_count, np = n1 + n2;
        if (np > 0) {
            const bool mine = lane < np, is_hit = lane < n1;
            const int slot = !mine ? 0 : (is_hit ? (int)w.hitq[w.wrap(w.hit_head + lane)] : (int)w.missq[w.wrap(w.miss_head + lane - n1)]);
            w.hit_head = w.wrap(w.hit_head + n1); w.hit_count = 0;
            w.miss_head = w.wrap(w.miss_head + n2); w.miss_count = 0;
            const long long mine_next = next + rank_in(__ballot(mine));
            bool to_ray = false, died = false;
            if (mine) {
                const uint32_t idx = lidx[slot];
                if (idx != PT_FRESH) {
                    const int tslot = is_hit ? (int)LF(L_AZ, slot) : -1;
                    const int id = is_hit ? gp(P.tris)[tslot].id : -1;
                    probe_store(out + (first + idx) * out_stride, is_hit, 0.0f, is_hit ? LFF(L_AX, slot) : 0.0f, is_hit ? LFF(L_AY, slot) : 0.0f, id, (float)n_park_phases);
                }
                if (mine_next < end) {
                    const float* x = in + mine_next * in_stride;
                    LF(L_AX, slot) = __float_as_uint(x[0]); LF(L_AY, slot) = __float_as_uint(x[1]); LF(L_AZ, slot) = __float_as_uint(x[2]);
                    LF(L_DIRX, slot) = __float_as_uint(x[3]); LF(L_DIRY, slot) = __float_as_uint(x[4]); LF(L_DIRZ, slot) = __float_as_uint(x[5]);
                    lidx[slot] = (uint32_t)(mine_next - first);
                    to_ray = true;
                } else {
                    lidx[slot] = PT_FRESH;
                    died = true;
                }
            }
            const unsigned long long m_ray = __ballot(to_ray);
            if (to_ray) w.rayq[w.wrap(w.wrap(w.ray_head + w.ray_count) + rank_in(m_ray))] = (uint8_t)slot;
            w.ray_count += popc64(m_ray);
            w.n_dead += popc64(__ballot(died));
            next += np;
            w.n_run = ns - w.n_dead;
        }
        // ---- group phase over the ray queue and the groups the last phase parked ----
        if (w.ray_count > 0 || n_parked > 0) {
            n_parked = traverse_groups<false>(P, w, lane, lds, park, n_parked, cn, P.box_exact != 0);
            n_park_phases += n_parked > 0 ? 1 : 0;
        }
    }
#undef LF
#undef LFF
}

extern "C" int PT_PROBE_LDS_STACK(void) { return PT_LDS_STACK; }
extern "C" size_t PT_PROBE_GROUP_LDS_BYTES(int lds_levels, int ns)
{
    return ((size_t)lds_levels * PT_WAVE + (size_t)(L_NFIELDS + 1) * ns) * 4 + (((size_t)3 * ns + 15) & ~(size_t)15);
}
extern "C" size_t PT_PROBE_GROUP_STATE_WORDS(void) { return (size_t)K_NFIELDS * PT_WAVE; }

extern "C" hipError_t PT_PROBE_LAUNCH(const PtKernelParams* p, int op, const float* in, int in_stride, float* out, int out_stride, long long n, int grid, size_t lds_bytes,
                                      uint32_t* scratch, hipStream_t stream)
{
    if (grid < 1) grid = 1;
    const int cap = p->stack_entries + 3;
    switch (op) {
    case PT_PROBE_QUAD: hipLaunchKernelGGL((PT_PROBE_QUAD_KERNEL<0x7fffffff, false>), dim3(grid), dim3(PT_WAVE), lds_bytes, stream, *p, in, in_stride, out, out_stride, n, scratch, cap); break;
    case PT_PROBE_QUAD + 1: hipLaunchKernelGGL((PT_PROBE_QUAD_KERNEL<0x7fffffff, true>), dim3(grid), dim3(PT_WAVE), lds_bytes, stream, *p, in, in_stride, out, out_stride, n, scratch, cap); break;
    case PT_PROBE_QUAD_OVF: hipLaunchKernelGGL((PT_PROBE_QUAD_KERNEL<PT_LDS_STACK, false>), dim3(grid), dim3(PT_WAVE), lds_bytes, stream, *p, in, in_stride, out, out_stride, n, scratch, cap); break;
    case PT_PROBE_QUAD_OVF + 1: hipLaunchKernelGGL((PT_PROBE_QUAD_KERNEL<PT_LDS_STACK, true>), dim3(grid), dim3(PT_WAVE), lds_bytes, stream, *p, in, in_stride, out, out_stride, n, scratch, cap); break;
    case PT_PROBE_GROUP:
    case PT_PROBE_GROUP + 1: hipLaunchKernelGGL(PT_PROBE_GROUP_KERNEL, dim3(grid), dim3(PT_WAVE), lds_bytes, stream, *p, in, in_stride, out, out_stride, n, PT_PROBE_GROUP_RAYS, scratch); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
