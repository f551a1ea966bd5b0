// gf_action_row.h — the action phase per float4 of the flat [N·D] action stream (D % 4 == 0: a float4 holds four consecutive DOFs of
// one env), and the statistics ring's upkeep.  Shared by gf_action.hip (action_kernel<true, true>) and gf_scene.hip (the tile tick
// with the action phase folded in, where the targets go from registers into the joints), so the two run the same statements in the
// same order and give the same bits.
#pragma once

#include "gf_device.h"

namespace gf {

__device__ __forceinline__ float action_target(float x, float s, float o, float lo, float hi, int mode) {
    if (mode == GF_ACTION_WITHIN_LIMITS) {
        x = clamp_min(x, -1.0f);
        x = clamp_max(x, 1.0f);
        return x * s + o;
    }
    float t = x * s + o;
    t = clamp_min(t, lo);
    t = clamp_max(t, hi);
    return t;
}

// `upkeep` leading workgroups do nothing but the statistics ring's housekeeping: zero the NEXT step's slot and fold the PREVIOUS
// step's shards into its vector row.  The fold is a chain of two scattered loads and a dozen cross-lane shuffles per entry (≈ 2.5 µs):
// inside the workgroups that also move actions it was those waves' tail, and with it the kernel's (5.8 µs in the benchmark loop at
// 65 536 envs).  On workgroups of their own it runs beside the main work.  `upkeep` is a multiple of 8, so workgroup b + upkeep still
// lands on the XCD workgroup b of the scene / post-physics kernels lands on (round-robin placement, see gf_action_step).
constexpr int kActionUpkeepBlocks = 24;

inline int action_upkeep_blocks(const GfActionArgs* a) { return (a->stats_zero || (a->stats_fold_src && a->stats_fold_dst)) ? kActionUpkeepBlocks : 0; }

// the body of an upkeep workgroup (blockIdx.x < upkeep); any workgroup size that is a multiple of the wave (`block`: a kernel that
// knows its size at compile time says so, and needs no implicit kernel argument for it)
__device__ __forceinline__ void action_upkeep(const GfActionArgs& a, const int upkeep, const unsigned block = blockDim.x) {
    const int t = (int)(blockIdx.x * block + threadIdx.x), nt = (int)(upkeep * block);
    if (a.stats_zero) {   // nobody else touches the next slot during this step
        constexpr int kWords = (int)(sizeof(GfStepStats) * GF_STATS_SHARDS / 4);
        for (int w = t; w < kWords; w += nt) reinterpret_cast<uint32_t*>(a.stats_zero)[w] = 0u;
    }
    if (a.stats_fold_src && a.stats_fold_dst) {   // the previous slot is complete by stream order: one entry per wave
        for (int v = t / GF_WAVE; v < GF_STATS_VECTOR_LEN; v += nt / GF_WAVE) fold_stats_entry(a.stats_fold_src, a.stats_fold_dst, a.stats_last_reset, v);
    }
}

// The constants of a float4 whose first element is DOF d0 (D % 4 == 0: the lane's four elements are four consecutive DOFs that never
// wrap — one 16-byte load per constant array, L1 / K$ resident, instead of sixteen scalar gathers).  No branch around the loads, so a
// caller can issue them beside its other loads: without clip arrays (within-limits mode) the scale is read in their place and dropped.
struct ActionConsts4 {
    float4 sc, of, lo, hi;
};
__device__ __forceinline__ ActionConsts4 action_consts4(const GfActionArgs& a, const int d0, const int mode) {
    const bool clip = mode == GF_ACTION_POSITION;
    ActionConsts4 c;
    c.sc = *reinterpret_cast<const float4*>(a.scale + d0);
    c.of = *reinterpret_cast<const float4*>(a.offset + d0);
    const float4 lo4 = *reinterpret_cast<const float4*>((clip ? a.clip_lo : a.scale) + d0);
    const float4 hi4 = *reinterpret_cast<const float4*>((clip ? a.clip_hi : a.scale) + d0);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    c.lo = clip ? lo4 : zero;
    c.hi = clip ? hi4 : zero;
    return c;
}

// One float4 of the stream: raw policy output x and the env's previous actions prev in, what the step leaves in env_last_actions,
// env_actions and targets out (the caller loads prev and stores last / actions only when the bookkeeping buffers are there), and
// the NaN (bit 0) / Inf (bit 1) bits OR-ed into flags.
__device__ __forceinline__ void action_row4(const GfActionArgs& a, const ActionConsts4& c, const int mode, const float4 x, const float4 prev,
                                            float4& last, float4& actions, float4& targets, int& flags) {
    last = prev;
    actions = x;
    const float xs[4] = {x.x, x.y, x.z, x.w};
    float ts[4];
    const float ss[4] = {c.sc.x, c.sc.y, c.sc.z, c.sc.w}, os[4] = {c.of.x, c.of.y, c.of.z, c.of.w};
    const float ls[4] = {c.lo.x, c.lo.y, c.lo.z, c.lo.w}, hs[4] = {c.hi.x, c.hi.y, c.hi.z, c.hi.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        ts[j] = action_target(xs[j], ss[j], os[j], ls[j], hs[j], mode);
        if (a.check_finite && mode == GF_ACTION_POSITION) {
            flags |= isnan(xs[j]) ? 1 : 0;
            flags |= isinf(xs[j]) ? 2 : 0;
        }
    }
    targets = make_float4(ts[0], ts[1], ts[2], ts[3]);
}

// NaN/Inf detection (position_action_manager.py:402-406): the reference syncs twice per step to print; here a flag word is OR-ed
// on device and polled lazily by the host.  Whole waves call this (ballot).
__device__ __forceinline__ void action_flags_commit(const GfActionArgs& a, const int flags) {
    if (a.stats && a.check_finite) {
        const unsigned long long nan_m = __ballot(flags & 1);
        const unsigned long long inf_m = __ballot(flags & 2);
        if ((nan_m | inf_m) && (threadIdx.x & (GF_WAVE - 1)) == 0) atomicOr(&stats_shard(a.stats)->action_flags, (nan_m ? 1 : 0) | (inf_m ? 2 : 0));
    }
}

}  // namespace gf
