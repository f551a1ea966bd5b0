// gf_policy_row.h — one env row of gf_policy_act (include/gf_step.h has the contract): the draws, the sample, the log-probability fold
// and the policy's storage rows.  Shared by gf_policy.hip (mean read from memory) and gf_mlp.hip (mean left in LDS by the actor MLP of
// the same launch), so the two sample by the same code.
#pragma once

#include "gf_device.h"

namespace gf {

constexpr float kLogSqrt2Pi = 0.918938533204672742f;   // math.log(math.sqrt(2 * math.pi)) rounded to f32, as torch subtracts it

// Box–Muller on two Philox words: u1 in (0, 1] (log stays finite), u2 in [0, 1); sincospi takes the exact f32 argument 2·u2
__device__ __forceinline__ void box_muller(uint32_t w1, uint32_t w2, float& z0, float& z1) {
    const float u1 = (float)((w1 >> 8) + 1u) * 5.9604644775390625e-8f;
    const float u2 = (float)(w2 >> 8) * 5.9604644775390625e-8f;
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(2.0f * u2, &s, &c);
    z0 = r * c;
    z1 = r * s;
}

// The action std of a column from the policy's parameter: the parameter itself (rsl_rl's noise_std_type "scalar") or expf of it
// ("log").  gf_policy_act, gf_mlp_act and gf_ppo_loss all come through here, so one log_std gives the same sigma bits in all three.
// The two sampling kernels pass a compile-time flag (LOG, a kernel instance of its own): their flag-0 code is what it was.
__device__ __forceinline__ float policy_sigma(float raw, int is_log) { return is_log ? expf(raw) : raw; }

template <bool V>
__device__ __forceinline__ void act_load4(const GF_GLOBAL float* p, int c0, int A, float (&v)[4]) {
    if (V) {
        const f32x4 x = *reinterpret_cast<const GF_GLOBAL f32x4*>(p + c0);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = c0 + k < A ? p[c0 + k] : 1.0f;   // (1: a finite filler the fold never reads)
    }
}

template <bool V>
__device__ __forceinline__ void act_store4(float* p, int64_t off, int c0, int A, const float (&v)[4]) {
    if (!p) return;
    GF_GLOBAL float* q = G(p) + off;
    if (V) {
        *reinterpret_cast<GF_GLOBAL f32x4*>(q + c0) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c0 + k < A) q[c0 + k] = v[k];
    }
}

// Row n of gf_policy_act.  `load_mean(c0, m)` fills m[0 … 3] with the mean of columns c0 … c0 + 3 (any finite filler past A).
// LOG: a.std holds log_std (a.std_is_log, decided at the launch).
template <bool V, bool LOG, class MeanLoad>
__device__ __forceinline__ void policy_act_row(const GfPolicyActArgs& a, const int64_t n, MeanLoad load_mean) {
    const int A = a.num_actions;
    const int64_t row = n * A;
    const GF_GLOBAL float* sd = G(a.std) + (a.std_per_env ? row : 0);
    const GF_GLOBAL float* noise = a.noise ? G(a.noise) + row : nullptr;
    const uint64_t key = a.seed ^ GF_POLICY_SEED_TAG;
    const uint32_t genv = a.env_offset + (uint32_t)n;
    float lp = 0.0f;
    for (int c0 = 0; c0 < A; c0 += 4) {
        float m[4], s[4], e[4], act[4];
        load_mean(c0, m);
        act_load4<V>(sd, c0, A, s);
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = policy_sigma(s[k], LOG);
        if (noise) {
            act_load4<V>(noise, c0, A, e);
        } else {
            const U4 r = philox4x32_10(genv, (uint32_t)(c0 >> 2), (uint32_t)a.stream, (uint32_t)(a.stream >> 32), (uint32_t)key,
                                       (uint32_t)(key >> 32));
            box_muller(r.x, r.y, e[0], e[1]);
            box_muller(r.z, r.w, e[2], e[3]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            act[k] = m[k] + s[k] * e[k];   // torch.normal(mean, std): eps * std, then + mean
            if (c0 + k < A) {              // Normal.log_prob: -((x - loc) ** 2) / (2 * var) - log(scale) - log(sqrt(2π))
                const float d = act[k] - m[k];
                const float var = s[k] * s[k];
                float t = -(d * d) / (2.0f * var);
                t = t - logf(s[k]);
                t = t - kLogSqrt2Pi;
                lp = c0 + k == 0 ? t : lp + t;   // .sum(-1) as a left fold
            }
        }
        act_store4<V>(a.actions, row, c0, A, act);
        act_store4<V>(a.actions_out, row, c0, A, act);
        act_store4<V>(a.mu_out, row, c0, A, m);
        act_store4<V>(a.sigma_out, row, c0, A, s);
    }
    if (a.values_out) G(a.values_out)[n] = G(a.values)[n];
    if (a.log_prob_out) G(a.log_prob_out)[n] = lp;
}

}  // namespace gf
