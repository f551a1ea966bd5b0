// gf_ppo.hip — the PPO update around the policy's GEMMs (rsl_rl PPO.update): the minibatch loss with its gradient w.r.t. the
// policy outputs, and clip_grad_norm_ + Adam with the adaptive learning rate over the flat gradient bucket.  include/gf_step.h has
// the contracts; neither entry point is a phase of the step.
//
// gf_ppo_loss: one lane per minibatch row walks its A columns in groups of four twice — log_prob and KL (left folds, as
// gf_policy_act), then, once the row's ratio is known, d loss / d mu and the row's share of d loss / d sigma.  16-byte loads and
// stores where A % 4 == 0 and every [mb, A] row is 16-byte aligned, scalar ones otherwise.  Each workgroup sums its rows' three
// loss terms and A sigma-gradient columns in double (wave butterfly, then the four waves in order through LDS) into its record
// of the workspace; a one-workgroup launch sums the records in a fixed order, one wave per column.  With sigma_is_log `sigma` is
// log_std: every loaded element goes through policy_sigma (gf_policy_row.h, gf_policy_act's expf) and the finalize launch writes
// d loss / d log_std = grad_sigma · sigma, one more f32 product.  Algorithmic traffic per row: R 16A + 20 (+ 8A
// re-read of mu / actions), W 4A + 4 bytes.  kl_rows > 0: rows past it add nothing to the KL sum and read row 0 of old_mu /
// old_sigma (which end at kl_rows); the finalize launch divides the KL sum by kl_rows.
//
// gf_adam_step: launch 1 — each workgroup sums g^2 of its 1 024-element chunks (double) into one partial; launch 2 — every
// workgroup sums all partials in the same order (so all agree on the norm without a hand-off), applies the schedule to
// state[parity], and updates its 1 024 elements.  Algorithmic traffic per element: R 4 (norm) + 16, W 16 bytes.
#include "gf_launch.h"
#include "gf_policy_row.h"
#include "gf_reduce.h"

namespace gf {

constexpr int kPpoBlock = GF_PPO_BLOCK_ROWS;
constexpr int kPpoFinBlock = 1024;
constexpr float kPpoLogSqrt2Pi = 0.918938533204672742f;   // (float)math.log(math.sqrt(2 * math.pi)), Normal.log_prob's constant
constexpr float kPpoEntropyC = 1.41893853320467274f;      // (float)(0.5 + 0.5 * math.log(2 * math.pi)), Normal.entropy's constant

template <bool V>
__device__ __forceinline__ void ppo_load4(const GF_GLOBAL float* p, int c0, int A, float (&v)[4]) {
    if (V) {
        const f32x4 x = *reinterpret_cast<const GF_GLOBAL f32x4*>(p + c0);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = c0 + k < A ? p[c0 + k] : 1.0f;   // (1: a finite filler no sum reads)
    }
}

// ---- gf_ppo_loss: rows ----------------------------------------------------------------------------------------------------------
template <bool V>
__global__ __launch_bounds__(kPpoBlock) void ppo_loss_rows_kernel(const GfPpoLossArgs a) {
    __shared__ double s_w[kPpoBlock / GF_WAVE];
    const int64_t mb = a.num_rows;
    const int64_t i = (int64_t)blockIdx.x * kPpoBlock + threadIdx.x;
    const bool in = i < mb;
    const int A = a.num_actions;
    const int64_t row = (in ? i : 0) * A;   // lanes past the end read row 0 and add nothing
    const int64_t nb = gridDim.x;
    GF_GLOBAL double* rec = G(reinterpret_cast<double*>(a.workspace)) + blockIdx.x;   // record q of this workgroup: rec[q * nb]
    const GF_GLOBAL float* mu = G(a.mu) + row;
    const GF_GLOBAL float* x = G(a.actions) + row;
    const bool in_kl = a.kl_rows == 0 || i < a.kl_rows;   // the KL covers the first kl_rows rows (0: all); old_mu / old_sigma end there
    const GF_GLOBAL float* omu = G(a.old_mu) + (in_kl ? row : 0);
    const GF_GLOBAL float* osd = G(a.old_sigma) + (in_kl ? row : 0);
    const GF_GLOBAL float* sd = G(a.sigma);
    // pass 1: log_prob and KL of the row
    float lp = 0.0f, kl = 0.0f;
    for (int c0 = 0; c0 < A; c0 += 4) {
        float m[4], xa[4], s[4], om[4], os[4];
        ppo_load4<V>(mu, c0, A, m);
        ppo_load4<V>(x, c0, A, xa);
        ppo_load4<V>(sd, c0, A, s);
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = policy_sigma(s[k], a.sigma_is_log);
        ppo_load4<V>(omu, c0, A, om);
        ppo_load4<V>(osd, c0, A, os);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (c0 + k >= A) continue;
            const float d = xa[k] - m[k];   // Normal.log_prob: -((x - loc) ** 2) / (2 * var) - log(scale) - log(sqrt(2π))
            const float var = s[k] * s[k];
            float t = -(d * d) / (2.0f * var);
            t = t - logf(s[k]);
            t = t - kPpoLogSqrt2Pi;
            lp = c0 + k == 0 ? t : lp + t;
            const float dm = om[k] - m[k];   // rsl_rl: log(sigma / old_sigma + 1e-5) + (old_sigma^2 + (old_mu - mu)^2) / (2 sigma^2) - 0.5
            const float u = (logf(s[k] / os[k] + 1.0e-5f) + (os[k] * os[k] + dm * dm) / (2.0f * var)) - 0.5f;
            kl = c0 + k == 0 ? u : kl + u;
        }
    }
    // the row's surrogate and value loss, and their gradients
    const float inv_mb = 1.0f / (float)mb;   // mean's backward: grad / numel
    const float eps = a.clip_param;
    const float adv = in ? G(a.advantages)[i] : 0.0f;
    const float ratio = expf(lp - (in ? G(a.old_log_prob)[i] : 0.0f));
    const float nadv = -adv;
    const float rc = fminf(fmaxf(ratio, 1.0f - eps), 1.0f + eps);
    const float s1 = nadv * ratio, s2 = nadv * rc;
    const float surr = fmaxf(s1, s2);
    const float g1 = s1 == s2 ? inv_mb * 0.5f : (s1 < s2 ? 0.0f : inv_mb);   // max's backward: half to each side on a tie
    const float g2 = s1 == s2 ? inv_mb * 0.5f : (s2 < s1 ? 0.0f : inv_mb);
    float dratio = g1 * nadv;
    if (ratio >= 1.0f - eps && ratio <= 1.0f + eps) dratio = dratio + g2 * nadv;   // clamp passes the gradient at its bounds
    const float dlp = in ? dratio * ratio : 0.0f;   // exp's backward
    const float v = in ? G(a.value)[i] : 0.0f;
    const float ret = in ? G(a.returns)[i] : 0.0f;
    const float gv = a.value_loss_coef / (float)mb;
    float vl, dv;
    if (a.use_clipped_value_loss) {
        const float tv = in ? G(a.target_values)[i] : 0.0f;
        const float dvt = v - tv;
        const float vc = tv + fminf(fmaxf(dvt, -eps), eps);
        const float e1 = v - ret, e2 = vc - ret;
        const float l1 = e1 * e1, l2 = e2 * e2;
        vl = fmaxf(l1, l2);
        const float h1 = l1 == l2 ? gv * 0.5f : (l1 < l2 ? 0.0f : gv);
        const float h2 = l1 == l2 ? gv * 0.5f : (l2 < l1 ? 0.0f : gv);
        dv = h1 * (2.0f * e1);
        if (dvt >= -eps && dvt <= eps) dv = dv + h2 * (2.0f * e2);
    } else {
        const float e = ret - v;
        vl = e * e;
        dv = -(gv * (2.0f * e));
    }
    if (in && a.grad_value) G(a.grad_value)[i] = dv;
    const double sums3[3] = {in ? (double)surr : 0.0, in ? (double)vl : 0.0, in && in_kl ? (double)kl : 0.0};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const double t = block_sum_all(sums3[q], s_w);
        if (threadIdx.x == 0) rec[q * nb] = t;
    }
    if (!a.grad_mu) return;   // (block-uniform)
    // pass 2: d loss / d mu of the row, the row's part of d loss / d sigma (summed over the workgroup)
    GF_GLOBAL float* gmu = G(a.grad_mu) + row;
    for (int c0 = 0; c0 < A; c0 += 4) {
        float m[4], xa[4], s[4], gm[4];
        double gs[4];
        ppo_load4<V>(mu, c0, A, m);
        ppo_load4<V>(x, c0, A, xa);
        ppo_load4<V>(sd, c0, A, s);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s[k] = policy_sigma(s[k], a.sigma_is_log);
            const float d = xa[k] - m[k];
            const float var = s[k] * s[k];
            gm[k] = (dlp / (2.0f * var)) * (2.0f * d);                  // d/d mu of -(d^2) / (2 var)
            gs[k] = (double)(dlp * ((d * d) / (var * s[k]) - 1.0f / s[k]));   // d/d sigma of -(d^2) / (2 sigma^2) - log(sigma)
        }
        if (in) {
            if (V) {
                *reinterpret_cast<GF_GLOBAL f32x4*>(gmu + c0) = f32x4{gm[0], gm[1], gm[2], gm[3]};
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c0 + k < A) gmu[c0 + k] = gm[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (c0 + k >= A) break;   // (uniform: A is a launch constant)
            const double t = block_sum_all(in ? gs[k] : 0.0, s_w);
            if (threadIdx.x == 0) rec[(3 + c0 + k) * nb] = t;
        }
    }
}

// ---- gf_ppo_loss: the records, in a fixed order ----------------------------------------------------------------------------------
// One wave per record column (16 at once): its lanes stride over the workgroups' records, then a butterfly — no barrier between
// the columns, every wave's loads in flight together.
__global__ __launch_bounds__(kPpoFinBlock) void ppo_loss_finalize_kernel(const GfPpoLossArgs a, const int64_t nb) {
    __shared__ double s_tot[3];
    const GF_GLOBAL double* ws = G(reinterpret_cast<const double*>(a.workspace));
    const int A = a.num_actions;
    const int want = a.grad_mu ? 3 + A : 3;
    const double mb = (double)a.num_rows;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (GF_WAVE - 1);
    for (int q = wave; q < want; q += kPpoFinBlock / GF_WAVE) {
        double acc = 0.0;
#pragma unroll 4
        for (int64_t b = lane; b < nb; b += GF_WAVE) acc += ws[q * nb + b];
        const double t = wave_xor_sum(acc);
        if (lane == 0) {
            if (q < 3) {
                s_tot[q] = t;
            } else {   // + the entropy term: sum over the rows of (-entropy_coef / mb) / sigma = -entropy_coef / sigma
                const float s = policy_sigma(G(a.sigma)[q - 3], a.sigma_is_log);
                const float g = (float)(t - (double)a.entropy_coef / (double)s);
                G(a.grad_sigma)[q - 3] = a.sigma_is_log ? g * s : g;   // exp's backward: d loss / d log_std = (d loss / d sigma) · sigma
            }
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float ent = 0.0f;   // every row's entropy is the same sum: its mean over the rows is that sum
    for (int c = 0; c < A; ++c) {
        const float e = kPpoEntropyC + logf(policy_sigma(G(a.sigma)[c], a.sigma_is_log));
        ent = c == 0 ? e : ent + e;
    }
    const double kl_n = a.kl_rows ? (double)a.kl_rows : mb;
    const float surrogate = (float)(s_tot[0] / mb), value_loss = (float)(s_tot[1] / mb), kl_mean = (float)(s_tot[2] / kl_n);
    const float loss = (surrogate + a.value_loss_coef * value_loss) - a.entropy_coef * ent;
    GF_GLOBAL float* out = G(a.out);
    out[0] = surrogate;
    out[1] = value_loss;
    out[2] = ent;
    out[3] = kl_mean;
    out[4] = loss;
    if (a.sums) {   // rsl_rl: mean_value_loss += value_loss.item(); mean_surrogate_loss += …; mean_entropy += … (Python floats)
        GF_GLOBAL double* sums = G(a.sums);
        sums[0] = sums[0] + (double)value_loss;
        sums[1] = sums[1] + (double)surrogate;
        sums[2] = sums[2] + (double)ent;
    }
}

// ---- gf_adam_step ---------------------------------------------------------------------------------------------------------------
constexpr int kAdamBlock = 256;
static_assert(kAdamBlock * 4 == GF_ADAM_BLOCK_ELEMS, "elements per workgroup and pass");
static_assert(kPpoBlock == kSumBlock && kAdamBlock == kSumBlock, "block_sum_all folds four waves");

template <bool V>
__device__ __forceinline__ void adam_load4(const GF_GLOBAL float* p, int64_t e, int64_t n, float (&v)[4]) {
    if (V) {
        const f32x4 x = *reinterpret_cast<const GF_GLOBAL f32x4*>(p + e);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = e + k < n ? p[e + k] : 0.0f;
    }
}

template <bool V>
__device__ __forceinline__ void adam_store4(float* p, int64_t e, int64_t n, const float (&v)[4]) {
    GF_GLOBAL float* q = G(p);
    if (V) {
        *reinterpret_cast<GF_GLOBAL f32x4*>(q + e) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e + k < n) q[e + k] = v[k];
    }
}

// workgroup b sums g^2 over chunks b, b + nb, … (1 024 elements each)
template <bool V>
__global__ __launch_bounds__(kAdamBlock) void adam_norm_kernel(const GfAdamArgs a) {
    __shared__ double s_w[kAdamBlock / GF_WAVE];
    const int64_t n = a.numel;
    const int64_t chunks = (n + GF_ADAM_BLOCK_ELEMS - 1) / GF_ADAM_BLOCK_ELEMS;
    double acc = 0.0;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t e = c * GF_ADAM_BLOCK_ELEMS + (int64_t)threadIdx.x * 4;
        if (e >= n) continue;
        float g[4];
        if (V && e + 4 <= n) adam_load4<true>(G(a.grads), e, n, g);
        else adam_load4<false>(G(a.grads), e, n, g);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += (double)g[k] * (double)g[k];
    }
    const double t = block_sum_all(acc, s_w);
    if (threadIdx.x == 0) G(reinterpret_cast<double*>(a.workspace))[blockIdx.x] = t;
}

template <bool V>
__global__ __launch_bounds__(kAdamBlock) void adam_update_kernel(const GfAdamArgs a, const int num_partials) {
    __shared__ double s_w[kAdamBlock / GF_WAVE];
    // the norm: every workgroup sums the same partials in the same order
    double acc = 0.0;
    for (int b = threadIdx.x; b < num_partials; b += kAdamBlock) acc += G(reinterpret_cast<const double*>(a.workspace))[b];
    const double sq = block_sum_all(acc, s_w);
    const float total_norm = (float)sqrt(sq);
    float coef = a.max_grad_norm / (total_norm + 1.0e-6f);   // clip_grad_norm_: max_norm / (total_norm + 1e-6), clamp(max=1)
    coef = coef > 1.0f ? 1.0f : coef;
    // the schedule (rsl_rl PPO.update), then the step's scalars (torch.optim.Adam, foreach, not capturable)
    const GF_GLOBAL GfAdamState* cur = G(a.state) + a.parity;
    double lr = cur->lr;
    const int64_t step = cur->step + 1;
    if (a.schedule == GF_ADAM_SCHEDULE_ADAPTIVE) {
        const float kl = *G(a.kl_mean);
        if (kl > (float)(a.desired_kl * 2.0)) {
            const double d = lr / 1.5;
            lr = d > 1.0e-5 ? d : 1.0e-5;           // max(1e-5, lr / 1.5)
        } else if (kl < (float)(a.desired_kl / 2.0) && kl > 0.0f) {
            const double u = lr * 1.5;
            lr = u < 1.0e-2 ? u : 1.0e-2;           // min(1e-2, lr * 1.5)
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        GF_GLOBAL GfAdamState* nx = G(a.state) + (1 - a.parity);
        nx->lr = lr;
        nx->step = step;
    }
    const double bc1 = 1.0 - pow(a.beta1, (double)step);
    const double bc2 = 1.0 - pow(a.beta2, (double)step);
    const float step_size = (float)((lr / bc1) * -1.0);
    const float bc2_sqrt = (float)sqrt(bc2);
    const float w1 = (float)(1.0 - a.beta1), b2 = (float)a.beta2, w2 = (float)(1.0 - a.beta2), eps = (float)a.eps;
    const int64_t n = a.numel;
    const int64_t e = (int64_t)blockIdx.x * GF_ADAM_BLOCK_ELEMS + (int64_t)threadIdx.x * 4;
    if (e >= n) return;
    float g[4], m[4], v[4], p[4];
    const bool vec = V && e + 4 <= n;
    if (vec) {
        adam_load4<true>(G(a.grads), e, n, g);
        adam_load4<true>(G(a.exp_avg), e, n, m);
        adam_load4<true>(G(a.exp_avg_sq), e, n, v);
        adam_load4<true>(G(a.params), e, n, p);
    } else {
        adam_load4<false>(G(a.grads), e, n, g);
        adam_load4<false>(G(a.exp_avg), e, n, m);
        adam_load4<false>(G(a.exp_avg_sq), e, n, v);
        adam_load4<false>(G(a.params), e, n, p);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        g[k] = g[k] * coef;                          // _foreach_mul_(grads, clip_coef_clamped)
        m[k] = m[k] + w1 * (g[k] - m[k]);            // _foreach_lerp_(exp_avgs, grads, 1 - beta1)
        v[k] = v[k] * b2;                            // _foreach_mul_(exp_avg_sqs, beta2)
        v[k] = v[k] + w2 * (g[k] * g[k]);            // _foreach_addcmul_(exp_avg_sqs, grads, grads, 1 - beta2)
        const float den = sqrtf(v[k]) / bc2_sqrt + eps;
        p[k] = p[k] + step_size * (m[k] / den);      // _foreach_addcdiv_(params, exp_avgs, denom, step_size)
    }
    if (vec) {
        adam_store4<true>(a.grads, e, n, g);
        adam_store4<true>(a.exp_avg, e, n, m);
        adam_store4<true>(a.exp_avg_sq, e, n, v);
        adam_store4<true>(a.params, e, n, p);
    } else {
        adam_store4<false>(a.grads, e, n, g);
        adam_store4<false>(a.exp_avg, e, n, m);
        adam_store4<false>(a.exp_avg_sq, e, n, v);
        adam_store4<false>(a.params, e, n, p);
    }
}

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_ppo_loss(const GfPpoLossArgs* a, void* stream) {
    if (!a || !a->mu || !a->sigma || !a->value || !a->actions || !a->old_log_prob || !a->advantages || !a->returns || !a->old_mu ||
        !a->old_sigma || !a->out || !a->workspace)
        return GF_E_NULL;
    if (a->use_clipped_value_loss && !a->target_values) return GF_E_NULL;
    const int grads = (a->grad_mu != nullptr) + (a->grad_value != nullptr) + (a->grad_sigma != nullptr);
    if (grads != 0 && grads != 3) return GF_E_NULL;   // half a gradient set
    if (a->num_rows < 0 || a->num_actions < 1 || (a->use_clipped_value_loss != 0 && a->use_clipped_value_loss != 1) ||
        (a->sigma_is_log != 0 && a->sigma_is_log != 1) || a->kl_rows < 0 || a->kl_rows > a->num_rows)
        return GF_E_RANGE;
    if (a->num_rows == 0) return GF_OK;
    const int64_t nb = (a->num_rows + gf::kPpoBlock - 1) / gf::kPpoBlock;
    if (nb > 0x7fffffff) return GF_E_RANGE;
    if (a->workspace_bytes < GF_PPO_LOSS_WORKSPACE_BYTES(a->num_rows, a->num_actions) || (reinterpret_cast<uintptr_t>(a->workspace) & 7u))
        return GF_E_RANGE;
    uintptr_t bits = 0;
    const void* rows[] = {a->mu, a->actions, a->old_mu, a->old_sigma, a->grad_mu, a->sigma};
    for (const void* p : rows) bits |= reinterpret_cast<uintptr_t>(p);
    const bool vec = (bits & 15u) == 0 && (a->num_actions & 3) == 0;
    hipStream_t s = (hipStream_t)stream;
    if (vec) gf::klaunch(gf::ppo_loss_rows_kernel<true>, dim3((unsigned)nb), dim3(gf::kPpoBlock), 0, s, *a);
    else gf::klaunch(gf::ppo_loss_rows_kernel<false>, dim3((unsigned)nb), dim3(gf::kPpoBlock), 0, s, *a);
    gf::klaunch(gf::ppo_loss_finalize_kernel, dim3(1), dim3(gf::kPpoFinBlock), 0, s, *a, nb);
    return gf::launch_status();
}

extern "C" __attribute__((visibility("default"))) int gf_adam_step(const GfAdamArgs* a, void* stream) {
    if (!a || !a->params || !a->grads || !a->exp_avg || !a->exp_avg_sq || !a->state || !a->workspace) return GF_E_NULL;
    if (a->schedule == GF_ADAM_SCHEDULE_ADAPTIVE && !a->kl_mean) return GF_E_NULL;
    if (a->schedule == GF_ADAM_SCHEDULE_FIXED && a->kl_mean) return GF_E_NULL;   // (a KL given to the fixed schedule: half a set)
    if (a->numel < 0 || (a->schedule != GF_ADAM_SCHEDULE_FIXED && a->schedule != GF_ADAM_SCHEDULE_ADAPTIVE) || (a->parity != 0 && a->parity != 1))
        return GF_E_RANGE;
    if (!(a->max_grad_norm > 0.0f) || (a->schedule == GF_ADAM_SCHEDULE_ADAPTIVE && !(a->desired_kl > 0.0))) return GF_E_RANGE;
    if (!(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0) || !(a->eps >= 0.0)) return GF_E_RANGE;
    if (a->numel == 0) return GF_OK;
    const int64_t chunks = (a->numel + GF_ADAM_BLOCK_ELEMS - 1) / GF_ADAM_BLOCK_ELEMS;
    if (chunks > 0x7fffffff) return GF_E_RANGE;
    if (a->workspace_bytes < GF_ADAM_WORKSPACE_BYTES(a->numel) || (reinterpret_cast<uintptr_t>(a->workspace) & 7u) ||
        (reinterpret_cast<uintptr_t>(a->state) & 7u))
        return GF_E_RANGE;
    const int partials = (int)(chunks < GF_ADAM_MAX_PARTIALS ? chunks : GF_ADAM_MAX_PARTIALS);
    uintptr_t bits = reinterpret_cast<uintptr_t>(a->params) | reinterpret_cast<uintptr_t>(a->grads) |
                     reinterpret_cast<uintptr_t>(a->exp_avg) | reinterpret_cast<uintptr_t>(a->exp_avg_sq);
    const bool vec = (bits & 15u) == 0;
    hipStream_t s = (hipStream_t)stream;
    if (vec) {
        gf::klaunch(gf::adam_norm_kernel<true>, dim3((unsigned)partials), dim3(gf::kAdamBlock), 0, s, *a);
        gf::klaunch(gf::adam_update_kernel<true>, dim3((unsigned)chunks), dim3(gf::kAdamBlock), 0, s, *a, partials);
    } else {
        gf::klaunch(gf::adam_norm_kernel<false>, dim3((unsigned)partials), dim3(gf::kAdamBlock), 0, s, *a);
        gf::klaunch(gf::adam_update_kernel<false>, dim3((unsigned)chunks), dim3(gf::kAdamBlock), 0, s, *a, partials);
    }
    return gf::launch_status();
}
