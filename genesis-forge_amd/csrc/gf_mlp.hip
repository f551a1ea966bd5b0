// gf_mlp.hip — gf_mlp_act (and gf_mlp_distill_act, gf_rnd_reward, gf_mlp_recurrent_act): the actor and critic MLPs of a collection step and gf_policy_act's sampling in one launch
// (include/gf_step.h has the contract).  The first kernel of the library on the matrix cores: every other one is bandwidth- or
// latency-bound, this one is 0.76 MFLOP per env.
//
// A workgroup of four waves owns kMlpRows = 32 rows of ONE net (blockIdx.y) and walks its layers.  Per layer y = x · Wᵀ + b runs on
// v_mfma_f32_32x32x2_f32: A operand = the tile's activations (lane l holds x[l & 31][k + (l >> 5)]), B operand = Wᵀ (lane l holds
// W[j0 + (l & 31)][k + (l >> 5)]), D = 32 rows x 32 output columns with the column on the lane.  Wave w owns the 32-column blocks
// w, w + 4, w + 8, w + 12 of the layer — up to four independent accumulators, each started from the bias — and issues the k steps in
// ascending order, so an output element is one k-ascending fma chain.
//   * Activations stay in LDS (x: 32 rows x 513 floats; the odd stride keeps the 32 rows of a k column on 32 banks).  A layer reads
//     x through its whole k loop into registers (the accumulators), the workgroup meets, and the ELU-ed outputs overwrite x: one
//     buffer, never written to memory.  The first layer's input is copied from the segments into x, 512 columns at a time (the
//     accumulators live through the passes) — through the net's input normaliser where it has one: (v - mean[k]) / (std[k] + eps)
//     per real element, k the column of the whole input; the zero padding stays zero.
//   * Weights never touch LDS: a lane reads its own row of W along k — torch's layout is contiguous there — 16 bytes at a time, a
//     whole chunk of k (32 … 128 columns, 64 registers per wave) ahead of its multiplications; where a wave has one or two output
//     blocks a second chunk is in flight meanwhile.  The two lane halves of a wave read the two halves of a chunk, so a register
//     holds column k in lanes 0–31 and column k + chunk / 2 in lanes 32–63; the MFMA wants k and k + 1 there: one v_permlane32_swap
//     per register pair turns (k | k + c/2), (k + 1 | k + 1 + c/2) into (k | k + 1), (k + c/2 | k + 1 + c/2).  No barrier inside a
//     layer: the waves only meet where x changes.  Rows whose start is not 16-byte aligned (in % 4 != 0) load by element.
//   * Tails — rows past num_envs, k past `in`, output columns past `out` — are zeros (in x, or selected into the weight registers of
//     the last chunk), never a branch around an MFMA.
//   * The last layer's outputs land in x like any other; lane r < 32 of the workgroup then finishes row r: the actor workgroup stores
//     `mean` and runs gf_policy_act's row (gf_policy_row.h) with the mean read from LDS, the critic workgroup stores the value.
// LDS: 65 664 B, registers <= 256: two workgroups per CU, so one's barriers, ELU and load latency hide behind the other's MFMAs.
// gf_mlp_distill_act is the same tile walk with grid y = student / teacher (a distillation collection step): the student workgroup is
// the actor path above, the teacher workgroup stores its outputs to two destinations and samples nothing.
// gf_mlp_recurrent_act puts an LSTM / GRU cell between a net's input and its MLP (rnn_cell below): a second LDS buffer, one workgroup per CU.
// gf_mlp_recurrent_distill_act (gf_mlp_rdistill.hip, which compiles this file's device functions with GF_BODIES_ONLY) is that walk on
// gf_mlp_distill_act's grid, with its finish.
#include <initializer_list>

#include "gf_launch.h"
#include "gf_policy_row.h"
#include "gf_reduce.h"

namespace gf {

constexpr int kMlpBlock = 256;
constexpr int kMlpWaves = kMlpBlock / GF_WAVE;
constexpr int kMlpRows = GF_MLP_TILE_ROWS;
constexpr int kMlpXS = GF_MLP_MAX_HIDDEN + 1;   // row stride of the activations
constexpr int kMlpMaxNB = GF_MLP_MAX_HIDDEN / 32 / kMlpWaves;   // 32-column blocks per wave at most
// k columns per chunk for NB 32-column blocks per wave: a lane holds chunk / 2 of them per block — 64 registers (48 for NB = 3) — and a
// chunk is 4 096 MFMA cycles per wave, which is what the next chunk's loads hide behind.  At least 32: a lane then reads 64 contiguous
// bytes and a wave-instruction pair whole 128-byte lines.
constexpr int mlp_kc(int nb) { return nb == 1 ? 128 : nb == 2 ? 64 : 32; }
static_assert(kMlpRows == 32 && kMlpMaxNB == 4, "tile shape");
static_assert(GF_MLP_MAX_ACTIONS <= GF_MLP_MAX_HIDDEN, "the last layer's outputs are kept like a hidden layer's");

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct MlpSmem {
    float x[kMlpRows * kMlpXS];
};

// This lane's weights of a chunk: for block b, row j_b (rowoff = j_b · K), columns kl + (0 … KC / 2 - 1), kl = the chunk's first column
// + lh · KC / 2.  FULL: the chunk lies inside `in`; otherwise an element past it loads the row's first and is zeroed (with VEC, K % 4
// == 0, a quad is inside or outside as a whole).  Straight-line either way.  Rows past `out` read row 0: their columns are never stored.
template <int NB, bool VEC, bool FULL>
__device__ __forceinline__ void mlp_load_w(const GF_GLOBAL float* W, const uint32_t (&rowoff)[NB], int K, int kl, float (&r)[NB][mlp_kc(NB) / 2]) {
    constexpr int H = mlp_kc(NB) / 2;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (VEC) {
#pragma unroll
            for (int e = 0; e < H; e += 4) {
                const bool in = FULL || kl + e < K;
                const f32x4 v = *reinterpret_cast<const GF_GLOBAL f32x4*>(W + (rowoff[b] + (uint32_t)(in ? kl + e : 0)));
                r[b][e] = in ? v.x : 0.0f; r[b][e + 1] = in ? v.y : 0.0f; r[b][e + 2] = in ? v.z : 0.0f; r[b][e + 3] = in ? v.w : 0.0f;
            }
        } else {
#pragma unroll
            for (int e = 0; e < H; ++e) {
                const bool in = FULL || kl + e < K;
                const float v = W[rowoff[b] + (uint32_t)(in ? kl + e : 0)];
                r[b][e] = in ? v : 0.0f;
            }
        }
    }
}

template <int NB, bool VEC>
__device__ __forceinline__ void mlp_load_chunk(const GF_GLOBAL float* W, const uint32_t (&rowoff)[NB], int K, int k, int lh, float (&r)[NB][mlp_kc(NB) / 2]) {
    constexpr int KC = mlp_kc(NB);
    if (k + KC <= K) mlp_load_w<NB, VEC, true>(W, rowoff, K, k + lh * (KC / 2), r);
    else mlp_load_w<NB, VEC, false>(W, rowoff, K, k + lh * (KC / 2), r);
}

// the chunk's MFMAs: after the swap register 2m holds columns (2m | 2m + 1) of the chunk's first half, register 2m + 1 those of the second
template <int NB>
__device__ __forceinline__ void mlp_multiply(const float* ap, float (&r)[NB][mlp_kc(NB) / 2], f32x16 (&acc)[NB]) {
    constexpr int H = mlp_kc(NB) / 2;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int m = 0; m < H; m += 2) {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(r[b][m]), __float_as_uint(r[b][m + 1]), false, false);
            r[b][m] = __uint_as_float(sw[0]);
            r[b][m + 1] = __uint_as_float(sw[1]);
        }
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int m = 0; m < H; m += 2) {
            const float av = ap[half * H + m];   // x[li][k0 + half · H + m + lh]
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, r[b][m + half], acc[b], 0, 0, 0);
        }
    }
}

// columns [k0, k1) of the layer's k loop, x (an activation buffer of row stride kMlpXS) holding column k at x[row][k - xk0]
template <int NB, bool VEC>
__device__ __forceinline__ void mlp_k_loop(const float* x, const GF_GLOBAL float* W, const uint32_t (&rowoff)[NB], int K, int k0, int k1, int xk0, int li, int lh,
                                           f32x16 (&acc)[NB]) {
    constexpr int KC = mlp_kc(NB), H = KC / 2;
    const float* ap = x + li * kMlpXS + lh - xk0;
    if constexpr (NB <= 2) {   // registers for two chunks: the one being multiplied and the one in flight, by turns
        float ra[NB][H], rb[NB][H];
        int k = k0;
        mlp_load_chunk<NB, VEC>(W, rowoff, K, k, lh, ra);
        for (;;) {
            if (k + KC < k1) mlp_load_chunk<NB, VEC>(W, rowoff, K, k + KC, lh, rb);
            mlp_multiply<NB>(ap + k, ra, acc);
            k += KC;
            if (k >= k1) break;
            if (k + KC < k1) mlp_load_chunk<NB, VEC>(W, rowoff, K, k + KC, lh, ra);
            mlp_multiply<NB>(ap + k, rb, acc);
            k += KC;
            if (k >= k1) break;
        }
    } else {   // one chunk (three or four accumulator tiles leave no room for two under 256 registers): its loads are issued as soon
               // as the last MFMA of the previous chunk has read them, and the other workgroup of the CU multiplies meanwhile
        float r[NB][H];
        for (int k = k0; k < k1; k += KC) {
            mlp_load_chunk<NB, VEC>(W, rowoff, K, k, lh, r);
            mlp_multiply<NB>(ap + k, r, acc);
        }
    }
}

// Columns [p0, p0 + cols) of the net's input from its segments into x[row][0 …], through the normaliser where `norm`: zeros past
// num_envs and from `cols` up to `padded`.  The callers meet before and after.
template <bool NORM>
__device__ __forceinline__ void mlp_stage_input(MlpSmem& sm, const GfMlpNet& net, const bool norm, const int p0, const int cols, const int padded,
                                                const int64_t row0, const int64_t N) {
    for (int e = (int)threadIdx.x; e < kMlpRows * padded; e += kMlpBlock) {
        const int row = e / padded, col = e - row * padded;
        const int64_t n = row0 + row;
        int k = p0 + col;
        const bool in = n < N && col < cols;
        const float* rows = net.inputs[0].rows;
        int64_t off = 0;
#pragma unroll
        for (int s = 0; s < GF_MLP_MAX_INPUTS; ++s) {
            const int w = s < net.num_inputs ? net.inputs[s].width : 0;
            const bool hit = in && k >= 0 && k < w;
            rows = hit ? net.inputs[s].rows : rows;
            const int stride = net.inputs[s].row_stride ? net.inputs[s].row_stride : w;
            off = hit ? n * stride + k : off;
            k -= w;
        }
        float v = G(rows)[off];
        if (NORM && norm) {   // rsl_rl EmpiricalNormalization.forward: one subtraction, one addition, one correctly rounded division
            const int c = in ? p0 + col : 0;
            v = (v - G(net.in_mean)[c]) / (G(net.in_std)[c] + net.in_eps);
        }
        sm.x[row * kMlpXS + col] = in ? v : 0.0f;
    }
}

// One Linear layer (+ ELU unless `last`) of the tile: x (LDS, K columns; the segments when `first`) -> x (O columns, zeros up to the
// next multiple of 32).  NB = 32-column blocks per wave: every wave multiplies NB blocks (the ones past `out` are not stored).
// NORM: the launch has a net with an input normaliser (a kernel of its own: the plain forward keeps the code it had).
// (LOG, the kernel's other flag — std holds log_std — is the same kind: only the sampling lanes at the end differ.)
template <int NB, bool NORM>
__device__ __forceinline__ void mlp_layer(MlpSmem& sm, const GfMlpNet& net, const GfMlpLayer& L, const int K, const bool first, const bool last,
                                          const int64_t row0, const int64_t N) {
    constexpr int KC = mlp_kc(NB);
    const int O = L.out_width;
    const int CB = (O + 31) >> 5;
    const bool vec = (K & 3) == 0 && (reinterpret_cast<uintptr_t>(L.weight) & 15u) == 0;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63, li = lane & 31, lh = lane >> 5;

    const bool norm = NORM && first && net.in_mean != nullptr;   // (workgroup-uniform)

    f32x16 acc[NB];
    const GF_GLOBAL float* W = G(L.weight);
    uint32_t rowoff[NB];   // (out · in <= 512 · 1 024: 32 bits)
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int j = (wave + kMlpWaves * b) * 32 + li;
        rowoff[b] = (uint32_t)(j < O ? j : 0) * (uint32_t)K;
        const float bv = G(L.bias)[j < O ? j : 0];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = j < O ? bv : 0.0f;   // (the column is on the lane: all 16 rows of it start from bias[j])
    }

    // the k loop, GF_MLP_MAX_HIDDEN columns of x at a time (a multiple of every chunk length; only a first layer has more)
    for (int p0 = 0; p0 < K; p0 += GF_MLP_MAX_HIDDEN) {
        const int cols = K - p0 < GF_MLP_MAX_HIDDEN ? K - p0 : GF_MLP_MAX_HIDDEN;
        if (first) {   // the input from its segments: zeros past num_envs and past K up to the chunk's end
            if (p0) __syncthreads();   // (the previous pass is multiplied)
            mlp_stage_input<NORM>(sm, net, norm, p0, cols, (cols + KC - 1) / KC * KC, row0, N);
            __syncthreads();
        }
        if (vec) mlp_k_loop<NB, true>(sm.x, W, rowoff, K, p0, p0 + cols, p0, li, lh, acc);
        else mlp_k_loop<NB, false>(sm.x, W, rowoff, K, p0, p0 + cols, p0, li, lh, acc);
    }
    __syncthreads();   // every wave is done reading x

    // out columns, then zeros up to the longest chunk the next layer may read to (its k tail multiplies them by zero weights)
    const int padded = (O + 127) / 128 * 128 < GF_MLP_MAX_HIDDEN ? (O + 127) / 128 * 128 : GF_MLP_MAX_HIDDEN;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int cb = wave + kMlpWaves * b;
        if (cb >= CB) continue;   // (wave-uniform)
        const bool real = cb * 32 + li < O;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
            float v = acc[b][r];
            if (!last) v = v > 0.0f ? v : expm1f(v);
            sm.x[row * kMlpXS + cb * 32 + li] = real ? v : 0.0f;
        }
    }
    for (int e = (int)threadIdx.x; e < kMlpRows * (padded - CB * 32); e += kMlpBlock) {
        const int w = padded - CB * 32, row = e / w;
        sm.x[row * kMlpXS + CB * 32 + (e - row * w)] = 0.0f;
    }
    __syncthreads();
}

// every layer of `net` on the tile's rows: the last layer's outputs are left in x; returns their width
template <bool NORM>
__device__ __forceinline__ int mlp_forward(MlpSmem& sm, const GfMlpNet& net, const int64_t row0, const int64_t N) {
    int K = 0;
    for (int s = 0; s < net.num_inputs; ++s) K += net.inputs[s].width;
    const int layers = net.num_layers;
    for (int l = 0; l < layers; ++l) {
        const GfMlpLayer& L = net.layers[l];
        const int nb = (((L.out_width + 31) >> 5) + kMlpWaves - 1) / kMlpWaves;
        const bool first = l == 0, last = l == layers - 1;
        if (nb == 1) mlp_layer<1, NORM>(sm, net, L, K, first, last, row0, N);
        else if (nb == 2) mlp_layer<2, NORM>(sm, net, L, K, first, last, row0, N);
        else if (nb == 3) mlp_layer<3, NORM>(sm, net, L, K, first, last, row0, N);
        else mlp_layer<4, NORM>(sm, net, L, K, first, last, row0, N);
        K = L.out_width;
    }
    return K;
}

// gf_policy_act's row n (gf_policy_row.h) with the mean read from the row's outputs in x: the sampling tail of both kernels, each of
// which fills `p` its own way
template <bool LOG>
__device__ __forceinline__ void mlp_sample_row(const GfPolicyActArgs& p, const float* out, const int64_t n, const int vec_rows) {
    const auto load_mean = [&](int c0, float (&m)[4]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = out[c0 + k];   // (columns past A: zeros, or x's finite leftovers — never folded or stored)
    };
    if (vec_rows) policy_act_row<true, LOG>(p, n, load_mean);
    else policy_act_row<false, LOG>(p, n, load_mean);
}

// one lane per row finishes it from the outputs in x (K of them): the critic's value, or the actor's mean and gf_policy_act's row
template <bool LOG>
__device__ __forceinline__ void mlp_act_finish(const GfMlpActArgs& a, const MlpSmem& sm, const bool is_critic, const int K, const int64_t row0,
                                               const int vec_rows) {
    const int64_t N = a.num_envs;
    const int r = (int)threadIdx.x;
    const int64_t n = row0 + r;
    if (r >= kMlpRows || n >= N) return;
    const float* out = sm.x + r * kMlpXS;
    if (is_critic) {
        const float v = out[0];
        if (a.values) G(a.values)[n] = v;
        if (a.values_out) G(a.values_out)[n] = v;
        return;
    }
    const int A = K;
    if (a.mean) {
        GF_GLOBAL float* m = G(a.mean) + n * A;
        for (int c = 0; c < A; ++c) m[c] = out[c];
    }
    if (!a.actions) return;
    GfPolicyActArgs p;
    p.num_envs = N;
    p.num_actions = A;
    p.std_per_env = a.std_per_env;
    p.mean = nullptr;
    p.std = a.std;
    p.values = nullptr;
    p.noise = a.noise;
    p.seed = a.seed;
    p.stream = a.stream;
    p.env_offset = a.env_offset;
    p.std_is_log = LOG;
    p.actions = a.actions;
    p.actions_out = a.actions_out;
    p.mu_out = a.mu_out;
    p.sigma_out = a.sigma_out;
    p.values_out = nullptr;   // (the critic workgroup's)
    p.log_prob_out = a.log_prob_out;
    mlp_sample_row<LOG>(p, out, n, vec_rows);
}

template <bool NORM, bool LOG>
__global__ __launch_bounds__(kMlpBlock, 2) void mlp_act_kernel(const GfMlpActArgs a, const int first_net, const int vec_rows) {
    __shared__ MlpSmem sm;
    const bool is_critic = (int)blockIdx.y + first_net == 1;
    const GfMlpNet& net = is_critic ? a.critic : a.actor;
    const int64_t row0 = (int64_t)blockIdx.x * kMlpRows;

    const int K = mlp_forward<NORM>(sm, net, row0, a.num_envs);
    mlp_act_finish<LOG>(a, sm, is_critic, K, row0, vec_rows);
}

// gf_mlp_distill_act: grid y = 0 the student (gf_mlp_act's actor path: mean, sample, the storage row), y = 1 the teacher (its output
// to two destinations).  LOG is a run-time, workgroup-uniform choice here — only the sampling lanes at the end differ, and two
// instances (NORM) are what the launch needs.
// one lane per row finishes it from the outputs in x (A of them): the teacher's output to its two destinations, or the student's mean
// and gf_policy_act's row (gf_mlp_recurrent_distill_act's finish too: gf_mlp_rdistill.hip)
__device__ __forceinline__ void mlp_distill_finish(const GfMlpDistillArgs& a, const MlpSmem& sm, const bool is_teacher, const int A, const int64_t row0,
                                                   const int vec_rows) {
    const int64_t N = a.num_envs;
    const int r = (int)threadIdx.x;
    const int64_t n = row0 + r;
    if (r >= kMlpRows || n >= N) return;
    const float* out = sm.x + r * kMlpXS;
    if (is_teacher) {
        GF_GLOBAL float* t0 = G(a.teacher_actions) + n * A;
        GF_GLOBAL float* t1 = a.teacher_actions_out ? G(a.teacher_actions_out) + n * A : nullptr;
        for (int c = 0; c < A; ++c) {
            const float v = out[c];
            t0[c] = v;
            if (t1) t1[c] = v;
        }
        return;
    }
    if (a.mean) {
        GF_GLOBAL float* m = G(a.mean) + n * A;
        for (int c = 0; c < A; ++c) m[c] = out[c];
    }
    GfPolicyActArgs p;
    p.num_envs = N;
    p.num_actions = A;
    p.std_per_env = 0;
    p.mean = nullptr;
    p.std = a.std;
    p.values = nullptr;
    p.noise = a.noise;
    p.seed = a.seed;
    p.stream = a.stream;
    p.env_offset = a.env_offset;
    p.std_is_log = (uint32_t)a.std_is_log;
    p.actions = a.actions;
    p.actions_out = a.actions_out;
    p.mu_out = nullptr;
    p.sigma_out = nullptr;
    p.values_out = nullptr;
    p.log_prob_out = nullptr;
    if (a.std_is_log) mlp_sample_row<true>(p, out, n, vec_rows);
    else mlp_sample_row<false>(p, out, n, vec_rows);
}

template <bool NORM>
__global__ __launch_bounds__(kMlpBlock, 2) void mlp_distill_kernel(const GfMlpDistillArgs a, const int vec_rows) {
    __shared__ MlpSmem sm;
    const bool is_teacher = blockIdx.y == 1;
    const GfMlpNet& net = is_teacher ? a.teacher : a.student;
    const int64_t row0 = (int64_t)blockIdx.x * kMlpRows;

    const int A = mlp_forward<NORM>(sm, net, row0, a.num_envs);
    mlp_distill_finish(a, sm, is_teacher, A, row0, vec_rows);
}

// gf_rnd_reward (rsl_rl RandomNetworkDistillation.get_intrinsic_reward): ONE workgroup walks the frozen target, stashes the tile's
// E <= GF_MLP_MAX_ACTIONS outputs in a second LDS array, walks the predictor from the re-staged input, and lane r < 32 finishes row
// r: ‖target − predictor‖₂, the weight, the storage row's add.  Chosen over grid y = net (gf_mlp_distill_act's shape) because the
// distance needs both embeddings of a row in one place: this way they never leave LDS and no second launch has to wait for them.
// LDS: 65 664 + 8 320 = 73 984 B, still two workgroups per CU.  With the reward normaliser updating, this launch leaves the raw
// distances in `intrinsic`, the new `avg` and one {rows, mean, M2} record of the tile's avg in the workspace, and a snapshot of the
// old statistics (workgroup 0); rnd_scale_kernel then folds the records — every workgroup the same fold, in index order — applies the
// update, scales its rows and adds.  The workgroup that stores the new statistics is the only one that touches them in that launch.
constexpr int kRndES = GF_MLP_MAX_ACTIONS + 1;   // row stride of the stashed embeddings (odd: 32 rows on 32 banks)
constexpr int kRndHead = 4;                      // doubles in front of the records: old mean, var, std, count (as int64)
static_assert(kSumBlock == kMlpBlock, "the scale launch folds with gf_reduce.h's four-wave sums");

// the row's end: i = v · weight -> intrinsic, rewards += i, the two per-env accumulators
__device__ __forceinline__ void rnd_finish_row(const GfRndRewardArgs& a, const int64_t n, const float v) {
    const float i = v * a.weight;
    G(a.intrinsic)[n] = i;
    if (a.rewards) {
        const float rw = G(a.rewards)[n];
        if (a.acc_extrinsic) G(a.acc_extrinsic)[n] = G(a.acc_extrinsic)[n] + (double)rw;
        G(a.rewards)[n] = rw + i;
    }
    if (a.acc_intrinsic) G(a.acc_intrinsic)[n] = G(a.acc_intrinsic)[n] + (double)i;
}

#ifndef GF_BODIES_ONLY
// (one instance, mlp_forward<true>: whether a net has a normaliser is its workgroup-uniform run-time test there; an instance
// without it came out at 256 VGPRs with 64 B of scratch once the two walks and the row's end shared a kernel, this one at 249)
__global__ __launch_bounds__(kMlpBlock, 2) void rnd_tile_kernel(const GfRndRewardArgs a, const int two_pass) {
    constexpr bool NORM = true;
    __shared__ MlpSmem sm;
    __shared__ float s_emb[kMlpRows * kRndES];
    const int64_t N = a.num_envs;
    const int64_t row0 = (int64_t)blockIdx.x * kMlpRows;

    const int E = mlp_forward<NORM>(sm, a.target, row0, N);
    for (int e = (int)threadIdx.x; e < kMlpRows * E; e += kMlpBlock) {
        const int row = e / E, c = e - row * E;
        s_emb[row * kRndES + c] = sm.x[row * kMlpXS + c];
    }
    __syncthreads();   // (the predictor's first layer stages its input over x)
    mlp_forward<NORM>(sm, a.predictor, row0, N);

    if (threadIdx.x >= GF_WAVE) return;   // wave 0 finishes the tile: lane r < 32 owns row r
    const int lane = (int)threadIdx.x;
    const int64_t n = row0 + lane;
    const bool live = lane < kMlpRows && n < N;
    float r = 0.0f;
    if (live) {
        const float* t = s_emb + lane * kRndES;
        const float* p = sm.x + lane * kMlpXS;
        double s = 0.0;
        for (int j = 0; j < E; ++j) {
            const float d = t[j] - p[j];
            s += (double)d * (double)d;
        }
        r = (float)sqrt(s);
    }
    if (!two_pass) {
        if (!live) return;
        float v = r;
        if (a.normalize) {   // (no update in this call: nobody writes the statistics)
            const float sd = G(a.std)[0];
            v = sd > 0.0f ? r / sd : r;
        }
        rnd_finish_row(a, n, v);
        return;
    }
    float av = 0.0f;
    if (live) {
        av = a.first ? r : __fadd_rn(__fmul_rn(G(a.avg)[n], a.gamma), r);   // rsl_rl: avg * gamma + rew, two roundings
        G(a.avg)[n] = av;
        G(a.intrinsic)[n] = r;   // (raw: the scale launch reads it back)
    }
    const int64_t left = N - row0;
    const double cnt = (double)(left < kMlpRows ? left : kMlpRows);
    const double mean = wave_xor_sum(live ? (double)av : 0.0) / cnt;
    const double dv = live ? (double)av - mean : 0.0;
    const double m2 = wave_xor_sum(dv * dv);
    if (lane != 0) return;
    GF_GLOBAL double* ws = G(reinterpret_cast<double*>(a.workspace));
    GF_GLOBAL double* rec = ws + kRndHead + 3 * (int64_t)blockIdx.x;
    rec[0] = cnt;
    rec[1] = mean;
    rec[2] = m2;
    if (blockIdx.x == 0) {   // the statistics as they were: the scale launch reads these, never the live ones
        ws[0] = (double)G(a.mean)[0];
        ws[1] = (double)G(a.var)[0];
        ws[2] = (double)G(a.std)[0];
        reinterpret_cast<GF_GLOBAL int64_t*>(ws)[3] = *G(a.count);
    }
}

// the reward normaliser's update and the rows' end: every workgroup folds the P records the same way (records strided over the lanes,
// the wave butterfly, the four waves in order), so all of them hold the same new std; workgroup 0 stores the statistics
__global__ __launch_bounds__(kSumBlock) void rnd_scale_kernel(const GfRndRewardArgs a, const int64_t P) {
    __shared__ double s_w[kSumBlock / GF_WAVE];
    const GF_GLOBAL double* ws = G(reinterpret_cast<const double*>(a.workspace));
    const GF_GLOBAL double* rec = ws + kRndHead;
    const int64_t count = reinterpret_cast<const GF_GLOBAL int64_t*>(ws)[3];
    float sd = (float)ws[2];
    if (!(a.until >= 0 && count >= a.until)) {   // (workgroup-uniform)
        const double m0 = rec[1];
        double a1 = 0.0, a2 = 0.0, am = 0.0;
        for (int64_t b = threadIdx.x; b < P; b += kSumBlock) {
            const double nb = rec[3 * b], dm = rec[3 * b + 1] - m0;
            a1 += nb * dm;
            a2 += nb * (dm * dm);
            am += rec[3 * b + 2];
        }
        a1 = block_sum_all(a1, s_w);
        a2 = block_sum_all(a2, s_w);
        am = block_sum_all(am, s_w);
        // rsl_rl's update lines on the batch of N avg values, in float64 from the f32 state (as gf_obs_norm_update)
        const double n = (double)a.num_envs;
        const double t = a1 / n;
        const double between = a2 - a1 * t;
        const double mx = m0 + t;
        const double vx = (am + (between > 0.0 ? between : 0.0)) / n;
        const double mean = ws[0], var = ws[1];
        const int64_t count1 = count + a.num_envs;
        const double rate = n / (double)count1;
        const double d = mx - mean;
        const double mean1 = mean + rate * d;
        const double var1 = var + rate * (vx - var + d * (mx - mean1));
        const float var_f = (float)var1;
        sd = sqrtf(var_f);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            G(a.mean)[0] = (float)mean1;
            G(a.var)[0] = var_f;
            G(a.std)[0] = sd;
            *G(a.count) = count1;
        }
    }
    const int64_t n = (int64_t)blockIdx.x * kSumBlock + threadIdx.x;
    if (n >= a.num_envs) return;
    const float r = G(a.intrinsic)[n];
    rnd_finish_row(a, n, sd > 0.0f ? r / sd : r);   // rsl_rl: no eps in this division
}
#endif  // GF_BODIES_ONLY

// gf_mlp_recurrent_act: an LSTM / GRU cell in front of each MLP, in the launch of gf_mlp_act.  The cell is the layer code's tile walk
// with the four accumulators of a wave holding the four gate columns of ONE 32-unit block (LSTM i, f, g, o; GRU n_x, r, z, n_h), so a
// lane has every pre-activation of its hidden unit for 16 rows and the non-linear tail needs no exchange.  Wave w owns the unit
// blocks w, w + 4, … in rounds (H <= 128: one round); per round the k loop runs over the input columns (x, staged through the
// normaliser in 512-column passes as a first layer's) and then the hidden columns, from a SECOND activation buffer that holds the
// tile's h (after the reset) for the whole cell — 2 x 65 664 = 131 328 B of LDS, one workgroup per CU.  (Not built: [x | h] as one k
// range in the one buffer, which keeps two workgroups per CU but re-stages h with every pass and round and cannot hold an input of
// 512 columns next to any h.)  h' and c' go to memory in place as a round ends — only this workgroup reads these rows, and it reads
// h from LDS — and when the rounds are over the workgroup reads its h' back into x: the MLP's input, staged as a layer's output is.
struct RnnSmem {
    MlpSmem m;
    float h[kMlpRows * kMlpXS];
};

__device__ __forceinline__ float rnn_sigmoid(float p) { return 1.0f / (1.0f + expf(-p)); }

template <bool LSTM>
__device__ __forceinline__ void rnn_cell(RnnSmem& sm, const GfMlpNet& net, const GfRnnCell& cell, const int K, const int64_t row0, const int64_t N) {
    constexpr int NBX = LSTM ? 4 : 3;   // accumulators the input columns feed (GRU: n_x, r, z), and the hidden ones (GRU: r, z, n_h)
    const int H = cell.hidden;
    const int UB = (H + 31) >> 5;
    const int rounds = (UB + kMlpWaves - 1) / kMlpWaves;
    const int passes = (K + GF_MLP_MAX_HIDDEN - 1) / GF_MLP_MAX_HIDDEN;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const bool norm = net.in_mean != nullptr;
    const bool vec_x = (K & 3) == 0 && (reinterpret_cast<uintptr_t>(cell.w_ih) & 15u) == 0;
    const bool vec_h = (H & 3) == 0 && (reinterpret_cast<uintptr_t>(cell.w_hh) & 15u) == 0;
    const GF_GLOBAL uint8_t* reset = cell.reset ? G(cell.reset) : nullptr;

    // h after the reset -> LDS (zeros past num_envs and from H to the chunk's end) and h_save
    const int hp = UB * 32;
    for (int e = (int)threadIdx.x; e < kMlpRows * hp; e += kMlpBlock) {
        const int row = e / hp, col = e - row * hp;
        const int64_t n = row0 + row;
        float v = 0.0f;
        if (n < N && col < H) {
            const bool rs = reset && reset[n] != 0;
            v = rs ? 0.0f : G(cell.h)[n * H + col];
            if (cell.h_save) G(cell.h_save)[n * H + col] = v;
        }
        sm.h[row * kMlpXS + col] = v;
    }

    for (int round = 0; round < rounds; ++round) {
        const int ub = round * kMlpWaves + wave;
        const bool active = ub < UB;   // (wave-uniform)
        const int j = ub * 32 + li;
        const bool real = active && j < H;
        const int jj = real ? j : 0;

        // gate g of unit j is row g · H + j of w_ih / w_hh; the accumulators in the order LSTM i f g o, GRU n_x r z n_h
        f32x16 acc[4];
        uint32_t rowx[NBX], rowh[NBX];   // (4 · 512 · 1 024 elements at most: 32 bits)
        {
            const GF_GLOBAL float* bi = G(cell.b_ih);
            const GF_GLOBAL float* bh = G(cell.b_hh);
            float b0[4];
            if (LSTM) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    b0[g] = bi[g * H + jj] + bh[g * H + jj];
                    rowx[g] = (uint32_t)(g * H + jj) * (uint32_t)K;
                    rowh[g] = (uint32_t)(g * H + jj) * (uint32_t)H;
                }
            } else {
                b0[0] = bi[2 * H + jj];
                b0[1] = bi[jj] + bh[jj];
                b0[2] = bi[H + jj] + bh[H + jj];
                b0[3] = bh[2 * H + jj];
                rowx[0] = (uint32_t)(2 * H + jj) * (uint32_t)K;
                rowx[1] = (uint32_t)jj * (uint32_t)K;
                rowx[2] = (uint32_t)(H + jj) * (uint32_t)K;
                rowh[0] = (uint32_t)jj * (uint32_t)H;
                rowh[1] = (uint32_t)(H + jj) * (uint32_t)H;
                rowh[2] = (uint32_t)(2 * H + jj) * (uint32_t)H;
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[g][r] = real ? b0[g] : 0.0f;
            }
        }

        // the input columns: x holds one pass at a time (a single pass stays for every round)
        for (int p = 0; p < passes; ++p) {
            const int p0 = p * GF_MLP_MAX_HIDDEN;
            const int cols = K - p0 < GF_MLP_MAX_HIDDEN ? K - p0 : GF_MLP_MAX_HIDDEN;
            if (round == 0 || passes > 1) {
                if (round || p) __syncthreads();   // (what x held is multiplied)
                mlp_stage_input<true>(sm.m, net, norm, p0, cols, (cols + 31) / 32 * 32, row0, N);
                __syncthreads();   // (round 0, pass 0: h is staged too)
            }
            if (active) {
                f32x16(&ax)[NBX] = reinterpret_cast<f32x16(&)[NBX]>(acc[0]);
                if (vec_x) mlp_k_loop<NBX, true>(sm.m.x, G(cell.w_ih), rowx, K, p0, p0 + cols, p0, li, lh, ax);
                else mlp_k_loop<NBX, false>(sm.m.x, G(cell.w_ih), rowx, K, p0, p0 + cols, p0, li, lh, ax);
            }
        }
        if (!active) continue;
        // the hidden columns, on the same chains (GRU: r, z and the second chain of n)
        {
            f32x16(&ah)[NBX] = reinterpret_cast<f32x16(&)[NBX]>(acc[LSTM ? 0 : 1]);
            if (vec_h) mlp_k_loop<NBX, true>(sm.h, G(cell.w_hh), rowh, H, 0, H, 0, li, lh, ah);
            else mlp_k_loop<NBX, false>(sm.h, G(cell.w_hh), rowh, H, 0, H, 0, li, lh, ah);
        }

        // the unit's tail, 16 rows per lane
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
            const int64_t n = row0 + row;
            if (!real || n >= N) continue;
            const int64_t at = n * H + j;
            float hn;
            if (LSTM) {
                const bool rs = reset && reset[n] != 0;
                const float c0 = rs ? 0.0f : G(cell.c)[at];
                if (cell.c_save) G(cell.c_save)[at] = c0;
                const float ig = rnn_sigmoid(acc[0][r]), fg = rnn_sigmoid(acc[1][r]), gg = tanhf(acc[2][r]), og = rnn_sigmoid(acc[3][r]);
                const float cn = __fadd_rn(__fmul_rn(fg, c0), __fmul_rn(ig, gg));
                G(cell.c)[at] = cn;
                hn = __fmul_rn(og, tanhf(cn));
            } else {
                const float h0 = sm.h[row * kMlpXS + j];
                const float rg = rnn_sigmoid(acc[1][r]), zg = rnn_sigmoid(acc[2][r]);
                const float ng = tanhf(__fadd_rn(acc[0][r], __fmul_rn(rg, acc[3][r])));
                hn = __fadd_rn(__fmul_rn(1.0f - zg, ng), __fmul_rn(zg, h0));
            }
            G(cell.h)[at] = hn;
        }
    }
    __syncthreads();   // x and h are read, h' is stored

    // h' -> x as a layer's output: H columns, zeros up to the longest chunk the first Linear may read to, zero rows past num_envs
    const int padded = (H + 127) / 128 * 128 < GF_MLP_MAX_HIDDEN ? (H + 127) / 128 * 128 : GF_MLP_MAX_HIDDEN;
    for (int e = (int)threadIdx.x; e < kMlpRows * padded; e += kMlpBlock) {
        const int row = e / padded, col = e - row * padded;
        const int64_t n = row0 + row;
        sm.m.x[row * kMlpXS + col] = n < N && col < H ? G(cell.h)[n * H + col] : 0.0f;
    }
    __syncthreads();
}

// every layer of `net` behind its cell on the tile's rows (a net without a cell: mlp_forward): the normaliser, the cell — state read,
// reset, advanced and stored in place — and the MLP walk from h'; the last layer's outputs are left in x; returns their width.
// gf_mlp_rdistill.hip's walk.  (mlp_recurrent_act_kernel keeps these lines in its own body: calling this function there allocated it
// one more VGPR, 194 for 193 — profiles/r27_recurrent_distill.md.)
__device__ __forceinline__ int rnn_forward(RnnSmem& sm, const GfMlpNet& net, const GfRnnCell& cell, const int64_t row0, const int64_t N) {
    int K;
    if (cell.type == GF_RNN_NONE) {
        K = mlp_forward<true>(sm.m, net, row0, N);
    } else {
        K = 0;
        for (int s = 0; s < net.num_inputs; ++s) K += net.inputs[s].width;
        if (cell.type == GF_RNN_LSTM) rnn_cell<true>(sm, net, cell, K, row0, N);
        else rnn_cell<false>(sm, net, cell, K, row0, N);
        K = cell.hidden;
        const int layers = net.num_layers;
        for (int l = 0; l < layers; ++l) {
            const GfMlpLayer& L = net.layers[l];
            const int nb = (((L.out_width + 31) >> 5) + kMlpWaves - 1) / kMlpWaves;
            const bool last = l == layers - 1;
            if (nb == 1) mlp_layer<1, true>(sm.m, net, L, K, false, last, row0, N);
            else if (nb == 2) mlp_layer<2, true>(sm.m, net, L, K, false, last, row0, N);
            else if (nb == 3) mlp_layer<3, true>(sm.m, net, L, K, false, last, row0, N);
            else mlp_layer<4, true>(sm.m, net, L, K, false, last, row0, N);
            K = L.out_width;
        }
    }
    return K;
}

#ifndef GF_BODIES_ONLY
// (one instance: the normaliser and log_std are workgroup-uniform run-time tests, as in rnd_tile_kernel and mlp_distill_kernel)
__global__ __launch_bounds__(kMlpBlock, 1) void mlp_recurrent_act_kernel(const GfMlpRecurrentActArgs ra, const int first_net, const int vec_rows) {
    __shared__ RnnSmem sm;
    const GfMlpActArgs& a = ra.act;
    const bool is_critic = (int)blockIdx.y + first_net == 1;
    const GfMlpNet& net = is_critic ? a.critic : a.actor;
    const GfRnnCell& cell = is_critic ? ra.critic_cell : ra.actor_cell;
    const int64_t N = a.num_envs;
    const int64_t row0 = (int64_t)blockIdx.x * kMlpRows;

    int K;
    if (cell.type == GF_RNN_NONE) {
        K = mlp_forward<true>(sm.m, net, row0, N);
    } else {
        K = 0;
        for (int s = 0; s < net.num_inputs; ++s) K += net.inputs[s].width;
        if (cell.type == GF_RNN_LSTM) rnn_cell<true>(sm, net, cell, K, row0, N);
        else rnn_cell<false>(sm, net, cell, K, row0, N);
        K = cell.hidden;
        const int layers = net.num_layers;
        for (int l = 0; l < layers; ++l) {
            const GfMlpLayer& L = net.layers[l];
            const int nb = (((L.out_width + 31) >> 5) + kMlpWaves - 1) / kMlpWaves;
            const bool last = l == layers - 1;
            if (nb == 1) mlp_layer<1, true>(sm.m, net, L, K, false, last, row0, N);
            else if (nb == 2) mlp_layer<2, true>(sm.m, net, L, K, false, last, row0, N);
            else if (nb == 3) mlp_layer<3, true>(sm.m, net, L, K, false, last, row0, N);
            else mlp_layer<4, true>(sm.m, net, L, K, false, last, row0, N);
            K = L.out_width;
        }
    }
    if (a.std_is_log) mlp_act_finish<true>(a, sm.m, is_critic, K, row0, vec_rows);
    else mlp_act_finish<false>(a, sm.m, is_critic, K, row0, vec_rows);
}
#endif  // GF_BODIES_ONLY

// GF_OK and the net's widths, or the refusal
static int mlp_check_net(const GfMlpNet& net, bool critic, int* out_width) {
    if (net.num_layers < 0 || net.num_layers > GF_MLP_MAX_LAYERS) return GF_E_RANGE;
    if (net.num_layers == 0) return GF_OK;
    if (net.num_inputs < 1 || net.num_inputs > GF_MLP_MAX_INPUTS) return GF_E_RANGE;
    int64_t in = 0;
    for (int s = 0; s < net.num_inputs; ++s) {
        if (!net.inputs[s].rows) return GF_E_NULL;
        if (net.inputs[s].width < 1 || (net.inputs[s].row_stride && net.inputs[s].row_stride < net.inputs[s].width)) return GF_E_RANGE;
        in += net.inputs[s].width;
    }
    if (in > GF_MLP_MAX_INPUT_WIDTH) return GF_E_RANGE;
    if (net.in_mean && !net.in_std) return GF_E_NULL;
    for (int l = 0; l < net.num_layers; ++l) {
        const GfMlpLayer& L = net.layers[l];
        if (!L.weight || !L.bias) return GF_E_NULL;
        if (L.out_width < 1) return GF_E_RANGE;
        if (l < net.num_layers - 1) {
            if (L.out_width > GF_MLP_MAX_HIDDEN) return GF_E_RANGE;
        } else if (critic) {
            if (L.out_width != 1) return GF_E_UNSUPPORTED;
        } else if (L.out_width > GF_MLP_MAX_ACTIONS) {
            return GF_E_RANGE;
        }
    }
    *out_width = net.layers[net.num_layers - 1].out_width;
    return GF_OK;
}

#ifndef GF_BODIES_ONLY
// gf_mlp_act's refusals (gf_mlp_recurrent_act's too): GF_OK, the actor's output width and which nets are there
static int mlp_act_check(const GfMlpActArgs& a, int* A, bool* has_actor, bool* has_critic) {
    if (a.num_envs < 0 || (a.std_per_env != 0 && a.std_per_env != 1) || (a.std_is_log != 0 && a.std_is_log != 1)) return GF_E_RANGE;
    int one = 0;
    int rc = mlp_check_net(a.actor, false, A);
    if (rc != GF_OK) return rc;
    rc = mlp_check_net(a.critic, true, &one);
    if (rc != GF_OK) return rc;
    const bool actor = a.actor.num_layers > 0, critic = a.critic.num_layers > 0;
    if (!actor && !critic) return GF_E_UNSUPPORTED;
    if (actor) {
        if (!a.mean && !a.actions) return GF_E_NULL;
        if (a.actions && !a.std) return GF_E_NULL;
        if (!a.actions && (a.actions_out || a.mu_out || a.sigma_out || a.log_prob_out)) return GF_E_NULL;
    } else if (a.mean || a.actions || a.actions_out || a.mu_out || a.sigma_out || a.log_prob_out) {
        return GF_E_NULL;
    }
    if (critic) {
        if (!a.values && !a.values_out) return GF_E_NULL;
    } else if (a.values || a.values_out) {
        return GF_E_NULL;
    }
    *has_actor = actor;
    *has_critic = critic;
    return GF_OK;
}
#endif  // GF_BODIES_ONLY

// gf_mlp_distill_act's refusals (gf_mlp_recurrent_distill_act's too): GF_OK and the output width of both nets
static int mlp_distill_check(const GfMlpDistillArgs& a, int* A) {
    if (a.num_envs < 0 || (a.std_is_log != 0 && a.std_is_log != 1)) return GF_E_RANGE;
    int At = 0;
    int rc = mlp_check_net(a.student, false, A);
    if (rc != GF_OK) return rc;
    rc = mlp_check_net(a.teacher, false, &At);
    if (rc != GF_OK) return rc;
    if (a.student.num_layers == 0 || a.teacher.num_layers == 0) return GF_E_UNSUPPORTED;
    if (*A != At) return GF_E_RANGE;
    if (!a.std || !a.actions || !a.teacher_actions) return GF_E_NULL;
    return GF_OK;
}

// a net's cell: GF_OK or the refusal (`present`: the net is in the launch)
static int rnn_check_cell(const GfRnnCell& c, bool present) {
    if (c.type != GF_RNN_NONE && c.type != GF_RNN_LSTM && c.type != GF_RNN_GRU) return GF_E_RANGE;
    if (c.type == GF_RNN_NONE) return c.h_save || c.c_save ? GF_E_NULL : GF_OK;
    if (!present) return GF_E_RANGE;
    if (c.hidden < 1 || c.hidden > GF_MLP_MAX_HIDDEN) return GF_E_RANGE;
    if (!c.w_ih || !c.w_hh || !c.b_ih || !c.b_hh || !c.h) return GF_E_NULL;
    if (c.type == GF_RNN_LSTM ? !c.c : (c.c || c.c_save)) return GF_E_NULL;
    return GF_OK;
}

// the launch's row tiles, or -1 where they pass a grid's x range
static int64_t mlp_tiles(int64_t num_envs) {
    const int64_t tiles = (num_envs + kMlpRows - 1) / kMlpRows;
    return tiles > 0x7fffffff ? -1 : tiles;
}

// whether the sampling lanes may use 16-byte accesses: every given [N, A] row pointer (and std) 16-byte aligned, A a multiple of 4
static int mlp_vec_rows(std::initializer_list<const void*> rows, int A) {
    uintptr_t bits = 0;
    for (const void* p : rows) bits |= reinterpret_cast<uintptr_t>(p);
    return (bits & 15u) == 0 && (A & 3) == 0;
}

}  // namespace gf

#ifndef GF_BODIES_ONLY
extern "C" __attribute__((visibility("default"))) int gf_mlp_act(const GfMlpActArgs* a, void* stream) {
    if (!a) return GF_E_NULL;
    int A = 0;
    bool actor = false, critic = false;
    const int rc = gf::mlp_act_check(*a, &A, &actor, &critic);
    if (rc != GF_OK) return rc;
    if (a->num_envs == 0) return GF_OK;
    const int64_t tiles = gf::mlp_tiles(a->num_envs);
    if (tiles < 0) return GF_E_RANGE;
    const int vec_rows = gf::mlp_vec_rows({a->noise, a->actions, a->actions_out, a->mu_out, a->sigma_out, a->std}, A);
    const bool norm = (actor && a->actor.in_mean) || (critic && a->critic.in_mean);
    const dim3 grid((unsigned)tiles, actor && critic ? 2u : 1u);
    const dim3 block(gf::kMlpBlock);
    hipStream_t s = (hipStream_t)stream;
    const int first_net = actor ? 0 : 1;
    if (a->std_is_log && a->actions) {   // (without actions nothing is sampled: the plain instances)
        if (norm) gf::klaunch(gf::mlp_act_kernel<true, true>, grid, block, 0, s, *a, first_net, vec_rows);
        else gf::klaunch(gf::mlp_act_kernel<false, true>, grid, block, 0, s, *a, first_net, vec_rows);
    } else {
        if (norm) gf::klaunch(gf::mlp_act_kernel<true, false>, grid, block, 0, s, *a, first_net, vec_rows);
        else gf::klaunch(gf::mlp_act_kernel<false, false>, grid, block, 0, s, *a, first_net, vec_rows);
    }
    return gf::launch_status();
}

extern "C" __attribute__((visibility("default"))) int gf_mlp_recurrent_act(const GfMlpRecurrentActArgs* ra, void* stream) {
    if (!ra) return GF_E_NULL;
    const GfMlpActArgs* a = &ra->act;
    int A = 0;
    bool actor = false, critic = false;
    int rc = gf::mlp_act_check(*a, &A, &actor, &critic);
    if (rc != GF_OK) return rc;
    rc = gf::rnn_check_cell(ra->actor_cell, actor);
    if (rc != GF_OK) return rc;
    rc = gf::rnn_check_cell(ra->critic_cell, critic);
    if (rc != GF_OK) return rc;
    if (ra->actor_cell.type == GF_RNN_NONE && ra->critic_cell.type == GF_RNN_NONE) return GF_E_UNSUPPORTED;   // gf_mlp_act's launch
    if (a->num_envs == 0) return GF_OK;
    const int64_t tiles = gf::mlp_tiles(a->num_envs);
    if (tiles < 0) return GF_E_RANGE;
    const int vec_rows = gf::mlp_vec_rows({a->noise, a->actions, a->actions_out, a->mu_out, a->sigma_out, a->std}, A);
    const dim3 grid((unsigned)tiles, actor && critic ? 2u : 1u);
    gf::klaunch(gf::mlp_recurrent_act_kernel, grid, dim3(gf::kMlpBlock), 0, (hipStream_t)stream, *ra, actor ? 0 : 1, vec_rows);
    return gf::launch_status();
}

extern "C" __attribute__((visibility("default"))) int gf_mlp_distill_act(const GfMlpDistillArgs* a, void* stream) {
    if (!a) return GF_E_NULL;
    int A = 0;
    const int rc = gf::mlp_distill_check(*a, &A);
    if (rc != GF_OK) return rc;
    if (a->num_envs == 0) return GF_OK;
    const int64_t tiles = gf::mlp_tiles(a->num_envs);
    if (tiles < 0) return GF_E_RANGE;
    const int vec_rows = gf::mlp_vec_rows({a->noise, a->actions, a->actions_out, a->std}, A);
    const dim3 grid((unsigned)tiles, 2u);
    const dim3 block(gf::kMlpBlock);
    hipStream_t s = (hipStream_t)stream;
    if (a->student.in_mean || a->teacher.in_mean) gf::klaunch(gf::mlp_distill_kernel<true>, grid, block, 0, s, *a, vec_rows);
    else gf::klaunch(gf::mlp_distill_kernel<false>, grid, block, 0, s, *a, vec_rows);
    return gf::launch_status();
}

extern "C" __attribute__((visibility("default"))) int gf_rnd_reward(const GfRndRewardArgs* a, void* stream) {
    if (!a) return GF_E_NULL;
    if (a->num_envs < 0 || (a->normalize != 0 && a->normalize != 1) || (a->update != 0 && a->update != 1) || (a->first != 0 && a->first != 1))
        return GF_E_RANGE;
    int Et = 0, Ep = 0;
    int rc = gf::mlp_check_net(a->target, false, &Et);
    if (rc != GF_OK) return rc;
    rc = gf::mlp_check_net(a->predictor, false, &Ep);
    if (rc != GF_OK) return rc;
    if (a->target.num_layers == 0 || a->predictor.num_layers == 0) return GF_E_UNSUPPORTED;
    if (Et != Ep || a->target.num_inputs != a->predictor.num_inputs) return GF_E_RANGE;
    for (int s = 0; s < a->target.num_inputs; ++s) {
        const GfMlpSegment &x = a->target.inputs[s], &y = a->predictor.inputs[s];
        if (x.rows != y.rows || x.width != y.width || x.row_stride != y.row_stride) return GF_E_RANGE;
    }
    if (!a->intrinsic || !a->workspace) return GF_E_NULL;
    if (a->normalize && (!a->avg || !a->mean || !a->var || !a->std || !a->count)) return GF_E_NULL;
    if (a->workspace_bytes < GF_RND_WORKSPACE_BYTES(a->num_envs) || (reinterpret_cast<uintptr_t>(a->workspace) & 7u) ||
        (a->normalize && (reinterpret_cast<uintptr_t>(a->count) & 7u)))
        return GF_E_RANGE;
    if (a->num_envs == 0) return GF_OK;
    const int64_t tiles = gf::mlp_tiles(a->num_envs);
    if (tiles < 0) return GF_E_RANGE;
    const int two_pass = a->normalize && a->update;
    const dim3 grid((unsigned)tiles), block(gf::kMlpBlock);
    hipStream_t s = (hipStream_t)stream;
    gf::klaunch(gf::rnd_tile_kernel, grid, block, 0, s, *a, two_pass);
    if (two_pass) {
        const int64_t nb = (a->num_envs + gf::kSumBlock - 1) / gf::kSumBlock;
        gf::klaunch(gf::rnd_scale_kernel, dim3((unsigned)nb), dim3(gf::kSumBlock), 0, s, *a, tiles);
    }
    return gf::launch_status();
}
#endif  // GF_BODIES_ONLY
