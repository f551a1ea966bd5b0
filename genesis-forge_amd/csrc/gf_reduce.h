// gf_reduce.h — the fixed-order double sums of the learner's loss and optimiser kernels (gf_ppo.hip, gf_mirror.hip, gf_distill.hip).
// One definition of the order is what keeps their results bitwise reproducible: the xor butterfly inside a wave, the
// four waves of a 256-thread workgroup in wave order, the workgroups' records strided over one workgroup's lanes.
#pragma once
#include "gf_device.h"

namespace gf {

constexpr int kSumBlock = 256;   // the workgroup sums below fold exactly four wave sums

// wave butterfly: every lane ends with the same sum, in the same order whatever the data (gf_device.h's wave_sum is the shift-down
// form, valid in lane 0 only)
__device__ __forceinline__ double wave_xor_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, GF_WAVE);
    return v;
}

// the four wave sums in s_w, added in wave order
__device__ __forceinline__ double fold_wave_sums(const double* s_w) { return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3]; }

// workgroup sum, for one use of s_w per kernel: lane 0 of each wave leaves its wave's sum in s_w, the workgroup meets; the thread
// that wants the total (thread 0 in every caller) then calls fold_wave_sums(s_w)
__device__ __forceinline__ void block_wave_sums(double v, double* s_w) {
    v = wave_xor_sum(v);
    if ((threadIdx.x & (GF_WAVE - 1)) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
}

// workgroup sum, for repeated use of s_w: every lane gets the result
__device__ __forceinline__ double block_sum_all(double v, double* s_w) {
    v = wave_xor_sum(v);
    __syncthreads();   // (s_w may still be read by an earlier use)
    if ((threadIdx.x & (GF_WAVE - 1)) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return fold_wave_sums(s_w);
}

// The finalize launch of a "mean of per-workgroup records" loss (gf_mirror_loss, gf_bc_loss), one workgroup of BLOCK threads: the nb
// records summed in a fixed order, the mean over rows · actions elements to out[0] and, where given, added to sums[0] (rsl_rl's
// mean_…_loss += loss.item())
template <int BLOCK>
__device__ __forceinline__ void finalize_mean_loss(const void* workspace, const int64_t nb, const int64_t rows, const int actions, float* out,
                                                   double* sums) {
    static_assert(BLOCK == kSumBlock, "four waves");
    __shared__ double s_w[BLOCK / GF_WAVE];
    const GF_GLOBAL double* ws = G(reinterpret_cast<const double*>(workspace));
    double acc = 0.0;
    for (int64_t b = threadIdx.x; b < nb; b += BLOCK) acc += ws[b];
    block_wave_sums(acc, s_w);
    if (threadIdx.x != 0) return;
    const float loss = (float)(fold_wave_sums(s_w) / ((double)rows * (double)actions));
    G(out)[0] = loss;
    if (sums) G(sums)[0] = G(sums)[0] + (double)loss;
}

}  // namespace gf
