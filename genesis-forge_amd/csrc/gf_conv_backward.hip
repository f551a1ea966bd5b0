// gf_conv_backward.hip — gf_conv_encode_backward (include/gf_step.h has the contract): the gradients of the conv depth encoder's
// parameters from the gradient of its latent, in THREE launches with nothing saved by the forward.  The forward's device functions
// (conv_layer, the weight chunks, the gather) are gf_conv.hip's and gf_mlp.hip's, compiled here with GF_CONV_BODIES_ONLY /
// GF_BODIES_ONLY and the same flags: the recomputed activations are gf_conv_encode's bit for bit.
//
// Launch A, conv_bwd_tile_kernel: a persistent grid; workgroup g (four waves) walks the tiles g, g + G, … of T envs.
//   * LDS: two k tables, the row blocks' address words, ONE buffer per activation — the image and every layer's output, `[T][size | 1]`
//     in torch's [C, H, W] order — and the tile's rows of grad_latent.  The forward ping-pongs; here every output stays, because the
//     backward needs each layer's output for its ELU derivative and each layer's input for its wgrad.
//   * Forward: the image, then conv_layer per layer; the last activation is copied to the workspace's feat[n, flat] for launch B.
//   * Head dgrad: rows are the tile's envs (one 32-row block), columns the `flat` positions in 32-column blocks dealt to the waves,
//     the reduction runs over the latent.  A: grad_latent from LDS; B: head_weight[j][k] read in place, 32 consecutive k per j.  The
//     result times the ELU derivative of the stored output a — a > 0 ? 1 : a + 1 — REPLACES a: from here on a layer's output buffer
//     holds d_pre, the gradient of its pre-activation.
//   * Per layer, last to first.  wgrad: the [Cout, K] gradient in 32 x 32 tiles dealt to the waves; the reduction runs over the
//     tile's (env, oy, ox) rows, two ox per MFMA.  A: d_pre[env][co][oy][ox]; B: the im2col gather of the layer's input through the
//     forward's table word of the lane's k.  The wave adds its tile into the workgroup's slice of the workspace (stores on the
//     workgroup's first tile): the same lane owns an element every time.  The bias gradient, column K of the slice's [Cout, K + 1]
//     block, is no GEMM: a wave sums a channel's d_pre over the tile in double (a float32 chain of T·Ho·Wo same-signed terms would
//     cost several ulps) and rounds once per tile.
//     dgrad (layers 2 and 3): rows are INPUT positions (env, iy, ix), columns ci, the reduction k' = (co, dy, dx).  A: the gather
//     d_pre[env][co][(iy + p − dy) / s][(ix + p − dx) / s] through a table word (co·Ho·Wo, dy, dx) — zero where the division leaves a
//     remainder or the position is outside, so no LDS atomics; B: W[co][ci][dy][dx] through a second table word (co·K + dy·k + dx).  The
//     result times the ELU derivative replaces the input's stored output in place: wgrad of this layer is done with it.
//   Rows past num_envs carry a zero grad_latent: every gradient they add is zero.
// Launch B, conv_bwd_head_kernel: dWh = gᵀ · feat.  A workgroup owns 128 k columns (32 per wave) and one contiguous env range;
//   the accumulators (two 32-row blocks of the latent per pass) stay in registers over the whole range, K of the MFMA is the env
//   index, both operands are read in place (32 consecutive floats per env).  Column `flat` reads 1: the head's bias gradient.
// Launch C, conv_bwd_reduce_kernel: one thread per gradient element sums its slices in ascending order in double and rounds once.
// Tails everywhere are zeros SELECTED into operands, never a branch around an MFMA.  Resources and timings: profiles/r35_conv_backward.md.
#define GF_CONV_BODIES_ONLY
#include "gf_conv.hip"
#undef GF_CONV_BODIES_ONLY

namespace gf {

constexpr int kBwdActs = GF_CONV_MAX_LAYERS + 1;
constexpr int kBwdSlab = kMlpWaves * 32;   // k columns of launch B per workgroup
constexpr int kBwdNBJ = 2;                 // 32-row blocks of the latent per pass of launch B
constexpr int kBwdMaxSplits = 128, kBwdSplitEnvs = 128;
static_assert(GF_CONV_MAX_STRIDE <= 3 && GF_CONV_BWD_LDS_BYTES / 4 < (1 << 20), "the dgrad's division; the table word's offset field");

struct ConvBwdPlan {
    ConvLayerPlan l[GF_CONV_MAX_LAYERS];
    int layers, T, G, S;
    int es[kBwdActs];      // env stride of every activation buffer (odd)
    int aoff[kBwdActs + 1];   // where buffer i starts behind the tables, in floats; the last: the grad_latent rows
    int gs;                // env stride of the grad_latent rows (odd)
    int flat, latent, tab; // tab: words of ONE table
    int lds_bytes;
    int woff[GF_CONV_MAX_LAYERS];   // a layer's [Cout, K + 1] block in a conv slice
    int conv_words;                 // a conv slice
    int64_t tiles, per;             // tiles of T envs; envs per range of launch B
    int64_t feat_off, conv_off, head_off, ws_floats;   // the workspace, in floats
};

__device__ __forceinline__ float elu_grad(const float a) { return a > 0.0f ? 1.0f : a + 1.0f; }
__device__ __forceinline__ int acc_row(const int r, const int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// the forward's table of a layer's k = (ci, dy, dx), `words` long: zeros past K
__device__ __forceinline__ void bwd_table(const ConvLayerPlan& L, uint32_t* tab, const int words) {
    const int kk = L.kernel * L.kernel;
    for (int k = (int)threadIdx.x; k < words; k += kMlpBlock) {
        const int ci = k / kk, r = k - ci * kk, dy = r / L.kernel, dx = r - dy * L.kernel;
        tab[k] = k < L.K ? (uint32_t)(ci * L.hin * L.win + dy * L.win + dx) | (uint32_t)dy << 20 | (uint32_t)dx << 23 | kConvTapValid : 0u;
    }
}

// d_feat = g · Wh, times the ELU derivative, in place of the last activation
__device__ __forceinline__ void bwd_head_dgrad(const GF_GLOBAL float* Wh, const float* gl, float* act, const int T, const int es, const int gs,
                                               const int flat, const int latent) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const bool rowin = li < T;
    const float* gp = gl + (rowin ? li : 0) * gs;
    const int CB = (flat + 31) >> 5;
    for (int cb = wave; cb < CB; cb += kMlpWaves) {   // (wave-uniform)
        const int k = cb * 32 + li;
        const bool kin = k < flat;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        for (int j0 = 0; j0 < latent; j0 += 16) {
            float b[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int j = j0 + 2 * m + lh;
                const bool in = kin && j < latent;
                const float v = Wh[in ? (uint32_t)j * (uint32_t)flat + (uint32_t)k : 0u];
                b[m] = in ? v : 0.0f;
            }
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int j = j0 + 2 * m + lh;
                const bool in = rowin && j < latent;
                const float x = gp[in ? j : 0];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(in ? x : 0.0f, b[m], acc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = acc_row(r, lh);
            if (row < T && kin) {
                float* q = act + row * es + k;
                *q = acc[r] * elu_grad(*q);
            }
        }
    }
}

// dW[co][k] and (column K) db[co] of the tile, added into (first: stored to) the workgroup's slice
__device__ __forceinline__ void bwd_wgrad(const ConvLayerPlan& L, const float* in, const float* dp, const uint32_t* tab, GF_GLOBAL float* dst, const int T,
                                          const int es_in, const int es_out, const bool first) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const int K1 = L.K + 1, KB = (L.K + 31) >> 5, CB = (L.cout + 31) >> 5, HW = L.hout * L.wout;
    for (int t = wave; t < KB * CB; t += kMlpWaves) {   // (wave-uniform)
        const int cb = t / KB, kb = t - cb * KB;
        const int co = cb * 32 + li, k = kb * 32 + li;
        const bool coin = co < L.cout;
        const uint32_t e = tab[k];
        const bool valid = (e & kConvTapValid) != 0;
        const int dy = (int)((e >> 20) & 7u), dx = (int)((e >> 23) & 7u), off = (int)(e & 0xFFFFFu);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        for (int env = 0; env < T; ++env) {
            for (int oy = 0; oy < L.hout; ++oy) {
                const int iy0 = oy * L.stride - L.pad;
                const bool yok = valid && (unsigned)(iy0 + dy) < (unsigned)L.hin;
                const int abase = env * es_out + (coin ? co : 0) * HW + oy * L.wout;
                const int bbase = env * es_in + off + iy0 * L.win - L.pad;
                for (int ox0 = 0; ox0 < L.wout; ox0 += 2) {
                    const int ox = ox0 + lh;
                    const bool live = ox < L.wout, ain = live && coin;
                    const bool tap = live && yok && (unsigned)(ox * L.stride - L.pad + dx) < (unsigned)L.win;
                    const float a = dp[ain ? abase + ox : 0];
                    const float x = in[tap ? bbase + ox * L.stride : 0];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ain ? a : 0.0f, tap ? x : 0.0f, acc, 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = cb * 32 + acc_row(r, lh);
            if (c < L.cout && k < L.K) {
                GF_GLOBAL float* q = dst + c * K1 + k;
                *q = first ? acc[r] : *q + acc[r];
            }
        }
    }
    for (int co = wave; co < L.cout; co += kMlpWaves) {   // the bias: channel co's d_pre over the tile, in double, a fixed order
        double sum = 0.0;
        for (int i = lane; i < T * HW; i += GF_WAVE) {
            const int env = i / HW;
            sum += (double)dp[env * es_out + co * HW + (i - env * HW)];
        }
        sum = wave_xor_sum(sum);
        if (lane == 0) {
            GF_GLOBAL float* q = dst + co * K1 + L.K;
            *q = first ? (float)sum : *q + (float)sum;
        }
    }
}

// n / s and its remainder for 0 <= n < 2^16, s in 1 … 3
__device__ __forceinline__ int bwd_div(const int n, const int s) { return s == 1 ? n : s == 2 ? n >> 1 : (int)(((uint32_t)n * 43691u) >> 17); }

// the gradient of a layer's INPUT, times that input's ELU derivative, in place of it (`act`, the output of the layer before)
template <int NB>
__device__ __forceinline__ void bwd_dgrad(const ConvLayerPlan& L, const GF_GLOBAL float* W, const float* dp, float* act, const uint32_t* tab, const uint32_t* wtab,
                                          int* rowaddr, const int T, const int es_in, const int es_out) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const int kk = L.kernel * L.kernel, KK = L.cout * kk, HWi = L.hin * L.win, M = T * HWi, RB = (M + 31) >> 5, s = L.stride;
    bool real[NB];
    uint32_t cioff[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        real[b] = b * 32 + li < L.cin;
        cioff[b] = (uint32_t)(real[b] ? b * 32 + li : 0) * (uint32_t)kk;
    }
    int* ra_w = rowaddr + wave * 32;
    for (int rb = wave; rb < RB; rb += kMlpWaves) {   // (wave-uniform)
        const int m = rb * 32 + li;
        const bool live = m < M;
        const int mm = live ? m : 0, env = mm / HWi, pos = mm - env * HWi, iy = pos / L.win, ix = pos - iy * L.win;
        const int ty = iy + L.pad, tx = ix + L.pad, dbase = env * es_out;
        if (lh == 0) ra_w[li] = live ? env * es_in + pos : -1;   // (read back by this wave only, behind its k loop)
        f32x16 acc[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = 0.0f;
        }
        for (int k0 = 0; k0 < KK; k0 += 16) {
            float w[NB][8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int kq = k0 + 2 * q + lh;
                const uint32_t wo = wtab[kq];
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const bool in = real[b] && kq < KK;
                    const float v = W[in ? wo + cioff[b] : 0u];
                    w[b][q] = in ? v : 0.0f;
                }
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const uint32_t e = tab[k0 + 2 * q + lh];
                const int ny = ty - (int)((e >> 20) & 7u), nx = tx - (int)((e >> 23) & 7u);
                const int oy = bwd_div(ny < 0 ? 0 : ny, s), ox = bwd_div(nx < 0 ? 0 : nx, s);
                const bool tap = live && (e & kConvTapValid) != 0 && ny >= 0 && nx >= 0 && oy * s == ny && ox * s == nx && oy < L.hout && ox < L.wout;
                const float x = dp[tap ? dbase + (int)(e & 0xFFFFFu) + oy * L.wout + ox : 0];
                const float av = tap ? x : 0.0f;
#pragma unroll
                for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, w[b][q], acc[b], 0, 0, 0);
            }
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int at = ra_w[acc_row(r, lh)];
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                if (at >= 0 && real[b]) {
                    float* q = act + at + (b * 32 + li) * HWi;
                    *q = acc[b][r] * elu_grad(*q);
                }
            }
        }
        __builtin_amdgcn_wave_barrier();   // (the next row block's address words)
    }
}

__global__ __launch_bounds__(kMlpBlock, 2) void conv_bwd_tile_kernel(const GfConvBackwardArgs ba, const ConvBwdPlan p) {
    extern __shared__ float bwd_smem[];
    const GfConvEncodeArgs& a = ba.enc;
    uint32_t* tab = reinterpret_cast<uint32_t*>(bwd_smem);
    uint32_t* wtab = tab + p.tab;
    int* rowaddr = reinterpret_cast<int*>(bwd_smem + 2 * p.tab);
    float* const base = bwd_smem + 2 * p.tab + kConvRowWords;
    const int T = p.T, tid = (int)threadIdx.x, layers = p.layers;
    float* const gl = base + p.aoff[layers + 1];
    const int64_t N = a.num_envs;
    GF_GLOBAL float* ws = G(reinterpret_cast<float*>(ba.workspace));
    GF_GLOBAL float* slice = ws + p.conv_off + (int64_t)blockIdx.x * p.conv_words;
    const int S0 = p.l[0].cin * p.l[0].hin * p.l[0].win;
    const int64_t istride = a.image_stride ? a.image_stride : S0, gstride = ba.grad_row_stride ? ba.grad_row_stride : p.latent;

    bool first = true;
    for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x, first = false) {
        const int64_t row0 = tile * T;
        // the image -> activation 0, grad_latent -> gl (zeros for the tile's rows past num_envs)
        for (int row = 0; row < T; ++row) {
            const int64_t n = row0 + row;
            const GF_GLOBAL float* src = G(a.image) + (n < N ? n : 0) * istride;
            for (int i = tid; i < S0; i += kMlpBlock) (base + p.aoff[0])[row * p.es[0] + i] = n < N ? src[i] : 0.0f;
            const GF_GLOBAL float* gsrc = G(ba.grad_latent) + (n < N ? n : 0) * gstride;
            for (int j = tid; j < p.latent; j += kMlpBlock) gl[row * p.gs + j] = n < N ? gsrc[j] : 0.0f;
        }
        // the forward, gf_conv_encode's: every output kept
        for (int l = 0; l < layers; ++l) {
            const ConvLayerPlan& L = p.l[l];
            const GfConvLayer& P = a.layers[l];
            bwd_table(L, tab, (L.K + 32) & ~31);
            __syncthreads();   // the table, and the layer's input
            const bool vec = (L.K & 3) == 0 && (reinterpret_cast<uintptr_t>(P.weight) & 15u) == 0;
            if (L.cout <= 32) {
                if (vec) conv_layer<1, true>(L, P, (base + p.aoff[l]), (base + p.aoff[l + 1]), tab, rowaddr, T, p.es[l], p.es[l + 1]);
                else conv_layer<1, false>(L, P, (base + p.aoff[l]), (base + p.aoff[l + 1]), tab, rowaddr, T, p.es[l], p.es[l + 1]);
            } else {
                if (vec) conv_layer<2, true>(L, P, (base + p.aoff[l]), (base + p.aoff[l + 1]), tab, rowaddr, T, p.es[l], p.es[l + 1]);
                else conv_layer<2, false>(L, P, (base + p.aoff[l]), (base + p.aoff[l + 1]), tab, rowaddr, T, p.es[l], p.es[l + 1]);
            }
            __syncthreads();   // every wave is done with the table; the output is whole
        }
        // the last activation -> feat[n, flat], for launch B
        for (int row = 0; row < T; ++row) {
            const int64_t n = row0 + row;
            if (n >= N) break;   // (workgroup-uniform)
            GF_GLOBAL float* dst = ws + p.feat_off + n * p.flat;
            for (int e = tid; e < p.flat; e += kMlpBlock) dst[e] = (base + p.aoff[layers])[row * p.es[layers] + e];
        }
        __syncthreads();   // the head dgrad overwrites what was just copied
        bwd_head_dgrad(G(a.head_weight), gl, (base + p.aoff[layers]), T, p.es[layers], p.gs, p.flat, p.latent);
        for (int l = layers - 1; l >= 0; --l) {
            const ConvLayerPlan& L = p.l[l];
            bwd_table(L, tab, (L.K + 32) & ~31);
            __syncthreads();   // the table, and d_pre of this layer's output
            bwd_wgrad(L, (base + p.aoff[l]), (base + p.aoff[l + 1]), tab, slice + p.woff[l], T, p.es[l], p.es[l + 1], first);
            __syncthreads();   // the dgrad's tables replace this one; it overwrites the wgrad's B operand
            if (l == 0) break;
            const int kk = L.kernel * L.kernel, KK = L.cout * kk, HWo = L.hout * L.wout;
            for (int k = tid; k < ((KK + 15) & ~15); k += kMlpBlock) {   // k' = (co, dy, dx)
                const int co = k / kk, r = k - co * kk, dy = r / L.kernel, dx = r - dy * L.kernel;
                tab[k] = k < KK ? (uint32_t)(co * HWo) | (uint32_t)dy << 20 | (uint32_t)dx << 23 | kConvTapValid : 0u;
                wtab[k] = k < KK ? (uint32_t)(co * L.K + r) : 0u;
            }
            __syncthreads();
            if (L.cin <= 32) bwd_dgrad<1>(L, G(a.layers[l].weight), (base + p.aoff[l + 1]), (base + p.aoff[l]), tab, wtab, rowaddr, T, p.es[l], p.es[l + 1]);
            else bwd_dgrad<2>(L, G(a.layers[l].weight), (base + p.aoff[l + 1]), (base + p.aoff[l]), tab, wtab, rowaddr, T, p.es[l], p.es[l + 1]);
            // (the next layer's table build meets before anything reads this one's result)
            __syncthreads();
        }
        // (the loop's last barrier: the next tile's loads overwrite what the wgrad of layer 0 read)
    }
}

// launch B: the partial [latent, flat + 1] of one env range, 128 k columns per workgroup
__global__ __launch_bounds__(kMlpBlock, 2) void conv_bwd_head_kernel(const GfConvBackwardArgs ba, const ConvBwdPlan p) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const int flat = p.flat, K1 = flat + 1, latent = p.latent;
    const int kb = (int)blockIdx.x * kMlpWaves + wave, k = kb * 32 + li;
    if (kb * 32 >= K1) return;   // (wave-uniform; nothing meets in this kernel)
    const bool kin = k < flat, kone = k == flat;
    const int64_t N = ba.enc.num_envs, n0 = (int64_t)blockIdx.y * p.per, n1 = n0 + p.per < N ? n0 + p.per : N;
    const int64_t gstride = ba.grad_row_stride ? ba.grad_row_stride : latent;
    GF_GLOBAL float* ws = G(reinterpret_cast<float*>(ba.workspace));
    const GF_GLOBAL float* feat = ws + p.feat_off;
    const GF_GLOBAL float* g = G(ba.grad_latent);
    GF_GLOBAL float* part = ws + p.head_off + (int64_t)blockIdx.y * latent * K1;
    const int JB = (latent + 31) >> 5;
    for (int jb0 = 0; jb0 < JB; jb0 += kBwdNBJ) {
        f32x16 acc[kBwdNBJ];
#pragma unroll
        for (int b = 0; b < kBwdNBJ; ++b) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = 0.0f;
        }
        for (int64_t n = n0; n < n1; n += 16) {
            float bv[8], av[kBwdNBJ][8];
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int64_t nn = n + 2 * m + lh;
                const bool nin = nn < n1;
                const float x = feat[nin && kin ? nn * flat + k : 0];
                bv[m] = nin && kin ? x : nin && kone ? 1.0f : 0.0f;
#pragma unroll
                for (int b = 0; b < kBwdNBJ; ++b) {
                    const int j = (jb0 + b) * 32 + li;
                    const bool jin = nin && j < latent;
                    const float y = g[jin ? nn * gstride + j : 0];
                    av[b][m] = jin ? y : 0.0f;
                }
            }
#pragma unroll
            for (int m = 0; m < 8; ++m) {
#pragma unroll
                for (int b = 0; b < kBwdNBJ; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[b][m], bv[m], acc[b], 0, 0, 0);
            }
        }
#pragma unroll
        for (int b = 0; b < kBwdNBJ; ++b) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = (jb0 + b) * 32 + acc_row(r, lh);
                if (j < latent && k < K1) part[(int64_t)j * K1 + k] = acc[b][r];
            }
        }
    }
}

// launch C: what to sum into what
struct BwdSegment {
    const float* src;    // slice 0
    float* dw;           // [rows, cols − 1]
    float* db;           // [rows]: column cols − 1
    int64_t stride;      // floats between slices
    int64_t begin;       // the segment's first element in the launch's index space
    int slices, cols;
};
struct BwdReduce {
    BwdSegment seg[GF_CONV_MAX_LAYERS + 1];
    int count;
    int64_t total;
};

__global__ __launch_bounds__(kSumBlock) void conv_bwd_reduce_kernel(const BwdReduce rd) {
    const int64_t e = (int64_t)blockIdx.x * kSumBlock + threadIdx.x;
    if (e >= rd.total) return;
    int s = 0;
#pragma unroll
    for (int i = 1; i <= GF_CONV_MAX_LAYERS; ++i) s = i < rd.count && e >= rd.seg[i].begin ? i : s;
    const BwdSegment& sg = rd.seg[s];
    const int64_t i = e - sg.begin, r = i / sg.cols;
    const int c = (int)(i - r * sg.cols);
    const GF_GLOBAL float* src = G(sg.src) + i;
    double sum = 0.0;
    for (int sl = 0; sl < sg.slices; ++sl) sum += (double)src[sl * sg.stride];   // ascending: the same bits on every launch
    if (c < sg.cols - 1) G(sg.dw)[r * (sg.cols - 1) + c] = (float)sum;
    else G(sg.db)[r] = (float)sum;
}

// gf_conv_encode_backward's shape and plan refusals (no pointer is looked at): GF_OK and the plan
static int conv_backward_plan(const GfConvBackwardArgs& ba, ConvBwdPlan* p) {
    const GfConvEncodeArgs& a = ba.enc;
    if (a.num_envs < 0 || a.num_layers < 1 || a.num_layers > GF_CONV_MAX_LAYERS) return GF_E_RANGE;
    if (a.channels < 1 || a.channels > GF_CONV_MAX_CHANNELS || a.height < 1 || a.width < 1 || a.height > 4096 || a.width > 4096) return GF_E_RANGE;
    if (a.latent_dim < 1 || a.latent_dim > GF_CONV_MAX_LATENT) return GF_E_RANGE;
    if (a.num_inputs < 0 || a.num_inputs > GF_MLP_MAX_INPUTS) return GF_E_RANGE;
    int64_t w1 = 0;
    for (int s = 0; s < a.num_inputs; ++s) {
        if (a.inputs[s].width < 1 || (a.inputs[s].row_stride && a.inputs[s].row_stride < a.inputs[s].width)) return GF_E_RANGE;
        w1 += a.inputs[s].width;
    }
    if (w1 > GF_MLP_MAX_INPUT_WIDTH) return GF_E_RANGE;
    int c = a.channels, h = a.height, w = a.width, tab = 0, words = 0;
    int64_t per_env = (int64_t)c * h * w | 1;
    if (a.image_stride && a.image_stride < (int64_t)c * h * w) return GF_E_RANGE;
    p->es[0] = (int)(per_env < 0x7fffffff ? per_env : 0x7fffffff);
    for (int l = 0; l < a.num_layers; ++l) {
        const GfConvLayer& L = a.layers[l];
        if (L.out_channels < 1 || L.out_channels > GF_CONV_MAX_CHANNELS || L.kernel < 1 || L.kernel > GF_CONV_MAX_KERNEL || L.stride < 1 ||
            L.stride > GF_CONV_MAX_STRIDE || L.padding < 0 || L.padding >= L.kernel)
            return GF_E_RANGE;
        if (h + 2 * L.padding < L.kernel || w + 2 * L.padding < L.kernel) return GF_E_RANGE;   // an output smaller than 1 x 1
        const int ho = (h + 2 * L.padding - L.kernel) / L.stride + 1, wo = (w + 2 * L.padding - L.kernel) / L.stride + 1;
        const int K = c * L.kernel * L.kernel, KK = L.out_channels * L.kernel * L.kernel;
        p->l[l] = ConvLayerPlan{c, h, w, L.out_channels, L.kernel, L.stride, L.padding, ho, wo, K};
        const int need = ((l ? (K + 1 > KK ? K + 1 : KK) : K + 1) + 31) & ~31;
        tab = need > tab ? need : tab;
        p->woff[l] = words;
        words += L.out_channels * (K + 1);
        c = L.out_channels, h = ho, w = wo;
        const int64_t size = (int64_t)c * h * w | 1;
        p->es[l + 1] = (int)(size < 0x7fffffff ? size : 0x7fffffff);
        per_env += size;
    }
    const int nl = a.num_layers;
    const int64_t flat = (int64_t)c * h * w;
    p->layers = nl, p->latent = a.latent_dim, p->gs = a.latent_dim | 1, p->tab = tab, p->conv_words = words;
    per_env = 4 * (per_env + p->gs);
    const int64_t fixed = 4 * (2 * (int64_t)tab + kConvRowWords);
    if (fixed + per_env > GF_CONV_BWD_LDS_BYTES) return GF_E_RANGE;   // one env's backward does not fit
    p->flat = (int)flat;
    if (ba.tile_envs < 0 || ba.tile_envs > GF_CONV_MAX_TILE_ENVS || ba.groups < 0 || ba.groups > GF_CONV_BWD_MAX_GROUPS) return GF_E_RANGE;
    int64_t T = (GF_CONV_BWD_LDS_BYTES - fixed) / per_env;
    T = T > GF_CONV_MAX_TILE_ENVS ? GF_CONV_MAX_TILE_ENVS : T;
    if (ba.tile_envs > T) return GF_E_RANGE;   // a forced tile that does not fit
    if (ba.tile_envs) T = ba.tile_envs;
    p->T = (int)T;
    p->aoff[0] = 0;
    for (int i = 0; i <= nl; ++i) p->aoff[i + 1] = p->aoff[i] + (int)T * p->es[i];
    p->lds_bytes = (int)(fixed + T * per_env);
    const int64_t N = a.num_envs;
    p->tiles = (N + T - 1) / T;
    const int64_t G = ba.groups ? ba.groups : GF_CONV_BWD_GROUPS;
    p->G = (int)(N && p->tiles < G ? p->tiles : G);
    const int64_t splits = (N + kBwdSplitEnvs - 1) / kBwdSplitEnvs < kBwdMaxSplits ? (N + kBwdSplitEnvs - 1) / kBwdSplitEnvs : kBwdMaxSplits;
    p->per = N ? ((N + splits - 1) / splits + 1) & ~(int64_t)1 : 2;
    p->S = (int)((N + p->per - 1) / p->per);
    p->feat_off = 0;
    p->conv_off = (N * flat + 3) & ~(int64_t)3;
    p->head_off = p->conv_off + (N ? (int64_t)p->G * words : 0);
    p->ws_floats = p->head_off + (int64_t)p->S * a.latent_dim * (flat + 1);
    return GF_OK;
}

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_conv_backward_sizeof(void) { return (int)sizeof(GfConvBackwardArgs); }

extern "C" __attribute__((visibility("default"))) int gf_conv_backward_plan(const GfConvBackwardArgs* a, int* tile_envs_out, int* groups_out, int* lds_bytes_out,
                                                                             int* flat_out) {
    if (!a) return GF_E_NULL;
    gf::ConvBwdPlan p;
    const int rc = gf::conv_backward_plan(*a, &p);
    if (rc != GF_OK) return rc;
    if (tile_envs_out) *tile_envs_out = p.T;
    if (groups_out) *groups_out = p.G;
    if (lds_bytes_out) *lds_bytes_out = p.lds_bytes;
    if (flat_out) *flat_out = p.flat;
    return GF_OK;
}

extern "C" __attribute__((visibility("default"))) int64_t gf_conv_backward_workspace_bytes(const GfConvBackwardArgs* a) {
    if (!a) return GF_E_NULL;
    gf::ConvBwdPlan p;
    const int rc = gf::conv_backward_plan(*a, &p);
    return rc != GF_OK ? rc : 4 * p.ws_floats;
}

extern "C" __attribute__((visibility("default"))) int gf_conv_encode_backward(const GfConvBackwardArgs* ba, void* stream) {
    (void)&gf::mlp_distill_check, (void)&gf::rnn_check_cell, (void)&gf::mlp_tiles, (void)&gf::mlp_vec_rows;   // (gf_mlp.hip's host helpers: not this entry's)
    if (!ba) return GF_E_NULL;
    gf::ConvBwdPlan p;
    const int rc = gf::conv_backward_plan(*ba, &p);
    if (rc != GF_OK) return rc;
    const GfConvEncodeArgs* a = &ba->enc;
    if (!a->image || !a->head_weight || !a->head_bias || !ba->grad_latent || !ba->grad_head_weight || !ba->grad_head_bias) return GF_E_NULL;
    for (int l = 0; l < a->num_layers; ++l)
        if (!a->layers[l].weight || !a->layers[l].bias || !ba->grad_weight[l] || !ba->grad_bias[l]) return GF_E_NULL;
    if (a->num_envs > 0 && !ba->workspace) return GF_E_NULL;
    if (ba->grad_row_stride && ba->grad_row_stride < a->latent_dim) return GF_E_RANGE;
    if (ba->workspace_bytes < 4 * p.ws_floats) return GF_E_RANGE;

    hipStream_t s = (hipStream_t)stream;
    const bool any = a->num_envs > 0;
#if GF_CONV_BWD_LDS_BYTES > 65536   // (a build with a larger budget: the launch needs the dynamic-LDS limit raised)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gf::conv_bwd_tile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, GF_CONV_BWD_LDS_BYTES);
#endif
    if (any) {
        gf::klaunch(gf::conv_bwd_tile_kernel, dim3((unsigned)p.G), dim3(gf::kMlpBlock), (size_t)p.lds_bytes, s, *ba, p);
        gf::klaunch(gf::conv_bwd_head_kernel, dim3((unsigned)((p.flat + 1 + gf::kBwdSlab - 1) / gf::kBwdSlab), (unsigned)p.S), dim3(gf::kMlpBlock), 0, s, *ba, p);
    }
    gf::BwdReduce rd{};
    const float* ws = reinterpret_cast<const float*>(ba->workspace);
    int64_t begin = 0;
    for (int l = 0; l < a->num_layers; ++l) {
        const int cols = p.l[l].K + 1;
        rd.seg[l] = gf::BwdSegment{any ? ws + p.conv_off + p.woff[l] : nullptr, ba->grad_weight[l], ba->grad_bias[l], p.conv_words, begin, any ? p.G : 0, cols};
        begin += (int64_t)p.l[l].cout * cols;
    }
    rd.seg[a->num_layers] = gf::BwdSegment{any ? ws + p.head_off : nullptr, ba->grad_head_weight, ba->grad_head_bias, (int64_t)a->latent_dim * (p.flat + 1), begin,
                                           any ? p.S : 0, p.flat + 1};
    begin += (int64_t)a->latent_dim * (p.flat + 1);
    rd.count = a->num_layers + 1, rd.total = begin;
    gf::klaunch(gf::conv_bwd_reduce_kernel, dim3((unsigned)((begin + gf::kSumBlock - 1) / gf::kSumBlock)), dim3(gf::kSumBlock), 0, s, rd);
    return gf::launch_status();
}
