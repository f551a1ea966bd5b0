// gf_conv.hip — gf_conv_encode (include/gf_step.h has the contract): the convolutional depth encoder in front of a distillation
// student — Conv2d + ELU (one to three), flatten, Linear — and the student's normalised 1-D columns, written as the student MLP's
// complete input row in ONE launch.  The weight access and the head's tile walk are gf_mlp.hip's device functions, compiled here with
// GF_BODIES_ONLY (as gf_mlp_rdistill.hip does); the conv layers' implicit GEMM is this file's.
//
// A workgroup of four waves owns a tile of T envs (conv_plan: the largest T <= 32 that fits the budget of 64 KB, two workgroups per CU).
//   * LDS holds two activation buffers the layers ping-pong between — the image and every even activation in buffer 0, the odd ones
//     in buffer 1 — each `[T][stride]` with an env's activation in torch's [C, H, W] order (so flatten is the identity) and an odd
//     stride; a table of one word per k of the current layer; 32 words per wave for the store addresses of a row block.  Nothing
//     between the image load and the `out` store goes to memory.
//   * A conv layer is the GEMM  rows (env in tile, oy, ox) x k (ci, dy, dx) x columns Cout  on v_mfma_f32_32x32x2_f32.  A wave takes
//     the 32-row blocks w, w + 4, … and all (one or two) 32-column blocks of each, so the gathered A operand is fetched once per k
//     for both.  B operand: lane l reads row j of the weight matrix in place along k — torch's [Cout, Cin, k, k] IS the row-major
//     [Cout, K] — 16 k per chunk (8 per lane half, 16 bytes at a time where K % 4 == 0 and the rows are aligned, by element
//     otherwise), the next chunk in flight while this one multiplies, and v_permlane32_swap turns (k | k + 8) into (k | k + 1) as in
//     gf_mlp.hip.  A operand: the im2col gather from LDS.  The table word of k holds (ci·H·W + dy·W + dx, dy, dx, k < K) — built once
//     per layer by the workgroup, so the k loop has no division — and a lane keeps its row's (base address, iy0, ix0): the tap is
//     in the image iff (unsigned)(iy0 + dy) < H and (unsigned)(ix0 + dx) < W.  Padding taps, rows past T·Ho·Wo, k past K and columns
//     past Cout are zeros SELECTED into the operands (the address falls back to the buffer's first word): never a branch around an
//     MFMA.  An output element is one k-ascending fma chain started from its bias; ELU; the store goes to the other buffer at
//     [env][j][oy][ox] through the row block's address words.
//   * The head is gf_mlp.hip's layer walk over ONE 32-row block whose rows are the tile's envs (rows past T read the last env's
//     activation; they are never stored): wave w owns the 32-column blocks w, w + 4, … of the latent, streams its weight rows in
//     gf_mlp.hip's chunks (mlp_load_chunk) and multiplies them against the flattened activation read straight from LDS (mlp_multiply).
//     The head's input buffer has its stride rounded up to the chunk and the columns past `flat` zeroed, as a layer's output there.
//     The accumulators go from registers to `out[n, W1 + j]`: no activation.
//   * The 1-D columns are copied (through the normaliser: gf_mlp.hip's staging arithmetic, one subtraction, one addition, one correctly
//     rounded division) by the whole workgroup while nothing else is in flight.
// Summation order is fixed by k alone: the same bits for any N, any T and any launch.
// Resources (the compiler's report): profiles/r33_conv_encoder.md.
#define GF_BODIES_ONLY
#include "gf_mlp.hip"
#undef GF_BODIES_ONLY

namespace gf {

constexpr int kConvKC = 16, kConvH = kConvKC / 2;   // k per chunk of a conv layer, and per lane half
constexpr int kConvRowWords = kMlpWaves * 32;       // the store addresses of one row block per wave
constexpr uint32_t kConvTapValid = 1u << 26;        // table word: bits 0–19 the tap's offset in an env's activation, 20–22 dy, 23–25 dx
static_assert(GF_CONV_MAX_KERNEL <= 7 && GF_CONV_LDS_BYTES / 4 < (1 << 20), "the table word's fields");
static_assert(GF_CONV_MAX_TILE_ENVS == kMlpRows && GF_CONV_MAX_CHANNELS <= 64, "the head is one row block; a conv layer has at most two column blocks");

struct ConvLayerPlan {
    int cin, hin, win, cout, kernel, stride, pad, hout, wout, K;
};

// what the host works out once per launch (conv_plan) and the kernel takes by value
struct ConvPlan {
    ConvLayerPlan l[GF_CONV_MAX_LAYERS];
    int T;            // envs per workgroup
    int es[2];        // env stride of the two activation buffers (odd)
    int flat;         // the head's input width
    int tab;          // table words: the longest K rounded up to the chunk
    int w1;           // 1-D columns
    int head_nb;      // 32-column blocks per wave in the head
    int lds_bytes;
};

// this lane's weights of a chunk: for block b, row rowoff[b] / K, columns kl + (0 … 7); zeros past K and in a block past Cout
template <int NB, bool VEC>
__device__ __forceinline__ void conv_load_w(const GF_GLOBAL float* W, const uint32_t (&rowoff)[NB], const bool (&real)[NB], int K, int kl,
                                            float (&r)[NB][kConvH]) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (VEC) {
#pragma unroll
            for (int e = 0; e < kConvH; e += 4) {
                const bool in = real[b] && kl + e < K;   // (K % 4 == 0: a quad is inside or outside as a whole)
                const f32x4 v = *reinterpret_cast<const GF_GLOBAL f32x4*>(W + (rowoff[b] + (uint32_t)(in ? kl + e : 0)));
                r[b][e] = in ? v.x : 0.0f; r[b][e + 1] = in ? v.y : 0.0f; r[b][e + 2] = in ? v.z : 0.0f; r[b][e + 3] = in ? v.w : 0.0f;
            }
        } else {
#pragma unroll
            for (int e = 0; e < kConvH; ++e) {
                const bool in = real[b] && kl + e < K;
                const float v = W[rowoff[b] + (uint32_t)(in ? kl + e : 0)];
                r[b][e] = in ? v : 0.0f;
            }
        }
    }
}

// a lane's row of the implicit GEMM: where its receptive field starts
struct ConvRow {
    int base;   // env · stride + iy0 · W + ix0 in the input buffer (may be negative: only valid taps are read)
    int iy0, ix0;
    bool live;
};

// the chunk's MFMAs: the swap as in mlp_multiply, the A operand gathered per k through the table
template <int NB>
__device__ __forceinline__ void conv_multiply(const float* in, const uint32_t* tab, const int k0, const int lh, const ConvRow& row, const int hin,
                                              const int win, float (&r)[NB][kConvH], f32x16 (&acc)[NB]) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int m = 0; m < kConvH; m += 2) {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(r[b][m]), __float_as_uint(r[b][m + 1]), false, false);
            r[b][m] = __uint_as_float(sw[0]);
            r[b][m + 1] = __uint_as_float(sw[1]);
        }
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int m = 0; m < kConvH; m += 2) {
            const uint32_t e = tab[k0 + half * kConvH + m + lh];
            const int dy = (int)((e >> 20) & 7u), dx = (int)((e >> 23) & 7u);
            const bool tap = row.live && (e & kConvTapValid) != 0 && (unsigned)(row.iy0 + dy) < (unsigned)hin && (unsigned)(row.ix0 + dx) < (unsigned)win;
            const float x = in[tap ? row.base + (int)(e & 0xFFFFFu) : 0];
            const float av = tap ? x : 0.0f;
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, r[b][m + half], acc[b], 0, 0, 0);
        }
    }
}

// One Conv2d + ELU of the tile: `in` (env stride es_in) -> `out` (env stride es_out).  The callers meet before (the table, `in`) and after.
template <int NB, bool VEC>
__device__ __forceinline__ void conv_layer(const ConvLayerPlan& L, const GfConvLayer& P, const float* in, float* out, const uint32_t* tab, int* rowaddr,
                                           const int T, const int es_in, const int es_out) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const int K = L.K, O = L.cout, HW = L.hout * L.wout, M = T * HW, RB = (M + 31) >> 5;
    const GF_GLOBAL float* W = G(P.weight);
    uint32_t rowoff[NB];
    bool real[NB];
    float bv[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int j = b * 32 + li;
        real[b] = j < O;
        rowoff[b] = (uint32_t)(real[b] ? j : 0) * (uint32_t)K;
        bv[b] = real[b] ? G(P.bias)[j] : 0.0f;
    }
    int* ra_w = rowaddr + wave * 32;

    for (int rb = wave; rb < RB; rb += kMlpWaves) {   // (wave-uniform)
        ConvRow row;
        {
            const int m = rb * 32 + li;
            row.live = m < M;
            const int mm = row.live ? m : 0;
            const int env = mm / HW, pos = mm - env * HW, oy = pos / L.wout, ox = pos - oy * L.wout;
            row.iy0 = oy * L.stride - L.pad;
            row.ix0 = ox * L.stride - L.pad;
            row.base = env * es_in + row.iy0 * L.win + row.ix0;
            if (lh == 0) ra_w[li] = row.live ? env * es_out + pos : -1;   // (read back by this wave only, behind its k loop)
        }
        f32x16 acc[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = bv[b];   // (the column is on the lane)
        }

        // the k loop: registers for two chunks, the one being multiplied and the one in flight, by turns
        float wa[NB][kConvH], wb[NB][kConvH];
        int k = 0;
        conv_load_w<NB, VEC>(W, rowoff, real, K, lh * kConvH, wa);
        for (;;) {
            if (k + kConvKC < K) conv_load_w<NB, VEC>(W, rowoff, real, K, k + kConvKC + lh * kConvH, wb);
            conv_multiply<NB>(in, tab, k, lh, row, L.hin, L.win, wa, acc);
            k += kConvKC;
            if (k >= K) break;
            if (k + kConvKC < K) conv_load_w<NB, VEC>(W, rowoff, real, K, k + kConvKC + lh * kConvH, wa);
            conv_multiply<NB>(in, tab, k, lh, row, L.hin, L.win, wb, acc);
            k += kConvKC;
            if (k >= K) break;
        }

        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int at = ra_w[(r & 3) + 8 * (r >> 2) + 4 * lh];
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const float v = acc[b][r];
                if (at >= 0 && real[b]) out[at + (b * 32 + li) * HW] = v > 0.0f ? v : expm1f(v);
            }
        }
        __builtin_amdgcn_wave_barrier();   // (the next row block's address words)
    }
}

// The head: out[n, w1 + j] = bias[j] + sum over k of act[env][k] · weight[j][k], NB 32-column blocks per wave, gf_mlp.hip's chunks.
template <int NB>
__device__ __forceinline__ void conv_head(const GfConvEncodeArgs& a, const ConvPlan& p, const float* in, const int es, const int64_t row0) {
    constexpr int KC = mlp_kc(NB);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const int K = p.flat, O = a.latent_dim, CB = (O + 31) >> 5;
    if (wave >= CB) return;   // (wave-uniform; nothing meets behind the head)
    const bool vec = (K & 3) == 0 && (reinterpret_cast<uintptr_t>(a.head_weight) & 15u) == 0;
    const GF_GLOBAL float* W = G(a.head_weight);
    f32x16 acc[NB];
    uint32_t rowoff[NB];   // (latent · flat <= 512 · 16 384: 32 bits)
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int j = (wave + kMlpWaves * b) * 32 + li;
        rowoff[b] = (uint32_t)(j < O ? j : 0) * (uint32_t)K;
        const float bv = G(a.head_bias)[j < O ? j : 0];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = j < O ? bv : 0.0f;
    }
    const float* ap = in + (li < p.T ? li : p.T - 1) * es + lh;
    float r[NB][KC / 2];
    for (int k = 0; k < K; k += KC) {
        if (vec) mlp_load_chunk<NB, true>(W, rowoff, K, k, lh, r);
        else mlp_load_chunk<NB, false>(W, rowoff, K, k, lh, r);
        mlp_multiply<NB>(ap + k, r, acc);
    }
    const int64_t N = a.num_envs;
    const int OS = p.w1 + O;
    GF_GLOBAL float* dst = G(a.out);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int j = (wave + kMlpWaves * b) * 32 + li;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int row = (rr & 3) + 8 * (rr >> 2) + 4 * lh;
            const int64_t n = row0 + row;
            if (row < p.T && n < N && j < O) dst[n * OS + p.w1 + j] = acc[b][rr];
        }
    }
}

#ifndef GF_CONV_BODIES_ONLY   // (gf_conv_banded.hip compiles the device functions above)
__global__ __launch_bounds__(kMlpBlock, 2) void conv_encode_kernel(const GfConvEncodeArgs a, const ConvPlan p) {
    extern __shared__ float conv_smem[];
    uint32_t* tab = reinterpret_cast<uint32_t*>(conv_smem);
    int* rowaddr = reinterpret_cast<int*>(conv_smem + p.tab);
    float* const buf0 = conv_smem + p.tab + kConvRowWords;
    float* const buf1 = buf0 + p.T * p.es[0];
    const int T = p.T, tid = (int)threadIdx.x;
    const int64_t N = a.num_envs, row0 = (int64_t)blockIdx.x * T;

    // the 1-D columns: segments -> out[n, 0 : W1], through the normaliser where there is one
    {
        const int W1 = p.w1, OS = W1 + a.latent_dim;
        const bool norm = a.in_mean != nullptr;
        for (int e = tid; e < T * W1; e += kMlpBlock) {
            const int row = e / W1, col = e - row * W1;
            const int64_t n = row0 + row;
            if (n >= N) break;   // (rows ascend with e)
            int k = col;
            const float* rows = a.inputs[0].rows;
            int64_t off = 0;
#pragma unroll
            for (int s = 0; s < GF_MLP_MAX_INPUTS; ++s) {
                const int w = s < a.num_inputs ? a.inputs[s].width : 0;
                const bool hit = k >= 0 && k < w;
                rows = hit ? a.inputs[s].rows : rows;
                const int stride = a.inputs[s].row_stride ? a.inputs[s].row_stride : w;
                off = hit ? n * stride + k : off;
                k -= w;
            }
            float v = G(rows)[off];
            if (norm) v = (v - G(a.in_mean)[col]) / (G(a.in_std)[col] + a.in_eps);   // gf_mlp.hip's mlp_stage_input
            G(a.out)[n * OS + col] = v;
        }
    }

    // the image -> buffer 0 (zeros for the tile's rows past num_envs)
    {
        const int S0 = p.l[0].cin * p.l[0].hin * p.l[0].win;
        const int64_t istride = a.image_stride ? a.image_stride : S0;
        for (int row = 0; row < T; ++row) {
            const int64_t n = row0 + row;
            const GF_GLOBAL float* src = G(a.image) + (n < N ? n : 0) * istride;
            for (int i = tid; i < S0; i += kMlpBlock) buf0[row * p.es[0] + i] = n < N ? src[i] : 0.0f;
        }
    }

    const int layers = a.num_layers;
    for (int l = 0; l < layers; ++l) {
        const ConvLayerPlan& L = p.l[l];
        const GfConvLayer& P = a.layers[l];
        const float* in = l & 1 ? buf1 : buf0;
        float* out = l & 1 ? buf0 : buf1;
        const int es_in = l & 1 ? p.es[1] : p.es[0], es_out = l & 1 ? p.es[0] : p.es[1];
        // the table of this layer's k: (ci, dy, dx) in torch's weight order
        const int kk = L.kernel * L.kernel, kpad = (L.K + kConvKC - 1) / kConvKC * kConvKC;
        for (int k = tid; k < kpad; k += kMlpBlock) {
            const int ci = k / kk, r = k - ci * kk, dy = r / L.kernel, dx = r - dy * L.kernel;
            tab[k] = k < L.K ? (uint32_t)(ci * L.hin * L.win + dy * L.win + dx) | (uint32_t)dy << 20 | (uint32_t)dx << 23 | kConvTapValid : 0u;
        }
        if (l == layers - 1) {   // the head reads whole chunks: zeros from `flat` to the stride's end (this layer reads the other buffer)
            const int w = es_out - p.flat;
            for (int e = tid; e < T * w; e += kMlpBlock) {
                const int row = e / w;
                out[row * es_out + p.flat + (e - row * w)] = 0.0f;
            }
        }
        __syncthreads();   // the table, and `in`: the image or the previous layer's stores
        const bool vec = (L.K & 3) == 0 && (reinterpret_cast<uintptr_t>(P.weight) & 15u) == 0;
        if (L.cout <= 32) {
            if (vec) conv_layer<1, true>(L, P, in, out, tab, rowaddr, T, es_in, es_out);
            else conv_layer<1, false>(L, P, in, out, tab, rowaddr, T, es_in, es_out);
        } else {
            if (vec) conv_layer<2, true>(L, P, in, out, tab, rowaddr, T, es_in, es_out);
            else conv_layer<2, false>(L, P, in, out, tab, rowaddr, T, es_in, es_out);
        }
        __syncthreads();   // every wave is done with the table and `in`; `out` is whole
    }

    const float* act = layers & 1 ? buf1 : buf0;
    const int es = layers & 1 ? p.es[1] : p.es[0];
    if (p.head_nb == 1) conv_head<1>(a, p, act, es, row0);
    else if (p.head_nb == 2) conv_head<2>(a, p, act, es, row0);
    else if (p.head_nb == 3) conv_head<3>(a, p, act, es, row0);
    else conv_head<4>(a, p, act, es, row0);
}

// gf_conv_encode's shape refusals and its tile (no pointer is looked at): GF_OK and the plan
static int conv_plan(const GfConvEncodeArgs& a, ConvPlan* p) {
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
    int c = a.channels, h = a.height, w = a.width, tab = 0;
    int64_t size[GF_CONV_MAX_LAYERS + 1];
    size[0] = (int64_t)c * h * w;
    if (a.image_stride && a.image_stride < size[0]) return GF_E_RANGE;
    for (int l = 0; l < a.num_layers; ++l) {
        const GfConvLayer& L = a.layers[l];
        if (L.out_channels < 1 || L.out_channels > GF_CONV_MAX_CHANNELS || L.kernel < 1 || L.kernel > GF_CONV_MAX_KERNEL || L.stride < 1 ||
            L.stride > GF_CONV_MAX_STRIDE || L.padding < 0 || L.padding >= L.kernel)
            return GF_E_RANGE;
        if (h + 2 * L.padding < L.kernel || w + 2 * L.padding < L.kernel) return GF_E_RANGE;   // an output smaller than 1 x 1
        const int ho = (h + 2 * L.padding - L.kernel) / L.stride + 1, wo = (w + 2 * L.padding - L.kernel) / L.stride + 1;
        const int K = c * L.kernel * L.kernel;
        p->l[l] = ConvLayerPlan{c, h, w, L.out_channels, L.kernel, L.stride, L.padding, ho, wo, K};
        const int kpad = (K + kConvKC - 1) / kConvKC * kConvKC;
        tab = kpad > tab ? kpad : tab;
        c = L.out_channels, h = ho, w = wo;
        size[l + 1] = (int64_t)c * h * w;
    }
    const int nl = a.num_layers;
    const int head_nb = (((a.latent_dim + 31) >> 5) + kMlpWaves - 1) / kMlpWaves;
    const int kc = mlp_kc(head_nb);
    int64_t es[2] = {0, 0};
    for (int i = 0; i <= nl; ++i) {
        const int64_t need = i == nl ? (size[i] + kc - 1) / kc * kc : size[i];   // (the head reads whole chunks)
        es[i & 1] = need > es[i & 1] ? need : es[i & 1];
    }
    es[0] |= 1, es[1] |= 1;   // odd: the head's 32 rows of a k column on 32 banks
    const int64_t fixed = 4 * ((int64_t)tab + kConvRowWords), per_env = 4 * (es[0] + es[1]);
    int64_t T = (GF_CONV_LDS_BYTES - fixed) / per_env;
    T = T > GF_CONV_MAX_TILE_ENVS ? GF_CONV_MAX_TILE_ENVS : T;
    if (T < 1) return GF_E_RANGE;   // one env's activations do not fit
    p->T = (int)T;
    p->es[0] = (int)es[0], p->es[1] = (int)es[1];
    p->flat = (int)size[nl];
    p->tab = tab;
    p->w1 = (int)w1;
    p->head_nb = head_nb;
    p->lds_bytes = (int)(fixed + T * per_env);
    return GF_OK;
}

#endif  // GF_CONV_BODIES_ONLY

}  // namespace gf

#ifndef GF_CONV_BODIES_ONLY
extern "C" __attribute__((visibility("default"))) int gf_conv_encode_sizeof(void) { return (int)sizeof(GfConvEncodeArgs); }

extern "C" __attribute__((visibility("default"))) int gf_conv_plan(const GfConvEncodeArgs* a, int* tile_envs_out, int* lds_bytes_out, int* flat_out) {
    if (!a) return GF_E_NULL;
    gf::ConvPlan p;
    const int rc = gf::conv_plan(*a, &p);
    if (rc != GF_OK) return rc;
    if (tile_envs_out) *tile_envs_out = p.T;
    if (lds_bytes_out) *lds_bytes_out = p.lds_bytes;
    if (flat_out) *flat_out = p.flat;
    return GF_OK;
}

extern "C" __attribute__((visibility("default"))) int gf_conv_encode(const GfConvEncodeArgs* a, void* stream) {
    (void)&gf::mlp_distill_check, (void)&gf::rnn_check_cell, (void)&gf::mlp_tiles, (void)&gf::mlp_vec_rows;   // (gf_mlp.hip's host helpers: not this entry's)
    if (!a) return GF_E_NULL;
    gf::ConvPlan p;
    const int rc = gf::conv_plan(*a, &p);
    if (rc != GF_OK) return rc;
    if (!a->image || !a->out || !a->head_weight || !a->head_bias || (a->in_mean && !a->in_std)) return GF_E_NULL;
    for (int l = 0; l < a->num_layers; ++l)
        if (!a->layers[l].weight || !a->layers[l].bias) return GF_E_NULL;
    for (int s = 0; s < a->num_inputs; ++s)
        if (!a->inputs[s].rows) return GF_E_NULL;
    if (a->num_envs == 0) return GF_OK;
    const int64_t tiles = (a->num_envs + p.T - 1) / p.T;
    if (tiles > 0x7fffffff) return GF_E_RANGE;
    gf::klaunch(gf::conv_encode_kernel, dim3((unsigned)tiles), dim3(gf::kMlpBlock), (size_t)p.lds_bytes, (hipStream_t)stream, *a, p);
    return gf::launch_status();
}
#endif  // GF_CONV_BODIES_ONLY
