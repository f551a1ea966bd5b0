// gf_conv_banded.hip — gf_conv_encode_banded (include/gf_step.h has the contract): gf_conv_encode's row for images whose activations
// do not fit one LDS tile, and for tiles of a few envs, in TWO launches.  The weight chunks, the gather and the MFMA sequence are
// gf_conv.hip's and gf_mlp.hip's device functions, compiled here with GF_CONV_BODIES_ONLY / GF_BODIES_ONLY: an output element is the
// same k-ascending fma chain, so `out` is gf_conv_encode's bit for bit wherever that serves the shape.
//
// Launch A, conv_banded_kernel: a workgroup of four waves owns (a tile of T envs, a band of R output rows of the LAST conv layer).
//   * conv_band_range walks the layers backwards from the band: the rows [lo, hi) of every activation the band needs — a layer's input
//     rows [olo·s − p, (ohi − 1)·s − p + k) clipped to the activation.  Neighbouring bands recompute the halo rows of the intermediate
//     layers: the price of keeping everything in LDS.
//   * LDS holds gf_conv.hip's two ping-pong buffers, each `[T][C · (hi − lo) · W]` (an odd env stride sized for the largest band), the
//     k table of the current layer and the row blocks' address words.  The image rows of the band are loaded, every layer is
//     conv_band_layer — gf_conv.hip's conv_layer with the band's row origin in the row decode: the tap test is in the activation's own
//     coordinates, the LDS address relative to the band's first row — so a row above row 0 or below H is padding, zeros selected, never
//     a computed value and never stale LDS.
//   * The band's last activation is copied from LDS to `feat[n, flat]` at torch's [C, H, W] offsets, contiguous runs of (hi − lo) · W.
//   * The workgroups of band 0 write the normalised 1-D columns, gf_conv.hip's arithmetic.
// Launch B, conv_head_kernel<NB, VEC>: a workgroup owns 32 envs; wave w owns the 32-column blocks w, w + 4, … of the latent (NB of them).
//   * `feat` rows go through LDS in slabs of 256 k columns, two buffers of `[32][257]`: a thread fetches its 32 floats of slab s + 1 into
//     registers (16 bytes at a time with VEC) before slab s is multiplied and stores them behind it — one barrier per slab.  Rows past
//     num_envs and columns past `flat` are zeros.
//   * The multiply is mlp_load_chunk / mlp_multiply from k = 0 upwards, no split-K; with one column block per wave (a latent of up to 128) the next
//     weight chunk is in flight while this one multiplies, across slab borders too.  The head's weights are read once per 32 envs.
// The host plan (conv_banded_plan) picks (T, R) within GF_CONV_LDS_BYTES: whole images with the largest T <= 32, a smaller R only
// where not even one env fits.
// Resources (the compiler's report) and timings: profiles/r34_conv_banded.md.
#define GF_CONV_BODIES_ONLY
#include "gf_conv.hip"
#undef GF_CONV_BODIES_ONLY

namespace gf {

constexpr int kHeadSlab = 256, kHeadSS = kHeadSlab + 1;   // k columns of `feat` per slab; the slab's row stride (odd: 32 rows of a column on 32 banks)
constexpr int kHeadStage = kMlpRows * kHeadSlab / kMlpBlock;   // floats of a slab per thread
static_assert(kHeadSlab % (2 * mlp_kc(1)) == 0 && kHeadStage % 4 == 0, "a full slab is an even number of chunks; a thread stages whole quads");

struct ConvBandPlan {
    ConvLayerPlan l[GF_CONV_MAX_LAYERS];
    int layers;
    int T, R, bands;  // envs per workgroup; rows of the last layer's output per band; bands
    int es[2];        // env stride of the two activation buffers (odd), sized for the band that needs most
    int flat;
    int tab;          // table words
    int w1;
    int head_nb;
    int lds_bytes;
};

// rows [lo, hi) of activation i (0: the image … layers: the last layer's output) that band b needs
__host__ __device__ __forceinline__ void conv_band_range(const ConvBandPlan& p, const int b, const int i, int& lo, int& hi) {
    lo = b * p.R;
    hi = lo + p.R < p.l[p.layers - 1].hout ? lo + p.R : p.l[p.layers - 1].hout;
    for (int l = p.layers - 1; l >= i; --l) {
        const ConvLayerPlan& L = p.l[l];
        const int first = lo * L.stride - L.pad, end = (hi - 1) * L.stride - L.pad + L.kernel;
        lo = first > 0 ? first : 0;
        hi = end < L.hin ? end : L.hin;
    }
}

// gf_conv.hip's conv_layer on a band: output rows [olo, olo + rout) of the layer, `in` holding the input's rows from ilo on
template <int NB, bool VEC>
__device__ __forceinline__ void conv_band_layer(const ConvLayerPlan& L, const GfConvLayer& P, const float* in, float* out, const uint32_t* tab, int* rowaddr,
                                                const int T, const int es_in, const int es_out, const int olo, const int rout, const int ilo) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const int K = L.K, O = L.cout, HW = rout * L.wout, M = T * HW, RB = (M + 31) >> 5;
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
            const int env = mm / HW, pos = mm - env * HW, oyl = pos / L.wout, ox = pos - oyl * L.wout;
            row.iy0 = (olo + oyl) * L.stride - L.pad;   // (in the activation: the tap test's coordinate)
            row.ix0 = ox * L.stride - L.pad;
            row.base = env * es_in + (row.iy0 - ilo) * L.win + row.ix0;   // (in the band: a valid tap's row is at or below ilo)
            if (lh == 0) ra_w[li] = row.live ? env * es_out + pos : -1;
        }
        f32x16 acc[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = bv[b];
        }

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

__global__ __launch_bounds__(kMlpBlock, 2) void conv_banded_kernel(const GfConvBandedArgs ba, const ConvBandPlan p) {
    extern __shared__ float band_smem[];
    const GfConvEncodeArgs& a = ba.enc;
    uint32_t* tab = reinterpret_cast<uint32_t*>(band_smem);
    int* rowaddr = reinterpret_cast<int*>(band_smem + p.tab);
    float* const buf0 = band_smem + p.tab + kConvRowWords;
    float* const buf1 = buf0 + p.T * p.es[0];
    const int T = p.T, tid = (int)threadIdx.x, band = (int)blockIdx.y;
    const int64_t N = a.num_envs, row0 = (int64_t)blockIdx.x * T;

    // the 1-D columns, by the tile's first band: segments -> out[n, 0 : W1], through the normaliser where there is one
    if (band == 0) {
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

    // the band's image rows -> buffer 0, channel by channel (zeros for the tile's rows past num_envs)
    {
        const ConvLayerPlan& L0 = p.l[0];
        int lo, hi;
        conv_band_range(p, band, 0, lo, hi);
        const int HW = L0.hin * L0.win, part = (hi - lo) * L0.win;
        const int64_t istride = a.image_stride ? a.image_stride : (int64_t)L0.cin * HW;
        for (int row = 0; row < T; ++row) {
            const int64_t n = row0 + row;
            const GF_GLOBAL float* src = G(a.image) + (n < N ? n : 0) * istride + lo * L0.win;
            for (int c = 0; c < L0.cin; ++c)
                for (int i = tid; i < part; i += kMlpBlock) buf0[row * p.es[0] + c * part + i] = n < N ? src[c * HW + i] : 0.0f;
        }
    }

    const int layers = p.layers;
    for (int l = 0; l < layers; ++l) {
        const ConvLayerPlan& L = p.l[l];
        const GfConvLayer& P = a.layers[l];
        const float* in = l & 1 ? buf1 : buf0;
        float* out = l & 1 ? buf0 : buf1;
        const int es_in = l & 1 ? p.es[1] : p.es[0], es_out = l & 1 ? p.es[0] : p.es[1];
        int ilo, ihi, olo, ohi;
        conv_band_range(p, band, l, ilo, ihi);
        conv_band_range(p, band, l + 1, olo, ohi);
        // the table of this layer's k: (ci, dy, dx) in torch's weight order, a channel of the input being the band's rows
        const int kk = L.kernel * L.kernel, kpad = (L.K + kConvKC - 1) / kConvKC * kConvKC, chan = (ihi - ilo) * L.win;
        for (int k = tid; k < kpad; k += kMlpBlock) {
            const int ci = k / kk, r = k - ci * kk, dy = r / L.kernel, dx = r - dy * L.kernel;
            tab[k] = k < L.K ? (uint32_t)(ci * chan + dy * L.win + dx) | (uint32_t)dy << 20 | (uint32_t)dx << 23 | kConvTapValid : 0u;
        }
        __syncthreads();   // the table, and `in`: the image rows or the previous layer's stores
        const bool vec = (L.K & 3) == 0 && (reinterpret_cast<uintptr_t>(P.weight) & 15u) == 0;
        if (L.cout <= 32) {
            if (vec) conv_band_layer<1, true>(L, P, in, out, tab, rowaddr, T, es_in, es_out, olo, ohi - olo, ilo);
            else conv_band_layer<1, false>(L, P, in, out, tab, rowaddr, T, es_in, es_out, olo, ohi - olo, ilo);
        } else {
            if (vec) conv_band_layer<2, true>(L, P, in, out, tab, rowaddr, T, es_in, es_out, olo, ohi - olo, ilo);
            else conv_band_layer<2, false>(L, P, in, out, tab, rowaddr, T, es_in, es_out, olo, ohi - olo, ilo);
        }
        __syncthreads();   // every wave is done with the table and `in`; `out` is whole
    }

    // the band of the last activation -> feat[n] at [c][olo …][·]: runs of (ohi − olo) · W floats
    {
        const ConvLayerPlan& L = p.l[layers - 1];
        const float* act = layers & 1 ? buf1 : buf0;
        const int es = layers & 1 ? p.es[1] : p.es[0];
        int olo, ohi;
        conv_band_range(p, band, layers, olo, ohi);
        const int part = (ohi - olo) * L.wout, HW = L.hout * L.wout, total = L.cout * part;
        for (int row = 0; row < T; ++row) {
            const int64_t n = row0 + row;
            if (n >= N) break;   // (workgroup-uniform)
            GF_GLOBAL float* dst = G(ba.feat) + n * p.flat + olo * L.wout;
            for (int e = tid; e < total; e += kMlpBlock) {
                const int c = e / part;
                dst[c * HW + (e - c * part)] = act[row * es + e];
            }
        }
    }
}

// what launch B takes by value
struct ConvHeadArgs {
    const float* feat;
    const float* weight;
    const float* bias;
    float* out;
    int64_t num_envs;
    int flat, latent, w1;
};

// this thread's floats of the slab from column k0: zeros past num_envs and past `flat` (VEC: flat % 4 == 0 and 16-byte rows)
template <bool VEC>
__device__ __forceinline__ void head_fetch(const ConvHeadArgs& h, const int64_t row0, const int k0, float (&st)[kHeadStage]) {
    const int tid = (int)threadIdx.x, K = h.flat;
    const GF_GLOBAL float* F = G(h.feat);
    if (VEC) {
#pragma unroll
        for (int i = 0; i < kHeadStage / 4; ++i) {
            const int q = tid + kMlpBlock * i, row = q / (kHeadSlab / 4), c = (q % (kHeadSlab / 4)) * 4;
            const int64_t n = row0 + row;
            const bool in = n < h.num_envs && k0 + c < K;   // (a quad is inside or outside as a whole)
            const f32x4 v = *reinterpret_cast<const GF_GLOBAL f32x4*>(F + (in ? n * K + k0 + c : 0));
            st[4 * i] = in ? v.x : 0.0f; st[4 * i + 1] = in ? v.y : 0.0f; st[4 * i + 2] = in ? v.z : 0.0f; st[4 * i + 3] = in ? v.w : 0.0f;
        }
    } else {
#pragma unroll
        for (int i = 0; i < kHeadStage; ++i) {   // (row i, column tid)
            const int64_t n = row0 + i;
            const bool in = n < h.num_envs && k0 + tid < K;
            const float v = F[in ? n * K + k0 + tid : 0];
            st[i] = in ? v : 0.0f;
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void head_store(float* slab, const float (&st)[kHeadStage]) {
    const int tid = (int)threadIdx.x;
    if (VEC) {
#pragma unroll
        for (int i = 0; i < kHeadStage / 4; ++i) {
            const int q = tid + kMlpBlock * i, at = q / (kHeadSlab / 4) * kHeadSS + (q % (kHeadSlab / 4)) * 4;
            slab[at] = st[4 * i]; slab[at + 1] = st[4 * i + 1]; slab[at + 2] = st[4 * i + 2]; slab[at + 3] = st[4 * i + 3];
        }
    } else {
#pragma unroll
        for (int i = 0; i < kHeadStage; ++i) slab[i * kHeadSS + tid] = st[i];
    }
}

template <int NB, bool VEC>
__global__ __launch_bounds__(kMlpBlock, 2) void conv_head_kernel(const ConvHeadArgs h) {
    constexpr int KC = mlp_kc(NB), H = KC / 2;
    __shared__ float slabs[2][kMlpRows * kHeadSS];
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const int K = h.flat, O = h.latent, CB = (O + 31) >> 5;
    const int64_t N = h.num_envs, row0 = (int64_t)blockIdx.x * kMlpRows;
    const bool mul = wave < CB;   // (wave-uniform: a wave without a column block only stages)
    const GF_GLOBAL float* W = G(h.weight);
    f32x16 acc[NB];
    uint32_t rowoff[NB];   // (latent · flat <= 512 · 16 384: 32 bits)
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int j = (wave + kMlpWaves * b) * 32 + li;
        rowoff[b] = (uint32_t)(j < O ? j : 0) * (uint32_t)K;
        const float bv = G(h.bias)[j < O ? j : 0];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = j < O ? bv : 0.0f;
    }

    float st[kHeadStage];
    float ra[NB][H];
    head_fetch<VEC>(h, row0, 0, st);
    if (NB == 1 && mul) mlp_load_chunk<NB, VEC>(W, rowoff, K, 0, lh, ra);
    const int count = (K + kHeadSlab - 1) / kHeadSlab;
    for (int s = 0; s < count; ++s) {
        float* cur = slabs[s & 1];
        head_store<VEC>(cur, st);   // (the waves are past the barrier of slab s − 1: nobody reads this buffer, slab s − 2's, any more)
        __syncthreads();
        if (s + 1 < count) head_fetch<VEC>(h, row0, (s + 1) * kHeadSlab, st);
        if (!mul) continue;
        const float* ap = cur + li * kHeadSS + lh - s * kHeadSlab;
        const int k1 = (s + 1) * kHeadSlab < K ? (s + 1) * kHeadSlab : K;
        int k = s * kHeadSlab;
        if constexpr (NB == 1) {   // registers for two chunks by turns (mlp_k_loop); a full slab is an even number of them, so `ra` is
                                   // the chunk in flight at every slab border.  (Two column blocks with the staged slab spill.)
            float rb[NB][H];
            for (;;) {
                if (k + KC < K) mlp_load_chunk<NB, VEC>(W, rowoff, K, k + KC, lh, rb);
                mlp_multiply<NB>(ap + k, ra, acc);
                k += KC;
                if (k >= k1) break;
                if (k + KC < K) mlp_load_chunk<NB, VEC>(W, rowoff, K, k + KC, lh, ra);
                mlp_multiply<NB>(ap + k, rb, acc);
                k += KC;
                if (k >= k1) break;
            }
        } else {
            for (; k < k1; k += KC) {
                mlp_load_chunk<NB, VEC>(W, rowoff, K, k, lh, ra);
                mlp_multiply<NB>(ap + k, ra, acc);
            }
        }
    }
    if (!mul) return;

    const int OS = h.w1 + O;
    GF_GLOBAL float* dst = G(h.out);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int j = (wave + kMlpWaves * b) * 32 + li;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int64_t n = row0 + (rr & 3) + 8 * (rr >> 2) + 4 * lh;
            if (n < N && j < O) dst[n * OS + h.w1 + j] = acc[b][rr];
        }
    }
}

template <int NB>
static void conv_head_launch(const ConvHeadArgs& h, const bool vec, hipStream_t stream) {
    const dim3 grid((unsigned)((h.num_envs + kMlpRows - 1) / kMlpRows)), block(kMlpBlock);
    if (vec) klaunch(conv_head_kernel<NB, true>, grid, block, 0, stream, h);
    else klaunch(conv_head_kernel<NB, false>, grid, block, 0, stream, h);
}

// the LDS bytes of (T, R), the env strides and the table in *p: 0 where R is no band height
static int64_t conv_band_lds(ConvBandPlan* p, const int T, const int R) {
    const int nl = p->layers, hl = p->l[nl - 1].hout;
    p->T = T, p->R = R, p->bands = (hl + R - 1) / R;
    int64_t es[2] = {0, 0};
    for (int b = 0; b < p->bands; ++b) {
        for (int i = 0; i <= nl; ++i) {
            int lo, hi;
            conv_band_range(*p, b, i, lo, hi);
            const int64_t need = i == 0 ? (int64_t)p->l[0].cin * (hi - lo) * p->l[0].win : (int64_t)p->l[i - 1].cout * (hi - lo) * p->l[i - 1].wout;
            es[i & 1] = need > es[i & 1] ? need : es[i & 1];
        }
    }
    es[0] |= 1, es[1] |= 1;
    const int64_t bytes = 4 * ((int64_t)p->tab + kConvRowWords) + 4 * T * (es[0] + es[1]);
    if (bytes <= GF_CONV_LDS_BYTES) p->es[0] = (int)es[0], p->es[1] = (int)es[1], p->lds_bytes = (int)bytes;
    return bytes;
}

// gf_conv_encode_banded's shape refusals and its (T, R) (no pointer is looked at): GF_OK and the plan
static int conv_banded_plan(const GfConvBandedArgs& ba, ConvBandPlan* p) {
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
    int c = a.channels, h = a.height, w = a.width, tab = 0;
    if (a.image_stride && a.image_stride < (int64_t)c * h * w) return GF_E_RANGE;
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
    }
    const int64_t flat = (int64_t)c * h * w;
    if (flat > 0x7fffffff / GF_CONV_MAX_LATENT) return GF_E_RANGE;   // (the head's row offsets are 32 bits)
    p->layers = a.num_layers;
    p->flat = (int)flat;
    p->tab = tab;
    p->w1 = (int)w1;
    p->head_nb = (((a.latent_dim + 31) >> 5) + kMlpWaves - 1) / kMlpWaves;
    if (ba.band_rows < 0 || ba.band_rows > h || ba.tile_envs < 0 || ba.tile_envs > GF_CONV_MAX_TILE_ENVS) return GF_E_RANGE;
    // R: the forced one, else the tallest band that fits T (the forced one, else one env)
    int R = ba.band_rows ? ba.band_rows : h;
    const int tmin = ba.tile_envs ? ba.tile_envs : 1;
    while (conv_band_lds(p, tmin, R) > GF_CONV_LDS_BYTES) {
        if (ba.band_rows || R == 1) return GF_E_RANGE;   // a forced value, or a one-row band of one env, that does not fit
        --R;
    }
    if (!ba.tile_envs) {   // T: the most that fit beside the table
        const int64_t fixed = 4 * ((int64_t)tab + kConvRowWords), per_env = 4 * ((int64_t)p->es[0] + p->es[1]);
        const int64_t T = (GF_CONV_LDS_BYTES - fixed) / per_env;
        conv_band_lds(p, T > GF_CONV_MAX_TILE_ENVS ? GF_CONV_MAX_TILE_ENVS : (int)T, R);
    }
    return GF_OK;
}

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_conv_encode_banded_sizeof(void) { return (int)sizeof(GfConvBandedArgs); }

extern "C" __attribute__((visibility("default"))) int gf_conv_banded_plan(const GfConvBandedArgs* a, int* tile_envs_out, int* band_rows_out, int* num_bands_out,
                                                                           int* lds_bytes_out, int* flat_out) {
    if (!a) return GF_E_NULL;
    gf::ConvBandPlan p;
    const int rc = gf::conv_banded_plan(*a, &p);
    if (rc != GF_OK) return rc;
    if (tile_envs_out) *tile_envs_out = p.T;
    if (band_rows_out) *band_rows_out = p.R;
    if (num_bands_out) *num_bands_out = p.bands;
    if (lds_bytes_out) *lds_bytes_out = p.lds_bytes;
    if (flat_out) *flat_out = p.flat;
    return GF_OK;
}

extern "C" __attribute__((visibility("default"))) int gf_conv_encode_banded(const GfConvBandedArgs* ba, void* stream) {
    (void)&gf::mlp_distill_check, (void)&gf::rnn_check_cell, (void)&gf::mlp_tiles, (void)&gf::mlp_vec_rows;   // (gf_mlp.hip's host helpers: not this entry's)
    if (!ba) return GF_E_NULL;
    gf::ConvBandPlan p;
    const int rc = gf::conv_banded_plan(*ba, &p);
    if (rc != GF_OK) return rc;
    const GfConvEncodeArgs* a = &ba->enc;
    if (!a->image || !a->out || !ba->feat || !a->head_weight || !a->head_bias || (a->in_mean && !a->in_std)) return GF_E_NULL;
    for (int l = 0; l < a->num_layers; ++l)
        if (!a->layers[l].weight || !a->layers[l].bias) return GF_E_NULL;
    for (int s = 0; s < a->num_inputs; ++s)
        if (!a->inputs[s].rows) return GF_E_NULL;
    if (a->num_envs == 0) return GF_OK;
    const int64_t tiles = (a->num_envs + p.T - 1) / p.T;
    if (tiles > 0x7fffffff) return GF_E_RANGE;
    gf::klaunch(gf::conv_banded_kernel, dim3((unsigned)tiles, (unsigned)p.bands), dim3(gf::kMlpBlock), (size_t)p.lds_bytes, (hipStream_t)stream, *ba, p);
    const gf::ConvHeadArgs h{ba->feat, a->head_weight, a->head_bias, a->out, a->num_envs, p.flat, a->latent_dim, p.w1};
    const bool vec = (p.flat & 3) == 0 && ((reinterpret_cast<uintptr_t>(ba->feat) | reinterpret_cast<uintptr_t>(a->head_weight)) & 15u) == 0;
    if (p.head_nb == 1) gf::conv_head_launch<1>(h, vec, (hipStream_t)stream);
    else if (p.head_nb == 2) gf::conv_head_launch<2>(h, vec, (hipStream_t)stream);
    else if (p.head_nb == 3) gf::conv_head_launch<3>(h, vec, (hipStream_t)stream);
    else gf::conv_head_launch<4>(h, vec, (hipStream_t)stream);
    return gf::launch_status();
}
