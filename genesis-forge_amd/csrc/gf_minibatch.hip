// gf_minibatch.hip — one PPO minibatch of a finished rollout as ONE gather launch (rsl_rl RolloutStorage.mini_batch_generator).
//
// rsl_rl draws one permutation of the T·N transitions per generator call and indexes every flattened [T·N, …] array with a
// slice of it: obs, critic obs, actions, values, advantages, returns, log-prob, mu, sigma — nine index launches per minibatch.
// Here every field of every selected row is copied by one launch:
//   dst_f[i, dst_col_f + c] = src_f[indices[i], c]     (c < src_width_f, i < num_rows)
// Workgroups own tiles of minibatch rows.  A tile's indices are loaded once (coalesced) into LDS and reused for every field;
// an index outside [0, num_src_rows) is never dereferenced: its row is written as quiet NaN in every field.  Within a field the
// lanes cover (row, column chunk) pairs of the tile — 16-byte chunks where the widths, the column offset and both base
// pointers allow it, 8- or 4-byte chunks otherwise — and each lane issues kMbUnits chunk loads before their stores, so several
// rows are in flight per wave.  Pure copy: bit-identical to src[indices].  Default-policy stores: the PPO forward pass reads
// the output next.  Algorithmic traffic: R 4·Σw + 8, W 4·Σw bytes per minibatch row.
// A field with a normaliser (mean != NULL: rsl_rl's EmpiricalNormalization.forward on the gathered observations) stores
// (v - mean[c]) / (std[c] + eps) instead of v, in the same pass: the chunking follows the rows as before, mean and std — [src_width]
// vectors that stay in cache, possibly a less aligned slice of a group's normaliser — are read by element.  NaN rows stay NaN.
// A history field (history_len = H > 1: the source is a frame-major rollout storage, gf_step.h) rebuilds the [H·O] row from H frames:
//   dst_f[i, dst_col_f + j·O + c] = src_f[indices[i] + (H-1-j)·N, c]     (j < H, c < O = src_width_f, N = frame_stride_rows_f)
// The lanes cover (row, chunk) pairs over the H·O destination columns; a chunk's frame j is one more magic division, its source
// address the row's plus (H-1-j)·N·O floats — no division by N.  Launches with a history field run kernels of their own
// (minibatch_gather_hist_kernel), so that the plain kernels keep the registers and the occupancy they had.
#include "gf_launch.h"

namespace gf {

constexpr int kMbBlock = 256;
constexpr int kMbMaxTile = 256;   // rows per workgroup at most (the host picks a smaller tile when the minibatch is small)
constexpr int kMbUnits = 4;       // chunks per lane in flight

// per-field launch constants the host derives once: chunk width, chunks per row, and the magic for (item / chunks)
struct MbConsts {
    uint64_t magic[GF_MINIBATCH_MAX_FIELDS];   // ceil(2^64 / chunks) (chunks >= 2): e / chunks = umulhi64(e, magic) for e·chunks < 2^64
    int32_t chunks[GF_MINIBATCH_MAX_FIELDS];
    int32_t vec[GF_MINIBATCH_MAX_FIELDS];      // floats per chunk: 4, 2 or 1
    int32_t tile;                              // rows per workgroup
    int32_t _pad;
};

typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int V> struct MbVec;
template <> struct MbVec<4> { typedef f32x4 T; };
template <> struct MbVec<2> { typedef f32x2 T; };
template <> struct MbVec<1> { typedef float T; };

// the normalised chunk at source columns c0 … c0 + V - 1: one subtraction, one addition, one correctly rounded division per element
template <int V>
__device__ __forceinline__ typename MbVec<V>::T mb_normalise(typename MbVec<V>::T v, const GF_GLOBAL float* mean, const GF_GLOBAL float* sd,
                                                             const float eps, const int64_t c0) {
    if constexpr (V == 1) {
        return (v - mean[c0]) / (sd[c0] + eps);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = (v[j] - mean[c0 + j]) / (sd[c0 + j] + eps);
        return v;
    }
}

template <int V, bool NORM>
__device__ __forceinline__ void mb_copy_field(const GfMinibatchField& f, const int64_t* __restrict__ tile_idx, const int64_t row0,
                                              const int rows, const int chunks, const uint64_t magic) {
    typedef typename MbVec<V>::T VT;
    const int64_t items = (int64_t)rows * chunks;
    const int64_t sw = f.src_width, dw = f.dst_width;
    const GF_GLOBAL float* src = G(f.src);
    GF_GLOBAL float* dst = G(f.dst) + row0 * dw + f.dst_col;
    for (int64_t base = threadIdx.x; base < items; base += (int64_t)kMbBlock * kMbUnits) {
        VT v[kMbUnits];
        int64_t at[kMbUnits];
#pragma unroll
        for (int k = 0; k < kMbUnits; ++k) {
            const int64_t it = base + (int64_t)k * kMbBlock;
            at[k] = -1;
            if (it < items) {
                const int64_t r = chunks == 1 ? it : (int64_t)__umul64hi((uint64_t)it, magic);
                const int64_t c = it - r * chunks;
                const int64_t s = tile_idx[r];
                at[k] = r * dw + c * V;
                if (s >= 0) {
                    v[k] = *reinterpret_cast<const GF_GLOBAL VT*>(src + s * sw + c * V);
                    if (NORM) v[k] = mb_normalise<V>(v[k], G(f.mean), G(f.std), f.eps, c * V);
                } else v[k] = (VT)__builtin_nanf("");   // (a scalar cast to an ext-vector splats)
            }
        }
#pragma unroll
        for (int k = 0; k < kMbUnits; ++k)
            if (at[k] >= 0) *reinterpret_cast<GF_GLOBAL VT*>(dst + at[k]) = v[k];
    }
}

// per-field constants of a launch with history fields: chunks per frame and the magic for (chunk / chunks per frame)
struct MbHistConsts {
    uint64_t magic[GF_MINIBATCH_MAX_FIELDS];   // ceil(2^64 / fchunks) (fchunks >= 2)
    int32_t fchunks[GF_MINIBATCH_MAX_FIELDS];  // chunks per frame: src_width / vec (a plain field: its chunks per row)
};

// a field of H = max(history_len, 1) frames per row (H = 1: the plain copy — every chunk is of frame 0, at the row itself)
template <int V, bool NORM>
__device__ __forceinline__ void mb_copy_history(const GfMinibatchField& f, const int64_t* __restrict__ tile_idx, const int64_t row0,
                                                const int rows, const int chunks, const uint64_t magic, const int fchunks, const uint64_t fmagic) {
    typedef typename MbVec<V>::T VT;
    const int64_t items = (int64_t)rows * chunks;
    const int64_t sw = f.src_width, dw = f.dst_width;
    const int64_t newest = f.history_len > 1 ? f.history_len - 1 : 0;
    const int64_t fstride = f.history_len > 1 ? (int64_t)f.frame_stride_rows * sw : 0;   // floats from a frame to the next newer one
    const GF_GLOBAL float* src = G(f.src);
    GF_GLOBAL float* dst = G(f.dst) + row0 * dw + f.dst_col;
    for (int64_t base = threadIdx.x; base < items; base += (int64_t)kMbBlock * kMbUnits) {
        VT v[kMbUnits];
        int64_t at[kMbUnits];
#pragma unroll
        for (int k = 0; k < kMbUnits; ++k) {
            const int64_t it = base + (int64_t)k * kMbBlock;
            at[k] = -1;
            if (it < items) {
                const int64_t r = chunks == 1 ? it : (int64_t)__umul64hi((uint64_t)it, magic);
                const int64_t c = it - r * chunks;                                                   // chunk of the H·O columns
                const int64_t j = fchunks == 1 ? c : (int64_t)__umul64hi((uint64_t)c, fmagic);       // its frame, newest first
                const int64_t s = tile_idx[r];
                at[k] = r * dw + c * V;
                if (s >= 0) {
                    v[k] = *reinterpret_cast<const GF_GLOBAL VT*>(src + s * sw + (newest - j) * fstride + (c - j * fchunks) * V);
                    if (NORM) v[k] = mb_normalise<V>(v[k], G(f.mean), G(f.std), f.eps, c * V);
                } else v[k] = (VT)__builtin_nanf("");
            }
        }
#pragma unroll
        for (int k = 0; k < kMbUnits; ++k)
            if (at[k] >= 0) *reinterpret_cast<GF_GLOBAL VT*>(dst + at[k]) = v[k];
    }
}

// NORM: some field carries a normaliser.  A kernel of its own, so that the pure copy keeps the registers (and the occupancy) it had.
template <bool NORM>
__global__ __launch_bounds__(kMbBlock) void minibatch_gather_kernel(const GfMinibatchArgs a, const MbConsts mc) {
    __shared__ int64_t tile_idx[kMbMaxTile];
    const int64_t row0 = (int64_t)blockIdx.x * mc.tile;
    const int64_t left = a.num_rows - row0;
    const int rows = left < mc.tile ? (int)left : mc.tile;
    if ((int)threadIdx.x < rows) {
        const int64_t s = G(a.indices)[row0 + threadIdx.x];
        tile_idx[threadIdx.x] = (s >= 0 && s < a.num_src_rows) ? s : -1;   // out of range: NaN row, no load
    }
    __syncthreads();
    for (int f = 0; f < a.num_fields; ++f) {
        const int v = mc.vec[f];
        if (NORM && a.fields[f].mean) {
            if (v == 4) mb_copy_field<4, true>(a.fields[f], tile_idx, row0, rows, mc.chunks[f], mc.magic[f]);
            else if (v == 2) mb_copy_field<2, true>(a.fields[f], tile_idx, row0, rows, mc.chunks[f], mc.magic[f]);
            else mb_copy_field<1, true>(a.fields[f], tile_idx, row0, rows, mc.chunks[f], mc.magic[f]);
            continue;
        }
        if (v == 4) mb_copy_field<4, false>(a.fields[f], tile_idx, row0, rows, mc.chunks[f], mc.magic[f]);
        else if (v == 2) mb_copy_field<2, false>(a.fields[f], tile_idx, row0, rows, mc.chunks[f], mc.magic[f]);
        else mb_copy_field<1, false>(a.fields[f], tile_idx, row0, rows, mc.chunks[f], mc.magic[f]);
    }
}

// some field is a history field: every field of the launch goes through mb_copy_history (a plain one as a history of one frame)
template <bool NORM>
__global__ __launch_bounds__(kMbBlock) void minibatch_gather_hist_kernel(const GfMinibatchArgs a, const MbConsts mc, const MbHistConsts hc) {
    __shared__ int64_t tile_idx[kMbMaxTile];
    const int64_t row0 = (int64_t)blockIdx.x * mc.tile;
    const int64_t left = a.num_rows - row0;
    const int rows = left < mc.tile ? (int)left : mc.tile;
    if ((int)threadIdx.x < rows) {
        const int64_t s = G(a.indices)[row0 + threadIdx.x];
        tile_idx[threadIdx.x] = (s >= 0 && s < a.num_src_rows) ? s : -1;   // out of range: NaN row, no load
    }
    __syncthreads();
    for (int f = 0; f < a.num_fields; ++f) {
        const int v = mc.vec[f];
        if (NORM && a.fields[f].mean) {
            if (v == 4) mb_copy_history<4, true>(a.fields[f], tile_idx, row0, rows, mc.chunks[f], mc.magic[f], hc.fchunks[f], hc.magic[f]);
            else if (v == 2) mb_copy_history<2, true>(a.fields[f], tile_idx, row0, rows, mc.chunks[f], mc.magic[f], hc.fchunks[f], hc.magic[f]);
            else mb_copy_history<1, true>(a.fields[f], tile_idx, row0, rows, mc.chunks[f], mc.magic[f], hc.fchunks[f], hc.magic[f]);
            continue;
        }
        if (v == 4) mb_copy_history<4, false>(a.fields[f], tile_idx, row0, rows, mc.chunks[f], mc.magic[f], hc.fchunks[f], hc.magic[f]);
        else if (v == 2) mb_copy_history<2, false>(a.fields[f], tile_idx, row0, rows, mc.chunks[f], mc.magic[f], hc.fchunks[f], hc.magic[f]);
        else mb_copy_history<1, false>(a.fields[f], tile_idx, row0, rows, mc.chunks[f], mc.magic[f], hc.fchunks[f], hc.magic[f]);
    }
}

int minibatch_prep(const GfMinibatchArgs* a) {
    if (!a) return GF_E_NULL;
    if (a->num_fields < 1 || a->num_fields > GF_MINIBATCH_MAX_FIELDS || a->num_rows < 0 || a->num_src_rows < 1) return GF_E_RANGE;
    if (!a->indices) return GF_E_NULL;
    for (int f = 0; f < a->num_fields; ++f) {
        const GfMinibatchField& d = a->fields[f];
        if (!d.src || !d.dst || (d.mean && !d.std)) return GF_E_NULL;
        if (d.src_width < 1 || d.dst_width < 1 || d.dst_col < 0 || d.history_len < 0) return GF_E_RANGE;
        if (d.history_len > 1 && d.frame_stride_rows < 1) return GF_E_RANGE;
        if ((int64_t)d.dst_col + (int64_t)(d.history_len > 1 ? d.history_len : 1) * d.src_width > d.dst_width) return GF_E_RANGE;
    }
    return GF_OK;
}

// widest chunk (floats) every row of the field can be moved in: source rows, destination rows and the column offset aligned to it —
// and, for a history field, every frame's source address: N·O floats from frame to frame
static int field_vec(const GfMinibatchField& d) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(d.src) | reinterpret_cast<uintptr_t>(d.dst);
    int64_t w = d.src_width | d.dst_width | d.dst_col;
    if (d.history_len > 1) w |= (int64_t)d.frame_stride_rows * d.src_width;
    if ((p & 15u) == 0 && (w & 3) == 0) return 4;
    if ((p & 7u) == 0 && (w & 1) == 0) return 2;
    return 1;
}

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_minibatch_gather(const GfMinibatchArgs* a, void* stream) {
    const int rc = gf::minibatch_prep(a);
    if (rc) return rc;
    if (a->num_rows == 0) return GF_OK;
    gf::MbConsts mc{};
    gf::MbHistConsts hc{};
    bool hist = false;
    for (int f = 0; f < a->num_fields; ++f) {
        const int v = gf::field_vec(a->fields[f]);
        const int H = a->fields[f].history_len > 1 ? a->fields[f].history_len : 1;
        const int fchunks = a->fields[f].src_width / v;
        const int64_t chunks = (int64_t)fchunks * H;
        if (chunks > 0x7fffffff) return GF_E_RANGE;
        hist = hist || H > 1;
        mc.vec[f] = v;
        mc.chunks[f] = (int32_t)chunks;
        mc.magic[f] = chunks > 1 ? ~(uint64_t)0 / (uint64_t)chunks + 1 : 0;   // ceil(2^64 / chunks); exact for powers of two too
        hc.fchunks[f] = fchunks;
        hc.magic[f] = fchunks > 1 ? ~(uint64_t)0 / (uint64_t)fchunks + 1 : 0;
    }
    // rows per workgroup: 256, halved while the minibatch would give fewer than ~4 workgroups per CU (the gait task's 24 576-row
    // minibatches of 3 KB rows would otherwise occupy 96 of the 256 CUs), down to 16
    int tile = gf::kMbMaxTile;
    while (tile > 16 && a->num_rows < (int64_t)tile * 1024) tile >>= 1;
    mc.tile = tile;
    const int64_t blocks = (a->num_rows + tile - 1) / tile;
    if (blocks > 0x7fffffff) return GF_E_RANGE;
    hipStream_t s = (hipStream_t)stream;
    bool norm = false;
    for (int f = 0; f < a->num_fields; ++f) norm = norm || a->fields[f].mean != nullptr;
    if (hist && norm) gf::klaunch(gf::minibatch_gather_hist_kernel<true>, dim3((unsigned)blocks), dim3(gf::kMbBlock), 0, s, *a, mc, hc);
    else if (hist) gf::klaunch(gf::minibatch_gather_hist_kernel<false>, dim3((unsigned)blocks), dim3(gf::kMbBlock), 0, s, *a, mc, hc);
    else if (norm) gf::klaunch(gf::minibatch_gather_kernel<true>, dim3((unsigned)blocks), dim3(gf::kMbBlock), 0, s, *a, mc);
    else gf::klaunch(gf::minibatch_gather_kernel<false>, dim3((unsigned)blocks), dim3(gf::kMbBlock), 0, s, *a, mc);
    return gf::launch_status();
}
