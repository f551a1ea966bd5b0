// gf_mirror.hip — mirror symmetry of the PPO update (rsl_rl's symmetry_cfg): the augmented minibatch and the mirror loss.
// include/gf_step.h has the contracts; neither entry point is a phase of the step.
//
// gf_mirror_rows: grid (row tiles, fields + 1).  Workgroup (t, f) stages rows t·tile … of field f in LDS — 16-byte loads, kMirUnits
// of them in flight per lane, every source row read from memory once — then walks the tile's destination chunks: the copy is the
// chunk itself, the mirror gathers its four elements from the row in LDS through perm (a random LDS read costs a bank conflict at
// worst) and multiplies by sign; with a normaliser both go through (v - mean[j]) / (std[j] + eps) at the destination column j.
// tile = min(kMirMaxTileRows, GF_MIRROR_MAX_WIDTH / width) rows: 64 rows of a 48-wide observation, 8 of a 1 024-wide one.  The last
// grid row (y = num_fields) replicates the per-row scalars, 1 024 elements per workgroup.  Algorithmic traffic per row and field:
// R 4·w, W 8·w bytes (4·w without dst_copy); the tables stay in cache.
//
// gf_mirror_loss: one lane per row walks its A columns; the workgroup's sum of d² (double: wave butterfly, then the four waves in
// order) is one record of the workspace, a one-workgroup launch sums the records in a fixed order.  The gradient needs no sum: it is
// added into `grad` by the lane that computed d.  R 8A (+ 4A of grad), W 4A bytes per row.
#include "gf_launch.h"
#include "gf_reduce.h"

namespace gf {

constexpr int kMirBlock = 256;
constexpr int kMirMaxTileRows = 64;
constexpr int kMirUnits = 4;            // chunk loads per lane in flight while staging
constexpr int kMirScalarTile = 1024;    // scalar elements per workgroup (256 lanes x 4)
constexpr int kMirLossBlock = GF_MIRROR_LOSS_BLOCK_ROWS;
constexpr int kMirFinBlock = 256;

typedef int i32x4 __attribute__((ext_vector_type(4)));

// per-field launch constants the host derives once
struct MirConsts {
    uint32_t magic[GF_MIRROR_MAX_FIELDS];   // ceil(2^32 / chunks) (chunks >= 2): it / chunks = umulhi(it, magic) for it·chunks < 2^32
    int32_t chunks[GF_MIRROR_MAX_FIELDS];   // chunks per row
    int32_t vec[GF_MIRROR_MAX_FIELDS];      // floats per chunk: 4 or 1
    int32_t tile[GF_MIRROR_MAX_FIELDS];     // rows per workgroup
};

template <int V> struct MirVec;
template <> struct MirVec<4> { typedef f32x4 T; };
template <> struct MirVec<1> { typedef float T; };

template <int V, bool NORM>
__device__ __forceinline__ void mirror_field(const GfMirrorField& f, const int64_t num_rows, const int tile, const int chunks,
                                             const uint32_t magic, float* __restrict__ s_tile) {
    typedef typename MirVec<V>::T VT;
    const int64_t row0 = (int64_t)blockIdx.x * tile;
    if (row0 >= num_rows) return;   // (block-uniform: this field has fewer tiles than the widest grid row)
    const int64_t left = num_rows - row0;
    const int rows = left < tile ? (int)left : tile;
    const int w = f.width;
    const int64_t stride = f.row_stride ? f.row_stride : w;
    const GF_GLOBAL float* src = G(f.src) + row0 * stride;
    const int items = rows * chunks;   // <= GF_MIRROR_MAX_WIDTH
    // stage: the tile's raw rows, contiguous in LDS
    for (int base = threadIdx.x; base < items; base += kMirBlock * kMirUnits) {
        VT v[kMirUnits];
        int at[kMirUnits];
#pragma unroll
        for (int k = 0; k < kMirUnits; ++k) {
            const int it = base + k * kMirBlock;
            at[k] = -1;
            if (it < items) {
                const int r = chunks == 1 ? it : (int)__umulhi((uint32_t)it, magic);
                const int c = it - r * chunks;
                at[k] = r * w + c * V;
                v[k] = *reinterpret_cast<const GF_GLOBAL VT*>(src + r * stride + c * V);
            }
        }
#pragma unroll
        for (int k = 0; k < kMirUnits; ++k)
            if (at[k] >= 0) *reinterpret_cast<VT*>(s_tile + at[k]) = v[k];
    }
    __syncthreads();
    GF_GLOBAL float* dc = f.dst_copy ? G(f.dst_copy) + row0 * w : nullptr;
    GF_GLOBAL float* dm = G(f.dst_mirror) + row0 * w;
    const GF_GLOBAL int32_t* perm = G(f.perm);
    const GF_GLOBAL float* sign = G(f.sign);
    const GF_GLOBAL float* mean = G(f.in_mean);
    const GF_GLOBAL float* sd = G(f.in_std);
    const float eps = f.in_eps;
    for (int it = threadIdx.x; it < items; it += kMirBlock) {
        const int r = chunks == 1 ? it : (int)__umulhi((uint32_t)it, magic);
        const int j0 = (it - r * chunks) * V;
        const float* row = s_tile + r * w;
        float cp[V], mi[V];
        int pm[V];
        float sg[V];
        if constexpr (V == 4) {
            const i32x4 p4 = *reinterpret_cast<const GF_GLOBAL i32x4*>(perm + j0);
            const f32x4 s4 = *reinterpret_cast<const GF_GLOBAL f32x4*>(sign + j0);
            pm[0] = p4.x; pm[1] = p4.y; pm[2] = p4.z; pm[3] = p4.w;
            sg[0] = s4.x; sg[1] = s4.y; sg[2] = s4.z; sg[3] = s4.w;
        } else {
            pm[0] = perm[j0];
            sg[0] = sign[j0];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            cp[k] = row[j0 + k];
            mi[k] = sg[k] * row[pm[k]];
            if (NORM) {   // one subtraction, one addition, one correctly rounded division: gf_minibatch_gather's mb_normalise
                const float m = mean[j0 + k], d = sd[j0 + k] + eps;
                cp[k] = (cp[k] - m) / d;
                mi[k] = (mi[k] - m) / d;
            }
        }
        const int at = r * w + j0;
        if constexpr (V == 4) {
            if (dc) *reinterpret_cast<GF_GLOBAL f32x4*>(dc + at) = f32x4{cp[0], cp[1], cp[2], cp[3]};
            *reinterpret_cast<GF_GLOBAL f32x4*>(dm + at) = f32x4{mi[0], mi[1], mi[2], mi[3]};
        } else {
            if (dc) dc[at] = cp[0];
            dm[at] = mi[0];
        }
    }
}

__global__ __launch_bounds__(kMirBlock) void mirror_rows_kernel(const GfMirrorRowsArgs a, const MirConsts mc) {
    __shared__ __attribute__((aligned(16))) float s_tile[GF_MIRROR_MAX_WIDTH];
    const int f = blockIdx.y;
    if (f < a.num_fields) {
        const GfMirrorField& d = a.fields[f];
        if (d.in_mean) {
            if (mc.vec[f] == 4) mirror_field<4, true>(d, a.num_rows, mc.tile[f], mc.chunks[f], mc.magic[f], s_tile);
            else mirror_field<1, true>(d, a.num_rows, mc.tile[f], mc.chunks[f], mc.magic[f], s_tile);
        } else {
            if (mc.vec[f] == 4) mirror_field<4, false>(d, a.num_rows, mc.tile[f], mc.chunks[f], mc.magic[f], s_tile);
            else mirror_field<1, false>(d, a.num_rows, mc.tile[f], mc.chunks[f], mc.magic[f], s_tile);
        }
        return;
    }
    // the per-row scalars: dst[i] = dst[rows + i] = src[i]
    const int64_t n = a.num_rows;
    const int64_t e0 = (int64_t)blockIdx.x * kMirScalarTile;
    for (int s = 0; s < a.num_scalars; ++s) {
        const GF_GLOBAL float* src = G(a.scalars[s].src);
        GF_GLOBAL float* dst = G(a.scalars[s].dst);
#pragma unroll
        for (int k = 0; k < kMirScalarTile / kMirBlock; ++k) {
            const int64_t i = e0 + k * kMirBlock + threadIdx.x;
            if (i < n) {
                const float v = src[i];
                dst[i] = v;
                dst[n + i] = v;
            }
        }
    }
}

static_assert(kMirLossBlock == kSumBlock, "block_wave_sums folds four waves");

__global__ __launch_bounds__(kMirLossBlock) void mirror_loss_rows_kernel(const GfMirrorLossArgs a) {
    __shared__ double s_w[kMirLossBlock / GF_WAVE];
    const int64_t mb = a.num_rows;
    const int64_t i = (int64_t)blockIdx.x * kMirLossBlock + threadIdx.x;
    const int A = a.num_actions;
    double acc = 0.0;
    if (i < mb) {
        const GF_GLOBAL float* mm = G(a.mu_mirror) + i * A;
        const GF_GLOBAL float* mo = G(a.mu_orig) + i * A;
        const GF_GLOBAL int32_t* perm = G(a.perm);
        const GF_GLOBAL float* sign = G(a.sign);
        GF_GLOBAL float* g = a.grad && a.coeff != 0.0f ? G(a.grad) + i * A : nullptr;   // (coeff 0: the buffer keeps its bits, a -0 included)
        const float inv = 1.0f / (float)(mb * A);   // mean's backward: grad / numel
        const float scale = a.coeff * inv;
        for (int j = 0; j < A; ++j) {
            const float d = mm[j] - sign[j] * mo[perm[j]];
            acc += (double)d * (double)d;
            if (g) g[j] = g[j] + scale * (2.0f * d);   // pow(2)'s backward: 2·d
        }
    }
    block_wave_sums(acc, s_w);
    if (threadIdx.x == 0) G(reinterpret_cast<double*>(a.workspace))[blockIdx.x] = fold_wave_sums(s_w);
}

__global__ __launch_bounds__(kMirFinBlock) void mirror_loss_finalize_kernel(const GfMirrorLossArgs a, const int64_t nb) {
    finalize_mean_loss<kMirFinBlock>(a.workspace, nb, a.num_rows, a.num_actions, a.out, a.sums);   // sums: mean_symmetry_loss
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_mirror_rows(const GfMirrorRowsArgs* a, void* stream) {
    if (!a) return GF_E_NULL;
    if (a->num_rows < 0 || a->num_fields < 0 || a->num_fields > GF_MIRROR_MAX_FIELDS || a->num_scalars < 0 ||
        a->num_scalars > GF_MIRROR_MAX_SCALARS || a->num_fields + a->num_scalars == 0)
        return GF_E_RANGE;
    for (int f = 0; f < a->num_fields; ++f) {
        const GfMirrorField& d = a->fields[f];
        if (!d.src || !d.dst_mirror || !d.perm || !d.sign || (d.in_mean && !d.in_std)) return GF_E_NULL;
        if (d.width < 1 || d.width > GF_MIRROR_MAX_WIDTH || d.row_stride < 0 || (d.row_stride != 0 && d.row_stride < d.width)) return GF_E_RANGE;
    }
    for (int s = 0; s < a->num_scalars; ++s)
        if (!a->scalars[s].src || !a->scalars[s].dst) return GF_E_NULL;
    if (a->num_rows == 0) return GF_OK;
    gf::MirConsts mc{};
    int64_t gx = a->num_scalars ? (a->num_rows + gf::kMirScalarTile - 1) / gf::kMirScalarTile : 1;
    for (int f = 0; f < a->num_fields; ++f) {
        const GfMirrorField& d = a->fields[f];
        const bool vec = (d.width & 3) == 0 && (d.row_stride & 3) == 0 && gf::aligned16(d.src) && gf::aligned16(d.dst_copy) &&
                         gf::aligned16(d.dst_mirror) && gf::aligned16(d.perm) && gf::aligned16(d.sign);
        const int v = vec ? 4 : 1;
        const int chunks = d.width / v;
        int tile = GF_MIRROR_MAX_WIDTH / d.width;
        if (tile > gf::kMirMaxTileRows) tile = gf::kMirMaxTileRows;
        mc.vec[f] = v;
        mc.chunks[f] = chunks;
        mc.tile[f] = tile;
        mc.magic[f] = chunks > 1 ? (uint32_t)(0xffffffffu / (uint32_t)chunks + 1u) : 0u;   // ceil(2^32 / chunks); exact for powers of two too
        const int64_t tiles = (a->num_rows + tile - 1) / tile;
        if (tiles > gx) gx = tiles;
    }
    if (gx > 0x7fffffff) return GF_E_RANGE;
    gf::klaunch(gf::mirror_rows_kernel, dim3((unsigned)gx, (unsigned)(a->num_fields + (a->num_scalars ? 1 : 0))), dim3(gf::kMirBlock), 0,
                (hipStream_t)stream, *a, mc);
    return gf::launch_status();
}

extern "C" __attribute__((visibility("default"))) int gf_mirror_loss(const GfMirrorLossArgs* a, void* stream) {
    if (!a || !a->mu_mirror || !a->mu_orig || !a->perm || !a->sign || !a->out || !a->workspace) return GF_E_NULL;
    if (a->num_rows < 0 || a->num_actions < 1) return GF_E_RANGE;
    if (a->num_rows == 0) return GF_OK;
    const int64_t nb = (a->num_rows + gf::kMirLossBlock - 1) / gf::kMirLossBlock;
    if (nb > 0x7fffffff) return GF_E_RANGE;
    if (a->workspace_bytes < GF_MIRROR_LOSS_WORKSPACE_BYTES(a->num_rows) || (reinterpret_cast<uintptr_t>(a->workspace) & 7u)) return GF_E_RANGE;
    hipStream_t s = (hipStream_t)stream;
    gf::klaunch(gf::mirror_loss_rows_kernel, dim3((unsigned)nb), dim3(gf::kMirLossBlock), 0, s, *a);
    gf::klaunch(gf::mirror_loss_finalize_kernel, dim3(1), dim3(gf::kMirFinBlock), 0, s, *a, nb);
    return gf::launch_status();
}
