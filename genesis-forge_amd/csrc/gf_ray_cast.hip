// gf_ray_cast.hip — gf_ray_cast: R rays per env against the terrain surface (managers/ray_caster.py), one launch.
// include/gf_step.h has the contract and the float32 operation sequence; this file follows it line by line.
//
// Composed from torch ops the cell walk is a data-dependent loop: every iteration a round of masked tensor ops over [N, R], hundreds
// of launches per cast.  Here a 256-lane workgroup owns a tile of kRcEnvs envs.  It stages the tile's frames (origin and nine matrix
// entries: the quaternion arithmetic happens once per env, in the tile's first kRcEnvs lanes) and the pattern ([R, 6], shared by every
// env) in LDS, then walks the tile's rows·R elements in flat order, consecutive lanes on consecutive rays — neighbouring pixels walk
// neighbouring cells, so a wave's taps fall into the same lines.  V = 4 elements per lane and pass where a 16-byte store is possible
// (the height scan's rule), V = 1 otherwise.  A ray is clipped to the field's rectangle (slab test in grid coordinates), then walks the
// cells it crosses (Amanatides–Woo, every crossing computed from the ray's origin, so nothing drifts); inside a cell the gap between ray
// and bilinear patch is a quadratic in the ray parameter, solved in the cancellation-free form — the square root and the two root
// divisions only where the discriminant admits a root.  The four taps are plain loads of a field every env shares (tens of KB: L1 /
// L2).  Lanes of a wave finish at different cells; a wave waits for its longest ray.  The walk is bounded by (cols-1) + (rows-1) + 1
// cells and every index is clamped before it is used, so no input, a NaN included, reads outside the field.
// Traffic: 4·R bytes out per env (+ 12·R with hits_out), 12 or 28 bytes in.
#include "gf_launch.h"
#include "gf_ray_walk.h"

namespace gf {

constexpr int kRcBlock = 256;
constexpr int kRcEnvs = GF_RAY_CAST_TILE_ENVS;

template <int V, bool HITS, bool FIELD>
__global__ __launch_bounds__(kRcBlock) void ray_cast_kernel(const GfRayCastArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_rc[];
    float* s_frame = s_rc;                        // [kRcEnvs, kRcFrame]
    float* s_pat = s_rc + kRcEnvs * kRcFrame;     // [R, 6]
    const int tid = (int)threadIdx.x;
    const int R = a.num_rays;
    const int64_t n0 = (int64_t)blockIdx.x * kRcEnvs;
    const int64_t left = a.num_envs - n0;
    const int rows = left < kRcEnvs ? (int)left : kRcEnvs;

    const GF_GLOBAL float* pat = G(a.pattern);
    for (int i = tid; i < 6 * R; i += kRcBlock) s_pat[i] = pat[i];
    if (tid < kRcEnvs) {
        rc_frame(s_frame + tid * kRcFrame, G(a.pos) + (n0 + tid) * a.pos_stride, G(a.quat) + (n0 + tid) * a.quat_stride, a.align, tid < rows);
    }
    __syncthreads();

    const RcGrid g = rc_grid<FIELD>(a.terrain, a.max_range);
    const bool depth = a.mode == GF_RAY_MODE_DEPTH;
    const float ax = a.axis[0], ay = a.axis[1], az = a.axis[2];
    const float miss = a.miss_value;

    const int total = rows * R;
    constexpr int kPass = V * kRcBlock;                // elements of one pass of the workgroup
    const int de = kPass / R, dp = kPass - de * R;     // workgroup-uniform
    int e = (V * tid) / R, p = V * tid - e * R;        // the lane's one division
    GF_GLOBAL float* out = G(a.out) + n0 * a.out_stride;
    GF_GLOBAL float* hits = HITS ? G(a.hits_out) + 3 * (n0 * R) : nullptr;

    for (int f = V * tid; f - V * tid < total; f += kPass) {   // (the bound is the pass's first element: uniform)
        float r[V];
        int64_t off[V];
        int ej = e, pj = p;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const bool live = f + j < total;
            const int es = live ? ej : 0, ps = live ? pj : 0;
            const RcRay y = rc_ray(s_frame + es * kRcFrame, s_pat + 6 * ps);
            float t;
            const bool hit = rc_hit<FIELD>(g, y, live, t);
            const float val = depth ? t * ((y.ex * ax + y.ey * ay) + y.ez * az) : t;
            r[j] = hit ? val : miss;
            off[j] = (int64_t)es * a.out_stride + ps;
            if (HITS && live) {
                const float te = hit ? t : g.tmax;
                GF_GLOBAL float* h = hits + 3 * (int64_t)(f + j);
                h[0] = y.ox + te * y.dx;
                h[1] = y.oy + te * y.dy;
                h[2] = y.oz + te * y.dz;
            }
            pj += 1;
            if (pj == R) { pj = 0; ej += 1; }
        }
        bool stored = false;
        if constexpr (V == 4) {
            if (f + 3 < total) {   // four live elements: consecutive addresses, 16-byte aligned (the host chose V = 4 for that)
                f32x4 q;
                q.x = r[0]; q.y = r[1]; q.z = r[2]; q.w = r[3];
                *reinterpret_cast<GF_GLOBAL f32x4*>(out + off[0]) = q;
                stored = true;
            }
        }
        if (!stored) {
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (f + j < total) out[off[j]] = r[j];
        }
        p += dp;
        e += de;
        if (p >= R) { p -= R; e += 1; }
    }
}

template <int V, bool HITS>
static void rc_launch(PhaseScope& scope, const GfRayCastArgs& a, unsigned grid, size_t lds, hipStream_t s) {
    if (a.terrain.height_field) GF_LAUNCH(scope, (ray_cast_kernel<V, HITS, true>), grid, kRcBlock, lds, s, a);
    else GF_LAUNCH(scope, (ray_cast_kernel<V, HITS, false>), grid, kRcBlock, lds, s, a);
}

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_ray_cast_sizeof(void) { return (int)sizeof(GfRayCastArgs); }

extern "C" __attribute__((visibility("default"))) int gf_ray_cast(const GfRayCastArgs* a, void* stream) {
    if (!a || !a->out || !a->pos || !a->pattern) return GF_E_NULL;
    if (a->align != GF_RAY_ALIGN_WORLD && !a->quat) return GF_E_NULL;
    const int64_t tiles = a->num_envs < 0 ? -1 : (a->num_envs + gf::kRcEnvs - 1) / gf::kRcEnvs;
    if (tiles < 0 || tiles > 0x7fffffff) return GF_E_RANGE;
    const int R = a->num_rays;
    if (R < 1 || R > GF_RAY_CAST_MAX_RAYS) return GF_E_RANGE;
    if (a->pos_stride < 3 || (a->quat && a->quat_stride < 4) || a->out_stride < R) return GF_E_RANGE;
    if (a->align < GF_RAY_ALIGN_WORLD || a->align > GF_RAY_ALIGN_BASE || (a->mode != GF_RAY_MODE_DISTANCE && a->mode != GF_RAY_MODE_DEPTH))
        return GF_E_RANGE;
    if (!(a->max_range >= 0.0f) || a->max_range == __builtin_huge_valf()) return GF_E_RANGE;   // (a NaN fails the first test)
    if (a->terrain.height_field && (a->terrain.rows < 2 || a->terrain.cols < 2)) return GF_E_RANGE;
    if (a->num_envs == 0) return GF_OK;
    // 16-byte stores under the height scan's rule: `out` aligned, and either dense rows (a tile starts a multiple of kRcEnvs·R floats
    // in) or every row aligned and made of whole quads
    static_assert(gf::kRcEnvs % 4 == 0, "a dense tile starts 16-byte aligned");
    const bool vec = !(reinterpret_cast<uintptr_t>(a->out) & 15u) && (a->out_stride == R || (R % 4 == 0 && a->out_stride % 4 == 0));
    hipStream_t s = (hipStream_t)stream;
    gf::PhaseScope scope(GF_PHASE_TERRAIN, s);
    const unsigned grid = (unsigned)tiles;
    const size_t lds = sizeof(float) * (size_t)(gf::kRcEnvs * gf::kRcFrame + 6 * R);
    if (vec && a->hits_out) gf::rc_launch<4, true>(scope, *a, grid, lds, s);
    else if (vec) gf::rc_launch<4, false>(scope, *a, grid, lds, s);
    else if (a->hits_out) gf::rc_launch<1, true>(scope, *a, grid, lds, s);
    else gf::rc_launch<1, false>(scope, *a, grid, lds, s);
    return gf::launch_status();
}
