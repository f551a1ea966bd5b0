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

namespace gf {

constexpr int kRcBlock = 256;
constexpr int kRcEnvs = GF_RAY_CAST_TILE_ENVS;
constexpr int kRcFrame = 12;   // floats per env in LDS: bx, by, bz, r00 | r01, r02, r10, r11 | r12, r20, r21, r22 (three 16-byte reads)

struct RcGrid {   // workgroup-uniform
    const GF_GLOBAL float* f;
    int W, H;
    float x_min, y_min, sx, sy, fw, fh, tmax, origin_z;
};

// the walk of include/gf_step.h; returns hit, t* in `t`
__device__ __forceinline__ bool rc_walk(const RcGrid& g, float ox, float oy, float oz, float dx, float dy, float dz, float& t) {
    const float inf = __builtin_huge_valf();
    const float gx0 = (ox - g.x_min) * g.sx, gy0 = (oy - g.y_min) * g.sy;
    const float du = dx * g.sx, dv = dy * g.sy;
    const float idu = 1.0f / du, idv = 1.0f / dv;
    float t0 = 0.0f, t1 = g.tmax;
    bool ok = true;
    if (du != 0.0f) {
        const float ta = (-gx0) * idu, tb = (g.fw - gx0) * idu;
        const float lo = ta < tb ? ta : tb, hi = ta < tb ? tb : ta;
        if (lo > t0) t0 = lo;
        if (hi < t1) t1 = hi;
    } else {
        ok = gx0 >= 0.0f && gx0 <= g.fw;
    }
    if (dv != 0.0f) {
        const float ta = (-gy0) * idv, tb = (g.fh - gy0) * idv;
        const float lo = ta < tb ? ta : tb, hi = ta < tb ? tb : ta;
        if (lo > t0) t0 = lo;
        if (hi < t1) t1 = hi;
    } else {
        ok = ok && gy0 >= 0.0f && gy0 <= g.fh;
    }
    if (!(ok && t0 <= t1)) return false;
    float tin = t0;
    const int W = g.W, H = g.H;
    int ix, iy;
    {
        const float gin = gx0 + tin * du, fl = floorf(gin);
        ix = (int)fl - ((du < 0.0f && gin == fl) ? 1 : 0);
        ix = ix < 0 ? 0 : (ix > W - 2 ? W - 2 : ix);
    }
    {
        const float gin = gy0 + tin * dv, fl = floorf(gin);
        iy = (int)fl - ((dv < 0.0f && gin == fl) ? 1 : 0);
        iy = iy < 0 ? 0 : (iy > H - 2 ? H - 2 : iy);
    }
    const int sgx = du > 0.0f ? 1 : -1, sgy = dv > 0.0f ? 1 : -1;
    const int fx = du > 0.0f ? 1 : 0, fy = dv > 0.0f ? 1 : 0;
    const int cells = (W - 1) + (H - 1) + 1;
    for (int it = 0; it < cells; ++it) {
        const float tnx = du != 0.0f ? ((float)(ix + fx) - gx0) * idu : inf;
        const float tny = dv != 0.0f ? ((float)(iy + fy) - gy0) * idv : inf;
        const float tn = tnx < tny ? tnx : tny;
        float tout = tn < t1 ? tn : t1;
        tout = tout > tin ? tout : tin;
        const float smax = tout - tin;
        float u0 = (gx0 + tin * du) - (float)ix;
        float v0 = (gy0 + tin * dv) - (float)iy;
        u0 = u0 < 0.0f ? 0.0f : u0;
        u0 = u0 > 1.0f ? 1.0f : u0;
        v0 = v0 < 0.0f ? 0.0f : v0;
        v0 = v0 > 1.0f ? 1.0f : v0;
        const float zin = oz + tin * dz;
        const GF_GLOBAL float* row = g.f + iy * W + ix;   // 0 <= ix <= W-2, 0 <= iy <= H-2: all four taps inside the field
        const float h00 = row[0], h10 = row[1], h01 = row[W], h11 = row[W + 1];
        const float a = h10 - h00, b = h01 - h00;
        const float k = (h00 - h10) - (h01 - h11);
        const float C = zin - (((h00 + a * u0) + b * v0) + (k * u0) * v0);
        if (C <= 0.0f) {
            t = tin;
            return true;
        }
        const float B = dz - ((a * du + b * dv) + k * (u0 * dv + v0 * du));
        const float A = -((k * du) * dv);
        float s = inf;
        if (A == 0.0f) {
            if (B < 0.0f) s = C / (-B);
        } else {
            const float disc = B * B - (4.0f * A) * C;
            if (disc >= 0.0f) {
                const float sq = sqrtf(disc);
                const float q = -0.5f * (B + (B < 0.0f ? -sq : sq));
                const float r1 = q / A, r2 = C / q;
                if (r1 >= 0.0f && r1 < s) s = r1;
                if (r2 >= 0.0f && r2 < s) s = r2;
            }
        }
        if (s <= smax) {
            t = tin + s;
            return true;
        }
        if (!(tn < t1)) return false;
        if (tnx <= tn) ix += sgx;
        if (tny <= tn) iy += sgy;
        if (ix < 0 || ix > W - 2 || iy < 0 || iy > H - 2) return false;
        tin = tout;
    }
    return false;
}

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
        float fr[kRcFrame] = {0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};   // (an env past the end: nobody stores from it)
        if (tid < rows) {
            const GF_GLOBAL float* b = G(a.pos) + (n0 + tid) * a.pos_stride;
            fr[0] = b[0];
            fr[1] = b[1];
            fr[2] = b[2];
            if (a.align != GF_RAY_ALIGN_WORLD) {
                const GF_GLOBAL float* q = G(a.quat) + (n0 + tid) * a.quat_stride;
                const float qw = q[0], qx = q[1], qy = q[2], qz = q[3];
                const float c = 1.0f - 2.0f * (qy * qy + qz * qz);
                const float s = 2.0f * (qw * qz + qx * qy);
                if (a.align == GF_RAY_ALIGN_YAW) {
                    const float nrm = sqrtf(c * c + s * s);
                    const bool flat = nrm < 1e-6f;
                    const float cy = flat ? 1.0f : c / nrm;
                    const float sy = flat ? 0.0f : s / nrm;
                    fr[3] = cy; fr[4] = -sy; fr[6] = sy; fr[7] = cy;
                } else {
                    fr[3] = c;
                    fr[4] = 2.0f * (qx * qy - qw * qz);
                    fr[5] = 2.0f * (qx * qz + qw * qy);
                    fr[6] = s;
                    fr[7] = 1.0f - 2.0f * (qx * qx + qz * qz);
                    fr[8] = 2.0f * (qy * qz - qw * qx);
                    fr[9] = 2.0f * (qx * qz - qw * qy);
                    fr[10] = 2.0f * (qy * qz + qw * qx);
                    fr[11] = 1.0f - 2.0f * (qx * qx + qy * qy);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < kRcFrame; ++i) s_frame[tid * kRcFrame + i] = fr[i];
    }
    __syncthreads();

    RcGrid g;
    g.f = G(a.terrain.height_field);
    g.W = a.terrain.cols;
    g.H = a.terrain.rows;
    g.x_min = a.terrain.x_min;
    g.y_min = a.terrain.y_min;
    g.fw = (float)(g.W - 1);
    g.fh = (float)(g.H - 1);
    g.sx = FIELD ? g.fw / a.terrain.x_span : 0.0f;
    g.sy = FIELD ? g.fh / a.terrain.y_span : 0.0f;
    g.tmax = a.max_range;
    g.origin_z = a.terrain.origin_z;
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
            const float2 p01 = *reinterpret_cast<const float2*>(s_pat + 6 * ps);
            const float2 p23 = *reinterpret_cast<const float2*>(s_pat + 6 * ps + 2);
            const float2 p45 = *reinterpret_cast<const float2*>(s_pat + 6 * ps + 4);
            const float px = p01.x, py = p01.y, pz = p23.x, ex = p23.y, ey = p45.x, ez = p45.y;
            const float4 f0 = *reinterpret_cast<const float4*>(s_frame + es * kRcFrame);       // bx, by, bz, r00
            const float4 f1 = *reinterpret_cast<const float4*>(s_frame + es * kRcFrame + 4);   // r01, r02, r10, r11
            const float4 f2 = *reinterpret_cast<const float4*>(s_frame + es * kRcFrame + 8);   // r12, r20, r21, r22
            const float ox = f0.x + ((f0.w * px + f1.x * py) + f1.y * pz);
            const float oy = f0.y + ((f1.z * px + f1.w * py) + f2.x * pz);
            const float oz = f0.z + ((f2.y * px + f2.z * py) + f2.w * pz);
            const float dx = (f0.w * ex + f1.x * ey) + f1.y * ez;
            const float dy = (f1.z * ex + f1.w * ey) + f2.x * ez;
            const float dz = (f2.y * ex + f2.z * ey) + f2.w * ez;
            float t = 0.0f;
            bool hit;
            if constexpr (FIELD) {
                hit = live && rc_walk(g, ox, oy, oz, dx, dy, dz, t);
            } else {
                const float C = oz - g.origin_z;
                const float tt = C / (-dz);
                const bool under = C <= 0.0f;
                hit = under || (dz < 0.0f && tt <= g.tmax);
                t = under ? 0.0f : tt;
            }
            const float val = depth ? t * ((ex * ax + ey * ay) + ez * az) : t;
            r[j] = hit ? val : miss;
            off[j] = (int64_t)es * a.out_stride + ps;
            if (HITS && live) {
                const float te = hit ? t : g.tmax;
                GF_GLOBAL float* h = hits + 3 * (int64_t)(f + j);
                h[0] = ox + te * dx;
                h[1] = oy + te * dy;
                h[2] = oz + te * dz;
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
