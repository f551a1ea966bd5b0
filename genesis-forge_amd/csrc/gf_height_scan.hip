// gf_height_scan.hip — gf_height_scan: the terrain height at P points around every env's base (managers/height_scanner.py), the
// pattern turned by the base's yaw, in one launch.  include/gf_step.h has the contract and the arithmetic.
//
// Composed from TerrainManager.get_terrain_height the scan is a broadcast pattern, a dozen elementwise launches for the rotation, one
// gf_terrain_height launch over N·P points that reads two [N·P] temporaries, and a subtraction and a clamp: about ten passes over
// [N, P] tensors for a result that is one [N, P] write.  Here a 256-lane workgroup owns a tile of kHsEnvs envs.  It stages the pattern
// ([P, 2], shared by every env) and the tile's frames (bx, by, bz - offset, cy, sy — the quaternion arithmetic, the square root and
// the two divisions happen once per env, in the tile's first kHsEnvs lanes) in LDS, then walks the tile's rows·P elements in flat
// order, consecutive lanes on consecutive p: V = 4 elements per lane and pass where a 16-byte store is possible (`out` aligned and
// either dense — the tile's rows are then ONE contiguous run, whatever P is: 187 too — or made of whole quads), V = 1 otherwise.  A
// lane divides once, for its first element; from pass to pass (e, p) advance by the workgroup-uniform quotient and remainder of the
// pass length by P, and inside a quad by one with a wrap.  Elements past the tile's end run the same straight-line code on element
// (0, 0) and are not stored.  The height itself is terrain_height() of gf_device.h, the function gf_terrain_height, base_height and the
// terrain spawn of the masked reset inline: the four taps are plain loads of a field every env shares (tens of KB: L1 / L2).
// Traffic: 4·P bytes out per env (+ 8·P with points_out), 12 or 28 bytes in.
#include "gf_launch.h"

namespace gf {

constexpr int kHsBlock = 256;
constexpr int kHsEnvs = GF_HEIGHT_SCAN_TILE_ENVS;
constexpr int kHsFrame = 8;   // floats per env in LDS: bx, by, bz - offset, cy | sy, three of padding (one 16-byte read + one 4-byte read)

template <int V, bool PTS>
__global__ __launch_bounds__(kHsBlock) void height_scan_kernel(const GfHeightScanArgs a) {
    __shared__ __attribute__((aligned(16))) float s_pat[2 * GF_HEIGHT_SCAN_MAX_POINTS];
    __shared__ __attribute__((aligned(16))) float s_frame[kHsEnvs * kHsFrame];
    const int tid = (int)threadIdx.x;
    const int P = a.num_points;
    const int64_t n0 = (int64_t)blockIdx.x * kHsEnvs;
    const int64_t left = a.num_envs - n0;
    const int rows = left < kHsEnvs ? (int)left : kHsEnvs;

    const GF_GLOBAL float* pat = G(a.pattern);
    for (int i = tid; i < 2 * P; i += kHsBlock) s_pat[i] = pat[i];
    if (tid < kHsEnvs) {
        float bx = 0.0f, by = 0.0f, bzo = 0.0f, cy = 1.0f, sy = 0.0f;   // (an env past the end: a finite frame nobody stores from)
        if (tid < rows) {
            const GF_GLOBAL float* b = G(a.pos) + (n0 + tid) * a.pos_stride;
            bx = b[0];
            by = b[1];
            bzo = b[2] - a.offset;
            if (a.align) {
                const GF_GLOBAL float* q = G(a.quat) + (n0 + tid) * a.quat_stride;
                const float qw = q[0], qx = q[1], qy = q[2], qz = q[3];
                const float c = 1.0f - 2.0f * (qy * qy + qz * qz);
                const float s = 2.0f * (qw * qz + qx * qy);
                const float nrm = sqrtf(c * c + s * s);
                const bool flat = nrm < 1e-6f;   // the base points straight up or down (or the quaternion is zero): no yaw to take
                cy = flat ? 1.0f : c / nrm;
                sy = flat ? 0.0f : s / nrm;
            }
        }
        float* fr = s_frame + tid * kHsFrame;
        fr[0] = bx; fr[1] = by; fr[2] = bzo; fr[3] = cy; fr[4] = sy;
    }
    __syncthreads();

    const int total = rows * P;
    constexpr int kPass = V * kHsBlock;                // elements of one pass of the workgroup
    const int de = kPass / P, dp = kPass - de * P;     // workgroup-uniform
    int e = (V * tid) / P, p = V * tid - e * P;        // the lane's one division
    GF_GLOBAL float* out = G(a.out) + n0 * a.out_stride;
    GF_GLOBAL float* pts = PTS ? G(a.points_out) + 2 * (n0 * P) : nullptr;
    const float lo = a.clip_lo, hi = a.clip_hi;
    const bool relative = a.relative != 0;

    for (int f = V * tid; f - V * tid < total; f += kPass) {   // (the bound is the pass's first element: uniform)
        float r[V];
        int64_t off[V];
        int ej = e, pj = p;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const bool live = f + j < total;
            const int es = live ? ej : 0, ps = live ? pj : 0;
            const float2 o = *reinterpret_cast<const float2*>(s_pat + 2 * ps);
            const float4 fr = *reinterpret_cast<const float4*>(s_frame + es * kHsFrame);   // bx, by, bz - offset, cy
            const float sy = s_frame[es * kHsFrame + 4];
            const float px = fr.x + (fr.w * o.x - sy * o.y);
            const float py = fr.y + (sy * o.x + fr.w * o.y);
            const float h = terrain_height(a.terrain, px, py);
            const float v = relative ? fr.z - h : h;
            r[j] = clamp_max(clamp_min(v, lo), hi);
            off[j] = (int64_t)es * a.out_stride + ps;
            if (PTS && live) {
                pts[2 * (f + j)] = px;
                pts[2 * (f + j) + 1] = py;
            }
            pj += 1;
            if (pj == P) { pj = 0; ej += 1; }
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
        if (p >= P) { p -= P; e += 1; }
    }
}

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_height_scan_sizeof(void) { return (int)sizeof(GfHeightScanArgs); }

extern "C" __attribute__((visibility("default"))) int gf_height_scan(const GfHeightScanArgs* a, void* stream) {
    if (!a || !a->out || !a->pos || !a->pattern) return GF_E_NULL;
    if (a->align == 1 && !a->quat) return GF_E_NULL;
    const int64_t tiles = a->num_envs < 0 ? -1 : (a->num_envs + gf::kHsEnvs - 1) / gf::kHsEnvs;
    if (tiles < 0 || tiles > 0x7fffffff) return GF_E_RANGE;
    const int P = a->num_points;
    if (P < 1 || P > GF_HEIGHT_SCAN_MAX_POINTS) return GF_E_RANGE;
    if (a->pos_stride < 3 || (a->quat && a->quat_stride < 4) || a->out_stride < P) return GF_E_RANGE;
    if ((a->align != 0 && a->align != 1) || (a->relative != 0 && a->relative != 1) || a->clip_lo > a->clip_hi) return GF_E_RANGE;
    if (a->terrain.height_field && (a->terrain.rows < 1 || a->terrain.cols < 1)) return GF_E_RANGE;
    if (a->num_envs == 0) return GF_OK;
    // 16-byte stores: `out` aligned, and either the rows follow each other without a gap (a tile starts a multiple of kHsEnvs·P floats
    // in: 16-byte aligned for every P) or every row starts aligned and is made of whole quads
    static_assert(gf::kHsEnvs % 4 == 0, "a dense tile starts 16-byte aligned");
    const bool vec = !(reinterpret_cast<uintptr_t>(a->out) & 15u) && (a->out_stride == P || (P % 4 == 0 && a->out_stride % 4 == 0));
    hipStream_t s = (hipStream_t)stream;
    gf::PhaseScope scope(GF_PHASE_TERRAIN, s);
    const unsigned grid = (unsigned)tiles;
    if (vec && a->points_out) GF_LAUNCH(scope, (gf::height_scan_kernel<4, true>), grid, gf::kHsBlock, 0, s, *a);
    else if (vec) GF_LAUNCH(scope, (gf::height_scan_kernel<4, false>), grid, gf::kHsBlock, 0, s, *a);
    else if (a->points_out) GF_LAUNCH(scope, (gf::height_scan_kernel<1, true>), grid, gf::kHsBlock, 0, s, *a);
    else GF_LAUNCH(scope, (gf::height_scan_kernel<1, false>), grid, gf::kHsBlock, 0, s, *a);
    return gf::launch_status();
}
