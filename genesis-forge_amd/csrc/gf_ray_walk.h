// gf_ray_walk.h — what one ray against the terrain surface is, shared by gf_ray_cast.hip and gf_depth_camera.hip: the frame of an env
// (origin and nine matrix entries), a ray of the pattern in that frame, the clip to the field's rectangle and the cell walk.
// include/gf_step.h (GfRayCastArgs) has the float32 operation sequence; this file follows it line by line, and both kernels get the
// same bits from it because every function here is one rounding per operation with nothing contracted.
#pragma once

#include "gf_device.h"

namespace gf {

constexpr int kRcFrame = 12;   // floats per env in LDS: bx, by, bz, r00 | r01, r02, r10, r11 | r12, r20, r21, r22 (three 16-byte reads)

struct RcGrid {   // workgroup-uniform
    const GF_GLOBAL float* f;
    int W, H;
    float x_min, y_min, sx, sy, fw, fh, tmax, origin_z;
};

template <bool FIELD>
__device__ __forceinline__ RcGrid rc_grid(const GfTerrainView& tv, float max_range) {
    RcGrid g;
    g.f = G(tv.height_field);
    g.W = tv.cols;
    g.H = tv.rows;
    g.x_min = tv.x_min;
    g.y_min = tv.y_min;
    g.fw = (float)(g.W - 1);
    g.fh = (float)(g.H - 1);
    g.sx = FIELD ? g.fw / tv.x_span : 0.0f;
    g.sy = FIELD ? g.fh / tv.y_span : 0.0f;
    g.tmax = max_range;
    g.origin_z = tv.origin_z;
    return g;
}

// the frame of one env into dst ([kRcFrame], LDS): b = its pos row, q = its quat row (never read with GF_RAY_ALIGN_WORLD); an env that
// is not `live` (past the end of the tile: nobody stores from it) gets the identity at the origin and reads nothing
__device__ __forceinline__ void rc_frame(float* dst, const GF_GLOBAL float* b, const GF_GLOBAL float* q, int align, bool live) {
    float bx = 0.0f, by = 0.0f, bz = 0.0f;
    float r00 = 1.0f, r01 = 0.0f, r02 = 0.0f, r10 = 0.0f, r11 = 1.0f, r12 = 0.0f, r20 = 0.0f, r21 = 0.0f, r22 = 1.0f;
    if (live) {
        bx = b[0];
        by = b[1];
        bz = b[2];
        if (align != GF_RAY_ALIGN_WORLD) {
            const float qw = q[0], qx = q[1], qy = q[2], qz = q[3];
            const float c = 1.0f - 2.0f * (qy * qy + qz * qz);
            const float s = 2.0f * (qw * qz + qx * qy);
            if (align == GF_RAY_ALIGN_YAW) {
                const float nrm = sqrtf(c * c + s * s);
                const bool flat = nrm < 1e-6f;
                const float cy = flat ? 1.0f : c / nrm;
                const float sy = flat ? 0.0f : s / nrm;
                r00 = cy; r01 = -sy; r10 = sy; r11 = cy;
            } else {
                r00 = c;
                r01 = 2.0f * (qx * qy - qw * qz);
                r02 = 2.0f * (qx * qz + qw * qy);
                r10 = s;
                r11 = 1.0f - 2.0f * (qx * qx + qz * qz);
                r12 = 2.0f * (qy * qz - qw * qx);
                r20 = 2.0f * (qx * qz - qw * qy);
                r21 = 2.0f * (qy * qz + qw * qx);
                r22 = 1.0f - 2.0f * (qx * qx + qy * qy);
            }
        }
    }
    dst[0] = bx; dst[1] = by; dst[2] = bz; dst[3] = r00;
    dst[4] = r01; dst[5] = r02; dst[6] = r10; dst[7] = r11;
    dst[8] = r12; dst[9] = r20; dst[10] = r21; dst[11] = r22;
}

struct RcRay {
    float ox, oy, oz, dx, dy, dz;   // world origin and direction
    float ex, ey, ez;               // the direction in the sensor's frame (the depth factor)
};

// ray `pat` ([6] in LDS: px, py, pz, ex, ey, ez) in the frame `fr` ([kRcFrame] in LDS, 16-byte aligned)
__device__ __forceinline__ RcRay rc_ray(const float* fr, const float* pat) {
    const float2 p01 = *reinterpret_cast<const float2*>(pat);
    const float2 p23 = *reinterpret_cast<const float2*>(pat + 2);
    const float2 p45 = *reinterpret_cast<const float2*>(pat + 4);
    const float px = p01.x, py = p01.y, pz = p23.x;
    RcRay r;
    r.ex = p23.y; r.ey = p45.x; r.ez = p45.y;
    const float4 f0 = *reinterpret_cast<const float4*>(fr);       // bx, by, bz, r00
    const float4 f1 = *reinterpret_cast<const float4*>(fr + 4);   // r01, r02, r10, r11
    const float4 f2 = *reinterpret_cast<const float4*>(fr + 8);   // r12, r20, r21, r22
    r.ox = f0.x + ((f0.w * px + f1.x * py) + f1.y * pz);
    r.oy = f0.y + ((f1.z * px + f1.w * py) + f2.x * pz);
    r.oz = f0.z + ((f2.y * px + f2.z * py) + f2.w * pz);
    r.dx = (f0.w * r.ex + f1.x * r.ey) + f1.y * r.ez;
    r.dy = (f1.z * r.ex + f1.w * r.ey) + f2.x * r.ez;
    r.dz = (f2.y * r.ex + f2.z * r.ey) + f2.w * r.ez;
    return r;
}

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

// one ray against the field (the walk) or the plane z = origin_z; a lane that is not `live` walks nothing.  Returns hit, t* in `t`.
template <bool FIELD>
__device__ __forceinline__ bool rc_hit(const RcGrid& g, const RcRay& r, bool live, float& t) {
    t = 0.0f;
    if constexpr (FIELD) {
        return live && rc_walk(g, r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, t);
    } else {
        const float C = r.oz - g.origin_z;
        const float tt = C / (-r.dz);
        const bool under = C <= 0.0f;
        t = under ? 0.0f : tt;
        return under || (r.dz < 0.0f && tt <= g.tmax);
    }
}

}  // namespace gf
