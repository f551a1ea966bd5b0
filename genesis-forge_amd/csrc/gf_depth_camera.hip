// gf_depth_camera.hip — gf_depth_camera: the camera model behind a depth policy (managers/depth_camera.py): frame rate, latency,
// range clip, noise, holes and the frame stack of a depth sensor, in one launch per control step.  include/gf_step.h has the
// contract and the float32 operation sequence; the cast itself is gf_ray_walk.h's, the code gf_ray_cast.hip runs.
//
// Composed around RayCaster.cast() the model pays a full cast every step and a chain of [N, R] tensor ops behind it, whether or not a
// new frame is due.  Here only the envs whose frame is due are cast, and an env that is not due costs its four bytes of
// episode_length.  A 256-lane workgroup owns a span of kDcSpan envs.  Its first wave reads the span's episode lengths, decides who is
// due and compacts those envs into an LDS list — one ballot, the rank of a lane is the popcount of the ballot below it.  A workgroup
// with an empty list is gone after one barrier, before it has staged anything.  Otherwise the first `ndue` lanes stage the frames of the
// due envs (origin and nine matrix entries, as the ray cast does), advance their ring heads and draw the latency of the fresh ones;
// all lanes stage the pattern.  The workgroup then walks ndue·R elements in flat order, consecutive lanes on consecutive rays of the
// COMPACTED envs: every lane is busy whichever envs are due (a lane per env under a mask would idle 1 − 1/interval of the machine, and
// its neighbours would walk unrelated cells).  V = 4 rays per lane and pass where 16-byte stores are possible (R % 4 == 0, so a quad
// never straddles two envs and every row of every slot and channel is aligned), V = 1 otherwise.
// A lane first moves the older channels of its quad — image[n, c] from the ring slots earlier launches wrote, loads and stores that
// nothing below depends on, so they drain while the rays walk — then casts, puts the value through the sensor and stores it from
// registers: to the ring slot, to channel 0 where the latency is zero, to every slot and channel for a fresh env.  The launch never
// reads what it writes, so nothing is ordered between lanes or workgroups.  No scratch: the only private array is r[V], unrolled.
// Traffic of a due env: 4·R·(1 + stack) bytes out, 4·R·(stack − [lag = 0]) in, 28 of pose, 8 of head and lag.
#include "gf_launch.h"
#include "gf_ray_walk.h"

namespace gf {

constexpr int kDcBlock = 256;
constexpr int kDcSpan = GF_DEPTH_CAMERA_SPAN_ENVS;
static_assert(kDcSpan >= 1 && kDcSpan <= GF_WAVE, "one wave takes the span's ballot");
static_assert(GF_DEPTH_CAMERA_MAX_SLOTS <= 128, "head and lag share an LDS word");

template <int V>
struct DcWord;
template <>
struct DcWord<1> { typedef float T; };
template <>
struct DcWord<4> { typedef f32x4 T; };

// step 6 of the contract: one pixel through the sensor
__device__ __forceinline__ float dc_sensor(const GfDepthCameraArgs& a, float d, uint32_t genv, uint32_t ray, uint32_t k0, uint32_t k1) {
    float v = d, u1 = 1.0f;
    if (a.noise != 0.0f || a.dropout != 0.0f) {   // workgroup-uniform
        const U4 w = philox4x32_10(genv, ray, a.tick, 0u, k0, k1);
        if (a.noise != 0.0f) v = d + a.noise * (2.0f * u24_to_unit(w.x) - 1.0f);
        u1 = u24_to_unit(w.y);
    }
    v = v < a.near_clip ? a.near_clip : v;
    v = v > a.far_clip ? a.far_clip : v;
    if (a.dropout != 0.0f && u1 < a.dropout) v = a.dropout_value;
    if (a.normalize) v = (v - a.near_clip) * a.inv_span - 0.5f;
    return v;
}

template <int V, bool FIELD>
__global__ __launch_bounds__(kDcBlock) void depth_camera_kernel(const GfDepthCameraArgs a) {
    typedef typename DcWord<V>::T W;
    extern __shared__ __attribute__((aligned(16))) float s_dc[];
    float* s_frame = s_dc;                        // [kDcSpan, kRcFrame], the first ndue rows in use
    float* s_pat = s_dc + kDcSpan * kRcFrame;     // [R, 6]
    __shared__ int s_env[kDcSpan];                // the due list: local env index | fresh << 8
    __shared__ int s_slot[kDcSpan];               // per list entry: new head | lag << 8
    __shared__ int s_ndue;
    const int tid = (int)threadIdx.x;
    const int R = a.num_rays;
    const int64_t n0 = (int64_t)blockIdx.x * kDcSpan;
    const int64_t left = a.num_envs - n0;
    const int rows = left < kDcSpan ? (int)left : kDcSpan;

    // 1-2: who is due (the first wave; everything it reads is read-only in the launch)
    if (tid < GF_WAVE) {
        bool fresh = false, due = false;
        if (tid < rows) {
            const int64_t n = n0 + tid;
            fresh = G(a.episode_length)[n] <= 1;
            const uint32_t phase = a.staggered ? (uint32_t)(n % (int64_t)a.interval) : 0u;
            due = fresh || (a.tick + phase) % (uint32_t)a.interval == 0u;
            if (a.due_out) G(a.due_out)[n] = due ? 1 : 0;
        }
        const unsigned long long m = __ballot(due);
        if (due) s_env[popc64(m & ((1ull << tid) - 1ull))] = tid | (fresh ? 0x100 : 0);
        if (tid == 0) s_ndue = popc64(m);
    }
    __syncthreads();
    const int ndue = s_ndue;
    if (ndue == 0) return;   // workgroup-uniform: nothing staged, nothing written

    // 4-5 and the staging: the pattern by everybody, a due env's frame, head and lag by one lane each
    const uint32_t k0 = (uint32_t)(a.seed ^ GF_DEPTH_CAMERA_SEED_TAG), k1 = (uint32_t)((a.seed ^ GF_DEPTH_CAMERA_SEED_TAG) >> 32);
    const int S = a.slots, stack = a.stack;
    const GF_GLOBAL float* pat = G(a.pattern);
    for (int i = tid; i < 6 * R; i += kDcBlock) s_pat[i] = pat[i];
    if (tid < ndue) {
        const int ef = s_env[tid];
        const int64_t n = n0 + (ef & 0xff);
        rc_frame(s_frame + tid * kRcFrame, G(a.pos) + n * a.pos_stride, G(a.quat) + n * a.quat_stride, a.align, true);
        int h = G(a.head)[n];
        h = (h < 0 || h >= S) ? 0 : h;
        h = h + 1 == S ? 0 : h + 1;
        G(a.head)[n] = h;
        int l;
        if (ef & 0x100) {
            const float u = u24_to_unit(philox4x32_10((uint32_t)n + a.env_offset, 0u, a.tick, 1u, k0, k1).x);
            const int w = a.latency_hi - a.latency_lo + 1;
            const int r = (int)(u * (float)w);
            l = a.latency_lo + (r < w - 1 ? r : w - 1);
            G(a.lag)[n] = l;
        } else {
            l = G(a.lag)[n];
            l = (l < 0 || l > S - stack) ? 0 : l;
        }
        s_slot[tid] = h | (l << 8);
    }
    __syncthreads();

    const RcGrid g = rc_grid<FIELD>(a.terrain, a.max_range);
    const bool depth = a.mode == GF_RAY_MODE_DEPTH;
    const float ax = a.axis[0], ay = a.axis[1], az = a.axis[2];
    const float miss = a.miss_value;
    const int64_t slot_stride = a.num_envs * (int64_t)R;   // floats between two slots of the ring

    // 6-7: ndue·R elements in flat order.  V == 4 only with R % 4 == 0: a lane's quad lies in one env and is whole.
    const int total = ndue * R;
    constexpr int kPass = V * kDcBlock;
    const int de = kPass / R, dp = kPass - de * R;     // workgroup-uniform
    int e = (V * tid) / R, p = V * tid - e * R;        // the lane's one division
    for (int f = V * tid; f < total; f += kPass) {
        const int ef = s_env[e], hl = s_slot[e];
        const bool fresh = (ef & 0x100) != 0;
        const int h = hl & 0xff, l = hl >> 8;
        const int64_t n = n0 + (ef & 0xff);
        GF_GLOBAL float* rrow = G(a.ring) + n * R + p;                    // slot 0
        GF_GLOBAL float* irow = G(a.image) + n * ((int64_t)stack * R) + p;   // channel 0
        if (!fresh) {
            // the older channels: slots other than h, written by earlier launches (1 <= l + c <= S - 1)
            for (int c = l == 0 ? 1 : 0; c < stack; ++c) {
                const int s = h - l - c;
                *reinterpret_cast<GF_GLOBAL W*>(irow + (int64_t)c * R) =
                    *reinterpret_cast<const GF_GLOBAL W*>(rrow + (int64_t)(s < 0 ? s + S : s) * slot_stride);
            }
        }
        const uint32_t genv = (uint32_t)n + a.env_offset;
        float r[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const RcRay y = rc_ray(s_frame + e * kRcFrame, s_pat + 6 * (p + j));
            float t;
            const bool hit = rc_hit<FIELD>(g, y, true, t);
            const float val = depth ? t * ((y.ex * ax + y.ey * ay) + y.ez * az) : t;
            r[j] = dc_sensor(a, hit ? val : miss, genv, (uint32_t)(p + j), k0, k1);
        }
        W q;
        if constexpr (V == 4) {
            q.x = r[0]; q.y = r[1]; q.z = r[2]; q.w = r[3];
        } else {
            q = r[0];
        }
        if (fresh) {
            for (int s = 0; s < S; ++s) *reinterpret_cast<GF_GLOBAL W*>(rrow + (int64_t)s * slot_stride) = q;
            for (int c = 0; c < stack; ++c) *reinterpret_cast<GF_GLOBAL W*>(irow + (int64_t)c * R) = q;
        } else {
            *reinterpret_cast<GF_GLOBAL W*>(rrow + (int64_t)h * slot_stride) = q;
            if (l == 0) *reinterpret_cast<GF_GLOBAL W*>(irow) = q;
        }
        p += dp;
        e += de;
        if (p >= R) { p -= R; e += 1; }
    }
}

template <int V>
static void dc_launch(PhaseScope& scope, const GfDepthCameraArgs& a, unsigned grid, size_t lds, hipStream_t s) {
    if (a.terrain.height_field) GF_LAUNCH(scope, (depth_camera_kernel<V, true>), grid, kDcBlock, lds, s, a);
    else GF_LAUNCH(scope, (depth_camera_kernel<V, false>), grid, kDcBlock, lds, s, a);
}

static bool dc_finite(float v) { return v >= -3.4028234663852886e38f && v <= 3.4028234663852886e38f; }   // (a NaN fails)

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_depth_camera_sizeof(void) { return (int)sizeof(GfDepthCameraArgs); }

extern "C" __attribute__((visibility("default"))) int gf_depth_camera(const GfDepthCameraArgs* a, void* stream) {
    if (!a || !a->pos || !a->pattern || !a->episode_length || !a->ring || !a->head || !a->lag || !a->image) return GF_E_NULL;
    if (a->align != GF_RAY_ALIGN_WORLD && !a->quat) return GF_E_NULL;
    // what gf_ray_cast refuses
    const int64_t spans = a->num_envs < 0 ? -1 : (a->num_envs + gf::kDcSpan - 1) / gf::kDcSpan;
    if (spans < 0 || spans > 0x7fffffff) return GF_E_RANGE;
    const int R = a->num_rays;
    if (R < 1 || R > GF_RAY_CAST_MAX_RAYS) return GF_E_RANGE;
    if (a->pos_stride < 3 || (a->quat && a->quat_stride < 4)) return GF_E_RANGE;
    if (a->align < GF_RAY_ALIGN_WORLD || a->align > GF_RAY_ALIGN_BASE || (a->mode != GF_RAY_MODE_DISTANCE && a->mode != GF_RAY_MODE_DEPTH))
        return GF_E_RANGE;
    if (!(a->max_range >= 0.0f) || a->max_range == __builtin_huge_valf()) return GF_E_RANGE;   // (a NaN fails the first test)
    if (a->terrain.height_field && (a->terrain.rows < 2 || a->terrain.cols < 2)) return GF_E_RANGE;
    // the camera's own
    if (a->interval < 1 || a->stack < 1 || a->latency_lo < 0 || a->latency_hi < a->latency_lo) return GF_E_RANGE;
    if (a->slots > GF_DEPTH_CAMERA_MAX_SLOTS || a->stack > a->slots || a->latency_hi > a->slots - a->stack) return GF_E_RANGE;
    if ((a->staggered != 0 && a->staggered != 1) || (a->normalize != 0 && a->normalize != 1)) return GF_E_RANGE;
    if (!gf::dc_finite(a->near_clip) || !gf::dc_finite(a->far_clip) || !(a->near_clip < a->far_clip)) return GF_E_RANGE;
    if (!(a->dropout >= 0.0f && a->dropout <= 1.0f) || !(a->noise >= 0.0f) || !gf::dc_finite(a->noise)) return GF_E_RANGE;
    if (a->num_envs == 0) return GF_OK;
    // 16-byte words: whole quads per row, and every row of every slot and channel starts a multiple of R floats into an aligned buffer
    const bool vec = R % 4 == 0 && !((reinterpret_cast<uintptr_t>(a->ring) | reinterpret_cast<uintptr_t>(a->image)) & 15u);
    hipStream_t s = (hipStream_t)stream;
    gf::PhaseScope scope(GF_PHASE_TERRAIN, s);
    const unsigned grid = (unsigned)spans;
    const size_t lds = sizeof(float) * (size_t)(gf::kDcSpan * gf::kRcFrame + 6 * R);
    if (vec) gf::dc_launch<4>(scope, *a, grid, lds, s);
    else gf::dc_launch<1>(scope, *a, grid, lds, s);
    return gf::launch_status();
}
