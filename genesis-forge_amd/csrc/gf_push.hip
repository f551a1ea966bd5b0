// gf_push.hip — gf_push: the random pushes of a rough-terrain task (managers/push.py; legged_gym's _push_robots, Isaac Lab's
// push_by_setting_velocity as an `interval` event): per-env interval timers and the velocity kick, in one launch.
// include/gf_step.h has the contract.
//
// Composed from torch the event is a chain of small launches every step — compare, draw, scale, where, scatter, redraw — whether or
// not anything is due.  Here a lane owns an env, as in the terrain curriculum: it reads its `due` word and its mask bytes, the wave
// takes a ballot of "done or due" and leaves when no lane needs work, having written its 64 `fired` bytes.  The timer is an absolute
// step, not a countdown, for exactly that: with intervals of hundreds of steps almost every wave of almost every launch reads 4 + 2
// bytes per lane, writes one and is gone.  A working lane takes its draws (two Philox blocks at most, or a dense parity row), rewrites
// its timer and, if it fires, touches at most 24 bytes of velocity, component by component (the rows are 12 bytes wide and need not be
// 16-byte aligned).  Nothing is shared between lanes, so there is no LDS; the counter is one vector atomicAdd per wave from the
// ballot's popcount.  A workgroup is four waves (256 envs), as in the curriculum: the waves are independent.
#include "gf_launch.h"

namespace gf {

constexpr int kPushBlock = GF_PUSH_BLOCK_ENVS;

__global__ __launch_bounds__(kPushBlock) void push_kernel(const GfPushArgs a) {
    const int lane = (int)(threadIdx.x & (GF_WAVE - 1));
    const int64_t n = (int64_t)blockIdx.x * kPushBlock + (int64_t)threadIdx.x;
    const bool in = n < a.num_envs;
    bool done = false, fire = false;
    if (in) {
        const uint32_t due = (uint32_t)G(a.due)[n];
        if (!a.global_timer) done = (a.mask && G(a.mask)[n]) || (a.mask2 && G(a.mask2)[n]);
        fire = !done && (int32_t)(a.step - due) >= 0;
    }
    if (in && a.fired) G(a.fired)[n] = fire ? 1 : 0;
    if (!__ballot(done || fire)) return;   // wave-uniform

    if (done || fire) {
        const uint32_t k0 = (uint32_t)(a.seed ^ GF_PUSH_SEED_TAG), k1 = (uint32_t)((a.seed ^ GF_PUSH_SEED_TAG) >> 32);
        const uint32_t genv = (uint32_t)n + a.env_offset;
        const GF_GLOBAL float* d = a.draws ? G(a.draws) + 7 * n : nullptr;
        float u[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (d) {
            u[3] = d[3];
        } else {
            // (a fired env needs the whole block, a done one only its fourth word: one block either way)
            const U4 r0 = philox4x32_10(genv, 0u, a.step, 0u, k0, k1);
            u[0] = u24_to_unit(r0.x); u[1] = u24_to_unit(r0.y); u[2] = u24_to_unit(r0.z); u[3] = u24_to_unit(r0.w);
            if (a.global_timer) u[3] = u24_to_unit(philox4x32_10(0xFFFFFFFFu, 0u, a.step, 0u, k0, k1).w);
        }

        // 3: the next push
        const int w = a.interval_hi - a.interval_lo + 1;
        const int r = (int)(u[3] * (float)w);
        G(a.due)[n] = (int32_t)(a.step + (uint32_t)a.interval_lo + (uint32_t)(r < w - 1 ? r : w - 1));

        // 4: the kick
        if (fire) {
            if (d) {
#pragma unroll
                for (int j = 0; j < 6; ++j)
                    if (a.comp_mask & (1 << j)) u[j < 3 ? j : j + 1] = d[j < 3 ? j : j + 1];
            } else if (a.comp_mask & 0x38) {
                const U4 r1 = philox4x32_10(genv, 1u, a.step, 0u, k0, k1);
                u[4] = u24_to_unit(r1.x); u[5] = u24_to_unit(r1.y); u[6] = u24_to_unit(r1.z);
            }
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                if (!(a.comp_mask & (1 << j))) continue;
                GF_GLOBAL float* p = (j < 3 ? G(a.lin_vel) + 3 * n + j : G(a.ang_vel) + 3 * n + (j - 3));
                const float v = uniform_range(u[j < 3 ? j : j + 1], a.lo[j], a.hi[j]) * a.scale;
                *p = a.mode ? *p + v : v;
            }
        }
    }
    const unsigned long long bf = __ballot(fire);
    if (lane == 0 && bf) atomicAdd(a.counts, popc64(bf));
}

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_push_sizeof(void) { return (int)sizeof(GfPushArgs); }

extern "C" __attribute__((visibility("default"))) int gf_push(const GfPushArgs* a, void* stream) {
    if (!a || !a->due || !a->lin_vel || !a->counts) return GF_E_NULL;
    if (a->comp_mask < 0 || a->comp_mask > 0x3f) return GF_E_RANGE;
    if ((a->comp_mask & 0x38) && !a->ang_vel) return GF_E_NULL;
    const int64_t blocks = a->num_envs < 0 ? -1 : (a->num_envs + gf::kPushBlock - 1) / gf::kPushBlock;
    if (blocks < 0 || blocks > 0x7fffffff) return GF_E_RANGE;
    if (a->interval_lo < 1 || a->interval_hi < a->interval_lo || (int64_t)a->interval_hi - (int64_t)a->interval_lo + 1 > (1 << 24)) return GF_E_RANGE;
    if ((a->mode != 0 && a->mode != 1) || (a->global_timer != 0 && a->global_timer != 1)) return GF_E_RANGE;
    // (written so that a NaN fails: only a finite value passes)
    const float big = 3.4028234663852886e38f;
    if (!(a->scale >= -big && a->scale <= big)) return GF_E_RANGE;
    for (int j = 0; j < 6; ++j) {
        if (!(a->lo[j] >= -big && a->lo[j] <= big) || !(a->hi[j] >= -big && a->hi[j] <= big)) return GF_E_RANGE;
        if ((a->comp_mask & (1 << j)) && a->hi[j] < a->lo[j]) return GF_E_RANGE;
    }
    if (a->num_envs == 0) return GF_OK;
    hipStream_t s = (hipStream_t)stream;
    gf::PhaseScope scope(GF_PHASE_TERRAIN, s);
    GF_LAUNCH(scope, gf::push_kernel, (unsigned)blocks, gf::kPushBlock, 0, s, *a);
    return gf::launch_status();
}
