// gf_action.hip — Phase A: GenesisEnv.step bookkeeping + PositionActionManager.step, one launch.
//
// Replaces (reference, /root/reference/genesis_forge/):
//   genesis_env.py:196-203          episode_length += 1; last_actions <- actions; actions <- new
//   managers/action/base.py:67-82   raw -> manager copy
//   managers/action/position_action_manager.py:402-414   NaN/Inf scan, a*scale+offset, clamp(lo,hi)
//   managers/action/position_within_limits.py:125-126    clamp(-1,1), a*scale+offset
// which the reference runs as ~13 separate elementwise launches + 2 host syncs.
//
// Layout: the [N,D] arrays are treated as one flat stream of N*D floats; each lane owns one
// float4 (16 B/lane, 1 KiB per wave instruction, fully coalesced).  The [D] constants are
// indexed with (4*i+j) % D and come from L1/K$.  Algorithmic traffic: 20*D B/env
// (R new, R prev, W last, W actions, W targets) + 8 B/env for episode_length.
#include "gf_action_row.h"
#include "gf_launch.h"

namespace gf {

// (the statistics ring's upkeep workgroups and the float4 row body live in gf_action_row.h, shared with the folded tile tick)
template <bool VEC4, bool CONST4 = false>
__global__ __launch_bounds__(256) void action_kernel(const GfActionArgs a, const int64_t total, const int upkeep) {
    if ((int)blockIdx.x < upkeep) {
        action_upkeep(a, upkeep);
        return;
    }
    const int64_t i = (int64_t)(blockIdx.x - upkeep) * blockDim.x + threadIdx.x;
    const int D = a.num_dofs;
    const int mode = a.mode;
    int flags = 0;

    // episode_length += 1  (genesis_env.py:197) — first N/4 lanes, int4 RMW
    if (a.episode_length) {
        const int64_t N = a.num_envs;
        if (VEC4 && (N & 3) == 0) {
            if (i < (N >> 2)) {
                int4* p = reinterpret_cast<int4*>(a.episode_length) + i;
                int4 v = *p;
                v.x += 1; v.y += 1; v.z += 1; v.w += 1;
                *p = v;
            }
        } else if (i < N) {
            a.episode_length[i] += 1;
        }
    }

    if (VEC4) {
        if (i < (total >> 2)) {
            const float4 x = reinterpret_cast<const float4*>(a.actions_in)[i];
            if (CONST4) {
                float4 prev = x, last, act, tg;
                if (a.env_actions) prev = reinterpret_cast<const float4*>(a.env_actions)[i];
                action_row4(a, action_consts4(a, (int)((i * 4) % D), mode), mode, x, prev, last, act, tg, flags);
                if (a.env_actions) {
                    reinterpret_cast<float4*>(a.env_last_actions)[i] = last;
                    reinterpret_cast<float4*>(a.env_actions)[i] = act;
                }
                reinterpret_cast<float4*>(a.targets)[i] = tg;
            } else {
                if (a.env_actions) {
                    const float4 prev = reinterpret_cast<const float4*>(a.env_actions)[i];
                    reinterpret_cast<float4*>(a.env_last_actions)[i] = prev;
                    reinterpret_cast<float4*>(a.env_actions)[i] = x;
                }
                const float xs[4] = {x.x, x.y, x.z, x.w};
                float ts[4];
                int d = (int)((i * 4) % D);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float lo = mode == GF_ACTION_POSITION ? a.clip_lo[d] : 0.f;
                    const float hi = mode == GF_ACTION_POSITION ? a.clip_hi[d] : 0.f;
                    ts[j] = action_target(xs[j], a.scale[d], a.offset[d], lo, hi, mode);
                    if (a.check_finite && mode == GF_ACTION_POSITION) {
                        flags |= isnan(xs[j]) ? 1 : 0;
                        flags |= isinf(xs[j]) ? 2 : 0;
                    }
                    d = d + 1 == D ? 0 : d + 1;
                }
                reinterpret_cast<float4*>(a.targets)[i] = make_float4(ts[0], ts[1], ts[2], ts[3]);
            }
        }
    } else {
        if (i < total) {
            const float x = a.actions_in[i];
            if (a.env_actions) {
                a.env_last_actions[i] = a.env_actions[i];
                a.env_actions[i] = x;
            }
            const int d = (int)(i % D);
            const float lo = mode == GF_ACTION_POSITION ? a.clip_lo[d] : 0.f;
            const float hi = mode == GF_ACTION_POSITION ? a.clip_hi[d] : 0.f;
            a.targets[i] = action_target(x, a.scale[d], a.offset[d], lo, hi, mode);
            if (a.check_finite && mode == GF_ACTION_POSITION) {
                flags |= isnan(x) ? 1 : 0;
                flags |= isinf(x) ? 2 : 0;
            }
        }
    }

    action_flags_commit(a, flags);
}

// What gf_action_step checks before it launches; also asked by gf_run_ops before it folds the phase into the scene tick.
int action_validate(const GfActionArgs* a) {
    if (!a || !a->actions_in || !a->targets || !a->scale || !a->offset) return GF_E_NULL;
    if (a->mode == GF_ACTION_POSITION && (!a->clip_lo || !a->clip_hi)) return GF_E_NULL;
    if (a->mode != GF_ACTION_POSITION && a->mode != GF_ACTION_WITHIN_LIMITS) return GF_E_RANGE;
    if (a->env_actions && !a->env_last_actions) return GF_E_NULL;
    if (a->num_envs < 0 || a->num_dofs <= 0) return GF_E_RANGE;
    return GF_OK;
}

static bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the streams can be moved as float4s (and episode_length as int4s) …
bool action_vec4(const GfActionArgs* a) {
    const int64_t total = (int64_t)a->num_envs * a->num_dofs;
    return (total & 3) == 0 && al16(a->actions_in) && al16(a->targets) && (!a->env_actions || (al16(a->env_actions) && al16(a->env_last_actions))) &&
           (!a->episode_length || al16(a->episode_length));
}

// … and a float4 is four consecutive DOFs of one env whose constants are one 16-byte load per array
bool action_const4(const GfActionArgs* a) {
    return (a->num_dofs & 3) == 0 && al16(a->scale) && al16(a->offset) && (a->mode != GF_ACTION_POSITION || (al16(a->clip_lo) && al16(a->clip_hi)));
}

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_action_step(const GfActionArgs* a, void* stream) {
    const int valid = gf::action_validate(a);
    if (valid != GF_OK) return valid;
    if (a->num_envs == 0) return GF_OK;
    const int64_t total = (int64_t)a->num_envs * a->num_dofs;
    const bool vec = gf::action_vec4(a);
    hipStream_t s = (hipStream_t)stream;
    gf::PhaseScope scope(GF_PHASE_ACTION, s);
    scope.begin_bracket();
    const int upkeep = gf::action_upkeep_blocks(a);
    if (vec) {
        int64_t lanes = total >> 2;
        if (a->episode_length) {
            const int64_t need = (a->num_envs & 3) == 0 ? (a->num_envs >> 2) : a->num_envs;
            if (need > lanes) lanes = need;
        }
        const bool const4 = gf::action_const4(a);
        // D = 12: 192 lanes = the float4s of exactly 64 envs, so workgroup b owns envs [64b, 64b+64) like workgroup b of the scene and
        // post-physics kernels does — with round-robin workgroup → XCD placement a tile stays on one XCD (one L2) across the step
        // (measured in the benchmark loop at 65 536 envs: action kernel 8.6 → 7.1 µs, step 22.8 → 20.4 µs; GF_ACTION_BLOCK256=1 restores
        // the flat 256-lane mapping for comparison)
        static const bool flat256 = getenv("GF_ACTION_BLOCK256") != nullptr;
        static const int forced = getenv("GF_ACTION_BLOCK") ? atoi(getenv("GF_ACTION_BLOCK")) : 0;   // experiments only
        const int block = forced > 0 ? forced : ((a->num_dofs == 12 && !flat256) ? 192 : 256);
        if (const4) gf::klaunch(gf::action_kernel<true, true>, dim3(gf::env_grid(lanes, block) + upkeep), dim3(block), 0, s, *a, total, upkeep);
        else gf::klaunch(gf::action_kernel<true>, dim3(gf::env_grid(lanes, block) + upkeep), dim3(block), 0, s, *a, total, upkeep);
    } else {
        int64_t lanes = total > a->num_envs ? total : a->num_envs;
        gf::klaunch(gf::action_kernel<false>, dim3(gf::env_grid(lanes, 256) + upkeep), dim3(256), 0, s, *a, total, upkeep);
    }
    return gf::launch_status();
}
