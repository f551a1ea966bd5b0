// gf_scene.hip — EntityManager body-frame getters as a standalone call, and the synthetic scene tick.
//
// gf_entity_rotate: EntityManager.get_projected_gravity / get_linear_velocity / get_angular_velocity
//   (managers/entity_manager.py:130-146, utils.py:13-55) for callers that ask for one vector outside a
//   fused phase (opaque user terms).  7-10 torch launches per call in the reference.
//
// gf_synth_scene_step: stands in for Genesis' scene.step() (managed_env.py:292) so the manager
//   pipeline can be driven, benchmarked and parity-tested without the simulator.
//   It is NOT physics: joints track their PD targets with a first-order lag, the base does a damped
//   random walk driven by Philox draws, contacts are sampled per slot.  What matters is that the
//   update is deterministic and integer-RNG driven with f32 ops in a fixed order, so this kernel, the
//   C oracle and the numpy model that drives the reference produce the same bits.
#include <stdlib.h>
#include <string.h>

#include "gf_launch.h"
#include "gf_scene_tile.h"

namespace gf {

__global__ __launch_bounds__(kEnvBlock) void rotate_kernel(const GfRotateArgs a) {
    const int64_t n = (int64_t)blockIdx.x * kEnvBlock + threadIdx.x;
    if (n >= a.num_envs) return;
    const float4 q = load_quat(a.entity.quat, n);
    V3 v{0.f, 0.f, -1.f};
    if (a.what == GF_ROT_LIN_VEL) v = load3(a.entity.lin_vel, n);
    else if (a.what == GF_ROT_ANG_VEL) v = load3(a.entity.ang_vel, n);
    const V3 o = rot_inv(q, v);
    float* r = a.out + 3 * n;
    r[0] = o.x; r[1] = o.y; r[2] = o.z;
}

// Where the synthetic scene puts link l relative to the base: scene link 0 is the ground entity, 1 the robot's base,
// then chains of four (hip, thigh, calf, foot) hanging 8.5 cm apart below the four corners of the body.
struct LinkOffset { float x, y, z; };
__device__ __forceinline__ LinkOffset synth_link_offset(int l) {
    if (l <= 1) return {0.0f, 0.0f, 0.0f};
    const int leg = (l - 2) / 4, depth = (l - 2) % 4 + 1;
    return {leg < 2 ? 0.19f : -0.19f, (leg & 1) ? -0.11f : 0.11f, -0.085f * (float)depth};
}

// The legacy lane-per-env tick (GF_SCENE_LEGACY=1): every load of the env first, then the joints, then the base.
template <int DV>
__device__ __forceinline__ void synth_state_body(const GfSynthSceneArgs& a, const int64_t n, SynthBase& out) {
    const int D = a.num_dofs;
    const float dt = a.dt;
    const uint32_t genv = (uint32_t)n + a.env_offset;
    // all loads first: joint rows as float4 (DV = D/4 when the rows are 16-byte tiles), base state, then one wait
    float4 tg[DV > 0 ? DV : 1], dp[DV > 0 ? DV : 1];
    if (DV > 0) {
        const float4* t4 = reinterpret_cast<const float4*>(a.targets + n * D);
        const float4* p4 = reinterpret_cast<const float4*>(a.dof_pos + n * D);
#pragma unroll
        for (int c = 0; c < DV; ++c) { tg[c] = t4[c]; dp[c] = p4[c]; }
    }
    const float4 q4 = load_quat(a.quat, n);
    const V3 w0 = load3(a.ang_vel, n), v0 = load3(a.lin_vel, n), p0 = load3(a.pos, n);
    const SynthDraws r = synth_draws(a, genv);
    if (DV > 0) {
        float4* v4 = reinterpret_cast<float4*>(a.dof_vel + n * D);
        float4* p4 = reinterpret_cast<float4*>(a.dof_pos + n * D);
#pragma unroll
        for (int c = 0; c < DV; ++c) {
            float4 v, p = dp[c];
            synth_joint(tg[c].x, p.x, v.x, a.joint_rate, dt);
            synth_joint(tg[c].y, p.y, v.y, a.joint_rate, dt);
            synth_joint(tg[c].z, p.z, v.z, a.joint_rate, dt);
            synth_joint(tg[c].w, p.w, v.w, a.joint_rate, dt);
            v4[c] = v;
            p4[c] = p;
        }
    } else {
        for (int d = 0; d < D; ++d) {
            float p = a.dof_pos[n * D + d], v;
            synth_joint(a.targets[n * D + d], p, v, a.joint_rate, dt);
            a.dof_vel[n * D + d] = v;
            a.dof_pos[n * D + d] = p;
        }
    }
    synth_base_math(a, q4, w0, v0, p0, r, out);
    float* wp = a.ang_vel + 3 * n;
    float* vp = a.lin_vel + 3 * n;
    float* pp = a.pos + 3 * n;
    float* qp = a.quat + 4 * n;
#pragma unroll
    for (int j = 0; j < 3; ++j) { wp[j] = out.w[j]; vp[j] = out.v[j]; pp[j] = out.p[j]; }
#pragma unroll
    for (int j = 0; j < 4; ++j) qp[j] = out.q[j];
}

template <int DV>
__global__ __launch_bounds__(kEnvBlock) void synth_scene_kernel(const GfSynthSceneArgs a) {
    const int64_t n = (int64_t)blockIdx.x * kEnvBlock + threadIdx.x;
    if (n >= a.num_envs) return;
    SynthBase b;
    synth_state_body<DV>(a, n, b);
}

// A scene without per-link outputs or contacts (the benchmark's): workgroup b ticks envs [64b, 64b+64), the tile workgroup b of
// the action and post-physics kernels owns, so with round-robin workgroup → XCD placement a tile stays on one XCD across the step.
template <int DV>
__global__ __launch_bounds__(kSynthTileBlock) void synth_scene_tile_kernel(const GfSynthSceneArgs a) {
    __shared__ float s3[3][GF_WAVE * 3];
    const int64_t n0 = (int64_t)blockIdx.x * GF_WAVE;
    const int rows = (int)((int64_t)a.num_envs - n0 < GF_WAVE ? (int64_t)a.num_envs - n0 : GF_WAVE);
    SynthBase b;
    synth_tick_tile<DV, GF_WAVE>(a, GfActionArgs{}, n0, rows, (int)threadIdx.x, s3, b);
}

// The action phase and the tick of a recorded step in ONE launch (gf_run_ops folds an action op directly in front of a scene op):
// the `upkeep` leading workgroups keep the statistics ring as they do in action_kernel, tile b is workgroup b + upkeep (upkeep is
// a multiple of 8: the tile stays on its XCD).  Same statements per element as the two launches, so the same bits.
template <int DV>
__global__ __launch_bounds__(kSynthTileBlock) void action_scene_tile_kernel(const GfActionArgs act, const GfSynthSceneArgs a, const int upkeep) {
    if ((int)blockIdx.x < upkeep) {
        action_upkeep(act, upkeep);
        return;
    }
    __shared__ float s3[3][GF_WAVE * 3];
    const int64_t n0 = (int64_t)(blockIdx.x - upkeep) * GF_WAVE;
    const int rows = (int)((int64_t)a.num_envs - n0 < GF_WAVE ? (int64_t)a.num_envs - n0 : GF_WAVE);
    SynthBase b;
    synth_tick_tile<DV, GF_WAVE, true>(a, act, n0, rows, (int)threadIdx.x, s3, b);
}

// Per-link outputs (orientation, velocity, position of scene link l of env n; flat index gid = n·NL + l) from the base state the
// tick just produced: consecutive lanes write consecutive floats.
__device__ __forceinline__ void synth_link_one(const GfSynthSceneArgs& a, const int64_t gid, const int l, const float* b /* p3 q4 v3 w3 */) {
    const V3 p{b[0], b[1], b[2]}, v{b[7], b[8], b[9]}, w{b[10], b[11], b[12]};
    if (a.links_quat_out) reinterpret_cast<float4*>(a.links_quat_out)[gid] = make_float4(b[3], b[4], b[5], b[6]);
    if (a.links_vel_out) {
        float* o = a.links_vel_out + gid * 3;
        o[0] = v.x + (float)(l % 3 == 0 ? 1 : 0) * 0.05f * w.x;
        o[1] = v.y + (float)(l % 3 == 1 ? 1 : 0) * 0.05f * w.y;
        o[2] = v.z + (float)(l % 3 == 2 ? 1 : 0) * 0.05f * w.z;
    }
    if (a.links_pos_out) {
        const LinkOffset o = synth_link_offset(l);
        const float wl = l % 3 == 0 ? w.x : (l % 3 == 1 ? w.y : w.z);
        float* lp = a.links_pos_out + gid * 3;
        lp[0] = p.x + o.x;
        lp[1] = p.y + o.y;
        lp[2] = (p.z + o.z) + 0.03f * wl;
    }
}

// Sampled contact of slot c of env n (flat index k = n·C + c): 32 B of output per lane, coalesced.  The second Philox block only
// feeds the z force of an ACTIVE slot; an empty slot's outputs are constants, so it is skipped for waves without an active slot.
// foot_link_mask != 0 selects the walking model (gf_step.h, GfSynthSceneArgs): the k-th foot owns slot k and touches the ground in
// the stance half of a 20-tick trot cycle; the ground sits on side a or side b of a contact at random.
__device__ __forceinline__ void synth_contact_one(const GfSynthSceneArgs& a, const int64_t k, const uint32_t genv, const int c, const float p0, const float p1) {
    const int NL = a.num_scene_links;
    const uint32_t col = (uint32_t)(8 + 8 * c);
    // columns col..col+3 share one Philox block, col+4 starts the next
    const U4 r0 = philox4x32_10(genv, col >> 2, (uint32_t)a.tick, (uint32_t)(a.tick >> 32), (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
    const float u_act = u24_to_unit(r0.x), u_link = u24_to_unit(r0.y);
    const uint32_t feet = a.foot_link_mask;
    bool active = u_act < a.contact_prob;
    int lb = 1 + (int)(u_link * (float)(NL - 1));
    bool robot_on_a = false, foot_slot = false;
    float fz = 0.0f;
    if (feet) {
        const int n_feet = __builtin_popcount(feet);
        if (c < n_feet) {
            uint32_t m = feet;
            for (int j = 0; j < c; ++j) m &= m - 1u;
            lb = __builtin_ctz(m);
            const uint32_t ph = ((uint32_t)a.tick + genv * 7u) % 20u;
            const bool pair_a = ((c ^ (c >> 1)) & 1) == 0;
            const bool stance = pair_a ? ph < 10u : ph >= 10u;
            const float p = stance ? fminf(1.8f * a.foot_contact_prob, 1.0f) : 0.2f * a.foot_contact_prob;
            active = u_act < p;
            robot_on_a = u_link < 0.5f;
            // a foot slot takes its normal force from the same draw as its side (both halves of [0, 1) map onto [0, 1), exactly):
            // every wave holds foot slots, so a second Philox block for them would be paid by every lane of every wave
            fz = robot_on_a ? u_link * 2.0f : u_link * 2.0f - 1.0f;
            foot_slot = true;
        } else {
            const int kk = (int)(u_link * (float)(2 * (NL - 1)));
            lb = 1 + (kk >> 1);
            robot_on_a = (kk & 1) != 0;
        }
    }
    if (active && !foot_slot) {
        const U4 r1 = philox4x32_10(genv, (col >> 2) + 1, (uint32_t)a.tick, (uint32_t)(a.tick >> 32), (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
        fz = u24_to_unit(r1.x);
    }
    const float fx = u24_to_unit(r0.z) * 2.0f - 1.0f, fy = u24_to_unit(r0.w) * 2.0f - 1.0f;
    if (lb > NL - 1) lb = NL - 1;
    // the stored force is the force on link_b: with the robot link on side a it is the reaction
    const float sx = fx * a.contact_force * 0.25f, sy = fy * a.contact_force * 0.25f, sz = fz * a.contact_force;
    a.link_a_out[k] = active ? (robot_on_a ? lb : 0) : -1;
    a.link_b_out[k] = active ? (robot_on_a ? 0 : lb) : -1;
    a.contact_force_out[k * 3 + 0] = active ? (robot_on_a ? -sx : sx) : 0.0f;
    a.contact_force_out[k * 3 + 1] = active ? (robot_on_a ? -sy : sy) : 0.0f;
    a.contact_force_out[k * 3 + 2] = active ? (robot_on_a ? -sz : sz) : 0.0f;
    a.contact_pos_out[k * 3 + 0] = active ? p0 + fx * 0.2f : 0.0f;
    a.contact_pos_out[k * 3 + 1] = active ? p1 + fy * 0.2f : 0.0f;
    a.contact_pos_out[k * 3 + 2] = 0.0f;
}

// A scene with per-link outputs and / or contacts, as ONE launch (two until round 2: the state tick, then a flat kernel over
// (env, link) and (env, slot) pairs that read the new base state back): workgroup b owns envs [64b, 64b+64) — the tick of
// synth_tick_tile (SPLIT; wave 0 alone with the lane-per-env body otherwise, GF_SCENE_LEGACY=1) leaves their new base state in
// LDS, then all four waves write the tile's link rows and contact slots, which are contiguous in memory.  Same statements per
// element, so the outputs are bit-identical to the two-launch version and the oracle.
// TE = envs per workgroup: 64 (the tile of the action / post-physics kernels, same XCD) when that still fills the chip, 16 below
// ~32 k envs (4 096 envs are 64 tiles of 64 — a quarter of the CUs — but 256 tiles of 16).
template <int DV, int TE, bool SPLIT, bool FOLD = false>
__device__ __forceinline__ void synth_tile_body(const GfSynthSceneArgs& a, const GfActionArgs& act, const int64_t n0, const int links, const int contacts,
                                                float (&s_base)[TE][13], float (&s3)[3][SPLIT ? TE * 3 : 1]) {
    static_assert(SPLIT || !FOLD, "only the split tick folds the action phase");
    const int rows = (int)((int64_t)a.num_envs - n0 < TE ? (int64_t)a.num_envs - n0 : TE);
    const int tid = threadIdx.x;
    SynthBase b;
    if constexpr (SPLIT) synth_tick_tile<DV, TE, FOLD>(a, act, n0, rows, tid, s3, b);
    else if (tid < rows) synth_state_body<DV>(a, n0 + tid, b);
    if (tid < rows) {
        float* r = s_base[tid];
        r[0] = b.p[0]; r[1] = b.p[1]; r[2] = b.p[2];
        r[3] = b.q[0]; r[4] = b.q[1]; r[5] = b.q[2]; r[6] = b.q[3];
        r[7] = b.v[0]; r[8] = b.v[1]; r[9] = b.v[2];
        r[10] = b.w[0]; r[11] = b.w[1]; r[12] = b.w[2];
    }
    __syncthreads();
    if (links) {
        const int NL = a.num_scene_links;
        for (int i = tid; i < rows * NL; i += kSynthTileBlock) {
            const int e = i / NL, l = i - e * NL;
            synth_link_one(a, n0 * NL + i, l, s_base[e]);
        }
    }
    if (contacts) {
        const int C = a.num_contacts;
        for (int i = tid; i < rows * C; i += kSynthTileBlock) {
            const int e = i / C, c = i - e * C;
            synth_contact_one(a, n0 * C + i, (uint32_t)(n0 + e) + a.env_offset, c, s_base[e][0], s_base[e][1]);
        }
    }
}

template <int DV, int TE, bool SPLIT>
__global__ __launch_bounds__(kSynthTileBlock) void synth_tile_kernel(const GfSynthSceneArgs a, const int links, const int contacts) {
    __shared__ float s_base[TE][13];   // p(3) q(4) v(3) w(3)
    __shared__ float s3[3][SPLIT ? TE * 3 : 1];
    synth_tile_body<DV, TE, SPLIT>(a, GfActionArgs{}, (int64_t)blockIdx.x * TE, links, contacts, s_base, s3);
}

// … and with the action phase folded in, as action_scene_tile_kernel
template <int DV, int TE>
__global__ __launch_bounds__(kSynthTileBlock) __attribute__((amdgpu_num_sgpr(96))) void action_synth_tile_kernel(const GfActionArgs act, const GfSynthSceneArgs a, const int links, const int contacts,
                                                                            const int upkeep) {
    if ((int)blockIdx.x < upkeep) {
        action_upkeep(act, upkeep);
        return;
    }
    __shared__ float s_base[TE][13];
    __shared__ float s3[3][TE * 3];
    synth_tile_body<DV, TE, true, true>(a, act, (int64_t)(blockIdx.x - upkeep) * TE, links, contacts, s_base, s3);
}

// host side of the fold (gf_action.hip)
int action_validate(const GfActionArgs* a);
bool action_vec4(const GfActionArgs* a);
bool action_const4(const GfActionArgs* a);

static bool env_switch_on(const char* name) {   // set, not empty and not "0"; read per call so one process can run both ways
    const char* v = getenv(name);
    return v && v[0] && strcmp(v, "0") != 0;
}

struct SynthPlan {
    bool links, contacts, small;
    int dv;
};
static SynthPlan synth_plan(const GfSynthSceneArgs* a) {
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    const bool rows16 = (a->num_dofs % 4 == 0) && al16(a->targets) && al16(a->dof_pos) && al16(a->dof_vel);
    SynthPlan p;
    p.links = (a->links_quat_out || a->links_vel_out || a->links_pos_out) && a->num_scene_links > 0;
    p.contacts = a->num_contacts > 0 && a->contact_force_out;
    p.dv = !rows16 ? 0 : (a->num_dofs == 12 ? 3 : (a->num_dofs == 28 ? 7 : 0));
    p.small = a->num_envs < 32768;
    return p;
}

// What gf_synth_scene_step checks before it launches
int scene_validate(const GfSynthSceneArgs* a) {
    if (!a || !a->pos || !a->quat || !a->lin_vel || !a->ang_vel || !a->dof_pos || !a->dof_vel || !a->targets) return GF_E_NULL;
    if (a->num_envs < 0 || a->num_dofs <= 0 || a->num_contacts < 0) return GF_E_RANGE;
    if (a->num_contacts > 0 && a->contact_force_out && (!a->contact_pos_out || !a->link_a_out || !a->link_b_out || a->num_scene_links < 2)) return GF_E_NULL;
    if (reinterpret_cast<uintptr_t>(a->quat) & 15u) return GF_E_UNSUPPORTED;
    if (a->links_quat_out && (reinterpret_cast<uintptr_t>(a->links_quat_out) & 15u)) return GF_E_UNSUPPORTED;
    return GF_OK;
}

// The conditions under which gf_run_ops runs an action op `act` directly in front of a scene op `a` inside the tick's launch, for its
// two peepholes (action_scene_try below; step_fold_try, gf_post.hip, which takes the post-physics op behind the pair along).
// Returns 0: the pair does not fold; 1: the action op fails its entry point's validation (*rc); 2: the scene op fails its validation
// (*rc); 3: the pair folds as planned in *plan.  Nothing is enqueued.
// Both ops are validated BEFORE the fold conditions are looked at, so with the switches in their default position an invalid scene op
// behind a valid action op leaves nothing enqueued even for a pair that would never fold (D = 5, say); when the peephole is off
// (GF_FOLD_ACTION=0, GF_SCENE_LEGACY, a profiled action / scene phase: 0 is returned before any validation) the action launch is
// enqueued and then the scene op fails, as it always did.  The return codes and the failed index are the same either way.
// GF_FOLD_ACTION=0 keeps the two launches (A/B runs, tests/test_action_fold.py).
int action_scene_launch(const GfActionArgs* act, const GfSynthSceneArgs* a, const ActionScenePlan& p, hipStream_t s);
int action_scene_check(const GfActionArgs* act, const GfSynthSceneArgs* a, int* rc, ActionScenePlan* plan) {
    const char* sw = getenv("GF_FOLD_ACTION");
    if (sw && strcmp(sw, "0") == 0) return 0;
    if (env_switch_on("GF_SCENE_LEGACY")) return 0;
    if (g_prof.phase == GF_PHASE_ACTION || g_prof.phase == GF_PHASE_SCENE) return 0;   // a profiled phase keeps its own launch
    if ((*rc = action_validate(act)) != GF_OK) return 1;
    if ((*rc = scene_validate(a)) != GF_OK) return 2;
    if (act->num_envs <= 0 || act->num_envs != a->num_envs || act->num_dofs != a->num_dofs || a->targets != act->targets) return 0;
    if (!action_vec4(act) || !action_const4(act)) return 0;
    const SynthPlan p = synth_plan(a);
    if (p.dv == 0) return 0;
    plan->dv = p.dv;
    plan->links = p.links;
    plan->contacts = p.contacts;
    plan->small = p.small;
    plan->upkeep = action_upkeep_blocks(act);
    return 3;
}

// gf_run_ops, action op `act` directly in front of scene op `a`: run the pair as one launch when that is possible.
// Returns 0: not folded, nothing enqueued — the caller runs the two ops through their entry points as ever;
//         1: the action op fails its entry point's validation (*rc), nothing enqueued;
//         2: the scene op fails its validation (*rc), nothing enqueued — or both ops are done, in one launch (*rc its status).
int action_scene_try(const GfActionArgs* act, const GfSynthSceneArgs* a, hipStream_t s, int* rc) {
    ActionScenePlan p;
    const int chk = action_scene_check(act, a, rc, &p);
    if (chk != 3) return chk;
    *rc = action_scene_launch(act, a, p, s);
    return 2;
}

// the pair's one launch, as action_scene_check planned it; returns the launch's status
int action_scene_launch(const GfActionArgs* act, const GfSynthSceneArgs* a, const ActionScenePlan& p, hipStream_t s) {
    const int upkeep = p.upkeep;
    const dim3 tb(kSynthTileBlock);
    if (p.links || p.contacts) {
        const dim3 tg(env_grid(a->num_envs, p.small ? 16 : 64) + upkeep);
#define GF_FOLD_TILE(DVV)                                                                                                        \
        if (p.small) klaunch(action_synth_tile_kernel<DVV, 16>, tg, tb, 0, s, *act, *a, (int)p.links, (int)p.contacts, upkeep);   \
        else klaunch(action_synth_tile_kernel<DVV, 64>, tg, tb, 0, s, *act, *a, (int)p.links, (int)p.contacts, upkeep)
        if (p.dv == 3) { GF_FOLD_TILE(3); } else { GF_FOLD_TILE(7); }
#undef GF_FOLD_TILE
    } else {
        const dim3 tg(env_grid(a->num_envs) + upkeep);
        if (p.dv == 3) klaunch(action_scene_tile_kernel<3>, tg, tb, 0, s, *act, *a, upkeep);
        else klaunch(action_scene_tile_kernel<7>, tg, tb, 0, s, *act, *a, upkeep);
    }
    return launch_status();
}

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_entity_rotate(const GfRotateArgs* a, void* stream) {
    if (!a || !a->out || !a->entity.quat) return GF_E_NULL;
    if (a->what < GF_ROT_PROJ_GRAVITY || a->what > GF_ROT_ANG_VEL || a->num_envs < 0) return GF_E_RANGE;
    if (a->what == GF_ROT_LIN_VEL && !a->entity.lin_vel) return GF_E_NULL;
    if (a->what == GF_ROT_ANG_VEL && !a->entity.ang_vel) return GF_E_NULL;
    if (reinterpret_cast<uintptr_t>(a->entity.quat) & 15u) return GF_E_UNSUPPORTED;
    if (a->num_envs == 0) return GF_OK;
    hipStream_t s = (hipStream_t)stream;
    gf::PhaseScope scope(GF_PHASE_ROTATE, s);
    scope.begin_bracket();
    gf::klaunch(gf::rotate_kernel, dim3(gf::env_grid(a->num_envs)), dim3(gf::kEnvBlock), 0, s, *a);
    return gf::launch_status();
}

extern "C" __attribute__((visibility("default"))) int gf_synth_scene_step(const GfSynthSceneArgs* a, void* stream) {
    const int valid = gf::scene_validate(a);
    if (valid != GF_OK) return valid;
    if (a->num_envs == 0) return GF_OK;
    hipStream_t s = (hipStream_t)stream;
    gf::PhaseScope scope(GF_PHASE_SCENE, s);
    scope.begin_bracket();
    const unsigned grid = gf::env_grid(a->num_envs);
    const gf::SynthPlan plan = gf::synth_plan(a);
    const bool links = plan.links, contacts = plan.contacts, small = plan.small;
    const int dv = plan.dv;
    // GF_SCENE_LEGACY=1: the lane-per-env tick (A/B runs and tests/test_scene_tile.py); read per call so one process can run both
    const bool legacy = gf::env_switch_on("GF_SCENE_LEGACY");
    if (links || contacts) {   // tick + per-link rows + contact slots of a 64-env tile in one launch
        const dim3 tb(gf::kSynthTileBlock);
        const dim3 tg(small ? gf::env_grid(a->num_envs, 16) : grid);
#define GF_SYNTH_TILE(DVV, SPLIT)                                                                                      \
        if (small) gf::klaunch(gf::synth_tile_kernel<DVV, 16, SPLIT>, tg, tb, 0, s, *a, (int)links, (int)contacts);   \
        else gf::klaunch(gf::synth_tile_kernel<DVV, 64, SPLIT>, tg, tb, 0, s, *a, (int)links, (int)contacts)
        if (legacy) {
            if (dv == 3) { GF_SYNTH_TILE(3, false); } else if (dv == 7) { GF_SYNTH_TILE(7, false); } else { GF_SYNTH_TILE(0, false); }
        } else {
            if (dv == 3) { GF_SYNTH_TILE(3, true); } else if (dv == 7) { GF_SYNTH_TILE(7, true); } else { GF_SYNTH_TILE(0, true); }
        }
#undef GF_SYNTH_TILE
    } else if (legacy) {
        if (dv == 3) gf::klaunch(gf::synth_scene_kernel<3>, dim3(grid), dim3(gf::kEnvBlock), 0, s, *a);
        else if (dv == 7) gf::klaunch(gf::synth_scene_kernel<7>, dim3(grid), dim3(gf::kEnvBlock), 0, s, *a);
        else gf::klaunch(gf::synth_scene_kernel<0>, dim3(grid), dim3(gf::kEnvBlock), 0, s, *a);
    } else {   // one 64-env tile per 256-lane workgroup
        const dim3 tb(gf::kSynthTileBlock);
        if (dv == 3) gf::klaunch(gf::synth_scene_tile_kernel<3>, dim3(grid), tb, 0, s, *a);
        else if (dv == 7) gf::klaunch(gf::synth_scene_tile_kernel<7>, dim3(grid), tb, 0, s, *a);
        else gf::klaunch(gf::synth_scene_tile_kernel<0>, dim3(grid), tb, 0, s, *a);
    }
    return gf::launch_status();
}
