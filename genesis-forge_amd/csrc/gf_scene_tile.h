// gf_scene_tile.h — the stand-in scene's tick of a 64-env (or 16-env) tile by a 256-lane workgroup, with or without the action phase
// folded in (gf_action_row.h).  Shared by gf_scene.hip (the scene and action-scene kernels) and gf_post_ws.h (the post-physics
// kernel's tick prologue: a recorded step as one launch), so every kernel that ticks a tile runs the same statements per element in
// the same order and gives the oracle's bits.
#pragma once

#include "gf_action_row.h"

namespace gf {

// the base state an env's tick leaves: position, quaternion, linear and angular velocity
struct SynthBase {
    float p[3], q[4], v[3], w[3];
};

// The two Philox blocks of an env's tick: columns 0..5 (block 0: x,y,z,w, block 1: x,y) are its six base-motion draws
struct SynthDraws {
    U4 b0, b1;
};
__device__ __forceinline__ SynthDraws synth_draws(const GfSynthSceneArgs& a, const uint32_t genv) {
    return SynthDraws{philox4x32_10(genv, 0u, (uint32_t)a.tick, (uint32_t)(a.tick >> 32), (uint32_t)a.seed, (uint32_t)(a.seed >> 32)),
                      philox4x32_10(genv, 1u, (uint32_t)a.tick, (uint32_t)(a.tick >> 32), (uint32_t)a.seed, (uint32_t)(a.seed >> 32))};
}

// The base part of one env's tick: damped random walk of the velocities, position and quaternion integration.  Every kernel
// that ticks the base goes through this one copy of the statements, so they all give the oracle's bits.
__device__ __forceinline__ void synth_base_math(const GfSynthSceneArgs& a, const float4 q4, const V3 w0, const V3 v0, const V3 p0,
                                                const SynthDraws& r, SynthBase& out) {
    const float dt = a.dt;
    const U4 b0 = r.b0, b1 = r.b1;
    const float s[6] = {u24_to_unit(b0.x) * 2.0f - 1.0f, u24_to_unit(b0.y) * 2.0f - 1.0f, u24_to_unit(b0.z) * 2.0f - 1.0f,
                        u24_to_unit(b0.w) * 2.0f - 1.0f, u24_to_unit(b1.x) * 2.0f - 1.0f, u24_to_unit(b1.y) * 2.0f - 1.0f};
    float w[3] = {w0.x, w0.y, w0.z}, v[3] = {v0.x, v0.y, v0.z}, p[3] = {p0.x, p0.y, p0.z};
#pragma unroll
    for (int j = 0; j < 3; ++j) w[j] = w[j] * 0.9f + s[j] * a.ang_noise;
    v[0] = v[0] * 0.9f + s[3] * a.lin_noise;
    v[1] = v[1] * 0.9f + s[4] * a.lin_noise;
    v[2] = (v[2] * 0.9f + (a.height_target - p[2]) * 2.0f) + s[5] * a.lin_noise;
#pragma unroll
    for (int j = 0; j < 3; ++j) p[j] = p[j] + v[j] * dt;
    const float h = 0.5f * dt;
    const float qw = q4.x, qx = q4.y, qy = q4.z, qz = q4.w;
    const float dw = ((-(w[0] * qx)) - w[1] * qy) - w[2] * qz;
    const float dx = (w[0] * qw + w[1] * qz) - w[2] * qy;
    const float dy = (w[1] * qw + w[2] * qx) - w[0] * qz;
    const float dz = (w[2] * qw + w[0] * qy) - w[1] * qx;
    float nq[4] = {qw + dw * h, qx + dx * h, qy + dy * h, qz + dz * h};
    const float nrm = sqrtf(((nq[0] * nq[0] + nq[1] * nq[1]) + nq[2] * nq[2]) + nq[3] * nq[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) nq[j] = nq[j] / nrm;
#pragma unroll
    for (int j = 0; j < 3; ++j) { out.w[j] = w[j]; out.v[j] = v[j]; out.p[j] = p[j]; }
#pragma unroll
    for (int j = 0; j < 4; ++j) out.q[j] = nq[j];
}

// One joint of the first-order tracking lag: v = (target - pos) * rate, pos += v * dt
__device__ __forceinline__ void synth_joint(float t, float& p, float& v, float rate, float dt) {
    v = (t - p) * rate;
    p = p + v * dt;
}

// ---------------------------------------------------------------------------------------------
// The tick of a tile of TE envs [n0, n0 + rows) by a 256-lane workgroup, split by wave:
//  * waves 1-3 stream the tile's joint rows.  targets / dof_pos / dof_vel of the tile are one contiguous block of rows·D floats
//    each, so lane t takes float4 t, t + 192, … (DV > 0) or float t, t + 192, … (DV = 0): every access is a whole 1 KiB (float4)
//    per wave instruction, where the lane-per-env tick read 48 B-strided records and kept the stream waiting behind the Philox work;
//  * wave 0 ticks the base with lane = env.  The tile's pos / lin_vel / ang_vel are contiguous blocks of rows·3 floats: they are
//    read and written as consecutive floats by consecutive lanes and transposed through LDS, the quaternions are one float4 per
//    lane already.  The Philox blocks are computed while those loads are in flight.
// The statements per element are the lane-per-env tick's, so the outputs are bit-identical to it and to the oracle.
// ---------------------------------------------------------------------------------------------
constexpr int kSynthTileBlock = 256;
constexpr int kSynthDofLanes = kSynthTileBlock - GF_WAVE;

// orders one wave's LDS accesses across lanes: LDS serves a wave's instructions in order, so it is enough that the compiler moves
// no LDS access across this point
__device__ __forceinline__ void wave_lds_sync() { __builtin_amdgcn_wave_barrier(); }

// What a tick hands to code that follows it in the same kernel, BESIDES its stores: `dof` is called by the lane that stores float4 i of
// the tile's five joint streams (FOLD only), `base` by lane e of wave 0 with the new base state of env e of the tile, `episode` by the
// same lane with that env's new step counter (FOLD only).  The default takes nothing and compiles to nothing; gf_post_ws.h hands
// the tile to its post-physics phase through LDS.  (The sink is called where the values are stored, inside the wave's branch: a
// result handed back to the caller instead would stay live in wave 0's registers while the other branch of the workgroup runs.)
struct SynthNoSink {
    __device__ __forceinline__ void dof(int, const float4&, const float4&, const float4&, const float4&, const float4&) const {}
    __device__ __forceinline__ void base(int, const SynthBase&) const {}
    __device__ __forceinline__ void episode(int, int32_t) const {}
};

// FOLD: the action phase of the step runs here too (gf_action_row.h).  The lanes that stream the tile's joint rows are the lanes
// that own the same float4s of the flat action stream, so the targets never leave the registers between the two phases: every
// load of the lane (raw actions, previous actions, joint positions) is issued before the first use, the row code runs, the
// bookkeeping rows and the targets are stored as the action kernel stores them, and the joints take the targets from the registers.
template <int DV, int TE, bool FOLD = false, class Sink = SynthNoSink>
__device__ __forceinline__ void synth_dof_tile(const GfSynthSceneArgs& a, const GfActionArgs& act, const int64_t n0, const int rows, const int t,
                                               const Sink& sink = Sink{}) {
    const float dt = a.dt, rate = a.joint_rate;
    if constexpr (FOLD) {
        static_assert(DV > 0, "the fold moves float4s");
        constexpr int kIt = (TE * (DV > 0 ? DV : 1) + kSynthDofLanes - 1) / kSynthDofLanes;
        const int cnt = rows * DV;
        const int64_t f0 = n0 * DV;   // the tile's first float4 in the flat [N·D] streams
        const float4* x4 = reinterpret_cast<const float4*>(act.actions_in) + f0;
        const bool keep = act.env_actions != nullptr;
        float4* e4 = reinterpret_cast<float4*>(keep ? act.env_actions : act.targets) + f0;
        float4* l4 = reinterpret_cast<float4*>(keep ? act.env_last_actions : act.targets) + f0;
        float4* t4 = reinterpret_cast<float4*>(act.targets) + f0;
        float4* p4 = reinterpret_cast<float4*>(a.dof_pos) + f0;
        float4* v4 = reinterpret_cast<float4*>(a.dof_vel) + f0;
        const int mode = act.mode;
        int flags = 0;
        // a lane past the tile re-reads the tile's last float4, and without bookkeeping buffers the raw actions stand in for the
        // previous ones: no branch around the loads, so all of them — with one float4 per lane the constants too, with more their
        // registers are not worth the lost occupancy — are in flight before the first wait
        constexpr bool kConstsFirst = kIt == 1;
        const float4* q4 = keep ? e4 : x4;
        float4 x[kIt], pv[kIt], dp[kIt];
        ActionConsts4 c0;
#pragma unroll
        for (int k = 0; k < kIt; ++k) {
            const int i = t + k * kSynthDofLanes < cnt ? t + k * kSynthDofLanes : cnt - 1;
            x[k] = x4[i];
            pv[k] = q4[i];
            dp[k] = p4[i];
            if constexpr (kConstsFirst) c0 = action_consts4(act, 4 * (i % DV), mode);   // (the tile starts at a row, so DOF = 4·(i mod DV))
        }
#pragma unroll
        for (int k = 0; k < kIt; ++k) {
            const int i = t + k * kSynthDofLanes;
            if constexpr (!kConstsFirst) c0 = action_consts4(act, 4 * ((i < cnt ? i : cnt - 1) % DV), mode);
            float4 last, actions, tg;
            int fl = 0;
            action_row4(act, c0, mode, x[k], pv[k], last, actions, tg, fl);
            float4 v, p = dp[k];
            synth_joint(tg.x, p.x, v.x, rate, dt);
            synth_joint(tg.y, p.y, v.y, rate, dt);
            synth_joint(tg.z, p.z, v.z, rate, dt);
            synth_joint(tg.w, p.w, v.w, rate, dt);
            if (i < cnt) {
                flags |= fl;
                if (keep) { l4[i] = last; e4[i] = actions; }
                t4[i] = tg;
                v4[i] = v;
                p4[i] = p;
                sink.dof(i, last, actions, tg, v, p);
            }
        }
        action_flags_commit(act, flags);   // whole waves get here
    } else if (DV > 0) {
        constexpr int kIt = DV > 0 ? (TE * DV + kSynthDofLanes - 1) / kSynthDofLanes : 1;
        const int cnt = rows * DV;
        const float4* t4 = reinterpret_cast<const float4*>(a.targets) + n0 * DV;
        float4* p4 = reinterpret_cast<float4*>(a.dof_pos) + n0 * DV;
        float4* v4 = reinterpret_cast<float4*>(a.dof_vel) + n0 * DV;
        float4 tg[kIt], dp[kIt];
#pragma unroll
        for (int k = 0; k < kIt; ++k) {
            const int i = t + k * kSynthDofLanes;
            if (i < cnt) { tg[k] = t4[i]; dp[k] = p4[i]; }
        }
#pragma unroll
        for (int k = 0; k < kIt; ++k) {
            const int i = t + k * kSynthDofLanes;
            if (i < cnt) {
                float4 v, p = dp[k];
                synth_joint(tg[k].x, p.x, v.x, rate, dt);
                synth_joint(tg[k].y, p.y, v.y, rate, dt);
                synth_joint(tg[k].z, p.z, v.z, rate, dt);
                synth_joint(tg[k].w, p.w, v.w, rate, dt);
                v4[i] = v;
                p4[i] = p;
            }
        }
    } else {
        const int64_t base = n0 * a.num_dofs;
        const int cnt = rows * a.num_dofs;
        for (int i = t; i < cnt; i += kSynthDofLanes) {
            float p = a.dof_pos[base + i], v;
            synth_joint(a.targets[base + i], p, v, rate, dt);
            a.dof_vel[base + i] = v;
            a.dof_pos[base + i] = p;
        }
    }
}

// wave 0: lane = env of the tile; s3 is this wave's LDS, 3 × [TE·3] floats.  Returns the lane's new base state (lane < rows).
// FOLD: episode_length[n] += 1 of the action phase (genesis_env.py:197) for the lane's env, its load issued with the others.
template <int TE, bool FOLD = false, class Sink = SynthNoSink>
__device__ __forceinline__ void synth_base_tile(const GfSynthSceneArgs& a, const GfActionArgs& act, const int64_t n0, const int rows, const int lane,
                                                float (&s3)[3][TE * 3], SynthBase& out, const Sink& sink = Sink{}) {
    constexpr int kJ = (TE * 3 + GF_WAVE - 1) / GF_WAVE;
    const int cnt = rows * 3;
    float* const pos = a.pos + n0 * 3;
    float* const lin = a.lin_vel + n0 * 3;
    float* const ang = a.ang_vel + n0 * 3;
    // float i of each block, i = lane + 64 j; a lane past the tile re-reads its last float (no branch around the loads)
    float xp[kJ], xv[kJ], xw[kJ];
#pragma unroll
    for (int j = 0; j < kJ; ++j) {
        const int i = lane + j * GF_WAVE < cnt ? lane + j * GF_WAVE : cnt - 1;
        xp[j] = pos[i]; xv[j] = lin[i]; xw[j] = ang[i];
    }
    const bool mine = lane < rows;
    const float4 q4 = load_quat(a.quat, n0 + (mine ? lane : rows - 1));
    int32_t ep = 0;
    if constexpr (FOLD) {   // (without the counter the lane reads a word of its quaternion instead: no branch around the load)
        const int32_t* e = act.episode_length ? act.episode_length : reinterpret_cast<const int32_t*>(a.quat);
        ep = e[n0 + (mine ? lane : rows - 1)];
    }
    const SynthDraws r = synth_draws(a, (uint32_t)(n0 + lane) + a.env_offset);
    // the Philox rounds run while the loads are in flight: the draws are pinned here, ahead of the first LDS write (which waits
    // for the loads); left alone, the compiler sinks the rounds to their first use behind that wait
    asm volatile("" ::"v"(r.b0.x), "v"(r.b0.y), "v"(r.b0.z), "v"(r.b0.w), "v"(r.b1.x), "v"(r.b1.y));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < kJ; ++j) {
        const int i = lane + j * GF_WAVE;
        if (i < TE * 3) { s3[0][i] = xp[j]; s3[1][i] = xv[j]; s3[2][i] = xw[j]; }
    }
    wave_lds_sync();
    const int e = mine ? lane : 0;
    const V3 p0{s3[0][3 * e], s3[0][3 * e + 1], s3[0][3 * e + 2]};
    const V3 v0{s3[1][3 * e], s3[1][3 * e + 1], s3[1][3 * e + 2]};
    const V3 w0{s3[2][3 * e], s3[2][3 * e + 1], s3[2][3 * e + 2]};
    synth_base_math(a, q4, w0, v0, p0, r, out);
    wave_lds_sync();
    if (mine) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { s3[0][3 * lane + j] = out.p[j]; s3[1][3 * lane + j] = out.v[j]; s3[2][3 * lane + j] = out.w[j]; }
    }
    wave_lds_sync();
#pragma unroll
    for (int j = 0; j < kJ; ++j) {
        const int i = lane + j * GF_WAVE;
        const float yp = s3[0][i < TE * 3 ? i : 0], yv = s3[1][i < TE * 3 ? i : 0], yw = s3[2][i < TE * 3 ? i : 0];
        if (i < cnt) { pos[i] = yp; lin[i] = yv; ang[i] = yw; }
    }
    if (mine) {
        reinterpret_cast<float4*>(a.quat)[n0 + lane] = make_float4(out.q[0], out.q[1], out.q[2], out.q[3]);
        sink.base(lane, out);
    }
    if constexpr (FOLD) {
        if (mine && act.episode_length) act.episode_length[n0 + lane] = ep + 1;
        if (mine) sink.episode(lane, ep + 1);
    }
}

// The tick of tile [n0, n0 + rows) by a whole workgroup (see above): wave 0 returns the base state of env n0 + lane in `b`.
// (`act` is read only with FOLD; `sink`: see SynthNoSink)
// `tid` is the lane's index in the tile's work, 0 … 255: threadIdx.x in the scene kernels; role · 64 + lane in a post-physics program
// that rotates its roles over the hardware waves (ws_rotates, gf_post_ws.h) — nothing below reads threadIdx.x itself.
template <int DV, int TE, bool FOLD = false, class Sink = SynthNoSink>
__device__ __forceinline__ void synth_tick_tile(const GfSynthSceneArgs& a, const GfActionArgs& act, const int64_t n0, const int rows, const int tid,
                                                float (&s3)[3][TE * 3], SynthBase& b, const Sink& sink = Sink{}) {
    if (tid >= GF_WAVE) synth_dof_tile<DV, TE, FOLD>(a, act, n0, rows, tid - GF_WAVE, sink);
    else synth_base_tile<TE, FOLD>(a, act, n0, rows, tid, s3, b, sink);
}

}  // namespace gf
