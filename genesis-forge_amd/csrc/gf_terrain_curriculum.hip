// gf_terrain_curriculum.hip — gf_terrain_curriculum: the terrain curriculum's promote / demote / respawn for the flagged envs
// (managers/terrain_curriculum.py, mdp.reset.terrain_curriculum_position), in one launch.  include/gf_step.h has the contract.
//
// Composed from torch the same bookkeeping is about forty small launches over index lists (nonzero, gathers, a norm, compares, a
// randint, wheres, scatters, two rands, the height launch, xyz_to_quat and more scatters).  Here a lane owns an env, as in the masked
// reset: a wave reads its 64 mask bytes, takes a ballot and leaves when no lane is flagged — at the 0.3-0.5 % of envs a step resets
// that is all most waves do.  A flagged lane reads its base position, spawn point, level, type and reference speed (five independent
// loads, in flight together), decides the level, takes its draws (two Philox blocks at most, or a dense parity row), places itself in
// its cell, samples the height through terrain_height() of gf_device.h — the function every other terrain query of the library
// inlines, so z equals gf_terrain_height at the kernel's own (x, y) bit for bit — and writes its rows.  Nothing is shared between
// lanes, so there is no LDS; the three counters are one vector atomicAdd per wave and counter from the ballots' popcounts.
// A workgroup is four waves (256 envs): the waves are independent, the width only keeps the grid at one workgroup per CU at 65 536 envs.
#include "gf_launch.h"

namespace gf {

constexpr int kTcBlock = GF_TERRAIN_CURRICULUM_BLOCK_ENVS;

__global__ __launch_bounds__(kTcBlock) void terrain_curriculum_kernel(const GfTerrainCurriculumArgs a) {
    const int lane = (int)(threadIdx.x & (GF_WAVE - 1));
    const int64_t n = (int64_t)blockIdx.x * kTcBlock + (int64_t)threadIdx.x;
    const bool go = n < a.num_envs && (G(a.mask)[n] || (a.mask2 && G(a.mask2)[n]));
    if (!__ballot(go)) return;   // wave-uniform

    bool up = false, down = false, wrapped = false;
    if (go) {
        const GF_GLOBAL float* pin = G(a.pos_in) + 3 * n;
        GF_GLOBAL float* sxy = G(a.spawn_xy) + 2 * n;
        const float bx = pin[0], by = pin[1];
        const float ox = sxy[0], oy = sxy[1];
        int l = G(a.level)[n];
        const int ty = G(a.type)[n];
        const float ref = a.speed_ref ? G(a.speed_ref)[n] : 0.0f;

        // 1, 2: distance walked and the level change
        if (a.update) {
            const float dx = bx - ox, dy = by - oy;
            const float dist = sqrtf(dx * dx + dy * dy);
            up = dist > a.promote_distance;
            const float thr = a.speed_ref ? ref * a.demote_time : a.demote_distance;
            down = !up && dist < thr;
            l = l + (up ? 1 : 0) - (down ? 1 : 0);
        }

        // 3: the draws (x, y, rot x, rot y, rot z, level)
        float u[6];
        if (a.draws) {
            const GF_GLOBAL float* d = G(a.draws) + 6 * n;
#pragma unroll
            for (int j = 0; j < 6; ++j) u[j] = d[j];
        } else {
            const uint32_t genv = (uint32_t)n + a.env_offset;
            const U4 r0 = philox4x32_10(genv, GF_SPAWN_BLOCK, (uint32_t)a.stream, (uint32_t)(a.stream >> 32), (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
            u[0] = u24_to_unit(r0.x); u[1] = u24_to_unit(r0.y); u[4] = u24_to_unit(r0.z); u[5] = u24_to_unit(r0.w);
            u[2] = 0.0f; u[3] = 0.0f;
            if (a.spawn_rot_mask & 3) {
                const U4 r1 = philox4x32_10(genv, GF_SPAWN_BLOCK + 1u, (uint32_t)a.stream, (uint32_t)(a.stream >> 32), (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
                u[2] = u24_to_unit(r1.x); u[3] = u24_to_unit(r1.y);
            }
        }

        // 4: past the top level -> a random level; below the bottom -> the bottom
        if (a.update) {
            if (l >= a.num_levels) {
                const int r = (int)(u[5] * (float)a.num_levels);
                l = r < a.num_levels - 1 ? r : a.num_levels - 1;
                wrapped = true;
            }
            if (l < 0) l = 0;
        }

        // 5, 6: the cell and the position inside it
        const int ix = a.level_axis == 0 ? l : ty, iy = a.level_axis == 0 ? ty : l;
        const float x = (u[0] * a.spawn_x_span + a.spawn_x_min) + (float)ix * a.cell_dx;
        const float y = (u[1] * a.spawn_y_span + a.spawn_y_min) + (float)iy * a.cell_dy;
        const float z = terrain_height(a.terrain, x, y) + a.height_offset;

        // 8: the writes
        GF_GLOBAL float* pout = G(a.pos_out) + 3 * n;
        pout[0] = x; pout[1] = y; pout[2] = z;
        if (a.set_quat) {
            // 7: spawn_pose's orientation rule
            const int m = a.spawn_rot_mask;
            const float rx = (m & 1) ? uniform_range(u[2], a.spawn_rot_lo[0], a.spawn_rot_hi[0]) : 0.0f;
            const float ry = (m & 2) ? uniform_range(u[3], a.spawn_rot_lo[1], a.spawn_rot_hi[1]) : 0.0f;
            const float rz = (m & 4) ? uniform_range(u[4], a.spawn_rot_lo[2], a.spawn_rot_hi[2]) : 0.0f;
            const float4 q = xyz_to_quat_det(rx, ry, rz);
            GF_GLOBAL f32x4* qp = reinterpret_cast<GF_GLOBAL f32x4*>(G(a.quat_out)) + n;
            if (a.quat_stash) reinterpret_cast<GF_GLOBAL f32x4*>(G(a.quat_stash))[n] = *qp;   // pre-reset quat for this tick's observation
            f32x4 qv;
            qv.x = q.x; qv.y = q.y; qv.z = q.z; qv.w = q.w;
            *qp = qv;
        }
        if (a.zero_velocity) {
            if (a.lin_vel) for (int j = 0; j < 3; ++j) G(a.lin_vel)[3 * n + j] = 0.0f;
            if (a.ang_vel) for (int j = 0; j < 3; ++j) G(a.ang_vel)[3 * n + j] = 0.0f;
            if (a.dof_vel) for (int d = 0; d < a.num_dofs; ++d) G(a.dof_vel)[n * a.num_dofs + d] = 0.0f;
        }
        sxy[0] = x; sxy[1] = y;
        G(a.level)[n] = l;
        if (a.command.command) {   // the command the new episode starts with (the old reference speed was read above)
            const GF_GLOBAL float* c = G(a.command.command) + n * (int64_t)cmd_stride(a.command);
            const float cx = c[0], cy = c[1];
            G(a.speed_ref)[n] = sqrtf(cx * cx + cy * cy);
        }
    }
    // the counters: one vector atomic per wave and counter that has something to add (update = 0 adds nothing)
    const unsigned long long bu = __ballot(up), bd = __ballot(down), bw = __ballot(wrapped);
    if (lane == 0) {
        if (bu) atomicAdd(a.counts + 0, popc64(bu));
        if (bd) atomicAdd(a.counts + 1, popc64(bd));
        if (bw) atomicAdd(a.counts + 2, popc64(bw));
    }
}

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_terrain_curriculum_sizeof(void) { return (int)sizeof(GfTerrainCurriculumArgs); }

extern "C" __attribute__((visibility("default"))) int gf_terrain_curriculum(const GfTerrainCurriculumArgs* a, void* stream) {
    if (!a || !a->mask || !a->pos_in || !a->pos_out || !a->spawn_xy || !a->level || !a->type || !a->counts) return GF_E_NULL;
    if (a->set_quat == 1 && !a->quat_out) return GF_E_NULL;
    if (a->command.command && !a->speed_ref) return GF_E_NULL;
    const int64_t blocks = a->num_envs < 0 ? -1 : (a->num_envs + gf::kTcBlock - 1) / gf::kTcBlock;
    if (blocks < 0 || blocks > 0x7fffffff) return GF_E_RANGE;
    if (a->num_levels < 1 || a->num_types < 1 || a->num_dofs < 0) return GF_E_RANGE;
    if ((a->level_axis != 0 && a->level_axis != 1) || (a->update != 0 && a->update != 1) || (a->set_quat != 0 && a->set_quat != 1)) return GF_E_RANGE;
    // (written so that a NaN fails: only a finite, non-negative threshold passes)
    if (!(a->promote_distance >= 0.0f && a->promote_distance <= 3.4028234663852886e38f)) return GF_E_RANGE;
    if (!(a->demote_time >= 0.0f && a->demote_time <= 3.4028234663852886e38f)) return GF_E_RANGE;
    if (!(a->demote_distance >= 0.0f && a->demote_distance <= 3.4028234663852886e38f)) return GF_E_RANGE;
    if (a->terrain.height_field && (a->terrain.rows < 1 || a->terrain.cols < 1)) return GF_E_RANGE;
    if (a->command.command && (a->command.width < 2 || (a->command.stride != 0 && a->command.stride < a->command.width))) return GF_E_RANGE;
    // a quaternion moves as one 16-byte unit
    if (a->set_quat && (reinterpret_cast<uintptr_t>(a->quat_out) & 15u)) return GF_E_UNSUPPORTED;
    if (a->set_quat && a->quat_stash && (reinterpret_cast<uintptr_t>(a->quat_stash) & 15u)) return GF_E_UNSUPPORTED;
    if (a->num_envs == 0) return GF_OK;
    hipStream_t s = (hipStream_t)stream;
    gf::PhaseScope scope(GF_PHASE_TERRAIN, s);
    GF_LAUNCH(scope, gf::terrain_curriculum_kernel, (unsigned)blocks, gf::kTcBlock, 0, s, *a);
    return gf::launch_status();
}
