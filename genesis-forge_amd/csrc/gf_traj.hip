// gf_traj.hip — gf_traj_table and gf_traj_gather: the trajectory minibatches of a recurrent policy's update (rsl_rl
// split_and_pad_trajectories / RolloutStorage.recurrent_mini_batch_generator; include/gf_step.h has the contract).
//
// gf_traj_table: ONE workgroup walks the envs kTrajBlock at a time.  A thread counts the trajectories of its env (a done ends one,
// the last step always does), the chunk's counts are scanned — a wave's shuffle scan, the four wave totals through LDS, the carry
// of the chunks before in a register of every thread — and the thread then writes its env's (env, t0, len) entries at its own
// offset.  No atomics: the order is the envs', whatever the schedule.  The dones are read twice, coalesced over the envs of a chunk;
// at 65 536 envs x 24 steps that is 3 MB through one workgroup, once per update.
// gf_traj_gather: grid y = job (0 the actor's padded observations, 1 the critic's, 2 the masks, the un-pad index and the initial
// states), grid-stride over the job's elements with the column fastest, so a row's read and write are contiguous.
#include "gf_launch.h"

namespace gf {

constexpr int kTrajBlock = 256;
constexpr int kTrajWaves = kTrajBlock / GF_WAVE;

__global__ __launch_bounds__(kTrajBlock) void traj_table_kernel(const GfTrajTableArgs a) {
    __shared__ int s_wave[kTrajWaves];
    const int T = a.num_steps, N = a.num_envs;
    const int tid = (int)threadIdx.x, lane = tid & (GF_WAVE - 1), wave = tid >> 6;
    const GF_GLOBAL uint8_t* dones = G(a.dones);
    GF_GLOBAL int32_t* table = G(a.table);
    int carry = 0;   // trajectories of the envs before this chunk (the same in every thread)
    for (int n0 = 0; n0 < N; n0 += kTrajBlock) {
        const int n = n0 + tid;
        int count = 0;
        if (n < N) {
            for (int t = 0; t < T - 1; ++t) count += dones[(int64_t)t * N + n] != 0;
            count += 1;   // (the last step ends a trajectory whether it is done or not)
        }
        int incl = count;   // inclusive scan over the wave, then over the waves
#pragma unroll
        for (int d = 1; d < GF_WAVE; d <<= 1) {
            const int up = __shfl_up(incl, d, GF_WAVE);
            if (lane >= d) incl += up;
        }
        if (lane == GF_WAVE - 1) s_wave[wave] = incl;
        __syncthreads();
        int before = carry, total = 0;
#pragma unroll
        for (int w = 0; w < kTrajWaves; ++w) {
            if (w < wave) before += s_wave[w];
            total += s_wave[w];
        }
        __syncthreads();   // (s_wave is written again in the next chunk)
        const int first = before + incl - count;
        if (n < N) {
            G(a.counts)[n] = count;
            G(a.offsets)[n] = first;
            int j = first, t0 = 0;
            for (int t = 0; t < T; ++t) {
                if (t == T - 1 || dones[(int64_t)t * N + n] != 0) {
                    table[3 * (int64_t)j] = n;
                    table[3 * (int64_t)j + 1] = t0;
                    table[3 * (int64_t)j + 2] = t + 1 - t0;
                    ++j;
                    t0 = t + 1;
                }
            }
        }
        carry += total;
    }
    if (tid == 0) G(a.offsets)[N] = carry;
}

__global__ __launch_bounds__(kTrajBlock) void traj_gather_kernel(const GfTrajGatherArgs a) {
    const int T = a.num_steps, N = a.num_envs, J = a.num_traj;
    const GF_GLOBAL int32_t* table = G(a.table) + 3 * (int64_t)a.first_traj;
    const int64_t stride = (int64_t)gridDim.x * kTrajBlock;
    const int64_t start = (int64_t)blockIdx.x * kTrajBlock + threadIdx.x;
    const int job = (int)blockIdx.y;
    if (job < 2) {   // padded observations [T, J, W]: row (s, j) is step t0 + s of trajectory j, zeros from its length on
        const GfTrajGroup& g = a.groups[job];
        const int W = g.width;
        if (W == 0 || !g.dst) return;
        const int64_t total = (int64_t)T * J * W;
        for (int64_t e = start; e < total; e += stride) {
            const int64_t row = e / W;
            const int col = (int)(e - row * W);
            const int s = (int)(row / J), j = (int)(row - (int64_t)s * J);
            const int env = table[3 * j], t0 = table[3 * j + 1], len = table[3 * j + 2];
            float v = 0.0f;
            if (s < len) {
                const int64_t src = (int64_t)(t0 + s) * N + env;
                int k = col;
#pragma unroll
                for (int i = 0; i < GF_MLP_MAX_INPUTS; ++i) {
                    if (i >= g.num_inputs) break;
                    const int w = g.inputs[i].width;
                    if (k < w) {
                        const int rs = g.inputs[i].row_stride ? g.inputs[i].row_stride : w;
                        v = G(g.inputs[i].rows)[src * rs + k];
                        break;
                    }
                    k -= w;
                }
                if (g.mean) v = (v - G(g.mean)[col]) / (G(g.std)[col] + g.eps);   // EmpiricalNormalization.forward, as gf_minibatch_gather
            }
            G(g.dst)[e] = v;
        }
        return;
    }
    // masks [T, J], the un-pad index [num_mb_envs · T] and the initial states [J, H] per net
    const int64_t rows = (int64_t)T * J;
    for (int64_t e = start; e < rows; e += stride) {
        const int s = (int)(e / J), j = (int)(e - (int64_t)s * J);
        const int env = table[3 * j], t0 = table[3 * j + 1], len = table[3 * j + 2];
        const bool real = s < len;
        G(a.masks)[e] = real ? 1 : 0;
        const int el = env - a.env_start;
        if (real && el >= 0 && el < a.num_mb_envs) G(a.unpad_index)[(int64_t)el * T + t0 + s] = (int64_t)j * T + s;
    }
#pragma unroll
    for (int net = 0; net < 2; ++net) {
        const GfTrajState& st = a.states[net];
        const int H = st.hidden;
        if (H == 0) continue;
        const int64_t total = (int64_t)J * H;
        for (int64_t e = start; e < total; e += stride) {
            const int j = (int)(e / H), col = (int)(e - (int64_t)j * H);
            const int env = table[3 * j], t0 = table[3 * j + 1];
            const int64_t src = (int64_t)env * H + col;
            G(st.h0)[e] = t0 == 0 ? G(st.h_start)[src] : 0.0f;   // a trajectory that starts later starts behind a done
            if (st.c0) G(st.c0)[e] = t0 == 0 ? G(st.c_start)[src] : 0.0f;
        }
    }
}

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_traj_table(const GfTrajTableArgs* a, void* stream) {
    if (!a) return GF_E_NULL;
    if (a->num_steps < 0 || a->num_envs < 0 || (int64_t)a->num_steps * a->num_envs > 0x7fffffff / 3) return GF_E_RANGE;
    if (!a->dones || !a->counts || !a->offsets || !a->table) return GF_E_NULL;
    if (a->num_steps == 0 || a->num_envs == 0) return GF_OK;
    gf::klaunch(gf::traj_table_kernel, dim3(1), dim3(gf::kTrajBlock), 0, (hipStream_t)stream, *a);
    return gf::launch_status();
}

extern "C" __attribute__((visibility("default"))) int gf_traj_gather(const GfTrajGatherArgs* a, void* stream) {
    if (!a) return GF_E_NULL;
    if (a->num_steps < 1 || a->num_envs < 1 || a->first_traj < 0 || a->num_traj < 0 || a->env_start < 0 || a->num_mb_envs < 0 ||
        a->env_start + (int64_t)a->num_mb_envs > a->num_envs || (int64_t)a->num_traj > (int64_t)a->num_steps * a->num_mb_envs ||
        a->num_traj < a->num_mb_envs || a->first_traj + (int64_t)a->num_traj > a->table_rows)
        return GF_E_RANGE;
    if (!a->table || !a->masks || !a->unpad_index) return GF_E_NULL;
    int64_t most = (int64_t)a->num_steps * a->num_traj;
    for (int i = 0; i < 2; ++i) {
        const GfTrajGroup& g = a->groups[i];
        if (g.width < 0 || g.width > GF_MLP_MAX_INPUT_WIDTH) return GF_E_RANGE;
        if (g.width == 0) {
            if (g.dst) return GF_E_NULL;
            continue;
        }
        if (g.num_inputs < 1 || g.num_inputs > GF_MLP_MAX_INPUTS) return GF_E_RANGE;
        if (!g.dst || (g.mean && !g.std)) return GF_E_NULL;
        int64_t w = 0;
        for (int s = 0; s < g.num_inputs; ++s) {
            if (!g.inputs[s].rows) return GF_E_NULL;
            if (g.inputs[s].width < 1 || (g.inputs[s].row_stride && g.inputs[s].row_stride < g.inputs[s].width)) return GF_E_RANGE;
            w += g.inputs[s].width;
        }
        if (w != g.width) return GF_E_RANGE;
        if ((int64_t)a->num_steps * a->num_traj * g.width > most) most = (int64_t)a->num_steps * a->num_traj * g.width;
    }
    for (int i = 0; i < 2; ++i) {
        const GfTrajState& st = a->states[i];
        if (st.hidden < 0 || st.hidden > GF_MLP_MAX_HIDDEN) return GF_E_RANGE;
        if (st.hidden == 0) {
            if (st.h0 || st.c0) return GF_E_NULL;
            continue;
        }
        if (!st.h_start || !st.h0 || (st.c0 && !st.c_start)) return GF_E_NULL;
        if ((int64_t)a->num_traj * st.hidden > most) most = (int64_t)a->num_traj * st.hidden;
    }
    if (a->num_traj == 0) return GF_OK;
    int64_t blocks = (most + gf::kTrajBlock - 1) / gf::kTrajBlock;
    if (blocks > 4096) blocks = 4096;   // (grid-stride beyond: 16 workgroups per CU's worth)
    gf::klaunch(gf::traj_gather_kernel, dim3((unsigned)blocks, 3u), dim3(gf::kTrajBlock), 0, (hipStream_t)stream, *a);
    return gf::launch_status();
}
