// gf_policy.hip — the per-step pieces of rsl_rl's collection loop around env.step(): Gaussian action sampling (PPO.act) and the
// time-out bootstrap with the runner's episode statistics (PPO.process_env_step, OnPolicyRunner.learn).  include/gf_step.h has
// the contracts; neither entry point is a phase of the step.
//
// gf_policy_act: one lane per env walks its A columns in groups of four — one Philox block per group gives the group's four
// normals — and folds log_prob left to right in a register.  16-byte loads and stores where A % 4 == 0 and every [N, A] row is
// 16-byte aligned, scalar ones otherwise; the arithmetic is the same.  With std_is_log every loaded std element goes through expf
// first (policy_sigma; a kernel instance of its own).  Algorithmic traffic per env: R 4A (mean) + 4A (std, [N, A]
// only) + 4A (noise, parity mode only) + 4, W 16A + 8 bytes.
//
// gf_episode_step: 256 lanes x 4 consecutive envs per workgroup.  A lane's done envs get their ranks from a wave scan and the
// wave totals in LDS; the count in front of the workgroup and the step's total come, up to GF_EPISODE_SINGLE_MAX envs, from the
// workgroup counting the whole done mask itself (16-byte units, cache-resident: 64 KiB per workgroup at 65 536 envs) and, above
// it, from a first launch that leaves one count per workgroup (1 M envs: the whole mask read 1 024 times would be 1 GiB of cache
// traffic).  No workgroup waits for another.  Algorithmic traffic per env: R 4 + 1 (+ 1 + 4 with time_outs) + 8, W 8 (+ 4) bytes.
#include "gf_launch.h"
#include "gf_policy_row.h"

namespace gf {

// ---- gf_policy_act --------------------------------------------------------------------------------------------------------------
// (the row's body is gf_policy_row.h: gf_mlp_act samples with it too)
constexpr int kActBlock = 256;

template <bool V, bool LOG>
__global__ __launch_bounds__(kActBlock) void policy_act_kernel(const GfPolicyActArgs a) {
    const int64_t n = (int64_t)blockIdx.x * kActBlock + threadIdx.x;
    if (n >= a.num_envs) return;
    const int A = a.num_actions;
    const GF_GLOBAL float* mean = G(a.mean) + n * A;
    policy_act_row<V, LOG>(a, n, [&](int c0, float (&m)[4]) { act_load4<V>(mean, c0, A, m); });
}

// ---- gf_episode_step ------------------------------------------------------------------------------------------------------------
constexpr int kEpBlock = 256;
constexpr int kEpPerLane = 4;
static_assert(kEpBlock * kEpPerLane == GF_EPISODE_BLOCK_ENVS, "envs per workgroup");

typedef uint32_t u32x4e __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int nonzero_bytes4(uint32_t x) { return __builtin_popcount((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u); }

__device__ __forceinline__ int block_sum(int v, int* s_w) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, GF_WAVE);
    __syncthreads();   // (s_w may still be read by an earlier use)
    if ((threadIdx.x & (GF_WAVE - 1)) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int i = 0; i < kEpBlock / GF_WAVE; ++i) t += s_w[i];
    return t;
}

// done envs of [b·1024, …) for the count launch: this lane's four
__device__ __forceinline__ int ep_lane_count(const GfEpisodeArgs& a, int64_t first) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < kEpPerLane; ++j)
        if (first + j < a.num_envs) c += G(a.dones)[first + j] != 0;
    return c;
}

__global__ __launch_bounds__(kEpBlock) void episode_count_kernel(const GfEpisodeArgs a) {
    __shared__ int s_w[kEpBlock / GF_WAVE];
    const int64_t first = ((int64_t)blockIdx.x * kEpBlock + threadIdx.x) * kEpPerLane;
    const int t = block_sum(ep_lane_count(a, first), s_w);
    if (threadIdx.x == 0) G(a.block_counts)[blockIdx.x] = t;
}

// (done envs in front of this workgroup, done envs of the step) from the whole mask: 16-byte units, four in flight per lane
__device__ __forceinline__ void ep_scan_mask(const GfEpisodeArgs& a, int64_t block_first, int aligned, int& pre, int& tot) {
    const int64_t N = a.num_envs, units = (N + 15) / 16;
    const GF_GLOBAL uint8_t* m = G(a.dones);
    for (int64_t u0 = threadIdx.x; u0 < units; u0 += 4 * kEpBlock) {
        int c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t u = u0 + (int64_t)k * kEpBlock;
            c[k] = 0;
            if (u >= units) continue;
            if (aligned && u * 16 + 16 <= N) {
                const u32x4e w = *reinterpret_cast<const GF_GLOBAL u32x4e*>(m + u * 16);
                c[k] = nonzero_bytes4(w.x) + nonzero_bytes4(w.y) + nonzero_bytes4(w.z) + nonzero_bytes4(w.w);
            } else {
                const int64_t hi = u * 16 + 16 < N ? u * 16 + 16 : N;
                for (int64_t e = u * 16; e < hi; ++e) c[k] += m[e] != 0;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tot += c[k];
            if ((u0 + (int64_t)k * kEpBlock) * 16 < block_first) pre += c[k];   // (block_first is a multiple of 16: units never straddle it)
        }
    }
}

__global__ __launch_bounds__(kEpBlock) void episode_kernel(const GfEpisodeArgs a, const int num_blocks, const int two_launch, const int al_f32,
                                                           const int al_u8, const int mask16) {
    __shared__ int s_w[kEpBlock / GF_WAVE];
    const int64_t N = a.num_envs;
    const int64_t block_first = (int64_t)blockIdx.x * GF_EPISODE_BLOCK_ENVS;
    const int64_t first = block_first + (int64_t)threadIdx.x * kEpPerLane;
    const bool stats = a.cur_reward_sum != nullptr;
    const bool boot = a.time_outs != nullptr;
    const bool vec = al_f32 && al_u8 && first + kEpPerLane <= N;
    float r[kEpPerLane] = {}, v[kEpPerLane] = {}, s[kEpPerLane] = {}, l[kEpPerLane] = {};
    uint32_t d = 0, to = 0;   // one byte per env
    if (vec) {
        const f32x4 r4 = *reinterpret_cast<const GF_GLOBAL f32x4*>(G(a.rewards) + first);
        r[0] = r4.x; r[1] = r4.y; r[2] = r4.z; r[3] = r4.w;
        if (boot) {
            const f32x4 v4 = *reinterpret_cast<const GF_GLOBAL f32x4*>(G(a.values) + first);
            v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
            to = *reinterpret_cast<const GF_GLOBAL uint32_t*>(G(a.time_outs) + first);
        }
        if (stats) {
            d = *reinterpret_cast<const GF_GLOBAL uint32_t*>(G(a.dones) + first);
            const f32x4 s4 = *reinterpret_cast<const GF_GLOBAL f32x4*>(G(a.cur_reward_sum) + first);
            const f32x4 l4 = *reinterpret_cast<const GF_GLOBAL f32x4*>(G(a.cur_episode_length) + first);
            s[0] = s4.x; s[1] = s4.y; s[2] = s4.z; s[3] = s4.w;
            l[0] = l4.x; l[1] = l4.y; l[2] = l4.z; l[3] = l4.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < kEpPerLane; ++j) {
            const int64_t n = first + j;
            const bool in = n < N;
            r[j] = in ? G(a.rewards)[n] : 0.0f;
            v[j] = in && boot ? G(a.values)[n] : 0.0f;
            s[j] = in && stats ? G(a.cur_reward_sum)[n] : 0.0f;
            l[j] = in && stats ? G(a.cur_episode_length)[n] : 0.0f;
            to |= (uint32_t)(in && boot && G(a.time_outs)[n] != 0) << (8 * j);
            d |= (uint32_t)(in && stats && G(a.dones)[n] != 0) << (8 * j);
        }
    }
    if (stats) {
        // the step's done envs in front of this workgroup, and in all
        int pre = 0, tot = 0;
        if (two_launch) {
            for (int b = threadIdx.x; b < num_blocks; b += kEpBlock) {
                const int c = G(a.block_counts)[b];
                tot += c;
                if (b < (int)blockIdx.x) pre += c;
            }
        } else {
            ep_scan_mask(a, block_first, mask16, pre, tot);
        }
        pre = block_sum(pre, s_w);
        tot = block_sum(tot, s_w);
        // this lane's rank among the workgroup's done envs: wave scan, then the waves in front
        uint32_t bits = 0;
#pragma unroll
        for (int j = 0; j < kEpPerLane; ++j) bits |= (uint32_t)(((d >> (8 * j)) & 0xffu) != 0) << j;
        const int mine = __builtin_popcount(bits);
        const int lane = threadIdx.x & (GF_WAVE - 1);
        int incl = mine;
#pragma unroll
        for (int o = 1; o < GF_WAVE; o <<= 1) {
            const int up = __shfl_up(incl, o, GF_WAVE);
            if (lane >= o) incl += up;
        }
        __syncthreads();   // (s_w is reused)
        if (lane == GF_WAVE - 1) s_w[threadIdx.x >> 6] = incl;
        __syncthreads();
        int64_t k = pre + incl - mine;
        for (int i = 0; i < (int)(threadIdx.x >> 6); ++i) k += s_w[i];
        const GF_GLOBAL int32_t* st = G(a.ring_state) + 2 * a.parity;
        const int64_t W = a.window;
        const int64_t head = st[0] >= 0 && st[0] < W ? st[0] : 0, fill = st[1] >= 0 && st[1] <= W ? st[1] : W;   // (never an index outside the ring)
        const int64_t keep_from = (int64_t)tot - W;   // ranks below it are pushed out by later ones of the same step
#pragma unroll
        for (int j = 0; j < kEpPerLane; ++j) {
            s[j] = s[j] + r[j];        // cur_reward_sum += rewards
            l[j] = l[j] + 1.0f;        // cur_episode_length += 1
            if (bits & (1u << j)) {
                if (k >= keep_from) {
                    const int64_t pos = (head + k) % W;
                    G(a.ring_reward)[pos] = s[j];
                    G(a.ring_length)[pos] = l[j];
                }
                ++k;
                s[j] = 0.0f;
                l[j] = 0.0f;
            }
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            GF_GLOBAL int32_t* nx = G(a.ring_state) + 2 * (1 - a.parity);
            nx[0] = (int32_t)((head + tot) % W);
            nx[1] = (int32_t)(fill + tot < W ? fill + tot : W);
        }
        if (vec) {
            *reinterpret_cast<GF_GLOBAL f32x4*>(G(a.cur_reward_sum) + first) = f32x4{s[0], s[1], s[2], s[3]};
            *reinterpret_cast<GF_GLOBAL f32x4*>(G(a.cur_episode_length) + first) = f32x4{l[0], l[1], l[2], l[3]};
        } else {
#pragma unroll
            for (int j = 0; j < kEpPerLane; ++j)
                if (first + j < N) { G(a.cur_reward_sum)[first + j] = s[j]; G(a.cur_episode_length)[first + j] = l[j]; }
        }
    }
    if (boot) {   // PPO.process_env_step: rewards += gamma * values * time_outs (one product, one product, one sum), after the statistics
#pragma unroll
        for (int j = 0; j < kEpPerLane; ++j) r[j] = r[j] + (a.gamma * v[j]) * (((to >> (8 * j)) & 0xffu) ? 1.0f : 0.0f);
        if (vec) {
            *reinterpret_cast<GF_GLOBAL f32x4*>(G(a.rewards) + first) = f32x4{r[0], r[1], r[2], r[3]};
        } else {
#pragma unroll
            for (int j = 0; j < kEpPerLane; ++j)
                if (first + j < N) G(a.rewards)[first + j] = r[j];
        }
    }
}

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_policy_act(const GfPolicyActArgs* a, void* stream) {
    if (!a || !a->mean || !a->std || !a->actions) return GF_E_NULL;
    if (a->values_out && !a->values) return GF_E_NULL;
    if (a->num_envs < 0 || a->num_actions < 1 || (a->std_per_env != 0 && a->std_per_env != 1) || a->std_is_log > 1u)
        return GF_E_RANGE;
    if (a->num_envs == 0) return GF_OK;
    const int64_t blocks = (a->num_envs + gf::kActBlock - 1) / gf::kActBlock;
    if (blocks > 0x7fffffff) return GF_E_RANGE;
    uintptr_t bits = 0;
    const void* rows[] = {a->mean, a->noise, a->actions, a->actions_out, a->mu_out, a->sigma_out, a->std};
    for (const void* p : rows) bits |= reinterpret_cast<uintptr_t>(p);
    const bool vec = (bits & 15u) == 0 && (a->num_actions & 3) == 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks), block(gf::kActBlock);
    if (a->std_is_log) {   // (a kernel instance of its own: the plain one keeps the code it had)
        if (vec) gf::klaunch(gf::policy_act_kernel<true, true>, grid, block, 0, s, *a);
        else gf::klaunch(gf::policy_act_kernel<false, true>, grid, block, 0, s, *a);
    } else {
        if (vec) gf::klaunch(gf::policy_act_kernel<true, false>, grid, block, 0, s, *a);
        else gf::klaunch(gf::policy_act_kernel<false, false>, grid, block, 0, s, *a);
    }
    return gf::launch_status();
}

extern "C" __attribute__((visibility("default"))) int gf_episode_step(const GfEpisodeArgs* a, void* stream) {
    if (!a || !a->rewards) return GF_E_NULL;
    if (a->num_envs < 0 || a->num_envs >= ((int64_t)1 << 31) || (a->parity != 0 && a->parity != 1)) return GF_E_RANGE;
    if (a->time_outs && !a->values) return GF_E_NULL;   // a bootstrap needs the value row
    const bool stats = a->cur_reward_sum != nullptr;
    if (stats) {
        if (!a->dones || !a->cur_episode_length || !a->ring_reward || !a->ring_length || !a->ring_state) return GF_E_NULL;
        if (a->window < 1) return GF_E_RANGE;
    } else if (a->cur_episode_length || a->ring_reward || a->ring_length || a->ring_state) {
        return GF_E_NULL;   // half a statistics set
    }
    if (!stats && !a->time_outs) return GF_OK;   // nothing asked
    if (a->num_envs == 0) return GF_OK;
    const int blocks = (int)((a->num_envs + GF_EPISODE_BLOCK_ENVS - 1) / GF_EPISODE_BLOCK_ENVS);
    const int two = stats && a->num_envs > GF_EPISODE_SINGLE_MAX;
    if (two && !a->block_counts) return GF_E_NULL;
    uintptr_t f = reinterpret_cast<uintptr_t>(a->rewards) | reinterpret_cast<uintptr_t>(a->values) |
                  reinterpret_cast<uintptr_t>(a->cur_reward_sum) | reinterpret_cast<uintptr_t>(a->cur_episode_length);
    uintptr_t b = reinterpret_cast<uintptr_t>(a->dones) | reinterpret_cast<uintptr_t>(a->time_outs);
    const int al_f32 = (f & 15u) == 0, al_u8 = (b & 3u) == 0, mask16 = (reinterpret_cast<uintptr_t>(a->dones) & 15u) == 0;
    hipStream_t s = (hipStream_t)stream;
    if (two) gf::klaunch(gf::episode_count_kernel, dim3(blocks), dim3(gf::kEpBlock), 0, s, *a);
    gf::klaunch(gf::episode_kernel, dim3(blocks), dim3(gf::kEpBlock), 0, s, *a, blocks, two, al_f32, al_u8, mask16);
    return gf::launch_status();
}
