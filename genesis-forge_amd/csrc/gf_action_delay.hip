// gf_action_delay.hip — gf_action_delay: actuator latency (managers/action_delay.py; Isaac Lab's DelayedPDActuator and its per-env
// DelayBuffer, the "action lag" buffer of the legged_gym forks): this step's position targets go into a ring of L steps, the
// actuators get the targets of lag[n] steps ago, and an env whose episode has just begun draws a new lag and has its ring primed —
// in one launch.  include/gf_step.h has the contract.
//
// Composed from torch this is a chain of small launches on [N, D] data every step: the slot write, a gather by a per-env index, a
// `where` for the fresh episodes, a draw and a scatter for the new lags.  Here the step is a pure stream.  The [N, D] arrays are one
// flat run of N*D words, as in gf_action.hip, and a lane owns one 16-byte word of it when D % 4 == 0 (four DOFs of ONE env, so the
// word has one lag and one freshness) or one element otherwise.  The ring is slot-major, [L, N, D]: the lane's word has the same
// offset in `in`, in `out` and in every slot, the write to slot `head` is as coalesced as the read of `in`, and the lagged read is
// a whole 16-byte word of another slot at that offset again.  An ordinary lane reads in, lag[n] and the freshness bytes, stores the
// slot, loads the lagged slot (never the one it stored: 1 <= lag <= L - 1) and stores out: 16 D bytes per env.  Freshness is decided
// from read-only inputs, so the lanes of an env agree without a word between them, and lag[n] is written only by the lane that
// owns the env's first word — the others compute the same draw and never read it back.  The fresh path (L stores per lane, one
// Philox block) sits behind the ordinary one; no LDS, nothing between lanes or workgroups.  Words move as integers: no bit changes.
#include "gf_launch.h"

namespace gf {

constexpr int kDelayBlock = 256;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <typename W>   // W: u32x4 (four DOFs of one env) or uint32_t (one DOF)
__global__ __launch_bounds__(kDelayBlock) void action_delay_kernel(const GfActionDelayArgs a, const int64_t words, const int64_t total) {
    constexpr int kPer = (int)(sizeof(W) / 4);
    const int64_t i = (int64_t)blockIdx.x * kDelayBlock + (int64_t)threadIdx.x;
    if (i >= words) return;
    const int64_t e = i * kPer;   // the word's first element in the flat [N*D] run
    const uint32_t D = (uint32_t)a.num_dofs;
    // (wave-uniform: a 32-bit division wherever the run is shorter than 2^32 elements)
    const int64_t n = total <= 0xffffffffll ? (int64_t)((uint32_t)e / D) : e / (int64_t)D;
    const int L = a.slots;

    const W x = reinterpret_cast<const GF_GLOBAL W*>(G(a.in))[i];
    bool fresh = a.prime_all != 0;
    if (a.episode_length) fresh = fresh || G(a.episode_length)[n] <= 1;
    if (a.mask) fresh = fresh || G(a.mask)[n] != 0;
    if (a.mask2) fresh = fresh || G(a.mask2)[n] != 0;
    GF_GLOBAL W* ring = reinterpret_cast<GF_GLOBAL W*>(G(a.ring));
    GF_GLOBAL W* out = reinterpret_cast<GF_GLOBAL W*>(G(a.out));

    if (!fresh) {
        // 4: the slot of this step, then the slot of lag[n] steps ago (another slot, or none at all)
        ring[(int64_t)a.head * words + i] = x;
        const int l = G(a.lag)[n];
        W y = x;
        if (l > 0 && l < L) {
            const int s = a.head - l;
            y = ring[(int64_t)(s < 0 ? s + L : s) * words + i];
        }
        out[i] = y;
        return;
    }

    // 2: the new lag (every lane of the env computes it; the owner of the env's first word stores it)
    if (e == n * (int64_t)D) {
        float u;
        if (a.draws) {
            u = G(a.draws)[n];
        } else {
            const uint64_t key = a.seed ^ GF_ACTION_DELAY_SEED_TAG;
            u = u24_to_unit(philox4x32_10((uint32_t)n + a.env_offset, 0u, a.step, 0u, (uint32_t)key, (uint32_t)(key >> 32)).x);
        }
        const int w = a.lag_hi - a.lag_lo + 1;
        const int r = (int)(u * (float)w);
        G(a.lag)[n] = a.lag_lo + (r < w - 1 ? r : w - 1);
    }
    // 3: every slot and the output are this step's targets
    for (int s = 0; s < L; ++s) ring[(int64_t)s * words + i] = x;
    out[i] = x;
}

static bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_action_delay_sizeof(void) { return (int)sizeof(GfActionDelayArgs); }

extern "C" __attribute__((visibility("default"))) int gf_action_delay(const GfActionDelayArgs* a, void* stream) {
    if (!a || !a->in || !a->out || !a->ring || !a->lag) return GF_E_NULL;
    if (a->num_envs < 0 || a->num_dofs <= 0) return GF_E_RANGE;
    if (a->slots < 1 || a->slots > GF_ACTION_DELAY_MAX_SLOTS || a->head < 0 || a->head >= a->slots) return GF_E_RANGE;
    if (a->lag_lo < 0 || a->lag_hi < a->lag_lo || a->lag_hi > a->slots - 1) return GF_E_RANGE;
    if (a->prime_all != 0 && a->prime_all != 1) return GF_E_RANGE;
    // (more elements than 2^31 - 1 workgroups of 16-byte words can own: refused before N * D is formed, which keeps L * N * D in int64)
    if (a->num_envs > (int64_t)0x7fffffff * gf::kDelayBlock * 4 / a->num_dofs) return GF_E_RANGE;
    const int64_t total = a->num_envs * (int64_t)a->num_dofs;
    const bool vec = (a->num_dofs & 3) == 0 && gf::al16(a->in) && gf::al16(a->out) && gf::al16(a->ring);
    const int64_t words = vec ? total >> 2 : total;
    const int64_t blocks = (words + gf::kDelayBlock - 1) / gf::kDelayBlock;
    if (blocks > 0x7fffffff) return GF_E_RANGE;
    if (a->num_envs == 0) return GF_OK;
    hipStream_t s = (hipStream_t)stream;
    gf::PhaseScope scope(GF_PHASE_TERRAIN, s);
    if (vec) GF_LAUNCH(scope, gf::action_delay_kernel<gf::u32x4>, (unsigned)blocks, gf::kDelayBlock, 0, s, *a, words, total);
    else GF_LAUNCH(scope, gf::action_delay_kernel<uint32_t>, (unsigned)blocks, gf::kDelayBlock, 0, s, *a, words, total);
    return gf::launch_status();
}
