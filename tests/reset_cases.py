"""gf_masked_reset, gf_command_step and gf_gait_step restated in numpy, and the cases that pin them at their edges.

The restatements are written from the contract in include/gf_step.h and the reference's Python (genesis_env.py:233-252,
reward_manager.py:197-222, contact_manager.py:316-329, position_action_manager.py:455-464, mdp/reset.py:102-124 and :199-226,
command_manager.py:152-170 and :290-303, examples/gait_trainer/gait_command_manager.py:185-255, 331-338, 347-394, 434-441): they work
on the index list of the envs a call resets or resamples, as the reference does, not lane by lane.  float32 arithmetic is one
rounding per operation; ``uniform_(lo, hi)`` is ``u * (hi - lo) + lo``; sqrt / rint are numpy's; draws come from
tests/philox.py with the GLOBAL env id ((local index + env_offset) mod 2^32) as an explicit argument.

A ``Spec`` holds one call: scalars by descriptor field name, arrays in their natural shape, and the names of the arrays whose
pointer the call leaves NULL (they are allocated all the same, so that "nothing wrote there" can be checked).  ``restate(spec)``
returns every array as the call must leave it plus the exact statistics: integer counters summed over the shards, and
``reward_episode_sum`` as ``math.fsum`` of the float32 quotients.  ``Launch`` runs a spec through the raw C ABI of either backend on
guarded buffers and compares through integer views.

Two things a restatement cannot say and the cases therefore avoid: the sign of a NaN an operation GENERATES (0 · inf, 0 / 0: it is the
platform's, x86 sets the sign bit — so no case lets one reach a float32 buffer; in the f64 statistics a NaN is compared as NaN),
and which blocks' swing / stance bytes a masked gait launch rewrites beyond those that hold a reset env (the header allows more:
the oracle rewrites every block, the kernel only the blocks it touched; ``restate(spec, flags_all=True)`` states the former)."""
import ctypes as C
import functools
import math

import numpy as np

import philox

F = np.float32
GF_SPAWN_BLOCK = 0x100000
CMD_STEP, CMD_MASKED, CMD_ALL = 0, 1, 2
E_UNSUPPORTED = -5
SIZES = (1, 63, 64, 65, 130, 4097)   # 4097 = 64 * 64 + 1: workgroup 64 wraps onto statistics shard 0
SHARDS = 64
TWO_PI = F(2.0 * math.pi)
DT = F(2.0 ** -6)
TROT = (0.0, 0.5, 0.5, 0.0)


# ---- float32 building blocks, in the documented operation order ------------------------------------------------------------------
def uniform_range(u, lo, hi):
    with np.errstate(all="ignore"):
        return np.asarray(u, F) * (F(hi) - F(lo)) + F(lo)


def sincos_det(x):
    """k = rint(x·2/π), three-part Cody-Waite reduction by π/2, Cephes polynomials on [-π/4, π/4], quadrant fix-up."""
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        k = np.rint(x * F(0.63661977236758134))
        r = x - k * F(1.5703125)
        r = r - k * F(4.837512969970703125e-4)
        r = r - k * F(7.54978995489188216e-8)
        z = r * r
        ps = ((F(-1.9515295891e-4) * z + F(8.3321608736e-3)) * z - F(1.6666654611e-1)) * z * r + r
        pc = ((F(2.443315711809948e-5) * z - F(1.388731625493765e-3)) * z + F(4.166664568298827e-2)) * z * z - F(0.5) * z + F(1.0)
        q = np.where(np.isnan(k), F(0), k).astype(np.int64) & 3
    odd = (q & 1) != 0
    sv, cv = np.where(odd, pc, ps), np.where(odd, ps, pc)
    return np.where((q & 2) != 0, -sv, sv).astype(F), np.where(((q + 1) & 2) != 0, -cv, cv).astype(F)


def xyz_to_quat(ax, ay, az):
    """Extrinsic x-y-z Euler angles -> (w, x, y, z), each product rounded, sums left to right."""
    h = F(0.5)
    (sx, cx), (sy, cy), (sz, cz) = sincos_det(np.asarray(ax, F) * h), sincos_det(np.asarray(ay, F) * h), sincos_det(np.asarray(az, F) * h)
    return np.stack([(cx * cy) * cz + (sx * sy) * sz, (sx * cy) * cz - (cx * sy) * sz,
                     (cx * sy) * cz + (sx * cy) * sz, (cx * cy) * sz - (sx * sy) * cz], axis=-1).astype(F)


def torch_remainder(a, b):
    """aten remainder: C fmod (exact), then moved to the divisor's sign."""
    a, b = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F))
    with np.errstate(all="ignore"):
        m = np.fmod(a, b)
        return np.where((m != 0) & ((b < 0) != (m < 0)), m + b, m).astype(F)


def terrain_height(tv, x, y):
    """terrain_manager.py:100-166: the in-place normalisation chain, then grid_sample(bilinear, border, align_corners=True); taps
    outside the field count as 0; the four products are summed nw, ne, sw, se."""
    x, y = np.asarray(x, F), np.asarray(y, F)
    f = tv["height_field"]
    if f is None:
        return np.full(x.shape, F(tv["origin_z"]), F)
    H, W = f.shape

    def index(v, v_min, span, size):
        n = (((v - F(v_min)) / F(span)) * F(2.0)) - F(1.0)
        i = ((n + F(1.0)) / F(2.0)) * F(size - 1)
        return np.minimum(np.maximum(i, F(0.0)), F(size - 1))

    ix, iy = index(x, tv["x_min"], tv["x_span"], W), index(y, tv["y_min"], tv["y_span"], H)
    fx0, fy0 = np.floor(ix), np.floor(iy)
    fx1, fy1 = fx0 + F(1.0), fy0 + F(1.0)
    nw, ne, sw, se = (fx1 - ix) * (fy1 - iy), (ix - fx0) * (fy1 - iy), (fx1 - ix) * (iy - fy0), (ix - fx0) * (iy - fy0)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    x1_in, y1_in = x0 + 1 < W, y0 + 1 < H
    x1, y1 = np.where(x1_in, x0 + 1, x0), np.where(y1_in, y0 + 1, y0)
    z = F(0.0)
    v_nw, v_ne = f[y0, x0], np.where(x1_in, f[y0, x1], z)
    v_sw, v_se = np.where(y1_in, f[y1, x0], z), np.where(x1_in & y1_in, f[y1, x1], z)
    return (((v_nw * nw + v_ne * ne) + v_sw * sw) + v_se * se).astype(F)


# ---- a call ------------------------------------------------------------------------------------------------------------------------
class Spec:
    def __init__(self, fn, sc, arr, null=(), stats=True, exact=True):
        self.fn, self.sc, self.arr, self.null, self.stats, self.exact = fn, dict(sc), dict(arr), set(null), stats, exact
        self.offs = {}        # array name -> elements of misalignment (refusal cases)
        self.flags_all = False

    def seen(self):
        """The arrays as the call sees them: None where the pointer is NULL."""
        return {k: (None if k in self.null else v.copy()) for k, v in self.arr.items()}

    def global_ids(self, ids):
        return ((np.asarray(ids, np.uint64) + np.uint64(self.sc.get("env_offset", 0))) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _go(sc, a, N):
    if sc.get("mode", CMD_MASKED) == CMD_STEP:
        return (a["episode_length"][:N].astype(np.int64) % int(sc["resample_steps"])) == 0
    if sc.get("mode", CMD_MASKED) == CMD_ALL:
        return np.ones(N, bool)
    go = a["mask"][:N] != 0
    if a.get("mask2") is not None:
        go = go | (a["mask2"][:N] != 0)
    return go


def _exact_sum(q):
    q = np.asarray(q, np.float64)
    return math.fsum(q.tolist()) if np.isfinite(q).all() else float(np.sum(q))   # inf / NaN: the same in any order


def restate_reset(spec):
    sc, a = spec.sc, spec.seen()
    N, D, T = sc["num_envs"], sc["num_dofs"], sc["num_reward_terms"]
    ids = np.nonzero(_go(sc, a, N))[0]
    genv = spec.global_ids(ids)
    seed, stream = sc.get("seed", 0), sc.get("stream", 0)
    st = dict(reset_count=len(ids), reward_episode_sum=[0.0] * 24, abs_sum=[0.0] * 24, n=len(ids))
    # GenesisEnv.reset (genesis_env.py:233-252)
    if a["env_actions"] is not None:
        a["env_actions"][ids] = 0
        a["env_last_actions"][ids] = 0
    if a["episode_length"] is not None:
        a["episode_length"][ids] = 0
    scaling = F(sc.get("max_random_scaling", 0.0))
    if a["max_episode_length"] is not None and scaling > 0:
        u = a["len_draws"][ids] if a["len_draws"] is not None else philox.uniform_ids(seed, stream, genv, 1)[:, 0]
        r = uniform_range(u, -1.0, 1.0) * scaling
        a["max_episode_length"][ids] = np.rint(F(sc["base_max_episode_length"]) + r).astype(np.int32)   # torch.round: half to even
    # RewardManager.reset (reward_manager.py:202-222)
    if a["episode_seconds"] is not None:
        if sc.get("reward_logging", 0) and a["episode_sums"] is not None:
            secs = a["episode_seconds"][ids]
            for t in range(T):
                if (sc.get("reward_log_mask", 0) >> t) & 1:            # cfg.weight != 0
                    with np.errstate(all="ignore"):
                        per_sec = a["episode_sums"][t, ids] / secs    # value[envs_idx] /= episode_seconds
                    st["reward_episode_sum"][t] = _exact_sum(per_sec)
                    st["abs_sum"][t] = _exact_sum(np.abs(per_sec))
                a["episode_sums"][t, ids] = 0
        a["episode_seconds"][ids] = F(1e-10)
    # ContactManager.reset (contact_manager.py:316-329)
    for m in range(sc.get("num_contact", 0)):
        for s in range(4):
            p = a.get("air_state.%d.%d" % (m, s))
            if p is not None:
                p[ids] = 0
    # PositionActionManager.reset (position_action_manager.py:455-464)
    noise = F(sc.get("dof_noise_scale", 0.0))
    if a["scene_dof_pos"] is not None:
        p = np.broadcast_to(a["default_dof_pos"][None, :], (len(ids), D)).astype(F)
        if noise != 0:
            u = a["dof_draws"][ids] if a["dof_draws"] is not None else philox.uniform_ids(seed, stream, genv, D, first_col=4)
            p = p + uniform_range(u, -1.0, 1.0) * noise
        a["scene_dof_pos"][ids] = p
        if a["scene_dof_vel"] is not None:
            a["scene_dof_vel"][ids] = 0
    # mdp.reset.position (reset.py:102-124) / randomize_terrain_position (reset.py:199-226, terrain_manager.py:236-247)
    if a["scene_pos"] is not None:
        pos = np.broadcast_to(np.asarray(sc["reset_pos"], F)[None, :], (len(ids), 3)).copy()
        quat = np.broadcast_to(np.asarray(sc["reset_quat"], F)[None, :], (len(ids), 4)).copy()
        set_quat = sc.get("set_quat", 0)
        if sc.get("spawn_mode", 0):
            rot = sc.get("spawn_rot_mask", 0)
            if a["spawn_draws"] is not None:
                u = a["spawn_draws"][ids]
            else:
                u = np.zeros((len(ids), 5), F)
                b0 = philox.block_uniform(seed, stream, genv, GF_SPAWN_BLOCK)
                u[:, 0], u[:, 1], u[:, 4] = b0[:, 0], b0[:, 1], b0[:, 2]
                if rot & 3:
                    b1 = philox.block_uniform(seed, stream, genv, GF_SPAWN_BLOCK + 1)
                    u[:, 2], u[:, 3] = b1[:, 0], b1[:, 1]
            pos[:, 0] = u[:, 0] * F(sc["spawn_x_span"]) + F(sc["spawn_x_min"])
            pos[:, 1] = u[:, 1] * F(sc["spawn_y_span"]) + F(sc["spawn_y_min"])
            tv = {k[8:]: v for k, v in sc.items() if k.startswith("terrain.")}
            tv["height_field"] = a.get("terrain.height_field")
            pos[:, 2] = terrain_height(tv, pos[:, 0], pos[:, 1]) + F(sc["spawn_height_offset"])
            ang = [uniform_range(u[:, 2 + k], sc["spawn_rot_lo"][k], sc["spawn_rot_hi"][k]) if (rot >> k) & 1 else np.zeros(len(ids), F)
                   for k in range(3)]
            quat = xyz_to_quat(*ang)
            set_quat = sc.get("spawn_set_quat", 0)
        a["scene_pos"][ids] = pos
        if set_quat and a["scene_quat"] is not None:
            if a["quat_stash"] is not None:
                a["quat_stash"][ids] = a["scene_quat"][ids]
            a["scene_quat"][ids] = quat
        if sc.get("zero_velocity", 0):
            for k in ("scene_lin_vel", "scene_ang_vel", "scene_dof_vel"):
                if a[k] is not None:
                    a[k][ids] = 0
    return a, st


def restate_command(spec):
    sc, a = spec.sc, spec.seen()
    N, R = sc["num_envs"], sc["num_ranges"]
    ids = np.nonzero(_go(sc, a, N))[0]
    u = a["draws"][ids] if a["draws"] is not None else philox.uniform_ids(sc.get("seed", 0), sc.get("stream", 0), spec.global_ids(ids), R)
    for i in range(R):
        a["command"][ids, i] = uniform_range(u[:, i], sc["lo"][i], sc["hi"][i])
    return a, dict(resample_count=len(ids) if sc["mode"] == CMD_STEP else 0)


def foot_flags(phase, offsets, two_pi):
    """[n] bytes: bit 2f = foot f in swing (0 <= phi < π), bit 2f+1 = in stance (π <= phi < 2π); gait_command_manager.py:331-338."""
    two_pi = F(two_pi)
    pi = F(0.5) * two_pi
    byte = np.zeros(len(phase), np.uint8)
    for f in range(4):
        with np.errstate(all="ignore"):
            phi = torch_remainder(phase + offsets[:, f], F(1.0)) * two_pi
        byte |= (((phi >= 0) & (phi < pi)).astype(np.uint8) << (2 * f)) | (((phi >= pi) & (phi < two_pi)).astype(np.uint8) << (2 * f + 1))
    return byte


def restate_gait(spec, flags_all=False):
    sc, a = spec.sc, spec.seen()
    N, G, mode = sc["num_envs"], sc["num_gaits"], sc["mode"]
    go = _go(sc, a, N)
    ids = np.nonzero(go)[0]
    st, sel = a["state"], a["selected"]
    if a["draws"] is not None:
        u = a["draws"][ids]
    else:
        u = philox.uniform_ids(sc.get("seed", 0), sc.get("stream", 0), spec.global_ids(ids), 3)
    # resample_command -> _set_gait (:185-211, 347-374); the gait is the inverse CDF of the cumulative weights at draw 0
    g = np.zeros(len(ids), np.int64)
    for k in range(G - 1):
        g += u[:, 0] >= F(sc["cum_weight"][k])
    sel[ids] = g
    st[ids, 0:4] = np.asarray(sc["gait_offsets"], F)[g]
    fixed = ((sc.get("fixed_clearance_mask", 0) >> g) & 1) != 0
    st[ids, 4] = np.where(fixed, F(sc["clearance_lo"]), uniform_range(u[:, 1], sc["clearance_lo"], sc["clearance_hi"]))
    st[ids, 5] = uniform_range(u[:, 2], sc["period_lo"], sc["period_hi"])
    stats = dict(gait_count=[0, 0, 0, 0])
    if mode != CMD_STEP:      # reset (:241-250)
        st[ids, 6:16] = 0
    else:                     # step (:224-239): the counts after this step's resample, then the clock of every env
        stats["gait_count"] = [int(np.sum(sel[:N] == k)) for k in range(4)]
        with np.errstate(all="ignore"):
            st[:N, 14] = torch_remainder(st[:N, 14] + F(sc["dt"]), st[:N, 5])
            st[:N, 15] = st[:N, 14] / st[:N, 5]
            for f in range(4):
                fp = torch_remainder(st[:N, 15] + st[:N, f], F(1.0))
                st[:N, 6 + f], st[:N, 10 + f] = sincos_det(F(sc["two_pi"]) * fp)
    if a["wave_flags"] is not None:
        byte = foot_flags(st[:N, 15], st[:N, 0:4], sc["two_pi"])
        for b in range((N + 63) // 64):
            if mode != CMD_MASKED or flags_all or go[64 * b:64 * b + 64].any():
                a["wave_flags"][b] = np.bitwise_or.reduce(byte[64 * b:64 * b + 64])
    return a, stats


def restate(spec, flags_all=False):
    if spec.fn == "masked_reset":
        return restate_reset(spec)
    if spec.fn == "command_step":
        return restate_command(spec)
    return restate_gait(spec, flags_all or spec.flags_all)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _f(rng, *shape):
    """Distinct-looking non-zero float32 values (never 0: a skipped store and a store of zero must differ)."""
    return (rng.uniform(0.5, 3.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(F)


def masks(N, kind, seed=1):
    """(mask, mask2 or None) of one named pattern."""
    m, m2 = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    rng = np.random.default_rng([seed, N])
    if kind == "none":
        pass
    elif kind == "first":
        m[0] = 1
    elif kind == "last":
        m[N - 1] = 1
    elif kind == "one_per_wave":
        for b in range((N + 63) // 64):
            m[min(N - 1, 64 * b + (17 * b + 5) % 64)] = 1
    elif kind == "whole_wave":
        m[64:128] = 1
    elif kind == "all":
        m[:] = 1
    elif kind == "mask2_null":
        m[rng.random(N) < 0.3] = 1
        return m, None
    elif kind == "mask2_disjoint":
        r = rng.random(N)
        m[r < 0.2] = 1
        m2[(r >= 0.2) & (r < 0.4)] = 1
    elif kind == "mask2_overlap":
        m[rng.random(N) < 0.3] = 1
        m2[rng.random(N) < 0.3] = 1
        m2[np.nonzero(m)[0][:3]] = 1
    elif kind == "bytes":
        m[rng.random(N) < 0.2] = 0x80
        m2[rng.random(N) < 0.2] = 0xFF
    elif kind == "mixed":     # the default of the other sections: both masks, every byte value, at least env 0 and env N - 1
        m[rng.random(N) < 0.25] = 1
        m2[rng.random(N) < 0.1] = 0xFF
        m[0], m2[N - 1] = 0x80, 1
    elif kind == "three_groups":   # an env in the first, a middle and the last workgroup, nothing else
        m[[min(3, N - 1), (((N + 63) // 64) // 2) * 64, N - 1]] = 1
    else:
        raise KeyError(kind)
    return m, m2


MASK_KINDS = ("none", "first", "last", "one_per_wave", "whole_wave", "all", "mask2_null", "mask2_disjoint", "mask2_overlap", "bytes")


@functools.lru_cache(maxsize=1)
def terrain_fixture():
    import helpers
    fix = helpers.load("terrain")   # [x, y] int16 cells; the view wants metres with rows = y, cols = x (terrain_manager.py:354-359)
    return np.ascontiguousarray((np.asarray(fix["height_field"], F) * F(0.005)).T)


def reset_spec(N, D=5, T=3, links=(4, 7), mask="mixed", philox_draws=True, exact=True, spawn=False, key=0):
    """Every section of the reset enabled, on distinct non-zero inputs."""
    rng = np.random.default_rng([N, D, T, key])
    m, m2 = masks(N, mask)
    arr = dict(mask=m, mask2=m2 if m2 is not None else np.zeros(N, np.uint8),
               env_actions=_f(rng, N, D), env_last_actions=_f(rng, N, D),
               episode_length=rng.integers(1, 500, N).astype(np.int32), max_episode_length=rng.integers(900, 1100, N).astype(np.int32),
               len_draws=rng.random(N).astype(F),
               episode_sums=(F(0.25) * rng.integers(-40, 41, (T, N)).astype(F)) if exact else rng.standard_normal((T, N)).astype(F),
               episode_seconds=(F(2.0) ** rng.integers(-2, 5, N).astype(F)) if exact else rng.uniform(0.1, 20.0, N).astype(F),
               scene_dof_pos=_f(rng, N, D), scene_dof_vel=_f(rng, N, D), default_dof_pos=_f(rng, D), dof_draws=rng.random((N, D)).astype(F),
               scene_pos=_f(rng, N, 3), scene_quat=_f(rng, N, 4), quat_stash=_f(rng, N, 4), scene_lin_vel=_f(rng, N, 3),
               scene_ang_vel=_f(rng, N, 3), spawn_draws=rng.random((N, 5)).astype(F))
    arr["terrain.height_field"] = terrain_fixture()
    for i, L in enumerate(links):
        for s in range(4):
            arr["air_state.%d.%d" % (i, s)] = _f(rng, N, L)
    H, W = arr["terrain.height_field"].shape
    sc = {"num_envs": N, "num_dofs": D, "num_reward_terms": T, "num_contact": len(links), "base_max_episode_length": 1000,
          "max_random_scaling": 100.0, "reward_log_mask": (1 << T) - 1, "reward_logging": 1,
          "air_links": list(links) + [0] * (4 - len(links)), "dof_noise_scale": 0.1, "reset_pos": [0.25, -1.5, 0.42],
          "reset_quat": [0.5, -0.5, 0.5, 0.5], "set_quat": 1, "zero_velocity": 1, "seed": 0x1234567887654321, "stream": (5 << 40) | 77,
          "env_offset": 0, "spawn_mode": 1 if spawn else 0, "spawn_set_quat": 1, "spawn_rot_mask": 7, "spawn_x_min": -2.5,
          "spawn_x_span": 11.0, "spawn_y_min": 2.0, "spawn_y_span": 9.0, "spawn_height_offset": 0.31, "spawn_rot_lo": [-0.4, -0.3, 0.0],
          "spawn_rot_hi": [0.4, 0.3, float(TWO_PI)], "terrain.rows": H, "terrain.cols": W, "terrain.x_min": -3.0, "terrain.x_span": 12.0,
          "terrain.y_min": 1.5, "terrain.y_span": 10.0, "terrain.origin_z": 0.25}
    null = set()
    if m2 is None:
        null.add("mask2")
    if philox_draws:
        null |= {"len_draws", "dof_draws", "spawn_draws"}
    return Spec("masked_reset", sc, arr, null, exact=exact)


def command_spec(N, R=3, mode=CMD_MASKED, mask="mixed", philox_draws=True, steps=7, key=0):
    rng = np.random.default_rng([N, R, mode, key, 11])
    m, m2 = masks(N, mask)
    ep = rng.choice(np.array([0, 6, 7, 8, 14, 2 ** 31 - 1], np.int32), N)
    if N > 64 and steps > 1:
        ep[64:128] = np.where(ep[64:128] % steps == 0, 6, ep[64:128])   # one wave has no env due
    arr = dict(episode_length=ep.astype(np.int32), mask=m, mask2=m2 if m2 is not None else np.zeros(N, np.uint8),
               draws=rng.random((N, R)).astype(F), command=_f(rng, N, R))
    lo = [-1.0, -0.5, 0.25, 0.0, -3.0, 1.0, -2.0, 0.5]
    hi = [1.0, 0.5, 0.75, 2.0, -1.0, 1.5, 2.0, 0.625]
    sc = {"num_envs": N, "num_ranges": R, "mode": mode, "resample_steps": steps, "seed": 0xFEDCBA9876543210, "stream": (1 << 40) | 9,
          "env_offset": 0, "lo": lo, "hi": hi}
    null = set()
    if m2 is None:
        null.add("mask2")
    if philox_draws:
        null.add("draws")
    return Spec("command_step", sc, arr, null)


def cum_weights(G):
    """f32 cumulative sum of the normalised weights exp(0..G-1) (gait_command_manager.py:383-392)."""
    w = np.exp(np.arange(G, dtype=F)).astype(F)
    w = (w / w.sum(dtype=F)).astype(F)
    return [float(x) for x in np.cumsum(w, dtype=F)] + [0.0] * (4 - G)


GAIT_TABLE = [list(TROT), [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.5, 0.5], [0.0, 0.5, 0.0, 0.5]]


def gait_spec(N, G=4, mode=CMD_STEP, mask="mixed", philox_draws=True, steps=7, fixed=0b0101, key=0):
    rng = np.random.default_rng([N, G, mode, key, 13])
    m, m2 = masks(N, mask)
    state = _f(rng, N, 16)
    state[:, 0:4] = rng.choice(np.array([0.0, 0.25, 0.5, 0.75], F), (N, 4))
    state[:, 5] = rng.uniform(0.3, 0.6, N).astype(F)
    state[:, 14] = (state[:, 5] * rng.random(N).astype(F)).astype(F)
    state[:, 15] = (state[:, 14] / state[:, 5]).astype(F)
    flags = np.full(((N + 63) // 64 + 3) // 4 * 4, 0xA5, np.uint8)
    arr = dict(episode_length=rng.choice(np.array([0, 6, 7, 8, 14, 2 ** 31 - 1], np.int32), N).astype(np.int32), mask=m,
               mask2=m2 if m2 is not None else np.zeros(N, np.uint8), draws=rng.random((N, 3)).astype(F), state=state,
               selected=rng.integers(0, 4, N).astype(np.int64), wave_flags=flags)
    sc = {"num_envs": N, "mode": mode, "resample_steps": steps, "num_gaits": G, "seed": 0x0BADC0DE12345678, "stream": (2 << 40) | 31,
          "env_offset": 0, "fixed_clearance_mask": fixed, "cum_weight": cum_weights(G), "gait_offsets": GAIT_TABLE,
          "clearance_lo": 0.05, "clearance_hi": 0.12, "period_lo": 0.3, "period_hi": 0.6, "dt": float(DT), "two_pi": float(TWO_PI)}
    null = set()
    if m2 is None:
        null.add("mask2")
    if philox_draws:
        null.add("draws")
    return Spec("gait_step", sc, arr, null)


def consistent_flags(spec):
    """Start the swing / stance bytes from the rows as they are (what the host keeps true), instead of the sentinel."""
    N = spec.sc["num_envs"]
    byte = foot_flags(spec.arr["state"][:, 15], spec.arr["state"][:, 0:4], spec.sc["two_pi"])
    for b in range((N + 63) // 64):
        spec.arr["wave_flags"][b] = np.bitwise_or.reduce(byte[64 * b:64 * b + 64])
    return spec


# ---- the case tables: name -> builder ---------------------------------------------------------------------------------------------------
RESET, COMMAND, GAIT = {}, {}, {}


def _case(table, name):
    def deco(fn):
        table[name] = fn
        return fn
    return deco


def _tweak(spec, null=(), keep=(), stats=None, **sc):
    spec.null |= set(null)
    spec.null -= set(keep)
    spec.sc.update(sc)
    if stats is not None:
        spec.stats = stats
    return spec


for _n in SIZES:
    RESET["size_%d" % _n] = functools.partial(reset_spec, _n, D=12 if _n < 4097 else 28, T=5)
    RESET["size_%d_spawn_dense" % _n] = functools.partial(reset_spec, _n, D=3, T=24, philox_draws=False, spawn=True)
    RESET["size_%d_random_quotients" % _n] = functools.partial(reset_spec, _n, D=1, T=7, exact=False)
for _k in MASK_KINDS:
    RESET["mask_" + _k] = functools.partial(reset_spec, 130, mask=_k)
# the term table
for _t in (0, 1, 23, 24):
    RESET["terms_%d" % _t] = functools.partial(reset_spec, 130, T=_t, D=1)
for _name, _bits in (("bit0", 1), ("bit23", 1 << 23), ("alternating", 0x555555), ("all", 0xFFFFFF)):
    RESET["log_mask_" + _name] = (lambda bits=_bits: _tweak(reset_spec(130, T=24, D=1), reward_log_mask=bits))
RESET["logging_off"] = lambda: _tweak(reset_spec(130), reward_logging=0)
RESET["sums_null"] = lambda: _tweak(reset_spec(130), null=["episode_sums"])
RESET["seconds_null"] = lambda: _tweak(reset_spec(130), null=["episode_seconds"])
RESET["stats_null"] = lambda: _tweak(reset_spec(130), stats=False)


@_case(RESET, "poison_bystander")
def _poison_bystander():
    """A non-reset env with NaN / inf sums and 0 seconds shares a wave with reset envs: the statistics stay finite, its rows stay."""
    s = reset_spec(130, T=4, mask="first")
    s.arr["mask"][[9, 70]] = 1
    for n in (1, 10, 69, 129):
        s.arr["episode_sums"][:, n] = [np.nan, np.inf, -np.inf, 1.0]
        s.arr["episode_seconds"][n] = 0.0
    return s


@_case(RESET, "poison_reset_env")
def _poison_reset_env():
    """Reset envs with episode_seconds == 0: +inf, -inf and (0 / 0) NaN, as the division says."""
    s = reset_spec(130, T=3, mask="first")
    s.arr["mask"][[9, 70]] = 1
    s.arr["episode_seconds"][[0, 70]] = 0.0
    s.arr["episode_sums"][:, 0] = [2.5, -2.5, 0.0]
    s.arr["episode_sums"][:, 70] = [0.25, -1.0, 1.0]
    return s


for _d in (1, 3, 4, 5, 12, 13, 28):
    RESET["dofs_%d_philox" % _d] = functools.partial(reset_spec, 130, D=_d, T=1, links=())
    RESET["dofs_%d_dense" % _d] = functools.partial(reset_spec, 130, D=_d, T=1, links=(), philox_draws=False)
RESET["dof_noise_zero"] = lambda: _tweak(reset_spec(130, D=5), dof_noise_scale=0.0)
RESET["dof_vel_null"] = lambda: _tweak(reset_spec(130, D=5), null=["scene_dof_vel"])


@_case(RESET, "episode_length_ties")
def _length_ties():
    """(2u - 1) · 2 is exact for every draw: 99.5 -> 100, 100.5 -> 100, 101.5 -> 102 (half to even), -2 and just under +2."""
    s = _tweak(reset_spec(130, mask="all", philox_draws=False), base_max_episode_length=100, max_random_scaling=2.0)
    s.arr["len_draws"][:] = np.resize(np.array([0.375, 0.625, 0.875, 0.0, 1.0 - 2.0 ** -24], F), 130)
    return s


RESET["episode_length_scaling_zero"] = lambda: _tweak(reset_spec(130), max_random_scaling=0.0)
for _name, _links in (("none", ()), ("one", (1,)), ("four", (1, 4, 7, 4))):
    RESET["air_" + _name] = functools.partial(reset_spec, 130, links=_links)
RESET["air_two_arrays_null"] = lambda: _tweak(reset_spec(130, links=(4, 7, 1)), null=["air_state.1.1", "air_state.1.2"])
RESET["pose_fixed_keep_quat"] = lambda: _tweak(reset_spec(130), set_quat=0)
RESET["pose_keep_velocity"] = lambda: _tweak(reset_spec(130), zero_velocity=0)
for _k in ("scene_lin_vel", "scene_ang_vel", "scene_dof_vel"):
    RESET["pose_zero_velocity_%s_null" % _k] = (lambda k=_k: _tweak(reset_spec(130), null=[k]))
RESET["pose_stash_null"] = lambda: _tweak(reset_spec(130), null=["quat_stash"])
RESET["pose_quat_null"] = lambda: _tweak(reset_spec(130), null=["scene_quat"])
RESET["pose_section_off"] = lambda: _tweak(reset_spec(130), null=["scene_pos"])
RESET["dof_section_off"] = lambda: _tweak(reset_spec(130), null=["scene_dof_pos"])
RESET["actions_off"] = lambda: _tweak(reset_spec(130), null=["env_actions", "env_last_actions", "episode_length", "max_episode_length"])
for _r in (0, 4, 3, 7, 1, 2, 6):   # the second Philox block is drawn for 1, 2, 3, 6, 7 (bits 0 and 1) only
    RESET["spawn_rot_%d_philox" % _r] = (lambda r=_r: _tweak(reset_spec(130, spawn=True), spawn_rot_mask=r))
    RESET["spawn_rot_%d_dense" % _r] = (lambda r=_r: _tweak(reset_spec(130, spawn=True, philox_draws=False), spawn_rot_mask=r))
RESET["spawn_keep_quat"] = lambda: _tweak(reset_spec(130, spawn=True), spawn_set_quat=0, set_quat=1)
RESET["spawn_flat"] = lambda: _tweak(reset_spec(130, spawn=True), null=["terrain.height_field"])


@_case(RESET, "spawn_field_border")
def _spawn_border():
    """Points on and beyond the first and last column and row (the border taps), and at exact cell corners."""
    s = _tweak(reset_spec(130, spawn=True, philox_draws=False, mask="all"), spawn_x_min=-3.0, spawn_x_span=12.0, spawn_y_min=1.5, spawn_y_span=10.0)
    edge = np.array([0.0, 1.0 - 2.0 ** -24, 0.5, 2.0 ** -24, 1.0, 0.25, 0.999], F)
    s.arr["spawn_draws"][:, 0] = np.resize(edge, 130)
    s.arr["spawn_draws"][:, 1] = np.resize(np.repeat(edge, 7), 130)
    return s


@_case(RESET, "spawn_field_outside")
def _spawn_outside():
    """A spawn area larger than the field: the index is clipped to the border."""
    return _tweak(reset_spec(130, spawn=True, mask="all"), spawn_x_min=-5.0, spawn_x_span=16.0, spawn_y_min=0.0, spawn_y_span=14.0)


@_case(RESET, "spawn_quadrants")
def _spawn_quadrants():
    """Rotation angles 0, π and 2π (and their neighbours): sincos_det changes quadrant at the half angles."""
    s = _tweak(reset_spec(130, spawn=True, philox_draws=False, mask="all"), spawn_rot_lo=[0.0, 0.0, 0.0], spawn_rot_hi=[float(TWO_PI)] * 3)
    u = np.array([0.0, 0.5, 1.0, 0.25, 0.75, 0.5 - 2.0 ** -25, 0.5 + 2.0 ** -24, 1.0 - 2.0 ** -24, 0.125], F)
    s.arr["spawn_draws"][:, 4] = np.resize(u, 130)
    s.arr["spawn_draws"][:, 2] = np.resize(np.repeat(u, 9), 130)
    s.arr["spawn_draws"][:, 3] = np.resize(np.repeat(u, 3), 130)
    return s


RESET["offset_wraps"] = lambda: _tweak(reset_spec(33, spawn=True, mask="all"), env_offset=0xFFFFFFF0)
RESET["shard_whole"] = functools.partial(reset_spec, 130, D=13, T=4, spawn=True, mask="mixed")

# ---- command -------------------------------------------------------------------------------------------------------------------------------
for _r in (1, 3, 4, 5, 8):
    for _p in (True, False):
        COMMAND["ranges_%d_%s" % (_r, "philox" if _p else "dense")] = functools.partial(command_spec, 130, R=_r, mode=CMD_STEP, philox_draws=_p)
for _n in SIZES:
    COMMAND["size_%d_step" % _n] = functools.partial(command_spec, _n, R=3, mode=CMD_STEP)
    COMMAND["size_%d_masked" % _n] = functools.partial(command_spec, _n, R=5, mode=CMD_MASKED)
    COMMAND["size_%d_all" % _n] = functools.partial(command_spec, _n, R=8, mode=CMD_ALL)
COMMAND["step_every_1"] = functools.partial(command_spec, 130, mode=CMD_STEP, steps=1)
COMMAND["step_every_7_no_stats"] = lambda: _tweak(command_spec(130, mode=CMD_STEP, steps=7), stats=False)
for _k in MASK_KINDS:
    COMMAND["mask_" + _k] = functools.partial(command_spec, 130, mode=CMD_MASKED, mask=_k)


@_case(COMMAND, "ranges_degenerate")
def _ranges_degenerate():
    """lo == hi, lo > hi, ±1e30 (hi - lo = 2e30 is still a float32) and ±3e38 (hi - lo overflows to ±inf; the draws are non-zero,
    so there is no 0 · inf)."""
    s = command_spec(130, R=7, mode=CMD_ALL, philox_draws=False)
    s.arr["draws"][:] = np.maximum(s.arr["draws"], F(2.0 ** -24))
    s.sc["lo"] = [0.75, 2.0, -1e30, 1e30, -3e38, 3e38, -0.0, 0.0]
    s.sc["hi"] = [0.75, -2.0, 1e30, -1e30, 3e38, -3e38, 0.0, 0.0]
    return s


COMMAND["offset_wraps"] = lambda: _tweak(command_spec(33, R=8, mode=CMD_ALL), env_offset=0xFFFFFFF0)
COMMAND["shard_whole"] = functools.partial(command_spec, 130, R=5, mode=CMD_STEP)

# ---- gait ----------------------------------------------------------------------------------------------------------------------------------
for _n in SIZES:
    GAIT["size_%d_step" % _n] = functools.partial(gait_spec, _n, mode=CMD_STEP)
    GAIT["size_%d_masked" % _n] = functools.partial(gait_spec, _n, mode=CMD_MASKED)
    GAIT["size_%d_all" % _n] = functools.partial(gait_spec, _n, mode=CMD_ALL)
for _g in (1, 2, 4):
    for _m in (0, 0b0101, 0b1111):
        GAIT["gaits_%d_fixed_%d" % (_g, _m)] = functools.partial(gait_spec, 130, G=_g, mode=CMD_STEP, fixed=_m, steps=1, philox_draws=False)
for _k in MASK_KINDS:
    GAIT["mask_" + _k] = functools.partial(gait_spec, 130, mode=CMD_MASKED, mask=_k)
GAIT["flags_null"] = lambda: _tweak(gait_spec(130, mode=CMD_STEP), null=["wave_flags"])
GAIT["flags_null_masked"] = lambda: _tweak(gait_spec(130, mode=CMD_MASKED), null=["wave_flags"])
GAIT["stats_null"] = lambda: _tweak(gait_spec(130, mode=CMD_STEP), stats=False)
GAIT["masked_65_last_block"] = functools.partial(gait_spec, 65, mode=CMD_MASKED, mask="last")


@_case(GAIT, "inverse_cdf_edges")
def _inverse_cdf():
    """Draw 0 exactly on every cumulative weight (the next gait) and one ulp below (this gait)."""
    s = gait_spec(130, G=4, mode=CMD_ALL, philox_draws=False)
    cw = np.array(s.sc["cum_weight"][:3], F)
    s.arr["draws"][:, 0] = np.resize(np.concatenate([cw, np.nextafter(cw, F(0)), np.nextafter(cw, F(1)), [F(0), F(1.0 - 2.0 ** -24)]]).astype(F), 130)
    return s


@_case(GAIT, "clock_edges")
def _clock_edges():
    """gait_time + dt below the period, exactly on it, between one and two periods, beyond two, and a NaN period; phase + offset
    exactly 1 and 1 - 2^-24.  No env is due (episode_length = 6 of 7): selected is counted as found."""
    s = gait_spec(130, mode=CMD_STEP, steps=7)
    s.arr["episode_length"][:] = 6
    st = s.arr["state"]
    dt = float(DT)
    rows = [(0.5, 0.1), (0.5, 0.5 - dt), (0.5, 0.6), (0.5, 0.5), (0.5, 1.0 - dt), (0.3, 1.3), (0.3, 7.75), (float("nan"), 0.2),
            (0.5, 0.25 - dt), (0.5, 0.25 - dt), (0.5, -0.2), (0.25, 0.25 - dt)]
    for n in range(130):
        st[n, 5], st[n, 14] = rows[n % len(rows)]
    st[8::len(rows), 0:4] = [0.5, F(0.5 - 2.0 ** -24), 0.0, 0.25]   # phase 0.5: sums of 1.0, 1 - 2^-24, 0.5 (phi == π) and 0.75
    s.arr["selected"][[3, 77]] = [-1, 7]                             # neither is one of the four gaits
    return s


@_case(GAIT, "step_all_due")
def _step_all_due():
    """Every env resamples (the period shortens under an old gait_time): selected is counted as just resampled."""
    s = gait_spec(130, mode=CMD_STEP, steps=1)
    s.arr["state"][:, 14] = np.resize(np.array([0.1, 0.45, 0.7, 1.3, 2.9], F), 130)
    return s


@_case(GAIT, "trot_after_reset")
def _trot():
    """One gait, trot offsets (0, 0.5, 0.5, 0), ALL mode: phase 0, so feet 1 and 2 sit exactly on phi == π — stance."""
    s = gait_spec(65, G=1, mode=CMD_ALL)
    s.sc["gait_offsets"] = [list(TROT)] * 4
    return s


TROT_BYTE = 0x01 | (0x02 << 2) | (0x02 << 4) | (0x01 << 6)
GAIT["offset_wraps"] = lambda: _tweak(gait_spec(33, mode=CMD_ALL), env_offset=0xFFFFFFF0)
GAIT["shard_whole"] = lambda: _tweak(gait_spec(130, mode=CMD_STEP), null=["wave_flags"])   # (blocks of 64 differ between the shardings)
TABLES = {"masked_reset": RESET, "command_step": COMMAND, "gait_step": GAIT}


@functools.lru_cache(maxsize=None)
def _spec(fn, name):
    return TABLES[fn][name]()


@functools.lru_cache(maxsize=None)
def case(fn, name, flags_all=False):
    """(spec, arrays as the call must leave them, exact statistics) — built once, shared by the CPU and GPU tests, never modified."""
    spec = _spec(fn, name)
    want, stats = restate(spec, flags_all)
    return spec, want, stats


def shard(spec, lo, hi):
    """Envs [lo, hi) of a spec as a call of their own with env_offset += lo."""
    N = spec.sc["num_envs"]
    arr = {}
    for k, v in spec.arr.items():
        if k == "episode_sums":
            arr[k] = np.ascontiguousarray(v[:, lo:hi])
        elif k == "wave_flags":
            arr[k] = v[:((hi - lo + 63) // 64 + 3) // 4 * 4].copy()
        elif v.ndim >= 1 and v.shape[0] == N and k not in ("default_dof_pos", "terrain.height_field"):
            arr[k] = np.ascontiguousarray(v[lo:hi])
        else:
            arr[k] = v.copy()
    s = Spec(spec.fn, spec.sc, arr, spec.null, spec.stats, spec.exact)
    s.sc["num_envs"], s.sc["env_offset"] = hi - lo, spec.sc["env_offset"] + lo
    return s


# ---- running a spec through the raw C ABI ---------------------------------------------------------------------------------------------------
PAD_ROWS = 64   # rows of sentinel behind every array, inside the checked region: where a store of a lane past num_envs would land


def _ints(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view({1: np.uint8, 4: np.int32, 8: np.int64}[a.itemsize])


def _set(args, name, value):
    obj, parts = args, name.split(".")
    for p in parts[:-1]:
        obj = obj[int(p)] if p.isdigit() else getattr(obj, p)
    last = parts[-1]
    if isinstance(value, (list, tuple)):
        dst = obj[int(last)] if last.isdigit() else getattr(obj, last)
        for i, v in enumerate(value):
            if isinstance(v, (list, tuple)):
                for j, w in enumerate(v):
                    dst[i][j] = w
            else:
                dst[i] = v
    elif last.isdigit():
        obj[int(last)] = value
    else:
        setattr(obj, last, value)


class Launch:
    """One spec's descriptor on guarded buffers of device ``dev``."""

    def __init__(self, dev, spec):
        import torch
        from genesis_forge_amd import _native as nat
        from guarded import Guarded
        self.dev, self.spec = dev, spec
        self.args = nat.PHASE_FUNCS[spec.fn]()
        self.bufs, self.sizes = {}, {}
        for k, v in spec.arr.items():
            pad = PAD_ROWS * (v.size // v.shape[0] if v.ndim > 1 and v.shape[0] else 1)
            g = Guarded(v.size + pad, torch.from_numpy(v[:0].reshape(-1)).dtype, dev, off=spec.offs.get(k, 0))
            g.t[:v.size].copy_(torch.from_numpy(np.ascontiguousarray(v).reshape(-1)))
            self.bufs[k], self.sizes[k] = g, v.size
            if k not in spec.null:
                _set(self.args, k, g.ptr)
        for k, v in spec.sc.items():
            _set(self.args, k, v)
        self.stats0 = np.zeros(SHARDS, np.dtype(nat.GfStepStats))
        for f in ("term_fired", "reset_count", "action_flags", "contact_flags", "resample_count", "gait_count"):
            self.stats0[f] = (1000 + np.arange(SHARDS)).reshape((SHARDS,) + (1,) * (self.stats0[f].ndim - 1))   # counters ADD to what is there
        self.stats = Guarded(self.stats0.nbytes, torch.uint8, dev, init=torch.from_numpy(self.stats0.view(np.uint8).reshape(-1)))
        if spec.stats:
            self.args.stats = self.stats.ptr

    def run(self, backend):
        from guarded import raw_call, sync
        rc = raw_call(backend, self.spec.fn, self.args)
        sync(self.dev)
        return rc

    def got(self, k):
        return self.bufs[k].cpu().numpy()[:self.sizes[k]].reshape(self.spec.arr[k].shape)

    def got_stats(self):
        from genesis_forge_amd import _native as nat
        return self.stats.cpu().numpy().view(np.dtype(nat.GfStepStats))

    def check_untouched(self, what=""):
        """After a refusal: every byte is as it was."""
        self.check(self.spec.arr, None, what)

    def check(self, want, want_stats, what=""):
        spec = self.spec
        for k, v in spec.arr.items():
            g = self.bufs[k]
            w = v if (k in spec.null or want.get(k) is None) else want[k]
            got = g.cpu().numpy()
            a, b = _ints(got[:v.size]), _ints(w)
            if not np.array_equal(a, b):
                i = int(np.nonzero(a != b)[0][0])
                row = i // max(1, v.size // max(1, v.shape[0])) if v.ndim > 1 else i
                raise AssertionError(f"{what}: {spec.fn} {k}{' (NULL in this call)' if k in spec.null else ''} differs at flat index {i} (row {row}): "
                                     f"got {got[:v.size][i]!r}, want {np.ascontiguousarray(w).reshape(-1)[i]!r}; {int((a != b).sum())} elements differ")
            assert bool((g.raw[g.start + v.size * v.itemsize:] == 0xA5).all()), f"{what}: {spec.fn} wrote behind {k} (rows past num_envs)"
            assert g.guards_ok(), f"{what}: {spec.fn} wrote in front of {k}"
        gs = self.got_stats()
        if not spec.stats or want_stats is None:
            assert np.array_equal(gs.view(np.uint8), self.stats0.view(np.uint8)), f"{what}: statistics changed without a stats pointer"
            return
        check_stats(spec, gs, self.stats0, want_stats, what)
        assert self.stats.guards_ok()


def stats_delta(gs, s0):
    out = {f: (gs[f].astype(np.int64) - s0[f].astype(np.int64)).sum(axis=0) for f in ("term_fired", "reset_count", "action_flags", "contact_flags", "resample_count", "gait_count")}
    out["reward_episode_sum"] = gs["reward_episode_sum"]
    return out


def sums_close(got, want_stats, exact, what=""):
    """reward_episode_sum against the exact sum: == when the quotients are dyadic (any order of f64 additions is exact); otherwise
    |got - fsum| <= n_reset · 2^-52 · Σ|per_sec| — n - 1 f64 additions, each off by at most 2^-53 of a partial sum that never exceeds
    Σ|per_sec|, to first order, with a factor of two to spare."""
    for t in range(24):
        w, g = want_stats["reward_episode_sum"][t], float(got[t])
        if math.isnan(w):
            assert math.isnan(g), f"{what}: term {t}: got {g}, want NaN"
        elif exact or math.isinf(w):
            assert g == w, f"{what}: term {t}: got {g!r}, want exactly {w!r}"
        else:
            bound = want_stats["n"] * 2.0 ** -52 * want_stats["abs_sum"][t]
            assert abs(g - w) <= bound, f"{what}: term {t}: |{g!r} - {w!r}| = {abs(g - w):.3e} > {bound:.3e}"


def check_stats(spec, gs, s0, want_stats, what=""):
    d = stats_delta(gs, s0)
    want = dict(term_fired=0, reset_count=0, action_flags=0, contact_flags=0, resample_count=0, gait_count=[0, 0, 0, 0])
    want.update({k: v for k, v in want_stats.items() if k in want})
    for f, w in want.items():
        assert np.array_equal(d[f], np.broadcast_to(np.asarray(w, np.int64), d[f].shape)), f"{what}: {spec.fn} statistics {f}: got {d[f]}, want {w}"
    total = [math.fsum(gs["reward_episode_sum"][:, t].tolist()) if np.isfinite(gs["reward_episode_sum"][:, t]).all()
             else float(np.sum(gs["reward_episode_sum"][:, t])) for t in range(24)]
    if spec.fn == "masked_reset":
        sums_close(total, want_stats, spec.exact, what)
    else:
        assert not any(total), f"{what}: {spec.fn} changed reward_episode_sum"


def run_ops(backend, launches):
    """The launches' descriptors as one gf_run_ops / gfo_run_ops call: (status, failed index)."""
    from genesis_forge_amd import _native as nat
    from guarded import sync
    ops = (nat.GfOp * len(launches))()
    for i, l in enumerate(launches):
        ops[i].phase, ops[i].args = nat.PHASE_OF_FN[l.spec.fn], C.addressof(l.args)
    failed = C.c_int(-1)
    if backend.name == "hip":
        rc = backend.lib.gf_run_ops(ops, len(launches), backend._stream(), C.byref(failed))
    else:
        rc = backend.lib.gfo_run_ops(ops, len(launches), C.byref(failed))
    sync(launches[0].dev)
    return rc, failed.value


# ---- groups both test files run, once per backend -------------------------------------------------------------------------------------------
def run_case(backend, dev, fn, name, flags_all=False):
    spec, want, stats = case(fn, name, flags_all)
    l = Launch(dev, spec)
    assert l.run(backend) == 0, (fn, name)
    l.check(want, stats, name)
    return l, want


def sharding_identity(backend, dev, fn):
    """130 envs in one call == envs [0, 65) and [65, 130) as two calls with env_offset 0 and 65: first on the restatement itself, then
    each shard's call against its restatement (the whole call against its own is the table's ``shard_whole`` case)."""
    spec, want, stats = case(fn, "shard_whole")
    whole = Spec(fn, spec.sc, {k: (spec.arr[k] if want[k] is None else want[k]) for k in spec.arr}, spec.null)
    counts = {}
    for lo, hi in ((0, 65), (65, 130)):
        part = shard(spec, lo, hi)
        w, s = restate(part)
        expect = shard(whole, lo, hi).arr
        for k in part.arr:
            if w[k] is not None:
                assert np.array_equal(_ints(w[k]), _ints(expect[k])), f"{fn}: the restatement of envs [{lo}, {hi}) differs from the whole in {k}"
        l = Launch(dev, part)
        assert l.run(backend) == 0
        l.check(w, s, f"{fn} shard [{lo}, {hi})")
        for k, v in s.items():
            counts[k] = np.asarray(v, np.float64) + counts.get(k, 0)
    for k in ("reset_count", "resample_count", "gait_count", "reward_episode_sum"):   # (dyadic quotients: the f64 sums add exactly)
        if k in stats:
            assert np.array_equal(counts[k], np.asarray(stats[k], np.float64)), (fn, k)


def refusal(backend, dev, spec, name):
    """``name`` one float off a 16-byte boundary: GF_E_UNSUPPORTED, and not a byte changes.  Nothing is launched."""
    spec.offs[name] = 1
    l = Launch(dev, spec)
    assert l.bufs[name].ptr % 16 == 4
    assert l.run(backend) == E_UNSUPPORTED, f"{spec.fn} accepted a misaligned {name}"
    l.check_untouched(f"refused {name}")
