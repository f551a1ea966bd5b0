"""Restatement and inputs for tests/test_terrain_curriculum.py: gf_terrain_curriculum's contract (include/gf_step.h) in numpy
float32 array operations, one rounding each — IEEE add, multiply and square root are correctly rounded there as on the GPU, and
nothing is fused —, the Philox draws of the kernel's block layout, random states that take every branch, and the sizes the kernel is
walked through.  Nothing here imports the HIP library."""
import numpy as np

import philox

BLOCK = 256            # GF_TERRAIN_CURRICULUM_BLOCK_ENVS: envs per workgroup (asserted against the binding in the tests)
WAVE = 64
SPAWN_BLOCK = 0x100000  # GF_SPAWN_BLOCK
F = np.float32

#: N at 1, around the wave, around the workgroup's env count, and one above twice that count
SIZES = [1, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1]


def sincos_det(x):
    """sincos_det of csrc/gf_device.h."""
    x = np.asarray(x, dtype=F)
    k = np.rint(x * F(0.63661977236758134))
    r = x - k * F(1.5703125)
    r = r - k * F(4.837512969970703125e-4)
    r = r - k * F(7.54978995489188216e-8)
    z = r * r
    ps = ((F(-1.9515295891e-4) * z + F(8.3321608736e-3)) * z - F(1.6666654611e-1)) * z * r + r
    pc = ((F(2.443315711809948e-5) * z - F(1.388731625493765e-3)) * z + F(4.166664568298827e-2)) * z * z - F(0.5) * z + F(1.0)
    q = k.astype(np.int32) & 3
    odd = (q & 1) != 0
    sv, cv = np.where(odd, pc, ps), np.where(odd, ps, pc)
    return np.where((q & 2) != 0, -sv, sv).astype(F), np.where(((q + 1) & 2) != 0, -cv, cv).astype(F)


def xyz_to_quat_det(ax, ay, az):
    sx, cx = sincos_det(ax * F(0.5))
    sy, cy = sincos_det(ay * F(0.5))
    sz, cz = sincos_det(az * F(0.5))
    q = np.stack([(cx * cy) * cz + (sx * sy) * sz, (sx * cy) * cz - (cx * sy) * sz,
                  (cx * sy) * cz + (sx * cy) * sz, (cx * cy) * sz - (sx * sy) * cz], axis=-1)
    assert q.dtype == F
    return q


def philox_draws(seed, stream, n, env_offset, rot_mask):
    """[n, 6] (x, y, rot x, rot y, rot z, level): block GF_SPAWN_BLOCK gives (u0, u1, u4, u5), block GF_SPAWN_BLOCK + 1 (u2, u3) —
    taken only when an x or y rotation is drawn —, counter n + env_offset (modulo 2^32)."""
    ids = ((np.arange(n, dtype=np.uint64) + np.uint64(env_offset)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    b0 = philox.block_uniform(seed, stream, ids, SPAWN_BLOCK)
    u = np.zeros((n, 6), dtype=F)
    u[:, 0], u[:, 1], u[:, 4], u[:, 5] = b0[:, 0], b0[:, 1], b0[:, 2], b0[:, 3]
    if rot_mask & 3:
        b1 = philox.block_uniform(seed, stream, ids, SPAWN_BLOCK + 1)
        u[:, 2], u[:, 3] = b1[:, 0], b1[:, 1]
    return u


def decide(dist, level, speed_ref, cfg, u5):
    """Steps 2 and 4 for arrays: returns (new level, up, down, wrapped)."""
    up = dist > F(cfg["promote_distance"])
    thr = speed_ref * F(cfg["demote_time"]) if speed_ref is not None else np.full_like(dist, F(cfg["demote_distance"]))
    down = ~up & (dist < thr)
    l = level.astype(np.int32) + up.astype(np.int32) - down.astype(np.int32)
    L = int(cfg["num_levels"])
    wrapped = l >= L
    r = np.minimum((u5 * F(L)).astype(np.int32), L - 1)
    l = np.where(wrapped, r, l)
    l = np.maximum(l, 0)
    return l.astype(np.int32), up, down, wrapped


def positions(l, typ, u, cfg):
    """Steps 5 and 6 without the height: (x, y)."""
    ix, iy = (l, typ) if cfg["level_axis"] == 0 else (typ, l)
    x = (u[:, 0] * F(cfg["spawn_x_span"]) + F(cfg["spawn_x_min"])) + ix.astype(F) * F(cfg["cell_dx"])
    y = (u[:, 1] * F(cfg["spawn_y_span"]) + F(cfg["spawn_y_min"])) + iy.astype(F) * F(cfg["cell_dy"])
    assert x.dtype == F and y.dtype == F
    return x, y


def reference(st, cfg, u, height):
    """The launch on a state ``st`` (a dict of numpy arrays; None for an absent buffer): returns the state after it.  ``cfg`` holds
    the descriptor's scalars, ``u`` the [N, 6] draws, ``height(x, y)`` the terrain height at float32 arrays (the shared sampler is
    checked against gf_terrain_height by the caller)."""
    out = {k: (None if v is None else np.array(v, copy=True)) for k, v in st.items()}
    n = st["pos_in"].shape[0]
    m = st["mask"].astype(bool)
    if st.get("mask2") is not None:
        m = m | st["mask2"].astype(bool)
    level, typ = st["level"].astype(np.int32), st["type"].astype(np.int32)
    up = down = wrapped = np.zeros(n, dtype=bool)
    l = level
    if cfg["update"]:
        dx = st["pos_in"][:, 0] - st["spawn_xy"][:, 0]
        dy = st["pos_in"][:, 1] - st["spawn_xy"][:, 1]
        dist = np.sqrt(dx * dx + dy * dy)
        assert dist.dtype == F
        l, up, down, wrapped = decide(dist, level, st.get("speed_ref"), cfg, u[:, 5])
    x, y = positions(l, typ, u, cfg)
    z = (height(x, y).astype(F) + F(cfg["height_offset"])).astype(F)
    out["pos_out"][m] = np.stack([x, y, z], axis=-1)[m]
    if cfg["set_quat"]:
        ang = []
        for k in range(3):
            lo, hi = F(cfg["rot_lo"][k]), F(cfg["rot_hi"][k])
            ang.append(u[:, 2 + k] * (hi - lo) + lo if cfg["rot_mask"] & (1 << k) else np.zeros(n, dtype=F))
        q = xyz_to_quat_det(*ang)
        if st.get("stash") is not None:
            out["stash"][m] = st["quat"][m]
        out["quat"][m] = q[m]
    if cfg["zero_velocity"]:
        for k in ("lin_vel", "ang_vel", "dof_vel"):
            if st.get(k) is not None:
                out[k][m] = 0.0
    out["spawn_xy"][m] = np.stack([x, y], axis=-1)[m]
    out["level"][m] = l[m]
    if st.get("command") is not None:
        cx, cy = st["command"][:, 0], st["command"][:, 1]
        out["speed_ref"][m] = np.sqrt(cx * cx + cy * cy)[m]
    out["counts"] = st["counts"] + np.array([(up & m).sum(), (down & m).sum(), (wrapped & m).sum()], dtype=np.int32)
    return out, (x, y)


def random_state(n, seed, cfg, dofs=12, cmd_width=3, with_speed=True, with_command=True):
    """A state whose flagged envs take every branch: a third walked past promote_distance, a third stayed put (demoted where the
    reference speed allows), the rest in between; levels over the whole range, the top level included (promotions there wrap)."""
    rng = np.random.default_rng(seed)
    L, T = int(cfg["num_levels"]), int(cfg["num_types"])
    spawn = rng.uniform(-6.0, 6.0, (n, 2)).astype(F)
    kind = rng.integers(0, 3, n)
    reach = np.where(kind == 0, rng.uniform(1.5, 3.0, n), np.where(kind == 1, rng.uniform(0.0, 0.2, n), rng.uniform(0.4, 0.9, n))) * cfg["promote_distance"]
    ang = rng.uniform(-np.pi, np.pi, n)
    pos = np.concatenate([spawn + (reach[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=-1)).astype(F),
                          rng.uniform(0.2, 0.6, (n, 1)).astype(F)], axis=-1).astype(F)
    q = rng.normal(size=(n, 4)).astype(F)
    st = {
        "pos_in": pos, "pos_out": pos.copy(), "quat": (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(F),
        "stash": rng.normal(size=(n, 4)).astype(F), "lin_vel": rng.normal(size=(n, 3)).astype(F), "ang_vel": rng.normal(size=(n, 3)).astype(F),
        "dof_vel": rng.normal(size=(n, dofs)).astype(F), "spawn_xy": spawn, "level": rng.integers(0, L, n).astype(np.int32),
        "type": rng.integers(0, T, n).astype(np.int32),
        "speed_ref": rng.uniform(0.0, 1.5, n).astype(F) if with_speed else None,
        "command": rng.uniform(-1.0, 1.0, (n, cmd_width)).astype(F) if with_command else None,
        "counts": np.array([3, 5, 7], dtype=np.int32), "mask": np.zeros(n, dtype=bool), "mask2": None,
    }
    return st


def masks(n, which, seed=0):
    """(mask, mask2) of the named pattern."""
    rng = np.random.default_rng(seed)
    z = np.zeros(n, dtype=bool)
    if which == "none":
        return z, None
    if which == "all":
        return ~z, None
    if which == "one_per_wave":   # exactly one lane of every wave, a different one each
        m = z.copy()
        for w in range((n + WAVE - 1) // WAVE):
            m[min(w * WAVE + (17 * w + 5) % WAVE, n - 1)] = True
        return m, None
    if which == "last":
        m = z.copy()
        m[n - 1] = True
        return m, None
    if which == "mask2_only":
        return z, rng.random(n) < 0.5
    if which == "both":
        return rng.random(n) < 0.3, rng.random(n) < 0.3
    raise KeyError(which)


def base_cfg(**kw):
    """The descriptor's scalars.  Four cells along either axis, all on the committed terrain fixture's field (x in [-3, 9], y in
    [1.5, 11.5]): x in [-2.75, 8.75], y in [1.75, 11.25] whichever axis carries the levels — every height is an interior sample."""
    cfg = dict(num_levels=4, num_types=3, level_axis=0, update=1, set_quat=1, zero_velocity=1, rot_mask=4, promote_distance=2.0,
               demote_time=1.25, demote_distance=0.5, spawn_x_min=-2.75, spawn_x_span=2.5, spawn_y_min=1.75, spawn_y_span=2.0,
               cell_dx=3.0, cell_dy=2.5, height_offset=0.4, rot_lo=(-0.3, -0.2, 0.0), rot_hi=(0.3, 0.2, 6.2831853))
    cfg.update(kw)
    return cfg
