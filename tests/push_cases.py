"""Restatement and inputs for tests/test_push.py: gf_push's contract (include/gf_step.h) in numpy — float32 array operations, one
rounding each (IEEE add and multiply are correctly rounded there as on the GPU, nothing is fused), integer sums modulo 2^32 —, the
Philox draws of the kernel's block layout, and the sizes and flagging patterns the kernel is walked through.  Nothing here imports
the HIP library."""
import numpy as np

import philox

BLOCK = 256            # GF_PUSH_BLOCK_ENVS: envs per workgroup (asserted against the binding in the tests)
WAVE = 64
SEED_TAG = 0x9D15B0057ED5EEDB   # GF_PUSH_SEED_TAG (asserted against the binding in the tests)
F = np.float32
COMPONENTS = ("x", "y", "z", "roll", "pitch", "yaw")

#: N at 1, around the wave, around the workgroup's env count, and a size of several workgroups that is no multiple of a wave
SIZES = [1, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1, 1000]

#: every single component alone, x and y (the default: no angular block), all six, and none
COMP_MASKS = [1 << j for j in range(6)] + [0x03, 0x3F, 0x00]


def philox_draws(seed, step, n, env_offset, comp_mask, global_timer):
    """[n, 7] (u0 … u6): key seed ^ SEED_TAG, counter (n + env_offset modulo 2^32, block, step, 0).  Block 0 gives (u0, u1, u2, u3),
    block 1 (u4, u5, u6) — taken only when an angular component is enabled, NaN otherwise: a value that is never drawn must never be
    used.  With ``global_timer`` u3 is the fourth word of the block with counter (0xFFFFFFFF, 0, step, 0) for every env."""
    key = (int(seed) ^ SEED_TAG) & 0xFFFFFFFFFFFFFFFF
    step = int(step) & 0xFFFFFFFF
    ids = ((np.arange(n, dtype=np.uint64) + np.uint64(env_offset)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    u = np.full((n, 7), np.nan, dtype=F)
    u[:, 0:4] = philox.block_uniform(key, step, ids, 0)
    if global_timer:
        u[:, 3] = philox.block_uniform(key, step, np.array([0xFFFFFFFF], dtype=np.uint32), 0)[0, 3]
    if comp_mask & 0x38:
        u[:, 4:7] = philox.block_uniform(key, step, ids, 1)[:, 0:3]
    return u


def base_cfg(**kw):
    """The descriptor's scalars."""
    cfg = dict(step=100, interval_lo=3, interval_hi=9, mode=0, comp_mask=0x03, global_timer=0, scale=1.0,
               lo=(-0.5, -0.75, -0.1, -1.0, -0.25, 0.125), hi=(0.5, 0.25, 0.3, 1.0, 0.75, 2.0))
    cfg.update(kw)
    return cfg


def reference(st, cfg, u):
    """The launch on a state ``st`` (a dict of numpy arrays; None for an absent buffer): returns the state after it and ``fire``.
    ``cfg`` holds the descriptor's scalars, ``u`` the [N, 7] draws."""
    out = {k: (None if v is None else np.array(v, copy=True)) for k, v in st.items()}
    n = st["due"].shape[0]
    step = np.uint32(int(cfg["step"]) & 0xFFFFFFFF)
    done = np.zeros(n, dtype=bool)
    if not cfg["global_timer"]:
        for k in ("mask", "mask2"):
            if st.get(k) is not None:
                done = done | st[k].astype(bool)
    late = np.full(n, step, dtype=np.uint32) - st["due"].astype(np.int32).view(np.uint32)     # modulo 2^32
    fire = ~done & (late.view(np.int32) >= 0)
    w = int(cfg["interval_hi"]) - int(cfg["interval_lo"]) + 1
    work = done | fire
    prod = u[:, 3] * F(w)
    assert prod.dtype == F
    r = np.minimum(np.where(work, prod, F(0)).astype(np.int32), w - 1)     # (a row that does no work may hold anything, NaN included)
    nxt = (np.full(n, step, dtype=np.uint32) + np.uint32(cfg["interval_lo"]) + r.astype(np.uint32)).view(np.int32)
    out["due"][work] = nxt[work]
    for j in range(6):
        if not (cfg["comp_mask"] & (1 << j)):
            continue
        vel = out["lin_vel"] if j < 3 else out["ang_vel"]
        lo, hi = F(cfg["lo"][j]), F(cfg["hi"][j])
        v = (u[:, j if j < 3 else j + 1] * (hi - lo) + lo) * F(cfg["scale"])
        assert v.dtype == F
        col = vel[:, j % 3]
        col[fire] = (col + v)[fire] if cfg["mode"] else v[fire]
    if st.get("fired") is not None:
        out["fired"] = fire.astype(np.uint8)
    out["counts"] = st["counts"] + np.array([fire.sum()], dtype=np.int32)
    return out, fire


def random_state(n, seed, with_ang=True):
    """Velocities, a counter that is not zero, timers far in the future (nothing is due) and no masks: the patterns edit it."""
    rng = np.random.default_rng(seed)
    return {"due": np.full(n, 1 << 20, dtype=np.int32), "lin_vel": rng.normal(size=(n, 3)).astype(F),
            "ang_vel": rng.normal(size=(n, 3)).astype(F) if with_ang else None, "fired": np.full(n, 7, dtype=np.uint8),
            "counts": np.array([11], dtype=np.int32), "mask": np.zeros(n, dtype=bool), "mask2": np.zeros(n, dtype=bool)}


PATTERNS = ["none", "one_lane", "all", "done_and_due", "no_mask2", "no_masks"]


def apply_pattern(st, which, step, seed=0):
    """Timers and masks of the named flagging pattern, for a launch at ``step``."""
    n = st["due"].shape[0]
    rng = np.random.default_rng(seed + 1000)
    step = int(step)
    if which == "none":                    # nothing is due and nobody is done: every wave leaves after the ballot
        pass
    elif which == "one_lane":              # exactly one lane of one wave (the last wave's, not its first lane where it has more)
        st["due"][max(n - 2, 0)] = step
    elif which == "all":                   # due now, or overdue by up to 40 steps
        st["due"][:] = step - rng.integers(0, 41, n)
    elif which == "done_and_due":          # a third done and due, a third done and not due, a sixth each due only / neither
        kind = rng.integers(0, 6, n)
        st["due"][(kind == 0) | (kind == 1) | (kind == 4)] = step - 1
        st["mask"][(kind == 0) | (kind == 2)] = True
        st["mask2"][(kind == 1) | (kind == 3)] = True
    elif which == "no_mask2":
        st["due"][rng.random(n) < 0.5] = step
        st["mask"][rng.random(n) < 0.3] = True
        st["mask2"] = None
    elif which == "no_masks":
        st["due"][rng.random(n) < 0.5] = step
        st["mask"] = st["mask2"] = None
    else:
        raise KeyError(which)
    return st


def dense_draws(n, seed, nan_cols=()):
    """[n, 7] U[0, 1) draws for parity mode; ``nan_cols`` are planted with NaN."""
    u = np.random.default_rng(seed + 5).random((n, 7)).astype(F)
    u[u >= 1.0] = 0.5
    for c in nan_cols:
        u[:, c] = np.nan
    return u
