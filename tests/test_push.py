"""Random pushes: gf_push (csrc/gf_push.hip, contract in include/gf_step.h), managers.PushDisturbance and
Go2RoughTerrainEnv(push=…).

CPU: the binding, every refusal of the entry (before any HIP call: they run without a GPU), the ValueErrors, PushDisturbance's torch
composition (_step_torch, the oracle backend has no push entry) against the numpy restatement (push_cases.reference) over the
sizes, flagging patterns, modes, component subsets, intervals, counter wraps and offsets, the env hook, the setter path.  GPU: the
kernel raw through the C ABI over the same matrix, every output a slice of a Guarded buffer, the kernel against _step_torch on the
device, the env recorded against ordinary.

Every comparison is exact: the restatement rounds once per operation, as the kernel does."""
import ctypes as C

import numpy as np
import pytest
import torch

import push_cases as pc
from guarded import Guarded, raw_call, sync

GF_OK, GF_E_NULL, GF_E_RANGE = 0, -1, -2   # include/gf_step.h
INF, NAN = float("inf"), float("nan")
M32 = 0xFFFFFFFF
OUT = ("due", "lin_vel", "ang_vel", "fired", "counts")


# ---------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------
def _lib(nat):
    lib = C.CDLL(nat.lib_path())
    lib.gf_push.restype = C.c_int
    lib.gf_push.argtypes = [C.c_void_p, C.c_void_p]
    return lib


def _fill(a, cfg):
    a.step, a.interval_lo, a.interval_hi = int(cfg["step"]) & M32, cfg["interval_lo"], cfg["interval_hi"]
    a.mode, a.comp_mask, a.global_timer, a.scale = cfg["mode"], cfg["comp_mask"], cfg["global_timer"], cfg["scale"]
    for j in range(6):
        a.lo[j], a.hi[j] = cfg["lo"][j], cfg["hi"][j]


def _valid_args(nat, n=4):
    """A descriptor gf_push accepts.  Its pointers are never followed: every case it is used in is refused, or has no envs."""
    a = nat.GfPushArgs()
    a.num_envs = n
    for f in ("mask", "mask2", "due", "lin_vel", "ang_vel", "fired", "counts", "draws"):
        setattr(a, f, 0x1000)
    _fill(a, pc.base_cfg(comp_mask=0x3F))
    return a


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    bad = _bits(got) != _bits(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0].tolist()}"


def _i32(v):
    """Python ints modulo 2^32 as int32."""
    return (np.asarray(v, dtype=np.int64) & M32).astype(np.uint32).view(np.int32)


class _Entity:
    """An entity with masked setters: the launch writes its velocity tensors in place."""

    def __init__(self, lin, ang):
        self.lin_vel, self.ang_vel = lin, ang

    def gf_masked_base(self):
        return None, None, self.lin_vel, self.ang_vel


class _Env:
    """The smallest env a PushDisturbance needs; ``dt`` of one second: ``interval_s`` is in steps."""

    def __init__(self, n, backend, robot=None, seed=0x1234, env_offset=0):
        self.num_envs, self.backend, self.robot, self.dt = n, backend, robot, 1.0
        self._rng_seed, self.env_offset = seed, env_offset

    def next_stream(self):
        raise AssertionError("PushDisturbance must not take a stream id from the env")


def _ranges(cfg):
    return {pc.COMPONENTS[j]: (cfg["lo"][j], cfg["hi"][j]) for j in range(6) if cfg["comp_mask"] & (1 << j)}


def _manager(n, backend, cfg, robot, key=(0x1234, 0)):
    from genesis_forge_amd.managers import PushDisturbance

    env = _Env(n, backend, robot, *key)
    pd = PushDisturbance(env, interval_s=(cfg["interval_lo"], cfg["interval_hi"]), velocity_range=_ranges(cfg),
                         mode="add" if cfg["mode"] else "set", per_env=not cfg["global_timer"], scale=cfg["scale"])
    assert (pd.interval_lo, pd.interval_hi, pd.comp_mask) == (cfg["interval_lo"], cfg["interval_hi"], cfg["comp_mask"])
    return env, pd


def run_manager(st, cfg, u=None, key=(0x1234, 0), dev="cpu", use_kernel=True):
    """One PushDisturbance.step on copies of ``st``; returns the state after it.  (With ``dev='cpu'`` and the oracle backend this is
    _step_torch.)"""
    from genesis_forge_amd import _native as nat

    n = st["due"].shape[0]
    T = lambda arr: None if arr is None else torch.from_numpy(np.ascontiguousarray(arr)).clone().to(dev)
    robot = _Entity(T(st["lin_vel"]), T(st["ang_vel"]))
    _env, pd = _manager(n, nat.get_backend(), cfg, robot, key)
    pd.build()
    _same(robot.lin_vel.cpu().numpy(), st["lin_vel"], "build() pushes nobody")
    assert int(pd.counts.item()) == 0
    pd.use_kernel = use_kernel
    pd.due.copy_(T(st["due"]))
    pd.counts.copy_(T(st["counts"]))
    pd._fired.copy_(T(st["fired"]))
    pd._step = (int(cfg["step"]) - 1) & M32
    pd.step(T(st["mask"]), T(st["mask2"]), draws=T(u))
    assert pd.fired.dtype == torch.bool and pd.fired.data_ptr() == pd._fired.data_ptr()
    sync(dev)
    return {"due": pd.due.cpu().numpy(), "lin_vel": robot.lin_vel.cpu().numpy(), "ang_vel": robot.ang_vel.cpu().numpy(),
            "fired": pd._fired.cpu().numpy(), "counts": pd.counts.cpu().numpy()}


def _raw_buffers(st, dev, off=0, init=True):
    n = st["due"].shape[0]
    G = lambda arr, dt, o=0: Guarded(arr.size, dt, dev, off=o, init=torch.from_numpy(np.ascontiguousarray(arr)) if init else None)
    g = {"due": G(st["due"], torch.int32), "lin_vel": G(st["lin_vel"], torch.float32, off), "fired": G(st["fired"], torch.uint8),
         "counts": G(st["counts"], torch.int32)}
    if st["ang_vel"] is not None:
        g["ang_vel"] = G(st["ang_vel"], torch.float32, off)
    return g, n


def _raw_args(nat, st, cfg, g, n, keep, u=None, key=None, dev="cuda"):
    T = lambda arr: keep.append(torch.from_numpy(np.ascontiguousarray(arr)).to(dev)) or keep[-1]
    a = nat.GfPushArgs()
    a.num_envs = n
    a.mask = None if st["mask"] is None else T(st["mask"]).data_ptr()
    a.mask2 = None if st["mask2"] is None else T(st["mask2"]).data_ptr()
    a.due, a.lin_vel, a.fired, a.counts = g["due"].ptr, g["lin_vel"].ptr, g["fired"].ptr, g["counts"].ptr
    a.ang_vel = g["ang_vel"].ptr if "ang_vel" in g else None
    if u is not None:
        a.draws = T(u).data_ptr()
    else:
        a.seed, a.env_offset = key
    _fill(a, cfg)
    return a


def run_raw(st, cfg, u=None, key=(0x1234, 0), off=0, no_fired=False):
    """One gf_push launch on copies of ``st`` in Guarded buffers through the binding; returns the state after it."""
    from genesis_forge_amd import _native as nat

    dev, keep = "cuda", []
    g, n = _raw_buffers(st, dev, off)
    a = _raw_args(nat, st, cfg, g, n, keep, u, key)
    if no_fired:
        a.fired = None
    nat.get_backend().push(a)
    sync(dev)
    assert all(v.guards_ok() for v in g.values()), "a write outside a buffer"
    shapes = {"due": (n,), "lin_vel": (n, 3), "ang_vel": (n, 3), "fired": (n,), "counts": (1,)}
    after = {k: v.cpu().numpy().reshape(shapes[k]).copy() for k, v in g.items()}
    after.setdefault("ang_vel", None)
    return after


def _check(run, st, cfg, u=None, key=(0x1234, 0), what="", **kw):
    """``run`` against the restatement, every output bit for bit.  Returns (after, fire)."""
    after = run(st, cfg, u=u, key=key, **kw)
    draws = u if u is not None else pc.philox_draws(key[0], cfg["step"], st["due"].shape[0], key[1], cfg["comp_mask"], cfg["global_timer"])
    want, fire = pc.reference(st, _cfg32(cfg), draws)
    for k in OUT:
        if want[k] is None:
            assert after[k] is None
        elif kw.get("no_fired") and k == "fired":
            _same(after[k], st[k], f"{what}: fired (not given: untouched)")
        else:
            _same(after[k], want[k], f"{what}: {k}")
    return after, fire


def _cfg32(cfg):
    """The scalars as the descriptor holds them (float fields rounded to float32 once)."""
    return dict(cfg, lo=tuple(np.float32(v) for v in cfg["lo"]), hi=tuple(np.float32(v) for v in cfg["hi"]), scale=np.float32(cfg["scale"]))


# ---------------------------------------------------------------------------------------------------------------------------
# the shared matrix: each takes ``run`` (run_manager on the CPU, run_raw on the GPU)
# ---------------------------------------------------------------------------------------------------------------------------
def sizes_and_patterns(run, n, which):
    cfg = pc.base_cfg(comp_mask=0x3F)
    st = pc.apply_pattern(pc.random_state(n, n), which, cfg["step"], seed=n)
    after, fire = _check(run, st, cfg, u=pc.dense_draws(n, n), what=f"N={n} {which}")
    if which == "none":
        assert not fire.any()
        for k in ("due", "lin_vel", "ang_vel", "counts"):
            _same(after[k], st[k], k)
        assert not after["fired"].any()         # … but `fired` is written by the waves that leave early too
    if which == "one_lane":
        assert fire.sum() == 1 and after["fired"].sum() == 1 and after["counts"][0] == st["counts"][0] + 1
    if which == "all":
        assert fire.all() and after["counts"][0] == st["counts"][0] + n
    if which == "done_and_due" and n >= pc.WAVE:
        done = st["mask"] | st["mask2"]
        due = st["due"] <= cfg["step"]
        assert (done & due).any() and not after["fired"][done].any()            # done and due: not pushed …
        assert (after["due"][done] > cfg["step"]).all()                           # … and a new timer
        _same(after["lin_vel"][done], st["lin_vel"][done], "a done env's velocity")
        assert after["fired"][~done & due].all()


def modes_and_components(run, mode, comp_mask):
    n = pc.BLOCK + 1
    cfg = pc.base_cfg(mode=mode, comp_mask=comp_mask, scale=0.75)
    st = pc.apply_pattern(pc.random_state(n, 3), "no_mask2", cfg["step"], seed=3)
    off = [j for j in range(6) if not comp_mask & (1 << j)]
    for j in off:                                # a NaN planted in a disabled component keeps its bits
        (st["lin_vel"] if j < 3 else st["ang_vel"])[::3, j % 3] = np.float32(np.nan)
    # parity draws of the disabled components are NaN: they must not reach any output (x, y only: block 1's u4 … u6 among them)
    u = pc.dense_draws(n, 4, nan_cols=[j if j < 3 else j + 1 for j in off])
    after, fire = _check(run, st, cfg, u=u, what=f"mode {mode} mask {comp_mask:#x}")
    assert fire.any() and not fire.all()
    for j in off:
        k = "lin_vel" if j < 3 else "ang_vel"
        _same(after[k][:, j % 3], st[k][:, j % 3], f"disabled component {j}")
    for j in range(6):
        if comp_mask & (1 << j):
            k = "lin_vel" if j < 3 else "ang_vel"
            assert np.isfinite(after[k][fire, j % 3]).all()
            assert not np.array_equal(after[k][fire, j % 3], st[k][fire, j % 3])
    # the same launch with Philox: block 1 is taken only with an angular component (philox_draws leaves NaN where it is not)
    _check(run, st, cfg, key=(0xFEED_5EED_0123, 0), what=f"philox, mode {mode} mask {comp_mask:#x}")


def every_step(run):
    """lo == hi == 1: every env fires in every launch."""
    n = pc.WAVE + 1
    cfg = pc.base_cfg(interval_lo=1, interval_hi=1, step=1)
    st = pc.random_state(n, 1)
    st["due"][:] = 1
    for t in range(1, 5):
        cfg["step"] = t
        after, fire = _check(run, st, cfg, key=(7, 0), what=f"step {t}")
        assert fire.all() and (after["due"] == t + 1).all()
        st = dict(st, **after)


def fixed_interval(run, k=5):
    """lo == hi == k: over 3k steps every env fires exactly at k, 2k, 3k."""
    n = pc.WAVE + 1
    cfg = pc.base_cfg(interval_lo=k, interval_hi=k)
    st = pc.random_state(n, 2)
    st["due"][:] = k
    st["counts"][:] = 0
    for t in range(1, 3 * k + 1):
        cfg["step"] = t
        after, fire = _check(run, st, cfg, key=(8, 0), what=f"step {t}")
        assert fire.all() if t % k == 0 else not fire.any(), t
        st = dict(st, **after)
    assert st["counts"][0] == 3 * n


def interval_spread(run):
    """lo < hi, a width of 4, 4 096 envs: every new timer lies in [lo, hi] steps ahead and both ends occur."""
    n = 4096
    cfg = pc.base_cfg(interval_lo=6, interval_hi=9, step=50)
    st = pc.apply_pattern(pc.random_state(n, 5), "all", cfg["step"], seed=5)
    after, fire = _check(run, st, cfg, key=(9, 0), what="spread")
    ahead = after["due"] - cfg["step"]
    assert fire.all() and ahead.min() == 6 and ahead.max() == 9 and set(np.unique(ahead)) == {6, 7, 8, 9}


def counter_wrap(run, edge):
    """``step`` carried across 2^31 and 2^32: timers and the counter seeded just below the wrap; a wide interval puts the new timers
    on the other side of it."""
    n = pc.WAVE + 1
    cfg = pc.base_cfg(interval_lo=2, interval_hi=5)
    st = pc.random_state(n, 6)
    st["due"] = _i32(edge - 3 + (np.arange(n) % 6))          # due at edge - 3 … edge + 2
    st["counts"][:] = 0
    total = 0
    for t in range(edge - 4, edge + 4):
        cfg["step"] = t & M32
        after, fire = _check(run, st, cfg, key=(10, 0), what=f"step {t} around {edge:#x}")
        late = (t - st["due"].astype(np.int64)) & M32
        _same(fire, late < (1 << 31), f"who fires at step {t}")
        ahead = (after["due"].astype(np.int64) - t) & M32
        assert ((ahead[fire] >= 2) & (ahead[fire] <= 5)).all()
        total += int(fire.sum())
        st = dict(st, **after)
    assert total >= n and st["counts"][0] == total


def counts_over_a_run(run):
    """counts equals the sum of `fired` over a 50-step run with random done masks."""
    n = pc.BLOCK + 1
    cfg = pc.base_cfg(interval_lo=2, interval_hi=6, comp_mask=0x09)
    st = pc.random_state(n, 7)
    st["due"][:] = 1 + (np.arange(n) % 5)
    st["counts"][:] = 0
    rng = np.random.default_rng(0)
    total = 0
    for t in range(1, 51):
        cfg["step"] = t
        st["mask"], st["mask2"] = rng.random(n) < 0.05, rng.random(n) < 0.05
        after, fire = _check(run, st, cfg, key=(11, 0), what=f"step {t}")
        total += int(after["fired"].sum())
        st = dict(st, **after)
    assert total > n and st["counts"][0] == total


def env_offset_shifts_the_draws(run):
    n = pc.WAVE + 1
    cfg = pc.base_cfg(comp_mask=0x3F)
    st = pc.apply_pattern(pc.random_state(n, 8), "all", cfg["step"], seed=8)
    outs = [_check(run, st, cfg, key=key, what=f"key {key}")[0]["lin_vel"] for key in ((0x1234_5678_9ABC, 0), (0x1234_5678_9ABC, 4_294_967_290),
                                                                                         (0x1234_5678_9ABD, 0))]
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], outs[2])       # the offset and the seed both matter
    a, _ = _check(run, st, cfg, key=(0x1234_5678_9ABC, 17), what="offset 17")                   # env n at offset 17 draws what env n + 17 draws at offset 0
    big = pc.apply_pattern(pc.random_state(n + 17, 8), "all", cfg["step"], seed=8)
    b, _ = _check(run, big, cfg, key=(0x1234_5678_9ABC, 0), what="offset 0")
    _same(a["due"], b["due"][17:], "shifted timers")


def philox_against_draws(run):
    """The restatement's own unit floats fed as `draws` give what Philox mode gives."""
    n = pc.BLOCK + 1
    for g in (0, 1):
        cfg = pc.base_cfg(comp_mask=0x3F, mode=1, global_timer=g)
        st = pc.apply_pattern(pc.random_state(n, 9), "no_mask2", cfg["step"], seed=9)
        key = (0xABCDEF, 5)
        a, _ = _check(run, st, cfg, key=key, what="philox")
        b, _ = _check(run, st, cfg, u=pc.philox_draws(key[0], cfg["step"], n, key[1], 0x3F, g), what="draws")
        for k in OUT:
            _same(a[k], b[k], k)


def global_timer(run, steps=200):
    """One timer: all `due` stay equal over 200 steps whatever the done masks say, and every env fires in the same steps."""
    n = pc.WAVE + 1
    cfg = pc.base_cfg(interval_lo=3, interval_hi=11, global_timer=1)
    st = pc.random_state(n, 10)
    st["due"][:] = 4
    st["counts"][:] = 0
    rng = np.random.default_rng(1)
    fired_steps = []
    for t in range(1, steps + 1):
        cfg["step"] = t
        masks = [(rng.random(n) < 0.2, rng.random(n) < 0.2), (rng.random(n) < 0.2, None), (None, None)][t % 3]
        st["mask"], st["mask2"] = masks
        after, fire = _check(run, st, cfg, key=(12, 3), what=f"step {t}")
        assert fire.all() or not fire.any()
        assert (after["due"] == after["due"][0]).all()
        if fire.any():
            fired_steps.append(t)
        st = dict(st, **after)
    gaps = np.diff(fired_steps)
    assert fired_steps[0] == 4 and len(fired_steps) > steps // 11 and gaps.min() >= 3 and gaps.max() <= 11 and len(set(gaps.tolist())) > 2


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: binding and refusals
# ---------------------------------------------------------------------------------------------------------------------------
NULL_CASES = {f: (lambda a, f=f: setattr(a, f, None)) for f in ("due", "lin_vel", "counts")}
NULL_CASES["ang_vel_with_angular_components"] = lambda a: setattr(a, "ang_vel", None)
NULL_CASES["ang_vel_with_one_angular_component"] = lambda a: (setattr(a, "ang_vel", None), setattr(a, "comp_mask", 0x20))


def _set(arr, j, v):
    return lambda a: getattr(a, arr).__setitem__(j, v)


RANGE_CASES = {
    "num_envs<0": lambda a: setattr(a, "num_envs", -1),
    "too_many_workgroups": lambda a: setattr(a, "num_envs", (0x7FFFFFFF + 1) * pc.BLOCK),
    "interval_lo=0": lambda a: setattr(a, "interval_lo", 0),
    "interval_lo<0": lambda a: setattr(a, "interval_lo", -3),
    "interval_hi<lo": lambda a: (setattr(a, "interval_lo", 5), setattr(a, "interval_hi", 4)),
    "interval_wider_than_2^24": lambda a: (setattr(a, "interval_lo", 1), setattr(a, "interval_hi", 1 + (1 << 24))),
    "interval_width_overflows": lambda a: (setattr(a, "interval_lo", 1), setattr(a, "interval_hi", 0x7FFFFFFF)),
    "mode=2": lambda a: setattr(a, "mode", 2),
    "mode=-1": lambda a: setattr(a, "mode", -1),
    "global_timer=2": lambda a: setattr(a, "global_timer", 2),
    "global_timer=-1": lambda a: setattr(a, "global_timer", -1),
    "comp_mask=64": lambda a: setattr(a, "comp_mask", 64),
    "comp_mask=-1": lambda a: setattr(a, "comp_mask", -1),
    "lo=nan": _set("lo", 1, NAN), "lo=-inf": _set("lo", 4, -INF), "hi=nan": _set("hi", 5, NAN), "hi=inf": _set("hi", 0, INF),
    "lo=nan_on_a_disabled_component": lambda a: (setattr(a, "comp_mask", 0x03), _set("lo", 2, NAN)(a)),
    "scale=nan": lambda a: setattr(a, "scale", NAN),
    "scale=inf": lambda a: setattr(a, "scale", INF),
    "scale=-inf": lambda a: setattr(a, "scale", -INF),
    "hi<lo_lin": lambda a: (_set("lo", 1, 0.5)(a), _set("hi", 1, 0.25)(a)),
    "hi<lo_ang": lambda a: (_set("lo", 5, 0.5)(a), _set("hi", 5, 0.25)(a)),
}

ACCEPTED = {
    "as_it_is": lambda a: None,
    "bare": lambda a: [setattr(a, f, None) for f in ("mask", "mask2", "fired", "draws")],
    "no_ang_vel_without_angular_components": lambda a: (setattr(a, "ang_vel", None), setattr(a, "comp_mask", 0x07)),
    "no_components": lambda a: (setattr(a, "comp_mask", 0), setattr(a, "ang_vel", None)),
    "hi<lo_on_a_disabled_component": lambda a: (setattr(a, "comp_mask", 0x3B), _set("lo", 2, 0.5)(a), _set("hi", 2, 0.25)(a)),
    "lo==hi": lambda a: (_set("lo", 0, 0.5)(a), _set("hi", 0, 0.5)(a)),
    "interval_2^24_wide": lambda a: (setattr(a, "interval_lo", 1), setattr(a, "interval_hi", 1 << 24)),
    "add_global": lambda a: (setattr(a, "mode", 1), setattr(a, "global_timer", 1)),
    "scale=0": lambda a: setattr(a, "scale", 0.0),
}


def test_binding_matches_the_header():
    from genesis_forge_amd import _native as nat

    lib = _lib(nat)
    assert lib.gf_push_sizeof() == C.sizeof(nat.GfPushArgs) == 160
    assert lib.gf_abi_version() == nat.GF_ABI_VERSION == 11          # additive: the version stays
    assert nat.GF_PUSH_BLOCK_ENVS == pc.BLOCK and nat.GF_PUSH_SEED_TAG == pc.SEED_TAG
    assert nat.GF_PUSH_SEED_TAG != nat.GF_POLICY_SEED_TAG
    assert "push" not in nat.PHASE_FUNCS and nat.GfPushArgs not in nat.ABI_STRUCTS


@pytest.mark.parametrize("case", sorted(NULL_CASES))
def test_entry_refuses_missing_pointers(case):
    from genesis_forge_amd import _native as nat

    a = _valid_args(nat)
    NULL_CASES[case](a)
    assert _lib(nat).gf_push(C.byref(a), None) == GF_E_NULL


def test_entry_refuses_null_args():
    from genesis_forge_amd import _native as nat

    assert _lib(nat).gf_push(None, None) == GF_E_NULL


@pytest.mark.parametrize("case", sorted(RANGE_CASES))
def test_entry_refuses_out_of_range_fields(case):
    from genesis_forge_amd import _native as nat

    a = _valid_args(nat)
    RANGE_CASES[case](a)
    assert _lib(nat).gf_push(C.byref(a), None) == GF_E_RANGE


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_entry_accepts_an_empty_launch_without_a_hip_call(case):
    """num_envs == 0 is GF_OK before any HIP call (this runs on a machine without a GPU) for every descriptor that is in range."""
    from genesis_forge_amd import _native as nat

    a = _valid_args(nat, n=0)
    ACCEPTED[case](a)
    assert _lib(nat).gf_push(C.byref(a), None) == GF_OK


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: ValueErrors
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(velocity_range={"w": (0.0, 1.0)}), dict(velocity_range={"x": (0.0, 1.0), "Yaw": (0.0, 1.0)}),
    dict(velocity_range={"x": (0.0, NAN)}), dict(velocity_range={"roll": (-INF, 0.0)}), dict(velocity_range={"y": (0.5, 0.25)}),
    dict(velocity_range={"z": 0.5}), dict(velocity_range={"z": (0.0, 0.5, 1.0)}),
    dict(mode="replace"), dict(mode=0),
    dict(interval_s=(5.0, 4.0)), dict(interval_s=(-1.0, 4.0)), dict(interval_s=(1.0, NAN)), dict(interval_s=(1.0, INF)), dict(interval_s=3.0),
    dict(interval_s=(1.0, 1.0 + (1 << 24))),
    dict(scale=NAN), dict(scale=INF),
], ids=repr)
def test_constructor_value_errors(oracle_backend, kw):
    from genesis_forge_amd.managers import PushDisturbance

    with pytest.raises(ValueError):
        PushDisturbance(_Env(4, oracle_backend), **kw)


def test_defaults_and_the_entity_it_needs(oracle_backend):
    import genesis_forge_amd
    from genesis_forge_amd.managers import PushDisturbance

    assert genesis_forge_amd.PushDisturbance is PushDisturbance
    env = _Env(5, oracle_backend, _Entity(torch.zeros(5, 3), torch.zeros(5, 3)))
    env.dt = 0.02
    pd = PushDisturbance(env)
    assert (pd.interval_lo, pd.interval_hi, pd.comp_mask, pd.mode, pd.per_env, pd.scale) == (500, 750, 0x03, 0, True, 1.0)
    assert (pd._lo[:2], pd._hi[:2]) == ([-0.5, -0.5], [0.5, 0.5]) and pd.use_kernel
    assert PushDisturbance(env, interval_s=(0.0, 0.001)).interval_lo == 1            # at least one step
    assert PushDisturbance(env, interval_s=(0.0, 0.001)).interval_hi == 1
    assert PushDisturbance(env, interval_s=(0.05, 0.07)).interval_hi == 4            # rounded
    pd.build()
    assert pd.due.dtype == torch.int32 and int(pd.due.min()) >= 500 and int(pd.due.max()) <= 750 and len(pd.due.unique()) > 1
    assert pd.read_counts() == 0 and not pd.fired.any()
    g = PushDisturbance(env, per_env=False)
    g.build()
    want = 500 + min(int(pc.philox_draws(env._rng_seed, 0, 1, 0, 0x03, 1)[0, 3] * np.float32(251)), 250)
    assert g.due.tolist() == [want] * 5                                               # one host-side draw of the same formula
    for bad in (torch.zeros(4, dtype=torch.bool), torch.zeros(5, dtype=torch.uint8), torch.zeros(10, dtype=torch.bool)[::2]):
        with pytest.raises(ValueError):
            pd.step(bad)                                                              # a mask of another size, type or stride
        with pytest.raises(ValueError):
            pd.step(None, bad)
    with pytest.raises(ValueError):
        pd.step(draws=torch.zeros(5, 6))
    pd.step(torch.zeros(5, dtype=torch.bool))                                         # … and the call after a refusal is checked again
    env.robot = object()
    with pytest.raises(ValueError):
        PushDisturbance(env).build()                                                  # neither masked base nor dof setters


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: _step_torch against the restatement
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", pc.SIZES)
@pytest.mark.parametrize("which", pc.PATTERNS)
def test_torch_sizes_and_patterns(oracle_backend, n, which):
    assert not hasattr(oracle_backend, "push")          # the composition is what runs here
    sizes_and_patterns(run_manager, n, which)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("comp_mask", pc.COMP_MASKS)
def test_torch_modes_and_components(oracle_backend, mode, comp_mask):
    modes_and_components(run_manager, mode, comp_mask)


def test_torch_fires_every_step(oracle_backend):
    every_step(run_manager)


def test_torch_fixed_interval(oracle_backend):
    fixed_interval(run_manager)


def test_torch_interval_spread(oracle_backend):
    interval_spread(run_manager)


@pytest.mark.parametrize("edge", [1 << 31, 1 << 32])
def test_torch_counter_wrap(oracle_backend, edge):
    counter_wrap(run_manager, edge)


def test_torch_counts_over_a_run(oracle_backend):
    counts_over_a_run(run_manager)


def test_torch_env_offset(oracle_backend):
    env_offset_shifts_the_draws(run_manager)


def test_torch_philox_against_draws(oracle_backend):
    philox_against_draws(run_manager)


def test_torch_global_timer(oracle_backend):
    global_timer(run_manager)


def test_step_counter_advances_by_itself(oracle_backend):
    """step() uses calls 1, 2, … (build() is call 0) and never asks the env for a stream id (_Env.next_stream raises)."""
    n = 70
    cfg = pc.base_cfg(interval_lo=1, interval_hi=3, comp_mask=0x3F)
    lin, ang = torch.zeros(n, 3), torch.zeros(n, 3)
    env, pd = _manager(n, oracle_backend, cfg, _Entity(lin, ang))
    pd.build()
    st = {"due": np.zeros(n, np.int32), "lin_vel": np.zeros((n, 3), np.float32), "ang_vel": np.zeros((n, 3), np.float32),
          "fired": np.zeros(n, np.uint8), "counts": np.zeros(1, np.int32), "mask": np.ones(n, bool), "mask2": None}
    st, _ = pc.reference(st, _cfg32(dict(cfg, step=0)), pc.philox_draws(env._rng_seed, 0, n, 0, 0x3F, 0))      # build(): all done at step 0
    _same(pd.due.numpy(), st["due"], "timers after build")
    for t in range(1, 7):
        pd.scale = 0.5 * t                                                             # a plain attribute, read at every step
        st["mask"] = np.arange(n) % 7 == t
        pd.step(torch.from_numpy(st["mask"]))
        st, _ = pc.reference(st, _cfg32(dict(cfg, step=t, scale=0.5 * t)), pc.philox_draws(env._rng_seed, t, n, 0, 0x3F, 0))
        for k, got in (("due", pd.due), ("lin_vel", lin), ("ang_vel", ang), ("fired", pd._fired), ("counts", pd.counts)):
            _same(got.numpy(), st[k], f"step {t}: {k}")
    assert pd.read_counts() == int(st["counts"][0]) > 0


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the setter path
# ---------------------------------------------------------------------------------------------------------------------------
class _SetterEntity:
    """An entity that has only the simulator's dof getters and setters."""

    def __init__(self, vel):
        self.vel, self.gets, self.sets = vel, [], []

    def get_dofs_velocity(self, dofs_idx_local=None, envs_idx=None):
        self.gets.append((dofs_idx_local, envs_idx))
        return self.vel[:, dofs_idx_local].clone()

    def set_dofs_velocity(self, velocity, dofs_idx_local=None, envs_idx=None):
        self.sets.append((velocity.clone(), dofs_idx_local, envs_idx))
        self.vel[:, dofs_idx_local] = velocity


def test_setter_path_hands_back_the_whole_block(oracle_backend):
    n = 130
    cfg = pc.base_cfg(interval_lo=2, interval_hi=2, comp_mask=0x23, step=2)
    rng = np.random.default_rng(3)
    vel = torch.from_numpy(rng.normal(size=(n, 18)).astype(np.float32))
    ent = _SetterEntity(vel.clone())
    env, pd = _manager(n, oracle_backend, cfg, ent)
    pd.build()
    assert not ent.sets and (pd.due == 2).all()
    mask = torch.from_numpy(rng.random(n) < 0.3)
    pd.step(None, None)                                                               # step 1: nothing is due
    pd.step(mask, None)                                                               # step 2: all but the done envs
    assert [g[0] for g in ent.gets] == [list(range(6))] * 2 and all(g[1] is None for g in ent.gets)
    assert len(ent.sets) == 2
    for block, dofs, ids in ent.sets:
        assert tuple(block.shape) == (n, 6) and dofs == list(range(6)) and ids is None        # every env, no index list
    assert torch.equal(ent.sets[0][0], vel[:, :6])                                    # unfired rows go back unchanged
    st = {"due": np.full(n, 2, np.int32), "lin_vel": vel[:, 0:3].numpy().copy(), "ang_vel": vel[:, 3:6].numpy().copy(),
          "fired": np.zeros(n, np.uint8), "counts": np.zeros(1, np.int32), "mask": mask.numpy(), "mask2": None}
    want, fire = pc.reference(st, _cfg32(cfg), pc.philox_draws(env._rng_seed, 2, n, 0, 0x23, 0))
    _same(ent.sets[1][0].numpy(), np.concatenate([want["lin_vel"], want["ang_vel"]], axis=1), "the block handed to the setter")
    assert fire.any() and not fire.all() and torch.equal(pd.fired, torch.from_numpy(fire))
    assert torch.equal(ent.vel[:, 6:], vel[:, 6:])                                    # the joints are not touched


# ---------------------------------------------------------------------------------------------------------------------------
# the env
# ---------------------------------------------------------------------------------------------------------------------------
def _env_run(dev, trace, push, n=16, steps=30, spy=False):
    from genesis_forge_amd import tasks

    kw = {} if push is None else {"push": dict(push)}
    env = tasks.Go2RoughTerrainEnv(num_envs=n, max_episode_length_s=0.5, cmd_resample_s=0.3, scene_kwargs=dict(ang_noise=0.4, seed=9), **kw)
    env.trace_enabled = trace
    env.build()
    env.seed(5)
    env.reset()
    log = []
    if spy:
        p, inner = env.push, env.push.step

        def spied(te, tr):
            cpu = lambda t: t.cpu().numpy().copy()
            pre = {"due": cpu(p.due), "lin_vel": cpu(env.robot.lin_vel), "ang_vel": cpu(env.robot.ang_vel), "fired": cpu(p._fired),
                   "counts": cpu(p.counts), "mask": cpu(te), "mask2": cpu(tr)}
            inner(te, tr)
            log.append((p._step, pre, {"due": cpu(p.due), "lin_vel": cpu(env.robot.lin_vel), "ang_vel": cpu(env.robot.ang_vel),
                                       "fired": cpu(p._fired), "counts": cpu(p.counts)}))

        p.step = spied
    g = torch.Generator().manual_seed(0)
    out = []
    for _ in range(steps):
        obs, rew, te, tr, _ex = env.step(torch.randn(n, 12, generator=g).to(dev))
        out.append(dict(obs=obs.cpu().clone(), rew=rew.cpu().clone(), te=te.cpu().clone(), tr=tr.cpu().clone(), rng=env._rng_c.value,
                        lin=env.robot.lin_vel.cpu().clone(), ang=env.robot.ang_vel.cpu().clone(),
                        due=None if env.push is None else env.push.due.cpu().clone(),
                        fired=None if env.push is None else env.push.fired.cpu().clone()))
    return env, out, log


def _equal_runs(a, b, keys):
    for t, (x, y) in enumerate(zip(a, b)):
        for k in keys:
            assert (x[k] == y[k]) if k == "rng" else torch.equal(x[k], y[k]), f"step {t}: {k}"


PUSH = dict(interval_s=(0.04, 0.08), velocity_range={"x": (-0.5, 0.5), "y": (-0.5, 0.5), "yaw": (-0.3, 0.3)})


def _no_host_read(monkeypatch, env=None):
    """done_ids() raises, as in the curriculum's env test; with ``env``, every host read of a tensor raises inside push.step()."""
    from genesis_forge_amd import genesis_env

    def no_done_ids(self, *a, **k):
        raise AssertionError("done_ids() was called: the pushes must not read the done list back")

    monkeypatch.setattr(genesis_env.GenesisEnv, "done_ids", no_done_ids)
    if env is None:
        return
    inner = env.push.step

    def guarded(te, tr):
        def refuse(name):
            def f(*a, **k):
                raise AssertionError(f"push.step() read a tensor back: {name}")
            return f

        with monkeypatch.context() as m:
            for name in ("item", "tolist", "cpu", "numpy", "nonzero", "__bool__", "__int__", "__float__", "__index__"):
                m.setattr(torch.Tensor, name, refuse(name))
            inner(te, tr)

    env.push.step = guarded


def test_env_with_push_stays_recorded_and_leaves_the_envs_stream_alone(oracle_backend, monkeypatch):
    plain_env, plain, _ = _env_run("cpu", trace=False, push=PUSH)
    assert plain_env._trace is None
    bare_env, bare, _ = _env_run("cpu", trace=True, push=None)
    assert bare_env.push is None and bare_env._trace is not None
    _no_host_read(monkeypatch)
    env, traced, _ = _env_run("cpu", trace=True, push=PUSH)
    assert env._trace is not None                                                     # the step is a recorded one after warm-up …
    _equal_runs(plain, traced, ("obs", "rew", "te", "tr", "rng", "lin", "ang", "due", "fired"))       # … and equals the ordinary one
    _equal_runs(bare, traced, ("rng",))                                               # env._rng_c advances exactly as without push
    assert env.push.read_counts() == sum(int(o["fired"].sum()) for o in traced) > 0
    assert any(o["fired"].any() and not o["fired"].all() for o in traced)


def test_env_with_a_zero_push_is_the_env_without(oracle_backend):
    """mode='add' with scale 0 adds 0 to the enabled components: observations, rewards and masks are those of an env built without."""
    _e, bare, _ = _env_run("cpu", trace=True, push=None)
    env, zero, _ = _env_run("cpu", trace=True, push=dict(PUSH, mode="add", scale=0.0))
    _equal_runs(bare, zero, ("obs", "rew", "te", "tr", "rng", "lin", "ang"))
    assert env.push.read_counts() > 0


def test_ahead_of_time_signature_is_the_one_without_push():
    """The no-GPU dry run that compiles a config's program ahead of time builds and steps the env with push= too — the dry-run
    backend launches nothing, the pushes included — and, the step inside being the same, finds the same program."""
    from genesis_forge_amd import _programs, tasks

    make = lambda push: (lambda n: tasks.Go2RoughTerrainEnv(num_envs=n, scene_kwargs=dict(ang_noise=0.05, seed=9), push=push))
    with_push, without = _programs.signature_of(make({})), _programs.signature_of(make(None))
    assert with_push is not None and with_push == without


def test_env_pushes_are_the_restatements(oracle_backend):
    """Default ranges, a push every two steps: lin_vel[:, :2] after the step is the restatement's where `fired`, the scene's own elsewhere."""
    n = 16
    env, out, log = _env_run("cpu", trace=True, push=dict(interval_s=(0.04, 0.04)), n=n, spy=True)
    p = env.push
    assert (p.interval_lo, p.interval_hi, p.comp_mask, p.mode) == (2, 2, 0x03, 0) and len(log) == len(out)
    cfg = pc.base_cfg(interval_lo=2, interval_hi=2, comp_mask=0x03, lo=(-0.5, -0.5, 0, 0, 0, 0), hi=(0.5, 0.5, 0, 0, 0, 0))
    mixed = 0
    for t, (step, pre, post) in enumerate(log):
        assert step == t + 1
        want, fire = pc.reference(pre, _cfg32(dict(cfg, step=step)), pc.philox_draws(env._rng_seed, step, n, env.env_offset, 0x03, 0))
        for k in OUT:
            _same(post[k], want[k], f"step {step}: {k}")
        _same(out[t]["lin"].numpy()[fire, :2], want["lin_vel"][fire, :2], "pushed rows")
        _same(out[t]["lin"].numpy()[~fire], pre["lin_vel"][~fire], "the scene's own rows")
        _same(out[t]["lin"].numpy()[:, 2], pre["lin_vel"][:, 2], "z")
        assert (np.abs(want["lin_vel"][fire, :2]) <= 0.5).all()
        mixed += bool(fire.any() and not fire.all())
    assert mixed > 0 and p.read_counts() > n


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the kernel raw through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", pc.SIZES)
@pytest.mark.parametrize("which", pc.PATTERNS)
def test_kernel_sizes_and_patterns(hip_backend, n, which):
    sizes_and_patterns(run_raw, n, which)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("comp_mask", pc.COMP_MASKS)
def test_kernel_modes_and_components(hip_backend, mode, comp_mask):
    modes_and_components(run_raw, mode, comp_mask)


@pytest.mark.gpu
def test_kernel_fires_every_step(hip_backend):
    every_step(run_raw)


@pytest.mark.gpu
def test_kernel_fixed_interval(hip_backend):
    fixed_interval(run_raw)


@pytest.mark.gpu
def test_kernel_interval_spread(hip_backend):
    interval_spread(run_raw)


@pytest.mark.gpu
@pytest.mark.parametrize("edge", [1 << 31, 1 << 32])
def test_kernel_counter_wrap(hip_backend, edge):
    counter_wrap(run_raw, edge)


@pytest.mark.gpu
def test_kernel_counts_over_a_run(hip_backend):
    counts_over_a_run(run_raw)


@pytest.mark.gpu
def test_kernel_env_offset(hip_backend):
    env_offset_shifts_the_draws(run_raw)


@pytest.mark.gpu
def test_kernel_philox_against_draws(hip_backend):
    philox_against_draws(run_raw)


@pytest.mark.gpu
def test_kernel_global_timer(hip_backend):
    global_timer(run_raw)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [pc.WAVE + 1, pc.BLOCK + 1, 1000])
def test_kernel_early_waves_write_fired_and_rows_off_alignment(hip_backend, n):
    """One lane of the last wave works: every other wave leaves after the ballot and still clears its `fired` bytes (planted with
    7).  lin_vel and ang_vel one float off 16-byte alignment; without `fired`; without ang_vel."""
    cfg = pc.base_cfg(comp_mask=0x3F, mode=1)
    st = pc.apply_pattern(pc.random_state(n, n), "one_lane", cfg["step"])
    after, fire = _check(run_raw, st, cfg, u=pc.dense_draws(n, 1), what="one lane", off=1)
    assert (st["fired"] == 7).all() and after["fired"].sum() == 1 and set(after["fired"].tolist()) == {0, 1}
    st = pc.apply_pattern(pc.random_state(n, n), "done_and_due", cfg["step"], seed=2)
    for off in (1, 2, 3):
        _check(run_raw, st, cfg, key=(5, 0), what=f"off {off}", off=off)
    _check(run_raw, st, cfg, key=(5, 0), what="no fired", no_fired=True)
    st = pc.apply_pattern(pc.random_state(n, n, with_ang=False), "done_and_due", cfg["step"], seed=2)
    _check(run_raw, st, dict(cfg, comp_mask=0x05), key=(5, 0), what="no ang_vel", off=1)


@pytest.mark.gpu
@pytest.mark.parametrize("g", [0, 1])
def test_kernel_equals_step_torch_on_the_device(hip_backend, g):
    n = 1000
    cfg = pc.base_cfg(comp_mask=0x3F, mode=1, global_timer=g, interval_lo=2, interval_hi=7, scale=1.5)
    st = pc.apply_pattern(pc.random_state(n, 4), "done_and_due", cfg["step"], seed=4)
    if g:
        st["due"][:] = cfg["step"]
    a = run_manager(st, cfg, key=(0x77, 9), dev="cuda", use_kernel=True)
    b = run_manager(st, cfg, key=(0x77, 9), dev="cuda", use_kernel=False)
    want, fire = pc.reference(st, _cfg32(cfg), pc.philox_draws(0x77, cfg["step"], n, 9, 0x3F, g))
    assert fire.any()
    for k in OUT:
        _same(a[k], b[k], f"kernel against _step_torch: {k}")
        _same(a[k], want[k], f"kernel against the restatement: {k}")


def _untouched_launch(nat, backend, edit, n=70):
    cfg = pc.base_cfg(comp_mask=0x3F)
    st = pc.apply_pattern(pc.random_state(n, 1), "all", cfg["step"])
    keep = []
    g, _n = _raw_buffers(st, "cuda", init=False)
    a = _raw_args(nat, st, cfg, g, n, keep, key=(1, 0))
    edit(a)
    rc = raw_call(backend, "push", a)
    sync("cuda")
    return rc, all(v.untouched() for v in g.values())


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(NULL_CASES) + sorted(RANGE_CASES))
def test_kernel_entry_refusals_leave_every_buffer_untouched(hip_backend, case):
    from genesis_forge_amd import _native as nat

    edit, code = (NULL_CASES[case], GF_E_NULL) if case in NULL_CASES else (RANGE_CASES[case], GF_E_RANGE)
    rc, untouched = _untouched_launch(nat, hip_backend, edit)
    assert rc == code and untouched


@pytest.mark.gpu
def test_kernel_empty_launch_leaves_every_buffer_untouched(hip_backend):
    from genesis_forge_amd import _native as nat

    rc, untouched = _untouched_launch(nat, hip_backend, lambda a: setattr(a, "num_envs", 0))
    assert rc == GF_OK and untouched


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the env on the HIP backend
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_env_on_the_hip_backend_recorded_equals_ordinary_without_a_host_read(hip_backend, monkeypatch):
    from genesis_forge_amd import tasks

    _e, plain, _ = _env_run("cuda", trace=False, push=PUSH)
    torch.cuda.synchronize()
    _no_host_read(monkeypatch)
    real_build = tasks.Go2RoughTerrainEnv.build

    def build(self):
        real_build(self)
        _no_host_read(monkeypatch, self)         # from here on push.step() runs with every tensor read-back refused

    monkeypatch.setattr(tasks.Go2RoughTerrainEnv, "build", build)
    env, traced, _ = _env_run("cuda", trace=True, push=PUSH)
    torch.cuda.synchronize()
    assert env._trace is not None and hasattr(env.backend, "push") and env.push.use_kernel
    _equal_runs(plain, traced, ("obs", "rew", "te", "tr", "rng", "lin", "ang", "due", "fired"))
    assert env.push.read_counts() == sum(int(o["fired"].sum()) for o in traced) > 0
