"""Actuator latency: gf_action_delay (csrc/gf_action_delay.hip, contract in include/gf_step.h), managers.ActuatorDelay,
managers.DelayedPositionActionManager and Go2RoughTerrainEnv(action_delay=…).

CPU: the binding, every refusal of the entry (before any HIP call: they run without a GPU), the ValueErrors, ActuatorDelay's torch
composition (_step_torch, the oracle backend has no action_delay entry) against the numpy restatement (action_delay_cases.reference)
over sequences of T = 2L + 3 calls — shapes, ring sizes, every source of freshness alone and combined, Philox and parity draws, the call
counter across 2^32, offsets —, the manager and the task hook.  GPU: the kernel raw through the C ABI over the same sequences, every
output a slice of a Guarded buffer, pointers off 16-byte alignment, the kernel against _step_torch on the device, the env recorded
against ordinary.

Every comparison is exact, on bits (float32 viewed as int32: NaN payloads count)."""
import ctypes as C

import numpy as np
import pytest
import torch

import action_delay_cases as ac
from guarded import Guarded, raw_call, sync

GF_OK, GF_E_NULL, GF_E_RANGE = 0, -1, -2   # include/gf_step.h
M32 = 0xFFFFFFFF
STATE = ("out", "ring", "lag")


# ---------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------
def _lib(nat):
    lib = C.CDLL(nat.lib_path())
    lib.gf_action_delay.restype = C.c_int
    lib.gf_action_delay.argtypes = [C.c_void_p, C.c_void_p]
    return lib


def _valid_args(nat, n=4):
    """A descriptor gf_action_delay accepts.  Its pointers are never followed: every case it is used in is refused, or has no envs."""
    a = nat.GfActionDelayArgs()
    a.num_envs, a.num_dofs, a.slots, a.head, a.lag_lo, a.lag_hi, a.prime_all, a.step = n, 12, 8, 3, 1, 5, 0, 7
    for f in ("in_", "out", "ring", "lag", "episode_length", "mask", "mask2", "draws"):
        setattr(a, f, 0x1000)
    return a


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    bad = _bits(got) != _bits(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0].tolist()}"


class _Env:
    """The smallest env an ActuatorDelay needs."""

    def __init__(self, n, backend, seed=0x1234, env_offset=0, dt=0.02):
        self.num_envs, self.backend, self.dt = n, backend, dt
        self._rng_seed, self.env_offset = seed, env_offset

    def next_stream(self):
        raise AssertionError("ActuatorDelay must not take a stream id from the env")


def run_manager(c, dev="cpu", use_kernel=True):
    """The case's calls through ActuatorDelay.step on copies of its start state; returns the state after every call.  (With
    ``dev='cpu'`` and the oracle backend this is _step_torch.)"""
    from genesis_forge_amd import _native as nat
    from genesis_forge_amd.managers import ActuatorDelay

    st, calls = ac.script(c)
    T = lambda arr: None if arr is None else torch.from_numpy(np.ascontiguousarray(arr)).clone().to(dev)
    env = _Env(c["n"], nat.get_backend(), c["key"], c["env_offset"])
    pd = ActuatorDelay(env, c["d"], lag_steps=c["lag"], max_lag=c["slots"] - 1)
    pd.build()
    pd.use_kernel = use_kernel
    assert tuple(pd.ring.shape) == (c["slots"], c["n"], c["d"]) and pd.lag.dtype == torch.int32
    pd.ring.copy_(T(st["ring"]))
    pd.lag.copy_(T(st["lag"]))
    pd.out.copy_(T(st["out"]))
    after = []
    for call in calls:
        if call["episode_length"] is None:
            env.__dict__.pop("episode_length", None)
        else:
            env.episode_length = T(call["episode_length"])
        pd._prime = bool(call["prime_all"])
        pd._head, pd._step = (call["head"] - 1) % c["slots"], (call["step"] - 1) & M32
        out = pd.step(T(call["in"]), T(call["mask"]), T(call["mask2"]), draws=None if c["philox"] else T(call["u"]))
        assert out is pd.out and pd._head == call["head"] and pd._step == call["step"] and not pd._prime
        sync(dev)
        after.append({"out": pd.out.cpu().numpy().copy(), "ring": pd.ring.cpu().numpy().copy(), "lag": pd.lag.cpu().numpy().copy()})
    return after


def _raw_args(nat, c, call, g, gin, keep, dev="cuda"):
    T = lambda arr: None if arr is None else (keep.append(torch.from_numpy(np.ascontiguousarray(arr)).to(dev)) or keep[-1].data_ptr())
    a = nat.GfActionDelayArgs()
    a.num_envs, a.num_dofs, a.slots = c["n"], c["d"], c["slots"]
    a.in_, a.out, a.ring, a.lag = gin.ptr, g["out"].ptr, g["ring"].ptr, g["lag"].ptr
    a.episode_length, a.mask, a.mask2 = T(call["episode_length"]), T(call["mask"]), T(call["mask2"])
    a.draws = None if c["philox"] else T(call["u"])
    a.seed, a.env_offset, a.step, a.head = c["key"], c["env_offset"], call["step"], call["head"]
    a.lag_lo, a.lag_hi, a.prime_all = c["lag"][0], c["lag"][1], call["prime_all"]
    return a


def _raw_buffers(c, st, dev, off=(0, 0, 0), init=True):
    T = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)) if init else None
    n, d, L = c["n"], c["d"], c["slots"]
    return {"out": Guarded(n * d, torch.float32, dev, off=off[1], init=T(st["out"])), "ring": Guarded(L * n * d, torch.float32, dev, off=off[2], init=T(st["ring"])),
            "lag": Guarded(n, torch.int32, dev, init=T(st["lag"]))}


def run_raw(c, off=(0, 0, 0)):
    """The case's calls as gf_action_delay launches through the binding, state in Guarded buffers (``off``: floats past a 16-byte
    boundary of in, out, ring); returns the state after every call."""
    from genesis_forge_amd import _native as nat

    dev = "cuda"
    st, calls = ac.script(c)
    n, d, L = c["n"], c["d"], c["slots"]
    g = _raw_buffers(c, st, dev, off)
    after = []
    for t, call in enumerate(calls):
        keep = []
        gin = Guarded(n * d, torch.float32, dev, off=off[0], init=torch.from_numpy(call["in"]))
        nat.get_backend().action_delay(_raw_args(nat, c, call, g, gin, keep))
        sync(dev)
        assert gin.guards_ok() and all(v.guards_ok() for v in g.values()), f"call {t}: a write outside a buffer"
        _same(gin.cpu().numpy().reshape(n, d), call["in"], f"call {t}: the input")
        after.append({"out": g["out"].cpu().numpy().reshape(n, d).copy(), "ring": g["ring"].cpu().numpy().reshape(L, n, d).copy(),
                      "lag": g["lag"].cpu().numpy().copy()})
    return after


def _check(run, c, **kw):
    """``run`` against the restatement, every output of every call bit for bit; then, on what ``run`` itself left: an ordinary env's
    lag and its slots other than ``head`` are those of the call before."""
    trail = ac.walk(c)
    ac.conditions(c, trail)
    st0, calls = ac.script(c)
    got = run(c, **kw)
    assert len(got) == len(trail) == 2 * c["slots"] + 3
    prev = st0
    for t, (have, (want, fresh, _read), call) in enumerate(zip(got, trail, calls)):
        for k in STATE:
            _same(have[k], want[k], f"{ac.case_id(c)} call {t}: {k}")
        old = ~fresh
        _same(have["lag"][old], prev["lag"][old], f"call {t}: the lag of an ordinary env")
        others = [s for s in range(c["slots"]) if s != call["head"]]
        _same(have["ring"][others][:, old], prev["ring"][others][:, old], f"call {t}: the other slots of an ordinary env")
        _same(have["ring"][:, fresh], np.broadcast_to(call["in"][fresh], (c["slots"],) + call["in"][fresh].shape), f"call {t}: a fresh env's ring")
        prev = have
    return got


CASES = ac.all_cases()
IDS = [ac.case_id(c) for c in CASES]


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the cases themselves, binding and refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_case_matrix_covers_what_it_claims():
    assert len(set(IDS)) == len(IDS)
    assert {c["n"] for c in CASES} >= set(ac.SIZES) and {c["d"] for c in CASES} >= set(ac.DOFS) and {c["slots"] for c in CASES} >= set(ac.SLOTS)
    assert {c["source"] for c in CASES} == set(ac.SOURCES)
    assert any(c["step0"] < (1 << 32) <= c["step0"] + c["calls"] for c in CASES)                 # the counter crosses 2^32
    assert any(not c["philox"] for c in CASES) and any(c["env_offset"] for c in CASES)
    assert any(c["n"] * c["d"] % 4 for c in CASES) and any(c["d"] == 3 and c["n"] * 3 % 4 == 0 for c in CASES)
    for c in CASES:
        ac.conditions(c)
        _st, calls = ac.script(c)
        assert [k["head"] for k in calls].count(0) >= 2                                          # head wraps
        x = np.concatenate([k["in"].reshape(-1) for k in calls])
        assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any() and (x.view(np.int32) == np.int32(-2 ** 31)).any()
    eps = np.concatenate([k["episode_length"] for c in CASES if c["source"] == "episode_length" for k in ac.script(c)[1]])
    assert {0, 1, 2} <= set(eps.tolist())


NULL_CASES = {f: (lambda a, f=f: setattr(a, f, None)) for f in ("in_", "out", "ring", "lag")}

RANGE_CASES = {
    "num_envs<0": lambda a: setattr(a, "num_envs", -1),
    "too_many_workgroups": lambda a: setattr(a, "num_envs", 1 << 40),
    "num_envs_times_dofs_overflows": lambda a: (setattr(a, "num_envs", 1 << 62), setattr(a, "num_dofs", 1 << 20)),
    "num_dofs=0": lambda a: setattr(a, "num_dofs", 0),
    "num_dofs<0": lambda a: setattr(a, "num_dofs", -12),
    "slots=0": lambda a: (setattr(a, "slots", 0), setattr(a, "head", 0), setattr(a, "lag_lo", 0), setattr(a, "lag_hi", 0)),
    "slots<0": lambda a: setattr(a, "slots", -1),
    "slots=65": lambda a: setattr(a, "slots", 65),
    "head<0": lambda a: setattr(a, "head", -1),
    "head=slots": lambda a: setattr(a, "head", 8),
    "lag_lo<0": lambda a: setattr(a, "lag_lo", -1),
    "lag_hi<lag_lo": lambda a: (setattr(a, "lag_lo", 4), setattr(a, "lag_hi", 3)),
    "lag_hi=slots": lambda a: setattr(a, "lag_hi", 8),
    "lag_hi=int_max": lambda a: setattr(a, "lag_hi", 0x7FFFFFFF),
    "prime_all=2": lambda a: setattr(a, "prime_all", 2),
    "prime_all=-1": lambda a: setattr(a, "prime_all", -1),
}

ACCEPTED = {
    "as_it_is": lambda a: None,
    "bare": lambda a: [setattr(a, f, None) for f in ("episode_length", "mask", "mask2", "draws")],
    "one_slot": lambda a: (setattr(a, "slots", 1), setattr(a, "head", 0), setattr(a, "lag_lo", 0), setattr(a, "lag_hi", 0)),
    "64_slots": lambda a: (setattr(a, "slots", 64), setattr(a, "head", 63), setattr(a, "lag_lo", 0), setattr(a, "lag_hi", 63)),
    "lo==hi": lambda a: (setattr(a, "lag_lo", 7), setattr(a, "lag_hi", 7)),
    "prime_all": lambda a: setattr(a, "prime_all", 1),
    "one_dof": lambda a: setattr(a, "num_dofs", 1),
}


def test_binding_matches_the_header():
    from genesis_forge_amd import _native as nat

    lib = _lib(nat)
    assert lib.gf_action_delay_sizeof() == C.sizeof(nat.GfActionDelayArgs) == 112
    assert lib.gf_abi_version() == nat.GF_ABI_VERSION == 11          # additive: the version stays
    assert nat.GF_ACTION_DELAY_MAX_SLOTS == ac.MAX_SLOTS and nat.GF_ACTION_DELAY_SEED_TAG == ac.SEED_TAG
    assert nat.GF_ACTION_DELAY_SEED_TAG not in (nat.GF_PUSH_SEED_TAG, nat.GF_POLICY_SEED_TAG)      # a key of its own
    assert "action_delay" not in nat.PHASE_FUNCS and nat.GfActionDelayArgs not in nat.ABI_STRUCTS
    assert hasattr(nat.HipBackend, "action_delay")


@pytest.mark.parametrize("case", sorted(NULL_CASES))
def test_entry_refuses_missing_pointers(case):
    from genesis_forge_amd import _native as nat

    a = _valid_args(nat)
    NULL_CASES[case](a)
    assert _lib(nat).gf_action_delay(C.byref(a), None) == GF_E_NULL


def test_entry_refuses_null_args():
    from genesis_forge_amd import _native as nat

    assert _lib(nat).gf_action_delay(None, None) == GF_E_NULL


@pytest.mark.parametrize("case", sorted(RANGE_CASES))
def test_entry_refuses_out_of_range_fields(case):
    from genesis_forge_amd import _native as nat

    a = _valid_args(nat)
    RANGE_CASES[case](a)
    assert _lib(nat).gf_action_delay(C.byref(a), None) == GF_E_RANGE


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_entry_accepts_an_empty_launch_without_a_hip_call(case):
    """num_envs == 0 is GF_OK before any HIP call (this runs on a machine without a GPU) for every descriptor that is in range."""
    from genesis_forge_amd import _native as nat

    a = _valid_args(nat, n=0)
    ACCEPTED[case](a)
    assert _lib(nat).gf_action_delay(C.byref(a), None) == GF_OK


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: ValueErrors
# ---------------------------------------------------------------------------------------------------------------------------
BAD_LAGS = [dict(lag_steps=(0.5, 2)), dict(lag_steps=(0, 2.0)), dict(lag_steps=("0", 2)), dict(lag_steps=(True, 2)), dict(lag_steps=(-1, 2)),
            dict(lag_steps=(0, -2)), dict(lag_steps=(3, 2)), dict(lag_steps=2), dict(lag_steps=(0, 1, 2)), dict(lag_steps=(0, 5), max_lag=4),
            dict(lag_steps=(0, 2), max_lag=64), dict(lag_steps=(0, 64)), dict(lag_steps=(0, 2), max_lag=2.5), dict(lag_steps=(0, 2), max_lag=-1)]


@pytest.mark.parametrize("kw", BAD_LAGS, ids=repr)
def test_constructor_value_errors(oracle_backend, kw):
    from genesis_forge_amd.managers import ActuatorDelay, DelayedPositionActionManager

    with pytest.raises(ValueError) as e:
        ActuatorDelay(_Env(4, oracle_backend), 12, **kw)
    shown = kw["max_lag"] if "max_lag" in kw and kw["lag_steps"] == (0, 2) else (64 if kw["lag_steps"] == (0, 64) else kw["lag_steps"])
    assert repr(shown) in str(e.value)                                                # the value is in the message
    with pytest.raises(ValueError):
        DelayedPositionActionManager(_ManagedStub(), **kw)                            # … and the manager refuses at construction


class _ManagedStub:
    """What BaseManager's constructor touches of an env."""
    num_envs = 4

    def __init__(self):
        self.managers = {}

    def add_manager(self, *a, **k):
        pass


@pytest.mark.parametrize("num_dofs", [0, -3, 2.0, None, True])
def test_num_dofs_value_errors(oracle_backend, num_dofs):
    from genesis_forge_amd.managers import ActuatorDelay

    with pytest.raises(ValueError, match=repr(num_dofs)):
        ActuatorDelay(_Env(4, oracle_backend), num_dofs)


def test_defaults_queries_and_tensor_checks(oracle_backend):
    import genesis_forge_amd
    from genesis_forge_amd.managers import ActuatorDelay, DelayedPositionActionManager

    assert genesis_forge_amd.ActuatorDelay is ActuatorDelay and genesis_forge_amd.DelayedPositionActionManager is DelayedPositionActionManager
    assert not hasattr(oracle_backend, "action_delay")                                # the composition is what runs here
    env = _Env(5, oracle_backend)
    pd = ActuatorDelay(env, 3)
    assert (pd.lag_lo, pd.lag_hi, pd.max_lag, pd.slots, pd.use_kernel) == (0, 2, 2, 3, True)
    assert ActuatorDelay(env, 3, lag_steps=(1, 2), max_lag=63).slots == 64
    assert ActuatorDelay(env, 3, lag_steps=(np.int64(1), np.int32(2))).lag_hi == 2   # whole numbers of any integer type
    assert pd.lag.dtype == torch.int32 and tuple(pd.lag.shape) == (5,) and tuple(pd.ring.shape) == (3, 5, 3)
    ring = pd.ring
    pd.build()
    assert pd.ring is ring                                                            # build() runs once
    x = torch.arange(15, dtype=torch.float32).reshape(5, 3)
    for bad in (torch.zeros(4, 3), torch.zeros(5, 4), torch.zeros(5, 3, dtype=torch.float64), torch.zeros(5, 6)[:, ::2], None, [[0.0] * 3] * 5):
        with pytest.raises(ValueError):
            pd.step(bad)
    for bad in (torch.zeros(4, dtype=torch.bool), torch.zeros(5, dtype=torch.uint8), torch.zeros(10, dtype=torch.bool)[::2]):
        with pytest.raises(ValueError):
            pd.step(x, bad)
        with pytest.raises(ValueError):
            pd.step(x, None, bad)
    with pytest.raises(ValueError):
        pd.step(x, draws=torch.zeros(5, 1))
    env.episode_length = torch.zeros(5, dtype=torch.int64)
    with pytest.raises(ValueError, match="episode_length"):
        pd.step(x)
    del env.episode_length
    assert pd._step == 0 and pd._prime                                                # a refused call counts for nothing
    out = pd.step(x)                                                                  # … and the call after a refusal is checked again
    assert out is pd.out and torch.equal(out, x) and pd._step == 1 and pd._head == 0
    assert torch.equal(pd.lag_seconds(), pd.lag.to(torch.float32) * 0.02) and pd.lag_seconds().dtype == torch.float32


def test_set_lag_range_value_errors(oracle_backend):
    from genesis_forge_amd.managers import ActuatorDelay

    pd = ActuatorDelay(_Env(4, oracle_backend), 2, lag_steps=(0, 1), max_lag=5)
    for lo, hi in ((0, 6), (-1, 2), (3, 2), (0.5, 2), (0, 2.0), (0, 64)):
        with pytest.raises(ValueError, match=str(hi)):
            pd.set_lag_range(lo, hi)
        assert (pd.lag_lo, pd.lag_hi) == (0, 1)
    pd.set_lag_range(2, 5)
    assert (pd.lag_lo, pd.lag_hi) == (2, 5)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: _step_torch against the restatement, and the host object's own bookkeeping
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_torch_sequences(oracle_backend, c):
    _check(run_manager, c)


def test_counters_advance_by_themselves_and_reset_primes_all(oracle_backend):
    """step() uses calls 1, 2, … and heads 0, 1, … modulo L, never asks the env for a stream id (_Env.next_stream raises); the first
    call primes every env whatever its episode_length says, and so does the call after reset()."""
    n, d, L = 70, 3, 4
    env = _Env(n, oracle_backend, seed=0xBEEF, env_offset=5)
    env.episode_length = torch.full((n,), 9, dtype=torch.int32)
    from genesis_forge_amd.managers import ActuatorDelay

    pd = ActuatorDelay(env, d, lag_steps=(0, 3))
    st = {"ring": np.zeros((L, n, d), np.float32), "lag": np.zeros(n, np.int32), "out": np.zeros((n, d), np.float32)}
    rng = np.random.default_rng(0)
    for t in range(1, 2 * L + 4):
        if t == L + 2:
            pd.reset()
        x = rng.normal(size=(n, d)).astype(np.float32)
        out = pd.step(torch.from_numpy(x))
        call = {"in": x, "episode_length": env.episode_length.numpy(), "mask": None, "mask2": None, "prime_all": int(t in (1, L + 2)),
                "head": (t - 1) % L, "u": ac.philox_draws(0xBEEF, t, n, 5)}
        st, fresh, _ = ac.reference(st, call, {"lag_lo": 0, "lag_hi": 3})
        assert fresh.all() == (t in (1, L + 2)) and fresh.any() == (t in (1, L + 2))
        for k, got in (("out", out), ("ring", pd.ring), ("lag", pd.lag)):
            _same(got.numpy(), st[k], f"call {t}: {k}")
        if t in (1, L + 2):
            _same(out.numpy(), x, "a primed env gets its own command")
            assert set(pd.lag.tolist()) == {0, 1, 2, 3}
    assert (pd._step, pd._head) == (2 * L + 3, (2 * L + 2) % L)


def test_set_lag_range_applies_at_the_next_redraw_only(oracle_backend):
    n, d = 64, 2
    env = _Env(n, oracle_backend)
    from genesis_forge_amd.managers import ActuatorDelay

    pd = ActuatorDelay(env, d, lag_steps=(1, 1), max_lag=4)
    env.episode_length = torch.full((n,), 5, dtype=torch.int32)
    xs = [torch.full((n, d), float(t)) for t in range(12)]
    pd.step(xs[0])
    assert (pd.lag == 1).all()
    pd.set_lag_range(3, 4)
    for t in (1, 2, 3):
        out = pd.step(xs[t])
        assert (pd.lag == 1).all() and torch.equal(out, xs[max(t - 1, 0)])            # nobody is fresh: the old lag holds
    env.episode_length[::2] = 1                                                       # every other env starts an episode
    out = pd.step(xs[4])
    assert (pd.lag[1::2] == 1).all() and set(pd.lag[::2].tolist()) == {3, 4}
    assert torch.equal(out[::2], xs[4][::2]) and torch.equal(out[1::2], xs[3][1::2])
    env.episode_length[:] = 6
    for t in range(5, 10):
        out = pd.step(xs[t])
        age = t - 4                                                                   # steps since the fresh envs' first
        want = torch.stack([xs[t - min(int(l), age)][i] if i % 2 == 0 else xs[t - 1][i] for i, l in enumerate(pd.lag.tolist())])
        assert torch.equal(out, want), t


# ---------------------------------------------------------------------------------------------------------------------------
# the manager and the task hook
# ---------------------------------------------------------------------------------------------------------------------------
def _env_run(dev, trace, delay, n=64, steps=40, before_first_step=None, **extra):
    from genesis_forge_amd import tasks

    kw = {} if delay is None else {"action_delay": dict(delay)}
    env = tasks.Go2RoughTerrainEnv(num_envs=n, max_episode_length_s=0.3, cmd_resample_s=0.2, scene_kwargs=dict(ang_noise=0.4, seed=9), **kw, **extra)
    env.trace_enabled = trace
    env.build()
    env.seed(5)
    env.reset()
    if before_first_step is not None:
        before_first_step(env)
    g = torch.Generator().manual_seed(0)
    am, out = env.action_manager, []
    c = lambda t: t.cpu().clone()
    for _ in range(steps):
        raw = torch.randn(n, 12, generator=g)
        age = c(env.episode_length) + 1                                               # episode_length when the action phase runs
        obs, rew, te, tr, _ex = env.step(raw.to(dev))
        rec = dict(obs=c(obs), rew=c(rew), te=c(te), tr=c(tr), rng=env._rng_c.value, raw=raw, age=age, actions=c(env.actions),
                   last=c(env.last_actions), targets=c(am.get_actions()), pos=c(env.robot.get_dofs_position(am.dofs_idx)))
        if delay is not None:
            assert am.actions is am.get_actions() and am.applied_actions is env.action_delay.out
            rec.update(applied=c(am.applied_actions), lag=c(env.action_delay.lag))
        out.append(rec)
    return env, out


def _equal_runs(a, b, keys):
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        for k in keys:
            assert (x[k] == y[k]) if k == "rng" else (x[k].dtype == y[k].dtype and torch.equal(x[k].view(torch.int32) if x[k].dtype == torch.float32 else x[k],
                                                                                              y[k].view(torch.int32) if y[k].dtype == torch.float32 else y[k])), f"step {t}: {k}"


ENV_KEYS = ("obs", "rew", "te", "tr", "rng", "actions", "last", "targets", "pos")


def test_task_hook_builds_the_delayed_manager_or_exactly_what_it_built(oracle_backend):
    from genesis_forge_amd import tasks
    from genesis_forge_amd.managers import ActuatorDelay, DelayedPositionActionManager, PositionActionManager

    env = tasks.Go2RoughTerrainEnv(num_envs=4)
    env.build()
    assert type(env.action_manager) is PositionActionManager and env.action_delay is None
    env = tasks.Go2RoughTerrainEnv(num_envs=4, action_delay={})
    env.build()
    am = env.action_manager
    assert type(am) is DelayedPositionActionManager and isinstance(env.action_delay, ActuatorDelay) and env.action_delay is am.delay
    assert (am.delay.lag_lo, am.delay.lag_hi, am.delay.slots, am.delay.num_dofs) == (0, 2, 3, 12)
    assert type(am).reset is PositionActionManager.reset                              # no reset() override: no index list
    env = tasks.Go2RoughTerrainEnv(num_envs=4, action_delay={"lag_steps": (1, 3), "max_lag": 7}, push={}, curriculum={}, height_scan={}, depth_camera={})
    env.build()
    env.reset()
    env.step(torch.zeros(4, 12))
    assert (env.action_delay.lag_lo, env.action_delay.lag_hi, env.action_delay.slots) == (1, 3, 8) and env.push is not None
    with pytest.raises(ValueError, match="5"):
        tasks.Go2RoughTerrainEnv(num_envs=4, action_delay={"lag_steps": (5, 3)}).build()


def test_env_with_a_zero_lag_is_the_env_without(oracle_backend):
    """lag_steps=(0, 0): the actuators get this step's targets through the delay's buffer — 40 steps at 64 envs, resets included,
    bit for bit the env built without the option (observations, rewards, masks, joint positions, the env's Philox counter)."""
    bare_env, bare = _env_run("cpu", trace=True, delay=None)
    assert bare_env._trace is not None and sum(int(o["te"].sum() + o["tr"].sum()) for o in bare) > 64      # resets happen
    env, zero = _env_run("cpu", trace=True, delay={"lag_steps": (0, 0)})
    _equal_runs(bare, zero, ENV_KEYS)
    assert all(torch.equal(o["applied"], o["targets"]) and (o["lag"] == 0).all() for o in zero)


@pytest.mark.parametrize("k", [1, 3])
def test_env_with_a_fixed_lag_applies_the_targets_of_k_steps_ago(oracle_backend, k):
    """applied_actions at step t is get_actions() of step t - k inside an episode — of the episode's first step while the episode is
    younger than that, so the current one in its first step —; env.actions / last_actions are the raw actions; the env's own Philox
    counter is that of the env without the delay; recorded equals ordinary, and the step stays a recorded one."""
    n = 64
    _b, bare = _env_run("cpu", trace=True, delay=None)
    plain_env, plain = _env_run("cpu", trace=False, delay={"lag_steps": (k, k)})
    env, run = _env_run("cpu", trace=True, delay={"lag_steps": (k, k)})
    assert plain_env._trace is None and env._trace is not None
    _equal_runs(plain, run, ENV_KEYS + ("applied", "lag"))
    _equal_runs(bare, run, ("rng",))
    firsts = late = 0
    for t, o in enumerate(run):
        assert (o["lag"] == k).all()
        back = torch.clamp(o["age"] - 1, max=k)                                       # steps back inside the episode
        assert int(back.max()) <= t
        want = torch.stack([run[t - int(b)]["targets"][i] for i, b in enumerate(back.tolist())])
        assert torch.equal(o["applied"].view(torch.int32), want.view(torch.int32)), f"step {t}"
        first = o["age"] == 1
        assert torch.equal(o["applied"][first], o["targets"][first])
        firsts += int(first.sum()) if t else 0
        late += int((back == k).sum())
        done = o["te"] | o["tr"]
        assert torch.equal(o["actions"][~done], o["raw"][~done])                      # the policy's raw actions …
        if t:
            assert torch.equal(o["last"][~done], run[t - 1]["actions"][~done])        # … also one step back
    assert firsts > n // 2 and late > n
    assert any(not torch.equal(o["applied"], o["targets"]) for o in run) and not all(torch.equal(a["obs"], b["obs"]) for a, b in zip(bare, run))


def test_first_call_primes_every_env_whatever_the_episode_lengths(oracle_backend):
    """Episode lengths written after reset() and before the first step (an ``init_at_random_ep_len``): the first call still primes."""
    def scatter(env):
        env.episode_length[:] = torch.randint(3, 12, (env.num_envs,), dtype=torch.int32)

    env, run = _env_run("cpu", trace=True, delay={"lag_steps": (1, 2)}, steps=4, before_first_step=scatter)
    assert (run[0]["age"] >= 4).all() and torch.equal(run[0]["applied"], run[0]["targets"])
    assert set(run[0]["lag"].tolist()) == {1, 2}
    assert not torch.equal(run[1]["applied"], run[1]["targets"])
    # … and after a reset of everything between two steps, again
    env.reset()
    scatter(env)
    env.step(torch.ones(env.num_envs, 12))
    assert torch.equal(env.action_manager.applied_actions, env.action_manager.get_actions())
    # a reset of some envs between two steps primes those and no others
    env.step(torch.full((env.num_envs, 12), 2.0))
    before = env.action_manager.get_actions().clone()
    env.reset(torch.tensor([1, 5, 6]))
    scatter(env)
    env.step(torch.full((env.num_envs, 12), -1.0))
    am, some = env.action_manager, torch.zeros(env.num_envs, dtype=torch.bool)
    some[[1, 5, 6]] = True
    assert torch.equal(am.applied_actions[some], am.get_actions()[some])
    held = ~some & (env.action_delay.lag > 0) & (env.episode_length > 2)
    assert held.any() and not torch.equal(am.applied_actions[held], am.get_actions()[held])
    assert torch.equal(am.applied_actions[held & (env.action_delay.lag == 1)], before[held & (env.action_delay.lag == 1)])


def test_ahead_of_time_signature_is_found_with_the_delay():
    """The no-GPU dry run that compiles a config's program ahead of time builds and steps the env with action_delay= too: the dry-run
    backend launches nothing, the delay included."""
    from genesis_forge_amd import _programs, tasks

    make = lambda delay: (lambda n: tasks.Go2RoughTerrainEnv(num_envs=n, scene_kwargs=dict(ang_noise=0.05, seed=9), action_delay=delay))
    assert _programs.signature_of(make({})) is not None


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the kernel raw through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_kernel_sequences(hip_backend, c):
    _check(run_raw, c)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["in", "out", "ring"])
@pytest.mark.parametrize("d", [4, 12])
def test_kernel_pointers_off_alignment(hip_backend, which, d):
    """D % 4 == 0 and one pointer a float past a 16-byte boundary: the launch goes element by element."""
    off = tuple(int(w == which) for w in ("in", "out", "ring"))
    for n in (64, 257):
        _check(run_raw, ac.case(n=n, d=d, slots=3, seed=90 + d), off=off)


@pytest.mark.gpu
@pytest.mark.parametrize("d,L", [(12, 3), (13, 8), (4, 64)])
def test_kernel_equals_step_torch_on_the_device(hip_backend, d, L):
    c = ac.case(n=1000, d=d, slots=L, seed=95, env_offset=9)
    a = _check(run_manager, c, dev="cuda", use_kernel=True)
    b = run_manager(c, dev="cuda", use_kernel=False)
    for t, (x, y) in enumerate(zip(a, b)):
        for k in STATE:
            _same(x[k], y[k], f"call {t}: kernel against _step_torch: {k}")


def _untouched_launch(nat, backend, edit):
    c = ac.case(n=70, d=12, slots=8, lag=(1, 5), head0=3)
    st, calls = ac.script(c)
    g = _raw_buffers(c, st, "cuda", init=False)
    gin = Guarded(70 * 12, torch.float32, "cuda")
    a = _raw_args(nat, c, calls[0], g, gin, [])
    edit(a)
    rc = raw_call(backend, "action_delay", a)
    sync("cuda")
    return rc, all(v.untouched() for v in g.values()) and gin.untouched()


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
def test_env_on_the_hip_backend_recorded_equals_ordinary(hip_backend):
    delay = {"lag_steps": (0, 3)}
    plain_env, plain = _env_run("cuda", trace=False, delay=delay)
    torch.cuda.synchronize()
    env, traced = _env_run("cuda", trace=True, delay=delay)
    torch.cuda.synchronize()
    assert plain_env._trace is None and env._trace is not None                        # the step is still a recorded one
    assert hasattr(env.backend, "action_delay") and env.action_delay.use_kernel
    _equal_runs(plain, traced, ENV_KEYS + ("applied", "lag"))
    lags = torch.cat([o["lag"] for o in traced])
    assert set(lags.tolist()) == {0, 1, 2, 3} and any(not torch.equal(o["applied"], o["targets"]) for o in traced)
