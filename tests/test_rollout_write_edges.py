"""gf_rollout_write and gf_rollout_policy_write through the raw C ABI, at the sizes where their launch takes another shape.

Both kernels size one launch by ``max(ceil(N*W / 4), N)`` lanes: a lane copies four floats of the [N, W] array and, if its index is
below N, moves env ``index``'s columns.  With W (or A) of 1, 2 or 3 the per-env lanes outnumber the copy lanes; the 16-byte copy path
needs every pointer aligned and ``N*W % 4 == 0``.  Every case runs on the GPU and on the CPU oracle twin, against torch ``copy_``,
``terminated | truncated`` and ``r + (gamma * v) * time_out`` in float32 — copied arrays bit for bit on int32 views (the sources
carry NaN payloads, -0.0, a denormal and inf), every array a slice of a guarded buffer (tests/guarded.py)."""
import numpy as np
import pytest
import torch

from genesis_forge_amd import _native as nat
from guarded import Guarded, raw_call, sync

GF_E_NULL, GF_E_RANGE = -1, -2
SIZES = [1, 3, 255, 256, 257, 1025]          # one lane … one workgroup of 256 lanes, one more, and five workgroups
MASK_BYTES = [0, 1, 2, 0x80, 0xFF]           # "nonzero = set": the stored done byte is 0 or 1 whatever the source byte
SPECIALS = (0x7FC01234, 0xFFA00001, 0x80000000, 0x00000001, 0x7F800000)
GAMMA = 0.99


def _bits(numel, seed):
    """Distinct float32 bit patterns as int32, specials among them."""
    x = np.arange(numel, dtype=np.int64) + 0x3F000000 + (seed << 16)
    for i, s in enumerate(SPECIALS):
        if numel:
            x[(i * 7919 + seed) % numel] = s
    return torch.from_numpy(x.astype(np.uint32).view(np.int32))


def _mask(n, seed, p=0.5):
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor(MASK_BYTES, dtype=torch.uint8)
    m = vals[torch.randint(1, len(MASK_BYTES), (n,), generator=g)]
    return torch.where(torch.rand(n, generator=g) < p, m, torch.zeros_like(m))


def _ptr(g):
    return None if g is None else g.ptr


# ---- gf_rollout_write ---------------------------------------------------------------------------------------------------------------
def _rollout(backend, dev, n, W, *, obs_out=True, reward_out=True, done_out=True, truncated=True, obs_off=0, width=None):
    width = W if width is None else width
    obs_src, rew_src = _bits(n * W, 1), _bits(n, 2)
    term, trunc = _mask(n, 3), _mask(n, 4, 0.3)
    G = lambda numel, dt, init=None, off=0: Guarded(numel, dt, dev, off=off, init=init)
    obs, reward = G(n * W, torch.int32, obs_src, obs_off), G(n, torch.int32, rew_src)
    te, tr = G(n, torch.uint8, term), G(n, torch.uint8, trunc)
    o_out, r_out, d_out = G(n * W, torch.int32), G(n, torch.int32), G(n, torch.uint8)
    a = nat.GfRolloutArgs()
    a.num_envs, a.obs_width = n, width
    a.obs, a.reward, a.terminated, a.truncated = obs.ptr, reward.ptr, te.ptr, (tr.ptr if truncated else None)
    a.obs_out, a.reward_out, a.done_out = (o_out.ptr if obs_out else None), (r_out.ptr if reward_out else None), (d_out.ptr if done_out else None)
    assert raw_call(backend, "rollout_write", a) == 0
    sync(dev)
    tag = (n, W, obs_out, reward_out, done_out, truncated, obs_off, width)
    for src in (obs, reward, te, tr):
        assert src.guards_ok(), tag
    assert torch.equal(obs.cpu(), obs_src) and torch.equal(reward.cpu(), rew_src) and torch.equal(te.cpu(), term) and torch.equal(tr.cpu(), trunc), ("a source changed", tag)
    if obs_out and width:
        assert o_out.guards_ok() and torch.equal(o_out.cpu(), obs_src), ("observations", tag)
    else:
        assert o_out.untouched(), ("obs_out NULL or obs_width 0", tag)
    if reward_out:
        assert r_out.guards_ok() and torch.equal(r_out.cpu(), rew_src), ("rewards", tag)
    else:
        assert r_out.untouched(), tag
    if done_out:
        want = ((term != 0) | (trunc != 0)) if truncated else (term != 0)
        assert d_out.guards_ok() and torch.equal(d_out.cpu(), want.to(torch.uint8)), ("dones: terminated | truncated as 0 / 1", tag)
    else:
        assert d_out.untouched(), tag


def _rollout_variants(backend, dev):
    for n, W in ((3, 2), (257, 3), (1025, 1), (256, 48)):
        _rollout(backend, dev, n, W, obs_out=False)                  # the launch is sized by N alone
        _rollout(backend, dev, n, W, truncated=False)
        _rollout(backend, dev, n, W, reward_out=False)
        _rollout(backend, dev, n, W, done_out=False)
        _rollout(backend, dev, n, W, width=0)                        # nothing to copy, the per-env columns still move
    for n, W in ((256, 1), (2, 2), (1025, 4), (3, 48)):             # N*W % 4 == 0, obs 4 bytes off: the element path by address
        assert (n * W) % 4 == 0
        _rollout(backend, dev, n, W, obs_off=1)


@pytest.mark.parametrize("W", [1, 2, 3, 4, 5, 48])
@pytest.mark.parametrize("n", SIZES)
def test_rollout_write_oracle(oracle_backend, n, W):
    _rollout(oracle_backend, "cpu", n, W)


@pytest.mark.gpu
@pytest.mark.parametrize("W", [1, 2, 3, 4, 5, 48])
@pytest.mark.parametrize("n", SIZES)
def test_rollout_write_hip(hip_backend, n, W):
    _rollout(hip_backend, "cuda", n, W)


def test_rollout_write_variants_oracle(oracle_backend):
    _rollout_variants(oracle_backend, "cpu")


@pytest.mark.gpu
def test_rollout_write_variants_hip(hip_backend):
    _rollout_variants(hip_backend, "cuda")


# ---- gf_rollout_policy_write ----------------------------------------------------------------------------------------------------------
ROWS = ("actions", "mu", "sigma")
COLS = ("values", "log_prob")


def _policy(backend, dev, n, A, *, drop=(), time_outs=True, off=None):
    """``drop``: outputs passed as NULL (their sources stay); ``off``: the one [N, A] source that starts 4 bytes off."""
    g = torch.Generator().manual_seed(n * 100 + A)
    src = {name: _bits(n * A, 5 + i) for i, name in enumerate(ROWS)}
    v, r = torch.randn(n, generator=g), torch.randn(n, generator=g)
    src["values"], src["log_prob"] = v.view(torch.int32).clone(), _bits(n, 9)
    to = _mask(n, 10)
    G = lambda numel, dt, init=None, o=0: Guarded(numel, dt, dev, off=o, init=init)
    ins = {name: G(src[name].numel(), torch.int32, src[name], 1 if name == off else 0) for name in ROWS + COLS}
    outs = {name: G(src[name].numel(), torch.int32) for name in ROWS + COLS}
    g_to, g_row = G(n, torch.uint8, to), G(n, torch.int32, r.view(torch.int32))
    a = nat.GfRolloutPolicyArgs()
    a.num_envs, a.num_actions, a.gamma = n, A, GAMMA
    for name in ROWS + COLS:
        setattr(a, name, ins[name].ptr)
        setattr(a, name + "_out", None if name in drop else outs[name].ptr)
    a.time_outs, a.reward_row = (g_to.ptr if time_outs else None), g_row.ptr
    assert raw_call(backend, "rollout_policy_write", a) == 0
    sync(dev)
    tag = (n, A, drop, time_outs, off)
    for name in ROWS + COLS:
        assert ins[name].guards_ok() and torch.equal(ins[name].cpu(), src[name]), ("a source changed", name, tag)
        if name in drop:
            assert outs[name].untouched(), (name, tag)
        else:
            assert outs[name].guards_ok() and torch.equal(outs[name].cpu(), src[name]), (name, tag)
    assert g_row.guards_ok() and g_to.guards_ok()
    want = r + (torch.tensor(GAMMA, dtype=torch.float32) * v) * (to != 0).to(torch.float32) if time_outs else r
    assert torch.equal(g_row.cpu(), want.view(torch.int32)), ("reward_row = r + (gamma * v) * time_out, or untouched without time_outs", tag)


def _policy_variants(backend, dev):
    for n, A in ((3, 1), (257, 3), (1025, 2), (256, 12)):
        for name in ROWS + COLS:
            _policy(backend, dev, n, A, drop=(name,))
        _policy(backend, dev, n, A, drop=ROWS)                       # the launch still covers the N per-env columns
        _policy(backend, dev, n, A, time_outs=False)
    for n, A in ((256, 1), (2, 2), (1025, 4), (3, 12)):
        assert (n * A) % 4 == 0
        for name in ROWS:
            _policy(backend, dev, n, A, off=name)


@pytest.mark.parametrize("A", [1, 2, 3, 4, 12, 37])
@pytest.mark.parametrize("n", SIZES)
def test_rollout_policy_write_oracle(oracle_backend, n, A):
    _policy(oracle_backend, "cpu", n, A)


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 2, 3, 4, 12, 37])
@pytest.mark.parametrize("n", SIZES)
def test_rollout_policy_write_hip(hip_backend, n, A):
    _policy(hip_backend, "cuda", n, A)


def test_rollout_policy_write_variants_oracle(oracle_backend):
    _policy_variants(oracle_backend, "cpu")


@pytest.mark.gpu
def test_rollout_policy_write_variants_hip(hip_backend):
    _policy_variants(hip_backend, "cuda")


def _refusals(backend, dev):
    """Before anything is launched: GF_E_NULL — args, an output without its source, time_outs without reward_row or values;
    GF_E_RANGE — a negative size.  num_envs == 0 is a no-op."""
    n, A = 5, 3
    buf = Guarded(n * A, torch.int32, dev)
    call = lambda a: raw_call(backend, "rollout_policy_write", a)

    def args(**kw):
        a = nat.GfRolloutPolicyArgs()
        a.num_envs, a.num_actions = n, A
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for name in ROWS + COLS:
        assert call(args(**{name + "_out": buf.ptr})) == GF_E_NULL, name
    assert call(args(time_outs=buf.ptr, values=buf.ptr)) == GF_E_NULL, "time_outs without reward_row"
    assert call(args(time_outs=buf.ptr, reward_row=buf.ptr)) == GF_E_NULL, "time_outs without values"
    assert call(args(num_envs=-1)) == GF_E_RANGE and call(args(num_actions=-1)) == GF_E_RANGE
    assert call(args(num_envs=0, actions=buf.ptr, actions_out=buf.ptr)) == 0
    r = nat.GfRolloutArgs()
    r.num_envs, r.obs_width = n, A
    rcall = lambda: raw_call(backend, "rollout_write", r)
    r.obs_out = buf.ptr
    assert rcall() == GF_E_NULL
    r.obs_out, r.reward_out = None, buf.ptr
    assert rcall() == GF_E_NULL
    r.reward_out, r.done_out = None, buf.ptr
    assert rcall() == GF_E_NULL
    r.done_out, r.num_envs = None, -1
    assert rcall() == GF_E_RANGE
    r.num_envs, r.obs_width = n, -1
    assert rcall() == GF_E_RANGE
    sync(dev)
    assert buf.untouched()


def test_rollout_refusals_oracle(oracle_backend):
    _refusals(oracle_backend, "cpu")


@pytest.mark.gpu
def test_rollout_refusals_hip(hip_backend):
    _refusals(hip_backend, "cuda")
