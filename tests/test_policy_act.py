"""RolloutStorage.act — rsl_rl's PPO.act (Normal(mean, std).sample(), log_prob(actions).sum(-1), the policy's storage rows) as one
``gf_policy_act`` launch.

* parity mode (``noise`` given): actions and the mu / sigma / values rows bit-identical to torch's ``torch.normal``-order expression
  and to the inputs; log_prob within 1e-5 of ``Normal.log_prob(...).sum(-1)`` and within a few ulp of an f32 left fold;
* Philox mode: the draws equal a numpy Philox4x32-10 + Box–Muller restatement; deterministic, a new stream per call, sharding by
  ``env_offset`` reproduces the unsharded rows, the env's own draws are untouched, and the draws have N(0, 1)'s moments;
* the CPU oracle backend evaluates the same expression from ``noise`` and refuses to draw."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from philox import philox4x32_10

TAG = 0xAC7105A3C7105EED
M32 = 0xFFFFFFFF


def _np_normals(seed: int, stream: int, env0: int, n: int, A: int) -> np.ndarray:
    """[n, A] float32: the kernel's Box–Muller on the Philox block (env0 + e, col // 4, stream) keyed by seed ^ TAG, with every f32
    rounding of the kernel restated (log, sqrt and cospi / sinpi evaluated in float64 and rounded)."""
    key = (seed ^ TAG) & 0xFFFFFFFFFFFFFFFF
    groups = (A + 3) // 4
    env = np.arange(env0, env0 + n, dtype=np.uint32)[:, None]
    grp = np.arange(groups, dtype=np.uint32)[None, :]
    w = philox4x32_10(env, grp, np.uint32(stream & M32), np.uint32((stream >> 32) & M32), key & M32, key >> 32)
    two24 = np.float32(5.9604644775390625e-8)

    def bm(w1, w2):
        u1 = ((w1 >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * two24
        u2 = (w2 >> np.uint32(8)).astype(np.float32) * two24
        lg = np.log(u1.astype(np.float64)).astype(np.float32)
        r = np.sqrt((np.float32(-2.0) * lg).astype(np.float64)).astype(np.float32)
        x = (np.float32(2.0) * u2).astype(np.float64) * np.pi
        return r * np.cos(x).astype(np.float32), r * np.sin(x).astype(np.float32)

    z0, z1 = bm(w[0], w[1])
    z2, z3 = bm(w[2], w[3])
    return np.stack([z0, z1, z2, z3], axis=-1).reshape(n, groups * 4)[:, :A]


def _left_fold_log_prob(actions, mean, std):
    """Normal.log_prob's operation order in f32, summed left to right (numpy): (log_prob [n], the sum of the magnitudes of every piece
    of every term [n] — the scale of the roundings that may differ)."""
    a, m, s = (x.detach().cpu().numpy().astype(np.float32) for x in (actions, mean, std.expand_as(mean)))
    d = a - m
    q = -(d * d) / (np.float32(2.0) * (s * s))
    ls = np.log(s.astype(np.float64)).astype(np.float32)
    t = (q - ls) - np.float32(math.log(math.sqrt(2 * math.pi)))
    lp = t[:, 0].copy()
    for c in range(1, t.shape[1]):
        lp = lp + t[:, c]
    return lp, (np.abs(q) + np.abs(ls) + np.float32(1.0)).sum(1)


def _assert_fold(lp, actions, mean, std):
    fold, scale = (torch.from_numpy(x).to(lp.device) for x in _left_fold_log_prob(actions, mean, std))
    tol = 4 * torch.finfo(torch.float32).eps * scale
    assert bool(((lp - fold).abs() <= tol).all()), "log_prob is a left fold of Normal.log_prob's terms"


def _inputs(n, A, std_rows, dev, seed=0):
    g = torch.Generator().manual_seed(seed * 1009 + n + A)
    mean = torch.randn(n, A, generator=g).to(dev)
    std = (torch.rand((n, A) if std_rows else (A,), generator=g) * 1.5 + 0.05).to(dev)
    values = torch.randn(n, 1, generator=g).to(dev)
    noise = torch.randn(n, A, generator=g).to(dev)
    return mean, std, values, noise


def _raw(backend, mean, std, values, noise=None, seed=1, stream=0, env_offset=0, rows=True):
    """gf_policy_act through the raw ABI into fresh output tensors: (actions, actions_out, mu, sigma, values, log_prob)."""
    from genesis_forge_amd import _native as nat

    n, A = mean.shape
    outs = [torch.full((n, A), 7.0, device=mean.device) for _ in range(4)] + [torch.full((n,), 7.0, device=mean.device) for _ in range(2)]
    a = nat.GfPolicyActArgs()
    a.num_envs, a.num_actions, a.std_per_env = n, A, 1 if std.dim() == 2 else 0
    a.mean, a.std, a.values, a.noise = mean.data_ptr(), std.data_ptr(), values.data_ptr(), None if noise is None else noise.data_ptr()
    a.seed, a.stream, a.env_offset = seed, stream, env_offset
    a.actions = outs[0].data_ptr()
    if rows:
        a.actions_out, a.mu_out, a.sigma_out, a.values_out, a.log_prob_out = (o.data_ptr() for o in outs[1:])
    backend.policy_act(a)
    torch.cuda.synchronize()
    return outs


# -- GPU ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1000, 4133, 65536])
@pytest.mark.parametrize("A", [1, 12, 28, 37])
@pytest.mark.parametrize("std_rows", [False, True])
def test_parity_noise(hip_backend, n, A, std_rows):
    mean, std, values, noise = _inputs(n, A, std_rows, "cuda")
    actions, act_row, mu, sigma, v, lp = _raw(hip_backend, mean, std, values, noise)
    want = mean + std * noise   # torch.normal(mean, std): normal_(0, 1) * std + mean
    assert torch.equal(actions, want) and torch.equal(act_row, want)
    assert torch.equal(mu, mean) and torch.equal(sigma, std.expand_as(mean)) and torch.equal(v, values[:, 0])
    ref = torch.distributions.Normal(mean, std).log_prob(actions).sum(-1)
    assert float((lp - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))
    _assert_fold(lp, actions, mean, std)


@pytest.mark.gpu
@pytest.mark.parametrize("n,A", [(1000, 12), (4133, 37), (65536, 12), (4133, 1)])
def test_philox_draws_match_numpy(hip_backend, n, A):
    mean, std, values, _ = _inputs(n, A, False, "cuda", seed=2)
    zero, one = torch.zeros_like(mean), torch.ones(A, device="cuda")
    eps = _raw(hip_backend, zero, one, values, seed=1234, stream=5)[0]
    want = _np_normals(1234, 5, 0, n, A)
    got = eps.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= 1e-6
    # with a real mean and std the sample is mean + std * eps, eps the same draws
    actions = _raw(hip_backend, mean, std, values, seed=1234, stream=5)[0]
    assert torch.equal(actions, mean + std * eps)


@pytest.mark.gpu
def test_draws_deterministic_streams_and_sharding(hip_backend):
    n, A = 4133, 12
    mean, std, values, _ = _inputs(n, A, True, "cuda", seed=3)
    a0 = _raw(hip_backend, mean, std, values, seed=77, stream=3)
    a1 = _raw(hip_backend, mean, std, values, seed=77, stream=3)
    for x, y in zip(a0, a1):
        assert torch.equal(x, y), "the same (seed, stream) draws the same"
    b = _raw(hip_backend, mean, std, values, seed=77, stream=4)[0]
    assert float((b == a0[0]).float().mean()) < 1e-3, "another stream draws other numbers"
    c = _raw(hip_backend, mean, std, values, seed=78, stream=3)[0]
    assert float((c == a0[0]).float().mean()) < 1e-3, "another seed draws other numbers"
    for k in (1, 1000, 2049):   # a rank holding envs k… of the same run
        part = _raw(hip_backend, mean[k:].contiguous(), std[k:].contiguous(), values[k:].contiguous(), seed=77, stream=3, env_offset=k)
        for x, y in zip(part, a0):
            assert torch.equal(x, y[k:]), f"env_offset={k} reproduces rows {k}… of the unsharded call"


@pytest.mark.gpu
def test_moments_of_the_draws(hip_backend):
    n, A = 65536, 12
    zero, one = torch.zeros(n, A, device="cuda"), torch.ones(A, device="cuda")
    eps = _raw(hip_backend, zero, one, torch.zeros(n, device="cuda"), seed=99, stream=0)[0].double()
    m, v = eps.mean(0), eps.var(0)
    assert float(m.abs().max()) < 5 / math.sqrt(n) and float((v - 1).abs().max()) < 5 * math.sqrt(2 / n)
    z = (eps - m) / v.sqrt()
    assert abs(float(z.pow(3).mean())) < 0.05 and abs(float(z.pow(4).mean()) - 3) < 0.1
    corr = torch.corrcoef(eps.T)
    off = corr - torch.eye(A, dtype=corr.dtype, device=corr.device)
    assert float(off.abs().max()) < 5 / math.sqrt(n), "columns (and the two halves of every Box–Muller pair) are uncorrelated"
    # successive envs (counter word 0) are independent too
    assert abs(float(torch.corrcoef(torch.stack([eps[:-1, 0], eps[1:, 0]]))[0, 1])) < 5 / math.sqrt(n)


@pytest.mark.gpu
def test_abi_sizes_and_refusals(hip_backend):
    from genesis_forge_amd import _native as nat

    lib = hip_backend.lib
    assert lib.gf_sizeof(nat.GF_SIZEOF_POLICY_ACT) == C.sizeof(nat.GfPolicyActArgs)
    n, A = 100, 12
    mean, std, values, noise = _inputs(n, A, False, "cuda")
    out = torch.zeros(n, A, device="cuda")
    vrow = torch.zeros(n, device="cuda")

    def args(**kw):
        a = nat.GfPolicyActArgs()
        a.num_envs, a.num_actions, a.mean, a.std, a.values, a.actions = n, A, mean.data_ptr(), std.data_ptr(), values.data_ptr(), out.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    call = lambda a: lib.gf_policy_act(C.byref(a), None)
    assert call(args()) == 0
    assert call(args(mean=None)) == -1 and call(args(std=None)) == -1 and call(args(actions=None)) == -1
    assert call(args(values=None, values_out=vrow.data_ptr())) == -1
    assert call(args(num_actions=0)) == -2 and call(args(num_envs=-1)) == -2 and call(args(std_per_env=2)) == -2
    out.fill_(3.0)
    torch.cuda.synchronize()
    assert call(args(num_envs=0)) == 0
    torch.cuda.synchronize()
    assert bool((out == 3).all()), "num_envs == 0 launches nothing"


def _go2(n, trace=True, seed=7):
    from genesis_forge_amd import tasks

    env = tasks.Go2CommandDirectionEnv(num_envs=n, max_episode_length_s=0.4, cmd_resample_s=0.2, scene_kwargs=dict(ang_noise=0.3, seed=3))
    env.trace_enabled = trace
    env.build()
    env.seed(seed)
    return env


@pytest.mark.gpu
def test_storage_act_rows_streams_and_env_draws(hip_backend):
    """Through RolloutStorage: row ``step`` (0 when full), a new stream per call, seed() restarts it, and the env's draws — its
    stream counter and the trajectory — are the same with and without act() calls in between."""
    from genesis_forge_amd.learner import RolloutStorage

    n, T = 1000, 3
    env, twin = _go2(n), _go2(n)
    obs, _ = env.reset()
    obs2, _ = twin.reset()
    store = RolloutStorage(env, T).attach()
    store.begin(obs)
    assert store.actions is None, "a storage allocates its policy rows on first use"
    A = env.action_space.shape[0]
    std = torch.full((A,), 0.5, device="cuda")
    first = None
    for k in range(2 * T + 1):
        mean = torch.randn(n, A, generator=torch.Generator().manual_seed(k)).cuda() * 0.1
        values = torch.zeros(n, 1, device="cuda")
        t = 0 if store.full else store.step
        rng = env._rng_stream
        actions = store.act(mean, std, values)
        assert env._rng_stream == rng, "act() never advances the env's stream"
        torch.cuda.synchronize()
        assert torch.equal(store.actions[t], actions) and torch.equal(store.mu[t], mean)
        assert torch.equal(store.sigma[t], std.expand(n, A)) and torch.equal(store.values[t], values[:, 0])
        eps = torch.from_numpy(_np_normals(env._rng_seed, k, 0, n, A)).cuda()
        assert float((actions - (mean + std * eps)).abs().max()) <= 1e-6
        if first is None:
            first = actions.clone()
        fixed = torch.zeros(n, A, device="cuda")   # the same action for both envs: the trajectories must stay equal
        out = env.step(fixed)
        out2 = twin.step(fixed)
        assert env._rng_stream == twin._rng_stream
        for x, y in zip(out[:4], out2[:4]):
            assert torch.equal(x, y), "the env's trajectory does not depend on act()"
    store.seed(env._rng_seed)
    again = store.act(torch.randn(n, A, generator=torch.Generator().manual_seed(0)).cuda() * 0.1, std, torch.zeros(n, device="cuda"))
    assert torch.equal(again, first), "seed() restarts the stream"


@pytest.mark.gpu
def test_act_refuses_bad_inputs(hip_backend):
    _check_refusals("cuda")


# -- CPU (oracle backend) -----------------------------------------------------------------------------------------------------------
def _check_refusals(dev):
    from genesis_forge_amd.learner import RolloutStorage

    env = _go2(64, trace=False)
    obs, _ = env.reset()
    store = RolloutStorage(env, 4).attach()
    store.begin(obs)
    n, A = 64, 12
    mean, std, values = torch.zeros(n, A, device=dev), torch.ones(A, device=dev), torch.zeros(n, device=dev)
    bad = [
        (mean.double(), std, values), (mean, std.half(), values), (mean, std, values.long()),
        (mean[:, :6], std, values), (mean, torch.ones(A + 1, device=dev), values), (mean, std, torch.zeros(n + 1, device=dev)),
        (mean, torch.ones(n, 1, device=dev), values), (mean[:-1], std, values[:-1]), (torch.zeros(n, 2 * A, device=dev)[:, ::2], std, values),
        (torch.zeros(n, A, device=dev).T.contiguous().T, std, values), (mean, std, torch.zeros(n, 2, device=dev)),
    ]
    other = "cpu" if dev != "cpu" else ("meta")
    bad.append((mean.to(other), std, values))
    for m, s, v in bad:
        with pytest.raises(ValueError):
            store.act(m, s, v, noise=torch.zeros(n, A, device=dev))
    with pytest.raises(ValueError):
        store.act(mean, std, values, noise=torch.zeros(n, A, device=dev, dtype=torch.float64))
    with pytest.raises(ValueError):
        store.act(mean, std, values, noise=torch.zeros(n, A + 1, device=dev))


def test_act_refuses_bad_inputs_cpu(oracle_backend):
    _check_refusals("cpu")


@pytest.mark.parametrize("A,std_rows", [(12, False), (37, True), (1, False)])
def test_oracle_act_matches_restatement(oracle_backend, A, std_rows):
    from genesis_forge_amd.learner import RolloutStorage

    n = 70
    env = _go2(n, trace=False)
    obs, _ = env.reset()
    store = RolloutStorage(env, 3).attach()
    store.begin(obs)
    mean, std, values, noise = _inputs(n, A, std_rows, "cpu")
    with pytest.raises(RuntimeError, match="noise"):
        store.act(mean, std, values)
    actions = store.act(mean, std, values, noise=noise)
    want = mean + std * noise
    assert torch.equal(actions, want) and torch.equal(store.actions[0], want) and torch.equal(store.mu[0], mean)
    assert torch.equal(store.sigma[0], std.expand(n, A)) and torch.equal(store.values[0], values[:, 0])
    ref = torch.distributions.Normal(mean, std).log_prob(actions).sum(-1)
    assert float((store.actions_log_prob[0] - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))
    _assert_fold(store.actions_log_prob[0], actions, mean, std)
