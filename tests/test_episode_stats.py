"""EpisodeStatistics and RolloutStorage.process_env_step — rsl_rl's runner bookkeeping (rewbuffer / lenbuffer) and PPO's time-out
bootstrap as one ``gf_episode_step`` launch, and the whole fused collection loop (act → env.step → process_env_step).

Everything is compared with a Python restatement of rsl_rl's lines (``collections.deque(maxlen=window)``): ring contents in order,
``cur_*`` and both means bit for bit; bootstrapped rewards bit-identical to ``r + (gamma * v) * time_out``."""
import ctypes as C
import math
import statistics
from collections import deque

import pytest
import torch


class RunnerRef:
    """OnPolicyRunner.learn's episode bookkeeping, line for line."""

    def __init__(self, n, window, dev):
        self.cur_reward_sum = torch.zeros(n, dtype=torch.float, device=dev)
        self.cur_episode_length = torch.zeros(n, dtype=torch.float, device=dev)
        self.rewbuffer, self.lenbuffer = deque(maxlen=window), deque(maxlen=window)

    def step(self, rewards, dones):
        self.cur_reward_sum += rewards
        self.cur_episode_length += 1
        new_ids = (dones > 0).nonzero(as_tuple=False)
        self.rewbuffer.extend(self.cur_reward_sum[new_ids][:, 0].cpu().numpy().tolist())
        self.lenbuffer.extend(self.cur_episode_length[new_ids][:, 0].cpu().numpy().tolist())
        self.cur_reward_sum[new_ids] = 0
        self.cur_episode_length[new_ids] = 0


def _same(stats, ref):
    assert stats.rewbuffer == list(ref.rewbuffer), "rewbuffer (oldest first)"
    assert stats.lenbuffer == list(ref.lenbuffer), "lenbuffer (oldest first)"
    assert torch.equal(stats.cur_reward_sum, ref.cur_reward_sum) and torch.equal(stats.cur_episode_length, ref.cur_episode_length)
    if ref.rewbuffer:
        assert stats.mean_reward() == statistics.mean(ref.rewbuffer)
        assert stats.mean_episode_length() == statistics.mean(ref.lenbuffer)
    else:
        assert stats.mean_reward() is None and stats.mean_episode_length() is None


def _done_mask(n, step, window, g):
    """A step's done mask: the step number picks how many envs finish — none, one, exactly window, more than window, or a fraction."""
    kind = step % 6
    count = [0, 1, window, window + 1 + step % 13, min(n, 3 * window + 5), -1][kind]
    if count < 0:
        return torch.rand(n, generator=g) < 0.02 * (1 + step % 4)
    mask = torch.zeros(n, dtype=torch.bool)
    mask[torch.randperm(n, generator=g)[:min(count, n)]] = True
    return mask


def _synthetic(dev, n, window, steps, check_every):
    from genesis_forge_amd.learner import EpisodeStatistics

    g = torch.Generator().manual_seed(n * 31 + window)
    stats, ref = EpisodeStatistics(n, window), RunnerRef(n, window, dev)
    for s in range(steps):
        rewards = (torch.randn(n, generator=g) * (1 + s % 5)).to(dev)
        dones = _done_mask(n, s, window, g).to(dev)
        stats.update(rewards, dones)
        ref.step(rewards, dones)
        if s % check_every == check_every - 1 or s == steps - 1:
            _same(stats, ref)
    stats.reset()
    assert stats.rewbuffer == [] and stats.mean_reward() is None and not bool(stats.cur_reward_sum.any())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1000, 4133, 65536, 1048576])
@pytest.mark.parametrize("window", [7, 100])
def test_synthetic_streams_hip(hip_backend, n, window):
    _synthetic("cuda", n, window, 300, 25 if n < 100000 else 60)


def test_synthetic_streams_cpu(oracle_backend):
    _synthetic("cpu", 4133, 7, 60, 7)
    _synthetic("cpu", 1000, 100, 60, 11)


# -- raw ABI ------------------------------------------------------------------------------------------------------------------------
def _ep_args(n, rewards, dones=None, time_outs=None, values=None, stats=None, gamma=0.99):
    from genesis_forge_amd import _native as nat

    a = nat.GfEpisodeArgs()
    a.num_envs, a.rewards, a.gamma = n, rewards, gamma
    a.dones, a.time_outs, a.values = dones, time_outs, values
    if stats is not None:
        stats._fill(a)
    return a


@pytest.mark.gpu
def test_abi_sizes_and_refusals(hip_backend):
    from genesis_forge_amd import _native as nat
    from genesis_forge_amd.learner import EpisodeStatistics

    lib = hip_backend.lib
    assert lib.gf_sizeof(nat.GF_SIZEOF_EPISODE) == C.sizeof(nat.GfEpisodeArgs)
    n = 5000
    r, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    d, to = torch.zeros(n, dtype=torch.bool, device="cuda"), torch.zeros(n, dtype=torch.bool, device="cuda")
    st = EpisodeStatistics(n, 10)
    call = lambda a: lib.gf_episode_step(C.byref(a), None)
    P = lambda t: t.data_ptr()
    assert call(_ep_args(n, P(r), P(d), stats=st)) == 0
    assert call(_ep_args(n, P(r), time_outs=P(to), values=P(v))) == 0
    assert call(_ep_args(n, None, P(d), stats=st)) == -1
    assert call(_ep_args(n, P(r), None, stats=st)) == -1
    assert call(_ep_args(n, P(r), time_outs=P(to))) == -1, "a bootstrap without a value row"
    a = _ep_args(n, P(r), P(d), stats=st)
    a.ring_state = None
    assert call(a) == -1
    a = _ep_args(n, P(r), P(d))
    a.ring_reward = P(st.ring_reward)
    assert call(a) == -1, "half a statistics set"
    a = _ep_args(n, P(r), P(d), stats=st)
    a.window = 0
    assert call(a) == -2
    a = _ep_args(n, P(r), P(d), stats=st)
    a.parity = 2
    assert call(a) == -2
    assert call(_ep_args(-1, P(r), P(d), stats=st)) == -2
    big = EpisodeStatistics(nat.GF_EPISODE_SINGLE_MAX + 1, 10)
    rb, db = torch.zeros(big.num_envs, device="cuda"), torch.zeros(big.num_envs, dtype=torch.bool, device="cuda")
    a = _ep_args(big.num_envs, P(rb), P(db), stats=big)
    a.block_counts = None
    assert call(a) == -1, "two launches need the per-block counts"
    torch.cuda.synchronize()


# -- through RolloutStorage ---------------------------------------------------------------------------------------------------------
def _go2(n, trace=True, noise=0.3, output="fresh"):
    from genesis_forge_amd import tasks
    from genesis_forge_amd.managers import ObservationManager

    old, ObservationManager.default_output = ObservationManager.default_output, output
    try:
        env = tasks.Go2CommandDirectionEnv(num_envs=n, max_episode_length_s=0.4, cmd_resample_s=0.2, scene_kwargs=dict(ang_noise=noise, seed=3))
        env.trace_enabled = trace
        env.build()
    finally:
        ObservationManager.default_output = old
    env.seed(7)
    return env


def _gait(n, trace=True):
    from genesis_forge_amd import tasks

    env = tasks.Go2GaitTrainingEnv(num_envs=n, max_episode_length_s=0.4, scene_kwargs=dict(ang_noise=0.3, seed=3, contact_prob=0.05))
    env.trace_enabled = trace
    env.build()
    env.seed(7)
    return env


def _recorded_env_stats(dev, n, steps, window):
    """A recorded go2_cmd env at a high reset rate: statistics and bootstrap from process_env_step vs the runner's lines and PPO's
    expression on what the step returned."""
    from genesis_forge_amd.learner import EpisodeStatistics, RolloutStorage

    env = _go2(n, noise=0.8)
    obs, _ = env.reset()
    T = 5
    store = RolloutStorage(env, T).attach()
    store.begin(obs)
    stats, ref = EpisodeStatistics(n, window), RunnerRef(n, window, dev)
    A = env.action_space.shape[0]
    g = torch.Generator().manual_seed(5)
    finished = 0
    for s in range(steps):
        values = torch.randn(n, generator=g).to(dev)
        actions = store.act(torch.zeros(n, A, device=dev), torch.full((A,), 0.3, device=dev), values, noise=torch.randn(n, A, generator=g).to(dev))
        _obs, rew, term, trunc, _ = env.step(actions)
        t = store.step - 1
        raw = store.rewards[t].clone()
        assert torch.equal(raw, rew)
        store.process_env_step(trunc, gamma=0.97, episodes=stats)
        ref.step(rew, term | trunc)
        finished += int((term | trunc).sum())
        want = raw + (0.97 * store.values[t]) * trunc.to(torch.float32)
        assert torch.equal(store.rewards[t], want), "the bootstrap is r + (gamma * v) * time_out"
        if s % 10 == 9 or s == steps - 1:
            _same(stats, ref)
    assert env._trace is not None and finished > 3 * window, "a high reset rate"


@pytest.mark.gpu
@pytest.mark.parametrize("n,window", [(4133, 100), (65536, 7)])
def test_recorded_env_stats_hip(hip_backend, n, window):
    _recorded_env_stats("cuda", n, 40, window)


def test_recorded_env_stats_cpu(oracle_backend):
    _recorded_env_stats("cpu", 70, 30, 7)


def _storage_refusals(dev):
    from genesis_forge_amd.learner import EpisodeStatistics, RolloutStorage

    n = 64
    env = _go2(n, trace=False)
    obs, _ = env.reset()
    store = RolloutStorage(env, 3).attach()
    store.begin(obs)
    A = env.action_space.shape[0]
    stats = EpisodeStatistics(n)
    with pytest.raises(RuntimeError, match="follows"):
        store.process_env_step(None, episodes=stats)
    *_, trunc, _ = env.step(torch.zeros(n, A, device=dev))
    with pytest.raises(RuntimeError, match="policy rows"):
        store.process_env_step(trunc, episodes=stats)
    z = torch.zeros(n, A, device=dev)
    store.add_policy(z, torch.zeros(n, device=dev), torch.zeros(n, device=dev), z, z + 1, time_outs=trunc)
    with pytest.raises(RuntimeError, match="bootstrapped"):
        store.process_env_step(trunc)
    store.process_env_step(None, episodes=stats)   # the statistics alone are fine
    with pytest.raises(ValueError):
        store.process_env_step(None, episodes=EpisodeStatistics(n + 1))
    store.act(z, torch.ones(A, device=dev), torch.zeros(n, device=dev), noise=z)
    *_, trunc, _ = env.step(torch.zeros(n, A, device=dev))
    store.process_env_step(trunc, episodes=stats)
    with pytest.raises(RuntimeError, match="bootstrapped"):
        store.process_env_step(trunc)
    with pytest.raises(ValueError):
        stats.update(torch.zeros(n, dtype=torch.float64, device=dev), trunc)
    with pytest.raises(ValueError):
        stats.update(torch.zeros(n + 1, device=dev), trunc)
    with pytest.raises(ValueError):
        EpisodeStatistics(n, 0)


@pytest.mark.gpu
def test_storage_refusals_hip(hip_backend):
    _storage_refusals("cuda")


def test_storage_refusals_cpu(oracle_backend):
    _storage_refusals("cpu")


# -- the whole collection loop ------------------------------------------------------------------------------------------------------
def _loops(dev, make_env, groups, T=24, rollouts=2):
    """Two identical envs in lockstep: the fused loop (act → step → process_env_step) and rsl_rl's (torch Normal → step →
    add_policy(time_outs=…) → the runner's bookkeeping), fed the same noise.  Rows, returns and statistics must agree."""
    from genesis_forge_amd.learner import ActorCriticMLP, EpisodeStatistics, RolloutStorage

    envs = [make_env(), make_env()]
    n, A = envs[0].num_envs, envs[0].action_space.shape[0]
    starts = [e.reset() for e in envs]
    stores = [RolloutStorage(e, T, obs_groups=groups).attach() for e in envs]
    for st, (obs, extras) in zip(stores, starts):
        st.begin(obs, extras)
    torch.manual_seed(0)
    policy = ActorCriticMLP(stores[0].obs_width, A, (64, 32), (64, 32), init_noise_std=0.7).to(dev)
    with torch.no_grad():
        policy.std.copy_(torch.linspace(0.3, 1.2, A))
    stats, ref = EpisodeStatistics(n, 50), RunnerRef(n, 50, dev)
    g = torch.Generator().manual_seed(1)
    obs = [s[0] for s in starts]
    sync = dev != "cpu"
    for k in range(T * rollouts):
        assert torch.equal(obs[0], obs[1])
        with torch.no_grad():
            mean, values = policy.act_mean(obs[0]), policy.evaluate(obs[0])
        noise = torch.randn(n, A, generator=g).to(dev)
        std = policy.std.detach()
        # fused
        if sync:
            torch.cuda.set_sync_debug_mode("error")
        try:
            actions = stores[0].act(mean, std, values, noise=noise)
        finally:
            if sync:
                torch.cuda.set_sync_debug_mode(0)
        o0, _r0, _te0, tr0, _ = envs[0].step(actions)
        if sync:
            torch.cuda.set_sync_debug_mode("error")
        try:
            stores[0].process_env_step(tr0, gamma=0.99, episodes=stats)
        finally:
            if sync:
                torch.cuda.set_sync_debug_mode(0)
        # rsl_rl
        dist = torch.distributions.Normal(mean, std)
        a_ref = mean + std * noise
        lp = dist.log_prob(a_ref).sum(-1)
        o1, r1, te1, tr1, _ = envs[1].step(a_ref)
        stores[1].add_policy(a_ref, values, lp, mean, std.expand(n, A), time_outs=tr1)
        ref.step(r1, te1 | tr1)
        assert torch.equal(actions, a_ref)
        obs = [o0, o1]
    s0, s1 = stores
    for name in ("observations", "rewards", "dones", "actions", "mu", "sigma", "values"):
        assert torch.equal(getattr(s0, name), getattr(s1, name)), f"storage rows '{name}'"
    for name in s0.group_rows:
        assert torch.equal(s0.group_rows[name], s1.group_rows[name])
    assert float((s0.actions_log_prob - s1.actions_log_prob).abs().max()) <= 1e-5 * max(1.0, float(s1.actions_log_prob.abs().max()))
    with torch.no_grad():
        last = policy.evaluate(obs[0])
    for st in stores:
        st.compute_returns(last, normalize=False)
    assert torch.equal(s0.returns, s1.returns) and torch.equal(s0.advantages, s1.advantages)
    _same(stats, ref)
    assert len(ref.rewbuffer) > 0
    return envs


@pytest.mark.gpu
@pytest.mark.parametrize("trace", [True, False])
@pytest.mark.parametrize("kind", ["go2", "gait"])
def test_fused_loop_hip(hip_backend, trace, kind):
    make = (lambda: _go2(1000, trace=trace)) if kind == "go2" else (lambda: _gait(1000, trace=trace))
    groups = {"policy": ["policy"], "critic": ["policy", "critic"]} if kind == "gait" else None
    envs = _loops("cuda", make, groups)
    assert (envs[0]._trace is not None) == trace


@pytest.mark.parametrize("trace", [True, False])
def test_fused_loop_cpu(oracle_backend, trace):
    _loops("cpu", lambda: _go2(70, trace=trace), None, T=6)
