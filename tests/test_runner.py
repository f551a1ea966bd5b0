"""runner.OnPolicyRunner — rsl_rl's runner over the learner's pieces — and PPO's optimizer state in torch.optim.Adam's format.

* the optimizer state interchanges with ``torch.optim.Adam`` in both directions, and every state this Adam cannot continue from is
  refused;
* ``runner.learn`` is the hand-written loop of INTEGRATION.md §4, bit for bit (Go2, the gait env with its two-member critic group,
  with and without observation normalisers; on the GPU with the kernel's own Philox draws, for both forwards);
* a run resumed from a checkpoint by a new runner continues exactly; the files ``learn`` writes; the reference's call site;
* the inference policy; the runner's host reads are those of the hand-written loop plus its log step.

Shapes: 70 envs (no multiple of the 32-row MLP tile or of a wave), 5 steps per env, hidden dims (32, 16), 4 minibatches (350
transitions leave a remainder that is never drawn), 2 epochs."""
import copy
import json
import os
import warnings

import pytest
import torch

from test_mlp_act import _bound
from test_ppo_update import GAIT_GROUPS, _env, host_reads

N, T, HIDDEN = 70, 5, [32, 16]
ALGO = dict(class_name="PPO", clip_param=0.2, desired_kl=0.01, entropy_coef=0.01, gamma=0.99, lam=0.95, learning_rate=0.001, max_grad_norm=1.0,
            num_learning_epochs=2, num_mini_batches=4, schedule="adaptive", use_clipped_value_loss=True, value_loss_coef=1.0)
MINIBATCHES = ALGO["num_learning_epochs"] * ALGO["num_mini_batches"]
KINDS = [("go2", False), ("gait", False), ("gait", True)]   # (env, empirical_normalization)
KIND_IDS = ["go2", "gait", "gait-normalized"]


def _cfg(kind="go2", norm=False, **top):
    cfg = {"algorithm": dict(ALGO),
           "policy": {"activation": "elu", "actor_hidden_dims": list(HIDDEN), "critic_hidden_dims": list(HIDDEN), "init_noise_std": 0.8,
                      "class_name": "ActorCritic"},
           "runner": {"experiment_name": "test", "max_iterations": 3}, "runner_class_name": "OnPolicyRunner",
           "seed": 1, "num_steps_per_env": T, "save_interval": 2, "empirical_normalization": norm}
    if kind == "gait":
        cfg["obs_groups"] = {k: list(v) for k, v in GAIT_GROUPS.items()}
    cfg.update(top)
    return cfg


def _built(kind):
    env = _env(kind, N)   # (built and seeded)
    env.reset()
    return env


def _runner(env, cfg, dev, log_dir=None, forward="hip", noise_seed=None):
    from genesis_forge_amd.runner import OnPolicyRunner

    torch.manual_seed(0)   # (the policy's initial weights)
    noise = None if noise_seed is None else torch.Generator().manual_seed(noise_seed)
    return OnPolicyRunner(env, cfg, log_dir, device=dev, forward=forward, action_noise=noise)


class _Hand:
    """The loop of INTEGRATION.md §4 written out with the learner's components: what a user had to copy before the runner."""

    def __init__(self, env, cfg, dev, forward="hip", noise_seed=None):
        from genesis_forge_amd.learner import PPO, ActorCriticMLP, PolicyForward, RolloutStorage

        self.env, self.dev, self.forward = env, dev, forward
        self.noise = None if noise_seed is None else torch.Generator().manual_seed(noise_seed)
        self.store = st = RolloutStorage(env, cfg["num_steps_per_env"], obs_groups=cfg.get("obs_groups")).attach()
        widths = {m.name: int(m.observation_space.shape[0]) for m in env.managers["observation"]}
        self.critic = None if st.obs_groups["critic"] == st.obs_groups["policy"] else st.obs_groups["critic"]
        A = env.action_space.shape[0]
        torch.manual_seed(0)
        self.policy = ActorCriticMLP.from_train_cfg(cfg, widths["policy"], A, num_critic_obs=sum(widths[m] for m in st.obs_groups["critic"])).to(dev)
        self.ppo = PPO(self.policy, st, **cfg["algorithm"])
        self.fwd = PolicyForward(self.policy)
        st.seed(cfg["seed"])
        self.gen = torch.Generator(device=dev).manual_seed(cfg["seed"])
        self.losses = []

    def _cobs(self, obs, extras):
        return obs if self.critic is None else tuple(extras["observations"][m] for m in self.critic)

    def start(self):
        from genesis_forge_amd.learner import EpisodeStatistics

        self.obs, self.extras = self.env.get_observations(), self.env.extras
        self.store.begin(self.obs, self.extras)
        self.policy.train()
        self.stats = EpisodeStatistics(self.env.num_envs)

    def iterate(self):
        env, st, policy, ppo = self.env, self.store, self.policy, self.ppo
        obs, extras = self.obs, self.extras
        n, A = env.num_envs, env.action_space.shape[0]
        cat = lambda c: c if isinstance(c, torch.Tensor) else torch.cat(c, dim=-1)
        for _ in range(st.num_steps):
            noise = None if self.noise is None else torch.randn(n, A, generator=self.noise).to(self.dev)
            cobs = self._cobs(obs, extras)
            if self.forward == "hip":
                actions = st.act_policy(self.fwd, obs, cobs, noise=noise)
            else:
                with torch.no_grad():
                    mean, values = policy.act_mean(obs), policy.evaluate(cat(cobs))
                actions = st.act(mean, policy.std.detach(), values, noise=noise)
            obs, _rew, _term, trunc, extras = env.step(actions)
            policy.update_normalization(obs, self._cobs(obs, extras))
            st.process_env_step(trunc, gamma=ppo.gamma, episodes=self.stats)
        if self.forward == "hip":
            st.compute_returns(self.fwd.value(self._cobs(obs, extras)), gamma=ppo.gamma, lam=ppo.lam)
        else:
            ppo.compute_returns(cat(self._cobs(obs, extras)))
        self.losses.append(ppo.update(generator=self.gen))
        self.obs, self.extras = obs, extras

    def run(self, iterations):
        self.start()
        for _ in range(iterations):
            self.iterate()
        return self


def _state(ppo, losses):
    """What two equal runs share: parameters, both Adam moments, the normalisers' buffers, the lr and the loss means."""
    tensors = [ppo.params.clone(), ppo.exp_avg.clone(), ppo.exp_avg_sq.clone()] + [b.clone().to(torch.float32) for b in ppo.policy.buffers()]
    return tensors, ppo.learning_rate, [[l[k] for k in ("value_function", "surrogate", "entropy")] for l in losses]


def _assert_same(got, want, what, slack=None):
    """``slack=None``: bit for bit.  Otherwise (the two reference runs differed): per quantity, four times their own difference."""
    for i, (a, b) in enumerate(zip(got[0], want[0])):
        if slack is None:
            assert torch.equal(a, b), f"{what}: tensor {i} differs by {float((a - b).abs().max())}"
        else:
            assert float((a - b).abs().max()) <= 4 * slack[0][i], f"{what}: tensor {i}"
    if slack is None:
        assert got[1] == want[1], f"{what}: lr {got[1]} vs {want[1]}"
        assert got[2] == want[2], f"{what}: losses {got[2]} vs {want[2]}"
    else:
        assert abs(got[1] - want[1]) <= 4 * slack[1]
        for g, w, s in zip(sum(got[2], []), sum(want[2], []), slack[2]):
            assert abs(g - w) <= 4 * s


def _runner_vs_hand(dev, kind, norm, forward, noise_seed, measure_reference=False):
    cfg = _cfg(kind, norm)
    want = _Hand(_built(kind), cfg, dev, forward, noise_seed).run(3)
    want = _state(want.ppo, want.losses)
    slack = None
    if measure_reference:   # does the hand-written loop reproduce itself?  (torch's backward is the only part not known to)
        again = _Hand(_built(kind), cfg, dev, forward, noise_seed).run(3)
        again = _state(again.ppo, again.losses)
        diffs = ([float((a - b).abs().max()) for a, b in zip(again[0], want[0])], abs(again[1] - want[1]),
                 [abs(a - b) for a, b in zip(sum(again[2], []), sum(want[2], []))])
        print(f"    hand-written loop run to run: tensors {max(diffs[0]):.3e}, lr {diffs[1]:.3e}, losses {max(diffs[2]):.3e}")
        if max(diffs[0]) > 0 or diffs[1] > 0 or max(diffs[2]) > 0:
            slack = diffs
    runner = _runner(_built(kind), copy.deepcopy(cfg), dev, forward=forward, noise_seed=noise_seed)
    losses, log = [], runner._log
    runner._log = lambda *a, **k: (log(*a, **k), losses.append(dict(runner.last_log)))   # (last_log, once per iteration)
    runner.learn(3)
    assert [l["iteration"] for l in losses] == [0, 1, 2] and runner.current_learning_iteration == 2
    assert float(runner.alg.exp_avg.abs().max()) > 0 and runner.alg._calls == 3 * MINIBATCHES
    _assert_same(_state(runner.alg, losses), want, f"{kind} {forward}", slack)
    if norm:
        assert int(runner.alg.policy.actor_obs_normalizer.count) == 3 * T * N == int(runner.alg.policy.critic_obs_normalizer.count)
    return runner


# ---- 1. optimizer interchange ---------------------------------------------------------------------------------------------------------
def _slices(flat, params):
    out, off = [], 0
    for p in params:
        out.append(flat[off:off + p.numel()].view_as(p))
        off += p.numel()
    return out


def test_optimizer_state_interchanges_with_torch_adam(oracle_backend):
    runner = _runner(_built("go2"), _cfg(), "cpu", noise_seed=3)
    ppo = runner.alg
    fresh = ppo.optimizer_state_dict()
    assert fresh["state"] == {} and len(fresh["param_groups"]) == 1
    runner.learn(3)   # three ppo.update() calls
    sd = ppo.optimizer_state_dict()
    params = list(ppo.policy.parameters())
    twin = [p.detach().clone().requires_grad_(True) for p in params]
    opt = torch.optim.Adam(twin, lr=1.0)
    theirs = opt.state_dict()["param_groups"][0]
    assert set(sd["param_groups"][0]) == set(theirs), "the group's keys are the installed torch's"
    assert sd["param_groups"][0]["params"] == list(range(len(params)))
    opt.load_state_dict(sd)
    for p, m, v in zip(twin, _slices(ppo.exp_avg, params), _slices(ppo.exp_avg_sq, params)):
        assert torch.equal(opt.state[p]["exp_avg"], m) and torch.equal(opt.state[p]["exp_avg_sq"], v)
        assert float(opt.state[p]["step"]) == 3 * MINIBATCHES
    assert opt.param_groups[0]["lr"] == ppo.learning_rate
    assert opt.param_groups[0]["betas"] == (0.9, 0.999) and opt.param_groups[0]["eps"] == 1e-8
    # the moments are clones, and the step is the tensor torch itself writes
    sd["state"][0]["exp_avg"].add_(1.0)
    assert not torch.equal(sd["state"][0]["exp_avg"], _slices(ppo.exp_avg, params)[0])
    probe = torch.optim.Adam(twin[:1], lr=1.0)
    twin[0].grad = torch.zeros_like(twin[0])
    probe.step()
    their_step = probe.state_dict()["state"][0]["step"]
    ours = ppo.optimizer_state_dict()["state"][0]["step"]
    assert ours.dtype == their_step.dtype and ours.shape == their_step.shape == () and ours.device == their_step.device
    # its own state loads back unchanged; an empty state resets the moments and the step
    before = (ppo.exp_avg.clone(), ppo.exp_avg_sq.clone(), ppo.learning_rate, ppo._calls)
    ppo.load_optimizer_state_dict(ppo.optimizer_state_dict())
    assert torch.equal(ppo.exp_avg, before[0]) and torch.equal(ppo.exp_avg_sq, before[1]) and (ppo.learning_rate, ppo._calls) == before[2:]
    ppo.load_optimizer_state_dict(dict(fresh, param_groups=[dict(fresh["param_groups"][0], lr=0.002)]))
    assert ppo._calls == 0 and ppo.learning_rate == 0.002 and not bool(ppo.exp_avg.any()) and not bool(ppo.exp_avg_sq.any())
    assert ppo.optimizer_state_dict()["state"] == {}


def test_optimizer_state_loads_from_torch_adam_and_steps_alike(oracle_backend):
    """Three real torch.optim.Adam steps (an odd count: the control block's other slot), loaded; then one further step from both.
    Bound: the one tests/test_ppo_update.py::test_adam_step_matches_torch holds PPO's Adam step to against torch's (rtol 1e-6, atol 1e-7)."""
    ppo = _runner(_built("go2"), _cfg(algorithm=dict(ALGO, schedule="fixed")), "cpu", noise_seed=3).alg
    params = list(ppo.policy.parameters())
    ref = [p.detach().clone().requires_grad_(True) for p in params]
    opt = torch.optim.Adam(ref, lr=3e-4)
    g = torch.Generator().manual_seed(5)

    def grads():
        flat = torch.randn(ppo.params.numel(), generator=g) * 0.05
        for p, s in zip(ref, _slices(flat, ref)):
            p.grad = s.clone()
        torch.nn.utils.clip_grad_norm_(ref, ppo.max_grad_norm)
        return flat

    for _ in range(3):
        grads()
        opt.step()
    ppo.load_optimizer_state_dict(opt.state_dict())
    cat = lambda xs: torch.cat([x.detach().reshape(-1) for x in xs])
    assert torch.equal(ppo.exp_avg, cat(opt.state[p]["exp_avg"] for p in ref))
    assert torch.equal(ppo.exp_avg_sq, cat(opt.state[p]["exp_avg_sq"] for p in ref))
    assert ppo._calls == 3 and ppo.learning_rate == 3e-4
    assert float(ppo.optimizer_state_dict()["state"][0]["step"]) == 3
    with torch.no_grad():
        ppo.params.copy_(cat(ref))
    ppo.grad_sync.bucket.copy_(grads())   # (unclipped: the step clips it itself)
    opt.step()
    ppo._adam_torch()
    assert ppo._calls == 4 and ppo.learning_rate == 3e-4
    torch.testing.assert_close(ppo.params, cat(ref), rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(ppo.exp_avg, cat(opt.state[p]["exp_avg"] for p in ref), rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(ppo.exp_avg_sq, cat(opt.state[p]["exp_avg_sq"] for p in ref), rtol=1e-6, atol=1e-7)


def test_optimizer_state_refusals(oracle_backend):
    runner = _runner(_built("go2"), _cfg(), "cpu", noise_seed=3)
    ppo = runner.alg
    runner.learn(1)
    good = ppo.optimizer_state_dict()
    P = len(good["param_groups"][0]["params"])

    def group(**kw):
        sd = copy.deepcopy(good)
        sd["param_groups"][0].update(kw)
        return sd

    def fewer():
        sd = copy.deepcopy(good)
        del sd["state"][P - 1]
        sd["param_groups"][0]["params"] = list(range(P - 1))
        return sd

    def dropped_state():
        sd = copy.deepcopy(good)
        del sd["state"][P - 1]
        return sd

    def reshaped():
        sd = copy.deepcopy(good)
        sd["state"][1]["exp_avg_sq"] = sd["state"][1]["exp_avg_sq"].unsqueeze(-1)   # (a bias: [32] -> [32, 1])
        return sd

    def uneven():
        sd = copy.deepcopy(good)
        sd["state"][1]["step"] = sd["state"][1]["step"] + 1
        return sd

    before = (ppo.exp_avg.clone(), ppo.learning_rate, ppo._calls)
    for bad, word in ((fewer(), "parameters"), (dropped_state(), "parameter count"), (reshaped(), "shape"), (uneven(), "step"),
                      (group(amsgrad=True), "amsgrad"), (group(weight_decay=0.1), "weight_decay"), (group(maximize=True), "maximize"),
                      (group(betas=(0.8, 0.999)), "betas"), (group(eps=1e-6), "eps")):
        with pytest.raises(ValueError, match=word):
            ppo.load_optimizer_state_dict(bad)
    assert torch.equal(ppo.exp_avg, before[0]) and (ppo.learning_rate, ppo._calls) == before[1:], "a refused state changes nothing"
    ppo.load_optimizer_state_dict(good)


# ---- 2. runner = hand-written loop ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,norm", KINDS, ids=KIND_IDS)
def test_learn_is_the_hand_written_loop_cpu(oracle_backend, kind, norm):
    _runner_vs_hand("cpu", kind, norm, "hip", noise_seed=11)


def test_learn_with_the_torch_forward_is_the_hand_written_loop_cpu(oracle_backend):
    _runner_vs_hand("cpu", "gait", False, "torch", noise_seed=11)


def test_log_std_policy_collects_alike_with_both_forwards_cpu(oracle_backend):
    """``noise_std_type="log"``: the torch forward hands ``log_std`` to ``act`` with ``std_is_log``.  On the oracle backend ``act_policy``
    is that very ``act`` call, so the two forwards give the same bits."""
    cfg = _cfg("gait")
    cfg["policy"]["noise_std_type"] = "log"
    runs = []
    for forward in ("hip", "torch"):
        runner = _runner(_built("gait"), copy.deepcopy(cfg), "cpu", forward=forward, noise_seed=11)
        runner.learn(2)
        assert hasattr(runner.alg.policy, "log_std") and runner.alg._calls == 2 * MINIBATCHES
        runs.append(_state(runner.alg, [runner.last_log]))
    _assert_same(runs[0], runs[1], "log std")


def test_action_noise_is_required_where_the_backend_cannot_draw(oracle_backend):
    runner = _runner(_built("go2"), _cfg(), "cpu")
    with pytest.raises(RuntimeError, match="noise="):
        runner.learn(1)


# ---- 3. resume --------------------------------------------------------------------------------------------------------------------------
def _resume(dev, kind, tmp_path, noise_seed):
    """``load`` restores the policy and its normalisers, Adam's moments / step / lr, the iteration, the storage's action-noise seed and
    stream, the permutation generator's state and — where the runner draws from ``action_noise`` — that generator's state (run B's
    is another object, seeded differently)."""
    cfg = _cfg(kind, True)
    path = os.path.join(str(tmp_path), "a.pt")
    a = _runner(_built(kind), copy.deepcopy(cfg), dev, noise_seed=noise_seed)
    a.learn(2)
    a.save(path)
    a.learn(2)
    env = _built(kind)
    _runner(env, copy.deepcopy(cfg), dev, noise_seed=noise_seed).learn(2)   # (the env is where run A's was at the save; the runner is discarded)
    from genesis_forge_amd.runner import OnPolicyRunner

    torch.manual_seed(1234)
    other = None if noise_seed is None else torch.Generator().manual_seed(noise_seed + 777)
    b = OnPolicyRunner(env, dict(copy.deepcopy(cfg), seed=99), None, device=dev, action_noise=other)
    assert not torch.equal(b.alg.params, a.alg.params)
    assert b.load(path) is None
    assert b.current_learning_iteration == 1
    b.learn(2)
    _assert_same(_state(b.alg, []), _state(a.alg, []), "resumed run")
    assert b.alg._calls == a.alg._calls == 4 * MINIBATCHES
    assert b.current_learning_iteration == a.current_learning_iteration == 2
    for k in ("iteration", "value_function", "surrogate", "entropy", "learning_rate", "mean_action_std", "mean_reward", "mean_episode_length"):
        assert b.last_log[k] == a.last_log[k], k


def test_resume_is_exact_cpu(oracle_backend, tmp_path):
    _resume("cpu", "gait", tmp_path, noise_seed=21)


# ---- 4. files ---------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_files(oracle_backend, tmp_path):
    log_dir = os.path.join(str(tmp_path), "logs")
    runner = _runner(_built("go2"), _cfg(norm=True), "cpu", log_dir=log_dir, noise_seed=2)
    runner.learn(3)
    # it % 2 == 0 for it in 0, 1, 2; the final save is rsl_rl's model_{current_learning_iteration}.pt = model_2.pt again
    assert sorted(os.listdir(log_dir)) == ["model_0.pt", "model_2.pt", "progress.jsonl"]
    assert runner.current_learning_iteration == 2
    lines = [json.loads(l) for l in open(os.path.join(log_dir, "progress.jsonl"))]
    assert [l["iteration"] for l in lines] == [0, 1, 2] and lines[-1] == runner.last_log
    for l in lines:
        assert set(l) == {"iteration", "value_function", "surrogate", "entropy", "learning_rate", "mean_action_std", "mean_reward",
                          "mean_episode_length", "steps_per_second", "collection_time", "learn_time"}
        assert l["steps_per_second"] > 0 and 0 < l["mean_action_std"] < 2
    assert lines[-1]["mean_reward"] is not None and lines[-1]["mean_episode_length"] > 0, "0.4 s episodes end within 15 steps"

    path = os.path.join(log_dir, "model_2.pt")
    ck = torch.load(path, weights_only=False)
    assert list(ck) == ["model_state_dict", "optimizer_state_dict", "iter", "infos", "genesis_forge_amd"]
    assert ck["iter"] == 2 and ck["infos"] is None
    policy, ppo = runner.alg.policy, runner.alg
    assert list(ck["model_state_dict"]) == list(policy.state_dict())
    seen = set()
    for k, v in ck["model_state_dict"].items():
        assert torch.equal(v, policy.state_dict()[k]), k
        store = v.untyped_storage()
        assert store.nbytes() == v.numel() * v.element_size(), f"{k} was saved with a storage of {store.nbytes()} bytes: the flat buffer's"
        assert store.data_ptr() not in seen
        seen.add(store.data_ptr())
    assert float(ck["optimizer_state_dict"]["state"][0]["step"]) == 3 * MINIBATCHES

    # a file with rsl_rl's four keys alone loads, into a runner built from other weights
    bare = os.path.join(str(tmp_path), "bare.pt")
    torch.save({k: ck[k] for k in ("model_state_dict", "optimizer_state_dict", "iter", "infos")}, bare)
    runner.save(os.path.join(str(tmp_path), "infos.pt"), infos={"note": 7})
    other = _runner(_built("go2"), _cfg(norm=True, seed=5), "cpu", noise_seed=2)
    with torch.no_grad():
        other.alg.params.add_(0.5)
    stream = other.storage._act_stream
    assert other.load(bare) is None
    assert torch.equal(other.alg.params, ppo.params) and torch.equal(other.alg.exp_avg, ppo.exp_avg) and other.alg._calls == ppo._calls
    assert other.alg.learning_rate == ppo.learning_rate and other.current_learning_iteration == 2
    assert other.storage._act_stream == stream and other.storage._act_seed == 5, "no block: the runner's own noise state stays"
    for k, v in policy.state_dict().items():
        assert torch.equal(other.alg.policy.state_dict()[k], v), k
    lo, hi = other.alg.params.data_ptr(), other.alg.params.data_ptr() + 4 * other.alg.params.numel()
    assert all(lo <= p.data_ptr() < hi for p in other.alg.policy.parameters()), "the parameters are still views of the flat buffer"
    assert int(other.alg.policy.actor_obs_normalizer.count) == 3 * T * N
    # load_optimizer=False leaves the moments, the step and the lr alone
    third = _runner(_built("go2"), _cfg(norm=True), "cpu", noise_seed=2)
    third.learn(1)
    keep = (third.alg.exp_avg.clone(), third.alg.exp_avg_sq.clone(), third.alg._calls, third.alg.learning_rate)
    assert third.load(os.path.join(str(tmp_path), "infos.pt"), load_optimizer=False) == {"note": 7}
    assert torch.equal(third.alg.params, ppo.params)
    assert torch.equal(third.alg.exp_avg, keep[0]) and torch.equal(third.alg.exp_avg_sq, keep[1]) and (third.alg._calls, third.alg.learning_rate) == keep[2:]
    assert third.storage._act_stream == runner.storage._act_stream and third.storage._act_seed == 1, "the block's noise state"
    # a state dict that does not fit raises torch's own error
    wide = _runner(_built("go2"), dict(_cfg(norm=True), policy=dict(_cfg()["policy"], actor_hidden_dims=[48, 16])), "cpu", noise_seed=2)
    with pytest.raises(RuntimeError, match="size mismatch"):
        wide.load(bare)
    no_norm = _runner(_built("go2"), _cfg(norm=False), "cpu", noise_seed=2)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        no_norm.load(bare)


def test_learn_without_log_dir_writes_nothing(oracle_backend, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    runner = _runner(_built("go2"), _cfg(), "cpu", noise_seed=2)
    runner.learn(1)
    assert os.listdir(str(tmp_path)) == [] and runner.last_log["iteration"] == 0


# ---- 5. the reference's call site ---------------------------------------------------------------------------------------------------------
def _simple_training_cfg(exp_name, max_iterations):
    """``training_cfg()`` of the reference's examples/simple/train.py, its settings as written but for the hidden dims."""
    return {
        "algorithm": {"class_name": "PPO", "clip_param": 0.2, "desired_kl": 0.01, "entropy_coef": 0.01, "gamma": 0.99, "lam": 0.95,
                      "learning_rate": 0.001, "max_grad_norm": 1.0, "num_learning_epochs": 5, "num_mini_batches": 4, "schedule": "adaptive",
                      "use_clipped_value_loss": True, "value_loss_coef": 1.0},
        "init_member_classes": {},
        "policy": {"activation": "elu", "actor_hidden_dims": [32, 16], "critic_hidden_dims": [32, 16], "init_noise_std": 1.0, "class_name": "ActorCritic"},
        "runner": {"checkpoint": -1, "experiment_name": exp_name, "load_run": -1, "log_interval": 1, "max_iterations": max_iterations,
                   "record_interval": -1, "resume": False, "resume_path": None, "run_name": ""},
        "runner_class_name": "OnPolicyRunner",
        "seed": 1,
        "num_steps_per_env": 24,
        "save_interval": 100,
        "empirical_normalization": None,
        "obs_groups": {"policy": ["policy"], "critic": ["policy"]},
    }


def test_reference_call_site(oracle_backend, tmp_path):
    import genesis_forge_amd
    from genesis_forge_amd import gs, tasks
    from genesis_forge_amd.runner import OnPolicyRunner
    from genesis_forge_amd.wrappers import RslRlWrapper, VideoWrapper

    assert genesis_forge_amd.OnPolicyRunner is OnPolicyRunner
    log_path = os.path.join(str(tmp_path), "logs", "go2-simple")
    cfg = _simple_training_cfg("go2-simple", 1)
    env = tasks.Go2CommandDirectionEnv(num_envs=N, max_episode_length_s=0.4, cmd_resample_s=0.2, scene_kwargs=dict(ang_noise=0.3, seed=3))
    env = VideoWrapper(env, video_length_sec=12, out_dir=os.path.join(log_path, "videos"), episode_trigger=lambda episode_id: episode_id % 5 == 0)
    steps = []
    step = env.step
    env.step = lambda actions: (steps.append(1), step(actions))[1]   # (the VideoWrapper sees every step)
    env = RslRlWrapper(env)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # (the synthetic scene has no camera)
        env.build()
    env.reset()
    runner = OnPolicyRunner(env, copy.deepcopy(cfg), log_path, device=gs.device, action_noise=torch.Generator().manual_seed(0))
    runner.git_status_repos = ["."]
    runner.learn(num_learning_iterations=1, init_at_random_ep_len=False)
    assert len(steps) == 24 and runner.storage.env is env.unwrapped
    assert runner.alg._calls == 20 and runner.current_learning_iteration == 0
    assert sorted(f for f in os.listdir(log_path) if f != "videos") == ["model_0.pt", "progress.jsonl"]
    # eval.py's three lines
    runner.load(os.path.join(log_path, "model_0.pt"))
    policy = runner.get_inference_policy(device=gs.device)
    obs, _ = env.unwrapped.reset()
    with torch.no_grad():
        assert torch.equal(policy(obs), runner.alg.policy.act_mean(obs))
    assert not runner.alg.policy.training
    runner.train_mode()
    assert runner.alg.policy.training

    for missing in ("num_steps_per_env", "algorithm"):
        bad = copy.deepcopy(cfg)
        del bad[missing]
        with pytest.raises(ValueError, match=missing):
            OnPolicyRunner(env, bad, None)
    with pytest.raises(ValueError, match="fast"):
        OnPolicyRunner(env, copy.deepcopy(cfg), None, forward="fast")
    # what the policy and PPO refuse stays refused, with their messages
    with pytest.raises(ValueError, match="activation"):
        OnPolicyRunner(env, dict(copy.deepcopy(cfg), policy=dict(cfg["policy"], activation="relu")), None)
    with pytest.raises(ValueError, match="schedule"):
        OnPolicyRunner(env, dict(copy.deepcopy(cfg), algorithm=dict(cfg["algorithm"], schedule="linear")), None)


def test_init_at_random_ep_len(oracle_backend):
    env = _built("go2")
    runner = _runner(env, _cfg(), "cpu", noise_seed=2)
    assert int(env.episode_length.max()) == 0
    limit = env.max_episode_length.clone()
    runner._randomize_episode_length(env)
    length = env.episode_length
    assert length.dtype == torch.int32 and bool((length >= 0).all()) and bool((length < limit).all()) and len(set(length.tolist())) > 3
    env.max_episode_length = None   # (an env without the per-env tensor: its base value)
    runner._randomize_episode_length(env)
    assert bool((env.episode_length < env.max_episode_length_steps).all())
    env._base_max_episode_length = None
    with pytest.raises(ValueError, match="max_episode_length"):
        runner.learn(1, init_at_random_ep_len=True)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("forward", ["hip", "torch"])
@pytest.mark.parametrize("kind,norm", KINDS, ids=KIND_IDS)
def test_learn_is_the_hand_written_loop_hip(hip_backend, kind, norm, forward):
    """The kernel's own Philox draws on both sides; the hand-written loop is first run twice to see whether it reproduces itself."""
    _runner_vs_hand("cuda", kind, norm, forward, noise_seed=None, measure_reference=True)


@pytest.mark.gpu
def test_resume_is_exact_hip(hip_backend, tmp_path):
    _resume("cuda", "gait", tmp_path, noise_seed=None)


def _f64(policy, obs):
    twin = copy.deepcopy(policy).double()
    with torch.no_grad():
        return twin.act_mean(obs.double())


@pytest.mark.gpu
def test_inference_policy(hip_backend):
    from genesis_forge_amd.learner import PolicyForward

    env = _built("go2")
    runner = _runner(env, _cfg(norm=True), "cuda")
    runner.learn(1)   # (the normalisers have seen data)
    policy = runner.alg.policy
    obs, _ = env.reset()
    act = runner.get_inference_policy(device="cuda:0")
    assert not policy.training
    fwd = PolicyForward(policy)
    got = act(obs)
    assert got.shape == (N, env.action_space.shape[0]) and torch.equal(got, fwd.mean(obs))
    k = obs.shape[1] // 2
    parts = (obs[:, :k].contiguous(), obs[:, k:].contiguous())
    assert torch.equal(act(parts), fwd.mean(parts)) and torch.equal(act(parts), got)
    before = {k: v.clone() for k, v in policy.state_dict().items()}
    policy.update_normalization(obs)
    assert all(torch.equal(v, before[k]) for k, v in policy.state_dict().items()), "eval mode: the normalisers no longer update"
    ref = _f64(policy, obs)
    with torch.no_grad():
        f32 = policy.act_mean(obs)
    _bound("forward='hip'", got, f32, ref)
    # forward="torch": act_mean under no_grad, for a tensor and for segments
    slow = _runner(_built("go2"), _cfg(norm=True), "cuda", forward="torch")
    slow.alg.policy.load_state_dict(policy.state_dict())
    act_t = slow.get_inference_policy()
    out = act_t(obs)
    assert not out.requires_grad and torch.equal(out, act_t(parts))
    _bound("forward='torch'", out, f32, ref)
    with pytest.raises(ValueError, match="device"):
        runner.get_inference_policy(device="cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("forward", ["hip", "torch"])
def test_runner_adds_host_reads_only_in_its_log_step(hip_backend, forward):
    """One iteration of the hand-written loop and one of ``learn``, both after a first iteration (allocations done): the runner reads
    the device as often as the loop does, plus what its log step reads.  The loop's own count is measured, not assumed."""
    cfg = _cfg("gait", True)
    hand = _Hand(_built("gait"), cfg, "cuda", forward)
    hand.run(1)
    with host_reads() as c:
        hand.start()
        hand.iterate()
    loop_reads = c[0]
    runner = _runner(_built("gait"), copy.deepcopy(cfg), "cuda", forward=forward)
    runner.learn(1)
    in_log = [0]
    log = runner._log

    def counted_log(*a, **k):
        at = c2[0]
        log(*a, **k)
        in_log[0] += c2[0] - at

    runner._log = counted_log
    with host_reads() as c2:
        runner.learn(1)
    print(f"    forward={forward}: hand-written iteration {loop_reads} host reads, learn(1) {c2[0]} of which {in_log[0]} in the log step")
    assert loop_reads >= 1, "PPO.update returns its three means: one read"
    assert c2[0] - in_log[0] == loop_reads
    assert in_log[0] >= 2, "the log reads the lr and the action std"
