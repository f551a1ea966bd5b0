#!/usr/bin/env python3
"""One PPO collection step (Go2 ``go2_cmd``, or ``--config gait``) with the actor and critic forward passes, in three forms:

* ``rsl_rl``: rsl_rl's PPO.act (torch ``Normal``: sample, log_prob(...).sum(-1), mean, stddev), env.step, ``add_policy(...,
  time_outs=…)``, then OnPolicyRunner.learn's episode bookkeeping verbatim — ``nonzero()`` and two ``.cpu()`` copies per step;
* ``fused``: ``RolloutStorage.act`` → env.step → ``process_env_step(episodes=…)`` (one gf_policy_act and one gf_episode_step launch
  around the step, no host synchronisation);
* ``fused_mlp``: ``RolloutStorage.act_policy(PolicyForward(policy), obs)`` → env.step → ``process_env_step(episodes=…)``: the two forward
  passes and the sampling are one gf_mlp_act launch (not in the default ``--forms``).

Prints one JSON line per (num_envs, form): µs per step (best and median of --reps batches of --steps steps, each batch ending in a
device synchronise).  HipBackend keeps no launch counter: count the kernels of a step in a separate run,
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_collect.py --sizes 4096 --forms fused --steps 100 --warmup 24 --reps 1
and divide the kernel count by the steps run (warm-up + timed).
``--normalize``: the policy carries rsl_rl's empirical observation normalisers (actor and critic) and every step updates them after
env.step(), where rsl_rl's process_env_step does: the ``rsl_rl`` form runs rsl_rl's normaliser lines in torch (tests/rsl_rl_norm.py
is the same class) around its forward, ``fused`` normalises through ``policy.act_mean`` / ``evaluate`` and updates both normalisers
with one gf_obs_norm_update, ``fused_mlp`` normalises inside the gf_mlp_act launch as well.
``--config gait``: the gait trainer (history_len 5, policy and critic managers, the asymmetric critic's ``obs_groups``).
``--history frames``: ``RolloutStorage(history="frames")`` — a history observation is stored once per frame (one gf_rollout_frame_write
launch behind the step's own); ``--output window``: the ObservationManagers hand out strided history windows (``frames`` only).
``--rnd``: random network distillation on top (``rnd_state`` = the policy observation, a 256-128 predictor and target with 16 outputs,
both normalisers on): after env.step() every form updates the state normaliser and adds the intrinsic reward to the storage row —
``rsl_rl`` with the module's torch lines (``RandomNetworkDistillation.get_intrinsic_reward``: one host read per step), ``fused`` /
``fused_mlp`` with ``RolloutStorage.intrinsic_reward(RndForward(rnd), …)`` (gf_rnd_reward) — and one more line per size times the RND
step ALONE in both forms, alternated in one process (``"form": "rnd_hip"`` / ``"rnd_torch"``).
``--policy recurrent [--rnn-type lstm|gru] [--rnn-hidden-dim 256]``: an ``ActorCriticRecurrent`` policy; per size three loops in ONE
process, their batches alternated: ``recurrent_hip`` (``RolloutStorage.act_recurrent``: normaliser, cell, MLP, sampling and rows in one
gf_mlp_recurrent_act launch, ``RecurrentForward.reset(dones)`` without a launch), ``recurrent_torch`` (the module's step, ``act`` and
``policy.reset(dones)``) and ``mlp_hip`` (the ``fused_mlp`` loop of the MLP policy), one JSON line each.
``collector()`` builds one such loop and times batches of it, for scripts that alternate several forms in one process.
    python tools/bench_collect.py [--sizes 4096,16384,65536] [--forms rsl_rl,fused,fused_mlp] [--steps 240] [--warmup 48] [--reps 5] [--normalize] [--noise-std-type scalar|log]
                                  [--config go2_cmd|gait] [--history rows|frames] [--output fresh|window] [--rnd]
                                  [--policy mlp|recurrent] [--rnn-type lstm|gru] [--rnn-hidden-dim 256]"""
import argparse
import json
import os
import statistics
import sys
import time
from collections import deque

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genesis-forge_amd"))
import torch
from genesis_forge_amd import gs, tasks
from genesis_forge_amd.learner import (ActorCriticMLP, ActorCriticRecurrent, EpisodeStatistics, RecurrentForward, PolicyForward, RandomNetworkDistillation, RndForward, RolloutStorage,
                                       _rnd_reward_torch)
from genesis_forge_amd.managers import ObservationManager

T = 24   # num_steps_per_env of examples/simple/train.py
torch.distributions.Normal.set_default_validate_args(False)   # as rsl_rl's ActorCritic.__init__ does (no per-step support checks)


class RslRlNormalizer(torch.nn.Module):
    """rsl_rl's EmpiricalNormalization, its lines in torch (the ``rsl_rl`` form of --normalize)."""

    def __init__(self, width: int, eps: float = 1e-2):
        super().__init__()
        self.eps = eps
        self.register_buffer("_mean", torch.zeros(width).unsqueeze(0))
        self.register_buffer("_var", torch.ones(width).unsqueeze(0))
        self.register_buffer("_std", torch.ones(width).unsqueeze(0))
        self.register_buffer("count", torch.tensor(0, dtype=torch.long))

    def forward(self, x):
        return (x - self._mean) / (self._std + self.eps)

    def update(self, x):
        count_x = x.shape[0]
        self.count += count_x
        rate = count_x / self.count
        var_x = torch.var(x, dim=0, unbiased=False, keepdim=True)
        mean_x = torch.mean(x, dim=0, keepdim=True)
        delta_mean = mean_x - self._mean
        self._mean += rate * delta_mean
        self._var += rate * (var_x - self._var + delta_mean * (mean_x - self._mean))
        self._std = torch.sqrt(self._var)


GAIT_GROUPS = {"policy": ["policy"], "critic": ["policy", "critic"]}   # obs_groups of examples/gait_trainer/train.py
RND_KWARGS = dict(num_outputs=16, predictor_hidden_dims=[256, 128], target_hidden_dims=[256, 128], weight=0.1, state_normalization=True,
                  reward_normalization=True)


def make_rnd(width: int) -> RandomNetworkDistillation:
    torch.manual_seed(1)
    return RandomNetworkDistillation(width, **RND_KWARGS).to(gs.device)


class collector:
    """One collection loop: ``batch(steps)`` runs ``steps`` of it and returns µs per step (ending in a device synchronise)."""

    def __init__(self, n: int, form: str, normalize: bool = False, config: str = "go2_cmd", history: str = "rows", output: str = "fresh",
                 noise_std_type: str = "scalar", rnd: bool = False, rnn_type: str = "lstm", rnn_hidden_dim: int = 256):
        old, ObservationManager.default_output = ObservationManager.default_output, output
        try:   # (the managers are created by env.config(), i.e. inside build())
            env = tasks.BASELINE_CONFIGS[config][1](n)
            env.build()
        finally:
            ObservationManager.default_output = old
        env.seed(1234)
        self.env, self.form, self.state = env, form, env.reset()
        groups = dict(GAIT_GROUPS) if config == "gait" else ({"policy": ["policy"], "critic": ["policy"]} if rnd else None)
        if rnd:
            groups["rnd_state"] = ["policy"]
        self.store = RolloutStorage(env, T, obs_groups=groups, history=history).attach()
        self.store.begin(*self.state)
        if form.startswith("recurrent"):
            self.step, self.stats, self.rewbuffer = _make_recurrent_step(env, self.store, form, normalize, rnn_type, rnn_hidden_dim)
        else:
            self.step, self.stats, self.rewbuffer = _make_step(env, self.store, form, normalize, noise_std_type, rnd)

    def batch(self, steps: int) -> float:
        obs, extras = self.state
        with torch.no_grad():
            t0 = time.perf_counter()
            for _ in range(steps):
                obs, extras = self.step(obs, extras)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        self.state = (obs, extras)
        return dt / steps * 1e6

    def mean_reward(self):
        if self.stats is not None:
            return self.stats.mean_reward()
        return statistics.mean(self.rewbuffer) if self.rewbuffer else None


def _make_step(env, store, form: str, normalize: bool, noise_std_type: str = "scalar", rnd: bool = False):
    n, A = env.num_envs, env.action_space.shape[0]
    if rnd:   # rsl_rl PPO.process_env_step's RND lines, between the step and the bootstrap
        module = make_rnd(store.obs_width)
        reward_with = module if form == "rsl_rl" else RndForward(module)

        def rnd_lines(obs):
            module.update_normalization(obs)
            store.intrinsic_reward(reward_with, obs)
    else:
        rnd_lines = lambda obs: None
    width = {m.name: int(m.observation_space.shape[0]) for m in env.managers["observation"]}
    critic = store.obs_groups["critic"]
    same = critic == store.obs_groups["policy"]
    critic_w = sum(width[m] for m in critic)
    parts = (lambda obs, extras: obs) if same else (lambda obs, extras: tuple(extras["observations"][m] for m in critic))
    cat = (lambda obs, extras: obs) if same else (lambda obs, extras: torch.cat([extras["observations"][m] for m in critic], dim=-1))
    torch.manual_seed(0)
    fused_norm = normalize and form != "rsl_rl"
    policy = ActorCriticMLP(store.obs_width, A, num_critic_obs=critic_w, actor_obs_normalization=fused_norm,
                            critic_obs_normalization=fused_norm, noise_std_type=noise_std_type).to(gs.device)
    is_log = noise_std_type == "log"
    std_param = policy.log_std if is_log else policy.std
    gamma = 0.99
    stats, rewbuffer = None, None
    if form == "fused":
        stats = EpisodeStatistics(n)

        def step(obs, extras):
            actions = store.act(policy.act_mean(obs), std_param, policy.evaluate(cat(obs, extras)), std_is_log=is_log)
            obs, _rew, _term, trunc, extras = env.step(actions)
            if normalize:
                policy.update_normalization(obs, parts(obs, extras))
            rnd_lines(obs)
            store.process_env_step(trunc, gamma=gamma, episodes=stats)
            return obs, extras
    elif form == "fused_mlp":
        stats = EpisodeStatistics(n)
        fwd = PolicyForward(policy)

        def step(obs, extras):
            actions = store.act_policy(fwd, obs, critic_obs=parts(obs, extras))
            obs, _rew, _term, trunc, extras = env.step(actions)
            if normalize:
                policy.update_normalization(obs, parts(obs, extras))
            rnd_lines(obs)
            store.process_env_step(trunc, gamma=gamma, episodes=stats)
            return obs, extras
    else:
        cur_reward_sum = torch.zeros(n, device=gs.device)
        cur_episode_length = torch.zeros(n, device=gs.device)
        rewbuffer, lenbuffer = deque(maxlen=100), deque(maxlen=100)
        actor_norm = RslRlNormalizer(store.obs_width).to(gs.device) if normalize else (lambda x: x)
        critic_norm = RslRlNormalizer(critic_w).to(gs.device) if normalize else (lambda x: x)

        def step(obs, extras):
            mean, values = policy.act_mean(actor_norm(obs)), policy.evaluate(critic_norm(cat(obs, extras)))
            std = torch.exp(std_param) if is_log else std_param
            dist = torch.distributions.Normal(mean, std.expand_as(mean))   # rsl_rl ActorCritic.update_distribution
            actions = dist.sample()
            log_prob = dist.log_prob(actions).sum(dim=-1)
            obs, rew, term, trunc, extras = env.step(actions)
            if normalize:   # rsl_rl PPO.process_env_step: policy.update_normalization(obs)
                actor_norm.update(obs)
                critic_norm.update(cat(obs, extras))
            rnd_lines(obs)
            store.add_policy(actions, values, log_prob, dist.mean, dist.stddev, time_outs=trunc, gamma=gamma)
            dones = term | trunc
            cur_reward_sum.add_(rew)   # OnPolicyRunner.learn
            cur_episode_length.add_(1)
            new_ids = (dones > 0).nonzero(as_tuple=False)
            rewbuffer.extend(cur_reward_sum[new_ids][:, 0].cpu().numpy().tolist())
            lenbuffer.extend(cur_episode_length[new_ids][:, 0].cpu().numpy().tolist())
            cur_reward_sum[new_ids] = 0
            cur_episode_length[new_ids] = 0
            return obs, extras

    return step, stats, rewbuffer


def _make_recurrent_step(env, store, form: str, normalize: bool, rnn_type: str, hidden: int):
    """``recurrent_hip`` / ``recurrent_torch``: one collection step of an ActorCriticRecurrent policy (the critic reads the policy group)."""
    n, A = env.num_envs, env.action_space.shape[0]
    torch.manual_seed(0)
    policy = ActorCriticRecurrent(store.obs_width, A, actor_obs_normalization=normalize, critic_obs_normalization=normalize,
                                  rnn_type=rnn_type, rnn_hidden_dim=hidden).to(gs.device)
    stats, gamma = EpisodeStatistics(n), 0.99
    if form == "recurrent_hip":
        fwd = RecurrentForward(policy)

        def step(obs, extras):
            row = store._act_row()
            actions = store.act_recurrent(fwd, obs)
            obs, _rew, _term, trunc, extras = env.step(actions)
            if normalize:
                policy.update_normalization(obs)
            store.process_env_step(trunc, gamma=gamma, episodes=stats)
            fwd.reset(store.dones[row])
            return obs, extras
    else:

        def step(obs, extras):
            row = store._act_row()
            actions = store.act(policy.act_mean(obs), policy.std, policy.evaluate(obs))
            obs, _rew, _term, trunc, extras = env.step(actions)
            if normalize:
                policy.update_normalization(obs)
            store.process_env_step(trunc, gamma=gamma, episodes=stats)
            policy.reset(store.dones[row])
            return obs, extras

    return step, stats, None


def run_recurrent(n: int, steps: int, warmup: int, reps: int, normalize: bool, rnn_type: str, hidden: int) -> list:
    """The three loops of ``--policy recurrent`` in one process, batches alternated."""
    forms = ("recurrent_hip", "recurrent_torch", "mlp_hip")
    cs = {f: collector(n, "fused_mlp" if f == "mlp_hip" else f, normalize, rnn_type=rnn_type, rnn_hidden_dim=hidden) for f in forms}
    for c in cs.values():
        c.batch(warmup)
    times = {f: [] for f in forms}
    for _ in range(reps):
        for f in forms:
            times[f].append(cs[f].batch(steps))
    out = [{"tool": "bench_collect", "policy": "recurrent", "rnn_type": rnn_type, "rnn_hidden_dim": hidden, "num_envs": n, "form": f,
            "normalize": normalize, "steps": steps, "warmup": warmup, "reps": reps, "us_per_step_best": round(min(t), 2),
            "us_per_step_median": round(statistics.median(t), 2), "us_per_step_all": [round(x, 2) for x in t]} for f, t in times.items()]
    for c in cs.values():
        c.store.detach()
    return out


def run(n: int, form: str, steps: int, warmup: int, reps: int, normalize: bool = False, config: str = "go2_cmd", history: str = "rows",
        output: str = "fresh", noise_std_type: str = "scalar", rnd: bool = False) -> dict:
    c = collector(n, form, normalize, config, history, output, noise_std_type, rnd)
    if warmup:
        c.batch(warmup)
    times = [c.batch(steps) for _ in range(reps)]
    out = {"tool": "bench_collect", "config": config, "history": history, "output": output, "num_envs": n, "form": form, "normalize": normalize,
           "noise_std_type": noise_std_type, "rnd": rnd,
           "steps": steps, "warmup": warmup, "reps": reps,
           "us_per_step_best": round(min(times), 2), "us_per_step_median": round(statistics.median(times), 2),
           "recorded_step": c.env._trace is not None, "mean_reward": c.mean_reward()}
    c.store.detach()
    return out


def run_rnd_alone(n: int, steps: int, warmup: int, reps: int, width: int = 48) -> list:
    """The RND step alone — the state normaliser's update, the intrinsic reward, the row's add and the two accumulators — on fixed
    random rnd_state rows: ``rnd_hip`` (gf_obs_norm_update + gf_rnd_reward) and ``rnd_torch`` (the module's lines) on copies of one
    module, batches alternated."""
    import copy

    base = make_rnd(width)
    modules = {"rnd_hip": base, "rnd_torch": copy.deepcopy(base)}
    fwd = RndForward(base)
    x = torch.randn(n, width, device=gs.device)
    rows = {k: torch.zeros(n, device=gs.device) for k in modules}
    acc = {k: torch.zeros(2, n, device=gs.device, dtype=torch.float64) for k in modules}

    def batch(form: str, k: int) -> float:
        m, r, a = modules[form], rows[form], acc[form]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            m.update_normalization(x)
            if form == "rnd_hip":
                fwd.reward(x, r, a[0], a[1])
            else:
                _rnd_reward_torch(m, x, r, a[0], a[1])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e6

    times = {k: [] for k in modules}
    for form in modules:
        batch(form, warmup)
    for _ in range(reps):
        for form in modules:
            times[form].append(batch(form, steps))
    return [{"tool": "bench_collect", "num_envs": n, "form": form, "rnd_state_width": width, "steps": steps, "warmup": warmup, "reps": reps,
             "us_per_step_best": round(min(t), 2), "us_per_step_median": round(statistics.median(t), 2)} for form, t in times.items()]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="4096,16384,65536")
    ap.add_argument("--forms", default="rsl_rl,fused")
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=48)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--normalize", action="store_true", help="empirical observation normalisation on the actor and the critic")
    ap.add_argument("--config", default="go2_cmd", choices=["go2_cmd", "gait"], help="the task: bench.py's Go2 config or the gait trainer")
    ap.add_argument("--history", default="rows", choices=["rows", "frames"], help="RolloutStorage(history=): rows, or one entry per frame")
    ap.add_argument("--output", default="fresh", choices=["fresh", "window"], help="what the ObservationManagers hand out")
    ap.add_argument("--noise-std-type", default="scalar", choices=["scalar", "log"], help="the policy's std parameter: std, or log_std")
    ap.add_argument("--rnd", action="store_true", help="random network distillation: the intrinsic reward joins every step; the RND step alone is timed too")
    ap.add_argument("--policy", default="mlp", choices=["mlp", "recurrent"], help="recurrent: the one-launch recurrent step against the module's torch step and the MLP policy's loop")
    ap.add_argument("--rnn-type", default="lstm", choices=["lstm", "gru"])
    ap.add_argument("--rnn-hidden-dim", type=int, default=256)
    a = ap.parse_args()
    if a.output == "window" and a.history != "frames":
        raise SystemExit("--output window needs --history frames: a row storage copies contiguous observation rows")
    if not torch.cuda.is_available():
        raise SystemExit("bench_collect.py times the collection loop on a ROCm GPU: no device visible")
    gs.set_device("cuda:0")
    for n in (int(x) for x in a.sizes.split(",")):
        if a.policy == "recurrent":
            for line in run_recurrent(n, a.steps, a.warmup, a.reps, a.normalize, a.rnn_type, a.rnn_hidden_dim):
                print(json.dumps(line), flush=True)
            continue
        for form in a.forms.split(","):
            if form not in ("rsl_rl", "fused", "fused_mlp"):
                raise SystemExit(f"unknown form {form!r}")
            print(json.dumps(run(n, form, a.steps, a.warmup, a.reps, a.normalize, a.config, a.history, a.output, a.noise_std_type, a.rnd)), flush=True)
        if a.rnd:
            for line in run_rnd_alone(n, a.steps, a.warmup, a.reps):
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
