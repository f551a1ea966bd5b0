#!/usr/bin/env python3
"""One PPO collection step (Go2 ``go2_cmd``) with the actor and critic forward passes, in three forms:

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
    python tools/bench_collect.py [--sizes 4096,16384,65536] [--forms rsl_rl,fused,fused_mlp] [--steps 240] [--warmup 48] [--reps 5] [--normalize]"""
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
from genesis_forge_amd.learner import ActorCriticMLP, EpisodeStatistics, PolicyForward, RolloutStorage

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


def run(n: int, form: str, steps: int, warmup: int, reps: int, normalize: bool = False) -> dict:
    env = tasks.bench_env(n)
    env.build()
    env.seed(1234)
    obs, extras = env.reset()
    A = env.action_space.shape[0]
    store = RolloutStorage(env, T).attach()
    store.begin(obs, extras)
    torch.manual_seed(0)
    fused_norm = normalize and form != "rsl_rl"
    policy = ActorCriticMLP(store.obs_width, A, actor_obs_normalization=fused_norm, critic_obs_normalization=fused_norm).to(gs.device)
    gamma = 0.99
    if form == "fused":
        stats = EpisodeStatistics(n)

        def step(obs):
            actions = store.act(policy.act_mean(obs), policy.std, policy.evaluate(obs))
            obs, _rew, _term, trunc, _ = env.step(actions)
            if normalize:
                policy.update_normalization(obs)
            store.process_env_step(trunc, gamma=gamma, episodes=stats)
            return obs
    elif form == "fused_mlp":
        stats = EpisodeStatistics(n)
        fwd = PolicyForward(policy)

        def step(obs):
            actions = store.act_policy(fwd, obs)
            obs, _rew, _term, trunc, _ = env.step(actions)
            if normalize:
                policy.update_normalization(obs)
            store.process_env_step(trunc, gamma=gamma, episodes=stats)
            return obs
    else:
        cur_reward_sum = torch.zeros(n, device=gs.device)
        cur_episode_length = torch.zeros(n, device=gs.device)
        rewbuffer, lenbuffer = deque(maxlen=100), deque(maxlen=100)
        actor_norm = RslRlNormalizer(store.obs_width).to(gs.device) if normalize else (lambda x: x)
        critic_norm = RslRlNormalizer(store.obs_width).to(gs.device) if normalize else (lambda x: x)

        def step(obs):
            mean, values = policy.act_mean(actor_norm(obs)), policy.evaluate(critic_norm(obs))
            dist = torch.distributions.Normal(mean, policy.std.expand_as(mean))   # rsl_rl ActorCritic.update_distribution
            actions = dist.sample()
            log_prob = dist.log_prob(actions).sum(dim=-1)
            obs, rew, term, trunc, _ = env.step(actions)
            if normalize:   # rsl_rl PPO.process_env_step: policy.update_normalization(obs)
                actor_norm.update(obs)
                critic_norm.update(obs)
            store.add_policy(actions, values, log_prob, dist.mean, dist.stddev, time_outs=trunc, gamma=gamma)
            dones = term | trunc
            cur_reward_sum.add_(rew)   # OnPolicyRunner.learn
            cur_episode_length.add_(1)
            new_ids = (dones > 0).nonzero(as_tuple=False)
            rewbuffer.extend(cur_reward_sum[new_ids][:, 0].cpu().numpy().tolist())
            lenbuffer.extend(cur_episode_length[new_ids][:, 0].cpu().numpy().tolist())
            cur_reward_sum[new_ids] = 0
            cur_episode_length[new_ids] = 0
            return obs

    times = []
    with torch.no_grad():
        for _ in range(warmup):
            obs = step(obs)
        torch.cuda.synchronize()
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(steps):
                obs = step(obs)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / steps * 1e6)
    out = {"tool": "bench_collect", "config": "go2_cmd", "num_envs": n, "form": form, "normalize": normalize, "steps": steps, "warmup": warmup, "reps": reps,
           "us_per_step_best": round(min(times), 2), "us_per_step_median": round(statistics.median(times), 2),
           "recorded_step": env._trace is not None}
    if form in ("fused", "fused_mlp"):
        out["mean_reward"] = stats.mean_reward()
    else:
        out["mean_reward"] = statistics.mean(rewbuffer) if rewbuffer else None
    store.detach()
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default="4096,16384,65536")
    ap.add_argument("--forms", default="rsl_rl,fused")
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--warmup", type=int, default=48)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--normalize", action="store_true", help="empirical observation normalisation on the actor and the critic")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_collect.py times the collection loop on a ROCm GPU: no device visible")
    gs.set_device("cuda:0")
    for n in (int(x) for x in a.sizes.split(",")):
        for form in a.forms.split(","):
            if form not in ("rsl_rl", "fused", "fused_mlp"):
                raise SystemExit(f"unknown form {form!r}")
            print(json.dumps(run(n, form, a.steps, a.warmup, a.reps, a.normalize)), flush=True)


if __name__ == "__main__":
    main()
