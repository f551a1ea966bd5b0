"""
rsl_rl's ``OnPolicyRunner`` over this package's learner (the call site of every ``examples/*/train.py``, ``eval.py`` and
``gamepad.py``)::

    runner = OnPolicyRunner(env, cfg, log_path, device=gs.device)
    runner.learn(num_learning_iterations=..., init_at_random_ep_len=False)   # writes model_{it}.pt
    runner.load(model); policy = runner.get_inference_policy(device=gs.device)

The runner adds no launch of its own.  It composes :class:`~.learner.RolloutStorage`, :class:`~.learner.PolicyForward`,
:class:`~.learner.EpisodeStatistics`, :class:`~.learner.ActorCriticMLP` and :class:`~.learner.PPO` in the order the ``PPO`` docstring
gives, writes rsl_rl's checkpoint files (``model_state_dict`` / ``optimizer_state_dict`` / ``iter`` / ``infos``, the optimizer state
in ``torch.optim.Adam``'s own format) and keeps one log record per iteration.

:class:`DistillationRunner` is rsl_rl's ``DistillationRunner`` in the same way: the same loop, files and arguments over
:class:`~.learner.StudentTeacherMLP`, :class:`~.learner.DistillForward` and :class:`~.learner.Distillation`, with a PPO checkpoint
as the source of its teacher.
"""
from __future__ import annotations

import json
import os
import time
from typing import Callable, Optional

import torch

from . import gs
from .learner import (ActorCriticMLP, ActorCriticRecurrent, DistillForward, Distillation, EpisodeStatistics, PolicyForward, PPO,
                      RecurrentDistillForward, RecurrentForward, RndForward, RolloutStorage, StudentTeacherMLP, StudentTeacherRecurrent, _cat,
                      _policy_std)
from .wrappers import RslRlWrapper

CHECKPOINT_VERSION = 1   # of the "genesis_forge_amd" block of a checkpoint file


class OnPolicyRunner:
    """``OnPolicyRunner(env, train_cfg, log_dir=None, device=None, *, forward="hip", action_noise=None)``.

    ``env``: a built ``ManagedEnvironment``, possibly inside ``VideoWrapper``, possibly inside ``RslRlWrapper`` (the reference's call
    site).  An outer ``RslRlWrapper`` only reformats and is stripped; the runner steps whatever is inside it, so a ``VideoWrapper``
    still sees every step.  The storage is built on ``env.unwrapped`` and attached to it.

    ``train_cfg``: the ``training_cfg()`` dict of ``examples/*/train.py`` as written.  Honoured: ``"policy"`` and
    ``"empirical_normalization"`` (``ActorCriticMLP.from_train_cfg``), ``"algorithm"`` (``PPO(**…)``), ``"num_steps_per_env"``,
    ``"save_interval"``, ``"obs_groups"`` (``RolloutStorage``; group members reach the kernels as segments, no ``torch.cat`` on the HIP
    path) and ``"seed"`` (``store.seed(seed)`` and the runner's own ``torch.Generator`` for the minibatch permutations; without it the
    storage keeps the env's seed and the generator takes ``torch.initial_seed()``).  Every other top-level key is ignored, as rsl_rl
    ignores it.  A missing ``"num_steps_per_env"`` or ``"algorithm"`` raises ``ValueError``; what ``from_train_cfg`` or ``PPO`` refuses
    stays refused, with their messages.

    ``forward``: ``"hip"`` (default) collects with ``store.act_policy(fwd, …)`` — the actor, the critic, the sampling and the rows in
    one ``gf_mlp_act`` launch — and takes the bootstrap value from ``fwd.value(…)``; ``"torch"`` collects with
    ``store.act(policy.act_mean(…), std or log_std, policy.evaluate(…), std_is_log=…)`` and ``ppo.compute_returns``.  Nothing switches
    between them by env count: the only measurements are the three sizes of profiles/r09_mlp_act.md — per collection step the HIP
    forward is 3.5 x faster than the torch forward at 4 096 envs, 1.4 x faster at 16 384 and 7 % slower at 65 536 — so the choice is
    the caller's.

    ``algorithm.rnd_cfg`` (random network distillation, ``PPO``'s docstring): ``obs_groups`` needs an ``"rnd_state"`` group; every
    collection step then runs ``alg.rnd.update_normalization(rnd_state)`` and ``store.intrinsic_reward(…, rnd_state)`` between
    ``policy.update_normalization`` and ``process_env_step`` — ``forward="hip"``: ``gf_rnd_reward`` (one launch, two with the reward
    normaliser, no host read); ``"torch"``: the module's lines (one host read per step with the reward normaliser).  The log record
    gains ``"rnd"`` (the predictor's loss), ``"mean_intrinsic_reward"`` / ``"mean_extrinsic_reward"`` (per env-step of the iteration,
    the weight included) and ``"rnd_weight"``; a checkpoint gains rsl_rl's ``"rnd_state_dict"`` / ``"rnd_optimizer_state_dict"`` and the
    module's ``update_counter`` in this package's block.  The reward normaliser's per-env discounted sums are not saved: they start
    again after a load, as rsl_rl's do.

    ``action_noise``: a CPU ``torch.Generator``; when given, each step's ``[N, A]`` standard normals are drawn from it and passed as
    ``noise=``.  Required on a backend that cannot draw (the test-only CPU oracle: ``act`` raises ``RuntimeError`` otherwise), optional on
    HIP, where the kernel's own Philox draws are the default.

    Attributes: ``alg`` (the ``PPO``; ``alg.policy``), ``current_learning_iteration``, ``log_dir``, ``git_status_repos`` (a plain list
    the reference assigns to; nothing reads it), ``last_log``.

    ``policy.class_name = "ActorCriticRecurrent"`` (rsl_rl's LSTM / GRU memory in front of the actor and the critic:
    :class:`~.learner.ActorCriticRecurrent`, ``policy.rnn_type`` / ``rnn_hidden_dim`` / ``rnn_num_layers``): ``forward="hip"`` collects
    with ``store.act_recurrent(fwd, …)`` — normaliser, cell, MLP, sampling and rows in one ``gf_mlp_recurrent_act`` launch, the hidden
    state advanced in place — and resets the memories of finished episodes without a launch (``fwd.reset(dones)``: the next launch of
    each net reads zeros there); ``"torch"`` steps the module and calls ``policy.reset(dones)``.  The bootstrap value advances the
    critic's memory once more, as rsl_rl's ``compute_returns`` does.  The update runs ``PPO``'s trajectory minibatches.  Measured
    per collection step (profiles/r26_recurrent.md, 256 units): ``"hip"`` is 3.5 x / 1.27 x / 1.10 x faster than ``"torch"`` at
    4 096 / 16 384 / 65 536 envs with an LSTM, 4.1 x / 1.54 x / 1.34 x with a GRU — the one to use at every size measured.  A checkpoint carries rsl_rl's keys (``memory_a.rnn.*``, ``memory_c.rnn.*``, …) and, in this package's block, the
    hidden states, so that a resumed run continues exactly; rsl_rl leaves them out and so does ``model_state_dict``.
    ``get_inference_policy()`` then returns a callable that keeps a hidden state of its own and has ``.reset(dones=None)``.

    Not here: multi-rank training, TensorBoard / W&B writers, video handling, and the env's own state — as with rsl_rl, a resumed run
    goes on from the env as it is."""

    def __init__(self, env, train_cfg: dict, log_dir: Optional[str] = None, device=None, *, forward: str = "hip",
                 action_noise: Optional[torch.Generator] = None):
        if forward not in ("hip", "torch"):
            raise ValueError(f"OnPolicyRunner: forward={forward!r} is not supported ('hip' or 'torch')")
        for key in ("num_steps_per_env", "algorithm"):
            if key not in train_cfg:
                raise ValueError(f"OnPolicyRunner: train_cfg has no '{key}'")
        self.env = env.env if isinstance(env, RslRlWrapper) else env   # (what is stepped)
        base = self.env.unwrapped
        self.device = torch.device(gs.device if device is None else device)
        self.forward, self.action_noise = forward, action_noise
        self.num_steps_per_env = int(train_cfg["num_steps_per_env"])
        self.save_interval = int(train_cfg.get("save_interval", 50))
        self.log_dir = log_dir
        self.git_status_repos: list = []
        self.current_learning_iteration = 0
        self.last_log: Optional[dict] = None

        groups = train_cfg.get("obs_groups")
        obs_name = "policy" if groups is None or "policy" not in groups or not groups["policy"] else groups["policy"][0]
        self.storage = store = RolloutStorage(base, self.num_steps_per_env, obs_name=obs_name, obs_groups=groups).attach()
        self._build_algorithm(train_cfg, base, store)
        self._generator = torch.Generator(device=self.device)
        seed = train_cfg.get("seed")
        if seed is None:
            self._generator.manual_seed(torch.initial_seed() & 0x7FFFFFFFFFFFFFFF)
        else:
            store.seed(int(seed))
            self._generator.manual_seed(int(seed))
        self._shared_critic = list(store.obs_groups["critic"]) == list(store.obs_groups["policy"])

    _NAME = "OnPolicyRunner"
    _INFERENCE_FORWARD = RecurrentForward   # the forward a recurrent policy's get_inference_policy() steps a state of its own with

    def _build_algorithm(self, train_cfg: dict, base, store: RolloutStorage) -> None:
        """``self.alg`` (the policy inside it) and ``self._fwd``, the one-launch forward of ``forward="hip"``."""
        width = lambda group: sum(store._widths[m] for m in store.obs_groups[group])
        name = dict(train_cfg.get("policy", {})).get("class_name", "ActorCritic")
        cls = ActorCriticRecurrent if name == "ActorCriticRecurrent" else ActorCriticMLP   # (any other name: from_train_cfg refuses it)
        policy = cls.from_train_cfg(train_cfg, width("policy"), base.action_space.shape[0], num_critic_obs=width("critic"))
        policy = policy.to(self.device)
        self.alg = PPO(policy, store, **train_cfg["algorithm"])
        self._recurrent = policy.is_recurrent
        if self._recurrent:
            self._fwd = RecurrentForward(policy) if self.forward == "hip" else None
        else:
            self._fwd = PolicyForward(policy) if self.forward == "hip" else None
        self._rnd_fwd = RndForward(self.alg.rnd) if self.forward == "hip" and self.alg.rnd is not None else None

    # -- observations ---------------------------------------------------------------------------------------------------------------
    def _group(self, names, obs: torch.Tensor, extras: dict):
        """The members of an observation group of this step: a tensor, or a tuple of segments."""
        rows = extras.get("observations", {}) if extras is not None else {}
        parts = tuple(obs if m == self.storage.obs_name else rows[m] for m in names)
        return parts[0] if len(parts) == 1 else parts

    def _inputs(self, obs: torch.Tensor, extras: dict):
        """(actor input, critic input or None where the critic reads the actor's) of this step: a tensor, or the group's members as a
        tuple of segments."""
        store = self.storage
        return (self._group(store.obs_groups["policy"], obs, extras),
                None if self._shared_critic else self._group(store.obs_groups["critic"], obs, extras))

    def _noise(self, n: int, A: int) -> Optional[torch.Tensor]:
        if self.action_noise is None:
            return None
        return torch.randn(n, A, generator=self.action_noise).to(self.device)

    # -- one iteration ----------------------------------------------------------------------------------------------------------------
    def _collect(self, obs: torch.Tensor, extras: dict, stats: EpisodeStatistics):
        """``num_steps_per_env`` steps: act -> step -> update_normalization -> process_env_step; returns the last (obs, extras)."""
        store, ppo, policy, env = self.storage, self.alg, self.alg.policy, self.env
        n, A = store.env.num_envs, ppo.num_actions
        rnd = ppo.rnd
        for _ in range(self.num_steps_per_env):
            x, cx = self._inputs(obs, extras)
            row = store._act_row()
            if self._fwd is not None and self._recurrent:
                actions = store.act_recurrent(self._fwd, x, cx, noise=self._noise(n, A))
            elif self._fwd is not None:
                actions = store.act_policy(self._fwd, x, cx, noise=self._noise(n, A))
            else:
                std, is_log = _policy_std(policy)   # (std, or log_std with std_is_log)
                if self._recurrent and row == 0:
                    store.keep_rnn_start(policy)
                with torch.no_grad():
                    mean = policy.act_mean(_cat(x))
                    values = policy.evaluate(_cat(x if cx is None else cx))
                actions = store.act(mean, std.detach(), values, noise=self._noise(n, A), std_is_log=is_log)
            obs, _rew, _terminated, truncated, extras = env.step(actions)
            x, cx = self._inputs(obs, extras)
            policy.update_normalization(x, cx)
            if rnd is not None:   # rsl_rl PPO.process_env_step: the intrinsic reward of the post-step state joins the row first
                rs = self._group(store.obs_groups["rnd_state"], obs, extras)
                rnd.update_normalization(rs)
                store.intrinsic_reward(rnd if self._rnd_fwd is None else self._rnd_fwd, rs)
            store.process_env_step(truncated, gamma=ppo.gamma, episodes=stats)
            if self._recurrent:   # rsl_rl PPO.process_env_step: policy.reset(dones)
                (policy if self._fwd is None else self._fwd).reset(store.dones[row])
        return obs, extras

    def _returns(self, obs: torch.Tensor, extras: dict) -> None:
        x, cx = self._inputs(obs, extras)
        last = x if cx is None else cx
        if self._fwd is not None:
            self.storage.compute_returns(self._fwd.value(last), gamma=self.alg.gamma, lam=self.alg.lam)
        else:
            self.alg.compute_returns(_cat(last))

    def _update(self) -> dict:
        return self.alg.update(generator=self._generator)

    def learn(self, num_learning_iterations: int, init_at_random_ep_len: bool = False) -> None:
        """rsl_rl's ``OnPolicyRunner.learn``: iterations ``current_learning_iteration … + num_learning_iterations``, each
        ``num_steps_per_env`` collection steps, the returns and ``PPO.update``.  With ``log_dir`` set, ``model_{it}.pt`` is written when
        ``it % save_interval == 0`` and once more after the loop (``model_{current_learning_iteration}.pt``, the last iteration run —
        rsl_rl's rule, so a resumed run starts at that index), and each iteration's log record is appended to ``progress.jsonl``.
        The episode statistics are fresh per call, as rsl_rl's buffers are locals of ``learn``.
        ``init_at_random_ep_len``: every env's ``episode_length`` starts at a random value below its ``max_episode_length``."""
        env, base, store = self.env, self.env.unwrapped, self.storage
        if init_at_random_ep_len:
            self._randomize_episode_length(base)
        obs = env.get_observations()
        extras = base.extras
        store.begin(obs if store.obs_name == "policy" else extras["observations"][store.obs_name], extras)
        self.train_mode()
        stats = EpisodeStatistics(base.num_envs)
        if self.log_dir is not None:
            os.makedirs(self.log_dir, exist_ok=True)
        start = self.current_learning_iteration
        for it in range(start, start + int(num_learning_iterations)):
            t0 = time.perf_counter()
            if store.rnd_sums is not None:
                store.rnd_sums.zero_()
            obs, extras = self._collect(obs, extras, stats)
            self._returns(obs, extras)
            t1 = time.perf_counter()
            losses = self._update()
            t2 = time.perf_counter()
            self.current_learning_iteration = it
            self._log(it, losses, stats, t1 - t0, t2 - t1)
            if self.log_dir is not None and it % self.save_interval == 0:
                self.save(os.path.join(self.log_dir, f"model_{it}.pt"))
        if self.log_dir is not None:
            self.save(os.path.join(self.log_dir, f"model_{self.current_learning_iteration}.pt"))

    @staticmethod
    def _randomize_episode_length(base) -> None:
        limit = getattr(base, "max_episode_length", None)
        if limit is None:
            limit = getattr(base, "max_episode_length_steps", None)
            if limit is None:
                raise ValueError("init_at_random_ep_len=True needs an env with a max_episode_length")
        length = base.episode_length
        with torch.no_grad():   # randint(0, max) per env: floor(U[0, 1) * max)
            top = (limit if isinstance(limit, torch.Tensor) else torch.full_like(length, int(limit))).to(length.dtype)
            drawn = (torch.rand(length.shape, device=length.device) * top.to(torch.float32)).to(length.dtype)
            length.copy_(torch.minimum(drawn, top - 1).clamp_(min=0))   # (the f32 product may round up to max itself)

    @staticmethod
    def _loss_record(losses: dict) -> dict:
        return {"value_function": losses["value_function"], "surrogate": losses["surrogate"], "entropy": losses["entropy"]}

    def _log(self, it: int, losses: dict, stats: EpisodeStatistics, collection_s: float, learn_s: float) -> None:
        """One record per iteration (the runner's own host reads are all here).  ``collection_time`` is the host's time to enqueue the
        rollout and ``learn_time`` ends at the update's one host read, which waits for the device: their sum is the iteration's."""
        steps = self.num_steps_per_env * self.storage.env.num_envs
        std = self.alg.policy.action_std.mean()
        curriculum = getattr(self.storage.env, "terrain_curriculum", None)
        if curriculum is None or curriculum.levels is None:
            std, level = float(std), None
        else:   # the mean terrain level rides in the read of the action std: one value more, not a read of its own
            std, level = torch.stack([std.detach().to(torch.float32), curriculum.mean_level().to(std.device)]).tolist()
        record = {"iteration": it, **self._loss_record(losses),
                  "learning_rate": self.alg.learning_rate, "mean_action_std": std,
                  "mean_reward": stats.mean_reward(), "mean_episode_length": stats.mean_episode_length(),
                  "steps_per_second": steps / max(collection_s + learn_s, 1e-9), "collection_time": collection_s, "learn_time": learn_s}
        if level is not None:      # (only for an env with a TerrainCurriculum: records without one keep their keys)
            record["Curriculum/terrain_level"] = level
        if "symmetry" in losses:   # (only with algorithm.symmetry_cfg: records without one keep their keys)
            record["symmetry"] = losses["symmetry"]
        if "rnd" in losses:        # (only with algorithm.rnd_cfg)
            extrinsic, intrinsic = self.storage.rnd_sums.sum(dim=1).tolist()
            record.update({"rnd": losses["rnd"], "mean_intrinsic_reward": intrinsic / steps, "mean_extrinsic_reward": extrinsic / steps,
                           "rnd_weight": self.alg.rnd.weight})
        self.last_log = record
        if self.log_dir is not None:
            with open(os.path.join(self.log_dir, "progress.jsonl"), "a") as f:
                f.write(json.dumps(record) + "\n")

    # -- checkpoints --------------------------------------------------------------------------------------------------------------------
    def save(self, path: str, infos=None) -> None:
        """rsl_rl's checkpoint: ``{"model_state_dict", "optimizer_state_dict", "iter", "infos"}`` — the state dict's tensors cloned (the
        parameters are views of ``PPO``'s flat buffer; the file does not carry that storage), the optimizer state in
        ``torch.optim.Adam``'s format — plus this package's own ``"genesis_forge_amd"`` block, which rsl_rl never looks at: the format
        version, the storage's action-noise seed and stream, the permutation generator's state and, where the runner draws its noise
        from ``action_noise``, that generator's state."""
        store = self.storage
        saved = {
            "model_state_dict": {k: v.detach().clone() for k, v in self.alg.policy.state_dict().items()},
            "optimizer_state_dict": self.alg.optimizer_state_dict(),
            "iter": self.current_learning_iteration,
            "infos": infos,
            "genesis_forge_amd": {"version": CHECKPOINT_VERSION, "act_seed": store._act_seed, "act_stream": store._act_stream,
                                  "generator_state": self._generator.get_state(),
                                  "action_noise_state": None if self.action_noise is None else self.action_noise.get_state()},
        }
        if getattr(self, "_recurrent", False):
            saved["genesis_forge_amd"]["hidden_states"] = self._hidden_states()
        rnd = getattr(self.alg, "rnd", None)
        if rnd is not None:   # rsl_rl's two keys, and the schedule's counter in this package's block
            saved["rnd_state_dict"] = {k: v.detach().clone() for k, v in rnd.state_dict().items()}
            saved["rnd_optimizer_state_dict"] = self.alg.rnd_optimizer_state_dict()
            saved["genesis_forge_amd"]["rnd_update_counter"] = rnd.update_counter
        torch.save(saved, path)

    def load(self, path: str, load_optimizer: bool = True):
        """rsl_rl's ``load``: the policy (copied in place, so the parameters stay views of ``PPO``'s flat buffer — checked), the optimizer
        state unless ``load_optimizer=False``, ``current_learning_iteration``, and this package's block if the file has one (a file with
        rsl_rl's four keys alone loads too).  Returns ``infos``.  A ``model_state_dict`` that does not fit raises torch's own error."""
        loaded = torch.load(path, map_location=self.device, weights_only=False)
        ppo = self.alg
        ppo.policy.load_state_dict(loaded["model_state_dict"])
        self._check_flat()
        if ppo.rnd is not None:
            if "rnd_state_dict" not in loaded:
                raise ValueError(f"{self._NAME}.load: the runner has an rnd_cfg, the checkpoint no 'rnd_state_dict'")
            ppo.rnd.load_state_dict(loaded["rnd_state_dict"])
            if load_optimizer:
                ppo.load_rnd_optimizer_state_dict(loaded["rnd_optimizer_state_dict"])
            ours = loaded.get("genesis_forge_amd") or {}
            if "rnd_update_counter" in ours:
                ppo.rnd.update_counter = int(ours["rnd_update_counter"])
                ppo.rnd.weight = ppo.rnd._scheduled_weight()
        return self._load_rest(loaded, load_optimizer)

    def _check_flat(self) -> None:
        """``load_state_dict`` copied in place: the stepped parameters are still views of the algorithm's flat buffer."""
        alg = self.alg
        lo, hi = alg.params.data_ptr(), alg.params.data_ptr() + alg.params.numel() * alg.params.element_size()
        stepped = {id(p) for p in alg.grad_sync.params}
        for name, p in alg.policy.named_parameters():
            if id(p) in stepped and not lo <= p.data_ptr() < hi:
                raise RuntimeError(f"{self._NAME}.load: parameter '{name}' no longer lives in {type(alg).__name__}'s flat buffer")

    def _load_rest(self, loaded: dict, load_optimizer: bool):
        """Everything of a checkpoint but the model: the optimizer state, the iteration and this package's block.  Returns ``infos``."""
        ppo = self.alg
        if load_optimizer:
            ppo.load_optimizer_state_dict(loaded["optimizer_state_dict"])
        self.current_learning_iteration = int(loaded["iter"])
        ours = loaded.get("genesis_forge_amd")
        if ours is not None:
            if ours.get("version") != CHECKPOINT_VERSION:
                raise ValueError(f"{self._NAME}.load: 'genesis_forge_amd' block of version {ours.get('version')!r}; this build reads {CHECKPOINT_VERSION}")
            self.storage._act_seed, self.storage._act_stream = ours["act_seed"], int(ours["act_stream"])
            self._generator.set_state(ours["generator_state"].cpu())
            if self.action_noise is not None and ours.get("action_noise_state") is not None:
                self.action_noise.set_state(ours["action_noise_state"].cpu())
            if getattr(self, "_recurrent", False) and "hidden_states" in ours:
                for m, hs in zip(self._memories(), ours["hidden_states"]):
                    to = lambda x: x.to(self.device).contiguous()
                    m.hidden_states = None if hs is None else (tuple(to(x) for x in hs) if isinstance(hs, (tuple, list)) else to(hs))
                if self._fwd is not None:
                    self._fwd._pending = dict.fromkeys(self._fwd._pending)
        return loaded.get("infos")

    _MEMORY_NAMES = (("actor", "memory_a"), ("critic", "memory_c"))   # (the forward's net name, the policy's memory) in get_hidden_states()'s order

    def _memories(self) -> tuple:
        """The policy's memory modules in ``get_hidden_states()``'s order (a net without one is left out, last)."""
        return tuple(m for m in (getattr(self.alg.policy, attr, None) for _name, attr in self._MEMORY_NAMES) if m is not None)

    def _hidden_states(self) -> tuple:
        """The memories' states as the next step will read them (copies; a pending reset of the one-launch forward applied)."""
        out = []
        for (name, _attr), hs in zip(self._MEMORY_NAMES, self.alg.policy.get_hidden_states()):
            if hs is None:
                out.append(None)
                continue
            parts = [x.detach().clone() for x in (hs if isinstance(hs, tuple) else (hs,))]
            flags = None if self._fwd is None else self._fwd._pending.get(name)
            if flags is not None:
                for x in parts:
                    x[:, flags.to(torch.bool)] = 0.0
            out.append(tuple(parts) if isinstance(hs, tuple) else parts[0])
        return tuple(out)

    # -- inference ----------------------------------------------------------------------------------------------------------------------
    def get_inference_policy(self, device=None) -> Callable:
        """``policy(obs) -> [N, A]`` in eval mode (the normalisers no longer update).  ``forward="hip"``: ``PolicyForward.mean`` — one
        launch, the normaliser applied inside; otherwise ``policy.act_mean`` under ``no_grad``.  ``obs``: a tensor or a sequence of
        segments, under ``PolicyForward``'s rules."""
        self.eval_mode()
        if device is not None and torch.device(device).type != self.device.type:   # (moving the module would take its parameters out of PPO's flat buffer)
            raise ValueError(f"get_inference_policy: the policy lives on {self.device}; device={device!r} is not supported")
        if getattr(self, "_recurrent", False):
            return _RecurrentInference(self._INFERENCE_FORWARD(self.alg.policy, own_state=True))
        if self._fwd is not None:
            return self._fwd.mean
        policy = self.alg.policy

        def act_mean(obs):
            with torch.no_grad():
                return policy.act_mean(_cat(tuple(obs) if isinstance(obs, (list, tuple)) else obs))

        return act_mean

    def train_mode(self) -> None:
        self.alg.policy.train()
        if getattr(self.alg, "rnd", None) is not None:
            self.alg.rnd.train()

    def eval_mode(self) -> None:
        self.alg.policy.eval()
        if getattr(self.alg, "rnd", None) is not None:
            self.alg.rnd.eval()


class _RecurrentInference:
    """``policy(obs) -> [N, A]`` of a recurrent policy with a hidden state of its own: an actor-only ``gf_mlp_recurrent_act`` launch
    per call (the module's torch step on a backend without it); ``reset(dones=None)`` zeroes the rows of finished episodes (``None``:
    all) before the next call."""

    def __init__(self, forward: RecurrentForward):
        self._fwd = forward

    def __call__(self, obs):
        return self._fwd.mean(tuple(obs) if isinstance(obs, (list, tuple)) else obs)

    def reset(self, dones=None) -> None:
        self._fwd.reset(None if dones is None else dones.reshape(-1).to(torch.bool).clone())   # (a copy: the caller's tensor may change before the next call)


class DistillationRunner(OnPolicyRunner):
    """``DistillationRunner(env, train_cfg, log_dir=None, device=None, *, forward="hip", action_noise=None)`` — rsl_rl's
    ``DistillationRunner``: :class:`OnPolicyRunner`'s loop, files and arguments over a :class:`~.learner.StudentTeacherMLP` and
    :class:`~.learner.Distillation`.

    ``train_cfg["obs_groups"]`` must have ``"policy"`` (the student's input — the deployable observations) and ``"teacher"`` (the
    privileged ones); ``"policy"`` is read by ``StudentTeacherMLP.from_train_cfg``, ``"algorithm"`` by ``Distillation(**…)``.

    ``learn`` needs a teacher: ``load(path)`` of a PPO checkpoint (an ``OnPolicyRunner``'s ``model_*.pt``) takes its actor — and the
    actor's normaliser — as the teacher and nothing else: not the optimizer, not the iteration counter, not the noise state.  A
    distillation checkpoint is a full resume.  Per iteration: ``num_steps_per_env`` steps of ``store.act_distill`` (ONE
    ``gf_mlp_distill_act`` launch for the student, the teacher, the sampling and the two rows; ``forward="torch"``: the two torch
    forwards and ``gf_policy_act``) → ``env.step`` → ``policy.update_normalization`` → ``store.process_env_step(None, episodes=…)``,
    then ``Distillation.update()``.  The log record carries ``"behavior"`` in place of the three PPO losses.
    ``get_inference_policy()`` is the student's mean.

    ``policy.class_name = "StudentTeacherRecurrent"`` (:class:`~.learner.StudentTeacherRecurrent`: ``policy.rnn_type`` /
    ``rnn_hidden_dim`` / ``rnn_num_layers`` / ``teacher_recurrent``; a recurrent PPO checkpoint as the teacher needs
    ``teacher_recurrent=True``): ``forward="hip"`` collects with ``store.act_distill_recurrent`` — ONE
    ``gf_mlp_recurrent_distill_act`` launch — and resets the memories of finished episodes without a launch (``fwd.reset(dones)``);
    ``"torch"`` steps the module and calls ``policy.reset(dones)``.  ``Distillation.update()`` then trains the student and its memory
    by truncated back-propagation through time.  A checkpoint carries both hidden states in this package's block, so a resumed run
    continues exactly; ``get_inference_policy()`` returns a callable with a hidden state of its own and ``.reset(dones=None)``."""

    _NAME = "DistillationRunner"

    def _build_algorithm(self, train_cfg: dict, base, store: RolloutStorage) -> None:
        if "teacher" not in store.obs_groups or not store.obs_groups["teacher"]:
            raise ValueError("DistillationRunner: train_cfg['obs_groups'] needs a 'teacher' group (the teacher's privileged observations)")
        width = lambda group: sum(store._widths[m] for m in store.obs_groups[group])
        name = dict(train_cfg.get("policy", {})).get("class_name", "StudentTeacher")
        cls = StudentTeacherRecurrent if name == "StudentTeacherRecurrent" else StudentTeacherMLP   # (any other name: from_train_cfg refuses it)
        policy = cls.from_train_cfg(train_cfg, width("policy"), width("teacher"), base.action_space.shape[0]).to(self.device)
        self.alg = Distillation(policy, store, **train_cfg["algorithm"])
        self._recurrent = bool(getattr(policy, "is_recurrent", False))
        if self.forward != "hip":
            self._fwd = None
        else:
            self._fwd = RecurrentDistillForward(policy) if self._recurrent else DistillForward(policy)

    _MEMORY_NAMES = (("student", "memory_s"), ("teacher", "memory_t"))
    _INFERENCE_FORWARD = RecurrentDistillForward

    def _collect(self, obs: torch.Tensor, extras: dict, stats: EpisodeStatistics):
        store, policy, env = self.storage, self.alg.policy, self.env
        n, A = store.env.num_envs, self.alg.num_actions
        groups = store.obs_groups
        for _ in range(self.num_steps_per_env):
            x, tx = self._group(groups["policy"], obs, extras), self._group(groups["teacher"], obs, extras)
            row = store._act_row()
            if self._fwd is not None and self._recurrent:
                actions = store.act_distill_recurrent(self._fwd, x, tx, noise=self._noise(n, A))
            elif self._fwd is not None:
                actions = store.act_distill(self._fwd, x, tx, noise=self._noise(n, A))
            else:
                std, is_log = _policy_std(policy)
                if self._recurrent and row == 0:
                    store.keep_distill_rnn_start(policy)
                with torch.no_grad():
                    mean, teacher = policy.act_mean(_cat(x)), policy.evaluate(_cat(tx))
                actions = store._act_distill_rows(mean, std.detach(), teacher, noise=self._noise(n, A), std_is_log=is_log)
            obs, _rew, _terminated, _truncated, extras = env.step(actions)
            policy.update_normalization(self._group(groups["policy"], obs, extras))
            store.process_env_step(None, episodes=stats)
            if self._recurrent:   # rsl_rl Distillation.process_env_step: policy.reset(dones)
                (policy if self._fwd is None else self._fwd).reset(store.dones[row])
        return obs, extras

    def _returns(self, obs: torch.Tensor, extras: dict) -> None:
        pass   # (no critic, no returns)

    def _update(self) -> dict:
        return self.alg.update()

    @staticmethod
    def _loss_record(losses: dict) -> dict:
        return {"behavior": losses["behavior"]}

    def learn(self, num_learning_iterations: int, init_at_random_ep_len: bool = False) -> None:
        if not self.alg.policy.loaded_teacher:
            raise ValueError("DistillationRunner.learn: no teacher is loaded — load() a PPO checkpoint (its actor becomes the teacher) "
                             "or a distillation checkpoint first")
        super().learn(num_learning_iterations, init_at_random_ep_len)

    def load(self, path: str, load_optimizer: bool = True):
        """A PPO checkpoint: the teacher (and its normaliser) only — ``StudentTeacherMLP.load_state_dict`` returned ``False``; the
        optimizer state, the iteration counter and this package's block are not taken.  A distillation checkpoint: everything, as
        ``OnPolicyRunner.load``.  Returns ``infos``."""
        loaded = torch.load(path, map_location=self.device, weights_only=False)
        resumed = self.alg.policy.load_state_dict(loaded["model_state_dict"])
        self._check_flat()
        if not resumed:
            return loaded.get("infos")
        return self._load_rest(loaded, load_optimizer)
