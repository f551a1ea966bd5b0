"""
The RL-library side of a step (first slice): what rsl_rl's OnPolicyRunner does with a step's outputs and
with the policy gradients (call site examples/simple/train.py:125-129; policy config :37-79).  rsl_rl itself is a third-party
dependency and stays one; this module provides the two pieces of it that touch the hot path's data and the xGMI links:

* :class:`RolloutStorage` — time-major ``observations [T+1, N, W]``, ``rewards [T, N]``, ``dones [T, N]``.  rsl_rl fills its
  storage with three ``copy_`` launches per step; attached to a ``ManagedEnvironment`` the step's own kernel stores the three
  rows (``gf_rollout_write`` phase by phase, the fused post-physics launch writes them from the tile it holds) — no extra
  launch, no re-read of the observation.
  The policy's half of a transition (actions, value, log-probability, action mean / std — five more ``copy_`` launches in rsl_rl's
  ``add_transitions``, after ``rewards += gamma * values * time_outs``) is one ``gf_rollout_policy_write`` launch
  (``add_policy``), and the end-of-rollout return computation (rsl_rl ``compute_returns``: a backwards loop of eight
  elementwise launches per step, then the advantage normalisation) is ``gf_gae`` (``compute_returns``): one lane per env
  walks its T steps, rows are coalesced, the recurrence is the torch loop's arithmetic operation for operation.
  ``history="frames"`` keeps a history observation (``history_len`` = H > 1) once per FRAME — ``frames[name] [T+H, N, O]`` instead of
  rows ``[T+1, N, H·O]``: a step stores O floats per env (``gf_rollout_frame_write``, one launch for all such managers, behind the
  step's own), the minibatch gather rebuilds the ``[mb, H·O]`` rows — and so follows an ``output="window"`` manager too.
  ``obs_groups`` (rsl_rl's dict form) adds the rows of further ObservationManagers — the gait trainer's asymmetric critic —
  stored by the step's own launches too, and ``mini_batch_generator`` reads the rollout back as PPO minibatches: rsl_rl's nine
  per-field index launches per minibatch are one ``gf_minibatch_gather`` launch.
  The two per-step pieces of rsl_rl's collection loop around ``env.step()`` are one launch each: ``act`` samples the Gaussian
  actions, their log-probability and the policy's rows (``PPO.act``: ~ten elementwise launches, then five ``copy_``) with
  ``gf_policy_act``, and ``process_env_step`` bootstraps the time-outs and keeps the runner's episode statistics
  (:class:`EpisodeStatistics`: ``rewbuffer`` / ``lenbuffer`` without the per-step ``nonzero()`` and ``.cpu()``) with
  ``gf_episode_step``.
  ``act_policy`` takes the observations instead of the network outputs: the actor and critic forward passes of a
  :class:`PolicyForward` run inside the same launch (``gf_mlp_act``: f32 MFMA, activations in LDS, weights read in place).
* :class:`GradientAllReduce` — the multi-GPU half: every rank owns a shard of envs and a replica of the policy; after
  ``backward()`` the gradients of all parameters are averaged with ONE all-reduce over a flat bucket (RCCL over xGMI on GPUs;
  the 512-256-128 actor + critic MLPs of the reference configs are 1.5 MB), overlapped with nothing because nothing follows
  it but the optimizer step.  This is the first place of the pipeline where xGMI bandwidth rather than latency matters.
* :class:`ActorCriticMLP` — the policy of ``examples/*/train.py`` (ELU, hidden dims 512-256-128, learnable action std) as a
  plain torch module, so the two pieces above can be exercised without rsl_rl.
* :class:`EmpiricalNormalization` — rsl_rl's running observation normaliser (the ``"empirical_normalization"`` switch of
  ``examples/*/train.py``; rsl_rl 3.x's ``actor_obs_normalization`` / ``critic_obs_normalization``): the statistics of both
  normalisers are ONE ``gf_obs_norm_update`` per collection step (two launches, no host read), and the normalisation itself has no
  launch of its own — ``gf_mlp_act`` applies it as it stages the first layer's input, ``gf_minibatch_gather`` as it copies the rows.
* :class:`PPO` — rsl_rl's ``PPO.update`` for the ``"algorithm"`` dict of ``examples/*/train.py``: per minibatch the MLP forward /
  backward stay in torch, the loss and its gradient w.r.t. the policy outputs are one ``gf_ppo_loss`` (two launches), the adaptive
  learning rate, ``clip_grad_norm_`` and Adam over the flat gradient bucket are one ``gf_adam_step`` (two launches) — no host
  synchronisation per minibatch; the three logged means are read once per update.  With rsl_rl's ``symmetry_cfg`` (a
  :class:`~genesis_forge_amd.symmetry.MirrorSymmetry` as its function) the augmented minibatch is one ``gf_mirror_rows`` and the mirror
  loss with its gradient one ``gf_mirror_loss``.
* :class:`StudentTeacherMLP`, :class:`DistillForward`, :class:`Distillation` — rsl_rl's ``Distillation`` algorithm with a
  ``StudentTeacher`` policy, the step after PPO: a student that reads only deployable observations is regressed onto the frozen PPO
  actor.  ``RolloutStorage.act_distill`` runs both MLPs of a collection step, the sampling and the two storage rows in ONE
  ``gf_mlp_distill_act`` launch; an update walks ``RolloutStorage.step_batches()`` with one ``gf_bc_loss`` per time step and one
  ``gf_adam_step`` every ``gradient_length`` steps, and reads the device once.
* :class:`RandomNetworkDistillation`, :class:`EmpiricalDiscountedVariationNormalization`, :class:`RndForward` — rsl_rl's curiosity
  bonus (``algorithm.rnd_cfg``): a frozen random target and a trained predictor read an ``"rnd_state"`` observation group, the distance
  of their outputs is an intrinsic reward.  ``RolloutStorage.intrinsic_reward`` adds it to the storage row of a collection step with
  ONE ``gf_rnd_reward`` launch — both MLPs, the distance, the reward normaliser, the weight and the add; two launches with the
  reward normaliser updating, no host read — and :class:`PPO` trains the predictor per minibatch (``group_rows_batch``,
  ``gf_bc_loss``, an Adam of its own).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import statistics
from typing import Dict, Iterable, Iterator, List, NamedTuple, Optional, Sequence

import torch

from . import _native as nat
from . import gs


class MiniBatch(NamedTuple):
    """One PPO minibatch (rsl_rl ``mini_batch_generator``): rows ``indices`` of the flattened ``[T·N, …]`` storage, fresh tensors."""
    obs: torch.Tensor            # [mb, W_policy group]
    critic_obs: torch.Tensor     # [mb, W_critic group] (``obs`` itself when the two groups are the same)
    actions: torch.Tensor        # [mb, A]
    values: torch.Tensor         # [mb]
    advantages: torch.Tensor     # [mb]
    returns: torch.Tensor        # [mb]
    old_log_prob: torch.Tensor   # [mb]
    old_mu: torch.Tensor         # [mb, A]
    old_sigma: torch.Tensor      # [mb, A]
    indices: torch.Tensor        # [mb] int64: transition (t, n) = divmod(index, N)


class RecurrentMiniBatch(NamedTuple):
    """One minibatch of trajectories (rsl_rl ``recurrent_mini_batch_generator``): the envs of a contiguous range, fresh tensors."""
    obs: torch.Tensor            # [T, ntraj, W_policy group] padded with zeros, through the actor's normaliser
    critic_obs: torch.Tensor     # [T, ntraj, W_critic group] (``obs`` itself when the two groups are the same)
    masks: torch.Tensor          # [T, ntraj] bool: the real steps
    hid_a: object                # the actor memory's initial state: h0 [1, ntraj, H], or (h0, c0) for an LSTM
    hid_c: object                # the critic memory's
    unpad_index: torch.Tensor    # [envs · T] int64: the policy's batch mode un-pads with it (index_select)
    rows: MiniBatch              # the per-row fields, [T · envs, …] in (t, env) order; its obs / critic_obs are None


_MB_FIELDS = ("actions", "values", "advantages", "returns", "actions_log_prob", "mu", "sigma")   # MiniBatch fields after the observations
_LOG_SQRT_2PI = math.log(math.sqrt(2 * math.pi))   # the constant of torch's Normal.log_prob


def _rows_ok(x: torch.Tensor) -> bool:
    """Contiguous rows — or the history window an ``ObservationManager(output="window")`` handed out (it marks its views): unit
    column stride, rows at least a width apart.  ``gf_mlp_act`` and ``gf_obs_norm_update`` read such a view in place (``row_stride``);
    any other strided tensor stays refused: nothing says how long its rows stay what they are."""
    return x.is_contiguous() or (getattr(x, "_gf_window", False) and x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= x.shape[1])


def _check_f32(x, name: str, shapes, device, window: bool = False) -> None:
    """``act``'s inputs are taken as they are: float32, contiguous, on the storage's device, one of ``shapes`` — nothing is cast.
    ``window``: an observation — the strided view of a window-mode ObservationManager is taken as it is too (``_rows_ok``)."""
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{name} must be a tensor")
    if x.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, not {x.dtype}")
    if x.device != device:
        raise ValueError(f"{name} lives on {x.device}, the storage on {device}")
    if tuple(x.shape) not in shapes:
        raise ValueError(f"{name} has shape {tuple(x.shape)}; expected one of {sorted(shapes)}")
    if not (_rows_ok(x) if window else x.is_contiguous()):
        raise ValueError(f"{name} must be contiguous")


def _check_mask(x, name: str, n: int, device) -> torch.Tensor:
    """A ``[N]`` done / time-out mask on ``device`` as the bytes the kernel reads (bool or uint8; anything else is compared with 0)."""
    if not isinstance(x, torch.Tensor) or x.device != device or x.numel() != n or (x.dim() == 2 and x.shape[1] != 1) or x.dim() > 2:
        raise ValueError(f"{name} must be a [{n}] tensor on {device}")
    x = x.reshape(n)
    if x.dtype != torch.bool and x.dtype != torch.uint8:
        x = x != 0
    return x.contiguous()


class _GroupRows:
    """The time-major rows ``[T+1, N, W]`` of one observation-group member other than the storage's ``obs_name`` manager, and the
    descriptor that stores them: a ``gf_rollout_write`` with only the observation row set — or, in a fused recorded step, the second
    destination of the manager's own history gather (no launch of its own)."""

    group_row = True   # (_trace.StepTrace tells these rollout_write calls from the storage's own by it)

    def __init__(self, om, rows: torch.Tensor):
        self.om, self.rows = om, rows
        self.args = nat.GfRolloutArgs()
        self.args.num_envs, self.args.obs_width = rows.shape[1], rows.shape[2]

    def unroll_ok(self) -> bool:
        """The manager's gather can store the row itself: its history is a ring, and every row start is 16-byte aligned."""
        return bool(self.om._unrolled) and (self.rows.stride(0) * 4) % 16 == 0 and self.rows.data_ptr() % 16 == 0

    def write(self, backend) -> None:
        out = self.om._last_out
        if not out.is_contiguous():
            raise ValueError(f"RolloutStorage copies contiguous observation rows: '{self.om.name}' is a strided view (output='window')")
        self.args.obs = out.data_ptr()
        self._keep = out
        backend.call("rollout_write", self.args, owner=self)

    def _trace(self, args, via_unroll: bool):
        """Recorded step: (Python patch or None, native patches).  The row address is advanced by the storage's own patch, which runs
        first (its rollout_write comes first); ``via_unroll``: the fused launch's gather writes the row as its second destination."""
        om, P = self.om, nat.GfReplayPatch
        if om._window:
            from ._trace import Untraceable
            raise Untraceable("the rollout rows of a window-mode observation (a strided view) cannot be copied by the step's launch")
        if via_unroll:
            def patch(_actions, a=args, u=om._unroll_args):
                u.out2 = a.obs_out

            return patch, []
        src = nat.field_addr(om._unroll_args, "out") if om._unrolled else nat.field_addr(om._args, "obs")
        return None, [P(nat.GF_PATCH_COPY, 0, nat.field_addr(args, "obs"), None, src)]


class RolloutStorage:
    """Rollout rows of ``num_steps`` transitions for ``env.num_envs`` envs (layout of rsl_rl's RolloutStorage, time-major).

    ``observations[t]`` is the policy input of transition ``t`` (row 0: the observation the rollout starts from; row
    ``num_steps``: the bootstrap observation), ``rewards[t]`` / ``dones[t]`` its outcome.  ``attach()`` makes every
    ``env.step()`` write transition ``step``'s rows and advance; after ``num_steps`` steps ``full`` is true and the next step
    starts the next rollout (its row 0 is the previous rollout's row ``num_steps``).

    ``obs_groups`` is rsl_rl's dict form (``{"policy": ["policy"], "critic": ["policy", "critic"]}``): a group's input is the
    concatenation of the named ObservationManagers' rows in list order.  Rows are kept once per distinct manager, not per group:
    ``observations`` for ``obs_name``, ``group_rows[name]`` for every member (the ``obs_name`` entry is ``observations``
    itself).  ``None``: both groups are ``[obs_name]`` — nothing beyond ``observations`` is stored.
    ``mini_batch_generator`` reads the rollout back as PPO minibatches.

    ``history="frames"``: every followed manager with ``history_len`` = H > 1 is kept once per frame — ``frames[name]`` is
    ``[T + H, N, O]``, observation row ``r`` (0 … T) of that manager is frames ``r … r+H-1``, frame ``r+H-1`` the newest (the
    reference's history is a pure sliding window — never cleared per env, untouched by a reset — so row ``t`` is frames
    ``t, t-1, … t-H+1``).  Such a manager has no entry in ``group_rows``, and ``observations`` is ``None`` when ``obs_name`` is one;
    ``observation_rows()`` materialises the rows.  A step stores the newest frame only (columns ``0 … O-1`` of the tensor the step
    returned, whatever its row stride: ``output="fresh"``, ``"static"`` and ``"window"`` are all newest first; ``"ring"`` is ordered
    by slot and refused), one ``gf_rollout_frame_write`` launch for all of them behind the step's own; the minibatch gather rebuilds
    the ``[mb, H·O]`` rows (a pure copy: the same bits).  Managers without a history keep their rows; the default ``"rows"`` is the
    layout above for every manager."""

    def __init__(self, env, num_steps: int, obs_name: str = "policy", obs_groups: Optional[Dict[str, Sequence[str]]] = None,
                 history: str = "rows"):
        if history not in ("rows", "frames"):
            raise ValueError(f"history must be 'rows' or 'frames', not {history!r}")
        self.env, self.num_steps, self.obs_name, self.history = env, int(num_steps), obs_name, history
        n = env.num_envs
        managers = {m.name: m for m in env.managers["observation"]}
        om = managers.get(obs_name)
        if om is None:
            raise ValueError(f"no ObservationManager named '{obs_name}'")
        self._om = om
        self.frames: Dict[str, torch.Tensor] = {}
        self._frame_oms: list = []   # the frame-stored managers, in the order of their segments
        self.obs_width = int(om.observation_space.shape[0])
        self._widths = {obs_name: self.obs_width}
        if self._framed(om):
            self.observations = None
            self._add_frames(om)
        else:
            self._refuse_window(om)
            self.observations = torch.zeros((self.num_steps + 1, n, self.obs_width), device=gs.device, dtype=torch.float32)
        groups = {"policy": [obs_name], "critic": [obs_name]} if obs_groups is None else {k: list(v) for k, v in obs_groups.items()}
        if "policy" not in groups:
            raise ValueError("obs_groups needs a 'policy' group")
        groups.setdefault("critic", list(groups["policy"]))
        self.obs_groups = groups
        self.group_rows: Dict[str, torch.Tensor] = {}
        self._group_writers: List[_GroupRows] = []
        for members in groups.values():
            if not members:
                raise ValueError("an observation group needs at least one ObservationManager")
            for name in members:
                if name in self.group_rows or name in self.frames:
                    continue
                m = managers.get(name)
                if m is None:
                    raise ValueError(f"obs_groups names '{name}', but the env has no ObservationManager of that name")
                self._widths[name] = int(m.observation_space.shape[0])
                if self._framed(m):
                    self._add_frames(m)
                    continue
                self._refuse_window(m)
                if name == obs_name:
                    self.group_rows[name] = self.observations
                    continue
                rows = torch.zeros((self.num_steps + 1, n, int(m.observation_space.shape[0])), device=gs.device, dtype=torch.float32)
                self.group_rows[name] = rows
                self._group_writers.append(_GroupRows(m, rows))
        self.rewards = torch.zeros((self.num_steps, n), device=gs.device, dtype=torch.float32)
        self._device = self.rewards.device
        self.dones = torch.zeros((self.num_steps, n), device=gs.device, dtype=torch.bool)
        self.step = 0            # transitions written in the current rollout
        self._args = nat.GfRolloutArgs()
        self._args.num_envs, self._args.obs_width = n, self.obs_width
        # one descriptor per GF_ROLLOUT_FRAME_MAX frame-stored managers: each is one gf_rollout_frame_write launch per step
        k = nat.GF_ROLLOUT_FRAME_MAX
        self._frame_parts = [(nat.GfRolloutFrameArgs(), self._frame_oms[at:at + k]) for at in range(0, len(self._frame_oms), k)]
        for fa, oms in self._frame_parts:
            fa.num_envs, fa.num_segs = n, len(oms)
            for seg, m in zip(fa.segs, oms):
                seg.width = self.frames[m.name].shape[2]
        # per frame-stored manager: (manager, frames, address of frame H, bytes per frame); the output mode its tensor was last checked in
        self._frame_dst = {m.name: (self.frames[m.name].data_ptr() + m._history_len * self.frames[m.name].stride(0) * 4, self.frames[m.name].stride(0) * 4)
                           for m in self._frame_oms}
        self._frame_checked: Dict[str, str] = {}
        # the policy's rows and the return computation (allocated on first use: a storage that only takes the env's rows stays small)
        self.num_actions = None
        self.actions = self.values = self.actions_log_prob = self.mu = self.sigma = self.returns = self.advantages = None
        self.privileged_actions = None   # [T, N, A] the teacher's actions of a distillation rollout (act_distill)
        self._pol_args = nat.GfRolloutPolicyArgs()
        self._gae_args = nat.GfGaeArgs()
        self._moments = None
        self._returns_ready = False
        self._mb_args = nat.GfMinibatchArgs()
        self._mb_normed = False   # the descriptor holds normaliser pointers (of the last gather)
        # the collection loop around env.step() (act / process_env_step).  `_serial` counts the transitions written; the policy rows
        # and the bootstrap are tracked as the serial of the transition they belong to.  The action noise has a Philox seed and
        # stream of its own (``seed()``): never the env's draws.
        self._serial = 0
        self._pol_serial = self._boot_serial = self._rnd_serial = self._proc_serial = -1
        self._act_seed: Optional[int] = None   # None: the env's seed (the kernel XORs GF_POLICY_SEED_TAG into it either way)
        self._act_stream = 0
        self._act_args = nat.GfPolicyActArgs()
        self._ep_args = nat.GfEpisodeArgs()
        self._grp_args = nat.GfMinibatchArgs()   # group_rows_batch's own descriptor (the minibatch gather's keeps its normaliser state)
        self.rnd_sums: Optional[torch.Tensor] = None   # [2, N] float64: per-env sums of the extrinsic / intrinsic rewards (intrinsic_reward)

    @staticmethod
    def _refuse_window(om) -> None:
        if getattr(om, "output", None) == "window" and om._history_len > 1:
            raise ValueError(f"RolloutStorage copies contiguous observation rows: ObservationManager '{om.name}' has output='window' and "
                             "hands out a strided view — use output='fresh' / 'static' for the managers the storage follows")

    def _framed(self, om) -> bool:
        return self.history == "frames" and om._history_len > 1

    def _add_frames(self, om) -> None:
        if getattr(om, "output", None) == "ring":
            raise ValueError(f"RolloutStorage(history='frames') stores the newest frame of a newest-first observation: ObservationManager "
                             f"'{om.name}' has output='ring', which is ordered by slot — use output='fresh', 'static' or 'window'")
        H = om._history_len
        O = int(om.observation_space.shape[0]) // H
        self.frames[om.name] = torch.zeros((self.num_steps + H, self.env.num_envs, O), device=gs.device, dtype=torch.float32)
        self._frame_oms.append(om)

    @property
    def device(self) -> torch.device:
        return self._device

    @property
    def full(self) -> bool:
        return self.step >= self.num_steps

    def attach(self) -> "RolloutStorage":
        self.env._rollout = self
        self.env.invalidate_trace()
        return self

    def detach(self) -> None:
        if self.env._rollout is self:
            self.env._rollout = None
            self.env.invalidate_trace()

    def begin(self, obs: torch.Tensor, extras: Optional[dict] = None) -> None:
        """Start a rollout from ``obs`` and ``extras`` (what ``env.reset()`` returned; the group members' starting rows are read from
        ``extras["observations"]``, so ``extras`` is required when ``obs_groups`` names a manager other than ``obs_name``)."""
        if self._group_writers or any(m is not self._om for m in self._frame_oms):
            if extras is None or "observations" not in extras:
                raise ValueError("begin(obs, extras): the observation groups need every member's starting rows — pass what env.reset() returned")
            for w in self._group_writers:
                w.rows[0].copy_(extras["observations"][w.om.name])
        for m in self._frame_oms:   # row 0 as its H frames: column block j (newest first) is frame H-1-j
            row = obs if m is self._om else extras["observations"][m.name]
            F = self.frames[m.name]
            H, O = m._history_len, F.shape[2]
            for j in range(H):
                F[H - 1 - j].copy_(row[:, j * O:(j + 1) * O])
        if self.observations is not None:
            self.observations[0].copy_(obs)
        self.step = 0
        self._pol_serial = self._boot_serial = self._rnd_serial = self._proc_serial = -1

    def _next_rows(self, a: nat.GfRolloutArgs) -> None:
        """Point the descriptor at transition ``step``'s rows and advance (wrapping into the next rollout)."""
        T = self.num_steps
        if self.step >= T:
            if self.observations is not None:
                self.observations[0].copy_(self.observations[T])
            for w in self._group_writers:
                w.rows[0].copy_(w.rows[T])
            for F in self.frames.values():   # row T's frames become row 0's: one contiguous block, which overlaps itself when H > T
                H = F.shape[0] - T
                F[:H].copy_(F[T:].clone() if H > T else F[T:])
            self.step = 0
        t = self.step
        a.obs_out = None if self.observations is None else self.observations.data_ptr() + (t + 1) * self.observations.stride(0) * 4
        a.reward_out = self.rewards.data_ptr() + t * self.rewards.stride(0) * 4
        a.done_out = self.dones.data_ptr() + t * self.dones.stride(0)
        for w in self._group_writers:
            w.args.obs_out = w.rows.data_ptr() + (t + 1) * w.rows.stride(0) * 4
        self.step = t + 1
        self._serial += 1

    def write(self, obs: torch.Tensor, reward: torch.Tensor, terminated: torch.Tensor, truncated: torch.Tensor) -> None:
        """One transition through ``gf_rollout_write`` (the phase-by-phase path; a recorded step fuses it, _trace.py)."""
        a = self._args
        if self.observations is None:   # (the observation is frame-stored: this launch writes the reward and done rows only)
            a.obs = None
        elif not obs.is_contiguous():   # (an ObservationManager switched to output="window" after this storage was made)
            raise ValueError("RolloutStorage copies contiguous observation rows: the observation it follows is a strided view (output='window')")
        else:
            a.obs = obs.data_ptr()
        a.reward = reward.data_ptr()
        a.terminated, a.truncated = terminated.data_ptr(), truncated.data_ptr()
        self._next_rows(a)
        self._keep = (obs, reward, terminated, truncated)
        self.env.backend.call("rollout_write", a, owner=self)
        for w in self._group_writers:   # (behind the storage's own launch: a recorded step advances the rows in that order)
            w.write(self.env.backend)
        if self._frame_parts:
            self._write_frames()

    def _write_frames(self) -> None:
        """The newest frame of every frame-stored manager into ``frames[step - 1 + H]``: one ``gf_rollout_frame_write`` per four of
        them, right behind the step's ``rollout_write`` (a recorded step calls this after its launches are enqueued, _trace.py) — or the
        same copy in torch on a backend without the entry point (the test-only oracle backend)."""
        t = self.step - 1
        fn = getattr(self.env.backend, "rollout_frame_write", None)
        keep = []
        for fa, oms in self._frame_parts:
            for seg, m in zip(fa.segs, oms):
                out = m._last_out
                if self._frame_checked.get(m.name) != m._output:   # (once, and again after the manager's output mode was switched)
                    self._check_frame_source(m, out)
                if fn is None:
                    F = self.frames[m.name]
                    F[t + m._history_len].copy_(out[:, :F.shape[2]])
                    continue
                base, step = self._frame_dst[m.name]
                seg.src, seg.src_stride, seg.dst = out.data_ptr(), out.stride(0), base + t * step
                keep.append(out)
            if fn is not None:
                fn(fa)
        self._keep_frames = keep

    def _check_frame_source(self, m, out: torch.Tensor) -> None:
        """What a manager's tensors are in one output mode: checked when the mode is first seen, not on every step."""
        F = self.frames[m.name]
        n, H, O = self.env.num_envs, m._history_len, F.shape[2]
        if m._output == "ring":   # (switched after this storage was made)
            raise ValueError(f"RolloutStorage(history='frames'): ObservationManager '{m.name}' has output='ring', which is ordered by slot")
        if (out.dtype != torch.float32 or out.dim() != 2 or tuple(out.shape) != (n, H * O) or out.device != F.device
                or (out.stride(1) != 1 and H * O > 1) or out.stride(0) < O):
            raise ValueError(f"RolloutStorage(history='frames'): the observation of '{m.name}' is not a float32 [{n}, {H * O}] tensor with unit column stride")
        self._frame_checked[m.name] = m._output

    def observation_rows(self, name: Optional[str] = None, t: Optional[int] = None) -> torch.Tensor:
        """The observation rows of manager ``name`` (``None``: ``obs_name``) as rsl_rl keeps them: a new ``[T+1, N, W]`` tensor, or the
        ``[N, W]`` of row ``t`` — for a frame-stored manager built from its frames with torch indexing (newest frame first).  For
        inspecting a rollout and for tests: it allocates; the minibatch gather reads the frames themselves."""
        name = self.obs_name if name is None else name
        T = self.num_steps
        if t is not None and not 0 <= int(t) <= T:
            raise ValueError(f"row {t} is outside 0 … {T}")
        F = self.frames.get(name)
        if F is None:
            rows = self.observations if name == self.obs_name else self.group_rows.get(name)
            if rows is None:
                raise ValueError(f"the storage follows no ObservationManager named '{name}'")
            return rows.clone() if t is None else rows[int(t)].clone()
        H = F.shape[0] - T
        if t is None:
            return torch.cat([F[H - 1 - j:H + T - j] for j in range(H)], dim=-1)
        return torch.cat([F[int(t) + H - 1 - j] for j in range(H)], dim=-1)

    # -- the policy's half of a transition, returns ---------------------------------------------------------------------------
    def _ensure_policy_rows(self, num_actions: int) -> None:
        if self.values is not None and self.num_actions == num_actions:   # (act_distill allocates `actions` alone)
            return
        T, n = self.num_steps, self.env.num_envs
        z = lambda *shape: torch.zeros(shape, device=gs.device, dtype=torch.float32)
        self.num_actions = int(num_actions)
        self.actions, self.mu, self.sigma = z(T, n, num_actions), z(T, n, num_actions), z(T, n, num_actions)
        self.values, self.actions_log_prob, self.returns, self.advantages = z(T, n), z(T, n), z(T, n), z(T, n)
        self._moments = torch.zeros(2, device=gs.device, dtype=torch.float64)

    def add_policy(self, actions: torch.Tensor, values: torch.Tensor, log_prob: torch.Tensor, mu: torch.Tensor, sigma: torch.Tensor,
                   time_outs: Optional[torch.Tensor] = None, gamma: float = 0.99) -> None:
        """What the policy produced for the transition the last ``env.step()`` wrote (row ``step - 1``): rsl_rl's
        ``add_transitions`` for actions / values / actions_log_prob / mu / sigma, after ``rewards[t] += gamma * values *
        time_outs`` (PPO.process_env_step) when ``time_outs`` (this step's truncated flags) is given.  One launch."""
        if self.step < 1:
            raise RuntimeError("add_policy() follows the env.step() whose transition it completes")
        f = lambda t: t if (t.dtype == torch.float32 and t.is_contiguous()) else t.to(torch.float32).contiguous()
        actions, mu, sigma = f(actions), f(mu), f(sigma)
        values, log_prob = f(values.reshape(-1)), f(log_prob.reshape(-1))
        self._ensure_policy_rows(actions.shape[-1])
        t, a = self.step - 1, self._pol_args
        a.num_envs, a.num_actions = self.env.num_envs, self.num_actions
        a.actions, a.values, a.log_prob, a.mu, a.sigma = (x.data_ptr() for x in (actions, values, log_prob, mu, sigma))
        self._policy_row_ptrs(a, t)
        if time_outs is not None:
            if time_outs.dtype != torch.bool and time_outs.dtype != torch.uint8:
                time_outs = time_outs != 0
            time_outs = time_outs.contiguous()
            a.time_outs, a.reward_row, a.gamma = time_outs.data_ptr(), self.rewards.data_ptr() + t * self.rewards.stride(0) * 4, float(gamma)
        else:
            a.time_outs, a.reward_row, a.gamma = None, None, 0.0
        self._keep_pol = (actions, values, log_prob, mu, sigma, time_outs)
        self.env.backend.call("rollout_policy_write", a, owner=None)
        self._pol_serial = self._serial
        if time_outs is not None:
            self._boot_serial = self._serial

    # -- the collection loop around env.step(): act -> env.step -> process_env_step ---------------------------------------------
    def seed(self, seed: int) -> None:
        """Seed of the action noise of ``act`` (Philox key ``seed ^ GF_POLICY_SEED_TAG``); its stream starts again at 0.  Until
        this is called the env's seed is used — with the tag, so the draws never repeat one of the env's."""
        self._act_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._act_stream = 0

    def act(self, mean: torch.Tensor, std: torch.Tensor, values: torch.Tensor, noise: Optional[torch.Tensor] = None,
            std_is_log: bool = False) -> torch.Tensor:
        """rsl_rl's ``PPO.act`` from the actor's ``mean`` ``[N, A]``, the action ``std`` (``[A]``, rsl_rl's ``noise_std_type=
        "scalar"``; or ``[N, A]``) and the critic's ``values`` (``[N]`` or ``[N, 1]``):
        returns ``Normal(mean, std).sample()`` as a fresh ``[N, A]`` tensor and writes the policy's rows of the transition the next
        ``env.step()`` writes (row ``step``, 0 once the storage is ``full``): actions, mu, sigma (``std`` expanded), values and
        ``log_prob(actions).sum(-1)``.  ``std_is_log=True`` (``noise_std_type="log"``): ``std`` is the policy's ``log_std`` and the
        kernel exponentiates it — the sample, the log-probability and the sigma row all see ``exp(log_std)``, the same bits
        ``gf_ppo_loss`` later derives from that ``log_std``.  One ``gf_policy_act`` launch; the draws are Philox + Box–Muller keyed by (seed, stream,
        global env id, column) — the stream advances once per call, the env's own stream is never touched.
        ``noise``: ``[N, A]`` standard normals used instead of the draws (parity tests; the only mode of the CPU oracle backend).
        Inputs must be float32, contiguous and on the storage's device: nothing is cast (``ValueError``)."""
        n, dev = self.env.num_envs, self.device
        if not isinstance(mean, torch.Tensor) or mean.dim() != 2 or mean.shape[0] != n or mean.shape[1] < 1:
            raise ValueError(f"mean must be a [{n}, A] tensor")
        A = int(mean.shape[1])
        _check_f32(mean, "mean", {(n, A)}, dev)
        _check_f32(std, "std", {(A,), (n, A)}, dev)
        _check_f32(values, "values", {(n,), (n, 1)}, dev)
        if noise is not None:
            _check_f32(noise, "noise", {(n, A)}, dev)
        self._ensure_policy_rows(A)
        return self._policy_act(mean, std, values, noise, std_is_log)

    def _open_act(self) -> tuple:
        """What every act call starts from: ``(t, stream, seed, env_offset)`` — the row of the transition the next ``env.step()``
        writes (``step``, 0 once the storage is ``full``: env.step() does the wrap's row copies, only the index is needed here), the
        noise stream (advanced by this call), the Philox seed and the global id of env 0."""
        stream = self._act_stream
        self._act_stream += 1
        seed = self.env._rng_seed if self._act_seed is None else self._act_seed
        return self._act_row(), stream, seed, int(getattr(self.env, "env_offset", 0))

    def _act_row(self) -> int:
        return 0 if self.full else self.step

    def _policy_row_ptrs(self, a, t: int, actions_only: bool = False) -> None:
        """Point the five ``*_out`` fields of a descriptor at row ``t`` of the policy's rows (``actions_only``: the other four are None)."""
        row = lambda x: x.data_ptr() + t * x.stride(0) * 4
        a.actions_out = row(self.actions)
        a.mu_out, a.sigma_out, a.values_out, a.log_prob_out = (
            (None,) * 4 if actions_only else (row(x) for x in (self.mu, self.sigma, self.values, self.actions_log_prob)))

    def _policy_act(self, mean, std, values, noise, std_is_log: bool) -> torch.Tensor:
        """``act`` behind its checks: one ``gf_policy_act`` launch.  ``values=None`` (a distillation step): only the action row is
        written."""
        n, A = mean.shape
        actions = torch.empty((n, A), device=self.device, dtype=torch.float32)
        t, stream, seed, env_offset = self._open_act()
        fn = getattr(self.env.backend, "policy_act", None)
        if fn is None:   # (the test-only oracle backend) the same expression in torch, from the given draws
            if noise is None:
                raise RuntimeError("act() draws its noise in the HIP kernel: on a backend without gf_policy_act pass noise=")
            self._act_torch(mean, std, values, noise, actions, t, std_is_log)
        else:
            a = self._act_args
            a.num_envs, a.num_actions, a.std_per_env = n, A, 1 if std.dim() == 2 else 0
            a.std_is_log = 1 if std_is_log else 0
            a.mean, a.std, a.values = mean.data_ptr(), std.data_ptr(), None if values is None else values.data_ptr()
            a.noise = None if noise is None else noise.data_ptr()
            a.seed, a.stream, a.env_offset = seed, stream, env_offset
            a.actions = actions.data_ptr()
            self._policy_row_ptrs(a, t, actions_only=values is None)
            self._keep_act = (mean, std, values, noise)
            fn(a)
        self._pol_serial = self._serial + 1   # (the transition the next env.step() writes)
        return actions

    def act_policy(self, forward: "PolicyForward", obs, critic_obs=None, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``act(policy.act_mean(obs), policy.std, policy.evaluate(critic_obs), noise)`` (``policy.log_std`` and ``std_is_log=True`` for
        a ``noise_std_type="log"`` policy) with the two forward passes inside the launch:
        ONE ``gf_mlp_act`` runs the actor and the critic MLP of ``forward`` (a :class:`PolicyForward`) on the f32 matrix cores, samples
        and writes the policy's rows — instead of torch's GEMM and ELU launch per layer and ``gf_policy_act`` behind them.  The row, the
        noise stream and seed, and the input rules are ``act``'s: a loop that replaces ``store.act(policy.act_mean(obs), policy.std,
        policy.evaluate(obs))`` by ``store.act_policy(fwd, obs)`` draws the same noise.  ``obs`` / ``critic_obs``: a ``[N, W]`` tensor
        or a sequence of up to four (the members of an observation group side by side — no ``torch.cat``); ``critic_obs=None``: the
        critic reads ``obs``.  The strided view of an ``output="window"`` ObservationManager is read in place (``row_stride``); any other
        non-contiguous tensor is refused.  The mean and the value are k-ascending f32 fma chains (``gf_step.h``), not torch's GEMM bits: within
        f32 rounding of ``policy.act_mean`` / ``evaluate``, and the same for a row whatever ``num_envs`` is.  A policy with observation
        normalisers (:class:`EmpiricalNormalization`) has them applied inside the same launch, to the raw ``obs`` / ``critic_obs``.
        Measured per collection step (profiles/r09_mlp_act.md): 3.5 x faster than ``act()`` on torch's forward at 4 096 envs, 1.4 x
        at 16 384, but 7 % SLOWER at 65 536 envs, where the large GEMMs win: there ``act()`` with the torch forward is the call to use.
        On a backend without ``gf_mlp_act`` (the test-only CPU oracle) this is exactly the ``act`` call above under ``no_grad``, and
        ``noise`` is required."""
        if not isinstance(forward, PolicyForward):
            raise ValueError("act_policy(forward, ...) takes a PolicyForward")
        if forward.actor is None or forward.critic is None or forward.num_actions is None:
            raise ValueError("act_policy needs a policy with an actor, a critic and a [A] std (or log_std)")
        return self._act_actor_critic(forward, obs, critic_obs, noise)

    def _act_actor_critic(self, forward, obs, critic_obs, noise) -> torch.Tensor:
        """``act_policy`` and ``act_recurrent`` behind their refusals: the checks, the row, the descriptor of ``forward`` — a forward
        with memories nests it as ``.act`` and has, at row 0, the state the rollout starts from saved into ``rnn_start`` — and the ONE
        launch of the forward's entry; on a backend without it (the test-only oracle backend) ``act`` on the module's torch step."""
        n, dev = self.env.num_envs, self.device
        segs = _segments(obs, "obs", n, dev, forward._reader("actor"))   # (a window-mode manager's strided view is read in place)
        csegs = _segments(obs if critic_obs is None else critic_obs, "obs (the critic's input)" if critic_obs is None else "critic_obs", n, dev,
                          forward._reader("critic"))
        A = forward.num_actions
        std, is_log = getattr(forward.policy, forward._std_name), forward.std_is_log
        first = bool(forward._memory) and self._act_row() == 0
        fn = getattr(self.env.backend, forward._ENTRY, None)
        if fn is None:   # today's path, bit for bit
            with torch.no_grad():
                if first:
                    self.keep_rnn_start(forward.policy)
                return self.act(forward.policy.act_mean(_cat(segs)), std.detach(), forward.policy.evaluate(_cat(csegs)), noise, std_is_log=is_log)
        _check_f32(std, "policy.log_std" if is_log else "policy.std", {(A,)}, dev)
        if noise is not None:
            _check_f32(noise, "noise", {(n, A)}, dev)
        self._ensure_policy_rows(A)
        save = None
        if first:   # (the launch writes them)
            save = self.rnn_start = {name: _rnn_state_rows(m, n, dev, empty=True) for name, m in forward._memory.items()}
        actions = torch.empty((n, A), device=dev, dtype=torch.float32)
        t, stream, seed, env_offset = self._open_act()
        d = forward._fill(n, segs, csegs, save)
        a = forward._args_parts[0]   # (d itself, or its .act where the descriptor is nested)
        _fill_sampling(a, std, is_log, noise, seed, stream, env_offset, actions)
        a.std_per_env, a.values = 0, None
        self._policy_row_ptrs(a, t)
        self._keep_act = (segs, csegs, noise)
        fn(d)
        self._pol_serial = self._serial + 1   # (the transition the next env.step() writes)
        return actions

    def act_recurrent(self, forward: "RecurrentForward", obs, critic_obs=None, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``act_policy`` for a recurrent policy: ONE ``gf_mlp_recurrent_act`` launch normalises the observations, advances the actor's
        and the critic's LSTM / GRU state by one step in place (rows flagged by ``forward.reset(dones)`` start from zeros), walks the two
        MLPs from the new hidden states, samples and writes the policy's rows.  The row, the noise stream and seed, and the input rules
        are ``act_policy``'s.  At the first step of a rollout (row 0) the launch also writes the state the rollout starts from, after
        the reset, into ``rnn_start`` (``{"actor": (h, c), "critic": (h, c)}``, ``[N, H]`` each, ``c`` None for a GRU): a trajectory that
        starts later starts behind a done, from zeros, so the rollout-start state is all an update needs (rsl_rl stores the state of
        every step).  The cell and the MLPs are k-ascending f32 fma chains with the device libm's ``expf`` / ``tanhf`` (``gf_step.h``):
        within f32 rounding of the module's torch step, not its bits.  Measured per collection step against ``act()`` on the module's
        torch step (go2_cmd, 256 units, profiles/r26_recurrent.md): 3.5 x / 1.27 x / 1.10 x faster at 4 096 / 16 384 / 65 536 envs with
        an LSTM, 4.1 x / 1.54 x / 1.34 x with a GRU — this is the call to use at every size measured.  Against the MLP policy's
        ``act_policy`` a recurrent step still costs 2.2 x – 4.4 x: every 32-row tile streams the cell's weights again.
        On a backend without the entry (the test-only CPU oracle) this is ``act`` on the module's torch step under ``no_grad``, and
        ``noise`` is required."""
        if not isinstance(forward, RecurrentForward):
            raise ValueError("act_recurrent(forward, ...) takes a RecurrentForward")
        return self._act_actor_critic(forward, obs, critic_obs, noise)

    def keep_rnn_start(self, policy) -> None:
        """Copy the hidden states ``policy.get_hidden_states()`` holds — the state the rollout starts from, zeros where a memory has
        none yet — into ``rnn_start``: what a loop on the module's torch step calls before the first step of a rollout (``act_recurrent``
        does it inside its launch)."""
        n, dev = self.env.num_envs, self.device
        self.rnn_start = {name: _rnn_state_rows(m, n, dev) for name, m in (("actor", policy.memory_a), ("critic", policy.memory_c))}

    # -- teacher–student distillation: the collection step and the update's batches ------------------------------------------------
    def _ensure_distill_rows(self, num_actions: int) -> None:
        T, n = self.num_steps, self.env.num_envs
        if self.actions is None or self.num_actions != num_actions:
            self.num_actions = int(num_actions)
            self.actions = torch.zeros((T, n, num_actions), device=gs.device, dtype=torch.float32)
            self.values = None   # (PPO's rows, if any, were of another width)
        if self.privileged_actions is None or self.privileged_actions.shape[2] != num_actions:
            self.privileged_actions = torch.zeros((T, n, num_actions), device=gs.device, dtype=torch.float32)

    def act_distill(self, forward: "DistillForward", obs, teacher_obs=None, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """rsl_rl's ``Distillation.act``: returns ``Normal(student(obs), std).sample()`` as a fresh ``[N, A]`` tensor and writes
        ``actions[t]`` and ``privileged_actions[t] = teacher(teacher_obs)`` (``[T, N, A]``, allocated on first use) for the transition
        the next ``env.step()`` writes — ONE ``gf_mlp_distill_act`` launch for both MLPs of ``forward`` (a :class:`DistillForward`), the
        sampling and the two rows.  The row, the noise seed and stream and the input rules are ``act_policy``'s (segments and the
        strided view of a window-mode manager are read in place; ``teacher_obs=None``: the teacher reads ``obs``).  No value,
        log-probability, mu or sigma row is written: ``process_env_step(None, episodes=stats)`` is what follows the step.  On a backend
        without the entry point (the test-only CPU oracle) the same values are computed in torch and ``noise`` is required."""
        if not isinstance(forward, DistillForward):
            raise ValueError("act_distill(forward, ...) takes a DistillForward")
        return self._act_student_teacher(forward, obs, teacher_obs, noise)

    def _act_student_teacher(self, forward, obs, teacher_obs, noise) -> torch.Tensor:
        """``act_distill`` and ``act_distill_recurrent`` behind their refusals: the rows, ``forward.act`` with them as its second
        destinations and — for a forward with memories, at row 0 — ``rnn_start["student"]`` as what the launch saves the state into."""
        n, dev, A = self.env.num_envs, self.device, forward.num_actions
        _segments(obs, "obs", n, dev, forward._reader("student"))   # (the storage's env count and device; act() checks the rest)
        self._ensure_distill_rows(A)
        save = None
        if forward._memory and self._act_row() == 0:
            save = self.rnn_start = {"student": _rnn_state_rows(forward._memory["student"], n, dev, empty=True)}
        t, stream, seed, env_offset = self._open_act()
        actions, _teacher = forward.act(obs, teacher_obs, noise, seed=seed, stream=stream, env_offset=env_offset, actions_out=self.actions[t],
                                        teacher_actions_out=self.privileged_actions[t], backend=self.env.backend, save=save)
        self._pol_serial = self._serial + 1   # (the transition the next env.step() writes)
        return actions

    def act_distill_recurrent(self, forward: "RecurrentDistillForward", obs, teacher_obs=None, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``act_distill`` for a recurrent student (a :class:`RecurrentDistillForward`): ONE ``gf_mlp_recurrent_distill_act`` launch
        normalises both observations, advances ``memory_s`` (and ``memory_t``, if the teacher has one) by one step in place — rows
        flagged by ``forward.reset(dones)`` start from zeros — walks the two MLPs, samples and writes ``actions[t]`` and
        ``privileged_actions[t]``.  At the first step of a rollout (row 0) the launch also writes the state the student starts the
        rollout from, after the reset, into ``rnn_start["student"]`` (``(h, c)``, ``[N, H]`` each, ``c`` None for a GRU): what
        ``Distillation.update`` replays the rollout from.  The teacher's start state is not kept: the update never steps the teacher.
        On a backend without the entry (the test-only CPU oracle) this is the module's torch step, and ``noise`` is required."""
        if not isinstance(forward, RecurrentDistillForward):
            raise ValueError("act_distill_recurrent(forward, ...) takes a RecurrentDistillForward")
        return self._act_student_teacher(forward, obs, teacher_obs, noise)

    def keep_distill_rnn_start(self, policy) -> None:
        """``rnn_start["student"]`` from ``policy.memory_s`` — the state the rollout starts from, zeros where the memory has none yet:
        what a loop on the module's torch step calls before the first step of a rollout (``act_distill_recurrent`` does it inside its
        launch)."""
        self.rnn_start = {"student": _rnn_state_rows(policy.memory_s, self.env.num_envs, self.device)}

    def _act_distill_rows(self, mean: torch.Tensor, std: torch.Tensor, teacher_actions: torch.Tensor, noise: Optional[torch.Tensor] = None,
                          std_is_log: bool = False) -> torch.Tensor:
        """``act_distill`` from the two networks' outputs (the torch forwards of ``DistillationRunner(forward="torch")``): ``act``'s
        sampling — ``gf_policy_act`` with only the action row — and a copy of ``teacher_actions`` into ``privileged_actions[t]``."""
        n, dev = self.env.num_envs, self.device
        A = int(mean.shape[1])
        for x, name, shapes in ((mean, "mean", {(n, A)}), (std, "std", {(A,)}), (teacher_actions, "teacher_actions", {(n, A)})):
            _check_f32(x, name, shapes, dev)
        if noise is not None:
            _check_f32(noise, "noise", {(n, A)}, dev)
        self._ensure_distill_rows(A)
        t = self._act_row()
        actions = self._policy_act(mean, std, None, noise, std_is_log)
        with torch.no_grad():
            self.privileged_actions[t].copy_(teacher_actions)
        return actions

    def step_batches(self, with_dones: bool = False) -> Iterator[tuple]:
        """rsl_rl's distillation ``generator()``: for ``t = 0 … T-1`` in time order ``(obs_t, privileged_actions[t])`` — the policy
        group's observation of transition ``t`` and the teacher's actions ``act_distill`` stored for it.  Views of the stored rows, no
        gather launch; a group of several managers is concatenated per step, a frame-stored manager goes through
        ``observation_rows(name, t)``.  ``with_dones=True``: ``(obs_t, privileged_actions[t], dones[t])``, what a recurrent student's
        update resets its state by."""
        if self.privileged_actions is None:
            raise RuntimeError("step_batches() reads the teacher's actions: collect the rollout with act_distill() first")
        names = self.obs_groups["policy"]

        def rows(name, t):
            if name in self.frames:
                return self.observation_rows(name, t)
            return (self.observations if name == self.obs_name else self.group_rows[name])[t]

        for t in range(self.num_steps):
            obs = rows(names[0], t) if len(names) == 1 else torch.cat([rows(m, t) for m in names], dim=-1)
            if with_dones:
                yield obs, self.privileged_actions[t], self.dones[t]
            else:
                yield obs, self.privileged_actions[t]

    def _act_torch(self, mean, std, values, noise, actions, t, std_is_log: bool = False) -> None:
        """``gf_policy_act``'s row in torch (the test-only oracle backend); ``values=None``: only the action row."""
        with torch.no_grad():
            sampled, sd = _sample_torch(mean, std, noise, std_is_log)
            actions.copy_(sampled)
            self.actions[t].copy_(actions)
            if values is None:
                return
            d = actions - mean
            term = -(d * d) / (2 * (sd * sd)) - sd.log() - _LOG_SQRT_2PI
            lp = term[:, 0].clone()
            for c in range(1, term.shape[1]):   # (a left fold, as the kernel)
                lp = lp + term[:, c]
            self.mu[t].copy_(mean)
            self.sigma[t].copy_(sd)
            self.values[t].copy_(values.reshape(-1))
            self.actions_log_prob[t].copy_(lp)

    def process_env_step(self, time_outs: Optional[torch.Tensor], gamma: float = 0.99, episodes: Optional["EpisodeStatistics"] = None) -> None:
        """After ``env.step()``: for the transition it wrote (row ``step - 1``) update ``episodes`` from the raw ``rewards`` / ``dones``
        rows as rsl_rl's runner does, then bootstrap ``rewards[t] += (gamma * values[t]) * time_outs`` (PPO.process_env_step) —
        one ``gf_episode_step`` launch.  ``time_outs=None``: the statistics only.  The transition's policy rows must be in (``act``
        before the step or ``add_policy`` after it), and a row is bootstrapped once: after ``add_policy(..., time_outs=…)`` pass
        ``time_outs=None``."""
        if self.step < 1 or self._serial == 0:
            raise RuntimeError("process_env_step() follows the env.step() whose transition it completes")
        t = self.step - 1
        if self._pol_serial != self._serial:
            raise RuntimeError(f"process_env_step() needs the policy rows of transition {t}: call act() before env.step() or add_policy() after it")
        n, dev = self.env.num_envs, self.device
        if time_outs is not None:
            if self._boot_serial == self._serial:
                raise RuntimeError(f"the rewards of transition {t} are already bootstrapped (add_policy(time_outs=...) or process_env_step)")
            time_outs = _check_mask(time_outs, "time_outs", n, dev)
        if episodes is not None and episodes.num_envs != n:
            raise ValueError(f"episodes keeps {episodes.num_envs} envs, the storage {n}")
        self._proc_serial = self._serial
        if time_outs is None and episodes is None:
            return
        if time_outs is not None and self.values is None:
            raise RuntimeError("process_env_step(time_outs) bootstraps with the value rows: a rollout collected with act_distill() has none")
        rewards, dones = self.rewards[t], self.dones[t]
        values = None if self.values is None else self.values[t]   # (None: a distillation rollout — the statistics only)
        fn = getattr(self.env.backend, "episode_step", None)
        if fn is None:   # (the test-only oracle backend) the runner's and PPO's torch expressions
            if episodes is not None:
                episodes._update_torch(rewards, dones)
            if time_outs is not None:
                with torch.no_grad():
                    rewards.copy_(rewards + (float(gamma) * values) * time_outs.to(torch.float32))
        else:
            a = self._ep_args
            a.num_envs, a.rewards, a.dones = n, rewards.data_ptr(), dones.data_ptr()
            a.time_outs = None if time_outs is None else time_outs.data_ptr()
            a.values = None if time_outs is None else values.data_ptr()
            a.gamma = float(gamma)
            if episodes is not None:
                episodes._fill(a)
            else:
                a.cur_reward_sum = a.cur_episode_length = a.ring_reward = a.ring_length = a.ring_state = a.block_counts = None
            self._keep_ep = time_outs
            fn(a)
            if episodes is not None:
                episodes._calls += 1
        if time_outs is not None:
            self._boot_serial = self._serial

    def intrinsic_reward(self, rnd, rnd_state) -> torch.Tensor:
        """rsl_rl's RND lines of ``PPO.process_env_step`` for the transition the last ``env.step()`` wrote (row ``step - 1``):
        ``rewards[t] += rnd.get_intrinsic_reward(rnd_state)``; returns the intrinsic reward ``[N]``.  ``rnd``: a :class:`RndForward` —
        ONE ``gf_rnd_reward`` launch (two with the reward normaliser updating) for both MLPs, the distance, the normaliser, the weight
        and the row's add, no host read — or the :class:`RandomNetworkDistillation` itself: its torch lines.  ``rnd_state``: the
        post-step observation of the ``"rnd_state"`` group, a ``[N, W]`` tensor or its members as segments.  It comes after
        ``env.step()`` and before ``process_env_step`` (the episode statistics then see extrinsic + intrinsic, as rsl_rl's
        ``rewbuffer`` does, and the bootstrap is added to the sum); a second call for one transition raises ``RuntimeError``.
        ``rnd_sums`` ``[2, N]`` (float64, allocated here) accumulates the extrinsic and the intrinsic reward per env — the runner's
        per-iteration means; zero it to start a new window."""
        if not isinstance(rnd, (RndForward, RandomNetworkDistillation)):
            raise ValueError("intrinsic_reward(rnd, ...) takes a RndForward or a RandomNetworkDistillation")
        if self.step < 1 or self._serial == 0:
            raise RuntimeError("intrinsic_reward() follows the env.step() whose transition it completes")
        t = self.step - 1
        if self._rnd_serial == self._serial:
            raise RuntimeError(f"the rewards of transition {t} already hold their intrinsic reward")
        if self._proc_serial == self._serial or self._boot_serial == self._serial:
            raise RuntimeError(f"intrinsic_reward() comes before process_env_step(): transition {t} is already processed")
        n = self.env.num_envs
        if self.rnd_sums is None:
            self.rnd_sums = torch.zeros((2, n), device=self.device, dtype=torch.float64)
        rewards = self.rewards[t]
        if isinstance(rnd, RndForward):
            _segments(rnd_state, "rnd_state", n, self.device, rnd.target)
            out = rnd.reward(rnd_state, rewards, self.rnd_sums[0], self.rnd_sums[1], backend=self.env.backend)
        else:
            x = _cat(tuple(rnd_state) if isinstance(rnd_state, (list, tuple)) else rnd_state)
            _check_f32(x, "rnd_state", {(n, rnd.num_states)}, self.device, window=True)
            out = _rnd_reward_torch(rnd, x, rewards, self.rnd_sums[0], self.rnd_sums[1])
        self._rnd_serial = self._serial
        return out

    def group_rows_batch(self, group: str, indices: torch.Tensor, normalizer=None) -> torch.Tensor:
        """Rows ``indices`` (transition ``divmod(index, N)``, observation row ``t``) of observation group ``group`` as a fresh
        ``[mb, W]`` tensor, its members side by side — through ``normalizer`` (an :class:`EmpiricalNormalization` of the group's
        width; ``None`` / ``nn.Identity``: raw).  ONE ``gf_minibatch_gather`` launch over the members (frame-stored ones rebuilt from
        their frames, as the minibatch gather does); plain indexing on a backend without it (the test-only CPU oracle).  What
        :class:`PPO` reads the ``"rnd_state"`` rows of a minibatch with: ``MiniBatch`` keeps its ten fields."""
        names = self.obs_groups.get(group)
        if not names:
            raise ValueError(f"the storage follows no observation group '{group}'")
        w = sum(self._widths[k] for k in names)
        norm = _as_normalizer(normalizer, w, "normalizer")
        rows = self._flat_rows()
        T, n = self.num_steps, self.env.num_envs
        gather = getattr(self.env.backend, "minibatch_gather", None)
        if gather is None:
            for k in names:
                if k in self.frames:
                    rows[k] = self.observation_rows(k)[:T].reshape(T * n, self._widths[k])
            x = rows[names[0]][indices] if len(names) == 1 else torch.cat([rows[k][indices] for k in names], dim=-1)
            if norm is None:
                return x
            with torch.no_grad():
                return norm(x)
        if indices.dtype != torch.int64 or indices.dim() != 1 or not indices.is_contiguous() or indices.device != self.device:
            raise ValueError(f"indices must be a contiguous int64 [mb] tensor on {self.device}")
        m = int(indices.shape[0])
        out = torch.empty((m, w), device=self.device, dtype=torch.float32)
        a = self._grp_args
        a.num_rows, a.num_src_rows, a.indices = m, T * n, indices.data_ptr()
        col, at = 0, 0
        members = list(names)
        while at < len(members):   # (more members than one launch holds: a further launch)
            part = members[at:at + nat.GF_MINIBATCH_MAX_FIELDS]
            a.num_fields = len(part)
            for f, k in zip(a.fields, part):
                src = rows[k]
                H = self.frames[k].shape[0] - T if k in self.frames else 0
                f.src, f.dst, f.src_width, f.dst_width, f.dst_col = src.data_ptr(), out.data_ptr(), src.shape[1], w, col
                f.history_len, f.frame_stride_rows = H, n if H else 0
                if norm is None:
                    f.mean = f.std = None
                else:
                    f.mean, f.std, f.eps = norm._mean.data_ptr() + 4 * col, norm._std.data_ptr() + 4 * col, norm.eps
                col += self._widths[k]
            gather(a)
            at += len(part)
        self._keep_grp = indices
        return out

    def compute_returns(self, last_values: torch.Tensor, gamma: float = 0.99, lam: float = 0.95, normalize: bool = True) -> None:
        """``returns`` / ``advantages`` of the finished rollout (rsl_rl ``RolloutStorage.compute_returns``; gamma / lam as
        examples/simple/train.py:41-47) — GAE over the T steps, then ``(adv - mean) / (std + 1e-8)`` over all T*N entries.
        ``last_values``: the critic's value of the bootstrap observation — ``policy.evaluate(last_obs)``, or one launch with
        ``PolicyForward(policy).value(last_obs)``."""
        if self.values is None:
            raise RuntimeError("compute_returns() needs the value estimates: call add_policy() for every transition")
        last_values = last_values.reshape(-1).to(torch.float32).contiguous()
        g = self._gae_args
        g.num_envs, g.num_steps = self.env.num_envs, self.num_steps
        g.rewards, g.values, g.dones, g.last_values = self.rewards.data_ptr(), self.values.data_ptr(), self.dones.data_ptr(), last_values.data_ptr()
        g.gamma, g.lam = float(gamma), float(lam)
        g.returns, g.advantages, g.moments = self.returns.data_ptr(), self.advantages.data_ptr(), self._moments.data_ptr()
        g.normalize = 1 if normalize else 0
        self._keep_gae = last_values
        self.env.backend.call("gae", g, owner=None)
        self._returns_ready = True

    # -- PPO minibatches ------------------------------------------------------------------------------------------------------------
    def mini_batch_generator(self, num_mini_batches: int, num_epochs: int = 1, generator: Optional[torch.Generator] = None,
                             obs_normalizer=None, critic_obs_normalizer=None) -> Iterator[MiniBatch]:
        """rsl_rl's ``RolloutStorage.mini_batch_generator``: ONE ``torch.randperm(num_mini_batches * mb)`` (``mb = T·N //
        num_mini_batches``; the remainder rows are never drawn) shared by all ``num_epochs`` epochs; minibatch ``i`` is rows
        ``indices[i·mb:(i+1)·mb]`` of every flattened ``[T·N, …]`` array, source row ``k`` being transition ``divmod(k, N)``.
        Each batch is gathered by one ``gf_minibatch_gather`` launch into fresh tensors (a consumer may keep a batch); the
        critic input is the concatenation of its group's members, written side by side by the same launch, and is ``obs`` itself
        when the two groups are the same (and so are the two normaliser objects).
        ``obs_normalizer`` / ``critic_obs_normalizer``: an :class:`EmpiricalNormalization` of the group's width (``None`` /
        ``nn.Identity``: none) — the batch's ``obs`` / ``critic_obs`` then come out as ``normalizer(rows)``, from the same single
        launch.  The storage itself keeps the raw observations, as rsl_rl's does."""
        if not self._returns_ready:
            raise RuntimeError("mini_batch_generator() reads returns and advantages: call compute_returns() first")
        num_mini_batches, num_epochs = int(num_mini_batches), int(num_epochs)
        T, n = self.num_steps, self.env.num_envs
        if num_mini_batches < 1 or num_epochs < 0:
            raise ValueError("num_mini_batches must be >= 1 and num_epochs >= 0")
        mb = (T * n) // num_mini_batches
        if mb < 1:
            raise ValueError(f"{T * n} transitions cannot fill {num_mini_batches} minibatches")
        width = lambda group: sum(self._widths[m] for m in self.obs_groups[group])
        norms = (_as_normalizer(obs_normalizer, width("policy"), "obs_normalizer"),
                 _as_normalizer(critic_obs_normalizer, width("critic"), "critic_obs_normalizer"))
        indices = torch.randperm(num_mini_batches * mb, device=gs.device, generator=generator)
        return self._mini_batches(indices, num_mini_batches, num_epochs, mb, norms)

    def _mini_batches(self, indices: torch.Tensor, num_mini_batches: int, num_epochs: int, mb: int, norms=(None, None)) -> Iterator[MiniBatch]:
        for _epoch in range(num_epochs):
            for i in range(num_mini_batches):
                yield self._gather(indices[i * mb:(i + 1) * mb], *norms)

    # -- trajectory minibatches (a recurrent policy's update) ----------------------------------------------------------------------------
    def recurrent_mini_batch_generator(self, num_mini_batches: int, num_epochs: int = 1, norms=(None, None)) -> Iterator["RecurrentMiniBatch"]:
        """rsl_rl's ``recurrent_mini_batch_generator``: the rollout cut into trajectories at the dones (``dones[T-1]`` counts as set),
        enumerated env-major; minibatch ``i`` is the envs ``[i·N // num_mini_batches, (i+1)·N // num_mini_batches)`` — contiguous,
        not shuffled, the same in every epoch — as padded ``[T, ntraj, W]`` observation sequences through ``norms`` (the actor's and
        the critic's :class:`EmpiricalNormalization` or None; padding stays zero), their masks, the initial hidden states and the
        int64 index the policy's batch mode un-pads with.  ``gf_traj_table`` runs once (and ONE host read fetches the
        ``num_mini_batches + 1`` trajectory offsets); every minibatch is one ``gf_traj_gather`` and one ``gf_minibatch_gather`` (the
        per-row fields, rows ``t·N + n`` in ``(t, env)`` order).

        The initial state of a trajectory is the rollout-start state ``act_recurrent`` saved (``rnn_start``) where it starts at
        ``t = 0``, zeros elsewhere — a later start lies behind a done; rsl_rl stores the state of every step to read the same values.
        ``history="frames"`` storage is refused (``ValueError``).  On a backend without the entries (the test-only oracle) the same
        batches come from rsl_rl's lines: ``nonzero``, ``torch.split``, ``pad_sequence``."""
        if not self._returns_ready:
            raise RuntimeError("recurrent_mini_batch_generator() reads returns and advantages: call compute_returns() first")
        if self.frames:
            raise ValueError('recurrent_mini_batch_generator: history="frames" storage is not supported (trajectories are gathered from observation rows)')
        start = getattr(self, "rnn_start", None)
        if not start:
            raise RuntimeError("recurrent_mini_batch_generator() needs the rollout-start hidden states: collect with act_recurrent()")
        M, num_epochs = int(num_mini_batches), int(num_epochs)
        T, n = self.num_steps, self.env.num_envs
        if M < 1 or M > n or num_epochs < 0:
            raise ValueError(f"num_mini_batches must be 1 … num_envs ({n}) and num_epochs >= 0")
        width = lambda group: sum(self._widths[m] for m in self.obs_groups[group])
        norms = (_as_normalizer(norms[0], width("policy"), "obs_normalizer"), _as_normalizer(norms[1], width("critic"), "critic_obs_normalizer"))
        bounds = [i * n // M for i in range(M + 1)]
        if getattr(self.env.backend, "traj_table", None) is None:
            return self._recurrent_batches_torch(bounds, num_epochs, norms, start)
        dev = self.device
        key = (T, n, M)
        if getattr(self, "_traj_key", None) != key:
            self._traj_counts = torch.empty(n, device=dev, dtype=torch.int32)
            self._traj_offsets = torch.empty(n + 1, device=dev, dtype=torch.int32)
            self._traj_table = torch.empty((T * n, 3), device=dev, dtype=torch.int32)
            self._traj_bounds = torch.tensor(bounds, device=dev, dtype=torch.int64)
            self._traj_rows = (torch.arange(T, device=dev) * n)[:, None] + torch.arange(n, device=dev)[None, :]   # [T, N]: row t·N + n
            self._traj_key = key
        a = nat.GfTrajTableArgs()
        a.num_steps, a.num_envs, a.dones = T, n, self.dones.data_ptr()
        a.counts, a.offsets, a.table = self._traj_counts.data_ptr(), self._traj_offsets.data_ptr(), self._traj_table.data_ptr()
        self.env.backend.traj_table(a)
        offs = self._traj_offsets.index_select(0, self._traj_bounds).tolist()   # the one host read
        return self._recurrent_batches_hip(bounds, offs, num_epochs, norms, start)

    def _recurrent_batches_hip(self, bounds, offs, num_epochs: int, norms, start) -> Iterator["RecurrentMiniBatch"]:
        T, n, dev = self.num_steps, self.env.num_envs, self.device
        rows = self._flat_rows()
        policy, critic = self.obs_groups["policy"], self.obs_groups["critic"]
        same = list(critic) == list(policy) and norms[1] is norms[0]
        a = nat.GfTrajGatherArgs()
        a.num_steps, a.num_envs, a.table, a.table_rows = T, n, self._traj_table.data_ptr(), offs[-1]
        for g, names, norm in zip(a.groups, (policy, critic), norms):
            g.num_inputs, g.width = len(names), sum(self._widths[k] for k in names)
            for seg, k in zip(g.inputs, names):
                seg.rows, seg.width, seg.row_stride = rows[k].data_ptr(), self._widths[k], rows[k].stride(0)
            if norm is not None:
                g.mean, g.std, g.eps = norm._mean.data_ptr(), norm._std.data_ptr(), norm.eps
        if same:
            a.groups[1].width = 0
        for st, name in zip(a.states, ("actor", "critic")):
            h, c = start[name]
            st.hidden, st.h_start, st.c_start = h.shape[1], h.data_ptr(), None if c is None else c.data_ptr()
        for _epoch in range(num_epochs):
            for i in range(len(bounds) - 1):
                e0, e1, J = bounds[i], bounds[i + 1], offs[i + 1] - offs[i]
                a.first_traj, a.num_traj, a.env_start, a.num_mb_envs = offs[i], J, e0, e1 - e0
                obs = torch.empty((T, J, a.groups[0].width), device=dev, dtype=torch.float32)
                critic_obs = obs if same else torch.empty((T, J, a.groups[1].width), device=dev, dtype=torch.float32)
                masks = torch.empty((T, J), device=dev, dtype=torch.bool)
                index = torch.empty((e1 - e0) * T, device=dev, dtype=torch.int64)
                a.groups[0].dst, a.groups[1].dst = obs.data_ptr(), None if same else critic_obs.data_ptr()
                a.masks, a.unpad_index = masks.data_ptr(), index.data_ptr()
                hid = []
                for st, name in zip(a.states, ("actor", "critic")):
                    h, c = start[name]
                    h0 = torch.empty((1, J, h.shape[1]), device=dev, dtype=torch.float32)
                    c0 = None if c is None else torch.empty_like(h0)
                    st.h0, st.c0 = h0.data_ptr(), None if c0 is None else c0.data_ptr()
                    hid.append(h0 if c0 is None else (h0, c0))
                self.env.backend.traj_gather(a)
                per = self._gather(self._traj_rows[:, e0:e1].reshape(-1), fields_only=True)
                yield RecurrentMiniBatch(obs, critic_obs, masks, hid[0], hid[1], index, per)

    def _recurrent_batches_torch(self, bounds, num_epochs: int, norms, start) -> Iterator["RecurrentMiniBatch"]:
        """rsl_rl's lines (``split_and_pad_trajectories``, ``recurrent_mini_batch_generator``) on the stored rows."""
        T, n = self.num_steps, self.env.num_envs
        rows = self._flat_rows()

        def group(names, norm):
            x = rows[names[0]] if len(names) == 1 else torch.cat([rows[m] for m in names], dim=-1)
            if norm is not None:
                with torch.no_grad():
                    x = norm(x)
            return x.reshape(T, n, -1)

        dones = self.dones.clone()
        dones[-1] = True
        flat_dones = dones.transpose(1, 0).reshape(-1, 1)
        done_indices = torch.cat((flat_dones.new_tensor([-1], dtype=torch.int64), flat_dones.nonzero()[:, 0]))
        trajectory_lengths = done_indices[1:] - done_indices[:-1]
        lengths = trajectory_lengths.tolist()

        def split_and_pad(tensor):
            trajectories = torch.split(tensor.transpose(1, 0).flatten(0, 1), lengths)
            trajectories = trajectories + (torch.zeros(tensor.shape[0], *tensor.shape[2:], device=tensor.device),)
            return torch.nn.utils.rnn.pad_sequence(trajectories)[:, :-1]

        policy, critic = self.obs_groups["policy"], self.obs_groups["critic"]
        same = list(critic) == list(policy) and norms[1] is norms[0]
        padded_obs = split_and_pad(group(policy, norms[0]))
        padded_critic = padded_obs if same else split_and_pad(group(critic, norms[1]))
        trajectory_masks = trajectory_lengths > torch.arange(0, T, device=dones.device).unsqueeze(1)
        starts = done_indices[:-1] + 1                   # env-major flat index e·T + t of every trajectory's first step
        env, t0 = starts // T, starts % T
        per_env = torch.bincount(env, minlength=n).cumsum(0)
        first = [0] + per_env.tolist()
        tn = (torch.arange(T) * n)[:, None] + torch.arange(n)[None, :]
        for _epoch in range(num_epochs):
            for i in range(len(bounds) - 1):
                e0, e1 = bounds[i], bounds[i + 1]
                j0, j1 = first[e0], first[e1]
                masks = trajectory_masks[:, j0:j1]
                hid = []
                for name in ("actor", "critic"):
                    state = tuple(torch.where((t0[j0:j1] == 0)[:, None], s[env[j0:j1]], torch.zeros(())).unsqueeze(0).contiguous()
                                  for s in start[name] if s is not None)
                    hid.append(state if len(state) == 2 else state[0])
                index = masks.transpose(1, 0).reshape(-1).nonzero()[:, 0]
                per = self._gather(tn[:, e0:e1].reshape(-1).to(self.device), fields_only=True)
                yield RecurrentMiniBatch(padded_obs[:, j0:j1], padded_critic[:, j0:j1], masks, hid[0], hid[1], index, per)

    def _flat(self) -> dict:
        """Every stored array as its ``[T·N, w]`` source rows (views); a frame-stored manager as its ``[(T+H)·N, O]`` frames, of which
        row ``t·N + n`` is the OLDEST frame of observation row ``t`` (its newer frames lie multiples of N rows further on)."""
        per = {k: getattr(self, k).flatten(0, 1) for k in _MB_FIELDS}   # ([T·N] or [T·N, A])
        return self._flat_rows(), per

    def _flat_rows(self) -> dict:
        """The observation half of ``_flat``: a storage without policy rows has it too."""
        T, n = self.num_steps, self.env.num_envs
        rows = {name: r[:T].view(T * n, r.shape[2]) for name, r in self.group_rows.items()}
        if self.obs_name not in rows and self.observations is not None:
            rows[self.obs_name] = self.observations[:T].view(T * n, self.obs_width)
        for name, F in self.frames.items():
            rows[name] = F.view(F.shape[0] * n, F.shape[2])
        return rows

    def _gather(self, idx: torch.Tensor, obs_norm=None, critic_norm=None, fields_only: bool = False) -> MiniBatch:
        """``fields_only``: the per-row fields alone (``obs`` / ``critic_obs`` None) — a recurrent update reads its observations as
        padded trajectories."""
        rows, per = self._flat()
        policy, critic = self.obs_groups["policy"], self.obs_groups["critic"]
        same = list(critic) == list(policy) and critic_norm is obs_norm
        gather = getattr(self.env.backend, "minibatch_gather", None)
        if gather is None:   # (the test-only oracle backend) rsl_rl's expression itself, on the materialised rows of a frame-stored manager
            T, n = self.num_steps, self.env.num_envs
            for k in self.frames:
                rows[k] = self.observation_rows(k)[:T].reshape(T * n, self._widths[k])

            def cat(names, norm):
                x = rows[names[0]][idx] if len(names) == 1 else torch.cat([rows[m][idx] for m in names], dim=-1)
                if norm is None:
                    return x
                with torch.no_grad():
                    return norm(x)

            if fields_only:
                return MiniBatch(None, None, *(per[k][idx] for k in _MB_FIELDS), idx)
            obs = cat(policy, obs_norm)
            return MiniBatch(obs, obs if same else cat(critic, critic_norm), *(per[k][idx] for k in _MB_FIELDS), idx)
        m = idx.shape[0]
        dev = self.device
        empty = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
        fields = []   # (source rows [T·N, w] or frames, destination, its width, first column, the group's normaliser or None, H or 0)
        frames, widths = self.frames, self._widths

        def group(names, norm):
            w = sum(widths[k] for k in names)
            out, col = empty(m, w), 0
            for k in names:
                fields.append((rows[k], out, w, col, norm, frames[k].shape[0] - self.num_steps if k in frames else 0))
                col += widths[k]
            return out

        obs = None if fields_only else group(policy, obs_norm)
        critic_obs = obs if same or fields_only else group(critic, critic_norm)
        outs = []
        for k in _MB_FIELDS:
            src = per[k]
            outs.append(empty(m, *src.shape[1:]))
            fields.append((src, outs[-1], src.shape[1] if src.dim() == 2 else 1, 0, None, 0))
        a = self._mb_args
        a.num_rows, a.num_src_rows, a.indices = m, self.num_steps * self.env.num_envs, idx.data_ptr()
        for at in range(0, len(fields), nat.GF_MINIBATCH_MAX_FIELDS):   # (more members than one launch holds: a further launch)
            part = fields[at:at + nat.GF_MINIBATCH_MAX_FIELDS]
            a.num_fields = len(part)
            for f, (src, dst, w, col, norm, H) in zip(a.fields, part):
                f.src, f.dst, f.src_width, f.dst_width, f.dst_col = src.data_ptr(), dst.data_ptr(), src.numel() // src.shape[0], w, col
                if frames:   # (a history field is rebuilt from its H frames; a row storage leaves the two words zero: plain fields)
                    f.history_len, f.frame_stride_rows = H, self.env.num_envs if H else 0
                if norm is not None:   # (the member's slice of the group's normaliser)
                    f.mean, f.std, f.eps = norm._mean.data_ptr() + 4 * col, norm._std.data_ptr() + 4 * col, norm.eps
                elif self._mb_normed:
                    f.mean = f.std = None
            normed = obs_norm is not None or critic_norm is not None
            if self._mb_normed and not normed:   # (the slots past this part may still hold a pointer of an earlier call)
                for f in a.fields:
                    f.mean = f.std = None
            self._mb_normed = normed
            gather(a)
        return MiniBatch(obs, critic_obs, *outs, idx)

    def _trace_patch(self, args, via_unroll=None):
        """Recorded step: advance the rows.  ``via_unroll`` = the policy ObservationManager when it keeps its history as a ring and
        the step is fused: the fused launch only holds the new frame, so the observation row is written by the manager's gather
        (second destination of gf_history_unroll) and the fused launch gets no observation row."""
        if self.observations is None:   # (frame-stored: no observation row, from the launch or from the gather)
            via_unroll = None

        def patch(_actions, a=args, self=self, om=via_unroll):
            self._next_rows(a)
            if om is not None:
                om._unroll_args.out2, a.obs_out = a.obs_out, None

        return patch

    def _trace_native(self, args, pol, fused: bool) -> list:
        """`obs` follows the tensor the observation launch (or the gather of a ring-kept history) writes this step — that
        manager's rotation comes earlier in the table."""
        P = nat.GfReplayPatch
        if self.observations is None:   # frame-stored: the launch stores no observation row (obs_out stays NULL), `obs` is not read
            args.obs = None
            return []
        if getattr(pol, "_window", False):
            from ._trace import Untraceable
            raise Untraceable("the rollout rows of a window-mode observation (a strided view) cannot be copied by the step's launch")
        if getattr(pol, "_unrolled", False):
            return [] if fused else [P(nat.GF_PATCH_COPY, 0, nat.field_addr(args, "obs"), None, nat.field_addr(pol._unroll_args, "out"))]
        return [P(nat.GF_PATCH_COPY, 0, nat.field_addr(args, "obs"), None, nat.field_addr(pol._args, "obs"))]


class EpisodeStatistics:
    """rsl_rl ``OnPolicyRunner.learn``'s episode bookkeeping, kept on the device: ``cur_reward_sum`` / ``cur_episode_length``
    (``[N]`` float32) and the last ``window`` finished returns and lengths (``rewbuffer`` / ``lenbuffer``, ``deque(maxlen=
    window)``) as a ring.  Every step: ``cur_reward_sum += rewards``, ``cur_episode_length += 1``; every done env appends its two
    values in ascending env order, then both are zeroed.  ``update`` (or ``RolloutStorage.process_env_step(..., episodes=)``)
    is one ``gf_episode_step`` launch with no host synchronisation; the reads below synchronise — once per log interval."""

    def __init__(self, num_envs: int, window: int = 100, device=None):
        if int(num_envs) < 1 or int(window) < 1:
            raise ValueError("EpisodeStatistics needs num_envs >= 1 and window >= 1")
        self.num_envs, self.window = int(num_envs), int(window)
        dev = torch.device(gs.device if device is None else device)
        z = lambda k, dt=torch.float32: torch.zeros(k, device=dev, dtype=dt)
        self.cur_reward_sum, self.cur_episode_length = z(self.num_envs), z(self.num_envs)
        self.ring_reward, self.ring_length = z(self.window), z(self.window)
        self.ring_state = z(4, torch.int32)   # [2][2] {head, fill}: a launch reads slot _calls & 1 and writes the other
        big = self.num_envs > nat.GF_EPISODE_SINGLE_MAX
        self._block_counts = z(-(-self.num_envs // nat.GF_EPISODE_BLOCK_ENVS), torch.int32) if big else None
        self._calls = 0
        self._args = nat.GfEpisodeArgs()

    @property
    def device(self) -> torch.device:
        return self.cur_reward_sum.device

    def _fill(self, a) -> None:
        """Point the statistics fields of a GfEpisodeArgs at these tensors."""
        a.cur_reward_sum, a.cur_episode_length = self.cur_reward_sum.data_ptr(), self.cur_episode_length.data_ptr()
        a.ring_reward, a.ring_length, a.ring_state = self.ring_reward.data_ptr(), self.ring_length.data_ptr(), self.ring_state.data_ptr()
        a.block_counts = None if self._block_counts is None else self._block_counts.data_ptr()
        a.window, a.parity = self.window, self._calls & 1

    def update(self, rewards: torch.Tensor, dones: torch.Tensor) -> None:
        """One step of the runner's bookkeeping from this step's ``rewards`` (``[N]`` float32, before any bootstrap) and ``dones``
        (``[N]``; bool / uint8, anything else is compared with 0), for loops without a :class:`RolloutStorage`.  One launch."""
        n, dev = self.num_envs, self.device
        if not isinstance(rewards, torch.Tensor) or rewards.dtype != torch.float32 or rewards.device != dev or rewards.numel() != n:
            raise ValueError(f"rewards must be a [{n}] float32 tensor on {dev}")
        rewards = rewards.reshape(n)
        if not rewards.is_contiguous():
            raise ValueError("rewards must be contiguous")
        dones = _check_mask(dones, "dones", n, dev)
        fn = getattr(nat.get_backend(), "episode_step", None)
        if fn is None:   # (the test-only oracle backend)
            self._update_torch(rewards, dones)
            return
        a = self._args
        a.num_envs, a.rewards, a.dones, a.time_outs, a.values, a.gamma = n, rewards.data_ptr(), dones.data_ptr(), None, None, 0.0
        self._fill(a)
        self._keep = (rewards, dones)
        fn(a)
        self._calls += 1

    def _update_torch(self, rewards: torch.Tensor, dones: torch.Tensor) -> None:
        """The runner's lines themselves (``nonzero`` and a host copy per step), for the CPU oracle backend."""
        with torch.no_grad():
            self.cur_reward_sum += rewards
            self.cur_episode_length += 1
            ids = (dones != 0).nonzero()[:, 0]
            k, W = int(ids.numel()), self.window
            head, fill = self._state()
            if k:
                keep = ids[max(0, k - W):]
                pos = (head + torch.arange(k - keep.numel(), k, device=ids.device)) % W
                self.ring_reward[pos] = self.cur_reward_sum[keep]
                self.ring_length[pos] = self.cur_episode_length[keep]
                self.cur_reward_sum[ids] = 0
                self.cur_episode_length[ids] = 0
            nxt = 1 - (self._calls & 1)
            self.ring_state[2 * nxt] = (head + k) % W
            self.ring_state[2 * nxt + 1] = min(fill + k, W)
        self._calls += 1

    def _state(self):
        head, fill = self.ring_state[2 * (self._calls & 1):2 * (self._calls & 1) + 2].tolist()
        return int(head), int(fill)

    def _ring(self, ring: torch.Tensor) -> List[float]:
        head, fill = self._state()
        if fill == 0:
            return []
        vals = ring.tolist()
        start = (head - fill) % self.window
        return [vals[(start + i) % self.window] for i in range(fill)]

    @property
    def rewbuffer(self) -> List[float]:
        """The finished returns, oldest first (rsl_rl's ``rewbuffer`` deque as a list)."""
        return self._ring(self.ring_reward)

    @property
    def lenbuffer(self) -> List[float]:
        """The matching episode lengths, oldest first (rsl_rl's ``lenbuffer``)."""
        return self._ring(self.ring_length)

    def mean_reward(self) -> Optional[float]:
        """``statistics.mean(rewbuffer)`` — the runner's "Mean reward" — or None while no episode has finished."""
        buf = self.rewbuffer
        return statistics.mean(buf) if buf else None

    def mean_episode_length(self) -> Optional[float]:
        """``statistics.mean(lenbuffer)`` — "Mean episode length" — or None while no episode has finished."""
        buf = self.lenbuffer
        return statistics.mean(buf) if buf else None

    def reset(self) -> None:
        for x in (self.cur_reward_sum, self.cur_episode_length, self.ring_reward, self.ring_length, self.ring_state):
            x.zero_()
        self._calls = 0


def _cat(x) -> torch.Tensor:
    """An observation as one tensor: itself, or its segments side by side (the only one as it is)."""
    if isinstance(x, torch.Tensor):
        return x
    return x[0] if len(x) == 1 else torch.cat(x, dim=-1)


def _sample_torch(mean, std, noise, std_is_log: bool) -> tuple:
    """``(mean + sigma · noise, sigma)``, ``sigma`` = ``std`` (``exp(std)`` where it is a log_std) expanded to ``mean``: the kernels'
    sampling expression in torch, for the test-only oracle backend."""
    sd = (std.exp() if std_is_log else std).expand_as(mean)
    return mean + sd * noise, sd


def _rnn_state_rows(memory, n: int, dev, empty: bool = False) -> tuple:
    """``(h, c)``, ``[n, H]`` each (``c`` None for a GRU): copies of the state ``memory`` (an ``rnn`` and its ``hidden_states``) holds —
    ``h[0].clone()``, ``c[0].clone()`` — zeros where it has none yet; ``empty``: rows of that shape for a launch to write."""
    rnn, hs = memory.rnn, memory.hidden_states
    if empty:
        row = lambda i: torch.empty((n, rnn.hidden_size), device=dev, dtype=torch.float32)
    elif hs is None:
        row = lambda i: torch.zeros((n, rnn.hidden_size), device=dev)
    else:
        row = lambda i: (hs[i] if isinstance(hs, tuple) else hs)[0].detach().clone()
    return row(0), (row(1) if isinstance(rnn, torch.nn.LSTM) else None)


def _segments(obs, name: str, n: Optional[int], dev, layers=None, norm_width: Optional[int] = None) -> tuple:
    """``obs`` as the tuple of ``[n, w]`` float32 segments that are read side by side (``act``'s rules: nothing is cast) — contiguous,
    or the strided view a window-mode ObservationManager handed out (``_rows_ok``).  The reader is the first layer of ``layers``
    (``[(weight, bias)]``), or a normaliser of ``norm_width`` columns; ``n`` / ``dev`` ``None``: the first segment's."""
    parts = (obs,) if isinstance(obs, torch.Tensor) else tuple(obs) if isinstance(obs, (list, tuple)) else None
    if not parts or len(parts) > nat.GF_MLP_MAX_INPUTS:
        raise ValueError(f"{name} must be a tensor or a sequence of 1 to {nat.GF_MLP_MAX_INPUTS} tensors")
    for i, x in enumerate(parts):
        what = f"{name}[{i}]" if len(parts) > 1 else name
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] < 1:
            raise ValueError(f"{what} must be a [N, W] tensor")
        if layers is None and not _rows_ok(x):
            raise ValueError(f"EmpiricalNormalization reads contiguous observation rows: {what} is a strided view (only the window an "
                             "ObservationManager with output='window' hands out is read in place)")
        n = int(x.shape[0]) if n is None else n
        dev = x.device if dev is None else dev
        _check_f32(x, what, {(n, int(x.shape[1]))}, dev, window=True)
    want = norm_width if layers is None else int(layers[0][0].shape[1])
    if sum(int(x.shape[1]) for x in parts) != want:
        reader = f"the normaliser keeps {want} columns" if layers is None else f"the first layer reads {want}"
        raise ValueError(f"{name} is {' + '.join(str(int(x.shape[1])) for x in parts)} wide; {reader}")
    if layers is not None and layers[0][0].device != parts[0].device:
        raise ValueError(f"{name} lives on {parts[0].device}, the policy on {layers[0][0].device}")
    return parts


class _NormScratch:
    """The native descriptor and the workspace of a module's ``gf_obs_norm_update`` calls: call-to-call scratch, so a copy or a
    pickle of the module starts with a fresh one (a ctypes struct that holds pointers can be neither copied nor pickled)."""

    def __init__(self):
        self.args = nat.GfObsNormArgs()
        self.workspace = None

    def __deepcopy__(self, memo):
        return _NormScratch()

    def __reduce__(self):
        return (_NormScratch, ())


class EmpiricalNormalization(torch.nn.Module):
    """rsl_rl's ``EmpiricalNormalization``: ``forward(x) = (x - mean) / (std + eps)`` with the running mean / variance of every batch
    ``update`` has seen.  The buffers carry rsl_rl's names and shapes (``_mean`` / ``_var`` / ``_std`` ``[1, W]``, ``count`` an int64
    scalar), so its checkpoints load.  ``until``: no update once ``count >= until``.

    ``update(x)`` takes a ``[N, W]`` tensor or a sequence of up to four segments side by side (an observation group's members, no
    ``torch.cat``); float32, contiguous (or the strided view a window-mode ObservationManager handed out, read in place), on the buffers'
    device — nothing is cast.  No-op in eval mode.  On the HIP backend it is one
    ``gf_obs_norm_update`` (two launches) that writes the buffers in place and never reads the device from the host, the ``until``
    test included; the batch moments and the update are evaluated in float64 and rounded to float32 once, so the buffers agree with
    rsl_rl's float32 lines to rounding, not bit for bit.  For CPU tensors, or on a backend without the entry point (the test-only CPU
    oracle), rsl_rl's lines run in torch.  ``ActorCriticMLP.update_normalization`` updates the actor's and the critic's in one call.
    The statistics are rank-local, as rsl_rl's: nothing averages them across the ranks of a multi-GPU run."""

    def __init__(self, shape, eps: float = 1e-2, until: Optional[int] = None):
        super().__init__()
        width = int(shape) if isinstance(shape, int) else (int(shape[0]) if len(shape) == 1 else None)
        if width is None or width < 1:
            raise ValueError(f"EmpiricalNormalization keeps one row of statistics: shape={shape!r} must be W or (W,), W >= 1")
        self.width, self.eps, self.until = width, float(eps), until
        self.register_buffer("_mean", torch.zeros(width).unsqueeze(0))
        self.register_buffer("_var", torch.ones(width).unsqueeze(0))
        self.register_buffer("_std", torch.ones(width).unsqueeze(0))
        self.register_buffer("count", torch.tensor(0, dtype=torch.long))
        self._scratch = _NormScratch()

    @property
    def mean(self) -> torch.Tensor:
        return self._mean.squeeze(0).clone()

    @property
    def std(self) -> torch.Tensor:
        return self._std.squeeze(0).clone()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return (x - self._mean) / (self._std + self.eps)

    def inverse(self, y: torch.Tensor) -> torch.Tensor:
        return y * (self._std + self.eps) + self._mean

    def update(self, x) -> None:
        if not self.training:
            return
        _update_normalizers([(self, _segments(x, "x", None, self._mean.device, norm_width=self.width))], self._scratch.args)

    def _update_torch(self, x: torch.Tensor) -> None:
        """rsl_rl's lines."""
        if self.until is not None and self.count >= self.until:
            return
        with torch.no_grad():
            count_x = x.shape[0]
            self.count += count_x
            rate = count_x / self.count
            var_x = torch.var(x, dim=0, unbiased=False, keepdim=True)
            mean_x = torch.mean(x, dim=0, keepdim=True)
            delta_mean = mean_x - self._mean
            self._mean += rate * delta_mean
            self._var += rate * (var_x - self._var + delta_mean * (mean_x - self._mean))
            self._std = torch.sqrt(self._var)

    def _fill(self, st, parts) -> None:
        """Point set ``st`` of a GfObsNormArgs at the segments, the buffers and this normaliser's workspace."""
        n, dev = int(parts[0].shape[0]), self._mean.device
        need = max(1, nat.obs_norm_workspace_bytes(n, self.width) // 8)
        ws = self._scratch.workspace
        if ws is None or ws.numel() < need or ws.device != dev:
            ws = self._scratch.workspace = torch.empty(need, device=dev, dtype=torch.float64)
        for b in (self._mean, self._var, self._std):
            if b.dtype != torch.float32 or not b.is_contiguous():
                raise ValueError("EmpiricalNormalization: the kernel updates float32 contiguous buffers in place")
        st.num_inputs = len(parts)
        for seg, t in zip(st.inputs, parts):
            seg.rows, seg.width, seg.row_stride = t.data_ptr(), t.shape[1], 0 if t.is_contiguous() else t.stride(0)
        st.mean, st.var, st.std, st.count = self._mean.data_ptr(), self._var.data_ptr(), self._std.data_ptr(), self.count.data_ptr()
        st.until = -1 if self.until is None else int(self.until)
        st.workspace, st.workspace_bytes = ws.data_ptr(), ws.numel() * 8


def _update_normalizers(pairs, args) -> None:
    """``[(normaliser, segments)]`` (at most GF_OBS_NORM_MAX_SETS, the same number of rows each) in one ``gf_obs_norm_update`` — or, for
    CPU tensors and on a backend without it, rsl_rl's torch lines per normaliser."""
    if not pairs:
        return
    n = int(pairs[0][1][0].shape[0])
    if any(int(parts[0].shape[0]) != n for _, parts in pairs):
        raise ValueError("the normalisers of one update read the same number of rows")
    fn = getattr(nat.get_backend(), "obs_norm_update", None) if pairs[0][1][0].device.type == "cuda" else None
    if fn is None:
        for norm, parts in pairs:
            norm._update_torch(_cat(parts))
        return
    args.num_rows, args.num_sets = n, len(pairs)
    for st, (norm, parts) in zip(args.sets, pairs):
        norm._fill(st, parts)
    fn(args)   # (the segments are the caller's tensors; the launches are on the current stream, in front of whatever frees them)


def _as_normalizer(m, width: int, what: str) -> Optional["EmpiricalNormalization"]:
    """``m`` as the EmpiricalNormalization of ``width`` columns it is, or None for ``None`` / ``nn.Identity``; anything else: ValueError."""
    if m is None or isinstance(m, torch.nn.Identity):
        return None
    if not isinstance(m, EmpiricalNormalization):
        raise ValueError(f"{what} is {type(m).__name__}; only EmpiricalNormalization or nn.Identity can be folded into the kernels")
    if m.width != width:
        raise ValueError(f"{what} keeps {m.width} columns; its input is {width} wide")
    return m


def _mlp(sizes) -> torch.nn.Sequential:
    """``Linear(sizes[i], sizes[i + 1])`` layers with ``ELU`` between them and nothing after the last."""
    layers = []
    for i in range(len(sizes) - 1):
        layers.append(torch.nn.Linear(sizes[i], sizes[i + 1]))
        if i < len(sizes) - 2:
            layers.append(torch.nn.ELU())
    return torch.nn.Sequential(*layers)


class EmpiricalDiscountedVariationNormalization(torch.nn.Module):
    """rsl_rl's ``EmpiricalDiscountedVariationNormalization``: a reward is divided by the running std of a per-env discounted sum of
    the rewards seen so far.  ``emp_norm`` is an :class:`EmpiricalNormalization` of width 1 (its buffers are the state dict);
    ``avg`` ``[N]`` is the discounted sum — not part of the state dict: ``None`` until the first call, and again after a load.
    Training mode: ``avg = rew`` on the first call, ``avg * gamma + rew`` after it, then ``emp_norm`` is updated with the ``N`` values
    of ``avg`` as one batch (``until`` included).  Either mode: ``rew / emp_norm._std`` if that std is positive, else ``rew`` — no eps
    in the division.  ``gamma`` is the normaliser's own, not PPO's.  This ``forward`` is the torch path (one host read, the ``if``);
    the HIP path is ``gf_rnd_reward`` (:class:`RndForward`), which reads ``avg`` and the buffers in place."""

    def __init__(self, shape=(), eps: float = 1e-2, gamma: float = 0.99, until: Optional[int] = None):
        super().__init__()
        self.emp_norm = EmpiricalNormalization(1, eps=eps, until=until)
        self.gamma = float(gamma)
        self.avg: Optional[torch.Tensor] = None

    def forward(self, rew: torch.Tensor) -> torch.Tensor:
        if self.training:
            with torch.no_grad():
                self.avg = rew.clone() if self.avg is None else self.avg * self.gamma + rew
                self.emp_norm._update_torch(self.avg.reshape(-1, 1))
        std = self.emp_norm._std.reshape(())
        return rew / std if std > 0 else rew

    def _load_from_state_dict(self, *args, **kwargs):
        self.avg = None   # (the discounted sums are not in the state dict: they start again, as a fresh module's)
        return super()._load_from_state_dict(*args, **kwargs)


_RND_SCHEDULE_KEYS = {"constant": (), "step": ("final_step", "final_value"), "linear": ("initial_step", "final_step", "final_value")}


class RandomNetworkDistillation(torch.nn.Module):
    """rsl_rl's ``RandomNetworkDistillation``: a frozen random ``target`` MLP and a trained ``predictor`` MLP read the ``rnd_state``
    observation; ``‖target(x) − predictor(x)‖₂`` per env is the intrinsic reward (``get_intrinsic_reward``), scaled by ``weight``.

    ``predictor`` / ``target``: ``Linear`` + ``ELU``, nothing after the last layer (only ``activation="elu"``; a hidden width of ``-1``
    means ``num_states``); the target is in eval mode with ``requires_grad=False`` whatever ``train()`` is given.
    ``state_normalization``: an :class:`EmpiricalNormalization` ``(num_states, until=10**8)`` in front of both nets, updated by
    ``update_normalization(rnd_state)``; ``reward_normalization``: an :class:`EmpiricalDiscountedVariationNormalization`
    ``(eps=1e-2, gamma=0.99, until=10**8)`` behind the distance; ``nn.Identity`` otherwise, as rsl_rl.
    ``weight_schedule``: ``None`` / ``{"mode": "constant"}``; ``{"mode": "step", "final_step", "final_value"}`` — the initial weight
    while ``update_counter < final_step``, then ``final_value``; ``{"mode": "linear", "initial_step", "final_step", "final_value"}``.
    The weight is a Python float computed on the host from ``update_counter`` (one more per ``get_intrinsic_reward``).

    The methods here are the torch path (CPU tensors, the oracle backend, ``forward="torch"``); :class:`RndForward` is the HIP one."""

    def __init__(self, num_states: int, num_outputs: int, predictor_hidden_dims: Sequence[int], target_hidden_dims: Sequence[int],
                 activation: str = "elu", weight: float = 0.0, state_normalization: bool = False, reward_normalization: bool = False,
                 weight_schedule: Optional[dict] = None):
        super().__init__()
        if activation != "elu":
            raise ValueError(f"RandomNetworkDistillation: activation={activation!r} is not supported (only 'elu')")
        self.num_states, self.num_outputs = int(num_states), int(num_outputs)
        if self.num_states < 1 or self.num_outputs < 1:
            raise ValueError("RandomNetworkDistillation: num_states and num_outputs must be >= 1")
        dims = lambda hidden: [self.num_states if int(h) == -1 else int(h) for h in hidden]
        self.predictor = _mlp([self.num_states, *dims(predictor_hidden_dims), self.num_outputs])
        self.target = _mlp([self.num_states, *dims(target_hidden_dims), self.num_outputs])
        for p in self.target.parameters():
            p.requires_grad_(False)
        self.initial_weight = self.weight = float(weight)
        self.weight_schedule = self._check_schedule(weight_schedule)
        self.state_normalization, self.reward_normalization = bool(state_normalization), bool(reward_normalization)
        self.state_normalizer = EmpiricalNormalization(self.num_states, until=10 ** 8) if state_normalization else torch.nn.Identity()
        self.reward_normalizer = (EmpiricalDiscountedVariationNormalization((), until=10 ** 8) if reward_normalization
                                  else torch.nn.Identity())
        self.update_counter = 0
        self.target.eval()

    @staticmethod
    def _check_schedule(sched) -> Optional[dict]:
        if sched is None:
            return None
        if not isinstance(sched, dict) or sched.get("mode") not in _RND_SCHEDULE_KEYS:
            raise ValueError(f"RandomNetworkDistillation: weight_schedule={sched!r} needs a 'mode' of {sorted(_RND_SCHEDULE_KEYS)}")
        want = _RND_SCHEDULE_KEYS[sched["mode"]]
        missing = [k for k in want if k not in sched]
        bad = sorted(k for k in sched if k != "mode" and k not in want)
        if missing or bad:
            raise ValueError(f"RandomNetworkDistillation: weight_schedule mode {sched['mode']!r} takes {list(want)}"
                             f"{'; missing ' + str(missing) if missing else ''}{'; unknown ' + str(bad) if bad else ''}")
        if sched["mode"] == "linear" and not int(sched["final_step"]) > int(sched["initial_step"]):
            raise ValueError("RandomNetworkDistillation: weight_schedule 'linear' needs final_step > initial_step")
        return dict(sched)

    def _scheduled_weight(self) -> float:
        s, step, w0 = self.weight_schedule, self.update_counter, self.initial_weight
        if s is None or s["mode"] == "constant":
            return w0
        if s["mode"] == "step":
            return w0 if step < s["final_step"] else float(s["final_value"])
        if step < s["initial_step"]:
            return w0
        if step > s["final_step"]:
            return float(s["final_value"])
        return w0 + (float(s["final_value"]) - w0) * (step - s["initial_step"]) / (s["final_step"] - s["initial_step"])

    def _advance(self) -> float:
        """The host half of ``get_intrinsic_reward``: ``update_counter += 1`` and the schedule's weight for this call."""
        self.update_counter += 1
        self.weight = self._scheduled_weight()
        return self.weight

    def update_normalization(self, rnd_state) -> None:
        if isinstance(self.state_normalizer, EmpiricalNormalization):
            self.state_normalizer.update(rnd_state)

    def get_intrinsic_reward(self, rnd_state: torch.Tensor) -> torch.Tensor:
        weight = self._advance()
        with torch.no_grad():
            x = self.state_normalizer(rnd_state)
            r = torch.linalg.norm(self.target(x) - self.predictor(x), dim=1)
            r = self.reward_normalizer(r)
        return r * weight

    def train(self, mode: bool = True):
        super().train(mode)
        self.target.eval()
        return self


class _ActionStd:
    """The learnable action std of :class:`ActorCriticMLP` and :class:`StudentTeacherMLP`: a ``std`` parameter ``[A]``
    (``noise_std_type="scalar"``) or a ``log_std`` one in its place (``"log"``) — rsl_rl's names."""

    def _set_noise_std_type(self, who: str, noise_std_type: str) -> None:
        if noise_std_type not in ("scalar", "log"):
            raise ValueError(f"{who}: noise_std_type={noise_std_type!r} is not supported ('scalar' or 'log')")
        self.noise_std_type = noise_std_type

    def _make_std(self, init_noise_std: float, num_actions: int) -> None:
        if self.noise_std_type == "scalar":
            self.std = torch.nn.Parameter(init_noise_std * torch.ones(num_actions))
        else:
            self.log_std = torch.nn.Parameter(torch.log(init_noise_std * torch.ones(num_actions)))

    @property
    def action_std(self) -> torch.Tensor:
        """The current action std ``[A]`` (detached): ``std``, or ``exp(log_std)``."""
        return self.log_std.detach().exp() if self.noise_std_type == "log" else self.std.detach().clone()


def _policy_cfg(train_cfg: dict, who: str, keys: tuple, class_name: str) -> dict:
    """``train_cfg["policy"]`` for ``who.from_train_cfg``; ``ValueError`` naming the key for an unknown one, another activation than
    ``"elu"``, another ``noise_std_type`` than ``"scalar"`` / ``"log"`` or another ``class_name`` than the one given."""
    pol = dict(train_cfg.get("policy", {}))
    bad = sorted(k for k in pol if k not in keys)
    if bad:
        raise ValueError(f"{who}: unsupported policy keys {bad}")
    if pol.get("activation", "elu") != "elu":
        raise ValueError(f"{who}: policy.activation={pol['activation']!r} is not supported (only 'elu')")
    if pol.get("noise_std_type", "scalar") not in ("scalar", "log"):
        raise ValueError(f"{who}: policy.noise_std_type={pol['noise_std_type']!r} is not supported ('scalar' or 'log')")
    if pol.get("class_name", class_name) != class_name:
        raise ValueError(f"{who}: policy.class_name={pol['class_name']!r} is not supported (only '{class_name}')")
    return pol


_POLICY_KEYS = ("class_name", "activation", "actor_hidden_dims", "critic_hidden_dims", "init_noise_std", "noise_std_type",
                "actor_obs_normalization", "critic_obs_normalization")
_RNN_KEYS = ("rnn_type", "rnn_hidden_dim", "rnn_num_layers")


def _actor_critic_kwargs(train_cfg: dict, pol: dict) -> dict:
    """The constructor keywords ``ActorCriticMLP.from_train_cfg`` reads from a checked ``train_cfg["policy"]`` (``_POLICY_KEYS``)."""
    both = bool(train_cfg.get("empirical_normalization"))
    return dict(actor_hidden_dims=tuple(pol.get("actor_hidden_dims", (512, 256, 128))), critic_hidden_dims=tuple(pol.get("critic_hidden_dims", (512, 256, 128))),
                init_noise_std=float(pol.get("init_noise_std", 1.0)),
                actor_obs_normalization=both or bool(pol.get("actor_obs_normalization", False)),
                critic_obs_normalization=both or bool(pol.get("critic_obs_normalization", False)),
                noise_std_type=pol.get("noise_std_type", "scalar"))


def _rnn_kwargs(pol: dict) -> dict:
    """The three ``_RNN_KEYS`` of a recurrent policy's ``train_cfg["policy"]``, with rsl_rl's defaults."""
    return dict(rnn_type=pol.get("rnn_type", "lstm"), rnn_hidden_dim=pol.get("rnn_hidden_dim", 256), rnn_num_layers=pol.get("rnn_num_layers", 1))


def _check_rnn_args(who: str, rnn_type, rnn_hidden_dim, rnn_num_layers) -> None:
    """What a recurrent policy's constructor refuses: ``ValueError`` (``who: key=…``) naming the key."""
    if rnn_type not in ("lstm", "gru"):
        raise ValueError(f"{who}: rnn_type={rnn_type!r} is not supported ('lstm' or 'gru')")
    if int(rnn_num_layers) != 1:
        raise ValueError(f"{who}: rnn_num_layers={rnn_num_layers} is not supported (only 1)")
    if not 1 <= int(rnn_hidden_dim) <= nat.GF_MLP_MAX_HIDDEN:
        raise ValueError(f"{who}: rnn_hidden_dim={rnn_hidden_dim} is not supported (1 to {nat.GF_MLP_MAX_HIDDEN})")


class ActorCriticMLP(_ActionStd, torch.nn.Module):
    """rsl_rl's ``ActorCritic`` as configured by the reference's training scripts (examples/simple/train.py:56-62).
    ``actor_obs_normalization`` / ``critic_obs_normalization`` (rsl_rl 3.x): an :class:`EmpiricalNormalization` in front of the net
    (``actor_obs_normalizer`` / ``critic_obs_normalizer``; ``nn.Identity()`` when off, as rsl_rl) — buffers only, so ``parameters()``
    and their order are the same either way.  ``num_critic_obs``: the critic's input width where it differs from the actor's.
    ``noise_std_type``: ``"scalar"`` — a ``std`` parameter ``[A]`` starting at ``init_noise_std``; ``"log"`` — a ``log_std``
    parameter starting at ``log(init_noise_std)`` in its place (no ``std`` parameter; rsl_rl's names, so checkpoints interchange),
    which keeps the std positive whatever step Adam takes.  ``action_std`` is the current std of either."""

    is_recurrent = False

    def __init__(self, num_obs: int, num_actions: int, actor_hidden_dims: Sequence[int] = (512, 256, 128),
                 critic_hidden_dims: Sequence[int] = (512, 256, 128), init_noise_std: float = 1.0, num_critic_obs: Optional[int] = None,
                 actor_obs_normalization: bool = False, critic_obs_normalization: bool = False, noise_std_type: str = "scalar"):
        super().__init__()
        self._set_noise_std_type("ActorCriticMLP", noise_std_type)

        num_critic_obs = num_obs if num_critic_obs is None else int(num_critic_obs)
        self.actor = _mlp([num_obs, *actor_hidden_dims, num_actions])
        self.critic = _mlp([num_critic_obs, *critic_hidden_dims, 1])
        self._make_std(init_noise_std, num_actions)
        self.actor_obs_normalizer = EmpiricalNormalization(num_obs) if actor_obs_normalization else torch.nn.Identity()
        self.critic_obs_normalizer = EmpiricalNormalization(num_critic_obs) if critic_obs_normalization else torch.nn.Identity()
        self._scratch = _NormScratch()

    @classmethod
    def from_train_cfg(cls, train_cfg: dict, num_obs: int, num_actions: int, num_critic_obs: Optional[int] = None) -> "ActorCriticMLP":
        """The policy of a ``training_cfg()`` dict of ``examples/*/train.py``: ``policy.actor_hidden_dims`` / ``critic_hidden_dims`` /
        ``init_noise_std``, rsl_rl 3.x's ``policy.actor_obs_normalization`` / ``critic_obs_normalization``, and the top-level
        ``empirical_normalization`` the scripts carry (truthy: both normalisers; ``None`` / ``False``: the policy keys decide).
        ``policy.noise_std_type`` (``"scalar"`` or ``"log"``).
        Anything that cannot be honoured — another activation than ``"elu"``, another ``noise_std_type`` than those two, an
        unknown policy key — raises ``ValueError`` naming the key."""
        pol = _policy_cfg(train_cfg, "ActorCriticMLP", _POLICY_KEYS, "ActorCritic")
        return cls(num_obs, num_actions, num_critic_obs=num_critic_obs, **_actor_critic_kwargs(train_cfg, pol))

    def act_mean(self, obs: torch.Tensor) -> torch.Tensor:
        return self.actor(self.actor_obs_normalizer(obs))

    def evaluate(self, obs: torch.Tensor) -> torch.Tensor:
        return self.critic(self.critic_obs_normalizer(obs))

    def update_normalization(self, obs, critic_obs=None) -> None:
        """rsl_rl's ``ActorCritic.update_normalization``: both normalisers see this step's observations (``critic_obs=None``: the critic
        reads ``obs``) — ONE ``gf_obs_norm_update`` for the two.  ``obs`` / ``critic_obs``: a ``[N, W]`` tensor or up to four segments."""
        pairs = []
        for norm, x, name in ((self.actor_obs_normalizer, obs, "obs"), (self.critic_obs_normalizer, obs if critic_obs is None else critic_obs, "critic_obs")):
            if isinstance(norm, EmpiricalNormalization) and norm.training:
                pairs.append((norm, _segments(x, name, None, norm._mean.device, norm_width=norm.width)))
        _update_normalizers(pairs, self._scratch.args)


class _Memory(torch.nn.Module):
    """rsl_rl's ``Memory``: a one-layer, sequence-major ``nn.LSTM`` / ``nn.GRU`` (``rnn``) and its hidden state — ``h [1, N, H]``, for
    an LSTM ``(h, c)`` — which is not part of the state dict."""

    def __init__(self, input_size: int, rnn_type: str, hidden_size: int):
        super().__init__()
        cls = torch.nn.GRU if rnn_type == "gru" else torch.nn.LSTM
        self.rnn = cls(input_size=input_size, hidden_size=hidden_size, num_layers=1)
        self.hidden_states = None

    def forward(self, x: torch.Tensor, masks=None, hidden_states=None, unpad_index=None) -> torch.Tensor:
        if masks is not None:   # batch mode: a padded [T, ntraj, W] sequence from the given states; the stored state is untouched
            if hidden_states is None:
                raise ValueError("hidden states not passed to the memory module during a policy update")
            out, _ = self.rnn(x, hidden_states)
            return _unpad_trajectories(out, masks, unpad_index)
        out, self.hidden_states = self.rnn(x.unsqueeze(0), self.hidden_states)   # step mode: [N, W] -> [1, N, H]
        return out

    def reset(self, dones=None) -> None:
        if dones is None:
            self.hidden_states = None   # (zeros again at the next step)
        elif self.hidden_states is not None:
            for s in self.hidden_states if isinstance(self.hidden_states, tuple) else (self.hidden_states,):
                s[..., dones.to(torch.bool).reshape(-1), :] = 0.0


class _StateHolder:
    """A hidden state of its own over a memory's ``rnn`` (``RecurrentForward(own_state=True)``)."""

    def __init__(self, rnn):
        self.rnn, self.hidden_states = rnn, None

    reset = _Memory.reset


def _unpad_trajectories(out: torch.Tensor, masks: torch.Tensor, unpad_index=None) -> torch.Tensor:
    """rsl_rl's ``unpad_trajectories``: the real steps of a padded ``[T, ntraj, H]`` batch, trajectory-major, back as ``[T, envs, H]``.
    ``unpad_index`` (int64, the positions of the set mask elements in the flattened ``[ntraj, T]`` mask): the same rows through
    ``index_select`` — no boolean indexing, so no host synchronisation."""
    T, H = masks.shape[0], out.shape[-1]
    flat = out.transpose(1, 0)
    if unpad_index is None:
        rows = flat[masks.transpose(1, 0)]
    else:
        rows = flat.reshape(-1, H).index_select(0, unpad_index)
    return rows.view(-1, T, H).transpose(1, 0)


_RECURRENT_POLICY_KEYS = _POLICY_KEYS + _RNN_KEYS


class ActorCriticRecurrent(_ActionStd, torch.nn.Module):
    """rsl_rl's ``ActorCriticRecurrent``: a one-layer LSTM or GRU ``Memory`` in front of the actor MLP and another in front of the
    critic MLP — ``obs -> normaliser -> rnn -> MLP`` (rsl_rl 3.x).  Modules and state-dict keys are rsl_rl's (``memory_a.rnn.*``,
    ``memory_c.rnn.*``, ``actor.*``, ``critic.*``, ``std`` or ``log_std``), so checkpoints interchange; the hidden state is no part of it.

    Step mode — ``act_mean(obs)`` / ``evaluate(obs)`` without ``masks`` — advances that net's hidden state (zeros at the first step)
    by one step; ``reset(dones)`` zeroes the rows where ``dones`` is set (``None``: all), ``get_hidden_states()`` returns
    ``(actor_state, critic_state)``.  Batch mode — ``masks=`` and ``hidden_states=`` given — runs the rnn over a padded
    ``[T, ntraj, W]`` sequence from the given initial states and un-pads the outputs to ``[T, envs, H]`` in front of the MLP (with
    ``unpad_index=`` through ``index_select``); the stored state is untouched.

    ``rnn_num_layers`` other than 1, ``rnn_type`` other than ``"lstm"`` / ``"gru"`` and ``rnn_hidden_dim`` above 512 (the one-launch
    step's limit, ``GF_MLP_MAX_HIDDEN``) raise ``ValueError`` naming the key."""

    is_recurrent = True

    def __init__(self, num_obs: int, num_actions: int, actor_hidden_dims: Sequence[int] = (512, 256, 128),
                 critic_hidden_dims: Sequence[int] = (512, 256, 128), init_noise_std: float = 1.0, num_critic_obs: Optional[int] = None,
                 actor_obs_normalization: bool = False, critic_obs_normalization: bool = False, noise_std_type: str = "scalar",
                 rnn_type: str = "lstm", rnn_hidden_dim: int = 256, rnn_num_layers: int = 1):
        super().__init__()
        self._set_noise_std_type("ActorCriticRecurrent", noise_std_type)
        _check_rnn_args("ActorCriticRecurrent", rnn_type, rnn_hidden_dim, rnn_num_layers)
        self.rnn_type, self.rnn_hidden_dim = rnn_type, int(rnn_hidden_dim)

        num_critic_obs = num_obs if num_critic_obs is None else int(num_critic_obs)
        self.memory_a = _Memory(num_obs, rnn_type, self.rnn_hidden_dim)
        self.memory_c = _Memory(num_critic_obs, rnn_type, self.rnn_hidden_dim)
        self.actor = _mlp([self.rnn_hidden_dim, *actor_hidden_dims, num_actions])
        self.critic = _mlp([self.rnn_hidden_dim, *critic_hidden_dims, 1])
        self._make_std(init_noise_std, num_actions)
        self.actor_obs_normalizer = EmpiricalNormalization(num_obs) if actor_obs_normalization else torch.nn.Identity()
        self.critic_obs_normalizer = EmpiricalNormalization(num_critic_obs) if critic_obs_normalization else torch.nn.Identity()
        self._scratch = _NormScratch()

    @classmethod
    def from_train_cfg(cls, train_cfg: dict, num_obs: int, num_actions: int, num_critic_obs: Optional[int] = None) -> "ActorCriticRecurrent":
        """As :meth:`ActorCriticMLP.from_train_cfg`, for ``policy.class_name = "ActorCriticRecurrent"`` with ``policy.rnn_type``,
        ``rnn_hidden_dim`` and ``rnn_num_layers``."""
        pol = _policy_cfg(train_cfg, "ActorCriticRecurrent", _RECURRENT_POLICY_KEYS, "ActorCriticRecurrent")
        return cls(num_obs, num_actions, num_critic_obs=num_critic_obs, **_actor_critic_kwargs(train_cfg, pol), **_rnn_kwargs(pol))

    def act_mean(self, obs: torch.Tensor, masks=None, hidden_states=None, unpad_index=None) -> torch.Tensor:
        return self.actor(self.memory_a(self.actor_obs_normalizer(obs), masks, hidden_states, unpad_index).squeeze(0))

    def evaluate(self, obs: torch.Tensor, masks=None, hidden_states=None, unpad_index=None) -> torch.Tensor:
        return self.critic(self.memory_c(self.critic_obs_normalizer(obs), masks, hidden_states, unpad_index).squeeze(0))

    def get_hidden_states(self) -> tuple:
        return self.memory_a.hidden_states, self.memory_c.hidden_states

    def reset(self, dones=None) -> None:
        self.memory_a.reset(dones)
        self.memory_c.reset(dones)

    update_normalization = ActorCriticMLP.update_normalization


_STUDENT_TEACHER_KEYS = ("class_name", "activation", "student_hidden_dims", "teacher_hidden_dims", "init_noise_std", "noise_std_type",
                         "student_obs_normalization", "teacher_obs_normalization")


def _student_teacher_kwargs(pol: dict) -> dict:
    """The constructor keywords ``StudentTeacherMLP.from_train_cfg`` reads from a checked ``train_cfg["policy"]`` (``_STUDENT_TEACHER_KEYS``)."""
    return dict(student_hidden_dims=tuple(pol.get("student_hidden_dims", (256, 256, 256))),
                teacher_hidden_dims=tuple(pol.get("teacher_hidden_dims", (256, 256, 256))), init_noise_std=float(pol.get("init_noise_std", 0.1)),
                student_obs_normalization=bool(pol.get("student_obs_normalization", False)),
                teacher_obs_normalization=bool(pol.get("teacher_obs_normalization", False)),
                noise_std_type=pol.get("noise_std_type", "scalar"))


class _StudentTeacher(_ActionStd, torch.nn.Module):
    """What :class:`StudentTeacherMLP` and :class:`StudentTeacherRecurrent` share: the frozen teacher side — ``teacher``, ``memory_t``
    where ``teacher_recurrent``, ``teacher_obs_normalizer`` — which stays in eval mode whatever ``train()`` is given, the student's
    normaliser update and rsl_rl's ``load_state_dict`` rule.  The feed-forward class is the case without memories."""

    is_recurrent = False
    teacher_recurrent = False

    def _finish(self, num_student_obs, num_teacher_obs, num_actions, init_noise_std, student_obs_normalization, teacher_obs_normalization) -> None:
        """What a constructor does once its nets (and memories) exist, in this order: the teacher side's parameters frozen, the std,
        the two normalisers, the teacher side in eval mode."""
        for m in self._frozen():
            for p in m.parameters():
                p.requires_grad_(False)
        self._make_std(init_noise_std, num_actions)
        self.student_obs_normalizer = EmpiricalNormalization(int(num_student_obs)) if student_obs_normalization else torch.nn.Identity()
        self.teacher_obs_normalizer = EmpiricalNormalization(int(num_teacher_obs)) if teacher_obs_normalization else torch.nn.Identity()
        self._scratch = _NormScratch()
        self._freeze()

    def _frozen(self) -> tuple:
        """The teacher's modules, the normaliser (created last) included once it exists."""
        mods = (self.teacher, self.memory_t) if self.teacher_recurrent else (self.teacher,)
        norm = getattr(self, "teacher_obs_normalizer", None)
        return mods if norm is None else mods + (norm,)

    def _freeze(self) -> None:
        for m in self._frozen():
            m.eval()

    def update_normalization(self, obs) -> None:
        """The student's normaliser sees this step's observations (a ``[N, W]`` tensor or up to four segments); the teacher's is
        frozen with the teacher."""
        norm = self.student_obs_normalizer
        if isinstance(norm, EmpiricalNormalization) and norm.training:
            _update_normalizers([(norm, _segments(obs, "obs", None, norm._mean.device, norm_width=norm.width))], self._scratch.args)

    def train(self, mode: bool = True):
        super().train(mode)
        self._freeze()
        return self

    def load_state_dict(self, state_dict, strict: bool = True) -> bool:
        who = f"{type(self).__name__}.load_state_dict"
        if any(k.startswith("actor.") for k in state_dict):   # a PPO checkpoint: its actor (and memory_a) becomes the teacher
            recurrent = any(k.startswith("memory_a.") for k in state_dict)
            if self.is_recurrent and recurrent != self.teacher_recurrent:   # (the feed-forward class reads only the keys it knows)
                raise ValueError(f"{who}: the PPO checkpoint is {'recurrent' if recurrent else 'feed-forward'} (it has "
                                 f"{'' if recurrent else 'no '}'memory_a.*' keys); this policy was built with teacher_recurrent={self.teacher_recurrent}")
            sub = lambda prefix: {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
            self.teacher.load_state_dict(sub("actor."), strict=strict)
            if self.teacher_recurrent:
                self.memory_t.load_state_dict(sub("memory_a."), strict=strict)
            norm = sub("actor_obs_normalizer.")
            if norm and isinstance(self.teacher_obs_normalizer, EmpiricalNormalization):
                self.teacher_obs_normalizer.load_state_dict(norm, strict=strict)
            resumed = False
        elif any(k.startswith("student.") for k in state_dict):
            super().load_state_dict(state_dict, strict=strict)
            resumed = True
        else:
            raise ValueError(f"{who}: the state dict has neither 'actor.*' keys (a PPO checkpoint) nor 'student.*' keys (a distillation checkpoint)")
        self.loaded_teacher = True
        self._freeze()
        return resumed


class StudentTeacherMLP(_StudentTeacher):
    """rsl_rl's ``StudentTeacher`` (feed-forward): a ``student`` that reads the deployable observations and is trained, and a frozen
    ``teacher`` that reads the privileged ones and labels every step.  Both are ``nn.Sequential`` of ``Linear`` with ``ELU`` between;
    ``std`` (or ``log_std`` with ``noise_std_type="log"``) is the exploration noise of the student's actions during collection;
    ``student_obs_normalizer`` / ``teacher_obs_normalizer`` are an :class:`EmpiricalNormalization` or ``nn.Identity`` — rsl_rl's
    names throughout, so model state dicts interchange.  The teacher's parameters have ``requires_grad=False`` and the teacher and its
    normaliser stay in eval mode whatever ``train()`` is given.

    ``load_state_dict`` follows rsl_rl's rule: a PPO checkpoint (``actor.*`` keys) fills the teacher — and the teacher's normaliser
    from ``actor_obs_normalizer.*`` when both exist — leaves the student alone and returns ``False`` ("not a resume"); a distillation
    checkpoint (``student.*`` keys) is loaded whole and returns ``True``; both set ``loaded_teacher``; anything else raises
    ``ValueError``."""

    def __init__(self, num_student_obs: int, num_teacher_obs: int, num_actions: int, student_hidden_dims: Sequence[int] = (256, 256, 256),
                 teacher_hidden_dims: Sequence[int] = (256, 256, 256), init_noise_std: float = 0.1, student_obs_normalization: bool = False,
                 teacher_obs_normalization: bool = False, noise_std_type: str = "scalar"):
        super().__init__()
        self._set_noise_std_type("StudentTeacherMLP", noise_std_type)
        self.loaded_teacher = False

        self.student = _mlp([int(num_student_obs), *student_hidden_dims, int(num_actions)])
        self.teacher = _mlp([int(num_teacher_obs), *teacher_hidden_dims, int(num_actions)])
        self._finish(num_student_obs, num_teacher_obs, num_actions, init_noise_std, student_obs_normalization, teacher_obs_normalization)

    @classmethod
    def from_train_cfg(cls, train_cfg: dict, num_student_obs: int, num_teacher_obs: int, num_actions: int) -> "StudentTeacherMLP":
        """The policy of a distillation ``train_cfg``: ``policy.student_hidden_dims`` / ``teacher_hidden_dims`` / ``init_noise_std`` /
        ``noise_std_type`` / ``student_obs_normalization`` / ``teacher_obs_normalization``.  Anything that cannot be honoured — an
        unknown policy key, another activation than ``"elu"``, another class name than ``"StudentTeacher"`` — raises ``ValueError``
        naming the key."""
        pol = _policy_cfg(train_cfg, "StudentTeacherMLP", _STUDENT_TEACHER_KEYS, "StudentTeacher")
        return cls(num_student_obs, num_teacher_obs, num_actions, **_student_teacher_kwargs(pol))

    def act_mean(self, obs: torch.Tensor) -> torch.Tensor:
        """The student on its normalised input (rsl_rl's ``act_inference``)."""
        return self.student(self.student_obs_normalizer(obs))

    def evaluate(self, teacher_obs: torch.Tensor) -> torch.Tensor:
        """The teacher's actions, under ``no_grad``."""
        with torch.no_grad():
            return self.teacher(self.teacher_obs_normalizer(teacher_obs))


_STUDENT_TEACHER_RECURRENT_KEYS = _STUDENT_TEACHER_KEYS + _RNN_KEYS + ("teacher_recurrent",)


class StudentTeacherRecurrent(_StudentTeacher):
    """rsl_rl's ``StudentTeacherRecurrent``: a one-layer LSTM or GRU ``Memory`` (``memory_s``) in front of the trained ``student`` MLP
    and, with ``teacher_recurrent=True``, another (``memory_t``) in front of the frozen ``teacher`` MLP — ``obs -> normaliser -> rnn ->
    MLP``; without it the teacher is :class:`StudentTeacherMLP`'s.  Modules and state-dict keys are rsl_rl's (``memory_s.rnn.*``,
    ``memory_t.rnn.*`` only with ``teacher_recurrent``, ``student.*``, ``teacher.*``, ``std`` or ``log_std``,
    ``student_obs_normalizer.*`` / ``teacher_obs_normalizer.*``); the hidden states are no part of the state dict.  ``student`` reads
    ``rnn_hidden_dim`` columns, and so does ``teacher`` when it is recurrent.  The teacher, ``memory_t`` and the teacher's normaliser
    are frozen and stay in eval mode whatever ``train()`` is given.

    ``act_mean(obs)`` advances ``memory_s`` by one step (zeros at the first) — with a graph when grad is enabled, which is what
    :class:`Distillation` back-propagates through; ``evaluate(teacher_obs)`` runs under ``no_grad`` and advances ``memory_t`` if
    there is one.  ``reset(dones)`` zeroes the rows of both states where ``dones`` is set, ``reset()`` forgets them,
    ``reset(hidden_states=(student_state, teacher_state))`` installs the given ones; ``get_hidden_states()`` returns that pair (the
    teacher's ``None`` without ``memory_t``); ``detach_hidden_states()`` cuts both from their graphs.

    ``load_state_dict`` is rsl_rl's rule: a PPO checkpoint (``actor.*`` keys) fills the teacher, the teacher's normaliser and — with
    ``teacher_recurrent`` — ``memory_t`` from ``memory_a.*``, and returns ``False``; a distillation checkpoint (``student.*`` keys)
    loads whole and returns ``True``.  A recurrent PPO checkpoint into ``teacher_recurrent=False``, or a feed-forward one into
    ``teacher_recurrent=True``, raises ``ValueError`` naming ``teacher_recurrent``.

    ``rnn_num_layers`` other than 1, ``rnn_type`` other than ``"lstm"`` / ``"gru"`` and ``rnn_hidden_dim`` outside 1 … 512 raise
    ``ValueError`` naming the key, as :class:`ActorCriticRecurrent`."""

    is_recurrent = True

    def __init__(self, num_student_obs: int, num_teacher_obs: int, num_actions: int, student_hidden_dims: Sequence[int] = (256, 256, 256),
                 teacher_hidden_dims: Sequence[int] = (256, 256, 256), init_noise_std: float = 0.1, student_obs_normalization: bool = False,
                 teacher_obs_normalization: bool = False, noise_std_type: str = "scalar", rnn_type: str = "lstm", rnn_hidden_dim: int = 256,
                 rnn_num_layers: int = 1, teacher_recurrent: bool = False):
        super().__init__()
        who = "StudentTeacherRecurrent"
        self._set_noise_std_type(who, noise_std_type)
        _check_rnn_args(who, rnn_type, rnn_hidden_dim, rnn_num_layers)
        self.rnn_type, self.rnn_hidden_dim, self.teacher_recurrent = rnn_type, int(rnn_hidden_dim), bool(teacher_recurrent)
        self.loaded_teacher = False

        H = self.rnn_hidden_dim
        self.memory_s = _Memory(int(num_student_obs), rnn_type, H)
        self.student = _mlp([H, *student_hidden_dims, int(num_actions)])
        if self.teacher_recurrent:
            self.memory_t = _Memory(int(num_teacher_obs), rnn_type, H)
        self.teacher = _mlp([H if self.teacher_recurrent else int(num_teacher_obs), *teacher_hidden_dims, int(num_actions)])
        self._finish(num_student_obs, num_teacher_obs, num_actions, init_noise_std, student_obs_normalization, teacher_obs_normalization)

    @classmethod
    def from_train_cfg(cls, train_cfg: dict, num_student_obs: int, num_teacher_obs: int, num_actions: int) -> "StudentTeacherRecurrent":
        """As :meth:`StudentTeacherMLP.from_train_cfg`, for ``policy.class_name = "StudentTeacherRecurrent"`` with ``policy.rnn_type``,
        ``rnn_hidden_dim``, ``rnn_num_layers`` and ``teacher_recurrent``."""
        pol = _policy_cfg(train_cfg, "StudentTeacherRecurrent", _STUDENT_TEACHER_RECURRENT_KEYS, "StudentTeacherRecurrent")
        return cls(num_student_obs, num_teacher_obs, num_actions, **_student_teacher_kwargs(pol), **_rnn_kwargs(pol),
                   teacher_recurrent=bool(pol.get("teacher_recurrent", False)))

    def act_mean(self, obs: torch.Tensor) -> torch.Tensor:
        """The student on one more step of ``memory_s`` (rsl_rl's ``act_inference``)."""
        return self.student(self.memory_s(self.student_obs_normalizer(obs)).squeeze(0))

    def evaluate(self, teacher_obs: torch.Tensor) -> torch.Tensor:
        """The teacher's actions, under ``no_grad``; a recurrent teacher's ``memory_t`` advances by one step."""
        with torch.no_grad():
            x = self.teacher_obs_normalizer(teacher_obs)
            return self.teacher(self.memory_t(x).squeeze(0) if self.teacher_recurrent else x)

    def get_hidden_states(self) -> tuple:
        return self.memory_s.hidden_states, self.memory_t.hidden_states if self.teacher_recurrent else None

    def reset(self, dones=None, hidden_states=None) -> None:
        memories = (self.memory_s, self.memory_t) if self.teacher_recurrent else (self.memory_s,)
        if hidden_states is not None:
            if dones is not None:
                raise ValueError("StudentTeacherRecurrent.reset: dones and hidden_states cannot both be given")
            for m, hs in zip(memories, hidden_states):
                m.hidden_states = hs
            return
        for m in memories:
            m.reset(dones)

    def detach_hidden_states(self) -> None:
        for m in (self.memory_s, self.memory_t) if self.teacher_recurrent else (self.memory_s,):
            hs = m.hidden_states
            if hs is not None:
                m.hidden_states = tuple(x.detach() for x in hs) if isinstance(hs, tuple) else hs.detach()


def _policy_std(policy):
    """``(parameter, is_log)``: ``policy.log_std`` where ``policy.noise_std_type == "log"`` (rsl_rl's attribute names: a foreign policy
    works too), ``policy.std`` otherwise; the parameter is None where the policy has none."""
    is_log = getattr(policy, "noise_std_type", "scalar") == "log"
    p = getattr(policy, "log_std" if is_log else "std", None)
    return (p if isinstance(p, torch.Tensor) else None), is_log


def _walk_mlp(net, name: str, max_out: int, who: str = "PolicyForward"):
    """[(weight, bias)] of the Linear layers of ``policy.<name>`` as ``gf_mlp_act`` / ``gf_mlp_distill_act`` read them (the Parameter
    objects: their storage may be re-seated later), or None for a missing net; ``ValueError`` (``who: policy.<name> …``) for anything
    the kernel cannot run."""
    if net is None:
        return None
    if not isinstance(net, torch.nn.Sequential) or len(net) == 0:
        raise ValueError(f"{who}: policy.{name} must be a non-empty nn.Sequential of Linear and ELU")
    layers = []
    for i, m in enumerate(net):
        if i % 2 == 0:
            if not isinstance(m, torch.nn.Linear):
                raise ValueError(f"{who}: policy.{name}[{i}] is {type(m).__name__}; expected Linear")
            if m.bias is None:
                raise ValueError(f"{who}: policy.{name}[{i}] has no bias")
            for p, what in ((m.weight, "weight"), (m.bias, "bias")):
                if p.dtype != torch.float32:
                    raise ValueError(f"{who}: policy.{name}[{i}].{what} is {p.dtype}; the kernel reads float32")
                if not p.is_contiguous():
                    raise ValueError(f"{who}: policy.{name}[{i}].{what} is not contiguous")
            layers.append((m.weight, m.bias))
        elif not isinstance(m, torch.nn.ELU) or float(m.alpha) != 1.0:
            what = f"ELU(alpha={m.alpha})" if isinstance(m, torch.nn.ELU) else type(m).__name__
            raise ValueError(f"{who}: policy.{name}[{i}] is {what}; only ELU(alpha=1) between Linear layers is supported")
    if len(net) % 2 == 0:
        raise ValueError(f"{who}: policy.{name} ends in an activation; the last module must be a Linear")
    if len(layers) > nat.GF_MLP_MAX_LAYERS:
        raise ValueError(f"{who}: policy.{name} has {len(layers)} Linear layers; at most {nat.GF_MLP_MAX_LAYERS}")
    if layers[0][0].shape[1] > nat.GF_MLP_MAX_INPUT_WIDTH:
        raise ValueError(f"{who}: policy.{name} reads {layers[0][0].shape[1]} inputs; at most {nat.GF_MLP_MAX_INPUT_WIDTH}")
    for i, (w, _b) in enumerate(layers[:-1]):
        if w.shape[0] > nat.GF_MLP_MAX_HIDDEN:
            raise ValueError(f"{who}: policy.{name} has a hidden layer of width {w.shape[0]}; at most {nat.GF_MLP_MAX_HIDDEN}")
    out = layers[-1][0].shape[0]
    if name == "critic" and out != 1:
        raise ValueError(f"{who}: policy.critic has {out} outputs; the value is one")
    if out > max_out:
        raise ValueError(f"{who}: policy.{name} has {out} outputs; at most {max_out}")
    return layers


def _fill_net(net, layers, parts, norm=None) -> None:
    """Point a GfMlpNet at the current weights of ``layers``, the input segments ``parts`` and the normaliser in front (``layers`` or
    ``parts`` None: the net is left out of the launch)."""
    if layers is None or parts is None:
        net.num_layers = 0
        return
    if norm is None:
        if net.in_mean is not None:
            net.in_mean = net.in_std = None
    else:
        if norm._mean.device != parts[0].device:
            raise ValueError(f"the observation lives on {parts[0].device}, the normaliser on {norm._mean.device}")
        net.in_mean, net.in_std, net.in_eps = norm._mean.data_ptr(), norm._std.data_ptr(), norm.eps
    net.num_layers, net.num_inputs = len(layers), len(parts)
    for seg, x in zip(net.inputs, parts):
        seg.rows, seg.width, seg.row_stride = x.data_ptr(), x.shape[1], 0 if x.is_contiguous() else x.stride(0)
    for lay, (w, b) in zip(net.layers, layers):
        lay.weight, lay.bias, lay.out_width = w.data_ptr(), b.data_ptr(), w.shape[0]


def _fill_sampling(a, std, std_is_log: bool, noise, seed: int, stream: int, env_offset: int, actions) -> None:
    """The sampling fields a GfMlpActArgs and a GfMlpDistillArgs share by name: the ``[A]`` std (or log_std), the given draws or the
    Philox key of the kernel's own, and the fresh ``[N, A]`` tensor the sample goes to.  ``mean`` is not kept."""
    a.std, a.std_is_log = std.data_ptr(), 1 if std_is_log else 0
    a.noise = None if noise is None else noise.data_ptr()
    a.seed, a.stream, a.env_offset = seed, stream, env_offset
    a.mean = None
    a.actions = actions.data_ptr()


def _walk_rnn(memory, name: str, layers) -> int:
    """The cell type of ``policy.<name>.rnn``; ``ValueError`` naming what the kernel cannot run."""
    who = f"RecurrentForward: policy.{name}.rnn"
    rnn = getattr(memory, "rnn", None)
    if not isinstance(rnn, (torch.nn.LSTM, torch.nn.GRU)):
        raise ValueError(f"{who} must be an nn.LSTM or nn.GRU, not {type(rnn).__name__}")
    if rnn.num_layers != 1 or rnn.bidirectional or not rnn.bias or rnn.batch_first or getattr(rnn, "proj_size", 0):
        raise ValueError(f"{who} must have num_layers=1, bias=True, batch_first=False, no projection and one direction")
    if not 1 <= rnn.hidden_size <= nat.GF_MLP_MAX_HIDDEN:
        raise ValueError(f"{who} has hidden_size {rnn.hidden_size}; 1 to {nat.GF_MLP_MAX_HIDDEN}")
    if rnn.input_size > nat.GF_MLP_MAX_INPUT_WIDTH:
        raise ValueError(f"{who} reads {rnn.input_size} inputs; at most {nat.GF_MLP_MAX_INPUT_WIDTH}")
    if int(layers[0][0].shape[1]) != rnn.hidden_size:
        raise ValueError(f"{who} has hidden_size {rnn.hidden_size}; the MLP behind it reads {int(layers[0][0].shape[1])}")
    for pn in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
        p = getattr(rnn, pn)
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise ValueError(f"{who}.{pn} must be contiguous float32")
    return nat.GF_RNN_LSTM if isinstance(rnn, torch.nn.LSTM) else nat.GF_RNN_GRU


class _MlpForward:
    """What the four forwards share.  A forward keeps ``policy``, per net name the ``[(weight, bias)]`` list ``_walk_mlp`` returned
    (or None) as the attribute of that name, and ``_memory``: ``{net name: memory}`` for the nets with an rnn in front (a
    :class:`RecurrentForward`; empty otherwise).  The descriptors come in two families — actor–critic (GfMlpActArgs) and
    student–teacher (GfMlpDistillArgs) — each bare, or, for a forward with memories, nested as ``.act`` beside one GfRnnCell per net."""

    _memory: dict = {}

    def _setup(self, policy, who: str, nets, missing: str, both: bool = True, memories=(), own_state: bool = False, same_width: bool = False) -> None:
        """A constructor's checks, under the class name ``who``: walk the two ``nets`` (``(name, most outputs)`` each) — ``both``
        required, or at least one, ``missing`` says which — ``same_width`` outputs, the ``memories`` (``(net name, attribute of the
        policy)`` each; ``own_state``: a state of this forward's own over their rnn), the normalisers, the ``[A]`` std (required with
        ``both``).  Sets ``num_actions`` (None without an actor or a std)."""
        self.policy, self._who = policy, who
        for name, max_out in nets:
            setattr(self, name, _walk_mlp(getattr(policy, name, None), name, max_out, who))
        (a, _), (b, _) = nets
        first, second = getattr(self, a), getattr(self, b)
        if (first is None or second is None) if both else (first is None and second is None):
            raise ValueError(f"{who}: {missing}")
        if same_width and int(second[-1][0].shape[0]) != int(first[-1][0].shape[0]):
            raise ValueError(f"{who}: policy.{a} has {int(first[-1][0].shape[0])} outputs, policy.{b} {int(second[-1][0].shape[0])}")
        if memories:
            self._memory = {name: getattr(policy, attr, None) for name, attr in memories}
            if own_state:
                self._memory = {name: _StateHolder(getattr(m, "rnn", None)) for name, m in self._memory.items()}
            self._cell_type = {name: _walk_rnn(self._memory[name], attr, getattr(self, name)) for name, attr in memories}
        self._pending = dict.fromkeys(self._memory)
        self._keep = None
        # what reads a net's observation: its cell's input weights, or its first layer (the Parameter objects, as the layers' are)
        self._readers = {name: [(self._memory[name].rnn.weight_ih_l0, None)] if name in self._memory else getattr(self, name) for name, _ in nets}
        self._in_width = {name: int(r[0][0].shape[1]) for name, r in self._readers.items() if r is not None}
        for name, _ in nets:
            self._normalizer(name)   # (refuses what the kernel cannot fold in)
        std, is_log = _policy_std(policy)   # the type is fixed here; the parameter itself is looked up per call
        self.std_is_log, self._std_name = is_log, "log_std" if is_log else "std"
        self.num_actions = None
        if first is not None and (both or std is not None):
            A = int(first[-1][0].shape[0])
            if std is None or std.dtype != torch.float32 or tuple(std.shape) != (A,):
                raise ValueError(f"{who}: policy.{self._std_name} must be a float32 [{A}] tensor" + ("" if both else f", not {std.dtype} {tuple(std.shape)}"))
            self.num_actions = A

    def _normalizer(self, name: str) -> Optional["EmpiricalNormalization"]:
        """The policy's current normaliser in front of net ``name`` — of its memory, where it has one (None: the input is read as it is)."""
        width = self._in_width.get(name)   # the cell's input_size, or the first layer's (None: the policy has no such net)
        if width is None:
            return None
        return _as_normalizer(getattr(self.policy, name + "_obs_normalizer", None), width, f"{self._who}: policy.{name}_obs_normalizer")

    def _reader(self, name: str):
        """What ``_segments`` checks an observation of net ``name`` against: its cell's input weights, or its first layer."""
        return self._readers[name]

    def _descriptors(self, cls, one_cls=None) -> None:
        """``_args``: the collection step's descriptor; ``_one_args``: the actor–critic one of ``_one`` (``one_cls`` None: the same).
        Beside each, its parts looked up once (ctypes builds a new view at every attribute read): ``(the act part, {field: (its
        GfMlpNet, its GfRnnCell or None)})``."""
        def parts(d):
            a = d.act if self._memory else d
            return a, {f: (getattr(a, f), getattr(d, f + "_cell") if self._memory else None) for f, t in a._fields_ if t is nat.GfMlpNet}

        self._args = cls()
        self._args_parts = parts(self._args)
        self._one_args = self._args if one_cls is None else one_cls()
        self._one_parts = self._args_parts if one_cls is None else parts(self._one_args)

    def _fill_desc(self, d_parts, n: int, slots, save=None):
        """A descriptor of either family (its ``_descriptors`` parts) for ``n`` rows; ``slots``: ``(field of the descriptor, net name,
        segments)`` twice — the net pointed at the current weights, normaliser and segments and, in a nested descriptor, its cell at
        the memory (``_fill_cell``; GF_RNN_NONE without one); segments None: that net is left out of the launch.  Returns the ``act``
        part."""
        a, nets = d_parts
        a.num_envs = n
        keep = []
        for slot, name, parts in slots:
            net, cell = nets[slot]
            if parts is None:
                net.num_layers = 0
            else:
                _fill_net(net, getattr(self, name), parts, self._normalizer(name))
            if cell is not None:
                if parts is not None and name in self._memory:
                    keep.append(self._fill_cell(name, cell, parts, n, save))
                    continue
                cell.type = nat.GF_RNN_NONE
                cell.h_save = cell.c_save = cell.reset = None
            keep.append(parts)
        self._keep = keep
        return a

    def _torch_step(self, name: str, x: torch.Tensor) -> torch.Tensor:
        """Net ``name`` of the module in torch on this forward's state (the policy's own unless ``own_state``), under ``no_grad``: the
        test-only oracle backend's path."""
        norm = self._normalizer(name)
        x = x if norm is None else norm(x)
        m = self._memory.get(name)
        if m is not None:
            x, m.hidden_states = m.rnn(x.unsqueeze(0), m.hidden_states)
            x = x.squeeze(0)
        return getattr(self.policy, name)(x)

    def _one(self, obs, name: str) -> torch.Tensor:
        """The output of net ``name`` alone for ``obs`` (one more step of its memory, where it has one), a fresh tensor: one
        ``gf_mlp_act`` / ``gf_mlp_recurrent_act`` launch on the actor–critic descriptor ``_one_args``, with the net in the critic's
        slot if it is the critic and in the actor's otherwise, the other slot left out and nothing sampled."""
        layers = getattr(self, name)
        if layers is None:
            raise ValueError(f"{self._who}: the policy has no {name}")
        parts = _segments(obs, "obs", None, None, self._reader(name))
        fn = getattr(nat.get_backend(), "mlp_recurrent_act" if self._memory else "mlp_act", None)
        if fn is None:   # (the test-only oracle backend)
            with torch.no_grad():
                return self._torch_step(name, _cat(parts))
        n = int(parts[0].shape[0])
        out = torch.empty((n, int(layers[-1][0].shape[0])), device=parts[0].device, dtype=torch.float32)
        slot, other = ("critic", "actor") if name == "critic" else ("actor", "critic")
        a = self._fill_desc(self._one_parts, n, ((slot, name, parts), (other, None, None)))
        a.std_is_log = a.std_per_env = 0
        a.std = a.noise = a.actions = a.actions_out = a.mu_out = a.sigma_out = a.values_out = a.log_prob_out = None
        a.mean, a.values = (None, out.data_ptr()) if name == "critic" else (out.data_ptr(), None)
        self._keep_one = out
        fn(self._one_args)
        return out


class _ActorCriticForward(_MlpForward):
    """What :class:`PolicyForward` and :class:`RecurrentForward` share: ``_args`` is the actor–critic descriptor of the collection step,
    and of ``mean`` / ``value``."""

    def _fill(self, n: int, actor_parts, critic_parts, save=None):
        """The descriptor with the given nets (None: left out) pointed at the current weights and inputs — and, where they have a
        memory, at its state and pending reset, which is consumed; ``save``: ``{name: (h_save, c_save)}``."""
        self._fill_desc(self._args_parts, n, (("actor", "actor", actor_parts), ("critic", "critic", critic_parts)), save)
        return self._args

    def mean(self, obs) -> torch.Tensor:
        """The actor's output ``[N, A]`` (``policy.act_mean(obs)``, one more step of its memory where it has one): one launch, a fresh
        tensor."""
        return self._one(obs, "actor")

    def value(self, critic_obs) -> torch.Tensor:
        """The critic's output ``[N, 1]`` (``policy.evaluate(critic_obs)``, one more step of its memory where it has one): one launch,
        a fresh tensor."""
        return self._one(critic_obs, "critic")


class PolicyForward(_ActorCriticForward):
    """The actor and critic of a policy as ``gf_mlp_act`` reads them: one launch per forward pass, weights read in place.

    ``policy.actor`` / ``policy.critic`` (either may be missing or ``None``) must be ``nn.Sequential`` of ``Linear`` layers with
    ``ELU(alpha=1)`` between them and nothing after the last, float32, contiguous, within the kernel's limits (hidden widths <= 512,
    input <= 1 024, actor output <= 64, critic output 1, at most 6 ``Linear``): anything else raises ``ValueError`` naming it.  Only the
    structure is kept: the weight addresses are read from the parameters at every call, so a ``PolicyForward`` made before a
    :class:`PPO` (which re-seats every ``p.data`` into its flat buffer and updates it in place) sees the current weights.

    ``policy.actor_obs_normalizer`` / ``policy.critic_obs_normalizer`` (missing, ``None``, ``nn.Identity`` or an
    :class:`EmpiricalNormalization` of the first layer's width — anything else raises ``ValueError``) are looked up at every call like
    the weights; the kernel normalises the input as it stages it, so a normalising policy's forward stays one launch.

    ``mean(obs)`` / ``value(critic_obs)``: play-time inference and the bootstrap value, one launch each, fresh tensors;
    ``RolloutStorage.act_policy(forward, obs)``: the collection step.  An observation is a ``[N, W]`` tensor or a sequence of up to
    four whose widths add up to the first layer's input (an observation group's members, no ``torch.cat``)."""

    _ENTRY = "mlp_act"   # the backend's one-launch step

    def __init__(self, policy):
        self._setup(policy, "PolicyForward", (("actor", nat.GF_MLP_MAX_ACTIONS), ("critic", 1)), "the policy has neither an actor nor a critic", both=False)
        self._descriptors(nat.GfMlpActArgs)

    def std_param(self):
        """``(policy.std, False)`` or, for a ``noise_std_type="log"`` policy, ``(policy.log_std, True)`` — the parameter is looked up at
        every call, the type was read at construction."""
        return getattr(self.policy, self._std_name, None), self.std_is_log



class RecurrentForward(_ActorCriticForward):
    """A recurrent policy (:class:`ActorCriticRecurrent`, or rsl_rl's: ``memory_a.rnn`` / ``memory_c.rnn`` one-layer ``nn.LSTM`` or
    ``nn.GRU``, ``actor`` / ``critic`` MLPs) as ``gf_mlp_recurrent_act`` reads it: normaliser, cell, MLP and the sampling in ONE launch
    per step, weights read in place and looked up at every call (as :class:`PolicyForward`), the hidden state — the policy's own
    ``memory_*.hidden_states`` tensors, created as zeros at the first step — read and advanced in place.

    ``reset(dones)`` is rsl_rl's ``policy.reset(dones)`` without a launch: it keeps ``dones`` (a ``[N]`` bool or uint8 tensor, read
    in place — the caller leaves it alone until both nets have stepped) as one pending flag row per net; the next launch of a net
    reads zeros for the flagged rows of that net's state and the flag is consumed.  So after a rollout the bootstrap ``value()``
    consumes the critic's pending reset and the first step of the next rollout the actor's, exactly the order rsl_rl's
    ``compute_returns`` (``policy.evaluate(last_obs)`` advances the critic once more) leaves behind.  ``reset(None)`` forgets both states.

    ``mean(obs)`` / ``value(critic_obs)``: an actor-only / critic-only launch that advances that net's state by one step — play-time
    inference and the bootstrap value.  ``RolloutStorage.act_recurrent(forward, obs)``: the collection step.  On a backend without
    the entry (the test-only CPU oracle) every call is the module's torch step under ``no_grad``.

    ``own_state=True``: the forward steps hidden states of its own instead of the policy's memories' — a play-time policy next to a
    training loop (``OnPolicyRunner.get_inference_policy``)."""

    _ENTRY = "mlp_recurrent_act"   # the backend's one-launch step; a backend without it takes the module's torch step

    def __init__(self, policy, own_state: bool = False):
        self._setup(policy, "RecurrentForward", (("actor", nat.GF_MLP_MAX_ACTIONS), ("critic", 1)), "the policy needs an actor and a critic",
                    memories=(("actor", "memory_a"), ("critic", "memory_c")), own_state=own_state)
        self._descriptors(nat.GfMlpRecurrentActArgs)

    def state(self, name: str, n: int, dev) -> tuple:
        """``(h, c)`` of net ``name`` (``c`` None for a GRU), ``[1, n, H]`` each: the memory's own tensors, zeros where it had none."""
        m = self._memory[name]
        H, lstm = m.rnn.hidden_size, self._cell_type[name] == nat.GF_RNN_LSTM
        hs = m.hidden_states
        parts = () if hs is None else (tuple(hs) if lstm else (hs,))
        dev = torch.device(dev)
        same_dev = lambda d: d.type == dev.type and (dev.index is None or d.index == dev.index)
        ok = len(parts) == (2 if lstm else 1) and all(
            s.shape == (1, n, H) and s.dtype == torch.float32 and s.is_contiguous() and same_dev(s.device) and not s.requires_grad for s in parts)
        if hs is not None and not ok:
            raise ValueError(f"RecurrentForward: the hidden state of the {name}'s memory is not [1, {n}, {H}] contiguous float32 on {dev}")
        if hs is None:
            parts = tuple(torch.zeros((1, n, H), device=dev, dtype=torch.float32) for _ in range(2 if lstm else 1))
            m.hidden_states = parts if lstm else parts[0]
        return parts[0], (parts[1] if lstm else None)

    def reset(self, dones=None) -> None:
        if dones is None or getattr(nat.get_backend(), self._ENTRY, None) is None:   # (None, or the test-only oracle backend)
            for m in self._memory.values():
                m.reset(dones)
            if dones is None:
                self._pending = dict.fromkeys(self._pending)
            return
        if not isinstance(dones, torch.Tensor) or dones.dim() != 1 or dones.dtype not in (torch.bool, torch.uint8) or not dones.is_contiguous():
            raise ValueError("RecurrentForward.reset(dones): dones must be a contiguous [N] bool or uint8 tensor")
        flags = dones.view(torch.uint8)
        for name, old in self._pending.items():
            self._pending[name] = flags if old is None else (old | flags)

    def _fill_cell(self, name: str, cell, parts, n: int, save=None) -> tuple:
        """Point ``cell`` at the memory of net ``name``: the current weights, the state (read and advanced in place), the pending
        reset — consumed — and ``save[name] = (h_save, c_save)``.  Returns what must outlive the launch."""
        rnn = self._memory[name].rnn
        h, c = self.state(name, n, parts[0].device)
        flags = self._pending[name]
        if flags is not None and (flags.shape[0] != n or flags.device != parts[0].device):
            raise ValueError(f"RecurrentForward: the pending reset is [{flags.shape[0]}] on {flags.device}; the step has {n} rows on {parts[0].device}")
        self._pending[name] = None
        cell.type, cell.hidden = self._cell_type[name], rnn.hidden_size
        cell.w_ih, cell.w_hh, cell.b_ih, cell.b_hh = (getattr(rnn, p).data_ptr() for p in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"))
        cell.h, cell.c = h.data_ptr(), None if c is None else c.data_ptr()
        cell.reset = None if flags is None else flags.data_ptr()
        cell.h_save = cell.c_save = None
        if save is not None and name in save:
            hs, cs = save[name]
            cell.h_save, cell.c_save = hs.data_ptr(), None if c is None else cs.data_ptr()
        return (parts, h, c, flags)


class _DistillAct:
    """The student–teacher half of :class:`DistillForward` and :class:`RecurrentDistillForward`: ``_args`` is the student–teacher
    descriptor of the collection step, ``_one_args`` an actor–critic one with the student in the actor's slot for ``mean``."""

    def _setup_distill(self, policy, who: str, memories=(), own_state: bool = False) -> None:
        self._setup(policy, who, (("student", nat.GF_MLP_MAX_ACTIONS), ("teacher", nat.GF_MLP_MAX_ACTIONS)), "the policy needs a student and a teacher",
                    memories=memories, own_state=own_state, same_width=True)
        self._descriptors(*((nat.GfMlpRecurrentDistillArgs, nat.GfMlpRecurrentActArgs) if memories else (nat.GfMlpDistillArgs, nat.GfMlpActArgs)))

    def mean(self, obs) -> torch.Tensor:
        """The student's output ``[N, A]`` (``policy.act_mean(obs)``, one more step of its memory where it has one): one launch, a
        fresh tensor."""
        return self._one(obs, "student")

    def act(self, obs, teacher_obs=None, noise: Optional[torch.Tensor] = None, seed: int = 0, stream: int = 0, env_offset: int = 0,
            actions_out: Optional[torch.Tensor] = None, teacher_actions_out: Optional[torch.Tensor] = None, backend=None, save=None):
        """``(actions, teacher_actions)``, fresh ``[N, A]`` tensors: ``Normal(student(obs), std).sample()`` and ``teacher(teacher_obs)``
        (``teacher_obs=None``: the teacher reads ``obs``) in ONE launch of the forward's entry — ``gf_mlp_distill_act``, or, with both
        memories advanced by one step in place, ``gf_mlp_recurrent_distill_act``; ``actions_out`` / ``teacher_actions_out``: contiguous
        ``[N, A]`` rows that receive the same values from the same launch.  ``noise`` / ``seed`` / ``stream`` / ``env_offset``: as
        ``gf_policy_act``'s.  ``save`` (a forward with memories): ``{"student": (h_save, c_save)}`` (``[N, H]`` each, ``c_save`` None
        for a GRU; ``"teacher"`` likewise) receive the state the step started from, after the reset.  On a backend without the entry
        point (the test-only CPU oracle) the same expression runs in torch on the module's step and ``noise`` is required."""
        segs = _segments(obs, "obs", None, None, self._reader("student"))
        n, dev = int(segs[0].shape[0]), segs[0].device
        tsegs = _segments(obs if teacher_obs is None else teacher_obs, "obs (the teacher's input)" if teacher_obs is None else "teacher_obs", n, dev,
                          self._reader("teacher"))
        A = self.num_actions
        std = getattr(self.policy, self._std_name)
        _check_f32(std, f"policy.{self._std_name}", {(A,)}, dev)
        for t, name in ((noise, "noise"), (actions_out, "actions_out"), (teacher_actions_out, "teacher_actions_out")):
            if t is not None:
                _check_f32(t, name, {(n, A)}, dev)
        backend = nat.get_backend() if backend is None else backend
        fn = getattr(backend, self._ENTRY, None)
        if fn is None:   # (the test-only oracle backend) the same expression in torch, from the given draws
            if noise is None:
                raise RuntimeError(f"act() draws its noise in the HIP kernel: on a backend without gf_{self._ENTRY} pass noise=")
            with torch.no_grad():
                for name, dst in (save or {}).items():
                    self._save_torch(name, dst)
                mean, teacher = self._torch_step("student", _cat(segs)), self._torch_step("teacher", _cat(tsegs)).clone()
                actions, _sd = _sample_torch(mean, std, noise, self.std_is_log)
                if actions_out is not None:
                    actions_out.copy_(actions)
                if teacher_actions_out is not None:
                    teacher_actions_out.copy_(teacher)
            return actions, teacher
        actions = torch.empty((n, A), device=dev, dtype=torch.float32)
        teacher = torch.empty((n, A), device=dev, dtype=torch.float32)
        a = self._fill_desc(self._args_parts, n, (("student", "student", segs), ("teacher", "teacher", tsegs)), save)
        _fill_sampling(a, std, self.std_is_log, noise, int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream), int(env_offset), actions)
        a.teacher_actions = teacher.data_ptr()
        a.actions_out = None if actions_out is None else actions_out.data_ptr()
        a.teacher_actions_out = None if teacher_actions_out is None else teacher_actions_out.data_ptr()
        self._keep = (self._keep, noise, actions_out, teacher_actions_out, save)
        fn(self._args)
        return actions, teacher

    def _save_torch(self, name: str, dst) -> None:
        """``h_save`` / ``c_save`` of the torch step: the state of net ``name`` as the step will read it (zeros where there is none)."""
        hs = self._memory[name].hidden_states
        parts = () if hs is None else (tuple(hs) if isinstance(hs, tuple) else (hs,))
        for i, d in enumerate(dst):
            if d is not None:
                d.copy_(parts[i][0]) if parts else d.zero_()


class DistillForward(_DistillAct, _MlpForward):
    """The student and the teacher of a policy (``policy.student`` / ``policy.teacher``, a :class:`StudentTeacherMLP` or anything of
    that shape) as ``gf_mlp_distill_act`` reads them — the counterpart of :class:`PolicyForward`, under its rules: the structure is
    checked once, the weight addresses and the normalisers (``policy.student_obs_normalizer`` / ``teacher_obs_normalizer``) are looked
    up at every call.  Both nets are required and must have the same output width; ``policy.std`` (``log_std``) must be ``[A]``.

    ``mean(obs)``: the student's mean — play-time inference, one ``gf_mlp_act`` launch.  ``act(obs, teacher_obs)``: the collection
    step, ONE ``gf_mlp_distill_act`` launch; ``RolloutStorage.act_distill`` calls it with its rows as the second destinations."""

    _ENTRY = "mlp_distill_act"

    def __init__(self, policy):
        self._setup_distill(policy, "DistillForward")


class RecurrentDistillForward(_DistillAct, RecurrentForward):
    """A recurrent student and its teacher (:class:`StudentTeacherRecurrent`, or rsl_rl's: ``memory_s.rnn`` in front of ``student``,
    optionally ``memory_t.rnn`` in front of ``teacher``) as ``gf_mlp_recurrent_distill_act`` reads them — :class:`DistillForward`'s
    checks for the two nets and ``std``, :class:`RecurrentForward`'s for every memory, weights and normalisers looked up at every call.
    The policy's own ``memory_s`` / ``memory_t`` state tensors (zeros at the first step) are read and advanced in place;
    ``own_state=True`` steps states of its own instead (``DistillationRunner.get_inference_policy``).

    ``reset(dones)``: one pending flag row per net with a memory, consumed by that net's next launch (:class:`RecurrentForward`'s
    scheme); ``reset(None)`` forgets the states.  ``act(obs, teacher_obs, …)``: the collection step, ONE launch — both normalisers,
    both cells, both MLPs, the student's sampling and the rows.  ``mean(obs)``: a student-only ``gf_mlp_recurrent_act`` launch that
    advances ``memory_s`` — play-time inference.  On a backend without the entry (the test-only CPU oracle) every call is the module's
    torch step under ``no_grad``, and ``noise`` is required."""

    _ENTRY = "mlp_recurrent_distill_act"

    def __init__(self, policy, own_state: bool = False):
        memories = (("student", "memory_s"), ("teacher", "memory_t")) if getattr(policy, "memory_t", None) is not None else (("student", "memory_s"),)
        self._setup_distill(policy, "RecurrentDistillForward", memories, own_state)

    def value(self, critic_obs):
        raise ValueError("RecurrentDistillForward: a student–teacher policy has no critic")


def _rnd_reward_torch(rnd: "RandomNetworkDistillation", rnd_state: torch.Tensor, rewards=None, acc_extrinsic=None, acc_intrinsic=None) -> torch.Tensor:
    """rsl_rl's lines: ``get_intrinsic_reward`` and ``rewards += intrinsic``, with ``gf_rnd_reward``'s two per-env accumulators."""
    intrinsic = rnd.get_intrinsic_reward(rnd_state)
    with torch.no_grad():
        if rewards is not None:
            if acc_extrinsic is not None:
                acc_extrinsic += rewards.to(torch.float64)
            rewards.copy_(rewards + intrinsic)
        if acc_intrinsic is not None:
            acc_intrinsic += intrinsic.to(torch.float64)
    return intrinsic


class RndForward:
    """The target and the predictor of a :class:`RandomNetworkDistillation` as ``gf_rnd_reward`` reads them — the counterpart of
    :class:`PolicyForward`, under its rules: the structure is checked once, the weight addresses, the state normaliser and the reward
    normaliser's buffers are looked up at every call (:class:`PPO` re-seats the predictor's parameters into a flat buffer of its own).

    ``reward(rnd_state, rewards=None)``: ``rnd.get_intrinsic_reward(rnd_state)`` as a fresh ``[N]`` tensor — both MLPs, the distance,
    the reward normaliser (its update included, in training mode) and the weight in ONE launch, two with the reward normaliser
    updating, and no host read; ``rewards`` (``[N]``, contiguous) is added to in place by the same launch, ``acc_extrinsic`` /
    ``acc_intrinsic`` (``[N]`` float64) accumulate the two terms per env.  ``rnd_state``: a ``[N, W]`` tensor or up to four segments.
    The embeddings are ``gf_mlp_act``'s fma chains, the normaliser's update is evaluated in float64: within rounding of the module's
    torch lines, not bit for bit.  ``update_counter`` and the schedule's weight advance on the host, as in the module.  For CPU
    tensors and on a backend without the entry point (the test-only CPU oracle) the module's own lines run."""

    def __init__(self, rnd: "RandomNetworkDistillation"):
        if not isinstance(rnd, RandomNetworkDistillation):
            raise ValueError("RndForward(rnd) takes a RandomNetworkDistillation")
        self.rnd = rnd
        self.target = _walk_mlp(rnd.target, "target", nat.GF_MLP_MAX_ACTIONS, "RndForward")
        self.predictor = _walk_mlp(rnd.predictor, "predictor", nat.GF_MLP_MAX_ACTIONS, "RndForward")
        self._state_norm()
        self._args = nat.GfRndRewardArgs()
        self._ws = self._avg_scratch = None

    def _state_norm(self) -> Optional[EmpiricalNormalization]:
        return _as_normalizer(self.rnd.state_normalizer, self.rnd.num_states, "RndForward: rnd.state_normalizer")

    def reward(self, rnd_state, rewards: Optional[torch.Tensor] = None, acc_extrinsic: Optional[torch.Tensor] = None,
               acc_intrinsic: Optional[torch.Tensor] = None, backend=None) -> torch.Tensor:
        rnd = self.rnd
        segs = _segments(rnd_state, "rnd_state", None, None, self.target)
        n, dev = int(segs[0].shape[0]), segs[0].device
        if rewards is not None:
            _check_f32(rewards, "rewards", {(n,)}, dev)
        for acc, name in ((acc_extrinsic, "acc_extrinsic"), (acc_intrinsic, "acc_intrinsic")):
            if acc is not None and (acc.dtype != torch.float64 or tuple(acc.shape) != (n,) or acc.device != dev or not acc.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous float64 [{n}] tensor on {dev}")
        backend = nat.get_backend() if backend is None else backend
        fn = getattr(backend, "rnd_reward", None) if dev.type == "cuda" else None
        if fn is None:
            return _rnd_reward_torch(rnd, _cat(segs), rewards, acc_extrinsic, acc_intrinsic)
        weight = rnd._advance()
        out = torch.empty(n, device=dev, dtype=torch.float32)
        a = self._args
        a.num_envs = n
        norm = self._state_norm()
        _fill_net(a.target, self.target, segs, norm)
        _fill_net(a.predictor, self.predictor, segs, norm)
        a.weight = weight
        need = nat.rnd_workspace_bytes(n) // 8
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty(need, device=dev, dtype=torch.float64)
        rn = rnd.reward_normalizer
        if isinstance(rn, EmpiricalDiscountedVariationNormalization):
            emp = rn.emp_norm
            a.normalize, a.update, a.gamma = 1, 1 if rn.training else 0, rn.gamma
            if rn.training:
                if rn.avg is not None and (tuple(rn.avg.shape) != (n,) or rn.avg.device != dev or not rn.avg.is_contiguous()):
                    raise ValueError(f"RndForward: the reward normaliser keeps {tuple(rn.avg.shape)} discounted sums on {rn.avg.device}; "
                                     f"this call has {n} envs on {dev}")
                a.first = 1 if rn.avg is None else 0
                if rn.avg is None:   # (the first call writes every element)
                    rn.avg = torch.empty(n, device=dev, dtype=torch.float32)
                avg = rn.avg
            else:   # (eval mode: avg is neither read nor written; the descriptor still wants an address)
                a.first = 0
                if self._avg_scratch is None or self._avg_scratch.numel() != n or self._avg_scratch.device != dev:
                    self._avg_scratch = torch.zeros(n, device=dev, dtype=torch.float32)
                avg = self._avg_scratch
            a.avg, a.mean, a.var, a.std, a.count = (t.data_ptr() for t in (avg, emp._mean, emp._var, emp._std, emp.count))
            a.until = -1 if emp.until is None else int(emp.until)
        else:
            a.normalize = a.update = a.first = 0
            a.avg = a.mean = a.var = a.std = a.count = None
        a.rewards = None if rewards is None else rewards.data_ptr()
        a.intrinsic = out.data_ptr()
        a.acc_extrinsic = None if acc_extrinsic is None else acc_extrinsic.data_ptr()
        a.acc_intrinsic = None if acc_intrinsic is None else acc_intrinsic.data_ptr()
        a.workspace, a.workspace_bytes = self._ws.data_ptr(), self._ws.numel() * 8
        self._keep = (segs, rewards, out)
        fn(a)
        return out


class GradientAllReduce:
    """Average the gradients of ``params`` over the ranks of ``group`` with one collective.

    All gradients live in ONE flat, persistent bucket (``param.grad`` are views into it), so the step after ``backward()`` is a
    single ``all_reduce`` of ``numel * 4`` bytes — RCCL's ring over xGMI moves it at link speed instead of paying the launch
    and latency cost of one collective per tensor (the reference policies have 16 parameter tensors).  ``average()`` divides
    by the world size in the same pass.  With one rank (or no process group) it is a no-op, so a training script is the same
    on one GPU and on eight."""

    def __init__(self, params: Iterable[torch.nn.Parameter], group=None, force: bool = False):
        """``force``: run the collective even in a group of ONE rank (the only RCCL group a one-GPU box can form: every call of the
        path executes, the sum over one rank is the identity — tests/test_learner.py)."""
        import torch.distributed as dist

        self.force = bool(force) and dist.is_available() and dist.is_initialized()

        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("no trainable parameters")
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        dev, dt = self.params[0].device, self.params[0].dtype
        self.bucket = torch.zeros(sum(p.numel() for p in self.params), device=dev, dtype=dt)
        off = 0
        for p in self.params:   # gradients are views of the bucket from now on: backward() accumulates straight into it
            p.grad = self.bucket[off:off + p.numel()].view_as(p)
            off += p.numel()
        self._work = None

    @property
    def nbytes(self) -> int:
        return self.bucket.numel() * self.bucket.element_size()

    def zero_grad(self) -> None:
        self.bucket.zero_()      # one memset; optimizer.zero_grad(set_to_none=True) would drop the views

    def average(self, async_op: bool = False):
        """Sum over ranks, divide by the world size.  ``async_op``: returns at once; call ``wait()`` before the optimizer step."""
        if self.world == 1 and not self.force:
            return None
        import torch.distributed as dist

        for p in self.params:    # a parameter whose grad was replaced (set_to_none) would silently leave the bucket
            if p.grad is None or p.grad.data_ptr() < self.bucket.data_ptr() or p.grad.data_ptr() >= self.bucket.data_ptr() + self.nbytes:
                raise RuntimeError("a parameter's .grad no longer lives in the bucket: use GradientAllReduce.zero_grad(), not set_to_none")
        self.bucket.div_(self.world)
        self._work = dist.all_reduce(self.bucket, op=dist.ReduceOp.SUM, group=self.group, async_op=async_op)
        return self._work

    def wait(self) -> None:
        if self._work is not None:
            self._work.wait()
            self._work = None

    def broadcast_parameters(self, src: int = 0) -> None:
        """Make every replica start from rank ``src``'s weights."""
        if self.world == 1 and not self.force:
            return
        import torch.distributed as dist

        for p in self.params:
            dist.broadcast(p.data, src=src, group=self.group)


# ---- the update: rsl_rl PPO.update ---------------------------------------------------------------------------------------------------
_PPO_KEYS = ("clip_param", "desired_kl", "entropy_coef", "gamma", "lam", "learning_rate", "max_grad_norm", "num_learning_epochs",
             "num_mini_batches", "schedule", "use_clipped_value_loss", "value_loss_coef")
_PPO_DEFAULTS = dict(clip_param=0.2, desired_kl=0.01, entropy_coef=0.01, gamma=0.99, lam=0.95, learning_rate=0.001, max_grad_norm=1.0,
                     num_learning_epochs=5, num_mini_batches=4, schedule="adaptive", use_clipped_value_loss=True, value_loss_coef=1.0)
# rsl_rl keys whose default is all this class does: accepted with that value only
_PPO_ONLY_DEFAULT = {"normalize_advantage_per_mini_batch": False}
# rsl_rl's rnd_cfg: RandomNetworkDistillation's keyword arguments (num_states comes from the storage) and the predictor's learning rate
_RND_KEYS = ("num_outputs", "predictor_hidden_dims", "target_hidden_dims", "activation", "weight", "state_normalization",
             "reward_normalization", "weight_schedule", "learning_rate")
_RND_REQUIRED = ("num_outputs", "predictor_hidden_dims", "target_hidden_dims")
_SYMMETRY_KEYS = ("use_data_augmentation", "use_mirror_loss", "mirror_loss_coeff", "data_augmentation_func")   # rsl_rl's symmetry_cfg
_ADAM_BETAS, _ADAM_EPS = (0.9, 0.999), 1e-8   # torch.optim.Adam's defaults, as rsl_rl constructs it


class _FlatAdam:
    """What :class:`PPO` and :class:`Distillation` share: the trainable parameters of ``grad_sync`` (a :class:`GradientAllReduce`) as
    views of ONE flat buffer in the bucket's order, flat Adam moments, the device control block (lr as a double, the step), the
    ``gf_adam_step`` call with its torch twin, and the optimizer state in ``torch.optim.Adam``'s format.  The host class provides
    ``grad_sync``, ``max_grad_norm``, ``adaptive``, ``desired_kl`` and — for the adaptive schedule — ``_out`` with ``kl_mean`` at [3]."""

    def _init_flat(self, learning_rate: float) -> None:
        sync = self.grad_sync
        # the parameters as views of one flat buffer, in the bucket's order
        self.params = torch.empty_like(sync.bucket)
        off = 0
        with torch.no_grad():
            for p in sync.params:
                k = p.numel()
                self.params[off:off + k].copy_(p.data.reshape(-1))
                p.data = self.params[off:off + k].view_as(p)
                off += k
        dev = self.params.device
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.params), torch.zeros_like(self.params)
        # device control block: GfAdamState[2] = {lr (double), step (int64)} x 2, read at parity, written at 1 - parity
        self._state = torch.zeros(4, device=dev, dtype=torch.int64)
        self._state_lr = self._state.view(torch.float64)
        self._state_lr[0] = float(learning_rate)
        self._calls = 0
        self._adam_ws = torch.zeros(max(1, nat.adam_workspace_bytes(self.params.numel()) // 8), device=dev, dtype=torch.float64)
        self._adam_args = nat.GfAdamArgs()

    @property
    def learning_rate(self) -> float:
        """The current learning rate (one host read)."""
        return float(self._state_lr[2 * (self._calls & 1)])

    # -- the optimizer state, in torch.optim.Adam's format ---------------------------------------------------------------------------
    def optimizer_state_dict(self) -> dict:
        """What ``torch.optim.Adam(policy.parameters(), lr).state_dict()`` would hold now (rsl_rl's ``"optimizer_state_dict"``):
        ``"state"`` — ``{i: {"step", "exp_avg", "exp_avg_sq"}}`` for parameter ``i`` of the bucket's order (``policy.parameters()``'s),
        the moments as clones shaped like the parameter, ``step`` the 0-dim tensor the installed torch writes; ``{}`` before the first
        step, as torch's — and one ``"param_groups"`` entry with the installed torch's own keys, the current ``lr`` (one host read),
        the module's betas and eps, and ``params = [0 … P-1]``."""
        # the group's keys and the step's dtype and device come from the installed torch: a throw-away Adam that takes one step
        dummy = torch.nn.Parameter(torch.zeros(1))
        dummy.grad = torch.zeros(1)
        probe = torch.optim.Adam([dummy], lr=1.0)
        probe.step()
        probe = probe.state_dict()
        step_like = probe["state"][0]["step"]
        params = self.grad_sync.params
        group = dict(probe["param_groups"][0], lr=self.learning_rate, betas=_ADAM_BETAS, eps=_ADAM_EPS, params=list(range(len(params))))
        state, off = {}, 0
        if self._calls > 0:
            for i, p in enumerate(params):
                k = p.numel()
                state[i] = {"step": torch.full_like(step_like, self._calls),
                            "exp_avg": self.exp_avg[off:off + k].view_as(p).clone(), "exp_avg_sq": self.exp_avg_sq[off:off + k].view_as(p).clone()}
                off += k
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd: dict) -> None:
        """The inverse: the moments are copied into the flat ``exp_avg`` / ``exp_avg_sq`` in place, ``lr`` and ``step`` go into the slot
        of the control block the next ``gf_adam_step`` reads.  An empty ``"state"`` zeroes the moments and the step.  ``ValueError`` for
        what this Adam cannot continue from: another parameter count or shape, ``step`` values that differ between the parameters,
        ``amsgrad`` / ``weight_decay`` / ``maximize`` off their defaults, betas or eps other than this module's."""
        who = f"{type(self).__name__}.load_optimizer_state_dict"
        groups = sd.get("param_groups") if isinstance(sd, dict) else None
        if not isinstance(groups, (list, tuple)) or len(groups) != 1 or not isinstance(sd.get("state"), dict):
            raise ValueError(f"{who}: expected torch.optim.Adam's {{'state', 'param_groups'}} with one parameter group")
        group, state, params = groups[0], sd["state"], self.grad_sync.params
        if len(group.get("params", ())) != len(params):
            raise ValueError(f"{who}: the state holds {len(group.get('params', ()))} parameters, the policy {len(params)}")
        for key, default in (("amsgrad", False), ("weight_decay", 0), ("maximize", False)):
            if group.get(key, default) != default:
                raise ValueError(f"{who}: {key}={group[key]!r} is not supported (only Adam's default {default!r})")
        if tuple(float(b) for b in group.get("betas", _ADAM_BETAS)) != _ADAM_BETAS:
            raise ValueError(f"{who}: betas={tuple(group['betas'])!r}; this Adam steps with {_ADAM_BETAS}")
        if float(group.get("eps", _ADAM_EPS)) != _ADAM_EPS:
            raise ValueError(f"{who}: eps={group['eps']!r}; this Adam steps with {_ADAM_EPS}")
        if "lr" not in group:
            raise ValueError(f"{who}: the parameter group has no lr")
        lr, step = float(group["lr"]), 0
        if state:
            ids = list(group["params"])
            if sorted(state) != sorted(ids):
                raise ValueError(f"{who}: the state covers parameters {sorted(state)}, the group lists {sorted(ids)}: a different parameter count")
            for i, p in zip(ids, params):
                for name in ("step", "exp_avg", "exp_avg_sq"):
                    if name not in state[i]:
                        raise ValueError(f"{who}: parameter {i} has no {name}")
                for name in ("exp_avg", "exp_avg_sq"):
                    if tuple(state[i][name].shape) != tuple(p.shape):
                        raise ValueError(f"{who}: {name} of parameter {i} has shape {tuple(state[i][name].shape)}, the parameter {tuple(p.shape)}")
            steps = {float(state[i]["step"]) for i in ids}
            step = int(steps.pop())
            if steps or step < 0:
                raise ValueError(f"{who}: the parameters' step values are not all equal (one flat bucket takes one step count)")
        with torch.no_grad():
            if state:
                off = 0
                for i, p in zip(ids, params):
                    k = p.numel()
                    self.exp_avg[off:off + k].view_as(p).copy_(state[i]["exp_avg"])
                    self.exp_avg_sq[off:off + k].view_as(p).copy_(state[i]["exp_avg_sq"])
                    off += k
            else:
                self.exp_avg.zero_()
                self.exp_avg_sq.zero_()
            par = step & 1   # (the slot the next step reads: every step reads `_calls & 1` and writes the other)
            self._state_lr[2 * par] = lr
            self._state[2 * par + 1] = step
        self._calls = step

    def _adam_step(self, backend) -> None:
        """One optimizer step over the flat bucket: ``gf_adam_step``, or its torch twin on a backend without it (the test-only
        oracle backend, whose losses went through autograd)."""
        if getattr(backend, "adam_step", None) is not None:
            self._adam_hip(backend)
        else:
            self._adam_torch()

    def _adam_hip(self, backend) -> None:
        a, par = self._adam_args, self._calls & 1
        a.numel = self.params.numel()
        a.params, a.grads, a.exp_avg, a.exp_avg_sq = (t.data_ptr() for t in (self.params, self.grad_sync.bucket, self.exp_avg, self.exp_avg_sq))
        a.state = self._state.data_ptr()
        a.kl_mean = self._out.data_ptr() + 3 * 4 if self.adaptive else None
        a.workspace, a.workspace_bytes = self._adam_ws.data_ptr(), self._adam_ws.numel() * 8
        a.desired_kl = self.desired_kl if self.adaptive else 0.0
        a.beta1, a.beta2, a.eps = _ADAM_BETAS[0], _ADAM_BETAS[1], _ADAM_EPS
        a.max_grad_norm = self.max_grad_norm
        a.schedule = nat.GF_ADAM_SCHEDULE_ADAPTIVE if self.adaptive else nat.GF_ADAM_SCHEDULE_FIXED
        a.parity = par
        backend.adam_step(a)
        self._calls += 1

    def _adam_torch(self) -> None:
        """The schedule, ``clip_grad_norm_`` and torch.optim.Adam's foreach arithmetic as tensor operations (no host read)."""
        par = self._calls & 1
        with torch.no_grad():
            lr = self._state_lr[2 * par].clone()
            if self.adaptive:
                kl = self._out[3]   # (float32 against a Python float: compared in float32, as rsl_rl's `kl_mean > desired_kl * 2.0`)
                down = torch.clamp(lr / 1.5, min=1e-5)
                up = torch.clamp(lr * 1.5, max=1e-2)
                lr = torch.where(kl > self.desired_kl * 2.0, down, torch.where((kl < self.desired_kl / 2.0) & (kl > 0.0), up, lr))
            step = self._calls + 1
            g = self.grad_sync.bucket
            torch.nn.utils.clip_grad_norm_(self.grad_sync.params, self.max_grad_norm)
            b1, b2 = _ADAM_BETAS
            bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
            step_size = ((lr / bc1) * -1).to(torch.float32)
            self.exp_avg.lerp_(g, 1 - b1)
            self.exp_avg_sq.mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = (self.exp_avg_sq.sqrt() / (bc2 ** 0.5)).add_(_ADAM_EPS)
            self.params.add_(step_size * (self.exp_avg / denom))
            self._state_lr[2 * (1 - par)] = lr
            self._state[2 * (1 - par) + 1] = step
        self._calls += 1


class _RndOptimizer(_FlatAdam):
    """The predictor's Adam of a :class:`PPO` with an ``rnd_cfg``: its parameters in a flat buffer and a bucket of their own, a fixed
    schedule and no clipping (the largest finite float as ``max_grad_norm``: a clip coefficient of exactly 1, Distillation's form)."""

    def __init__(self, rnd: "RandomNetworkDistillation", learning_rate: float):
        self.grad_sync = GradientAllReduce(rnd.predictor.parameters())   # (one rank: a bucket, never a collective)
        self.max_grad_norm = torch.finfo(torch.float32).max
        self.schedule, self.adaptive, self.desired_kl = "fixed", False, None
        self._init_flat(float(learning_rate))


class PPO(_FlatAdam):
    """rsl_rl's ``PPO`` (non-recurrent) over a :class:`RolloutStorage` and an :class:`ActorCriticMLP`.

    ``PPO(policy, storage, **train_cfg["algorithm"])`` takes the dict of ``examples/*/train.py`` as written (``class_name`` is
    ignored); unknown keys and unsupported values raise ``ValueError``.  ``grad_sync``: the :class:`GradientAllReduce` of a multi-rank
    run (a one-rank bucket is made otherwise).  At construction the policy's trainable parameters move into ONE flat buffer in the
    bucket's order (each ``p.data`` becomes a view of it) and the Adam state, the workspaces and the device control block (lr as a
    double, the step) are allocated once.

    Per minibatch ``update()`` zeroes the bucket, runs the actor / critic forward, ``gf_ppo_loss`` (the loss, its gradient w.r.t.
    mu / value / std — or log_std, for a ``noise_std_type="log"`` policy: the kernel exponentiates it and returns
    ``d loss / d log_std``), back-propagates the kernel's gradients, all-reduces ``kl_mean`` over the ranks when there are several,
    averages the bucket, and ``gf_adam_step`` (schedule, clipping, Adam) — no host synchronisation; the returned means are one read
    at the end.  On a backend without these entry points (the test-only CPU oracle) the same arithmetic runs in torch.

    A policy with observation normalisers (:class:`EmpiricalNormalization` as ``policy.actor_obs_normalizer`` /
    ``critic_obs_normalizer``) gets its minibatches normalised by the gather's own launch and ``policy.actor`` / ``policy.critic``
    run on them directly — the statistics are frozen during an update, so this is rsl_rl's ``policy.act(obs_batch)``.  The
    collection loop updates them where rsl_rl's ``process_env_step`` does::

        actions = storage.act_policy(forward, obs)
        obs, rew, term, trunc, extras = env.step(actions)
        policy.update_normalization(obs)
        storage.process_env_step(trunc, gamma=ppo.gamma, episodes=stats)

    ``symmetry_cfg`` (rsl_rl's dict: ``use_data_augmentation``, ``use_mirror_loss``, ``mirror_loss_coeff``, ``data_augmentation_func``)
    is honoured when its function is a :class:`~genesis_forge_amd.symmetry.MirrorSymmetry` whose tables fit the policy input, the
    critic input and the actions; anything else — no function, a string, a plain callable (the HIP path runs tables, not Python),
    other widths, other keys — raises ``ValueError``.  Augmentation: the minibatch is gathered raw, ONE ``gf_mirror_rows`` writes the
    originals and their mirrors (observations through the normalisers, actions, the four replicated per-row scalars), the actor and
    the critic run on ``2·mb`` rows and ``gf_ppo_loss`` takes the KL of the schedule from the first ``mb`` (``kl_rows``).  The symmetry
    loss ``MSE(actor(mirror(obs)), mirror(actor(obs)).detach())`` is one ``gf_mirror_loss``: on the ``mu`` of that forward when
    augmenting, on one extra actor forward of the mirrored rows otherwise; its gradient joins the update only with
    ``use_mirror_loss`` (``mirror_loss_coeff`` times), and ``update()`` returns its mean as ``"symmetry"`` either way.

    ``rnd_cfg`` (rsl_rl's dict: :class:`RandomNetworkDistillation`'s keyword arguments and ``learning_rate``, default ``1e-3``) adds
    random network distillation: ``self.rnd`` is the module, ``num_states`` the width of the storage's ``"rnd_state"`` observation
    group.  The collection loop adds the intrinsic reward between ``update_normalization`` and ``process_env_step``::

        ppo.rnd.update_normalization(rnd_state)
        storage.intrinsic_reward(RndForward(ppo.rnd), rnd_state)      # rewards[t] += intrinsic: gf_rnd_reward

    and every minibatch also trains the predictor: ``storage.group_rows_batch("rnd_state", indices, state normaliser)`` (one gather
    launch; with augmentation the original rows only), the two nets' forward in torch, ``gf_bc_loss`` (mse) for
    ``MSE(predictor(s), target(s))`` and its gradient, and a ``gf_adam_step`` of the predictor's own flat Adam — fixed schedule, no
    clipping, one rank.  ``update()`` returns the mean loss as ``"rnd"``.  A storage without that group, a missing
    ``num_outputs`` / ``predictor_hidden_dims`` / ``target_hidden_dims``, an unknown key, a bad ``weight_schedule``, another
    activation than ``"elu"`` or a multi-rank ``grad_sync`` raises ``ValueError`` naming ``rnd_cfg``.

    A recurrent policy (``policy.is_recurrent``: :class:`ActorCriticRecurrent`) is updated on the trajectory minibatches of
    ``storage.recurrent_mini_batch_generator`` — contiguous env ranges, not shuffled, ``generator`` unused: the memories run over the
    padded sequences from the stored initial states in torch (BPTT is ``nn.LSTM`` / ``nn.GRU``'s), ``mu`` / ``value`` ``[T·envs, ·]``
    go through the same ``gf_ppo_loss`` and ``gf_adam_step`` with the rnn parameters in the flat bucket; one more host read per
    update (the trajectory offsets).  The rollout is collected with ``storage.act_recurrent`` (or ``storage.keep_rnn_start(policy)``
    before a rollout on the module's torch step).  ``symmetry_cfg`` or ``rnd_cfg`` with such a policy raises ``ValueError`` naming the key.
    """

    def __init__(self, policy: "ActorCriticMLP", storage: RolloutStorage, grad_sync: Optional[GradientAllReduce] = None, **algorithm):
        algorithm = dict(algorithm)
        algorithm.pop("class_name", None)
        symmetry_cfg = algorithm.pop("symmetry_cfg", None)
        rnd_cfg = algorithm.pop("rnd_cfg", None)
        bad = [k for k in algorithm if k not in _PPO_KEYS and k not in _PPO_ONLY_DEFAULT]
        if bad:
            raise ValueError(f"PPO: unsupported algorithm keys {sorted(bad)}")
        for k, want in _PPO_ONLY_DEFAULT.items():
            if k in algorithm and algorithm[k] != want:
                raise ValueError(f"PPO: {k}={algorithm[k]!r} is not supported (only {want!r})")
        cfg = dict(_PPO_DEFAULTS, **{k: v for k, v in algorithm.items() if k in _PPO_KEYS})
        if cfg["schedule"] not in ("adaptive", "fixed"):
            raise ValueError(f"PPO: schedule={cfg['schedule']!r} is not supported ('adaptive' or 'fixed')")
        if int(cfg["num_learning_epochs"]) < 1 or int(cfg["num_mini_batches"]) < 1:
            raise ValueError("PPO: num_learning_epochs and num_mini_batches must be >= 1")
        if not float(cfg["max_grad_norm"]) > 0.0:
            raise ValueError(f"PPO: max_grad_norm={cfg['max_grad_norm']!r} must be > 0")
        if cfg["schedule"] == "adaptive" and cfg["desired_kl"] is not None and not float(cfg["desired_kl"]) > 0.0:
            raise ValueError(f"PPO: desired_kl={cfg['desired_kl']!r} must be > 0")
        self.policy, self.storage = policy, storage
        self.clip_param, self.entropy_coef, self.value_loss_coef = float(cfg["clip_param"]), float(cfg["entropy_coef"]), float(cfg["value_loss_coef"])
        self.gamma, self.lam, self.max_grad_norm = float(cfg["gamma"]), float(cfg["lam"]), float(cfg["max_grad_norm"])
        self.num_learning_epochs, self.num_mini_batches = int(cfg["num_learning_epochs"]), int(cfg["num_mini_batches"])
        self.use_clipped_value_loss = bool(cfg["use_clipped_value_loss"])
        self.schedule = cfg["schedule"]
        self.desired_kl = None if cfg["desired_kl"] is None else float(cfg["desired_kl"])
        self.adaptive = self.schedule == "adaptive" and self.desired_kl is not None   # (rsl_rl: `if desired_kl is not None and schedule == "adaptive"`)
        std, _is_log = _policy_std(policy)
        if std is None or std.dim() != 1:
            raise ValueError("PPO needs a policy with act_mean(), evaluate() and a [A] std (or, with noise_std_type='log', log_std) parameter (ActorCriticMLP)")
        self.num_actions = int(std.numel())
        self.recurrent = bool(getattr(policy, "is_recurrent", False))
        for key, cfg_ in (("symmetry_cfg", symmetry_cfg), ("rnd_cfg", rnd_cfg)):
            if self.recurrent and cfg_ is not None:
                raise ValueError(f"PPO: {key} is not supported with a recurrent policy")
        self.symmetry = self._parse_symmetry(symmetry_cfg)   # None, or {"func", "augment", "mirror", "coeff"}
        self.rnd, rnd_lr = self._parse_rnd(rnd_cfg, grad_sync, std.device)   # None, or the RandomNetworkDistillation
        self.grad_sync = grad_sync if grad_sync is not None else GradientAllReduce(policy.parameters())
        sync = self.grad_sync
        ids = {id(p) for p in sync.params}
        if any(p.requires_grad and id(p) not in ids for p in policy.parameters()) or id(std) not in ids:
            raise ValueError("grad_sync must hold every trainable parameter of the policy")
        self._init_flat(float(cfg["learning_rate"]))
        dev = self.params.device
        self._out = torch.zeros(nat.GF_PPO_OUT_COUNT, device=dev, dtype=torch.float32)   # surrogate, value_loss, entropy, kl_mean, loss
        self._sums = torch.zeros(5, device=dev, dtype=torch.float64)                      # value_function, surrogate, entropy, symmetry, rnd
        self._rnd_opt = None if self.rnd is None else _RndOptimizer(self.rnd, rnd_lr)
        self._rnd_loss_args, self._rnd_key = nat.GfBcLossArgs(), None
        self._rnd_out = torch.zeros(1, device=dev, dtype=torch.float32)
        self._mb_key = None
        self._loss_args = nat.GfPpoLossArgs()
        if self.symmetry is not None:   # the tables go up here, once: no copy from the host inside an update
            for kind in ("policy", "critic", "actions"):
                self.symmetry["func"].tables(kind, dev)
        self._sym_key = None
        self._mir_args, self._mir_loss_args = nat.GfMirrorRowsArgs(), nat.GfMirrorLossArgs()

    def _parse_symmetry(self, cfg) -> Optional[dict]:
        """rsl_rl's ``symmetry_cfg`` as this class runs it, or ``ValueError`` (always naming ``symmetry_cfg``)."""
        from .symmetry import MirrorSymmetry

        if cfg is None:
            return None
        if not isinstance(cfg, dict):
            raise ValueError(f"PPO: symmetry_cfg={cfg!r} must be a dict (or None)")
        bad = sorted(k for k in cfg if k not in _SYMMETRY_KEYS)
        if bad:
            raise ValueError(f"PPO: symmetry_cfg has unsupported keys {bad} (honoured: {list(_SYMMETRY_KEYS)})")
        fn = cfg.get("data_augmentation_func")
        if fn is None:
            raise ValueError("PPO: symmetry_cfg needs a data_augmentation_func (a MirrorSymmetry): without one there is nothing to mirror with")
        if isinstance(fn, str):
            raise ValueError(f"PPO: symmetry_cfg data_augmentation_func={fn!r} is a string; pass the MirrorSymmetry object itself "
                             "(nothing is resolved by name)")
        if not isinstance(fn, MirrorSymmetry):
            raise ValueError(f"PPO: symmetry_cfg data_augmentation_func is {type(fn).__name__}: the HIP path cannot run a Python callable — "
                             "it mirrors with the validated tables of a genesis_forge_amd.MirrorSymmetry")
        st = self.storage
        width = lambda group: sum(st._widths[m] for m in st.obs_groups[group])
        for what, have, want in (("policy observation", fn.obs_width, width("policy")), ("critic observation", fn.critic_obs_width, width("critic")),
                                 ("action", fn.num_actions, self.num_actions)):
            if have != want:
                raise ValueError(f"PPO: symmetry_cfg: the {what} table of the MirrorSymmetry is {have} wide, the {what} {want}")
        return {"func": fn, "augment": bool(cfg.get("use_data_augmentation", False)), "mirror": bool(cfg.get("use_mirror_loss", False)),
                "coeff": float(cfg.get("mirror_loss_coeff", 0.0))}

    def _parse_rnd(self, cfg, grad_sync, device):
        """rsl_rl's ``rnd_cfg`` as ``(RandomNetworkDistillation on device, the predictor's lr)``, ``(None, None)`` without one, or
        ``ValueError`` (always naming ``rnd_cfg``)."""
        if cfg is None:
            return None, None
        if not isinstance(cfg, dict):
            raise ValueError(f"PPO: rnd_cfg={cfg!r} must be a dict (or None)")
        bad = sorted(k for k in cfg if k not in _RND_KEYS)
        if bad:
            raise ValueError(f"PPO: rnd_cfg has unsupported keys {bad} (honoured: {list(_RND_KEYS)})")
        missing = [k for k in _RND_REQUIRED if k not in cfg]
        if missing:
            raise ValueError(f"PPO: rnd_cfg needs {missing}")
        st = self.storage
        if not st.obs_groups.get("rnd_state"):
            raise ValueError("PPO: rnd_cfg needs a storage with an 'rnd_state' observation group (obs_groups={..., 'rnd_state': [...]})")
        if grad_sync is not None and grad_sync.world > 1:
            raise ValueError("PPO: rnd_cfg runs on one rank: the predictor's gradients are not averaged over a multi-rank grad_sync")
        kwargs = {k: v for k, v in cfg.items() if k != "learning_rate"}
        lr = float(cfg.get("learning_rate", 1e-3))
        if not lr > 0.0:
            raise ValueError(f"PPO: rnd_cfg learning_rate={cfg['learning_rate']!r} must be > 0")
        try:
            rnd = RandomNetworkDistillation(sum(st._widths[m] for m in st.obs_groups["rnd_state"]), **kwargs)
        except (ValueError, TypeError) as e:
            raise ValueError(f"PPO: rnd_cfg: {e}") from e
        return rnd.to(device), lr

    def rnd_optimizer_state_dict(self) -> dict:
        """rsl_rl's ``"rnd_optimizer_state_dict"``: ``torch.optim.Adam``'s format over ``rnd.predictor.parameters()``."""
        return self._rnd_opt.optimizer_state_dict()

    def load_rnd_optimizer_state_dict(self, sd: dict) -> None:
        self._rnd_opt.load_optimizer_state_dict(sd)

    def _rnd_step(self, backend, indices: torch.Tensor) -> None:
        """rsl_rl PPO.update's RND lines for one minibatch: the predictor is regressed onto the target on the batch's rnd_state rows
        (row ``t`` of the transitions, through the state normaliser) and its own Adam steps."""
        rnd, opt = self.rnd, self._rnd_opt
        opt.grad_sync.zero_grad()
        norm = rnd.state_normalizer if isinstance(rnd.state_normalizer, EmpiricalNormalization) else None
        s = self.storage.group_rows_batch("rnd_state", indices, norm)
        pred = rnd.predictor(s)
        with torch.no_grad():
            tgt = rnd.target(s)
        if getattr(backend, "bc_loss", None) is not None:
            mb, E = int(pred.shape[0]), int(pred.shape[1])
            if self._rnd_key != (mb, E):
                self._rnd_grad = torch.empty((mb, E), device=pred.device, dtype=torch.float32)
                self._rnd_ws = torch.empty(max(1, nat.bc_loss_workspace_bytes(mb) // 8), device=pred.device, dtype=torch.float64)
                self._rnd_key = (mb, E)
            a = self._rnd_loss_args
            a.num_rows, a.num_actions, a.loss_type = mb, E, nat.GF_BC_LOSS_MSE
            a.mu, a.target, a.grad = pred.data_ptr(), tgt.data_ptr(), self._rnd_grad.data_ptr()
            a.out, a.sums = self._rnd_out.data_ptr(), self._sums.data_ptr() + 4 * 8
            a.workspace, a.workspace_bytes = self._rnd_ws.data_ptr(), self._rnd_ws.numel() * 8
            self._keep_rnd = (pred, tgt, s)
            backend.bc_loss(a)
            torch.autograd.backward(pred, self._rnd_grad)
        else:   # (the test-only oracle backend) rsl_rl's lines with autograd
            loss = torch.nn.functional.mse_loss(pred, tgt)
            loss.backward()
            with torch.no_grad():
                self._sums[4].add_(loss.detach().to(torch.float64))
        opt._adam_step(backend)

    def compute_returns(self, last_critic_obs: torch.Tensor) -> None:
        """rsl_rl ``PPO.compute_returns``: the critic's value of the bootstrap observation, then GAE over the storage.  The value is
        torch's forward (so results stay what they were); a loop that wants the one-launch forward passes
        ``PolicyForward(policy).value(last_critic_obs)`` to ``storage.compute_returns`` itself.

        With a recurrent policy this is rsl_rl's ``policy.evaluate(last_obs)`` in step mode: the critic's hidden state advances once
        more — by the bootstrap observation, after the rollout's last reset — and the next rollout's first critic step goes on from
        there, while the actor's state waits (with its last reset still to be applied) for the next rollout's first step.  A loop on
        :class:`RecurrentForward` passes ``forward.value(last_critic_obs)`` to ``storage.compute_returns`` for the same step in one
        launch: it consumes the critic's pending reset, the actor's stays pending."""
        with torch.no_grad():
            last_values = self.policy.evaluate(last_critic_obs)
        self.storage.compute_returns(last_values, gamma=self.gamma, lam=self.lam)

    def update(self, generator: Optional[torch.Generator] = None) -> Dict[str, float]:
        """``num_learning_epochs x num_mini_batches`` minibatches of ``storage.mini_batch_generator`` (``generator``: its randperm's);
        returns rsl_rl 3.x's ``{"value_function", "surrogate", "entropy"}`` means — and ``"symmetry"`` with a ``symmetry_cfg``, ``"rnd"`` with an ``rnd_cfg`` — the one
        host read of the update."""
        self._sums.zero_()
        norms = self._normalizers()
        if self.recurrent:
            for batch in self.storage.recurrent_mini_batch_generator(self.num_mini_batches, self.num_learning_epochs, norms):
                self._minibatch_recurrent(batch)
        elif self.symmetry is None:
            for batch in self.storage.mini_batch_generator(self.num_mini_batches, self.num_learning_epochs, generator=generator,
                                                           obs_normalizer=norms[0], critic_obs_normalizer=norms[1]):
                self._minibatch(batch, norms)
        else:
            for batch in self._symmetry_batches(generator, norms):
                self._minibatch_symmetry(batch, norms)
        vf, surr, ent, symm, rnd = self._sums.tolist()
        k = self.num_learning_epochs * self.num_mini_batches
        out = {"value_function": vf / k, "surrogate": surr / k, "entropy": ent / k}
        if self.symmetry is not None:
            out["symmetry"] = symm / k
        if self.rnd is not None:
            out["rnd"] = rnd / k
        return out

    def _symmetry_batches(self, generator, norms) -> Iterator[MiniBatch]:
        """The minibatches ``_minibatch_symmetry`` takes: the observations RAW (the mirror is taken of the raw value; ``gf_mirror_rows``
        normalises), the critic's rows too when augmenting — otherwise they are not mirrored and the gather normalises them as ever."""
        critic_norm = None if self.symmetry["augment"] else norms[1]
        return self.storage.mini_batch_generator(self.num_mini_batches, self.num_learning_epochs, generator=generator,
                                                 obs_normalizer=None, critic_obs_normalizer=critic_norm)

    # -- one minibatch ------------------------------------------------------------------------------------------------------------
    def _normalizers(self):
        """The policy's (actor, critic) observation normalisers that are EmpiricalNormalization; None for Identity / a missing one."""
        pick = lambda m: m if isinstance(m, EmpiricalNormalization) else None
        return pick(getattr(self.policy, "actor_obs_normalizer", None)), pick(getattr(self.policy, "critic_obs_normalizer", None))

    def _minibatch(self, b: MiniBatch, norms=(None, None)) -> None:
        """``norms``: the normalisers the batch's ``obs`` / ``critic_obs`` have already been through (the gather applied them)."""
        sync, policy = self.grad_sync, self.policy
        sync.zero_grad()
        mu = policy.act_mean(b.obs) if norms[0] is None else policy.actor(b.obs)
        value = policy.evaluate(b.critic_obs) if norms[1] is None else policy.critic(b.critic_obs)
        backend = self.storage.env.backend
        hip = getattr(backend, "ppo_loss", None) is not None   # (else the test-only oracle backend: rsl_rl's expression, autograd, torch Adam)
        if hip:
            gmu, gval = self._loss_hip(backend, mu, value, b)
            torch.autograd.backward((mu, value), (gmu, gval.view_as(value)))
        else:
            self._loss_torch(mu, value, b)
        self._reduce_kl()
        sync.average()
        sync.wait()
        self._adam_step(backend)
        if self.rnd is not None:
            self._rnd_step(backend, b.indices)

    # -- one minibatch with a symmetry_cfg ---------------------------------------------------------------------------------------------
    def _minibatch_recurrent(self, rb: RecurrentMiniBatch) -> None:
        """One minibatch of trajectories: the memories run over the padded sequences from their initial states in torch (BPTT is
        ``nn.LSTM`` / ``nn.GRU``'s), the un-padded outputs ``[T, envs, H]`` go through the MLPs, and ``mu`` / ``value`` ``[T·envs, ·]``
        through the loss, clipping and Adam of ``_minibatch``.  The observations come normalised from the gather."""
        sync, policy = self.grad_sync, self.policy
        sync.zero_grad()
        mu = policy.actor(policy.memory_a(rb.obs, rb.masks, rb.hid_a, rb.unpad_index))
        value = policy.critic(policy.memory_c(rb.critic_obs, rb.masks, rb.hid_c, rb.unpad_index))
        mu, value, b = mu.reshape(-1, mu.shape[-1]), value.reshape(-1, 1), rb.rows
        backend = self.storage.env.backend
        if getattr(backend, "ppo_loss", None) is not None:
            gmu, gval = self._loss_hip(backend, mu, value, b)
            torch.autograd.backward((mu, value), (gmu, gval.view_as(value)))
        else:
            self._loss_torch(mu, value, b)
        self._reduce_kl()
        sync.average()
        sync.wait()
        self._adam_step(backend)

    def _minibatch_symmetry(self, b: MiniBatch, norms=(None, None)) -> None:
        """One minibatch of ``_symmetry_batches`` (rsl_rl PPO.update with ``symmetry``).  ``norms``: the policy's normalisers —
        applied here, by ``gf_mirror_rows`` (or by the policy's own modules on a backend without it)."""
        sync, backend = self.grad_sync, self.storage.env.backend
        sync.zero_grad()
        if getattr(backend, "mirror_rows", None) is None:   # (the test-only oracle backend) the same arithmetic in torch
            self._symmetry_torch(b)
        else:
            self._symmetry_hip(backend, b, norms)
        self._reduce_kl()
        sync.average()
        sync.wait()
        self._adam_step(backend)
        if self.rnd is not None:
            self._rnd_step(backend, b.indices)

    def _symmetry_torch(self, b: MiniBatch) -> None:
        """rsl_rl's lines through the MirrorSymmetry's ``__call__`` (plain torch): ``b`` carries raw observations, the policy's own
        normaliser modules apply (``act_mean`` / ``evaluate``) — except the critic's rows of a batch that is not augmented, which the
        gather normalised."""
        sym, policy = self.symmetry, self.policy
        fn, mb = sym["func"], int(b.actions.shape[0])
        if sym["augment"]:
            obs, actions = fn(obs=b.obs, actions=b.actions, env=self.storage.env, obs_type="policy")
            critic_obs, _ = fn(obs=b.critic_obs, actions=None, env=self.storage.env, obs_type="critic")
            rep = lambda t: t.repeat(fn.num_aug)
            b2 = b._replace(obs=obs, critic_obs=critic_obs, actions=actions, values=rep(b.values), advantages=rep(b.advantages),
                            returns=rep(b.returns), old_log_prob=rep(b.old_log_prob))
            mu, value = policy.act_mean(obs), policy.evaluate(critic_obs)
            mu_all = mu
        else:
            b2 = b
            mu = policy.act_mean(b.obs)
            normed = isinstance(getattr(policy, "critic_obs_normalizer", None), EmpiricalNormalization)
            value = policy.critic(b.critic_obs) if normed else policy.evaluate(b.critic_obs)
            obs2, _ = fn(obs=b.obs, actions=None, env=self.storage.env, obs_type="policy")
            with contextlib.nullcontext() if sym["mirror"] else torch.no_grad():
                mu_all = torch.cat([mu, policy.act_mean(obs2[mb:])], dim=0)
        _, target = fn(obs=None, actions=mu_all[:mb].detach(), env=self.storage.env)
        symmetry_loss = torch.nn.functional.mse_loss(mu_all[mb:], target[mb:])
        self._loss_torch(mu, value, b2, kl_rows=mb if sym["augment"] else 0, extra=sym["coeff"] * symmetry_loss if sym["mirror"] else None)
        with torch.no_grad():
            self._sums[3].add_(symmetry_loss.detach().to(torch.float64))

    def _symmetry_buffers(self, mb: int, critic_too: bool):
        """The destinations of ``gf_mirror_rows`` for ``mb`` original rows, kept from minibatch to minibatch (the graph of a minibatch
        is gone before the next one writes them)."""
        fn = self.symmetry["func"]
        key = (mb, critic_too)
        if self._sym_key != key:
            dev = self.params.device
            e = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
            self._sym_obs = e(2 * mb, fn.obs_width)
            self._sym_critic = e(2 * mb, fn.critic_obs_width) if critic_too else None
            self._sym_actions = e(2 * mb, self.num_actions)
            self._sym_scalars = e(4, 2 * mb)   # old_log_prob, advantages, values, returns
            self._sym_grad = e(mb, self.num_actions)
            self._sym_out = torch.zeros(1, device=dev, dtype=torch.float32)
            self._sym_ws = torch.empty(max(1, nat.mirror_loss_workspace_bytes(mb) // 8), device=dev, dtype=torch.float64)
            self._sym_key = key
        return self._sym_obs, self._sym_critic, self._sym_actions, self._sym_scalars

    @staticmethod
    def _mirror_field(f, src, dst, mb: int, tables, norm, copy: bool = True) -> None:
        """Field ``f`` of a GfMirrorRowsArgs: ``src`` ``[mb, W]`` into the two halves of ``dst`` ``[2·mb, W]`` (``copy=False``: the
        mirrored half only, into ``dst`` ``[mb, W]``)."""
        w = int(src.shape[1])
        f.src, f.width, f.row_stride = src.data_ptr(), w, 0 if src.is_contiguous() else src.stride(0)
        f.dst_copy = dst.data_ptr() if copy else None
        f.dst_mirror = dst.data_ptr() + (mb * w * 4 if copy else 0)
        f.perm, f.sign = tables[0].data_ptr(), tables[1].data_ptr()
        if norm is None:
            f.in_mean = f.in_std = None
            f.in_eps = 0.0
        else:
            f.in_mean, f.in_std, f.in_eps = norm._mean.data_ptr(), norm._std.data_ptr(), norm.eps

    def _mirror_loss_hip(self, backend, mu_mirror, mu_orig, grad) -> None:
        a, fn = self._mir_loss_args, self.symmetry["func"]
        perm, sign = fn.tables("actions", mu_mirror.device)
        a.num_rows, a.num_actions, a.coeff = int(mu_mirror.shape[0]), self.num_actions, self.symmetry["coeff"]
        a.mu_mirror, a.mu_orig, a.perm, a.sign = mu_mirror.data_ptr(), mu_orig.data_ptr(), perm.data_ptr(), sign.data_ptr()
        a.grad = None if grad is None else grad.data_ptr()
        a.out, a.sums = self._sym_out.data_ptr(), self._sums.data_ptr() + 3 * 8
        a.workspace, a.workspace_bytes = self._sym_ws.data_ptr(), self._sym_ws.numel() * 8
        backend.mirror_loss(a)

    def _symmetry_hip(self, backend, b: MiniBatch, norms) -> None:
        sym, policy = self.symmetry, self.policy
        fn, mb, A, dev = sym["func"], int(b.actions.shape[0]), self.num_actions, self.params.device
        actor = policy.act_mean if norms[0] is None else policy.actor        # (a normaliser is applied by gf_mirror_rows)
        a = self._mir_args
        a.num_rows = mb
        if sym["augment"]:
            critic = policy.evaluate if norms[1] is None else policy.critic
            # the critic reads the actor's rows when the two inputs, their tables and their normalisers are the same
            shared = b.critic_obs is b.obs and norms[1] is norms[0] and fn._host["critic"] is fn._host["policy"]
            obs2, cobs2, act2, scal2 = self._symmetry_buffers(mb, not shared)
            self._mirror_field(a.fields[0], b.obs, obs2, mb, fn.tables("policy", dev), norms[0])
            self._mirror_field(a.fields[1], b.actions, act2, mb, fn.tables("actions", dev), None)
            a.num_fields = 2
            if not shared:
                self._mirror_field(a.fields[2], b.critic_obs, cobs2, mb, fn.tables("critic", dev), norms[1])
                a.num_fields = 3
            for sc, src, dst in zip(a.scalars, (b.old_log_prob, b.advantages, b.values, b.returns), scal2):
                sc.src, sc.dst = src.data_ptr(), dst.data_ptr()
            a.num_scalars = 4
            backend.mirror_rows(a)
            mu, value = actor(obs2), critic(obs2 if shared else cobs2)
            b2 = b._replace(obs=obs2, critic_obs=obs2 if shared else cobs2, actions=act2, old_log_prob=scal2[0], advantages=scal2[1],
                            values=scal2[2], returns=scal2[3])
            gmu, gval = self._loss_hip(backend, mu, value, b2, kl_rows=mb)
            # the mirrored half of that forward against the mirror of the original half; its gradient joins the mirrored half's
            self._mirror_loss_hip(backend, mu[mb:], mu[:mb], gmu[mb:] if sym["mirror"] else None)
            torch.autograd.backward((mu, value), (gmu, gval.view_as(value)))
            return
        critic = policy.evaluate if norms[1] is None else policy.critic   # (the critic's rows came normalised from the gather)
        obs2 = self._symmetry_buffers(mb, False)[0]
        # the originals go through the normaliser here too (the gather left them raw); without one the batch's own rows are the input
        self._mirror_field(a.fields[0], b.obs, obs2, mb, fn.tables("policy", dev), norms[0])
        if norms[0] is None:
            a.fields[0].dst_copy = None
        a.num_fields, a.num_scalars = 1, 0
        backend.mirror_rows(a)
        mu = actor(b.obs if norms[0] is None else obs2[:mb])
        value = critic(b.critic_obs)
        gmu, gval = self._loss_hip(backend, mu, value, b)
        if sym["mirror"]:   # one extra actor forward on the mirrored rows; its output's gradient starts from zero
            mu_m = actor(obs2[mb:])
            gm = self._sym_grad.zero_()
            self._mirror_loss_hip(backend, mu_m, mu, gm)
            torch.autograd.backward((mu, value, mu_m), (gmu, gval.view_as(value), gm))
        else:               # logging only
            with torch.no_grad():
                mu_m = actor(obs2[mb:])
            self._mirror_loss_hip(backend, mu_m, mu, None)
            torch.autograd.backward((mu, value), (gmu, gval.view_as(value)))

    def _reduce_kl(self) -> None:
        """rsl_rl: with several ranks, ``all_reduce(kl_mean, SUM)`` then ``kl_mean /= world_size`` (every rank then takes the same lr)."""
        sync = self.grad_sync
        if not self.adaptive or (sync.world == 1 and not sync.force):
            return
        import torch.distributed as dist

        kl = self._out[3:4]
        dist.all_reduce(kl, op=dist.ReduceOp.SUM, group=sync.group)
        kl.div_(sync.world)

    def _buffers(self, mb: int):
        key = (mb, self.num_actions)
        if self._mb_key != key:
            dev, A = self.params.device, self.num_actions
            self._grad_mu = torch.empty((mb, A), device=dev, dtype=torch.float32)
            self._grad_value = torch.empty((mb, 1), device=dev, dtype=torch.float32)
            self._loss_ws = torch.empty(max(1, nat.ppo_loss_workspace_bytes(mb, A) // 8), device=dev, dtype=torch.float64)
            self._mb_key = key
        return self._grad_mu, self._grad_value

    def _loss_hip(self, backend, mu, value, b: MiniBatch, kl_rows: int = 0):
        """``kl_rows``: the KL covers the first ``kl_rows`` rows (``b.old_mu`` / ``b.old_sigma`` hold that many); 0: all of them."""
        mb, A = int(b.actions.shape[0]), self.num_actions
        std, is_log = _policy_std(self.policy)   # (std, or log_std: the kernel exponentiates and applies exp's backward)
        for name, t, shape in (("mu", mu, (mb, A)), ("value", value, (mb, 1))):
            if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"PPO: the policy's {name} must be a contiguous float32 {shape} tensor, not {tuple(t.shape)} {t.dtype}")
        gmu, gval = self._buffers(mb)
        a = self._loss_args
        a.num_rows, a.num_actions, a.use_clipped_value_loss = mb, A, 1 if self.use_clipped_value_loss else 0
        a.mu, a.sigma, a.value = mu.data_ptr(), std.data_ptr(), value.data_ptr()
        a.actions, a.old_log_prob, a.advantages = b.actions.data_ptr(), b.old_log_prob.data_ptr(), b.advantages.data_ptr()
        a.target_values, a.returns, a.old_mu, a.old_sigma = b.values.data_ptr(), b.returns.data_ptr(), b.old_mu.data_ptr(), b.old_sigma.data_ptr()
        a.clip_param, a.value_loss_coef, a.entropy_coef = self.clip_param, self.value_loss_coef, self.entropy_coef
        a.sigma_is_log = 1 if is_log else 0
        # d loss / d std (d loss / d log_std) goes straight into its slot of the (just zeroed) bucket: nothing in the graph of mu / value reaches std
        a.grad_mu, a.grad_value, a.grad_sigma = gmu.data_ptr(), gval.data_ptr(), std.grad.data_ptr()
        a.out, a.sums = self._out.data_ptr(), self._sums.data_ptr()
        a.workspace, a.workspace_bytes = self._loss_ws.data_ptr(), self._loss_ws.numel() * 8
        a.kl_rows = int(kl_rows)
        self._keep = (mu, value, b)
        backend.ppo_loss(a)
        return gmu, gval

    # -- the same arithmetic in torch (backends without gf_ppo_loss / gf_adam_step) -------------------------------------------------
    def _loss_torch(self, mu, value, b: MiniBatch, kl_rows: int = 0, extra=None) -> None:
        """rsl_rl PPO.update's loss lines, ``loss.backward()``, and the values gf_ppo_loss leaves in ``out`` / ``sums``.  ``kl_rows``:
        the KL is taken from the first ``kl_rows`` rows (0: all); ``extra``: a term added to the loss before ``backward()``."""
        std, is_log = _policy_std(self.policy)
        sigma = (torch.exp(std) if is_log else std).expand_as(mu)
        dist = torch.distributions.Normal(mu, sigma, validate_args=False)   # (rsl_rl's ActorCritic turns validation off: no host read)
        logp = dist.log_prob(b.actions).sum(dim=-1)
        entropy = dist.entropy().sum(dim=-1)
        with torch.no_grad():
            mu_kl, sigma_kl = (mu[:kl_rows], sigma[:kl_rows]) if kl_rows else (mu, sigma)
            kl = torch.sum(torch.log(sigma_kl / b.old_sigma + 1.0e-5) + (torch.square(b.old_sigma) + torch.square(b.old_mu - mu_kl))
                           / (2.0 * torch.square(sigma_kl)) - 0.5, dim=-1)
            kl_mean = torch.mean(kl)
        ratio = torch.exp(logp - torch.squeeze(b.old_log_prob))
        surrogate = -torch.squeeze(b.advantages) * ratio
        surrogate_clipped = -torch.squeeze(b.advantages) * torch.clamp(ratio, 1.0 - self.clip_param, 1.0 + self.clip_param)
        surrogate_loss = torch.max(surrogate, surrogate_clipped).mean()
        v, tv, ret = value.reshape(-1), b.values, b.returns
        if self.use_clipped_value_loss:
            value_clipped = tv + (v - tv).clamp(-self.clip_param, self.clip_param)
            value_loss = torch.max((v - ret).pow(2), (value_clipped - ret).pow(2)).mean()
        else:
            value_loss = (ret - v).pow(2).mean()
        ent_mean = entropy.mean()
        loss = surrogate_loss + self.value_loss_coef * value_loss - self.entropy_coef * ent_mean
        if extra is not None:
            loss = loss + extra
        loss.backward()
        with torch.no_grad():
            self._out.copy_(torch.stack([surrogate_loss, value_loss, ent_mean, kl_mean, loss]).to(torch.float32))
            self._sums[:3].add_(torch.stack([value_loss, surrogate_loss, ent_mean]).to(torch.float64))


# ---- teacher–student distillation: rsl_rl Distillation.update -----------------------------------------------------------------------
_DISTILL_KEYS = ("num_learning_epochs", "gradient_length", "learning_rate", "max_grad_norm", "loss_type")
_DISTILL_DEFAULTS = dict(num_learning_epochs=1, gradient_length=15, learning_rate=1e-3, max_grad_norm=None, loss_type="mse")
_BC_LOSS_TYPES = {"mse": nat.GF_BC_LOSS_MSE, "huber": nat.GF_BC_LOSS_HUBER}


class Distillation(_FlatAdam):
    """rsl_rl's ``Distillation`` (feed-forward student, one rank) over a :class:`RolloutStorage` collected with ``act_distill`` and a
    :class:`StudentTeacherMLP`: the student is regressed onto the teacher's stored actions.

    ``Distillation(policy, storage, **train_cfg["algorithm"])``: ``num_learning_epochs``, ``gradient_length``, ``learning_rate``,
    ``max_grad_norm`` (``None``: no clipping) and ``loss_type`` (``"mse"`` or ``"huber"``); ``class_name`` is ignored, unknown keys
    and bad values raise ``ValueError``.  At construction the STUDENT's parameters move into one flat buffer with flat Adam moments
    and the device control block, as :class:`PPO` does it; ``std`` and the teacher stay where they are and are never stepped.

    ``update()`` walks ``storage.step_batches()`` in time order, ``num_learning_epochs`` times: per step the student's forward and
    backward stay in torch, the loss and its gradient w.r.t. the student's mean are one ``gf_bc_loss`` (two launches) whose gradient
    is back-propagated into the bucket; every ``gradient_length`` steps — the counter runs on across the epochs of one update — one
    ``gf_adam_step`` (fixed schedule; ``max_grad_norm=None`` is passed as the largest finite float, a clip coefficient of exactly 1)
    applies the accumulated gradient and the bucket is zeroed.  Gradients still pending when the update ends are dropped — rsl_rl's
    behaviour: the loss accumulated since the last optimizer step is discarded — so the steps behind the update's last optimizer step
    run their forward without a graph and ``gf_bc_loss`` in its loss-only mode: they are logged, nothing is back-propagated.  No host synchronisation per step (rsl_rl reads
    ``behavior_loss.item()`` each time); the returned mean is the one read of the update.  On a backend without the entry points
    (the test-only CPU oracle) the same arithmetic runs in torch.

    ``optimizer_state_dict()`` is ``torch.optim.Adam``'s format over the student's parameters.  It is NOT interchangeable with
    rsl_rl's distillation checkpoints, whose Adam was built over every parameter of the policy (the teacher's and ``std`` take index
    slots there); only the model state interchanges.

    A recurrent student (``policy.is_recurrent``: :class:`StudentTeacherRecurrent`, collected with ``act_distill_recurrent``) is
    trained by truncated back-propagation through time.  The trained parameters are ``policy.student``'s and ``policy.memory_s``'s,
    both in the flat buffer.  Per epoch the student's state is set to ``storage.rnn_start["student"]``, detached — rsl_rl's
    ``last_hidden_states``: the state update k leaves behind is the one collection k + 1 starts from.  Per stored step, in time
    order, ``policy.act_mean(obs_t)`` advances ``memory_s`` with a graph and ``gf_bc_loss`` writes the loss and its gradient w.r.t.
    that step's mean into row ``cnt % gradient_length`` of a ``[gradient_length, N, A]`` buffer; every ``gradient_length`` steps ONE
    ``torch.autograd.backward`` over the window's means and gradient rows back-propagates through time inside the window only, then
    ``gf_adam_step``, the bucket is zeroed and the state detached; then the rows with ``dones[t]`` set restart from zeros (no
    gradient crosses a done).  The pending tail runs under ``no_grad``, loss-only, and still advances the state.  After the last
    epoch ``memory_s`` holds the replay's end state — the last ``dones`` applied, detached, contiguous — which the next collection
    step advances in place.  Still one host read per update.  A ``history="frames"`` storage, or one without
    ``rnn_start["student"]``, raises ``ValueError``.  Two deliberate deviations from rsl_rl: ``update()`` never touches the teacher's
    memory, which keeps what the collection left (rsl_rl's per-epoch ``reset(hidden_states=…)`` rewinds it to the state before the
    previous update); and ``max_grad_norm`` clips the norm over ALL trained parameters, ``memory_s``'s included, because
    ``gf_adam_step`` takes one norm per bucket (rsl_rl clips ``student.parameters()`` only)."""

    def __init__(self, policy: "StudentTeacherMLP", storage: RolloutStorage, **algorithm):
        algorithm = dict(algorithm)
        algorithm.pop("class_name", None)
        bad = sorted(k for k in algorithm if k not in _DISTILL_KEYS)
        if bad:
            raise ValueError(f"Distillation: unsupported algorithm keys {bad}")
        cfg = dict(_DISTILL_DEFAULTS, **algorithm)
        if cfg["loss_type"] not in _BC_LOSS_TYPES:
            raise ValueError(f"Distillation: loss_type={cfg['loss_type']!r} is not supported ('mse' or 'huber')")
        if int(cfg["gradient_length"]) < 1 or int(cfg["num_learning_epochs"]) < 1:
            raise ValueError("Distillation: gradient_length and num_learning_epochs must be >= 1")
        if cfg["max_grad_norm"] is not None and not float(cfg["max_grad_norm"]) > 0.0:
            raise ValueError(f"Distillation: max_grad_norm={cfg['max_grad_norm']!r} must be > 0 (or None)")
        if not isinstance(getattr(policy, "student", None), torch.nn.Module) or not isinstance(getattr(policy, "teacher", None), torch.nn.Module):
            raise ValueError("Distillation needs a policy with a student, a teacher, act_mean() and evaluate() (StudentTeacherMLP)")
        self.policy, self.storage = policy, storage
        self.num_learning_epochs, self.gradient_length = int(cfg["num_learning_epochs"]), int(cfg["gradient_length"])
        self.loss_type = cfg["loss_type"]
        # None: the largest finite float — the norm of a finite gradient never exceeds it, so the clip coefficient is exactly 1
        self.max_grad_norm = torch.finfo(torch.float32).max if cfg["max_grad_norm"] is None else float(cfg["max_grad_norm"])
        self.schedule, self.adaptive, self.desired_kl = "fixed", False, None
        self.num_actions = int(policy.student[-1].weight.shape[0])
        self.recurrent = bool(getattr(policy, "is_recurrent", False))
        if self.recurrent and not isinstance(getattr(getattr(policy, "memory_s", None), "rnn", None), (torch.nn.LSTM, torch.nn.GRU)):
            raise ValueError("Distillation: a recurrent policy needs memory_s.rnn, an nn.LSTM or nn.GRU (StudentTeacherRecurrent)")
        trained = list(policy.student.parameters()) + (list(policy.memory_s.parameters()) if self.recurrent else [])
        self.grad_sync = GradientAllReduce(trained)   # (one rank: a bucket, never a collective)
        self._init_flat(float(cfg["learning_rate"]))
        dev = self.params.device
        self._out = torch.zeros(1, device=dev, dtype=torch.float32)
        self._sums = torch.zeros(1, device=dev, dtype=torch.float64)
        self._loss_args = nat.GfBcLossArgs()
        self._grad = self._loss_ws = self._grad_window = None

    def _bc_hip(self, backend, mu: torch.Tensor, target: torch.Tensor, want_grad: bool = True, grad: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``gf_bc_loss`` of one step; the gradient goes to ``grad`` (a contiguous ``[n, A]`` row of the caller's) or the module's own."""
        n, A = int(target.shape[0]), self.num_actions
        if tuple(mu.shape) != (n, A) or mu.dtype != torch.float32 or not mu.is_contiguous():
            raise ValueError(f"Distillation: the student's mean must be a contiguous float32 {(n, A)} tensor, not {tuple(mu.shape)} {mu.dtype}")
        if self._grad is None or tuple(self._grad.shape) != (n, A):
            self._grad = torch.empty((n, A), device=mu.device, dtype=torch.float32)
            self._loss_ws = torch.empty(max(1, nat.bc_loss_workspace_bytes(n) // 8), device=mu.device, dtype=torch.float64)
        grad = self._grad if grad is None else grad
        a = self._loss_args
        a.num_rows, a.num_actions, a.loss_type = n, A, _BC_LOSS_TYPES[self.loss_type]
        a.mu, a.target, a.grad = mu.data_ptr(), target.data_ptr(), grad.data_ptr() if want_grad else None
        a.out, a.sums = self._out.data_ptr(), self._sums.data_ptr()
        a.workspace, a.workspace_bytes = self._loss_ws.data_ptr(), self._loss_ws.numel() * 8
        self._keep = (mu, target)
        backend.bc_loss(a)
        return grad

    def _bc_torch(self, mu: torch.Tensor, target: torch.Tensor, backward: bool = True) -> torch.Tensor:
        """rsl_rl's ``loss_fn(actions, privileged_actions)`` and its ``backward()``, which accumulates into the bucket; returns the loss."""
        fn = torch.nn.functional.mse_loss if self.loss_type == "mse" else torch.nn.functional.huber_loss
        loss = fn(mu, target)
        if backward:
            loss.backward()
        with torch.no_grad():
            self._out[0] = loss.detach()
            self._sums[0] += loss.detach().to(torch.float64)
        return loss

    def update(self) -> Dict[str, float]:
        """One distillation update over the stored rollout; returns ``{"behavior": mean loss per step}`` — its one host read."""
        if self.recurrent:
            return self._update_recurrent()
        sync, policy, backend = self.grad_sync, self.policy, self.storage.env.backend
        hip = getattr(backend, "bc_loss", None) is not None   # (else the test-only oracle backend: torch's loss, autograd, torch Adam)
        self._sums.zero_()
        sync.zero_grad()
        total = self.num_learning_epochs * self.storage.num_steps
        stepped = total - total % self.gradient_length   # the steps past it never reach an optimizer step: their loss is logged only
        cnt = 0
        for _epoch in range(self.num_learning_epochs):
            for obs, target in self.storage.step_batches():
                if cnt >= stepped:   # no graph, no gradient, no backward
                    with torch.no_grad():
                        mu = policy.act_mean(obs)
                        if hip:
                            self._bc_hip(backend, mu, target, want_grad=False)
                        else:
                            self._bc_torch(mu, target, backward=False)
                    cnt += 1
                    continue
                mu = policy.act_mean(obs)
                if hip:
                    torch.autograd.backward(mu, self._bc_hip(backend, mu, target))
                else:
                    self._bc_torch(mu, target)
                cnt += 1
                if cnt % self.gradient_length == 0:
                    self._adam_step(backend)
                    sync.zero_grad()
        return {"behavior": self._sums.tolist()[0] / cnt}

    def _update_recurrent(self) -> Dict[str, float]:
        """``update()`` for a recurrent student: truncated back-propagation through time, one backward per window (the class docstring)."""
        sync, policy, store, backend = self.grad_sync, self.policy, self.storage, self.storage.env.backend
        if store.history == "frames":
            raise ValueError('Distillation: a recurrent student over a history="frames" storage is not supported')
        start = (getattr(store, "rnn_start", None) or {}).get("student")
        if start is None:
            raise ValueError('Distillation: the storage has no rnn_start["student"] — collect the rollout with act_distill_recurrent() '
                             "(or call keep_distill_rnn_start(policy) before its first step)")
        hip = getattr(backend, "bc_loss", None) is not None   # (else the test-only oracle backend: torch's loss, autograd, torch Adam)
        memory, L, lstm = policy.memory_s, self.gradient_length, isinstance(policy.memory_s.rnn, torch.nn.LSTM)
        if hip:
            shape = (L, store.env.num_envs, self.num_actions)
            if self._grad_window is None or tuple(self._grad_window.shape) != shape:
                self._grad_window = torch.empty(shape, device=self.params.device, dtype=torch.float32)
        self._sums.zero_()
        sync.zero_grad()
        total = self.num_learning_epochs * store.num_steps
        stepped = total - total % L   # the steps past it never reach an optimizer step: their loss is logged only
        cnt, window, loss = 0, [], None

        def states(fn) -> None:
            hs = memory.hidden_states
            memory.hidden_states = tuple(fn(x) for x in hs) if isinstance(hs, tuple) else fn(hs)

        for _epoch in range(self.num_learning_epochs):
            h0 = tuple(x.detach().unsqueeze(0) for x in start if x is not None)
            memory.hidden_states = h0 if lstm else h0[0]
            for obs, target, dones in store.step_batches(with_dones=True):
                if cnt >= stepped:   # no graph, no gradient, no backward: the state still advances
                    with torch.no_grad():
                        mu = policy.act_mean(obs)
                        if hip:
                            self._bc_hip(backend, mu, target, want_grad=False)
                        else:
                            self._bc_torch(mu, target, backward=False)
                else:
                    mu = policy.act_mean(obs)
                    if hip:
                        self._bc_hip(backend, mu, target, grad=self._grad_window[cnt % L])
                        window.append(mu)
                    else:
                        step_loss = self._bc_torch(mu, target, backward=False)
                        loss = step_loss if loss is None else loss + step_loss
                cnt += 1
                if cnt <= stepped and cnt % L == 0:
                    if hip:
                        torch.autograd.backward(window, list(self._grad_window.unbind(0)))
                    else:
                        loss.backward()
                    self._adam_step(backend)
                    sync.zero_grad()
                    states(lambda x: x.detach())
                    window, loss = [], None
                keep = dones.reshape(1, -1, 1)
                states(lambda x: torch.where(keep, 0.0, x))   # a done row restarts from zeros: no gradient crosses it
        states(lambda x: x.detach().contiguous())
        return {"behavior": self._sums.tolist()[0] / cnt}
