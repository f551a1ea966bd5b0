"""
ActuatorDelay — a randomised actuator latency, as Isaac Lab's ``DelayedPDActuator`` (a per-env ``DelayBuffer``) and the "action lag"
buffer of the legged_gym forks have it: the position targets a policy commands reach the motors a few control steps late, and the
lag differs per robot and per episode.  The reference accepts ``delay_step`` and never primes its FIFO (quirk q3), so it has no
counterpart that does anything.

Composed from torch the delay is a chain of small launches on ``[N, D]`` data every step — write a ring slot, gather by a per-env
index, a ``where`` for the fresh episodes, a draw and a scatter for their new lags.  ``step()`` is ONE ``gf_action_delay`` launch
(``csrc/gf_action_delay.hip``; the sequence is written out in ``include/gf_step.h``): this step's targets go into slot ``head`` of a
ring of ``max_lag + 1`` steps, every env gets the targets of ``lag[n]`` steps ago, and an env whose episode has just begun
(``episode_length <= 1``, a mask, or everything after ``reset()``) draws a new lag from ``lag_steps`` and has every slot of its ring
set to its current targets — Isaac Lab's rule: a cleared buffer is filled with the first value pushed.  No index list, no host read.
A backend without the entry (the test-only CPU oracle) runs the same sequence as separate tensor ops.

The draws are Philox blocks of the env's seed under a key of their own (``GF_ACTION_DELAY_SEED_TAG``) and the delay's own call
counter: ``step()`` does not take a stream id from the env, so every other draw of the env is what it is without the delay.

The delay is not a manager: it registers nothing with the env.  ``DelayedPositionActionManager`` (managers/action.py) puts it
between the processed targets and the actuators; ``INTEGRATION.md`` has the three lines for any other action manager.
"""
from __future__ import annotations

import operator
from typing import Optional

import torch

from .. import _native as nat
from .. import gs
from .terrain_curriculum import _f32, _philox_block, _unit

_M32 = 0xFFFFFFFF
MAX_LAG = nat.GF_ACTION_DELAY_MAX_SLOTS - 1


def _lag_pair(lag_steps) -> tuple:
    """``(lo, hi)`` as two plain ints, or ValueError: whole numbers, 0 <= lo <= hi."""
    try:
        lo, hi = lag_steps
    except (TypeError, ValueError):
        raise ValueError(f"lag_steps must be a (lo, hi) pair of control steps, got {lag_steps!r}") from None
    out = []
    for v in (lo, hi):
        if isinstance(v, bool):
            raise ValueError(f"lag_steps must be whole numbers of control steps, got {lag_steps!r}")
        try:
            out.append(operator.index(v))
        except TypeError:
            raise ValueError(f"lag_steps must be whole numbers of control steps, got {lag_steps!r}") from None
    lo, hi = out
    if lo < 0 or hi < 0:
        raise ValueError(f"lag_steps must not be negative, got {(lo, hi)}")
    if lo > hi:
        raise ValueError(f"lag_steps needs lo <= hi, got {(lo, hi)}")
    return lo, hi


def check_lags(lag_steps, max_lag) -> tuple:
    """``(lo, hi, max_lag)`` of the constructor arguments, or ValueError.  ``max_lag`` None: ``hi``."""
    lo, hi = _lag_pair(lag_steps)
    if max_lag is None:
        max_lag = hi
    if isinstance(max_lag, bool):
        raise ValueError(f"max_lag must be a whole number of control steps, got {max_lag!r}")
    try:
        max_lag = operator.index(max_lag)
    except TypeError:
        raise ValueError(f"max_lag must be a whole number of control steps, got {max_lag!r}") from None
    if max_lag > MAX_LAG:
        raise ValueError(f"max_lag must be at most {MAX_LAG} steps, got {max_lag}")
    if hi > max_lag:
        raise ValueError(f"lag_steps {(lo, hi)} exceeds max_lag {max_lag}")
    return lo, hi, max_lag


class ActuatorDelay:
    """Delays ``[N, num_dofs]`` float32 targets by a per-env number of control steps.

    ``lag_steps`` ``(lo, hi)``: the lag of an episode is uniform over the whole numbers lo … hi.  ``max_lag`` (default ``hi``) is what
    the ring is allocated for — ``max_lag + 1`` slots, at most 64 —, so that ``set_lag_range`` can widen the range later (a latency
    curriculum).  ``use_kernel = False`` runs the torch composition even on a backend that has the entry
    (tools/bench_action_delay.py times both)."""

    def __init__(self, env, num_dofs: int, lag_steps=(0, 2), max_lag: Optional[int] = None):
        lo, hi, max_lag = check_lags(lag_steps, max_lag)
        if isinstance(num_dofs, bool) or not isinstance(num_dofs, int) or num_dofs <= 0:
            raise ValueError(f"num_dofs must be a positive int, got {num_dofs!r}")
        self.env, self.num_dofs, self.max_lag = env, num_dofs, max_lag
        self.lag_lo, self.lag_hi = lo, hi
        self.slots = max_lag + 1
        self.ring: Optional[torch.Tensor] = None
        self.out: Optional[torch.Tensor] = None
        self._lag: Optional[torch.Tensor] = None
        self._args = nat.GfActionDelayArgs()
        self._keep: Optional[tuple] = None   # the tensors the descriptor points at
        self._step = 0                       # the delay's own call counter (uint32, wrapping): the first step() is call 1
        self._head = self.slots - 1          # the slot the last call wrote: the first step() writes slot 0
        self._prime = True                   # the next call primes every env
        self._built = False
        #: False: run the torch composition even on a backend that has the entry
        self.use_kernel = True

    # -- build ---------------------------------------------------------------------------------------------------------------
    def build(self) -> None:
        """Allocates the ring, the lags and the output.  Runs once."""
        if self._built:
            return
        N, D, L, dev = self.env.num_envs, self.num_dofs, self.slots, gs.device
        self.ring = torch.zeros(L, N, D, device=dev, dtype=torch.float32)
        self.out = torch.zeros(N, D, device=dev, dtype=torch.float32)
        self._lag = torch.zeros(N, device=dev, dtype=torch.int32)
        a = self._args
        a.num_envs, a.num_dofs, a.slots = N, D, L
        a.out, a.ring, a.lag = self.out.data_ptr(), self.ring.data_ptr(), self._lag.data_ptr()
        self._built = True

    # -- queries and settings ------------------------------------------------------------------------------------------------------
    @property
    def lag(self) -> torch.Tensor:
        """int32 ``[N]``: the lag of every env's current episode in control steps (the launch's own state, no copy) — a privileged
        input of a critic."""
        self.build()
        return self._lag

    def lag_seconds(self) -> torch.Tensor:
        """float32 ``[N]``: ``lag * env.dt``."""
        return self.lag.to(torch.float32) * float(self.env.dt)

    def set_lag_range(self, lo: int, hi: int) -> None:
        """A new ``(lo, hi)`` within the allocated ``max_lag``: every env takes it at its next re-draw (a latency curriculum)."""
        lo, hi = _lag_pair((lo, hi))
        if hi > self.max_lag:
            raise ValueError(f"lag range {(lo, hi)} exceeds the allocated max_lag {self.max_lag}")
        self.lag_lo, self.lag_hi = lo, hi

    def reset(self) -> None:
        """The next ``step()`` treats every env as fresh: new lags, every ring primed with that step's targets."""
        self._prime = True

    # -- the launch ------------------------------------------------------------------------------------------------------------
    def step(self, targets: torch.Tensor, mask: Optional[torch.Tensor] = None, mask2: Optional[torch.Tensor] = None,
             draws: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One ``gf_action_delay`` launch: ``targets`` (float32 ``[N, num_dofs]``) in, the delayed targets out (``self.out``, the same
        tensor every step).  ``mask`` / ``mask2`` (bool ``[N]``) mark envs that are fresh besides those with ``env.episode_length <= 1``;
        ``draws`` ``[N]`` replaces Philox (parity mode)."""
        self.build()
        env, a = self.env, self._args
        ep = getattr(env, "episode_length", None)
        new = (targets, mask, mask2, draws, ep)
        if self._keep is None or any(x is not y for x, y in zip(new, self._keep)):
            # a tensor is checked and bound when it is first seen: an action manager hands in the same target buffer every step
            N, D = env.num_envs, self.num_dofs
            for name, t, shape, dt in (("targets", targets, (N, D), torch.float32), ("mask", mask, (N,), torch.bool), ("mask2", mask2, (N,), torch.bool),
                                       ("draws", draws, (N,), torch.float32), ("env.episode_length", ep, (N,), torch.int32)):
                if t is None and name != "targets":
                    continue
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device.type != gs.device.type:
                    raise ValueError(f"{name} must be a contiguous {dt} tensor of shape {shape} on {gs.device}")
            ptr = lambda t: None if t is None else t.data_ptr()
            a.in_, a.mask, a.mask2, a.draws, a.episode_length = ptr(targets), ptr(mask), ptr(mask2), ptr(draws), ptr(ep)
            self._keep = new
        self._step = (self._step + 1) & _M32
        self._head = (self._head + 1) % self.slots
        # what may change between calls
        a.seed, a.step, a.env_offset, a.head = env._rng_seed, self._step, env.env_offset, self._head
        a.lag_lo, a.lag_hi, a.prime_all = self.lag_lo, self.lag_hi, int(self._prime)
        self._prime = False
        launch = getattr(env.backend, "action_delay", None) if self.use_kernel else None
        if launch is None:
            self._step_torch(a, *self._keep)
        else:
            launch(a)
        return self.out

    def _step_torch(self, a, targets, mask, mask2, draws, ep) -> None:
        """The kernel's sequence (include/gf_step.h) as separate tensor ops over every env.  Values move as int32 views: bits."""
        dev, N, L, head = self._lag.device, int(a.num_envs), int(a.slots), int(a.head)
        x, ring = targets.view(torch.int32), self.ring.view(torch.int32)
        # 1: who is fresh
        fresh = torch.full((N,), bool(a.prime_all), device=dev, dtype=torch.bool)
        if ep is not None:
            fresh = fresh | (ep <= 1)
        for m in (mask, mask2):
            if m is not None:
                fresh = fresh | m
        # 2: their new lags
        if draws is not None:
            u = draws
        else:
            key = (int(a.seed) ^ nat.GF_ACTION_DELAY_SEED_TAG) & 0xFFFFFFFFFFFFFFFF
            ids = (torch.arange(N, device=dev, dtype=torch.int64) + int(a.env_offset)) & _M32
            u = _unit(_philox_block(ids, 0, int(a.step), key)[0])
        w = int(a.lag_hi) - int(a.lag_lo) + 1
        r = torch.clamp((u * _f32(float(w), dev)).to(torch.int64), max=w - 1)
        old = self._lag.to(torch.int64)
        # 4: this step's slot, then the slot of lag[n] steps ago (a lag outside 0 … L-1 reads as 0; a fresh env reads its own targets)
        ring[head].copy_(x)
        l = torch.where(fresh | (old < 0) | (old >= L), torch.zeros_like(old), old)
        rows = torch.arange(N, device=dev, dtype=torch.int64)
        self.out.view(torch.int32).copy_(ring[(head + L - l) % L, rows])
        # 3: the fresh envs' rings are their targets in every slot
        ring.copy_(torch.where(fresh.view(1, N, 1), x.unsqueeze(0), ring))
        self._lag.copy_(torch.where(fresh, (int(a.lag_lo) + r).to(torch.int32), self._lag))
