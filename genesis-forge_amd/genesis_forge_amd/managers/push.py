"""
PushDisturbance — the random pushes of legged_gym (``push_robots`` / ``_push_robots``) and Isaac Lab (``push_by_setting_velocity`` as an
``interval`` event): every few seconds the base of a robot gets a random velocity.  The reference has no counterpart.

Composed from torch such an event is a chain of small launches every step — decrement or compare the timers, draw, scale, ``where``,
scatter, redraw — and usually a ``nonzero()`` host read.  ``step()`` is ONE ``gf_push`` launch (``csrc/gf_push.hip``; the arithmetic is
written out in ``include/gf_step.h``): every env owns a timer ``due`` (the step at which it is pushed next), an env that finished its
episode in this step is not pushed and gets a fresh timer (Isaac Lab's per-env interval rule; ``per_env=False``: one timer for all envs,
legged_gym's), and the envs that are due get their kick — no index list, no host read.  A backend without the entry (the test-only
CPU oracle) runs the same float32 sequence as separate tensor ops.

The draws are Philox blocks of the env's seed under a key of their own (``GF_PUSH_SEED_TAG``) and the push's own call counter:
``step()`` does not take a stream id from the env, so every other draw of the env is what it is without the pushes.

The disturbance is not a manager: it registers nothing with the env.  ``Go2RoughTerrainEnv(push={…})`` puts it behind the step
(``INTEGRATION.md`` has the two lines for any other env).
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from .. import _native as nat
from .. import gs
from .terrain_curriculum import _f32, _philox_block, _unit

COMPONENTS = ("x", "y", "z", "roll", "pitch", "yaw")   # bit j of comp_mask; 0..2 linear, 3..5 angular
_M32 = 0xFFFFFFFF


def _interval_steps(u3: float, lo: int, hi: int) -> int:
    """Step 3 of the contract for one draw, on the host: float32 product, truncated, clamped."""
    w = hi - lo + 1
    r = int((torch.tensor(u3, dtype=torch.float32) * torch.tensor(float(w), dtype=torch.float32)).item())
    return lo + min(r, w - 1)


class PushDisturbance:
    """Random velocity kicks of the base of ``entity_manager.entity`` (or ``env.<entity_attr>``).

    ``interval_s`` ``(lo, hi)`` seconds between two pushes of an env, converted to steps with the env's ``dt`` (rounded, at least 1),
    uniform over the whole steps in between.  ``velocity_range``: ``{"x" | "y" | "z" | "roll" | "pitch" | "yaw": (lo, hi)}`` — the keys
    given are the components a push touches, the others are left alone.  ``mode``: ``"set"`` replaces them (legged_gym, Isaac Lab),
    ``"add"`` adds to them.  ``per_env``: every env has its own timer, restarted when its episode ends; ``False``: one timer, every env is
    pushed in the same steps.  ``scale`` multiplies every drawn velocity; it is a plain attribute a training script may change between
    steps (a magnitude curriculum) — the only one: intervals, ranges and mode go into the descriptor once, at ``build()``."""

    def __init__(self, env, entity_manager=None, entity_attr: str = "robot", interval_s=(10.0, 15.0), velocity_range: Optional[dict] = None,
                 mode: str = "set", per_env: bool = True, scale: float = 1.0):
        velocity_range = {"x": (-0.5, 0.5), "y": (-0.5, 0.5)} if velocity_range is None else dict(velocity_range)
        bad = [k for k in velocity_range if k not in COMPONENTS]
        if bad:
            raise ValueError(f"velocity_range keys must be among {COMPONENTS}, got {bad}")
        self.comp_mask, self._lo, self._hi = 0, [0.0] * 6, [0.0] * 6
        for j, k in enumerate(COMPONENTS):
            if k not in velocity_range:
                continue
            try:
                lo, hi = (float(v) for v in velocity_range[k])
            except (TypeError, ValueError):
                raise ValueError(f"velocity_range['{k}'] must be a (lo, hi) pair, got {velocity_range[k]!r}") from None
            if not (math.isfinite(lo) and math.isfinite(hi)):
                raise ValueError(f"velocity_range['{k}'] must be finite, got {(lo, hi)}")
            if lo > hi:
                raise ValueError(f"velocity_range['{k}'] needs lo <= hi, got {(lo, hi)}")
            self.comp_mask |= 1 << j
            self._lo[j], self._hi[j] = lo, hi
        if mode not in ("set", "add"):
            raise ValueError("mode must be 'set' or 'add'")
        try:
            t_lo, t_hi = (float(v) for v in interval_s)
        except (TypeError, ValueError):
            raise ValueError(f"interval_s must be a (lo, hi) pair of seconds, got {interval_s!r}") from None
        if not (math.isfinite(t_lo) and math.isfinite(t_hi) and 0.0 <= t_lo <= t_hi):
            raise ValueError(f"interval_s needs finite 0 <= lo <= hi, got {(t_lo, t_hi)}")
        if not math.isfinite(float(scale)):
            raise ValueError(f"scale must be finite, got {scale}")
        dt = float(env.dt)
        self.interval_lo = max(1, int(round(t_lo / dt)))
        self.interval_hi = max(self.interval_lo, int(round(t_hi / dt)))
        if self.interval_hi - self.interval_lo + 1 > 1 << 24:
            raise ValueError("interval_s spans more than 2^24 steps")
        self.env, self.entity_manager, self._entity_attr = env, entity_manager, entity_attr
        self.mode, self.per_env = (0 if mode == "set" else 1), bool(per_env)
        self.scale = float(scale)
        self.entity = None
        self.due: Optional[torch.Tensor] = None
        self.counts: Optional[torch.Tensor] = None
        self._fired: Optional[torch.Tensor] = None
        self._staging: Optional[tuple] = None
        self._args = nat.GfPushArgs()
        self._keep: Optional[tuple] = None   # the tensors the descriptor points at
        self._step = 0          # the push's own call counter (uint32, wrapping): build() is call 0
        self._built = False
        #: False: run the torch composition even on a backend that has the entry (tools/bench_push.py times both)
        self.use_kernel = True

    # -- build ---------------------------------------------------------------------------------------------------------------
    def build(self) -> None:
        """Finds the entity, allocates the state and starts every timer.  Runs once."""
        if self._built:
            return
        em = self.entity_manager
        ent = getattr(em, "entity", None) if em is not None else None
        if ent is None:
            ent = getattr(self.env, self._entity_attr if em is None else getattr(em, "_entity_attr", self._entity_attr))
        if not hasattr(ent, "gf_masked_base") and not (hasattr(ent, "get_dofs_velocity") and hasattr(ent, "set_dofs_velocity")):
            raise ValueError("PushDisturbance needs an entity with gf_masked_base(), or with get_dofs_velocity() and set_dofs_velocity()")
        self.entity = ent
        N, dev = self.env.num_envs, gs.device
        self.due = torch.zeros(N, device=dev, dtype=torch.int32)
        self._fired = torch.zeros(N, device=dev, dtype=torch.uint8)
        self.counts = torch.zeros(1, device=dev, dtype=torch.int32)
        if not hasattr(ent, "gf_masked_base"):
            self._base_dofs = list(range(6))
            self._staging = (torch.zeros(N, 3, device=dev, dtype=torch.float32), torch.zeros(N, 3, device=dev, dtype=torch.float32))
        # the descriptor's fixed part: the state and everything the constructor settled
        a = self._args
        a.num_envs = N
        a.due, a.fired, a.counts = self.due.data_ptr(), self._fired.data_ptr(), self.counts.data_ptr()
        a.interval_lo, a.interval_hi = self.interval_lo, self.interval_hi
        a.mode, a.comp_mask, a.global_timer = self.mode, self.comp_mask, int(not self.per_env)
        for j in range(6):
            a.lo[j], a.hi[j] = self._lo[j], self._hi[j]
        self._built = True
        self._step = 0
        if self.per_env:
            # one launch under an all-true mask: every env is "done", so nothing fires and every timer is drawn
            lin, ang = self._velocities(fetch=False)
            self._launch(torch.ones(N, device=dev, dtype=torch.bool), None, lin, ang)
        else:
            # the masks are not looked at with one timer for all: the same draw of the same formula, once, on the host
            key = (self.env._rng_seed ^ nat.GF_PUSH_SEED_TAG) & 0xFFFFFFFFFFFFFFFF
            w = _philox_block(torch.tensor([_M32], dtype=torch.int64), 0, 0, key)[3]
            self.due.fill_(_interval_steps(float(_unit(w)[0]), self.interval_lo, self.interval_hi))

    # -- queries ---------------------------------------------------------------------------------------------------------------
    @property
    def fired(self) -> torch.Tensor:
        """bool ``[N]``: the envs the last ``step()`` pushed (a view of the launch's output, no copy)."""
        return self._fired.view(torch.bool)

    def read_counts(self) -> int:
        """Pushes since ``build()``.  A host read: the caller chooses when to pay for it."""
        return int(self.counts.item())

    # -- the launch ------------------------------------------------------------------------------------------------------------
    def _velocities(self, fetch: bool = True):
        ent = self.entity
        if self._staging is None:
            _pos, _quat, lin, ang = ent.gf_masked_base()
            return lin, ang
        lin, ang = self._staging
        if fetch:
            v = ent.get_dofs_velocity(dofs_idx_local=self._base_dofs)
            lin.copy_(v[:, :3])
            ang.copy_(v[:, 3:6])
        return lin, ang

    def step(self, terminated: Optional[torch.Tensor] = None, truncated: Optional[torch.Tensor] = None, draws: Optional[torch.Tensor] = None) -> None:
        """One ``gf_push`` launch with this step's done masks (bool ``[N]``; None: no env finished).  ``draws`` ``[N, 7]`` replaces
        Philox (parity mode).  On an entity without ``gf_masked_base()`` the base velocities of every env go through a staging block:
        fetched, pushed where due, handed back with ``set_dofs_velocity`` for all envs — an unfired row is written back unchanged."""
        self.build()
        self._step = (self._step + 1) & _M32
        lin, ang = self._velocities()
        self._launch(terminated, truncated, lin, ang, draws)
        if self._staging is not None:
            self.entity.set_dofs_velocity(torch.cat([lin, ang], dim=1), dofs_idx_local=self._base_dofs)

    def _launch(self, mask, mask2, lin, ang, draws=None) -> None:
        env, a = self.env, self._args
        new = (mask, mask2, lin, ang, draws)
        if self._keep is None or any(x is not y for x, y in zip(new, self._keep)):
            # a tensor is checked and bound when it is first seen: a recorded step hands out the same mask tensors every step
            N = env.num_envs
            for name, t, shape, dt in (("terminated", mask, (N,), torch.bool), ("truncated", mask2, (N,), torch.bool), ("lin_vel", lin, (N, 3), torch.float32),
                                       ("ang_vel", ang, (N, 3), torch.float32), ("draws", draws, (N, 7), torch.float32)):
                if t is not None and (tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device.type != gs.device.type):
                    raise ValueError(f"{name} must be a contiguous {dt} tensor of shape {shape} on {gs.device}")
            a.mask, a.mask2 = (None if mask is None else mask.data_ptr()), (None if mask2 is None else mask2.data_ptr())
            a.lin_vel, a.ang_vel = lin.data_ptr(), ang.data_ptr()
            a.draws = None if draws is None else draws.data_ptr()
            self._keep = new
        a.seed, a.step, a.env_offset, a.scale = env._rng_seed, self._step, env.env_offset, float(self.scale)     # what may change between calls
        launch = getattr(env.backend, "push", None) if self.use_kernel else None
        if launch is None:
            self._step_torch(a, *self._keep)
        else:
            launch(a)

    def _step_torch(self, a, mask, mask2, lin, ang, draws) -> None:
        """The kernel's operation sequence (include/gf_step.h) as separate tensor ops over every env — one float32 rounding each —,
        written back under the masks."""
        dev, N = self.due.device, int(a.num_envs)
        f = lambda v: _f32(float(v), dev)   # (a descriptor's float field read back is already rounded to float32)
        step = int(a.step)
        done = torch.zeros(N, device=dev, dtype=torch.bool)
        if not a.global_timer:
            for m in (mask, mask2):
                if m is not None:
                    done = done | m
        late = (step - self.due.to(torch.int64)) & _M32          # step - due modulo 2^32: not negative as an int32 below 2^31
        fire = ~done & (late < (1 << 31))
        if draws is not None:
            u = [draws[:, j] for j in range(7)]
        else:
            key = (int(a.seed) ^ nat.GF_PUSH_SEED_TAG) & 0xFFFFFFFFFFFFFFFF
            ids = (torch.arange(N, device=dev, dtype=torch.int64) + int(a.env_offset)) & _M32
            u = [_unit(w) for w in _philox_block(ids, 0, step, key)] + [None] * 3
            if a.global_timer:
                u[3] = _unit(_philox_block(torch.full((N,), _M32, device=dev, dtype=torch.int64), 0, step, key)[3])
            if a.comp_mask & 0x38:
                u[4:7] = [_unit(w) for w in _philox_block(ids, 1, step, key)[:3]]
        w = int(a.interval_hi) - int(a.interval_lo) + 1
        r = torch.clamp((u[3] * f(float(w))).to(torch.int64), max=w - 1)
        nxt = (step + int(a.interval_lo) + r) & _M32
        nxt = torch.where(nxt >= (1 << 31), nxt - (1 << 32), nxt).to(torch.int32)
        self.due.copy_(torch.where(done | fire, nxt, self.due))
        for j in range(6):
            if not (a.comp_mask & (1 << j)):
                continue
            col = (lin if j < 3 else ang)[:, j % 3]
            v = (u[j if j < 3 else j + 1] * (f(a.hi[j]) - f(a.lo[j])) + f(a.lo[j])) * f(a.scale)
            col.copy_(torch.where(fire, col + v if a.mode else v, col))
        self._fired.copy_(fire.to(torch.uint8))
        self.counts += fire.sum().to(torch.int32)
