"""
TerrainCurriculum — the game-style terrain curriculum of legged_gym (``_update_terrain_curriculum``) and Isaac Lab
(``terrain_levels_vel``): the terrain is a grid of sub-terrains whose difficulty grows along one axis; every env owns a
``(level, type)`` cell and respawns inside it.  An env that walked further than ``promote_distance`` in an episode moves up a level,
one that fell short of where its command should have taken it moves down, one that clears the top level is sent to a random level.
The reference has no counterpart: its rough-terrain example drops every robot anywhere on one patch.

Composed from torch the bookkeeping is about forty small launches over index lists per reset.  ``respawn()`` is ONE
``gf_terrain_curriculum`` launch (``csrc/gf_terrain_curriculum.hip``; the arithmetic is written out in ``include/gf_step.h``) driven
by the step's done masks: level change, draws, position with the terrain height, orientation, velocities and the bookkeeping for the
flagged envs, no index list and no host read.  A backend without the entry (the test-only CPU oracle) runs the same float32
sequence as separate tensor ops.

Two deviations from legged_gym, both deliberate:

* the distance walked is measured from the env's actual spawn point, not from the cell centre — robots here spawn anywhere in the
  cell's usable area, so the centre says little about where an episode began;
* the demotion threshold is ``|command_xy| * demote_time`` of the command the episode BEGAN with (recorded at the respawn), not the
  one it ended with.  Both are proxies for "where the command should have taken it"; the first one is known when the episode starts
  and does not change under the robot when the command is resampled.

The curriculum is not a manager: it registers nothing with the env.  ``mdp.reset.terrain_curriculum_position`` puts it to use as an
``EntityManager`` ``on_reset`` entry (``INTEGRATION.md``).
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from .. import _native as nat
from .. import gs

SPAWN_BLOCK = 0x100000   # GF_SPAWN_BLOCK of include/gf_step.h


def _f32(v, dev):
    return torch.tensor(v, dtype=torch.float32, device=dev)


def _sqrt(t: torch.Tensor) -> torch.Tensor:
    """Correctly rounded float32 square root, as the kernel's: numpy on the host (torch's CPU sqrt goes through a vector maths
    library that is not correctly rounded on every CPU), torch on a device."""
    if t.device.type == "cpu":
        return torch.from_numpy(np.sqrt(t.contiguous().numpy()))
    return torch.sqrt(t)


def _philox_block(env_ids: torch.Tensor, block: int, stream: int, seed: int) -> tuple:
    """The four words of Philox4x32-10 with counter (env id, block, stream) and key ``seed`` as int64 tensors in [0, 2^32): the
    integer sequence of csrc/gf_device.h, on whatever device ``env_ids`` lives."""
    m32 = 0xFFFFFFFF

    def mulhilo(m: int, c: torch.Tensor):
        ch, cl = c >> 16, c & 0xFFFF            # m * ch and m * cl stay below 2^48
        a, b = ch * m, cl * m
        return ((a + (b >> 16)) >> 16), ((b + ((a & 0xFFFF) << 16)) & m32)

    c0 = env_ids.to(torch.int64) & m32
    c1 = torch.full_like(c0, block & m32)
    c2 = torch.full_like(c0, stream & m32)
    c3 = torch.full_like(c0, (stream >> 32) & m32)
    k0, k1 = seed & m32, (seed >> 32) & m32
    for _ in range(10):
        hi0, lo0 = mulhilo(0xD2511F53, c0)
        hi1, lo1 = mulhilo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + 0x9E3779B9) & m32, (k1 + 0xBB67AE85) & m32
    return c0, c1, c2, c3


def _unit(w: torch.Tensor) -> torch.Tensor:
    return (w >> 8).to(torch.float32) * 5.9604644775390625e-8


def _sincos_det(x: torch.Tensor):
    """sincos_det of csrc/gf_device.h, one float32 tensor op per operation."""
    dev = x.device
    f = lambda v: _f32(v, dev)
    k = torch.round(x * f(0.63661977236758134))
    r = x - k * f(1.5703125)
    r = r - k * f(4.837512969970703125e-4)
    r = r - k * f(7.54978995489188216e-8)
    z = r * r
    ps = ((f(-1.9515295891e-4) * z + f(8.3321608736e-3)) * z - f(1.6666654611e-1)) * z * r + r
    pc = ((f(2.443315711809948e-5) * z - f(1.388731625493765e-3)) * z + f(4.166664568298827e-2)) * z * z - f(0.5) * z + f(1.0)
    q = k.to(torch.int32) & 3
    odd = (q & 1) != 0
    sv, cv = torch.where(odd, pc, ps), torch.where(odd, ps, pc)
    return torch.where((q & 2) != 0, -sv, sv), torch.where(((q + 1) & 2) != 0, -cv, cv)


def _xyz_to_quat_det(ax, ay, az) -> torch.Tensor:
    """xyz_to_quat_det of csrc/gf_device.h → [n, 4] (w, x, y, z)."""
    h = _f32(0.5, ax.device)
    sx, cx = _sincos_det(ax * h)
    sy, cy = _sincos_det(ay * h)
    sz, cz = _sincos_det(az * h)
    return torch.stack([(cx * cy) * cz + (sx * sy) * sz, (sx * cy) * cz - (cx * sy) * sz,
                        (cx * sy) * cz + (sx * cy) * sz, (cx * cy) * sz - (sx * sy) * cz], dim=-1)


def rotation_ranges(rotation: Optional[dict]) -> Optional[list]:
    """``{"z": (lo, hi), …}`` → one ``(lo, hi)`` or None per axis, None for ``rotation=None`` (the quaternion is then left alone).
    Only axes given as tuples are randomised, as in ``mdp.reset.randomize_terrain_position``."""
    if rotation is None:
        return None
    return [rotation.get(axis) if isinstance(rotation.get(axis), tuple) else None for axis in "xyz"]


class TerrainCurriculum:
    """Per-env terrain levels on a ``TerrainManager`` whose terrain is a grid of sub-terrains.

    ``level_axis`` (``"x"`` / ``"y"``) is the grid axis along which difficulty grows; the other axis holds the terrain types.
    ``promote_distance`` (default: half the cell size along the level axis) moves an env up when ``dist > promote_distance``;
    otherwise ``dist < |command_xy at spawn| * demote_time`` (``command_manager`` given; default ``demote_time``: half of
    ``max_episode_length_sec``) or ``dist < demote_distance`` (no command manager) moves it down.  Initial levels are uniform in
    ``[0, max_init_level]`` (default: the top level) from torch's CPU generator at ``build()``; types are ``n * num_types // N`` —
    contiguous blocks of envs per type, as legged_gym has."""

    def __init__(self, env, terrain_manager, command_manager=None, level_axis: str = "x", promote_distance: Optional[float] = None,
                 demote_time: Optional[float] = None, demote_distance: float = 0.0, max_init_level: Optional[int] = None,
                 usable_ratio: float = 0.5):
        if level_axis not in ("x", "y"):
            raise ValueError("level_axis must be 'x' or 'y'")
        for name, v in (("promote_distance", promote_distance), ("demote_time", demote_time), ("demote_distance", demote_distance)):
            if v is not None and not (math.isfinite(float(v)) and float(v) >= 0.0):
                raise ValueError(f"{name} must be finite and not negative, got {v}")
        if not (0.0 < float(usable_ratio) <= 1.0):
            raise ValueError(f"usable_ratio must be in (0, 1], got {usable_ratio}")
        if max_init_level is not None and int(max_init_level) < 0:
            raise ValueError(f"max_init_level must not be negative, got {max_init_level}")
        if command_manager is not None and command_manager._command.shape[1] < 2:
            raise ValueError("the command manager's command needs at least two columns (the commanded x and y velocity)")
        self.env, self.terrain_manager, self.command_manager = env, terrain_manager, command_manager
        self.level_axis = 0 if level_axis == "x" else 1
        self._promote, self._demote_time, self.demote_distance = promote_distance, demote_time, float(demote_distance)
        self._max_init_level = max_init_level
        self.usable_ratio = float(usable_ratio)
        self.levels: Optional[torch.Tensor] = None
        self.types: Optional[torch.Tensor] = None
        self.spawn_xy: Optional[torch.Tensor] = None
        self.speed_ref: Optional[torch.Tensor] = None
        self.counts: Optional[torch.Tensor] = None
        self._args = nat.GfTerrainCurriculumArgs()
        self._keep: tuple = ()
        self._built = False
        #: False: run the torch composition even on a backend that has the entry (tools/bench_terrain_curriculum.py times both)
        self.use_kernel = True

    # -- build ---------------------------------------------------------------------------------------------------------------
    def build(self) -> None:
        """Reads the grid off the (built) terrain manager and allocates the per-env state.  Runs once."""
        if self._built:
            return
        grid = self.terrain_manager.subterrain_grid() if hasattr(self.terrain_manager, "subterrain_grid") else None
        if grid is None:
            raise ValueError("TerrainCurriculum needs a terrain made of sub-terrains (TerrainManager.subterrain_grid() is None)")
        nx, ny, sx, sy = grid
        self.num_levels, self.num_types = (nx, ny) if self.level_axis == 0 else (ny, nx)
        self.cell_size = (sx, sy)
        if self._max_init_level is not None and int(self._max_init_level) > self.num_levels - 1:
            raise ValueError(f"max_init_level must be 0 … {self.num_levels - 1}, got {self._max_init_level}")
        top = self.num_levels - 1 if self._max_init_level is None else int(self._max_init_level)
        self.promote_distance = float(self._promote) if self._promote is not None else 0.5 * (sx if self.level_axis == 0 else sy)
        mel = getattr(self.env, "max_episode_length_sec", None)
        self.demote_time = float(self._demote_time) if self._demote_time is not None else 0.5 * float(mel or 0.0)
        N, dev = self.env.num_envs, gs.device
        self.levels = torch.randint(0, top + 1, (N,), dtype=torch.int32).to(dev)       # (the CPU generator: the same on every device)
        self.types = ((torch.arange(N, dtype=torch.int64) * self.num_types) // max(N, 1)).to(torch.int32).to(dev)
        self.spawn_xy = torch.zeros(N, 2, device=dev, dtype=torch.float32)
        self.speed_ref = torch.zeros(N, device=dev, dtype=torch.float32) if self.command_manager is not None else None
        self.counts = torch.zeros(3, device=dev, dtype=torch.int32)
        self._built = True

    # -- queries ---------------------------------------------------------------------------------------------------------------
    def mean_level(self) -> torch.Tensor:
        """The mean terrain level, a 0-d tensor on the device: one reduction, no host read."""
        return self.levels.to(torch.float32).mean()

    def read_counts(self) -> dict:
        """``{"promoted", "demoted", "wrapped"}`` since ``build()``.  A host read: the caller chooses when to pay for it."""
        p, d, w = self.counts.tolist()
        return {"promoted": p, "demoted": d, "wrapped": w}

    def set_levels(self, levels, envs_idx=None) -> None:
        """Assign levels (an int or one per listed env; ``envs_idx=None``: every env).  The envs move there at their next respawn."""
        self.build()
        t = torch.as_tensor(levels, dtype=torch.int32)
        if t.numel() > 0 and (int(t.min()) < 0 or int(t.max()) > self.num_levels - 1):
            raise ValueError(f"levels must be 0 … {self.num_levels - 1}")
        t = t.to(gs.device)
        if envs_idx is None:
            self.levels.copy_(t.expand(self.env.num_envs) if t.dim() == 0 else t)
        else:
            self.levels[torch.as_tensor(envs_idx, device=gs.device, dtype=torch.long)] = t

    def cell_rect(self, level: int, type_: int) -> tuple:
        """``(x_min, x_max, y_min, y_max)`` of the usable rectangle of the cell of ``(level, type)``."""
        ix, iy = (level, type_) if self.level_axis == 0 else (type_, level)
        return self.terrain_manager.cell_usable_area(ix, iy, self.usable_ratio)

    # -- the launch ------------------------------------------------------------------------------------------------------------
    def respawn(self, mask: torch.Tensor, mask2: Optional[torch.Tensor], pos_in: torch.Tensor, pos_out: torch.Tensor,
                quat_out: Optional[torch.Tensor] = None, quat_stash: Optional[torch.Tensor] = None, lin_vel: Optional[torch.Tensor] = None,
                ang_vel: Optional[torch.Tensor] = None, dof_vel: Optional[torch.Tensor] = None, update: bool = False,
                height_offset: float = 0.1e-3, rotation: Optional[list] = None, zero_velocity: bool = True,
                draws: Optional[torch.Tensor] = None) -> None:
        """Respawns the envs flagged in ``mask`` (or ``mask2``), bool ``[N]``: one ``gf_terrain_curriculum`` launch.  ``pos_in`` /
        ``pos_out`` ``[N, 3]`` may be the same tensor; ``quat_out`` ``[N, 4]`` is written when ``rotation`` (``rotation_ranges``) is
        not None, its old rows copied to ``quat_stash`` first; the velocity tensors are zeroed with ``zero_velocity``.  ``update``
        moves levels first (the in-step reset of finished episodes); without it the envs respawn in the cell they have.  ``draws``
        ``[N, 6]`` replaces Philox (parity mode)."""
        self.build()
        env, N = self.env, self.env.num_envs
        for name, t, shape, dt in (("mask", mask, (N,), torch.bool), ("mask2", mask2, (N,), torch.bool), ("pos_in", pos_in, (N, 3), torch.float32),
                                   ("pos_out", pos_out, (N, 3), torch.float32), ("quat_out", quat_out, (N, 4), torch.float32),
                                   ("quat_stash", quat_stash, (N, 4), torch.float32), ("lin_vel", lin_vel, (N, 3), torch.float32),
                                   ("ang_vel", ang_vel, (N, 3), torch.float32), ("draws", draws, (N, 6), torch.float32)):
            if t is not None and (tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device.type != gs.device.type):
                raise ValueError(f"{name} must be a contiguous {dt} tensor of shape {shape} on {gs.device}")
        if dof_vel is not None and (dof_vel.dim() != 2 or dof_vel.shape[0] != N or dof_vel.dtype != torch.float32 or not dof_vel.is_contiguous()):
            raise ValueError(f"dof_vel must be a contiguous float32 [{N}, D] tensor")
        if rotation is not None and quat_out is None:
            raise ValueError("a rotation needs quat_out")
        x_min, x_max, y_min, y_max = self.terrain_manager.cell_usable_area(0, 0, self.usable_ratio)
        a = self._args
        a.num_envs = N
        a.mask, a.mask2 = mask.data_ptr(), (None if mask2 is None else mask2.data_ptr())
        a.pos_in, a.pos_out = pos_in.data_ptr(), pos_out.data_ptr()
        a.quat_out = None if quat_out is None else quat_out.data_ptr()
        a.quat_stash = None if quat_stash is None or rotation is None else quat_stash.data_ptr()
        a.lin_vel = None if lin_vel is None else lin_vel.data_ptr()
        a.ang_vel = None if ang_vel is None else ang_vel.data_ptr()
        a.dof_vel, a.num_dofs = (None, 0) if dof_vel is None else (dof_vel.data_ptr(), int(dof_vel.shape[1]))
        a.spawn_xy, a.level, a.type = self.spawn_xy.data_ptr(), self.levels.data_ptr(), self.types.data_ptr()
        a.speed_ref = None if self.speed_ref is None else self.speed_ref.data_ptr()
        a.counts = self.counts.data_ptr()
        a.draws = None if draws is None else draws.data_ptr()
        cm = self.command_manager
        if cm is not None:
            a.command.command, a.command.width, a.command.stride = cm._command.data_ptr(), int(cm._command.shape[1]), 0
        else:
            a.command.command, a.command.width, a.command.stride = None, 0, 0
        a.seed, a.stream, a.env_offset = env._rng_seed, env.next_stream(), env.env_offset
        a.num_levels, a.num_types, a.level_axis = self.num_levels, self.num_types, self.level_axis
        a.update, a.set_quat, a.zero_velocity = int(bool(update)), int(rotation is not None), int(bool(zero_velocity))
        a.promote_distance, a.demote_time, a.demote_distance = self.promote_distance, self.demote_time, self.demote_distance
        a.spawn_x_min, a.spawn_x_span = x_min, x_max - x_min     # the double difference, rounded once when stored as f32
        a.spawn_y_min, a.spawn_y_span = y_min, y_max - y_min
        a.cell_dx, a.cell_dy = self.cell_size
        a.height_offset = float(height_offset)
        a.spawn_rot_mask = 0
        for k in range(3):
            a.spawn_rot_lo[k] = a.spawn_rot_hi[k] = 0.0
            if rotation is not None and rotation[k] is not None:
                a.spawn_rot_mask |= 1 << k
                a.spawn_rot_lo[k], a.spawn_rot_hi[k] = float(rotation[k][0]), float(rotation[k][1])
        self.terrain_manager.gf_view(a.terrain)
        self._keep = (mask, mask2, pos_in, pos_out, quat_out, quat_stash, lin_vel, ang_vel, dof_vel, draws)
        launch = getattr(env.backend, "terrain_curriculum", None) if self.use_kernel else None
        if launch is None:
            self._respawn_torch(a, *self._keep)
        else:
            launch(a)

    def _respawn_torch(self, a, mask, mask2, pos_in, pos_out, quat_out, quat_stash, lin_vel, ang_vel, dof_vel, draws) -> None:
        """The kernel's operation sequence (include/gf_step.h) as separate float32 tensor ops over every env — one rounding each —,
        written back under the mask."""
        dev = pos_in.device
        f = lambda v: _f32(float(v), dev)   # (a descriptor's float field read back is already rounded to float32)
        m = mask if mask2 is None else (mask | mask2)
        lev, typ = self.levels, self.types
        l = lev.clone()
        zero = torch.zeros_like(m)
        up = down = wrapped = zero
        if a.update:
            dx, dy = pos_in[:, 0] - self.spawn_xy[:, 0], pos_in[:, 1] - self.spawn_xy[:, 1]
            dist = _sqrt(dx * dx + dy * dy)
            up = dist > f(a.promote_distance)
            thr = self.speed_ref * f(a.demote_time) if self.speed_ref is not None else f(a.demote_distance)
            down = ~up & (dist < thr)
            l = l + up.to(torch.int32) - down.to(torch.int32)
        if draws is not None:
            u = [draws[:, j] for j in range(6)]
        else:
            ids = torch.arange(a.num_envs, device=dev, dtype=torch.int64) + int(a.env_offset)
            r0 = _philox_block(ids, SPAWN_BLOCK, int(a.stream), int(a.seed))
            u = [_unit(r0[0]), _unit(r0[1]), torch.zeros_like(pos_in[:, 0]), torch.zeros_like(pos_in[:, 0]), _unit(r0[2]), _unit(r0[3])]
            if a.spawn_rot_mask & 3:
                r1 = _philox_block(ids, SPAWN_BLOCK + 1, int(a.stream), int(a.seed))
                u[2], u[3] = _unit(r1[0]), _unit(r1[1])
        if a.update:
            wrapped = l >= a.num_levels
            r = torch.clamp((u[5] * f(float(a.num_levels))).to(torch.int32), max=a.num_levels - 1)
            l = torch.where(wrapped, r, l)
            l = torch.clamp(l, min=0)
        ix, iy = (l, typ) if a.level_axis == 0 else (typ, l)
        x = (u[0] * f(a.spawn_x_span) + f(a.spawn_x_min)) + ix.to(torch.float32) * f(a.cell_dx)
        y = (u[1] * f(a.spawn_y_span) + f(a.spawn_y_min)) + iy.to(torch.float32) * f(a.cell_dy)
        z = self.terrain_manager.get_terrain_height(x, y) + f(a.height_offset)
        mc = m.unsqueeze(-1)
        pos_out.copy_(torch.where(mc, torch.stack([x, y, z], dim=-1), pos_out))
        if a.set_quat:
            ang = []
            for k in range(3):
                if a.spawn_rot_mask & (1 << k):
                    ang.append(u[2 + k] * (f(a.spawn_rot_hi[k]) - f(a.spawn_rot_lo[k])) + f(a.spawn_rot_lo[k]))
                else:
                    ang.append(torch.zeros_like(x))
            q = _xyz_to_quat_det(*ang)
            if quat_stash is not None and a.quat_stash:
                quat_stash.copy_(torch.where(mc, quat_out, quat_stash))
            quat_out.copy_(torch.where(mc, q, quat_out))
        if a.zero_velocity:
            for v in (lin_vel, ang_vel, dof_vel):
                if v is not None:
                    v.masked_fill_(mc, 0.0)
        self.spawn_xy.copy_(torch.where(mc, torch.stack([x, y], dim=-1), self.spawn_xy))
        lev.copy_(torch.where(m, l, lev))
        if self.speed_ref is not None and a.command.command:
            c = self.command_manager._command
            cx, cy = c[:, 0], c[:, 1]
            self.speed_ref.copy_(torch.where(m, _sqrt(cx * cx + cy * cy), self.speed_ref))
        self.counts += torch.stack([(up & m).sum(), (down & m).sum(), (wrapped & m).sum()]).to(torch.int32)
