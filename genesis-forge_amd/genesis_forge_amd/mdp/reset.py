"""
Entity reset functions — same names and arguments as genesis_forge/mdp/reset.py.

``position`` (reset.py:67-124), used by every BASELINE config except rough_terrain, is absorbed into
the fused masked reset when the scene exposes masked setters; called directly it behaves like the
reference (index-list scatter through the entity's setters).  The others call straight into the
entity's setters — there is no per-env math to fuse.
"""
from __future__ import annotations

import math
from typing import Callable, Literal

import torch

from .. import gs
from ..managers.config import ResetMdpFnClass


def zero_all_dofs_velocity(env, entity, envs_idx):
    entity.zero_all_dofs_velocity(envs_idx)


def xyz_to_quat(xyz: torch.Tensor) -> torch.Tensor:
    """Euler xyz (radians, extrinsic x-y-z) → quaternion (w,x,y,z); stands in for genesis.utils.geom.xyz_to_quat."""
    hx, hy, hz = xyz[..., 0] * 0.5, xyz[..., 1] * 0.5, xyz[..., 2] * 0.5
    cx, sx, cy, sy, cz, sz = torch.cos(hx), torch.sin(hx), torch.cos(hy), torch.sin(hy), torch.cos(hz), torch.sin(hz)
    return torch.stack([cx * cy * cz + sx * sy * sz, sx * cy * cz - cx * sy * sz, cx * sy * cz + sx * cy * sz,
                        cx * cy * sz - sx * sy * cz], dim=-1)


def set_rotation(env, entity, envs_idx, x=0, y=0, z=0):
    """Randomised euler rotation (reset.py:33-64).  As in the reference's code, only axes given as ``(lo, hi)`` tuples are
    written — a scalar angle is accepted and ignored (the angle buffer stays 0 for that axis, :52-58)."""
    angle_buffer = torch.zeros((len(envs_idx), 3), device=gs.device)
    for k, v in enumerate((x, y, z)):
        if isinstance(v, tuple):
            angle_buffer[:, k].uniform_(*v)
    entity.set_quat(xyz_to_quat(angle_buffer), envs_idx=envs_idx)


class position(ResetMdpFnClass):
    """Fixed spawn pose: ``params = {"position": (x, y, z), "quat": (w, x, y, z) | None, "zero_velocity": bool}`` — the
    ``on_reset`` entry of every shipped example but rough_terrain (reference: mdp/reset.py:67-124).

    Inside a step this object is only DESCRIBED to the native reset (``EntityManager._fill_reset`` reads ``reset_pos`` /
    ``reset_quat`` / ``zero_velocity``; the pose is written per lane by ``gf_masked_reset`` / the fused launch).  Calling it with
    an index list — the public signature — hands the pose to the entity's ``envs_idx`` setters as a broadcast view: one row
    per listed env, no per-env staging buffer to scatter into and gather back from."""

    def __init__(self, env, entity, position, quat=None, zero_velocity: bool = True):
        self.env = env
        self.zero_velocity = bool(zero_velocity)
        self.reset_pos = torch.as_tensor(position, device=gs.device, dtype=gs.tc_float).reshape(3)
        self.reset_quat = None if quat is None else torch.as_tensor(quat, device=gs.device, dtype=gs.tc_float).reshape(4)

    def __call__(self, env, entity, envs_idx, position=None, quat=None, zero_velocity: bool = True):
        ids = torch.as_tensor(envs_idx, device=gs.device)
        rows = int(ids.numel())
        if rows == 0:
            return
        entity.set_pos(self.reset_pos.expand(rows, 3), envs_idx=envs_idx, zero_velocity=self.zero_velocity)
        if self.reset_quat is not None:
            entity.set_quat(self.reset_quat.expand(rows, 4), envs_idx=envs_idx, zero_velocity=self.zero_velocity)


class randomize_terrain_position(ResetMdpFnClass):
    """Random position on the terrain and (by default) a random yaw (reset.py:127-226).

    On an entity with masked setters the EntityManager folds this whole function into the masked reset (``GfResetArgs.spawn_*``:
    the draws, the terrain-height lookup, ``xyz_to_quat`` and the pose write happen per lane, no ``nonzero`` / gather / scatter);
    ``gf_spawn`` describes it.  Called directly it runs the reference's sequence through the public setters."""

    def __init__(self, env, entity, terrain_manager, height_offset: float = 0.1e-3, subterrain=None,
                 rotation: dict | None = {"z": (0, 2 * math.pi)}, zero_velocity: bool = True):
        self.env = env
        self.rotation = rotation
        self._rotation_buffer = None
        self._quat_buffer = None

    def build(self):
        self._rotation_buffer = torch.zeros((self.env.num_envs, 3), device=gs.device, dtype=gs.tc_float)
        self._quat_buffer = torch.zeros((self.env.num_envs, 4), device=gs.device, dtype=gs.tc_float)

    def define_quat(self, envs_idx, rotation: dict):
        """Only axes given as ``(lo, hi)`` tuples are written; scalars leave the axis at 0 (reset.py:172-196)."""
        for k, axis in enumerate("xyz"):
            v = rotation.get(axis, 0)
            if isinstance(v, tuple):
                self._rotation_buffer[envs_idx, k] = torch.empty(len(envs_idx), device=gs.device).uniform_(*v)
        self._quat_buffer[envs_idx] = xyz_to_quat(self._rotation_buffer[envs_idx])

    def gf_spawn(self, terrain_manager, height_offset: float = 0.1e-3, subterrain=None, rotation: dict | None = {"z": (0, 2 * math.pi)},
                 zero_velocity: bool = True):
        """(usable area, height offset, rotation ranges, zero_velocity) for the fused reset, or None when it cannot be described
        statically (``subterrain`` given as a callable is re-evaluated by the reference on every reset)."""
        if callable(subterrain) or not hasattr(terrain_manager, "gf_view"):
            return None
        rot = None
        if rotation is not None:
            rot = [rotation.get(axis) if isinstance(rotation.get(axis), tuple) else None for axis in "xyz"]
        return terrain_manager.usable_area(0.5, subterrain), float(height_offset), rot, bool(zero_velocity)

    def __call__(self, env, entity, envs_idx, terrain_manager, height_offset: float = 0.1e-3, subterrain=None,
                 rotation: dict | None = {"z": (0, 2 * math.pi)}, zero_velocity: bool = True):
        sub = subterrain() if callable(subterrain) else subterrain
        pos = terrain_manager.generate_random_env_pos(envs_idx=envs_idx, subterrain=sub, height_offset=height_offset)
        entity.set_pos(pos, envs_idx=envs_idx, zero_velocity=zero_velocity)
        if rotation is not None:
            self.define_quat(envs_idx, rotation)
            entity.set_quat(self._quat_buffer[envs_idx], envs_idx=envs_idx, zero_velocity=zero_velocity)


class terrain_curriculum_position(ResetMdpFnClass):
    """Respawn in the env's own terrain cell, moving terrain levels first when the reset ends an episode
    (``managers.TerrainCurriculum``; legged_gym's ``_update_terrain_curriculum``, Isaac Lab's ``terrain_levels_vel``).
    ``params = {"curriculum": TerrainCurriculum, "height_offset": float, "rotation": {"z": (lo, hi), …} | None, "zero_velocity": bool}``
    with ``randomize_terrain_position``'s meaning of the last three.

    Whichever way it is reached it is ONE ``gf_terrain_curriculum`` launch driven by a mask.  Levels move (``update``) only in the
    in-step reset of finished episodes (``env._in_step``): the first ``reset()`` and resets a training script calls between steps
    respawn the envs in the cell they have.

    * In the step of an env whose EntityManager has this function as its only ``on_reset`` entry, on an entity with masked setters, the
      manager is called with the step's termination masks (``EntityManager._masked_reset``): no index list, no host read, and the
      step stays a recorded one.  Observations of the reset tick rotate by the pre-reset quaternion, as after the fused spawn.
    * Called with an index list — the public signature — the list becomes a mask (``env._ids_to_mask``).  On an entity with masked
      setters the launch writes the scene's buffers; otherwise it writes staging rows that reach the simulator through ``set_pos`` /
      ``set_quat`` by index list, in ``randomize_terrain_position.__call__``'s order."""

    def __init__(self, env, entity, curriculum, height_offset: float = 0.1e-3, rotation: dict | None = {"z": (0, 2 * math.pi)},
                 zero_velocity: bool = True):
        from ..managers.terrain_curriculum import TerrainCurriculum

        if not isinstance(curriculum, TerrainCurriculum):
            raise ValueError("curriculum must be a managers.TerrainCurriculum")
        self._check(height_offset, rotation)
        self.env = env
        self._curriculum = curriculum
        self._stage = None

    @staticmethod
    def _check(height_offset, rotation) -> None:
        if not math.isfinite(float(height_offset)):
            raise ValueError(f"height_offset must be finite, got {height_offset}")
        if rotation is not None:
            if not isinstance(rotation, dict) or any(k not in ("x", "y", "z") for k in rotation):
                raise ValueError("rotation must be None or a dict with keys among 'x', 'y', 'z'")
            for v in rotation.values():
                if isinstance(v, tuple) and (len(v) != 2 or not all(math.isfinite(float(b)) for b in v)):
                    raise ValueError(f"a rotation range must be a finite (lo, hi) pair, got {v}")

    def build(self):
        self._curriculum.build()   # (entity managers are built behind the terrain manager; a terrain without a grid is refused here)

    def respawn(self, mask, mask2, update: bool, pos_in, pos_out, quat, stash, lin_vel, ang_vel, dof_vel, curriculum,
                height_offset: float = 0.1e-3, rotation: dict | None = {"z": (0, 2 * math.pi)}, zero_velocity: bool = True):
        """The launch.  Returns True when it wrote quaternions (``rotation`` is not None)."""
        from ..managers.terrain_curriculum import rotation_ranges

        self._check(height_offset, rotation)
        rot = rotation_ranges(rotation)
        draws = self.env.take_draws("curriculum")
        curriculum.respawn(mask, mask2, pos_in, pos_out, quat_out=quat if rot is not None else None, quat_stash=stash, lin_vel=lin_vel,
                           ang_vel=ang_vel, dof_vel=dof_vel, update=update, height_offset=height_offset, rotation=rot,
                           zero_velocity=zero_velocity, draws=draws)
        return rot is not None

    def __call__(self, env, entity, envs_idx, curriculum, height_offset: float = 0.1e-3,
                 rotation: dict | None = {"z": (0, 2 * math.pi)}, zero_velocity: bool = True):
        mask = env._ids_to_mask(envs_idx)
        update = bool(env._in_step)
        if hasattr(entity, "gf_masked_base"):
            pos, quat, lin, ang = entity.gf_masked_base()
            dof_vel = entity.gf_masked_dofs(None)[1] if hasattr(entity, "gf_masked_dofs") else None
            self.respawn(mask, None, update, pos, pos, quat, None, lin, ang, dof_vel, curriculum, height_offset, rotation, zero_velocity)
            return
        N = env.num_envs
        if self._stage is None:
            self._stage = (torch.zeros(N, 3, device=gs.device, dtype=gs.tc_float), torch.zeros(N, 4, device=gs.device, dtype=gs.tc_float))
        pos_in = entity.get_pos().to(gs.tc_float).contiguous()
        spos, squat = self._stage
        with_quat = self.respawn(mask, None, update, pos_in, spos, squat, None, None, None, None, curriculum, height_offset, rotation,
                                 zero_velocity)
        ids = slice(None) if envs_idx is None else torch.as_tensor(envs_idx, device=gs.device, dtype=torch.long)
        entity.set_pos(spos[ids], envs_idx=envs_idx, zero_velocity=zero_velocity)
        if with_quat:
            entity.set_quat(squat[ids], envs_idx=envs_idx, zero_velocity=zero_velocity)


class randomize_link_mass_shift(ResetMdpFnClass):
    """Mass shift of the links whose name matches ``link_name`` (reference: mdp/reset.py:229-284) — a pure call into Genesis'
    ``set_mass_shift`` at reset time, nothing per env to compute (out of the hot path).

    What reaches the simulator is pinned to the reference's OBSERVABLE behaviour rather than to its intent: there the uniform
    draw lands in the temporary that advanced indexing returns (:271), so the shift handed to ``set_mass_shift`` is the all-zero
    ``[num_envs, n_links]`` tensor, passed whole together with ``envs_idx`` (:274-278).  Here that is stated directly: a zero
    shift per matching link, one draw of the same shape taken from torch's generator so the global RNG stream advances exactly
    as it does in the reference."""

    def __init__(self, _env, entity, link_name: str, add_mass_range: tuple[float, float] = (-0.2, 0.2)):
        self.env = _env
        self.add_mass_range = add_mass_range
        self._entity = entity
        self._link_name = link_name
        self.build()

    def build(self):
        from ..utils import links_by_name_pattern

        matches = links_by_name_pattern(self._entity, self._link_name) if self._link_name is not None else []
        self._links_idx_local = [link.idx_local for link in matches]
        self._zero_shift = torch.zeros((self.env.num_envs, len(self._links_idx_local)), device=gs.device) if matches else None

    def __call__(self, env, entity, envs_idx, link_name: str, add_mass_range: tuple[float, float] = (-0.2, 0.2)):
        lo, hi = self.add_mass_range
        torch.empty((len(envs_idx), len(self._links_idx_local)), device=gs.device).uniform_(lo, hi)   # (drawn and dropped, as upstream)
        self._entity.set_mass_shift(self._zero_shift, links_idx_local=self._links_idx_local, envs_idx=envs_idx)
