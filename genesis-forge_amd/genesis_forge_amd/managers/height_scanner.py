"""
HeightScanner — the terrain height at a pattern of points around the base (legged_gym's ``measured_heights``, Isaac Lab's
``height_scan``): the standard privileged input of a critic or a teacher on rough terrain.  The reference has no counterpart; its
rough-terrain example trains a blind policy.

Composed from ``TerrainManager.get_terrain_height`` a scan is a broadcast pattern, about a dozen elementwise launches for the yaw
rotation, one height launch over ``N·P`` points that reads two ``[N·P]`` temporaries, and a subtraction and a clamp.  ``scan()`` is ONE
``gf_height_scan`` launch (``csrc/gf_height_scan.hip``; arithmetic in ``include/gf_step.h``): the yaw's cosine and sine once per env
from the quaternion, the pattern from LDS, the height through the device function every other terrain query of the library uses —
so ``out`` equals ``clamp((bz - offset) - get_terrain_height(px, py), *clip)`` bit for bit — and ``pos`` / ``quat`` / ``out`` read and
written in place, row strides included (columns of a state tensor in, a column block of a wider observation tensor out).

A backend without the entry (the test-only CPU oracle) gets the same operation sequence as separate float32 tensor ops around
``get_terrain_height``.

The scanner is not a manager: it registers nothing with the env and takes no part in the step loop.  ``mdp.observations.height_scan``
makes it an observation item (``INTEGRATION.md``).
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from .. import _native as nat
from .. import gs


def grid_pattern(size: Sequence[float], resolution: float) -> np.ndarray:
    """``[ny·nx, 2]`` float32 body-frame offsets (x forward, y left) of a grid of ``size`` metres centred on the base:
    ``n = round(size / resolution) + 1`` points per axis at ``-size/2 + i·resolution`` (float64, rounded once), x fastest."""
    if resolution <= 0.0 or size[0] < 0.0 or size[1] < 0.0:
        raise ValueError("size must be non-negative and resolution positive")
    nx, ny = int(round(size[0] / resolution)) + 1, int(round(size[1] / resolution)) + 1
    xs = -float(size[0]) / 2.0 + np.arange(nx, dtype=np.float64) * float(resolution)
    ys = -float(size[1]) / 2.0 + np.arange(ny, dtype=np.float64) * float(resolution)
    return np.stack([np.tile(xs, ny), np.repeat(ys, nx)], axis=-1).astype(np.float32)


class HeightScanner:
    """``scan()`` → ``[N, P]`` heights under ``P`` points around every env's base.

    ``size`` / ``resolution`` give the grid (default 1.6 m × 1.0 m at 0.1 m: 17 × 11 = 187 points, point ``p = j·nx + i``);
    ``pattern`` replaces it with explicit ``[P, 2]`` offsets.  ``align="yaw"`` turns the pattern with the base's heading, ``"world"``
    keeps the world axes (the quaternion is then never read).  ``relative=True`` gives ``(bz - offset) - h`` (how far the ground is
    below the sensor plane ``offset`` under the base), ``False`` the terrain height ``h`` itself; either is clamped to ``clip``
    (``±inf`` allowed)."""

    def __init__(self, env, terrain_manager, entity_manager=None, entity_attr: str = "robot", size: Sequence[float] = (1.6, 1.0),
                 resolution: float = 0.1, pattern=None, align: str = "yaw", offset: float = 0.5, clip: Sequence[float] = (-1.0, 1.0),
                 relative: bool = True):
        if align not in ("yaw", "world"):
            raise ValueError("align must be 'yaw' or 'world'")
        lo, hi = float(clip[0]), float(clip[1])
        if lo > hi:
            raise ValueError("clip[0] must not exceed clip[1]")
        if pattern is None:
            pat = torch.from_numpy(grid_pattern(size, resolution))
        else:
            pat = torch.as_tensor(pattern).detach().to("cpu", torch.float32)
            if pat.dim() != 2 or pat.shape[1] != 2:
                raise ValueError(f"pattern must be [P, 2], got {tuple(pat.shape)}")
        if not 1 <= pat.shape[0] <= nat.GF_HEIGHT_SCAN_MAX_POINTS:
            raise ValueError(f"a scan has 1 … {nat.GF_HEIGHT_SCAN_MAX_POINTS} points, got {pat.shape[0]}")
        self.env = env
        self.terrain_manager = terrain_manager
        self._entity_manager, self._entity_attr = entity_manager, entity_attr
        self.align, self.relative, self.offset, self.clip = align, bool(relative), float(offset), (lo, hi)
        self.pattern = pat.contiguous().to(gs.device)   # uploaded once
        self._out: Optional[torch.Tensor] = None        # the ONE default output: every scan() without out= returns it
        self._args = nat.GfHeightScanArgs()
        self._keep: tuple = ()

    @property
    def num_points(self) -> int:
        return int(self.pattern.shape[0])

    @property
    def entity(self):
        return self._entity_manager.entity if self._entity_manager is not None else getattr(self.env, self._entity_attr)

    # -- inputs ------------------------------------------------------------------------------------------------------------
    def _base_state(self):
        """The entity's position and quaternion now.  An env that snapshots the base state per tick (``GenesisEnv.entity_views``: the
        synthetic scene's own buffers, or one ``get_pos()`` / ``get_quat()`` of a Genesis-shaped scene per tick) is asked for that;
        anything else for the getters themselves."""
        views = getattr(self.env, "entity_views", None)
        if views is not None:
            v = views(self.entity)
            return v.pos, v.quat
        ent = self.entity
        return ent.get_pos(), (ent.get_quat() if self.align == "yaw" else None)

    @staticmethod
    def _rows(t: torch.Tensor, what: str, n: Optional[int], width: int) -> int:
        """Checks a ``[n, width]`` float32 tensor with unit column stride on the device; returns its row stride in floats."""
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError(f"{what} must be a float32 tensor")
        if t.device.type != gs.device.type:
            raise ValueError(f"{what} lives on {t.device}, the scan runs on {gs.device}")
        if t.dim() != 2 or t.shape[1] != width or (n is not None and t.shape[0] != n):
            raise ValueError(f"{what} must be [{'N' if n is None else n}, {width}], got {tuple(t.shape)}")
        if width > 1 and t.stride(1) != 1:
            raise ValueError(f"{what} must have unit column stride")
        stride = int(t.stride(0))
        if t.shape[0] <= 1:
            return max(stride, width)
        if stride < width:
            raise ValueError(f"{what} must have a row stride of at least {width} floats, got {stride}")
        return stride

    # -- the scan ------------------------------------------------------------------------------------------------------------
    def scan(self, pos: Optional[torch.Tensor] = None, quat: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
             points_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Heights for ``pos`` ``[N, 3]`` / ``quat`` ``[N, 4]`` (default: the entity's, now), strided 2-D views read in place.  Returns
        ``out``: by default ONE persistent ``[N, P]`` buffer — the same tensor object every call, overwritten by the next; an
        ``out=`` view with a row stride is written in place.  ``points_out`` ``[N, P, 2]`` (contiguous) receives the world sample
        points."""
        P = self.num_points
        yaw = self.align == "yaw"
        if pos is None or (quat is None and yaw):
            bpos, bquat = self._base_state()
            pos = bpos if pos is None else pos
            quat = bquat if quat is None else quat
        pos_stride = self._rows(pos, "pos", None, 3)
        N = int(pos.shape[0])
        quat_stride = self._rows(quat, "quat", N, 4) if yaw else 4
        if out is None:
            if self._out is None or self._out.shape[0] != N:
                if self._out is not None:
                    raise ValueError(f"the default output holds {self._out.shape[0]} envs, pos has {N}: pass out=")
                self._out = torch.zeros((N, P), device=gs.device, dtype=torch.float32)
            out = self._out
        out_stride = self._rows(out, "out", N, P)
        if points_out is not None:
            if (not isinstance(points_out, torch.Tensor) or points_out.dtype != torch.float32 or tuple(points_out.shape) != (N, P, 2)
                    or not points_out.is_contiguous() or points_out.device.type != gs.device.type):
                raise ValueError(f"points_out must be a contiguous float32 [{N}, {P}, 2] tensor on {gs.device}")
        backend = self.env.backend
        launch = getattr(backend, "height_scan", None)
        if launch is None:
            return self._scan_torch(pos, quat if yaw else None, out, points_out)
        a = self._args
        a.num_envs, a.num_points = N, P
        a.pos, a.pos_stride = pos.data_ptr(), pos_stride
        a.quat, a.quat_stride = (quat.data_ptr(), quat_stride) if yaw else (None, 4)
        a.pattern = self.pattern.data_ptr()
        a.out, a.out_stride = out.data_ptr(), out_stride
        a.points_out = None if points_out is None else points_out.data_ptr()
        self.terrain_manager.gf_view(a.terrain)   # per call, as get_terrain_height does
        a.align, a.relative = int(yaw), int(self.relative)
        a.offset, (a.clip_lo, a.clip_hi) = self.offset, self.clip
        self._keep = (pos, quat, out, points_out)   # fresh getter tensors and views of temporaries outlive the launch
        launch(a)
        return out

    def _scan_torch(self, pos, quat, out, points_out) -> torch.Tensor:
        """The kernel's operation sequence (include/gf_step.h) as separate float32 tensor ops — one rounding each."""
        f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=pos.device)
        ox, oy = self.pattern[:, 0].unsqueeze(0), self.pattern[:, 1].unsqueeze(0)
        bx, by, bz = pos[:, 0:1], pos[:, 1:2], pos[:, 2:3]
        if quat is not None:
            qw, qx, qy, qz = quat[:, 0:1], quat[:, 1:2], quat[:, 2:3], quat[:, 3:4]
            c = f32(1.0) - f32(2.0) * (qy * qy + qz * qz)
            s = f32(2.0) * (qw * qz + qx * qy)
            nrm = torch.sqrt(c * c + s * s)
            flat = nrm < f32(1e-6)
            cy = torch.where(flat, f32(1.0), c / nrm)
            sy = torch.where(flat, f32(0.0), s / nrm)
        else:
            cy, sy = torch.ones_like(bx), torch.zeros_like(bx)
        px = bx + (cy * ox - sy * oy)
        py = by + (sy * ox + cy * oy)
        if points_out is not None:
            points_out[..., 0] = px
            points_out[..., 1] = py
        h = self.terrain_manager.get_terrain_height(px.reshape(-1), py.reshape(-1)).view(px.shape)
        v = (bz - f32(self.offset)) - h if self.relative else h
        out.copy_(torch.clamp(v, min=self.clip[0], max=self.clip[1]))
        return out
