"""
RayCaster — rays from a sensor on the base against the terrain surface (Isaac Lab's ``RayCaster`` and its camera, the depth images of
the parkour papers): what a deployable student sees on rough terrain, where ``HeightScanner`` is what its teacher sees.  The
reference has no counterpart.

The surface is the bilinear interpolant ``TerrainManager.get_terrain_height`` defines, inside the field's rectangle only; a ray is
clipped to the rectangle, walks the cells it crosses and solves the quadratic that the gap between ray and bilinear patch is inside
each cell — exact, not marched (``include/gf_step.h`` has the contract and the float32 operation sequence).  Composed from torch ops
that walk is a data-dependent loop: every iteration a round of masked tensor ops, hundreds of launches per step.  ``cast()`` is ONE
``gf_ray_cast`` launch (``csrc/gf_ray_cast.hip``).  A backend without the entry (the test-only CPU oracle) gets the same sequence as
float32 tensor ops, all rays in lockstep under masks.

The caster is not a manager: it registers nothing with the env.  ``mdp.observations.ray_cast`` makes it an observation item.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _native as nat
from .. import gs
from .height_scanner import HeightScanner, grid_pattern

_ALIGN = {"world": 0, "yaw": 1, "base": 2}


# ---------------------------------------------------------------------------------------------------------------------------
# patterns: [R, 6] float64 rows (start offset, direction) in the sensor's frame, x forward, y left, z up
# ---------------------------------------------------------------------------------------------------------------------------
def _unit(d: np.ndarray) -> np.ndarray:
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def pinhole_pattern(width: int, height: int, horizontal_fov_deg: float, vertical_fov_deg: Optional[float] = None) -> np.ndarray:
    """``[width·height, 6]`` float64: a pinhole camera looking along +x, one ray through every pixel centre, row-major, top-left pixel
    first (ray ``j·width + i``: column ``i`` from the left, row ``j`` from the top).  Without ``vertical_fov_deg`` the pixels are
    square.  Pair it with ``output="depth"`` for a depth image."""
    if width < 1 or height < 1 or not 0.0 < horizontal_fov_deg < 180.0:
        raise ValueError("a pinhole pattern needs width, height >= 1 and a horizontal field of view inside 0 … 180 degrees")
    th = math.tan(math.radians(horizontal_fov_deg) / 2.0)
    if vertical_fov_deg is None:
        tv = th * height / width
    elif 0.0 < vertical_fov_deg < 180.0:
        tv = math.tan(math.radians(vertical_fov_deg) / 2.0)
    else:
        raise ValueError("the vertical field of view lies inside 0 … 180 degrees")
    u = ((np.arange(width, dtype=np.float64) + 0.5) / width * 2.0 - 1.0) * th      # to the right of the axis
    v = ((np.arange(height, dtype=np.float64) + 0.5) / height * 2.0 - 1.0) * tv    # below it
    d = np.stack([np.ones(width * height), -np.tile(u, height), -np.repeat(v, width)], axis=-1)
    return np.concatenate([np.zeros_like(d), _unit(d)], axis=-1)


def lidar_pattern(channels: int, vertical_fov_deg: Sequence[float], horizontal_fov_deg: float = 360.0,
                  horizontal_res_deg: float = 11.25) -> np.ndarray:
    """``[channels·A, 6]`` float64: ``channels`` elevations spread evenly over ``vertical_fov_deg = (low, high)``, each swept over
    ``horizontal_fov_deg`` centred on +x in steps of ``horizontal_res_deg`` (a full circle has ``360 / res`` azimuths, an arc
    ``fov / res + 1``).  Ray ``c·A + a``: the azimuth is the fast axis, the lowest channel comes first."""
    if channels < 1 or horizontal_res_deg <= 0.0 or not 0.0 < horizontal_fov_deg <= 360.0:
        raise ValueError("a lidar pattern needs channels >= 1, a positive resolution and a horizontal field of view in (0, 360]")
    lo, hi = float(vertical_fov_deg[0]), float(vertical_fov_deg[1])
    steps = int(round(horizontal_fov_deg / horizontal_res_deg))
    n_az = steps if horizontal_fov_deg >= 360.0 else steps + 1
    az = np.radians(-horizontal_fov_deg / 2.0 + np.arange(n_az, dtype=np.float64) * horizontal_res_deg)
    el = np.radians(np.linspace(lo, hi, channels) if channels > 1 else np.array([(lo + hi) / 2.0]))
    az, el = np.tile(az, channels), np.repeat(el, n_az)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=-1)
    return np.concatenate([np.zeros_like(d), _unit(d)], axis=-1)


def down_pattern(size: Sequence[float], resolution: float, height: float) -> np.ndarray:
    """``[ny·nx, 6]`` float64: the height scan's grid (``grid_pattern``) cast straight down from ``height`` above the base."""
    g = grid_pattern(size, resolution).astype(np.float64)
    n = g.shape[0]
    return np.concatenate([g, np.full((n, 1), float(height)), np.zeros((n, 2)), -np.ones((n, 1))], axis=-1)


def mount_rotation(euler_deg: Sequence[float]) -> np.ndarray:
    """The 3 x 3 float64 matrix of the intrinsic z-y'-x'' rotation (yaw, then pitch, then roll) from ``(roll, pitch, yaw)`` in degrees;
    a positive pitch turns +x towards the ground."""
    r, p, y = (math.radians(float(v)) for v in euler_deg)
    cr, sr, cp, sp, cy, sy = math.cos(r), math.sin(r), math.cos(p), math.sin(p), math.cos(y), math.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]], dtype=np.float64)


class RayCaster:
    """``cast()`` → ``[N, R]`` distances (or depths) of ``R`` rays per env against the terrain.

    ``pattern`` is ``[R, 6]`` (start offset and direction per ray in the sensor's frame; the builders above make one);
    ``offset_pos`` / ``offset_euler`` (roll, pitch, yaw in degrees) mount the sensor on the base and are folded into the pattern once,
    in float64, directions normalised there and rounded to float32 once.  ``align="base"`` turns the rays with the base's full
    attitude, ``"yaw"`` with its heading only (the height scan's), ``"world"`` not at all (the quaternion is then never read).
    ``output="distance"`` gives the length along the ray, ``"depth"`` its component along the sensor's optical axis (the mounted +x).
    A ray that meets no surface within ``max_range`` gives ``miss_value`` (default ``max_range``; any float, ``inf`` and ``0`` too)."""

    def __init__(self, env, terrain_manager, entity_manager=None, entity_attr: str = "robot", pattern=None,
                 offset_pos: Sequence[float] = (0.0, 0.0, 0.0), offset_euler: Sequence[float] = (0.0, 0.0, 0.0), align: str = "base",
                 max_range: float = 4.0, output: str = "distance", miss_value: Optional[float] = None):
        if align not in _ALIGN:
            raise ValueError("align must be 'base', 'yaw' or 'world'")
        if output not in ("distance", "depth"):
            raise ValueError("output must be 'distance' or 'depth'")
        max_range = float(max_range)
        if not (math.isfinite(max_range) and max_range >= 0.0):
            raise ValueError("max_range must be finite and non-negative")
        if pattern is None:
            pattern = pinhole_pattern(16, 12, 87.0)
        pat = torch.as_tensor(pattern).detach().to("cpu", torch.float64).numpy()
        if pat.ndim != 2 or pat.shape[1] != 6:
            raise ValueError(f"pattern must be [R, 6], got {tuple(pat.shape)}")
        if not 1 <= pat.shape[0] <= nat.GF_RAY_CAST_MAX_RAYS:
            raise ValueError(f"a cast has 1 … {nat.GF_RAY_CAST_MAX_RAYS} rays, got {pat.shape[0]}")
        if len(offset_pos) != 3 or len(offset_euler) != 3:
            raise ValueError("offset_pos and offset_euler have three entries")
        rm = mount_rotation(offset_euler)
        d = pat[:, 3:6] @ rm.T
        norm = np.linalg.norm(d, axis=-1, keepdims=True)
        if not (np.isfinite(pat).all() and (norm > 0.0).all()):
            raise ValueError("pattern rows must be finite with a non-zero direction")
        p = pat[:, 0:3] @ rm.T + np.asarray(offset_pos, dtype=np.float64)
        self.env = env
        self.terrain_manager = terrain_manager
        self._entity_manager, self._entity_attr = entity_manager, entity_attr
        self.align, self.output, self.max_range = align, output, max_range
        self.miss_value = max_range if miss_value is None else float(miss_value)
        self.axis = tuple(float(np.float32(v)) for v in rm[:, 0])                       # the optical axis in the body frame
        self.pattern = torch.from_numpy(np.concatenate([p, d / norm], axis=-1).astype(np.float32)).contiguous().to(gs.device)
        self._out: Optional[torch.Tensor] = None        # the ONE default output: every cast() without out= returns it
        self._args = nat.GfRayCastArgs()
        self._keep: tuple = ()

    @property
    def num_rays(self) -> int:
        return int(self.pattern.shape[0])

    @property
    def entity(self):
        return self._entity_manager.entity if self._entity_manager is not None else getattr(self.env, self._entity_attr)

    def _base_state(self):
        """As ``HeightScanner._base_state``: the env's per-tick snapshot where it has one, the entity's getters otherwise."""
        views = getattr(self.env, "entity_views", None)
        if views is not None:
            v = views(self.entity)
            return v.pos, v.quat
        ent = self.entity
        return ent.get_pos(), (ent.get_quat() if self.align != "world" else None)

    _rows = staticmethod(HeightScanner._rows)

    # -- the cast ------------------------------------------------------------------------------------------------------------
    def cast(self, pos: Optional[torch.Tensor] = None, quat: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
             hits_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Casts from ``pos`` ``[N, 3]`` / ``quat`` ``[N, 4]`` (default: the entity's, now), strided 2-D views read in place.  Returns
        ``out``: by default ONE persistent ``[N, R]`` buffer — the same tensor object every call, overwritten by the next; an
        ``out=`` view with a row stride is written in place.  ``hits_out`` ``[N, R, 3]`` (contiguous) receives the world hit points,
        the ray's end at ``max_range`` for a miss."""
        R = self.num_rays
        turned = self.align != "world"
        if pos is None or (quat is None and turned):
            bpos, bquat = self._base_state()
            pos = bpos if pos is None else pos
            quat = bquat if quat is None else quat
        pos_stride = self._rows(pos, "pos", None, 3)
        N = int(pos.shape[0])
        quat_stride = self._rows(quat, "quat", N, 4) if turned else 4
        if out is None:
            if self._out is None or self._out.shape[0] != N:
                if self._out is not None:
                    raise ValueError(f"the default output holds {self._out.shape[0]} envs, pos has {N}: pass out=")
                self._out = torch.zeros((N, R), device=gs.device, dtype=torch.float32)
            out = self._out
        out_stride = self._rows(out, "out", N, R)
        if hits_out is not None:
            if (not isinstance(hits_out, torch.Tensor) or hits_out.dtype != torch.float32 or tuple(hits_out.shape) != (N, R, 3)
                    or not hits_out.is_contiguous() or hits_out.device.type != gs.device.type):
                raise ValueError(f"hits_out must be a contiguous float32 [{N}, {R}, 3] tensor on {gs.device}")
        launch = getattr(self.env.backend, "ray_cast", None)
        if launch is None:
            return self._cast_torch(pos, quat if turned else None, out, hits_out)
        a = self._args
        a.num_envs, a.num_rays = N, R
        a.pos, a.pos_stride = pos.data_ptr(), pos_stride
        a.quat, a.quat_stride = (quat.data_ptr(), quat_stride) if turned else (None, 4)
        a.pattern = self.pattern.data_ptr()
        a.out, a.out_stride = out.data_ptr(), out_stride
        a.hits_out = None if hits_out is None else hits_out.data_ptr()
        self.terrain_manager.gf_view(a.terrain)
        a.align, a.mode = _ALIGN[self.align], int(self.output == "depth")
        a.axis[0], a.axis[1], a.axis[2] = self.axis
        a.max_range, a.miss_value = self.max_range, self.miss_value
        self._keep = (pos, quat, out, hits_out)   # fresh getter tensors and views of temporaries outlive the launch
        launch(a)
        return out

    # -- the same sequence in torch ops ---------------------------------------------------------------------------------------
    def _cast_torch(self, pos, quat, out, hits_out) -> torch.Tensor:
        """The kernel's operation sequence (include/gf_step.h) as separate float32 tensor ops, one rounding each: every ray of every
        env in lockstep, the cell walk a bounded loop under masks, the taps by indexing."""
        dev = pos.device
        c32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
        ZERO, ONE, TWO, HALF, FOUR, INF = (c32(v) for v in (0.0, 1.0, 2.0, 0.5, 4.0, math.inf))
        sel = torch.where
        bx, by, bz = pos[:, 0:1], pos[:, 1:2], pos[:, 2:3]
        one, zero = torch.ones_like(bx), torch.zeros_like(bx)
        if quat is None:
            rot = (one, zero, zero, zero, one, zero, zero, zero, one)
        else:
            qw, qx, qy, qz = quat[:, 0:1], quat[:, 1:2], quat[:, 2:3], quat[:, 3:4]
            c = ONE - TWO * (qy * qy + qz * qz)
            s = TWO * (qw * qz + qx * qy)
            if self.align == "yaw":
                nrm = torch.sqrt(c * c + s * s)
                flat = nrm < c32(1e-6)
                cy, sy = sel(flat, ONE, c / nrm), sel(flat, ZERO, s / nrm)
                rot = (cy, -sy, zero, sy, cy, zero, zero, zero, one)
            else:
                rot = (c, TWO * (qx * qy - qw * qz), TWO * (qx * qz + qw * qy),
                       s, ONE - TWO * (qx * qx + qz * qz), TWO * (qy * qz - qw * qx),
                       TWO * (qx * qz - qw * qy), TWO * (qy * qz + qw * qx), ONE - TWO * (qx * qx + qy * qy))
        r00, r01, r02, r10, r11, r12, r20, r21, r22 = rot
        px, py, pz, ex, ey, ez = (self.pattern[:, i].unsqueeze(0) for i in range(6))
        ox = bx + ((r00 * px + r01 * py) + r02 * pz)
        oy = by + ((r10 * px + r11 * py) + r12 * pz)
        oz = bz + ((r20 * px + r21 * py) + r22 * pz)
        dx = (r00 * ex + r01 * ey) + r02 * ez
        dy = (r10 * ex + r11 * ey) + r12 * ez
        dz = (r20 * ex + r21 * ey) + r22 * ez
        tmax = c32(self.max_range)
        view = self.terrain_manager.gf_view()
        field = self.terrain_manager._height_field
        if field is None:
            C = oz - c32(view.origin_z)
            under = C <= ZERO
            tt = C / (-dz)
            hit = under | ((dz < ZERO) & (tt <= tmax))
            t = sel(under, ZERO, tt)
        else:
            t, hit = self._walk_torch(field, view, ox, oy, oz, dx, dy, dz, tmax, (ZERO, ONE, HALF, FOUR, INF))
        val = t
        if self.output == "depth":
            ax, ay, az = (c32(v) for v in self.axis)
            val = t * ((ex * ax + ey * ay) + ez * az)
        out.copy_(sel(hit, val, c32(self.miss_value)))
        if hits_out is not None:
            te = sel(hit, t, tmax)
            hits_out[..., 0] = ox + te * dx
            hits_out[..., 1] = oy + te * dy
            hits_out[..., 2] = oz + te * dz
        return out

    @staticmethod
    def _walk_torch(field, view, ox, oy, oz, dx, dy, dz, tmax, consts):
        ZERO, ONE, HALF, FOUR, INF = consts
        sel = torch.where
        dev = ox.device
        c32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
        H, W = int(field.shape[0]), int(field.shape[1])
        if H < 2 or W < 2:
            raise ValueError("a ray cast needs a height field of at least 2 x 2")
        flat_field = field.reshape(-1)
        fw, fh = c32(float(W - 1)), c32(float(H - 1))
        sx, sy = fw / c32(view.x_span), fh / c32(view.y_span)
        gx0, gy0 = (ox - c32(view.x_min)) * sx, (oy - c32(view.y_min)) * sy
        du, dv = dx * sx, dy * sy
        idu, idv = ONE / du, ONE / dv
        t0, t1 = torch.zeros_like(ox), tmax.expand_as(ox).clone()
        ok = torch.ones_like(ox, dtype=torch.bool)
        for g0, dd, idd, far in ((gx0, du, idu, fw), (gy0, dv, idv, fh)):
            moving = dd != ZERO
            ta, tb = (-g0) * idd, (far - g0) * idd
            lo, hi = sel(ta < tb, ta, tb), sel(ta < tb, tb, ta)
            t0 = sel(moving & (lo > t0), lo, t0)
            t1 = sel(moving & (hi < t1), hi, t1)
            ok = ok & (moving | ((g0 >= ZERO) & (g0 <= far)))
        ok = ok & (t0 <= t1)
        tin = t0
        cell = []
        for g0, dd, last in ((gx0, du, W - 2), (gy0, dv, H - 2)):
            gin = g0 + tin * dd
            fl = torch.floor(gin)
            i = sel(ok, fl, ZERO).nan_to_num(0.0, 0.0, 0.0).to(torch.int64) - ((dd < ZERO) & (gin == fl)).to(torch.int64)
            cell.append(i.clamp(0, last))
        ix, iy = cell
        sgx, sgy = sel(du > ZERO, 1, -1), sel(dv > ZERO, 1, -1)
        active = ok.clone()
        hit = torch.zeros_like(ok)
        t = torch.zeros_like(ox)
        for _ in range((W - 1) + (H - 1) + 1):
            if not bool(active.any()):
                break
            tnx = sel(du != ZERO, ((ix + (du > ZERO)).to(torch.float32) - gx0) * idu, INF)
            tny = sel(dv != ZERO, ((iy + (dv > ZERO)).to(torch.float32) - gy0) * idv, INF)
            tn = sel(tnx < tny, tnx, tny)
            tout = sel(tn < t1, tn, t1)
            tout = sel(tout > tin, tout, tin)
            smax = tout - tin
            u0 = (gx0 + tin * du) - ix.to(torch.float32)
            v0 = (gy0 + tin * dv) - iy.to(torch.float32)
            u0 = sel(u0 < ZERO, ZERO, u0)
            u0 = sel(u0 > ONE, ONE, u0)
            v0 = sel(v0 < ZERO, ZERO, v0)
            v0 = sel(v0 > ONE, ONE, v0)
            zin = oz + tin * dz
            base = iy * W + ix
            h00, h10, h01, h11 = flat_field[base], flat_field[base + 1], flat_field[base + W], flat_field[base + W + 1]
            a, b = h10 - h00, h01 - h00
            k = (h00 - h10) - (h01 - h11)
            C = zin - (((h00 + a * u0) + b * v0) + (k * u0) * v0)
            B = dz - ((a * du + b * dv) + k * (u0 * dv + v0 * du))
            A = -((k * du) * dv)
            s = sel((A == ZERO) & (B < ZERO), C / (-B), INF)
            disc = B * B - (FOUR * A) * C
            quad = (A != ZERO) & (disc >= ZERO)
            sq = torch.sqrt(sel(quad, disc, ZERO))
            q = -HALF * (B + sel(B < ZERO, -sq, sq))
            r1, r2 = q / A, C / q
            s = sel(quad & (r1 >= ZERO) & (r1 < s), r1, s)
            s = sel(quad & (r2 >= ZERO) & (r2 < s), r2, s)
            under = C <= ZERO
            found = active & (under | (s <= smax))
            t = sel(found, sel(under, tin, tin + s), t)
            hit = hit | found
            active = active & ~found & (tn < t1)
            ix = sel(active & (tnx <= tn), ix + sgx, ix)
            iy = sel(active & (tny <= tn), iy + sgy, iy)
            active = active & (ix >= 0) & (ix <= W - 2) & (iy >= 0) & (iy <= H - 2)
            ix, iy = ix.clamp(0, W - 2), iy.clamp(0, H - 2)
            tin = sel(active, tout, tin)
        return t, hit
