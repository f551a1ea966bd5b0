"""
DepthCamera — the camera model between a ``RayCaster`` and a depth policy: what a deployed sensor does to the image.  A real camera
delivers a frame every few control steps (Extreme-Parkour-style training uses one frame per 5 steps, Isaac Lab's sensors have an
``update_period``), the frame arrives a frame or two late, it is clipped to the sensor's range, it carries noise and holes, and the
policy is fed the last few frames as channels.  The reference has no counterpart.

Composed in torch around ``caster.cast()`` all of that pays a full cast per step, whether or not a new frame is due, and a chain of
``[N, R]`` tensor ops behind it.  ``step()`` is ONE ``gf_depth_camera`` launch (``csrc/gf_depth_camera.hip``; the sequence is written
out in ``include/gf_step.h``): only the envs whose frame is due are cast — with ``phase="staggered"`` about ``N / interval`` of them per
step — and an env that is not due costs four bytes of ``episode_length``.  Per env the camera keeps a ring of ``latency_hi + stack``
frames; ``image`` row ``n`` holds the frames ``lag[n]``, ``lag[n] + 1``, … captures old, newest first.  An env whose episode has just
begun (``episode_length <= 1``, ``ActuatorDelay``'s rule, read in place: no index list, no ``reset()`` override) is always due, draws a
new latency and gets its first frame into every slot and channel, so it never sees another episode's frames.  A backend without the
entry (the test-only CPU oracle) runs the same sequence as torch ops: gather the due rows, ``caster.cast`` on them, the pixel
operations, the ring indexing.

The draws (noise, holes, latency) are Philox blocks under a key of the camera's own (``seed ^ GF_DEPTH_CAMERA_SEED_TAG``) with the
camera's call counter ``tick``, the env and the ray as the counter: the env's stream stays untouched.

The camera is not a manager: it registers nothing with the env.  ``Go2RoughTerrainEnv(depth_camera={…, "model": {…}})`` runs it behind
the step and makes ``image`` the ``"depth"`` observation.  A student's observation ``(proprio_block, camera.image)`` with
``ConvEncoder(image_shape=(stack, H, W), …)`` needs no further change: ``image`` is ``[N, stack·H·W]`` in exactly that order.
"""
from __future__ import annotations

import math
import operator
from typing import Optional

import torch

from .. import _native as nat
from .. import gs
from .terrain_curriculum import _f32, _unit

_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF
_ALIGN = {"world": 0, "yaw": 1, "base": 2}


def _whole(v, what: str, lo: int) -> int:
    if isinstance(v, bool):
        raise ValueError(f"{what} must be a whole number, got {v!r}")
    try:
        v = operator.index(v)
    except TypeError:
        raise ValueError(f"{what} must be a whole number, got {v!r}") from None
    if v < lo:
        raise ValueError(f"{what} must be at least {lo}, got {v}")
    return v


def _latency_pair(latency) -> tuple:
    try:
        lo, hi = latency
    except (TypeError, ValueError):
        raise ValueError(f"latency must be a (lo, hi) pair of frames, got {latency!r}") from None
    lo, hi = _whole(lo, "latency lo", 0), _whole(hi, "latency hi", 0)
    if lo > hi:
        raise ValueError(f"latency needs lo <= hi, got {(lo, hi)}")
    return lo, hi


def _philox(c0: torch.Tensor, c1, c2: int, c3: int, key: int) -> tuple:
    """Philox4x32-10 of csrc/gf_device.h with counter (c0, c1, c2, c3) as int64 tensors in [0, 2^32); ``c0`` and ``c1`` broadcast."""
    def mulhilo(m: int, c: torch.Tensor):
        ch, cl = c >> 16, c & 0xFFFF            # m * ch and m * cl stay below 2^48
        a, b = ch * m, cl * m
        return ((a + (b >> 16)) >> 16), ((b + ((a & 0xFFFF) << 16)) & _M32)

    c0 = c0.to(torch.int64) & _M32
    c1 = (c1 if isinstance(c1, torch.Tensor) else torch.full_like(c0, c1)).to(torch.int64) & _M32
    c0, c1 = torch.broadcast_tensors(c0, c1)
    c2, c3 = torch.full_like(c0, c2 & _M32), torch.full_like(c0, c3 & _M32)
    k0, k1 = key & _M32, (key >> 32) & _M32
    for _ in range(10):
        hi0, lo0 = mulhilo(0xD2511F53, c0)
        hi1, lo1 = mulhilo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


class DepthCamera:
    """``step()`` → ``image`` ``[N, stack·R]``: the last ``stack`` frames of ``caster``'s sensor as the policy would get them.

    ``interval``: control steps between two frames of an env.  ``phase``: ``"staggered"`` — env ``n`` captures in the steps with
    ``(tick + n % interval) % interval == 0``, so every step casts about ``N / interval`` envs — or ``"global"`` — every env in the same
    steps.  ``stack``: frames handed out, newest first.  ``latency`` ``(lo, hi)``: the newest frame handed out is ``lag`` captures old,
    ``lag`` uniform over the whole numbers lo … hi per env and episode; ``max_latency`` (default ``hi``) is what the ring is allocated
    for, so that ``set_latency`` can widen the range later.  ``near`` / ``far`` (default: the caster's ``max_range``) clip the value,
    ``noise`` is the half-width in metres of a uniform error added before the clip, ``dropout`` the probability that a pixel reads
    ``dropout_value`` (default ``far``) instead, ``normalize`` maps ``[near, far]`` to ``[-0.5, 0.5]`` last.  ``use_kernel = False``
    runs the torch composition even on a backend that has the entry (tools/bench_depth_camera.py times both)."""

    def __init__(self, caster, interval: int = 5, phase: str = "staggered", stack: int = 1, latency=(0, 0), near: float = 0.0,
                 far: Optional[float] = None, noise: float = 0.0, dropout: float = 0.0, dropout_value: Optional[float] = None,
                 normalize: bool = False, seed: int = 0, max_latency: Optional[int] = None):
        self.interval = _whole(interval, "interval", 1)
        if interval > 0x7FFFFFFF:
            raise ValueError(f"interval must fit 31 bits, got {interval}")
        if phase not in ("staggered", "global"):
            raise ValueError(f"phase must be 'staggered' or 'global', got {phase!r}")
        self.stack = _whole(stack, "stack", 1)
        self.latency_lo, self.latency_hi = _latency_pair(latency)
        self.max_latency = self.latency_hi if max_latency is None else _whole(max_latency, "max_latency", self.latency_hi)
        self.slots = self.max_latency + self.stack
        if self.slots > nat.GF_DEPTH_CAMERA_MAX_SLOTS:
            raise ValueError(f"the latency's upper end plus stack must be at most {nat.GF_DEPTH_CAMERA_MAX_SLOTS} frames, got {self.slots}")
        far = caster.max_range if far is None else far
        for name, v in (("near", near), ("far", far), ("noise", noise), ("dropout", dropout)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"{name} must be a finite number, got {v!r}")
        self.near, self.far = (float(torch.tensor(float(v), dtype=torch.float32)) for v in (near, far))   # as the kernel sees them
        if not self.near < self.far:
            raise ValueError(f"near must be below far, got near {near!r}, far {far!r}")
        if noise < 0.0:
            raise ValueError(f"noise must not be negative, got {noise!r}")
        if not 0.0 <= dropout <= 1.0:
            raise ValueError(f"dropout is a probability in 0 … 1, got {dropout!r}")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed must be an int, got {seed!r}")
        self.caster, self.env, self.phase = caster, caster.env, phase
        self.noise, self.dropout, self.normalize, self.seed = float(noise), float(dropout), bool(normalize), seed & _M64
        self.dropout_value = self.far if dropout_value is None else float(dropout_value)
        self.inv_span = 1.0 / (self.far - self.near)   # in double; rounded once where it becomes a float32
        self.ring: Optional[torch.Tensor] = None
        self.head: Optional[torch.Tensor] = None
        self._lag: Optional[torch.Tensor] = None
        self._image: Optional[torch.Tensor] = None
        self._due: Optional[torch.Tensor] = None
        self._tick = 0                       # the camera's own call counter (uint32, wrapping): the first step() is tick 0
        self._args = nat.GfDepthCameraArgs()
        self._keep: tuple = ()
        #: False: run the torch composition even on a backend that has the entry
        self.use_kernel = True

    # -- state ---------------------------------------------------------------------------------------------------------------
    def build(self, num_envs: Optional[int] = None) -> None:
        """Allocates the ring, the heads, the lags and the image (zeros) for ``num_envs`` (default: the env's).  Runs once."""
        if self.ring is not None:
            return
        N, R, dev = int(self.env.num_envs if num_envs is None else num_envs), self.caster.num_rays, gs.device
        self.ring = torch.zeros(self.slots, N, R, device=dev, dtype=torch.float32)
        self.head = torch.zeros(N, device=dev, dtype=torch.int32)
        self._lag = torch.zeros(N, device=dev, dtype=torch.int32)
        self._image = torch.zeros(N, self.stack * R, device=dev, dtype=torch.float32)
        self._due = torch.zeros(N, device=dev, dtype=torch.bool)

    @property
    def image(self) -> torch.Tensor:
        """float32 ``[N, stack·R]``: the ONE persistent image, the same tensor object on every call; channel ``c`` of env ``n`` is the
        frame ``lag[n] + c`` captures old."""
        self.build()
        return self._image

    @property
    def lag(self) -> torch.Tensor:
        """int32 ``[N]``: the latency of every env's current episode in frames (the launch's own state, no copy) — a privileged input
        of a critic."""
        self.build()
        return self._lag

    @property
    def due(self) -> torch.Tensor:
        """bool ``[N]``: the envs the last ``step()`` cast."""
        self.build()
        return self._due

    @property
    def tick(self) -> int:
        """The number of ``step()`` calls so far; call ``k`` (counted from 0) runs with tick ``k``."""
        return self._tick

    def set_latency(self, lo: int, hi: int) -> None:
        """A new ``(lo, hi)`` within the allocated ``max_latency``: every env takes it at its next re-draw (a latency curriculum)."""
        lo, hi = _latency_pair((lo, hi))
        if hi > self.max_latency:
            raise ValueError(f"latency {(lo, hi)} exceeds the allocated max_latency {self.max_latency}")
        self.latency_lo, self.latency_hi = lo, hi

    # -- the launch ----------------------------------------------------------------------------------------------------------
    def step(self, pos: Optional[torch.Tensor] = None, quat: Optional[torch.Tensor] = None,
             episode_length: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One ``gf_depth_camera`` launch: casts the envs that are due from ``pos`` ``[N, 3]`` / ``quat`` ``[N, 4]`` (default: the
        entity's, now; strided 2-D views are read in place) and returns ``image``.  ``episode_length`` (int32 ``[N]``, default the
        env's) marks the fresh envs."""
        c, env = self.caster, self.env
        turned = c.align != "world"
        if pos is None or (quat is None and turned):
            bpos, bquat = c._base_state()
            pos = bpos if pos is None else pos
            quat = bquat if quat is None else quat
        pos_stride = c._rows(pos, "pos", None, 3)
        N = int(pos.shape[0])
        quat_stride = c._rows(quat, "quat", N, 4) if turned else 4
        ep = getattr(env, "episode_length", None) if episode_length is None else episode_length
        if (not isinstance(ep, torch.Tensor) or ep.dtype != torch.int32 or tuple(ep.shape) != (N,) or not ep.is_contiguous()
                or ep.device.type != gs.device.type):
            raise ValueError(f"episode_length must be a contiguous int32 tensor of shape ({N},) on {gs.device}")
        self.build(N)
        if self._image.shape[0] != N:
            raise ValueError(f"the camera holds {self._image.shape[0]} envs, pos has {N}")
        tick = self._tick
        self._tick = (tick + 1) & _M32
        launch = getattr(env.backend, "depth_camera", None) if self.use_kernel else None
        if launch is None:
            self._step_torch(pos, quat if turned else None, ep, tick)
            return self._image
        a = self._args
        a.num_envs, a.num_rays = N, c.num_rays
        a.pos, a.pos_stride = pos.data_ptr(), pos_stride
        a.quat, a.quat_stride = (quat.data_ptr(), quat_stride) if turned else (None, 4)
        a.pattern, a.episode_length = c.pattern.data_ptr(), ep.data_ptr()
        a.ring, a.head, a.lag, a.image, a.due_out = (t.data_ptr() for t in (self.ring, self.head, self._lag, self._image, self._due))
        c.terrain_manager.gf_view(a.terrain)
        a.seed, a.tick, a.env_offset = self.seed, tick, getattr(env, "env_offset", 0)
        a.align, a.mode = _ALIGN[c.align], int(c.output == "depth")
        a.axis[0], a.axis[1], a.axis[2] = c.axis
        a.max_range, a.miss_value = c.max_range, c.miss_value
        a.interval, a.staggered, a.stack, a.slots = self.interval, int(self.phase == "staggered"), self.stack, self.slots
        a.latency_lo, a.latency_hi, a.normalize = self.latency_lo, self.latency_hi, int(self.normalize)
        a.near_clip, a.far_clip, a.noise, a.dropout = self.near, self.far, self.noise, self.dropout
        a.dropout_value, a.inv_span = self.dropout_value, self.inv_span
        self._keep = (pos, quat, ep)   # fresh getter tensors and views of temporaries outlive the launch
        launch(a)
        return self._image

    # -- the same sequence in torch ops ----------------------------------------------------------------------------------------
    def _step_torch(self, pos, quat, ep, tick: int) -> None:
        """The kernel's sequence (include/gf_step.h) as separate tensor ops: the due rows gathered, ``caster.cast`` on them, the
        pixel operations one float32 op each, the ring by indexing."""
        dev, c = self._image.device, self.caster
        N, R, S, K, I = int(pos.shape[0]), c.num_rays, self.slots, self.stack, self.interval
        f = lambda v: _f32(v, dev)
        sel = torch.where
        key = (self.seed ^ nat.GF_DEPTH_CAMERA_SEED_TAG) & _M64
        # 1-2: who is due
        n = torch.arange(N, device=dev, dtype=torch.int64)
        fresh = ep <= 1
        phase = n % I if self.phase == "staggered" else torch.zeros_like(n)
        due = fresh | ((((tick + phase) & _M32) % I) == 0)
        self._due.copy_(due)
        idx = due.nonzero().squeeze(1)
        if idx.numel() == 0:
            return
        ids = (idx + int(getattr(self.env, "env_offset", 0))) & _M32
        fr = fresh[idx]
        # 4: the latency
        w = self.latency_hi - self.latency_lo + 1
        u = _unit(_philox(ids, 0, tick, 1, key)[0])
        drawn = self.latency_lo + torch.clamp((u * f(float(w))).to(torch.int64), max=w - 1)
        old = self._lag[idx].to(torch.int64)
        lag = sel(fr, drawn, sel((old < 0) | (old > S - K), torch.zeros_like(old), old))
        self._lag[idx] = sel(fr, drawn, old).to(torch.int32)
        # 5: the head
        h = self.head[idx].to(torch.int64)
        h = (sel((h < 0) | (h >= S), torch.zeros_like(h), h) + 1) % S
        self.head[idx] = h.to(torch.int32)
        # 6: the cast, then the sensor
        d = torch.empty((idx.numel(), R), device=dev, dtype=torch.float32)
        c.cast(pos[idx], None if quat is None else quat[idx], out=d)
        v, u1 = d, None
        if self.noise != 0.0 or self.dropout != 0.0:
            words = _philox(ids.unsqueeze(1), torch.arange(R, device=dev, dtype=torch.int64).unsqueeze(0), tick, 0, key)
            if self.noise != 0.0:
                v = d + f(self.noise) * (f(2.0) * _unit(words[0]) - f(1.0))
            u1 = _unit(words[1])
        near, far = f(self.near), f(self.far)
        v = sel(v < near, near, v)
        v = sel(v > far, far, v)
        if self.dropout != 0.0:
            v = sel(u1 < f(self.dropout), f(self.dropout_value), v)
        if self.normalize:
            v = (v - near) * f(self.inv_span) - f(0.5)
        # 7: the ring and the channels (a fresh env's frame fills every slot, so whichever slot a channel names holds it)
        self.ring[h, idx] = v
        self.ring[:, idx[fr]] = v[fr]
        image = self._image.view(N, K, R)
        for ch in range(K):
            image[idx, ch] = self.ring[(h - lag - ch) % S, idx]
