"""The camera model of gf_depth_camera (include/gf_step.h) restated in numpy: the pixel operations in float32, one rounding per
operation, with tests/philox.py's draws, and the schedule and ring as a plain list of frames per env."""
import numpy as np

import philox

F = np.float32
M32 = 0xFFFFFFFF
SEED_TAG = 0xDE97CA3E5A11F0A3
SPAN = 16        # GF_DEPTH_CAMERA_SPAN_ENVS (asserted against the binding in the tests)
SENTINEL = F(777.0)
DEFAULTS = dict(interval=5, phase="staggered", stack=1, latency=(0, 0), near=0.0, far=4.0, noise=0.0, dropout=0.0, dropout_value=None,
                normalize=False, seed=0)


def _unit(w):
    return (w >> np.uint32(8)).astype(F) * F(5.9604644775390625e-8)


def _key(cfg):
    k = cfg["seed"] ^ SEED_TAG
    return k & M32, k >> 32


def pixels(d, env_ids, tick, cfg):
    """Step 6: the cast values d [k, R] of the envs env_ids through the sensor."""
    near, far = F(cfg["near"]), F(cfg["far"])
    v = d
    if cfg["noise"] or cfg["dropout"]:
        w = philox.philox4x32_10(np.asarray(env_ids, np.uint32)[:, None], np.arange(d.shape[1], dtype=np.uint32)[None, :], tick, 0, *_key(cfg))
        if cfg["noise"]:
            v = d + F(cfg["noise"]) * (F(2.0) * _unit(w[0]) - F(1.0))
        u1 = _unit(w[1])
    v = np.where(v < near, near, v)
    v = np.where(v > far, far, v)
    if cfg["dropout"]:
        v = np.where(u1 < F(cfg["dropout"]), F(far if cfg["dropout_value"] is None else cfg["dropout_value"]), v)
    if cfg["normalize"]:
        v = (v - near) * F(1.0 / (float(far) - float(near))) - F(0.5)
    return v.astype(F)


class Model:
    """Per env a list of the last S frames, newest last; ring, head, lag, image and due are read off it after every step."""

    def __init__(self, n, r, cfg):
        self.cfg, self.n, self.r = cfg, n, r
        self.S = cfg["latency"][1] + cfg["stack"]
        self.frames = [[np.full(r, SENTINEL)] * self.S for _ in range(n)]
        self.head, self.lag = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.ring = np.full((self.S, n, r), SENTINEL)
        self.image = np.full((n, cfg["stack"] * r), SENTINEL)
        self.due = np.zeros(n, bool)

    def step(self, cast, episode_length, tick):
        """cast [n, R]: caster.cast() of this step's poses."""
        c, S = self.cfg, self.S
        n = np.arange(self.n)
        fresh = episode_length <= 1
        phase = n % c["interval"] if c["phase"] == "staggered" else 0
        self.due = fresh | ((tick + phase) % c["interval"] == 0)
        lo, hi = c["latency"]
        u = _unit(philox.philox4x32_10(n.astype(np.uint32), 0, tick, 1, *_key(c))[0])
        drawn = lo + np.minimum((u * F(hi - lo + 1)).astype(np.int32), hi - lo)
        v = pixels(cast, n, tick, c)
        for i in np.flatnonzero(self.due):
            if fresh[i]:
                self.lag[i] = drawn[i]
                self.frames[i] = [v[i]] * S
            else:
                self.frames[i] = (self.frames[i] + [v[i]])[-S:]
            self.head[i] = (self.head[i] + 1) % S
            for k in range(S):
                self.ring[(self.head[i] - k) % S, i] = self.frames[i][-1 - k]
            self.image[i] = np.concatenate([self.frames[i][-1 - self.lag[i] - ch] for ch in range(c["stack"])])
        return self
