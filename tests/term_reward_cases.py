"""gf_termination_step, gf_reward_step and gf_entity_rotate restated in numpy, and the cases that pin them at their edges.

The restatements are written from ``termination_body`` / ``reward_body`` (csrc/gf_termination.hip, csrc/gf_reward.hip), the term
bodies of csrc/gf_terms.h and the helpers of csrc/gf_device.h (``rot_inv``, ``norm2``, ``norm3``, ``clamp_max``, ``clamp_min``,
``terrain_height``) against the reference's managers/termination_manager.py:151-190, managers/reward_manager.py:166-195,
mdp/terminations.py and mdp/rewards.py.  float32 arithmetic is one rounding per operation in the order of the code (the library is
built with -ffp-contract=off); the two fused operations of the step kernels, the ``fmaf`` chains of ``norm2`` / ``norm3``, are
evaluated exactly (``fma32``: the product is exact in float64, the sum is rounded to odd there and once more to float32).  The
reward is the left fold ``buf += v * w`` in table order, ``episode_sums[row] += v * w`` starts from the value the launch found,
``episode_seconds += dt``, and ``BODY_ACCEL_EXP`` writes the body-frame velocities back into its state rows.

Every evaluator takes the number type as an argument: run with float64 it is the same formula at high precision — what shows that
the float32 restatement is the operation and not a copy of a kernel's mistake (``f64_gap``; the project's rule
``atol = 1e-5 * max(1, max|want|)``).

Descriptors are ``reset_cases.Spec`` objects whose array and scalar names are the dotted paths of the descriptor fields
(``entity.quat``, ``contact.3.num_links``, ``ext.15``) plus a list of term rows; ``Launch`` below fills the term table and
otherwise is ``reset_cases.Launch``: guarded buffers, 64 sentinel rows behind every array, NULL-pointer buffers allocated all the
same, comparison through integer views.

Terms that pass through ``expf`` (BODY_ACCEL_EXP, CMD_TRACK_LIN_VEL, CMD_TRACK_ANG_VEL, GAIT_PHASE, FOOT_HEIGHT) stay out of the
structural cases: the device's ``expf`` and libm's need not agree to the bit.  Each has one EVAL-mode case of its own (``EXP``):
rows whose argument is exactly 0 or overflows are compared with ``==``, random rows under the 1e-5 rule against float64.

Probe values stay clear of every decision threshold (tests/test_mask_edges.py owns those), and no case but the rotate one lets a
NaN reach a float32 buffer (the sign of a generated NaN is the platform's)."""
import functools

import numpy as np

import reset_cases as rc
from genesis_forge_amd import _native as nat
from reset_cases import F, PAD_ROWS, SHARDS, SIZES, Spec, _f, _ints, command_spec, gait_spec  # noqa: F401  (some re-exported for the tests)

F64 = np.float64
STEP, EVAL = nat.GF_REWARD_MODE_STEP, nat.GF_REWARD_MODE_EVAL
CMD, TERRAIN, MAX, FIRST = nat.GF_RW_FLAG_CMD, nat.GF_RW_FLAG_TERRAIN, nat.GF_RW_FLAG_MAX, nat.GF_RW_FLAG_FIRST_CALL
TIME_OUT = nat.GF_TERM_FLAG_TIME_OUT
EXP_OPS = (nat.GF_R_BODY_ACCEL_EXP, nat.GF_R_CMD_TRACK_LIN_VEL, nat.GF_R_CMD_TRACK_ANG_VEL, nat.GF_R_GAIT_PHASE, nat.GF_R_FOOT_HEIGHT)
GAIT_ROW, GAIT_OBS_WIDTH = 16, 14   # GF_GAIT_ROW, GF_GAIT_OBS_WIDTH
TERRAIN_SC = {"terrain.x_min": -3.0, "terrain.x_span": 12.0, "terrain.y_min": 1.5, "terrain.y_span": 10.0, "terrain.origin_z": 0.25}


# ---- float32 building blocks, in the documented operation order ------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, exactly: a·b is exact in float64; the float64 sum is rounded to odd (TwoSum gives its error),
    so the second rounding, to float32, is the only one that counts."""
    a, b, c = (np.asarray(x, F).astype(F64) for x in np.broadcast_arrays(a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = np.ascontiguousarray(p + c)
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F)


class Num:
    """The arithmetic of one number type: float32 (the restatement) or float64 (the same formulas at high precision)."""

    def __init__(self, dt):
        self.dt = dt

    def __call__(self, x):
        """A descriptor scalar: it is a float32 whatever it is computed with afterwards."""
        return self.dt(F(x))

    def arr(self, x):
        return None if x is None else np.asarray(x).astype(self.dt)

    def fma(self, a, b, c):
        return fma32(a, b, c) if self.dt is F else a * b + c

    def norm3(self, x, y, z):   # sqrtf(fmaf(z, z, fmaf(y, y, x * x)))
        return np.sqrt(self.fma(z, z, self.fma(y, y, x * x)))

    def norm2(self, x, y):      # sqrtf(fmaf(y, y, x * x))
        return np.sqrt(self.fma(y, y, x * x))

    def exp(self, x):           # the one operation that is NOT restated to the bit: float64 exp, rounded once
        return np.exp(np.asarray(x, F64)).astype(self.dt)


X32, X64 = Num(F), Num(F64)


def rot_inv(q, v):
    """transform_by_quat(v, inv_quat(q)), gf_device.h ``rot_inv``: q [n, 4] (w, x, y, z), v [n, 3]."""
    two = q.dtype.type(2.0)
    w, a, b, c = q[:, 0], -q[:, 1], -q[:, 2], -q[:, 3]
    t0 = (b * v[:, 2] - c * v[:, 1]) * two
    t1 = (c * v[:, 0] - a * v[:, 2]) * two
    t2 = (a * v[:, 1] - b * v[:, 0]) * two
    return np.stack([(v[:, 0] + w * t0) + (b * t2 - c * t1), (v[:, 1] + w * t1) + (c * t0 - a * t2), (v[:, 2] + w * t2) + (a * t1 - b * t0)], axis=1)


def gravity(q):
    return rot_inv(q, np.broadcast_to(np.array([0.0, 0.0, -1.0], q.dtype), (q.shape[0], 3)))


def clamp_max(x, hi):
    return np.where(x > hi, hi, x)   # x > hi ? hi : x — a NaN stays


def clamp_min(x, lo):
    return np.where(x < lo, lo, x)


def terrain_height(X, tv, x, y):
    """gf_device.h ``terrain_height``: the in-place normalisation chain, border clip, four taps summed nw, ne, sw, se."""
    f = tv["height_field"]
    if f is None:
        return np.full(x.shape, X(tv["origin_z"]))
    H, W = f.shape
    f = f.astype(X.dt)
    one, two, zero = X.dt(1.0), X.dt(2.0), X.dt(0.0)

    def index(v, v_min, span, size):
        n = v - X(v_min)
        n = n / X(span)
        n = n * two
        n = n - one
        i = ((n + one) / two) * X.dt(size - 1)
        return clamp_max(clamp_min(i, zero), X.dt(size - 1))

    ix, iy = index(x, tv["x_min"], tv["x_span"], W), index(y, tv["y_min"], tv["y_span"], H)
    fx0, fy0 = np.floor(ix), np.floor(iy)
    fx1, fy1 = fx0 + one, fy0 + one
    nw, ne, sw, se = (fx1 - ix) * (fy1 - iy), (ix - fx0) * (fy1 - iy), (fx1 - ix) * (iy - fy0), (ix - fx0) * (iy - fy0)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    x1_in, y1_in = x0 + 1 < W, y0 + 1 < H
    x1, y1 = np.where(x1_in, x0 + 1, x0), np.where(y1_in, y0 + 1, y0)
    v_nw, v_ne = f[y0, x0], np.where(x1_in, f[y0, x1], zero)
    v_sw, v_se = np.where(y1_in, f[y1, x0], zero), np.where(x1_in & y1_in, f[y1, x1], zero)
    return ((v_nw * nw + v_ne * ne) + v_sw * sw) + v_se * se


# ---- a term row -----------------------------------------------------------------------------------------------------------------------
def T(op, w=1.0, p=(), i=(), flags=0, row=None):
    return dict(op=op, flags=flags, w=w, p=list(p) + [0.0] * (4 - len(p)), i=list(i) + [0] * (4 - len(i)), row=row)


def table(*terms, rows=None):
    """The rows in table order; ``row`` is the position unless ``rows`` names it."""
    out = []
    for k, t in enumerate(terms):
        t = dict(t)
        t["row"] = (rows[k] if rows is not None else k) if t["row"] is None else t["row"]
        out.append(t)
    return out


def tspec(fn, sc, arr, terms, null=(), stats=False):
    s = Spec(fn, sc, arr, null, stats=stats)
    s.terms = list(terms)
    s.sc["num_terms"] = len(s.terms)
    return s


def with_arrays(spec, arr):
    """The same call on other arrays."""
    s = tspec(spec.fn, spec.sc, arr, spec.terms, spec.null, spec.stats)
    s.offs = dict(spec.offs)
    return s


# ---- termination ------------------------------------------------------------------------------------------------------------------------
def termination_values(spec, a, X):
    """[K] boolean [N] arrays: ``eval_termination_term`` of gf_terms.h for every env."""
    N = spec.sc["num_envs"]
    has_max = a.get("max_episode_length") is not None
    ep = a["episode_length"] if a.get("episode_length") is not None else np.zeros(N, np.int32)
    out = []
    for t in spec.terms:
        op, p, i = t["op"], t["p"], t["i"]
        if op == nat.GF_T_TIMEOUT:
            v = (ep > a["max_episode_length"]) if has_max else np.zeros(N, bool)
        elif op == nat.GF_T_BAD_ORIENTATION:
            g = gravity(X.arr(a["entity.quat"]))
            tilt_sin = clamp_max(X.norm2(g[:, 0], g[:, 1]), X(0.99))
            v = ~(ep <= i[0]) & (tilt_sin > X(p[0]))
        elif op == nat.GF_T_BASE_HEIGHT_BELOW:
            v = X.arr(a["entity.pos"])[:, 2] < X(p[0])
        elif op == nat.GF_T_OUT_OF_BOUNDS:
            pos = X.arr(a["entity.pos"])
            v = (pos[:, 0] < X(p[0])) | (pos[:, 0] > X(p[1])) | (pos[:, 1] < X(p[2])) | (pos[:, 1] > X(p[3]))
        elif op in (nat.GF_T_HAS_CONTACT, nat.GF_T_CONTACT_FORCE, nat.GF_T_CONTACT_FORCE_GRACE):
            f = X.arr(a["contact.%d.contacts" % i[0]])
            cnt = (X.norm3(f[:, :, 0], f[:, :, 1], f[:, :, 2]) > X(p[0])).sum(axis=1)
            v = {nat.GF_T_HAS_CONTACT: cnt >= i[1], nat.GF_T_CONTACT_FORCE: cnt > 0, nat.GF_T_CONTACT_FORCE_GRACE: ~(ep <= i[1]) & (cnt > 0)}[op]
        elif op == nat.GF_T_EXTERNAL:
            v = a["ext.%d" % i[0]] != 0
        else:
            raise KeyError(op)
        out.append(np.asarray(v, bool))
    return out


def restate_termination(spec, X=X32):
    sc, a = spec.sc, spec.seen()
    N = sc["num_envs"]
    term, trunc = np.zeros(N, bool), np.zeros(N, bool)
    fired = [0] * nat.GF_MAX_TERM_TERMS
    with np.errstate(all="ignore"):
        vals = termination_values(spec, a, X)
    for k, (t, v) in enumerate(zip(spec.terms, vals)):
        if t["flags"] & TIME_OUT:
            trunc |= v
        else:
            term |= v
        if a["term_out"] is not None:
            a["term_out"][k, :] = v
        fired[k] = int(v.sum())
    a["terminated"][:] = term
    a["truncated"][:] = trunc
    return a, dict(term_fired=fired)


# ---- reward ---------------------------------------------------------------------------------------------------------------------------
def _cmd_cols(a, X, view):
    return X.arr(a["command.%d.command" % view])


def reward_values(spec, a, X):
    """[T] arrays [N]: ``eval_reward_term`` for every env, in table order.  BODY_ACCEL_EXP updates its state rows in ``a``."""
    sc = spec.sc
    N, D = sc["num_envs"], sc["num_dofs"]
    dt = X.dt
    zero, one = dt(0.0), dt(1.0)
    memo = {}

    def once(name, fn):
        if name not in memo:
            memo[name] = fn()
        return memo[name]

    quat = lambda: once("quat", lambda: X.arr(a["entity.quat"]))
    pos = lambda: once("pos", lambda: X.arr(a["entity.pos"]))
    blin = lambda: once("blin", lambda: rot_inv(quat(), X.arr(a["entity.lin_vel"])))
    bang = lambda: once("bang", lambda: rot_inv(quat(), X.arr(a["entity.ang_vel"])))
    grav = lambda: once("grav", lambda: gravity(quat()))

    def dof_dev():
        p, d0 = X.arr(a["dof_pos"]), X.arr(a["default_dof_pos"])
        s = np.zeros(N, dt)
        for d in range(D):   # dof_dev += fabsf(dof_pos[d] - default[d]), columns in order
            s = s + np.abs(p[:, d] - d0[d])
        return s

    def act_rate():
        la, ac = X.arr(a["last_actions"]), X.arr(a["actions"])
        s = np.zeros(N, dt)
        for d in range(D):
            df = la[:, d] - ac[:, d]
            s = s + df * df
        return s

    def cmd01(view):
        c = _cmd_cols(a, X, view)
        return c[:, 0], c[:, 1]

    out = []
    for t in spec.terms:
        op, p, i, flags = t["op"], t["p"], t["i"], t["flags"]
        if op == nat.GF_R_IS_ALIVE:
            v = np.where(a["terminated"] != 0, zero, one)
        elif op == nat.GF_R_TERMINATED:
            v = np.where(a["terminated"] != 0, one, zero)
        elif op == nat.GF_R_BASE_HEIGHT:
            h = pos()[:, 2]
            if flags & TERRAIN:
                tv = {k[8:]: w for k, w in sc.items() if k.startswith("terrain.")}
                tv["height_field"] = a.get("terrain.height_field")
                h = h - terrain_height(X, tv, pos()[:, 0], pos()[:, 1])
            target = _cmd_cols(a, X, i[0])[:, 0] if flags & CMD else X(p[0])
            e = h - target
            v = e * e
        elif op == nat.GF_R_DOF_SIMILAR_TO_DEFAULT:
            v = once("dof_dev", dof_dev)
        elif op == nat.GF_R_LIN_VEL_Z_L2:
            v = blin()[:, 2] * blin()[:, 2]
        elif op == nat.GF_R_ANG_VEL_XY_L2:
            v = bang()[:, 0] * bang()[:, 0] + bang()[:, 1] * bang()[:, 1]
        elif op == nat.GF_R_FLAT_ORIENTATION_L2:
            v = grav()[:, 0] * grav()[:, 0] + grav()[:, 1] * grav()[:, 1]
        elif op == nat.GF_R_BODY_ACCEL_EXP:
            st = a["state.%d" % i[0]]
            prev = X.arr(st)
            la, aa = np.zeros((N, 3), dt), np.zeros((N, 3), dt)
            if not flags & FIRST:
                la, aa = (blin() - prev[:, 0:3]) / X(sc["dt"]), (bang() - prev[:, 3:6]) / X(sc["dt"])
            st[:, 0:3], st[:, 3:6] = blin(), bang()   # (float32 rows: the float64 run writes its own copy)
            motion = X.norm3(la[:, 0], la[:, 1], la[:, 2]) + X.norm3(aa[:, 0], aa[:, 1], aa[:, 2])
            v = one - X.exp((-X(p[0])) * motion)
        elif op == nat.GF_R_ACTION_RATE_L2:
            v = once("act_rate", act_rate)
        elif op == nat.GF_R_CMD_TRACK_LIN_VEL:
            c0, c1 = cmd01(i[0])
            e0, e1 = c0 - blin()[:, 0], c1 - blin()[:, 1]
            err = e0 * e0 + e1 * e1
            v = X.exp((-err) / X(p[0]))
        elif op == nat.GF_R_CMD_TRACK_ANG_VEL:
            e = _cmd_cols(a, X, i[0])[:, i[1]] - bang()[:, 2]
            v = X.exp((-(e * e)) / X(p[0]))
        elif op == nat.GF_R_STAND_STILL:
            c0, c1 = cmd01(i[0])
            v = once("dof_dev", dof_dev) * np.where(X.norm2(c0, c1) < X(p[0]), one, zero)
        elif op in (nat.GF_R_HAS_CONTACT, nat.GF_R_CONTACT_FORCE, nat.GF_R_FEET_SLIDE):
            f = X.arr(a["contact.%d.contacts" % i[0]])
            fn = X.norm3(f[:, :, 0], f[:, :, 1], f[:, :, 2])
            if op == nat.GF_R_HAS_CONTACT:
                v = np.where((fn > X(p[0])).sum(axis=1) >= i[1], one, zero)
            else:
                if op == nat.GF_R_FEET_SLIDE:
                    w = X.arr(a["contact.%d.link_vel" % i[0]])
                    per = X.norm3(w[:, :, 0], w[:, :, 1], w[:, :, 2]) * np.where(fn > one, one, zero)
                else:
                    per = clamp_min(fn - X(p[0]), zero)
                v = np.zeros(N, dt)
                for l in range(f.shape[1]):   # links in order
                    v = v + per[:, l]
        elif op == nat.GF_R_FEET_AIR_TIME:
            cc, la = X.arr(a["contact.%d.current_contact_time" % i[0]]), X.arr(a["contact.%d.last_air_time" % i[0]])
            made = np.where((cc > zero) & (cc < X(p[2])), one, zero)
            air = (la - X(p[0])) * made
            if flags & MAX:
                air = clamp_max(air, X(p[1]))
            v = np.zeros(N, dt)
            for l in range(cc.shape[1]):
                v = v + air[:, l]
            if i[1] >= 0:
                c0, c1 = cmd01(i[1])
                v = v * np.where(X.norm2(c0, c1) > X(0.1), one, zero)
        elif op == nat.GF_R_EXTERNAL:
            v = X.arr(a["ext.%d" % i[0]])
        elif op == nat.GF_R_GAIT_PHASE:
            f, w = X.arr(a["contact.%d.contacts" % i[0]]), X.arr(a["contact.%d.link_vel" % i[0]])
            flag_bytes = a.get("gait_wave_flags")
            any_bits = int(np.bitwise_or.reduce(flag_bytes)) if flag_bytes is not None else 0   # (pad bytes are zero: the host's rule)
            v = None
            for k in range(4):
                l = (i[2] >> (8 * k)) & 0xFF
                force, vel = X.norm3(f[:, l, 0], f[:, l, 1], f[:, l, 2]), X.norm3(w[:, l, 0], w[:, l, 1], w[:, l, 2])
                # swing / stance is decided on the float32 rows in either run: it is a decision, not a value
                fl = (rc.foot_flags(a["command.%d.command" % i[1]][:, 15], a["command.%d.command" % i[1]][:, 0:4], p[1]) >> (2 * k)) & 3
                if flag_bytes is not None and N > 0:   # the reference's env-0 index-list quirk
                    if (any_bits >> (2 * k + 1)) & 1:
                        fl[0] = 2
                    elif (any_bits >> (2 * k)) & 1:
                        fl[0] = 1
                fw, vw = np.where(fl & 1, -one, zero), np.where(fl & 2, -one, zero)
                foot = vw * vel + fw * force
                v = foot if k == 0 else v + foot
            v = X.exp(v)
        elif op == nat.GF_R_FOOT_HEIGHT:
            g = _cmd_cols(a, X, i[1])
            w, lp = X.arr(a["contact.%d.link_vel" % i[0]]), X.arr(a["contact.%d.link_pos" % i[0]])
            err = None
            for k in range(4):
                l = (i[2] >> (8 * k)) & 0xFF
                d = lp[:, l, 2] - g[:, 4]
                e = X.norm2(w[:, l, 0], w[:, l, 1]) * (d * d)
                err = e if k == 0 else err + e
            v = X.exp((-err) / X(p[0]))
        else:
            raise KeyError(op)
        out.append(np.asarray(v, dt))
    return out


def fold(vals, terms, dt=F, reverse=False):
    """``buf += v * w`` over the table, left to right (or, for the order-sensitivity check, right to left)."""
    buf = np.zeros(vals[0].shape if vals else 0, dt)
    pairs = list(zip(vals, terms))
    for v, t in (reversed(pairs) if reverse else pairs):
        buf = buf + v * dt(F(t["w"]))
    return buf


def restate_reward(spec):
    sc, a = spec.sc, spec.seen()
    N = sc["num_envs"]
    with np.errstate(all="ignore"):
        vals = reward_values(spec, a, X32)
        if sc["mode"] == EVAL:
            for t, v in zip(spec.terms, vals):
                a["term_out"][t["row"], :] = v
        else:
            buf = np.zeros(N, F)
            for t, v in zip(spec.terms, vals):
                vw = v * F(t["w"])
                buf = buf + vw
                if sc["logging_enabled"] and a["episode_sums"] is not None:
                    a["episode_sums"][t["row"], :] = a["episode_sums"][t["row"]] + vw
            a["reward"][:] = buf
            a["episode_seconds"][:] = a["episode_seconds"] + F(sc["dt"])
    return a, None


def rotate_values(spec, a, X):
    q, what = X.arr(a["entity.quat"]), spec.sc["what"]
    with np.errstate(all="ignore"):
        return gravity(q) if what == nat.GF_ROT_PROJ_GRAVITY else rot_inv(q, X.arr(a["entity.lin_vel"] if what == nat.GF_ROT_LIN_VEL else a["entity.ang_vel"]))


def restate_rotate(spec):
    a = spec.seen()
    a["out"][:] = rotate_values(spec, a, X32)
    return a, None


def rotate_f64_gap(spec):
    """|float32 restatement − float64 evaluation| of the rotated vectors in units of 1e-5 · max(1, max|float64 value|); the NaN env
    must be NaN in both and is left out."""
    v32, v64 = rotate_values(spec, spec.seen(), X32), rotate_values(spec, spec.seen(), X64)
    assert np.array_equal(np.isnan(v32), np.isnan(v64))
    fin = ~np.isnan(v64)
    return float(np.abs(v32[fin].astype(F64) - v64[fin]).max() / (1e-5 * max(1.0, float(np.abs(v64[fin]).max()))))


def restate(spec, flags_all=False):
    if spec.fn == "termination_step":
        return restate_termination(spec)
    if spec.fn == "reward_step":
        return restate_reward(spec)
    if spec.fn == "entity_rotate":
        return restate_rotate(spec)
    return rc.restate(spec, flags_all)


def f64_gap(spec):
    """The largest |float32 restatement − float64 evaluation| over the call's term values (and the folded reward in STEP mode), in units
    of the project's tolerance 1e-5 · max(1, max|float64 value|).  Values that are not finite must agree exactly."""
    with np.errstate(all="ignore"):
        v32, v64 = reward_values(spec, spec.seen(), X32), reward_values(spec, spec.seen(), X64)
        pairs = list(zip(v32, v64))
        if spec.sc["mode"] == STEP and v32:
            pairs.append((fold(v32, spec.terms), fold(v64, spec.terms, F64)))
    worst = 0.0
    for g, w in pairs:
        fin = np.isfinite(w)
        assert np.array_equal(g[~fin].astype(F64), w[~fin], equal_nan=True)
        if fin.any():
            worst = max(worst, float(np.abs(g[fin].astype(F64) - w[fin]).max() / (1e-5 * max(1.0, float(np.abs(w[fin]).max())))))
    return worst


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def _cmd_rows(rng, N, width, stride):
    """Command rows whose first two columns are jointly tiny (norm < 0.05) or large (> 0.7) — clear of the 0.1 and 0.3 gates; the floats
    between the rows of a strided view are NaN: a read of a wrong column poisons its env."""
    c = _f(rng, N, width)
    c[rng.random(N) < 0.4, :min(2, width)] *= F(0.01)
    rows = np.full((N, stride or width), np.nan, F)
    rows[:, :width] = c
    return rows


def needed(terms, mode, logging):
    """The arrays a term table reads or writes (what ``reward_prep`` asks for); everything else may be NULL."""
    need = {"reward", "episode_seconds"} | ({"episode_sums"} if logging else set()) if mode == STEP else {"term_out"}
    for t in terms:
        op, i, fl = t["op"], t["i"], t["flags"]
        cv = "contact.%d." % i[0]
        need |= {
            nat.GF_R_IS_ALIVE: {"terminated"}, nat.GF_R_TERMINATED: {"terminated"},
            nat.GF_R_BASE_HEIGHT: {"entity.pos"} | ({"command.%d.command" % i[0]} if fl & CMD else set()) | ({"terrain.height_field"} if fl & TERRAIN else set()),
            nat.GF_R_DOF_SIMILAR_TO_DEFAULT: {"dof_pos", "default_dof_pos"},
            nat.GF_R_LIN_VEL_Z_L2: {"entity.quat", "entity.lin_vel"}, nat.GF_R_ANG_VEL_XY_L2: {"entity.quat", "entity.ang_vel"},
            nat.GF_R_FLAT_ORIENTATION_L2: {"entity.quat"},
            nat.GF_R_BODY_ACCEL_EXP: {"entity.quat", "entity.lin_vel", "entity.ang_vel", "state.%d" % i[0]},
            nat.GF_R_ACTION_RATE_L2: {"actions", "last_actions"},
            nat.GF_R_CMD_TRACK_LIN_VEL: {"entity.quat", "entity.lin_vel", "command.%d.command" % i[0]},
            nat.GF_R_CMD_TRACK_ANG_VEL: {"entity.quat", "entity.ang_vel", "command.%d.command" % i[0]},
            nat.GF_R_STAND_STILL: {"dof_pos", "default_dof_pos", "command.%d.command" % i[0]},
            nat.GF_R_HAS_CONTACT: {cv + "contacts"}, nat.GF_R_CONTACT_FORCE: {cv + "contacts"},
            nat.GF_R_FEET_AIR_TIME: {cv + "contacts", cv + "last_air_time", cv + "current_contact_time"} | ({"command.%d.command" % i[1]} if i[1] >= 0 else set()),
            nat.GF_R_FEET_SLIDE: {cv + "contacts", cv + "link_vel"},
            nat.GF_R_EXTERNAL: {"ext.%d" % i[0]},
            nat.GF_R_GAIT_PHASE: {cv + "contacts", cv + "link_vel", "command.%d.command" % i[1]},
            nat.GF_R_FOOT_HEIGHT: {cv + "contacts", cv + "link_vel", cv + "link_pos", "command.%d.command" % i[1]},
        }[op]
    return need


def reward_spec(N, D=12, terms=(), mode=STEP, logging=1, links=(4,), cmds=((3, 0),), exts=(), rows=None, null_unneeded=False, keep=(), key=0):
    """A reward call on distinct non-zero inputs: contact views 0 … with ``links`` links, command views 0 … with ``cmds`` = (width,
    stride) (None leaves a view unbound), ext slots ``exts``."""
    rng = np.random.default_rng([N, D, key, 17])
    R = rows or max([t["row"] for t in terms] + [0]) + 1
    quat = rng.standard_normal((N, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True) if N else 1.0
    pos = np.stack([rng.uniform(-2.5, 8.5, N), rng.uniform(2.0, 11.0, N), rng.uniform(0.2, 0.7, N)], axis=1)
    arr = {"entity.pos": pos.astype(F), "entity.quat": quat.astype(F), "entity.lin_vel": _f(rng, N, 3) * F(0.5), "entity.ang_vel": _f(rng, N, 3) * F(0.5),
           "dof_pos": _f(rng, N, D), "default_dof_pos": _f(rng, D), "actions": _f(rng, N, D), "last_actions": _f(rng, N, D),
           "terminated": rng.choice(np.array([0, 0, 0, 1, 0x80, 0xFF], np.uint8), N)}
    sc = {"num_envs": N, "num_dofs": D, "mode": mode, "dt": float(rc.DT), "logging_enabled": logging}
    for v, L in enumerate(links):
        if L is None:
            continue
        big = rng.random((N, L, 1)) < 0.5   # a link presses (|f| > 3.4) or it does not (|f| < 0.27): clear of the thresholds 1 and 2
        arr["contact.%d.contacts" % v] = (_f(rng, N, L, 3) * np.where(big, F(4.0), F(0.05))).astype(F)
        arr["contact.%d.last_air_time" % v] = rng.uniform(0.05, 0.6, (N, L)).astype(F)
        arr["contact.%d.current_contact_time" % v] = rng.choice(np.array([0.0, 0.005, 0.5], F), (N, L))   # (p2 = dt + 1e-8 ≈ 0.0156)
        arr["contact.%d.link_vel" % v] = _f(rng, N, L, 3)
        arr["contact.%d.link_pos" % v] = _f(rng, N, L, 3) * F(0.2)
        sc["contact.%d.num_links" % v] = L
    for v, ws in enumerate(cmds):
        if ws is None:
            continue
        arr["command.%d.command" % v] = _cmd_rows(rng, N, *ws)
        sc["command.%d.width" % v], sc["command.%d.stride" % v] = ws
    for s in exts:
        arr["ext.%d" % s] = _f(rng, N)
    arr["state.0"] = _f(rng, N, 6)
    arr.update({"reward": _f(rng, N), "episode_sums": _f(rng, R, N), "episode_seconds": rng.uniform(0.1, 20.0, N).astype(F), "term_out": _f(rng, R, N)})
    arr["terrain.height_field"] = rc.terrain_fixture()
    sc["terrain.rows"], sc["terrain.cols"] = arr["terrain.height_field"].shape
    sc.update(TERRAIN_SC)
    null = {"term_out"} if mode == STEP else {"reward", "episode_sums", "episode_seconds"}
    if null_unneeded:
        null = (set(arr) - needed(terms, mode, logging)) - set(keep)
    return tspec("reward_step", sc, arr, terms, null)


ROWVEC_TABLE = (T(nat.GF_R_DOF_SIMILAR_TO_DEFAULT, w=-0.7), T(nat.GF_R_ACTION_RATE_L2, w=-0.013), T(nat.GF_R_STAND_STILL, w=-0.41, p=[0.3], i=[0]))
ROWVEC_D = (8, 12, 16, 20, 24, 28, 1, 4, 5, 13, 32)   # one per reward_kernel<2 … 7>, then the scalar path
P2 = float(F(rc.DT) + F(1e-8))                         # feet_air_time: (float)(dt + 1e-8)


def mixed_table():
    """Every kind of input once, no exp term."""
    return table(T(nat.GF_R_IS_ALIVE, w=0.5), T(nat.GF_R_BASE_HEIGHT, w=-3.0, p=[0.35]), T(nat.GF_R_DOF_SIMILAR_TO_DEFAULT, w=-0.1),
                 T(nat.GF_R_LIN_VEL_Z_L2, w=-2.0), T(nat.GF_R_ANG_VEL_XY_L2, w=-0.05), T(nat.GF_R_FLAT_ORIENTATION_L2, w=-1.5),
                 T(nat.GF_R_ACTION_RATE_L2, w=-0.01), T(nat.GF_R_HAS_CONTACT, w=-1.0, p=[1.0], i=[0, 2]),
                 T(nat.GF_R_FEET_AIR_TIME, w=1.25, p=[0.25, 0.0, P2], i=[0, 0]), T(nat.GF_R_TERMINATED, w=-20.0))


def full_table():
    """GF_MAX_TERMS exact terms, the repeats with other parameters and weights of mixed sign and size (the left fold rounds differently
    in another order), on rows that are a permutation of 0 … 23."""
    ts = [T(nat.GF_R_IS_ALIVE, w=0.37), T(nat.GF_R_TERMINATED, w=-17.0), T(nat.GF_R_BASE_HEIGHT, w=-31.0, p=[0.35]),
          T(nat.GF_R_BASE_HEIGHT, w=5.5, i=[1], flags=CMD), T(nat.GF_R_BASE_HEIGHT, w=-2.25, p=[0.1], flags=TERRAIN),
          T(nat.GF_R_BASE_HEIGHT, w=0.013, i=[0], flags=CMD | TERRAIN), T(nat.GF_R_DOF_SIMILAR_TO_DEFAULT, w=-0.11),
          T(nat.GF_R_LIN_VEL_Z_L2, w=-2.3), T(nat.GF_R_ANG_VEL_XY_L2, w=0.051), T(nat.GF_R_FLAT_ORIENTATION_L2, w=-1.7),
          T(nat.GF_R_ACTION_RATE_L2, w=-0.0031), T(nat.GF_R_STAND_STILL, w=0.9, p=[0.3], i=[0]), T(nat.GF_R_STAND_STILL, w=-0.29, p=[0.3], i=[1]),
          T(nat.GF_R_HAS_CONTACT, w=-1.1, p=[1.0], i=[0, 2]), T(nat.GF_R_HAS_CONTACT, w=0.77, p=[2.0], i=[1, 1]),
          T(nat.GF_R_CONTACT_FORCE, w=-0.019, p=[1.0], i=[0]), T(nat.GF_R_CONTACT_FORCE, w=0.0023, p=[2.0], i=[1]),
          T(nat.GF_R_FEET_AIR_TIME, w=1.3, p=[0.25, 0.0, P2], i=[0, -1]), T(nat.GF_R_FEET_AIR_TIME, w=-0.6, p=[0.25, 0.2, P2], i=[1, -1], flags=MAX),
          T(nat.GF_R_FEET_AIR_TIME, w=2.9, p=[0.1, 0.0, P2], i=[0, 0]), T(nat.GF_R_FEET_SLIDE, w=-0.043, i=[1]),
          T(nat.GF_R_EXTERNAL, w=0.61, i=[3]), T(nat.GF_R_EXTERNAL, w=-7.1, i=[15]), T(nat.GF_R_DOF_SIMILAR_TO_DEFAULT, w=0.0007)]
    assert len(ts) == nat.GF_MAX_TERMS
    return table(*ts, rows=[(5 * k + 3) % 24 for k in range(24)])


FULL = dict(links=(4, 7), cmds=((3, 0), (5, 8)), exts=(3, 15))
REWARD, TERMINATION, ROTATE, EXP = {}, {}, {}, {}

for _n in SIZES:
    REWARD["size_%d" % _n] = functools.partial(reward_spec, _n, D=12 if _n < 4097 else 28, terms=mixed_table())
for _d in ROWVEC_D:
    for _n in (65, 130):
        REWARD["rowvec_D%d_N%d" % (_d, _n)] = functools.partial(reward_spec, _n, D=_d, terms=table(*ROWVEC_TABLE))


def _misaligned(n, which):
    s = reward_spec(n, D=12, terms=table(*ROWVEC_TABLE), key=3)
    s.offs[which] = 1   # one float past a 16-byte boundary: rows16 is false, reward_kernel<0>
    return s


for _w in ("dof_pos", "actions", "last_actions"):
    for _n in (65, 130):
        REWARD["rowvec_D12_%s_off1_N%d" % (_w, _n)] = functools.partial(_misaligned, _n, _w)

# needs nothing / one need bit: every pointer the table does not need is NULL, so gsel() sends those loads to the zero pad
NEED_TABLES = {
    "nothing": [T(nat.GF_R_IS_ALIVE, w=0.5)], "POS": [T(nat.GF_R_BASE_HEIGHT, w=-3.0, p=[0.35])], "QUAT_LIN": [T(nat.GF_R_LIN_VEL_Z_L2, w=-2.0)],
    "QUAT_ANG": [T(nat.GF_R_ANG_VEL_XY_L2, w=-0.05)], "QUAT_GRAV": [T(nat.GF_R_FLAT_ORIENTATION_L2, w=-1.5)],
    "DOF_DEV": [T(nat.GF_R_DOF_SIMILAR_TO_DEFAULT, w=-0.1)], "ACT_RATE": [T(nat.GF_R_ACTION_RATE_L2, w=-0.01)],
    "TERMINATED": [T(nat.GF_R_TERMINATED, w=-20.0)], "CMD0": [T(nat.GF_R_FEET_AIR_TIME, w=1.25, p=[0.25, 0.0, P2], i=[0, 0])],
}
for _k, _t in NEED_TABLES.items():
    for _d in (12, 28):
        REWARD["needs_%s_D%d" % (_k, _d)] = functools.partial(reward_spec, 65, D=_d, terms=table(*_t), null_unneeded=True, key=5)

ROWS = (7, 0, 23, 3, 11)
ROWS_TABLE = (T(nat.GF_R_BASE_HEIGHT, w=-3.0, p=[0.35]), T(nat.GF_R_IS_ALIVE, w=0.5), T(nat.GF_R_ACTION_RATE_L2, w=-0.01),
              T(nat.GF_R_LIN_VEL_Z_L2, w=-2.0), T(nat.GF_R_CONTACT_FORCE, w=-0.02, p=[1.0], i=[0]))
REWARD["rows_step"] = functools.partial(reward_spec, 130, terms=table(*ROWS_TABLE, rows=ROWS), rows=24)
REWARD["rows_eval"] = functools.partial(reward_spec, 130, terms=table(*ROWS_TABLE, rows=ROWS), rows=24, mode=EVAL)
REWARD["full_table"] = functools.partial(reward_spec, 130, terms=full_table(), **FULL)
REWARD["full_table_eval"] = functools.partial(reward_spec, 65, terms=full_table(), mode=EVAL, **FULL)
REWARD["logging_off"] = functools.partial(reward_spec, 130, terms=mixed_table(), logging=0, null_unneeded=True, keep=("episode_sums",), key=1)
REWARD["logging_off_sums_null"] = functools.partial(reward_spec, 130, terms=mixed_table(), logging=0, null_unneeded=True, key=1)

CMD_SHAPES = ((1, 0), (2, 0), (3, 0), (3, 8), (5, 5))


def _cmd_table(view, width):
    ts = [T(nat.GF_R_BASE_HEIGHT, w=-3.0, i=[view], flags=CMD)]
    if width >= 2:
        ts += [T(nat.GF_R_STAND_STILL, w=-0.41, p=[0.3], i=[view]), T(nat.GF_R_FEET_AIR_TIME, w=1.25, p=[0.25, 0.0, P2], i=[0, view])]
    return table(*ts)


for _w, _s in CMD_SHAPES:
    REWARD["cmd_view0_w%d_s%d" % (_w, _s)] = functools.partial(reward_spec, 130, terms=_cmd_table(0, _w), cmds=((_w, _s),), key=7)
    REWARD["cmd_view2_w%d_s%d" % (_w, _s)] = functools.partial(reward_spec, 130, terms=_cmd_table(2, _w), cmds=(None, None, (_w, _s)), key=7)

LINKS = (1, 3, 4, 5, 8, 9, 17)   # around the four-link passes of link_rows4
for _l in LINKS:
    REWARD["links_%d" % _l] = functools.partial(
        reward_spec, 130, links=(_l,), key=9,
        terms=table(T(nat.GF_R_HAS_CONTACT, w=-1.0, p=[1.0], i=[0, (_l + 1) // 2]), T(nat.GF_R_CONTACT_FORCE, w=-0.02, p=[2.0], i=[0]),
                    T(nat.GF_R_FEET_SLIDE, w=-0.04, i=[0]), T(nat.GF_R_FEET_AIR_TIME, w=1.25, p=[0.25, 0.2, P2], i=[0, -1], flags=MAX)))


def _terrain(where, field=True):
    s = reward_spec(130, terms=table(T(nat.GF_R_BASE_HEIGHT, w=-3.0, p=[0.3], flags=TERRAIN), T(nat.GF_R_BASE_HEIGHT, w=1.0, i=[0], flags=TERRAIN | CMD)), key=11)
    edge = np.array([0.0, 1.0 - 2.0 ** -24, 0.5, 2.0 ** -24, 1.0, 0.25, 0.999], F)
    if where == "border":     # on the first / last column and row, at and next to cell corners
        s.arr["entity.pos"][:, 0] = np.resize(edge, 130) * F(12.0) + F(-3.0)
        s.arr["entity.pos"][:, 1] = np.resize(np.repeat(edge, 7), 130) * F(10.0) + F(1.5)
    elif where == "outside":  # the index is clipped to the border
        rng = np.random.default_rng(130)
        s.arr["entity.pos"][:, 0] = rng.choice(np.array([-9.0, -3.5, 9.5, 40.0], F), 130)
        s.arr["entity.pos"][:, 1] = rng.choice(np.array([-2.0, 1.0, 12.0, 99.0, 5.0], F), 130)
    if not field:
        s.null.add("terrain.height_field")
    return s


for _k in ("inside", "border", "outside"):
    REWARD["terrain_" + _k] = functools.partial(_terrain, _k)
REWARD["terrain_no_field"] = functools.partial(_terrain, "inside", field=False)
REWARD["external_slots_3_15"] = functools.partial(reward_spec, 130, exts=(3, 15), terms=table(T(nat.GF_R_EXTERNAL, w=0.61, i=[15]), T(nat.GF_R_EXTERNAL, w=-7.1, i=[3])))
REWARD["envs_0"] = functools.partial(reward_spec, 0, terms=mixed_table())
REWARD["terms_0"] = functools.partial(reward_spec, 130, terms=())
REWARD["shard_whole"] = functools.partial(reward_spec, 130, D=16, terms=full_table(), **FULL)


# ---- the exp terms: one EVAL case each ----------------------------------------------------------------------------------------------------
EXACT_ROWS = 8   # envs 1 … 8 hold the exact rows (env 0 carries the gait quirk), alternately "argument 0" and "argument overflows"


def _exp_rows():
    zero_arg = np.arange(1, 1 + EXACT_ROWS, 2)
    return zero_arg, zero_arg + 1


def exp_track_lin():
    """CMD_TRACK_LIN_VEL on view 0 (the cmd0 registers) and on view 1 (memory): command == body velocity, and 1e30 away from it."""
    s = reward_spec(130, mode=EVAL, cmds=((3, 0), (3, 8)), key=21, terms=table(T(nat.GF_R_CMD_TRACK_LIN_VEL, p=[4.0], i=[0]), T(nat.GF_R_CMD_TRACK_LIN_VEL, p=[8.0], i=[1])))
    z, o = _exp_rows()
    b = rot_inv(s.arr["entity.quat"], s.arr["entity.lin_vel"])
    for v in (0, 1):
        s.arr["command.%d.command" % v][z, 0:2] = b[z, 0:2]
        s.arr["command.%d.command" % v][o, 0] = F(1e30)
    return s, {0: (z, 1.0, o, 0.0), 1: (z, 1.0, o, 0.0)}


def exp_track_ang():
    s = reward_spec(130, mode=EVAL, cmds=((3, 0), (5, 5)), key=22, terms=table(T(nat.GF_R_CMD_TRACK_ANG_VEL, p=[4.0], i=[0, 2]), T(nat.GF_R_CMD_TRACK_ANG_VEL, p=[8.0], i=[1, 4])))
    z, o = _exp_rows()
    b = rot_inv(s.arr["entity.quat"], s.arr["entity.ang_vel"])
    s.arr["command.0.command"][z, 2], s.arr["command.1.command"][z, 4] = b[z, 2], b[z, 2]
    s.arr["command.0.command"][o, 2], s.arr["command.1.command"][o, 4] = F(1e30), F(-1e30)
    return s, {0: (z, 1.0, o, 0.0), 1: (z, 1.0, o, 0.0)}


def _gait_views(s, key):
    """Command view 1 = the gait manager's 16-float rows (width 14), contact view 0 = five links of which rows 4, 0, 2, 1 are the feet."""
    g = rc.consistent_flags(rc.gait_spec(130, key=key))
    s.arr["command.1.command"] = g.arr["state"].copy()
    s.sc["command.1.width"], s.sc["command.1.stride"] = GAIT_OBS_WIDTH, GAIT_ROW
    flags = g.arr["wave_flags"].copy()
    flags[(130 + 63) // 64:] = 0   # the host pads the bytes with zeros to whole 32-bit words
    return flags


FEET = 4 | (0 << 8) | (2 << 16) | (1 << 24)


def exp_gait_phase():
    """GAIT_PHASE with the env-0 quirk on: feet at rest (every norm 0, argument ±0) and the active quantity of every foot infinite
    (force in swing, speed in stance; the other stays finite, so no 0 · inf)."""
    s = reward_spec(130, mode=EVAL, links=(5,), cmds=((3, 0),), key=23, terms=table(T(nat.GF_R_GAIT_PHASE, p=[0.0, float(rc.TWO_PI), float(F(0.5) * rc.TWO_PI)], i=[0, 1, FEET])))
    s.arr["gait_wave_flags"] = _gait_views(s, 23)
    s.arr["contact.0.contacts"] *= F(0.02)   # arguments of a few units, not of hundreds
    s.arr["contact.0.link_vel"] *= F(0.3)
    z, o = _exp_rows()
    s.arr["contact.0.contacts"][z], s.arr["contact.0.link_vel"][z] = 0, 0
    st = s.arr["command.1.command"]
    fl = rc.foot_flags(st[:, 15], st[:, 0:4], rc.TWO_PI)
    for k in range(4):
        l = (FEET >> (8 * k)) & 0xFF
        assert (((fl[o] >> (2 * k)) & 3) != 0).all()   # every foot is in one half of its cycle
        swing = ((fl[o] >> (2 * k)) & 1) != 0
        s.arr["contact.0.contacts"][o[swing], l, 0] = np.inf
        s.arr["contact.0.link_vel"][o[~swing], l, 0] = np.inf
    return s, {0: (z, 1.0, o, 0.0)}


def exp_foot_height():
    s = reward_spec(130, mode=EVAL, links=(5,), cmds=((3, 0),), key=24, terms=table(T(nat.GF_R_FOOT_HEIGHT, p=[2.0], i=[0, 1, FEET])))
    _gait_views(s, 24)
    s.arr["command.1.command"][:, 4] = np.random.default_rng(24).uniform(0.05, 0.12, 130).astype(F)
    z, o = _exp_rows()
    for k in range(4):
        l = (FEET >> (8 * k)) & 0xFF
        s.arr["contact.0.link_pos"][z, l, 2] = s.arr["command.1.command"][z, 4]
    s.arr["contact.0.link_pos"][o, 4, 2] = F(1e30)
    return s, {0: (z, 1.0, o, 0.0)}


def exp_body_accel():
    """Two consecutive launches on the same state rows: FIRST_CALL (no acceleration: 1 − exp(−0) = 0 in every env), then the real one —
    envs whose velocities did not change (argument 0, value 0) and envs whose velocity jumped by 1e30 (|a|² overflows: value 1)."""
    s = reward_spec(130, mode=EVAL, key=25, terms=table(T(nat.GF_R_BODY_ACCEL_EXP, p=[0.1], i=[0], flags=FIRST)))
    z, o = _exp_rows()
    rng = np.random.default_rng(25)
    lin2, ang2 = s.arr["entity.lin_vel"] + _f(rng, 130, 3) * F(0.05), s.arr["entity.ang_vel"] + _f(rng, 130, 3) * F(0.05)
    lin2[z], ang2[z] = s.arr["entity.lin_vel"][z], s.arr["entity.ang_vel"][z]
    lin2[o, 0] = F(1e30)
    return s, {0: (np.arange(130), 0.0, np.arange(0), 1.0)}, dict(lin_vel=lin2.astype(F), ang_vel=ang2.astype(F)), {0: (z, 0.0, o, 1.0)}


def second_call(spec, want, new):
    """The spec of the launch that follows ``spec`` on the same buffers: its outputs as inputs, new velocities, FIRST_CALL cleared."""
    arr = {k: (spec.arr[k] if want.get(k) is None else want[k]).copy() for k in spec.arr}
    arr["entity.lin_vel"], arr["entity.ang_vel"] = new["lin_vel"], new["ang_vel"]
    s = with_arrays(spec, arr)
    s.terms = [dict(t, flags=t["flags"] & ~FIRST) for t in spec.terms]
    return s


EXP = {"track_lin_vel": exp_track_lin, "track_ang_vel": exp_track_ang, "gait_phase": exp_gait_phase, "foot_height": exp_foot_height, "body_accel": exp_body_accel}


def ulp_distance(got, want64):
    """|got − want| in units of the float32 spacing at want, for finite rows."""
    w32 = want64.astype(F)
    fin = np.isfinite(want64) & np.isfinite(got)
    return np.abs(got[fin].astype(F64) - want64[fin]) / np.spacing(np.maximum(np.abs(w32[fin]), np.finfo(F).tiny)).astype(F64)


# ---- termination cases -------------------------------------------------------------------------------------------------------------------------
SIN30 = float(F(0.5))
EIGHT = (T(nat.GF_T_TIMEOUT, flags=TIME_OUT), T(nat.GF_T_BAD_ORIENTATION, p=[SIN30, float(np.arcsin(F(0.5)))], i=[10]), T(nat.GF_T_BASE_HEIGHT_BELOW, p=[0.25]),
         T(nat.GF_T_OUT_OF_BOUNDS, p=[-2.0, 2.0, -1.5, 1.5]), T(nat.GF_T_HAS_CONTACT, p=[1.0], i=[0, 1]), T(nat.GF_T_CONTACT_FORCE, p=[1.0], i=[3]),
         T(nat.GF_T_CONTACT_FORCE_GRACE, p=[2.0], i=[3, 10]), T(nat.GF_T_EXTERNAL, flags=TIME_OUT, i=[15]))
TAIL_TERM = 2   # BASE_HEIGHT_BELOW fires in the tail-adjacent envs only


def tail_envs(N):
    return sorted({N - 1, 64 * ((N - 1) // 64)}) if N else []


def termination_spec(N, terms=EIGHT, key=0, null=(), stats=True):
    """Every term fires on a subset of its own (drawn independently, so the ORs are not any one term's mask); BASE_HEIGHT_BELOW fires
    in env N − 1 and in the first env of the last wave only.  Probe values: tilt 5° or 60° against 30°, heights 0.1 | 0.4 against 0.25,
    x, y within ±1 or at ±5 against ±2 / ±1.5, forces of 0.1 or 10 against 1 and 2, episode lengths 5 beyond either side of the limit
    and 3 against a grace of 10."""
    rng = np.random.default_rng([N, key, 19])
    hit = lambda p: rng.random(N) < p
    grace = hit(0.2)
    max_len = rng.integers(900, 1100, N).astype(np.int32)
    ep = np.where(hit(0.3), max_len + 5, max_len - 5).astype(np.int32)
    ep[grace] = 3
    ang = np.where(hit(0.3), np.radians(60.0), np.radians(5.0)) * rng.choice([-1.0, 1.0], N)
    yaw = rng.uniform(-3.0, 3.0, N)
    axis = rng.uniform(0.0, 2 * np.pi, N)
    # tilt by `ang` about a horizontal axis, then any yaw: the projected gravity's xy norm is sin|ang|
    tilt = np.stack([np.cos(ang / 2), np.sin(ang / 2) * np.cos(axis), np.sin(ang / 2) * np.sin(axis), np.zeros(N)], axis=1)
    yq = np.stack([np.cos(yaw / 2), np.zeros(N), np.zeros(N), np.sin(yaw / 2)], axis=1)
    w1, x1, y1, z1 = yq.T
    w2, x2, y2, z2 = tilt.T
    quat = np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=1)
    pos = np.stack([rng.uniform(-1.0, 1.0, N), rng.uniform(-1.0, 1.0, N), np.full(N, 0.4)], axis=1)
    oob = hit(0.25)
    pos[oob, rng.integers(0, 2, int(oob.sum()))] = rng.choice([-5.0, 5.0], int(oob.sum()))
    pos[np.array(tail_envs(N), np.int64), 2] = 0.1
    c0 = _f(rng, N, 1, 3) * np.where(hit(0.3), F(4.0), F(0.03))[:, None, None]
    c3 = _f(rng, N, 5, 3) * F(0.03)
    press = np.nonzero(hit(0.35))[0]
    c3[press, press % 5] *= F(130.0)   # one link of five presses
    arr = {"entity.pos": pos.astype(F), "entity.quat": quat.astype(F), "episode_length": ep, "max_episode_length": max_len,
           "contact.0.contacts": c0.astype(F), "contact.3.contacts": c3.astype(F), "ext.15": rng.choice(np.array([0, 0, 0, 1, 0x80], np.uint8), N),
           "ext.2": rng.choice(np.array([0, 0, 1, 0xFF], np.uint8), N),
           "terminated": np.full(N, 0x5A, np.uint8), "truncated": np.full(N, 0x5A, np.uint8), "term_out": np.full((max(1, len(terms)), N), 0x5A, np.uint8)}
    if N:
        arr["ext.15"][0], arr["ext.2"][0] = 1, 0xFF   # env 0 fires: the tail lanes of the last wave are clamped to it and must not vote
    sc = {"num_envs": N, "contact.0.num_links": 1, "contact.3.num_links": 5}
    return tspec("termination_step", sc, arr, table(*terms), null, stats=stats)


SIXTEEN = EIGHT + (T(nat.GF_T_BAD_ORIENTATION, p=[float(F(0.3)), float(np.arcsin(F(0.3)))], i=[2]), T(nat.GF_T_BASE_HEIGHT_BELOW, p=[0.5]),
                   T(nat.GF_T_OUT_OF_BOUNDS, p=[-6.0, 0.0, -6.0, 6.0], flags=TIME_OUT), T(nat.GF_T_HAS_CONTACT, p=[1.0], i=[3, 2]),
                   T(nat.GF_T_CONTACT_FORCE, p=[2.0], i=[0]), T(nat.GF_T_CONTACT_FORCE_GRACE, p=[1.0], i=[0, 1200]), T(nat.GF_T_EXTERNAL, i=[2]),
                   T(nat.GF_T_TIMEOUT))
for _n in SIZES:
    TERMINATION["size_%d" % _n] = functools.partial(termination_spec, _n)
TERMINATION["term_out_null"] = functools.partial(termination_spec, 130, null=("term_out",))
TERMINATION["stats_null"] = functools.partial(termination_spec, 130, stats=False)
TERMINATION["max_length_null"] = functools.partial(termination_spec, 130, null=("max_episode_length",))
TERMINATION["max_length_and_length_null"] = functools.partial(
    termination_spec, 130, terms=(EIGHT[0], EIGHT[2], EIGHT[3], EIGHT[4], EIGHT[7]), null=("max_episode_length", "episode_length", "entity.quat", "contact.3.contacts"))
TERMINATION["terms_16"] = functools.partial(termination_spec, 130, terms=SIXTEEN)
TERMINATION["terms_16_4097"] = functools.partial(termination_spec, 4097, terms=SIXTEEN)
TERMINATION["terms_0"] = functools.partial(termination_spec, 130, terms=())
TERMINATION["envs_0"] = functools.partial(termination_spec, 0)


# ---- rotate cases ----------------------------------------------------------------------------------------------------------------------------
NAN_ENV = 2


def rotate_spec(N, what, key=0):
    """Random unit quaternions; env 0 has norm 0.5 at every size, env 1 is the identity, env ``NAN_ENV`` holds a NaN, and the last
    three envs (the partial last wave) have norm 3, the zero quaternion and the identity; ``out`` starts one float past a 16-byte
    boundary."""
    rng = np.random.default_rng([N, what, key, 23])
    q = rng.standard_normal((N, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    one, zero = [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]
    # env 0 (every size, N = 1 too) is non-unit; the last three envs put the specials into the partial last wave as well
    for n, special in ((0, 0.5), (1, one), (NAN_ENV, "nan"), (N - 1, 3.0), (N - 2, zero), (N - 3, one)):
        if 0 <= n < N and (n > NAN_ENV or special in (0.5, one, "nan")):
            if isinstance(special, float):
                q[n] *= special
            elif special == "nan":
                q[n, 1] = np.nan
            else:
                q[n] = special
    arr = {"entity.quat": q.astype(F), "entity.lin_vel": _f(rng, N, 3), "entity.ang_vel": _f(rng, N, 3), "out": _f(rng, N, 3)}
    s = tspec("entity_rotate", {"num_envs": N, "what": what}, arr, ())
    s.sc.pop("num_terms")
    s.offs["out"] = 1
    return s


for _n in SIZES:
    for _w, _name in ((nat.GF_ROT_PROJ_GRAVITY, "gravity"), (nat.GF_ROT_LIN_VEL, "lin_vel"), (nat.GF_ROT_ANG_VEL, "ang_vel")):
        ROTATE["%s_%d" % (_name, _n)] = functools.partial(rotate_spec, _n, _w)

TABLES = {"reward_step": REWARD, "termination_step": TERMINATION, "entity_rotate": ROTATE}


@functools.lru_cache(maxsize=None)
def case(fn, name):
    """(spec, arrays as the call must leave them, exact statistics) — built once, shared by the CPU and GPU tests, never modified."""
    spec = TABLES[fn][name]()
    want, stats = restate(spec)
    return spec, want, stats


# ---- running ----------------------------------------------------------------------------------------------------------------------------------
class Launch(rc.Launch):
    """``reset_cases.Launch`` plus the term table; ``check(loose=…)`` leaves the named arrays to the caller's own comparison (the
    sentinel rows behind them are still checked)."""

    def __init__(self, dev, spec):
        super().__init__(dev, spec)
        self.set_terms(getattr(spec, "terms", ()))

    def set_terms(self, terms):
        for k, t in enumerate(terms):
            d = self.args.terms[k]
            d.op, d.flags, d.w, d.row = t["op"], t["flags"], t["w"], t["row"]
            for j in range(4):
                d.p[j], d.i[j] = t["p"][j], t["i"][j]

    def upload(self, k, v):
        import torch
        self.bufs[k].t[:v.size].copy_(torch.from_numpy(np.ascontiguousarray(v).reshape(-1)))

    def check(self, want, want_stats, what="", loose=()):
        want = dict(want)
        for k in loose:
            want[k] = self.got(k)
        super().check(want, want_stats, what)


def run_case(backend, dev, fn, name):
    spec, want, stats = case(fn, name)
    l = Launch(dev, spec)
    assert l.run(backend) == 0, (fn, name)
    if fn == "entity_rotate":   # the NaN env: NaN where the restatement has NaN, no bits compared
        want = dict(want)
        got, nan = l.got("out"), np.isnan(want["out"])
        assert np.array_equal(np.isnan(got), nan), name
        want["out"] = np.where(nan, got, want["out"])
    l.check(want, stats, name)
    return l, want


def shard(spec, lo, hi):
    """Envs [lo, hi) of a reward spec as a call of their own."""
    N = spec.sc["num_envs"]
    arr = {}
    for k, v in spec.arr.items():
        if k in ("episode_sums", "term_out"):
            arr[k] = np.ascontiguousarray(v[:, lo:hi])
        elif k in ("default_dof_pos", "terrain.height_field"):
            arr[k] = v.copy()
        else:
            assert v.shape[0] == N, k
            arr[k] = np.ascontiguousarray(v[lo:hi])
    s = with_arrays(spec, arr)
    s.sc["num_envs"] = hi - lo
    return s


def sharding_identity(backend, dev):
    """The launch over [0, 130) equals launches over [0, 64) and [64, 130) on sliced buffers: first on the restatement itself, then each
    shard's call against its restatement (the whole call against its own is the table's ``shard_whole`` case)."""
    spec, want, _ = case("reward_step", "shard_whole")
    whole = with_arrays(spec, {k: (spec.arr[k] if want[k] is None else want[k]) for k in spec.arr})
    for lo, hi in ((0, 64), (64, 130)):
        part = shard(spec, lo, hi)
        w, _ = restate(part)
        expect = shard(whole, lo, hi).arr
        for k in part.arr:
            if w[k] is not None:
                assert np.array_equal(_ints(w[k]), _ints(expect[k])), f"the restatement of envs [{lo}, {hi}) differs from the whole in {k}"
        l = Launch(dev, part)
        assert l.run(backend) == 0
        l.check(w, None, f"reward shard [{lo}, {hi})")


def exp_case(backend, dev, name):
    """One exp term: every buffer but ``term_out`` bit for bit; the exact rows of ``term_out`` with ==, the others under
    1e-5 · max(1, max|float64 value|) against the float64 evaluation.  Returns the largest distance to float64 in float32 ulp."""
    built = EXP[name]()
    spec, exact = built[0], built[1]
    l = Launch(dev, spec)
    worst = 0.0
    for call in range(2 if len(built) > 2 else 1):
        if call == 1:
            spec = second_call(spec, want, built[2])
            exact = built[3]
            l.spec = spec
            l.upload("entity.lin_vel", spec.arr["entity.lin_vel"])
            l.upload("entity.ang_vel", spec.arr["entity.ang_vel"])
            l.set_terms(spec.terms)
        want, _ = restate(spec)
        with np.errstate(all="ignore"):
            v64 = reward_values(spec, spec.seen(), X64)
        assert l.run(backend) == 0, name
        l.check(want, None, f"{name}, launch {call}", loose=("term_out",))
        got = l.got("term_out")
        for k, t in enumerate(spec.terms):
            z, zv, o, ov = exact[k]
            g, w = got[t["row"]], v64[k]
            assert np.array_equal(want["term_out"][t["row"]][z], np.full(len(z), zv, F)) and np.array_equal(want["term_out"][t["row"]][o], np.full(len(o), ov, F)), "the case's own rows"
            assert np.array_equal(g[z], np.full(len(z), zv, F)), f"{name} term {k}: argument 0 must give exactly {zv}: {g[z]}"
            assert np.array_equal(g[o], np.full(len(o), ov, F)), f"{name} term {k}: an overflowing argument must give exactly {ov}: {g[o]}"
            tol = 1e-5 * max(1.0, float(np.abs(w[np.isfinite(w)]).max()))
            assert not np.isnan(g).any() and float(np.abs(g.astype(F64) - w).max()) <= tol, f"{name} term {k}: {float(np.abs(g.astype(F64) - w).max()):.3e} > {tol:.3e}"
            rest = np.setdiff1d(np.arange(len(g)), np.concatenate([z, o]))   # (an exact row's float64 argument is not exactly 0)
            d = ulp_distance(g[rest], w[rest])
            worst = max(worst, float(d.max()) if d.size else 0.0)
    return worst


# ---- chain A: [termination, reward, command(step) × k, gait(step), gait(masked)] through gf_run_ops ---------------------------------------------
CHAIN_SIZES = (65, 130, 4097)
CHAIN_D = (12, 28, 16, 5)   # chain_a_kernel<3>, <7>, <0>, <0>; unchained reward_kernel<3>, <7>, <4>, <0>
CHAIN_LISTS = {"term_reward_cmd2": "TRCC", "term_reward": "TR", "reward_cmd": "RC", "term_reward_cmd3": "TRCCC", "term_reward_gait": "TRGM"}


def chain_table():
    """IS_ALIVE / TERMINATED read the mask the termination op of the same launch writes; STAND_STILL and BASE_HEIGHT|CMD read command
    rows the command ops of the same launch resample (view 0 through the cmd0 registers, view 1 from memory in the term body)."""
    return table(T(nat.GF_R_IS_ALIVE, w=0.5), T(nat.GF_R_TERMINATED, w=-20.0), T(nat.GF_R_STAND_STILL, w=-0.41, p=[0.3], i=[0]),
                 T(nat.GF_R_BASE_HEIGHT, w=-3.0, i=[0], flags=CMD), T(nat.GF_R_STAND_STILL, w=0.23, p=[0.3], i=[1]),
                 T(nat.GF_R_BASE_HEIGHT, w=1.5, i=[1], flags=CMD), T(nat.GF_R_DOF_SIMILAR_TO_DEFAULT, w=-0.1), T(nat.GF_R_ACTION_RATE_L2, w=-0.01))


@functools.lru_cache(maxsize=None)
def chain(kind, N, D):
    """(specs, links): the ops of one list and the buffers they share — (op, name, owner op, owner's name): the op's pointer ``name``
    addresses the owner's buffer (its own buffer of that name is allocated all the same and must stay untouched)."""
    ops, specs, links = CHAIN_LISTS[kind], [], []
    t_at = ops.find("T")
    r_at = ops.find("R")
    n_cmd = ops.count("C")
    widths = (3, 5, 4)
    if t_at >= 0:
        t = termination_spec(N, key=3)
        done, _ = restate(t)
        t.arr["terminated"] = (1 - done["terminated"]).astype(np.uint8)   # a stale read flips every env
        t.arr["truncated"] = (1 - done["truncated"]).astype(np.uint8)
        specs.append(t)
    r = reward_spec(N, D=D, terms=chain_table() if n_cmd else table(*chain_table()[:2], *chain_table()[6:]), cmds=((3, 0), (5, 0)), key=31)
    specs.append(r)
    if t_at >= 0:
        links.append((r_at, "terminated", t_at, "terminated"))
    for c in range(n_cmd):
        s = command_spec(N, R=widths[c], mode=rc.CMD_STEP, steps=1, key=c)   # every env is due: a late read changes every env
        s.arr["command"][np.random.default_rng([N, c]).random(N) < 0.4, :2] *= F(0.01)   # both sides of the stand-still gate before the resample
        specs.append(s)
        if c < 2:
            links.append((r_at, "command.%d.command" % c, len(specs) - 1, "command"))
    if "G" in ops:
        g = gait_spec(N, mode=rc.CMD_STEP, steps=1)
        g.arr["state"][:, 14] = np.resize(np.array([0.1, 0.45, 0.7, 1.3, 2.9], F), N)   # reset_cases' step_all_due
        # only the last env is reset, so only the last block holds a reset env: in the chain gait.step leaves every byte alone and the
        # masked launch must take over ALL of them (the deferred hand-over); without it the other blocks keep the bytes they had
        m = gait_spec(N, mode=rc.CMD_MASKED, mask="last", key=1)
        m.flags_all = True   # every block's byte is recomputed from the post-step rows, chained or not
        specs += [g, m]
        gi = len(specs) - 2
        links += [(gi + 1, k, gi, k) for k in ("state", "selected", "wave_flags")]
    return specs, links


def chain_restate(specs, links):
    """The ops applied in sequence: [(arrays each launch's own buffers must hold at the end, statistics)]."""
    store = {(i, k): v.copy() for i, s in enumerate(specs) for k, v in s.arr.items()}
    stats = []
    for i, s in enumerate(specs):
        src = {k: (oi, ok) for (di, k, oi, ok) in links if di == i}
        logical = with_arrays(s, {k: store[src.get(k, (i, k))] for k in s.arr}) if hasattr(s, "terms") else rc.Spec(s.fn, s.sc, {k: store[src.get(k, (i, k))] for k in s.arr}, s.null, s.stats)
        logical.flags_all = s.flags_all
        out, st = restate(logical, s.flags_all)
        for k, v in out.items():
            if v is not None:
                store[src.get(k, (i, k))] = v
        stats.append(st)
    return [({k: store[(i, k)] for k in s.arr}, stats[i]) for i, s in enumerate(specs)]


def chain_launches(dev, specs, links):
    ls = []
    for i, s in enumerate(specs):
        phys = with_arrays(s, s.arr) if hasattr(s, "terms") else rc.Spec(s.fn, s.sc, s.arr, s.null, s.stats)
        phys.null = set(s.null) | {k for (di, k, _oi, _ok) in links if di == i}   # (its own buffer: allocated, never addressed)
        ls.append(Launch(dev, phys))
    for di, k, oi, ok in links:
        rc._set(ls[di].args, k, ls[oi].bufs[ok].ptr)
    return ls


def run_chain(backend, dev, kind, N, D):
    specs, links = chain(kind, N, D)
    wants = chain_restate(specs, links)
    for option in (1, 0):
        if backend.name == "hip":
            backend.set_option(nat.GF_OPT_CHAIN, option)
        try:
            ls = chain_launches(dev, specs, links)
            assert rc.run_ops(backend, ls) == (0, -1)
        finally:
            if backend.name == "hip":
                backend.set_option(nat.GF_OPT_CHAIN, 1)
        for i, (l, (w, st)) in enumerate(zip(ls, wants)):
            l.check(w, st, f"op {i} ({l.spec.fn}) of {kind}, chain option {option}, {N} envs, {D} dofs")
        if backend.name != "hip":
            break
