"""gf_observe restated in numpy, a model of the kernel's dispatch, and the cases that pin the kernel at its plan, gather, write-out
and history edges.

The restatement is written from the reference's managers/observation_manager.py:218-256 (per item: the value, ``*= scale`` when
``scale != 1``, ``+= uniform_(-1, 1) * noise`` when ``noise != 0``, ``torch.cat``; the history list is newest first) and
mdp/observations.py (the getters: [N, w] rows, ``torch.norm(contacts, dim=-1)``, the body-frame vectors of
managers/entity_manager.py:130-146, which rotate by the quaternion cached BEFORE this tick's reset, :189-195), not from the kernel.
It works on whole [N, w] arrays item by item, as the reference does.  ``restate_frame`` takes the number type: float32 is one
rounding per operation in the documented order (``uniform_(lo, hi)`` is ``u * (hi - lo) + lo``, the norm is the fused chain of
``norm3``: term_reward_cases.fma32), float64 is the same formulas on the same float32 inputs.  The draws are not the reference's
(torch's generator) but this project's: Philox words by GLOBAL env id and frame column (tests/philox.py), or the dense ``noise_draws``
array indexed [n, column].

``dispatch`` is a model of the paths a descriptor takes through ``observe_body`` (csrc/gf_observe.hip) and the history helpers
(csrc/gf_obs_hist.h), one record per tile shape.  It exists for COVERAGE assertions only — which case reaches which edge — and is
never the expected result of anything.

``Launch`` puts a case on guarded buffers (tests/guarded.py) of either backend: every buffer is a slice of a sentinel-filled
allocation with 64 floats of guard in front, ``PAD_ROWS`` sentinel rows behind it and the requested misalignment; the sources are
compared byte for byte after every call, the outputs float for float on integer views.  Sources of copied and scale-only items hold
integers (a dropped or shifted column is off by at least 1); sources of noisy items, contact forces and velocities hold |v| <= 4.
A history case that is not a ring runs three calls on two buffers used in turn, so a case that misaligns only one of ``obs`` /
``prev_obs`` takes the other history path in its second call (``dispatch`` describes the first)."""
import collections
import functools
import re
import zlib

import numpy as np

import philox
from term_reward_cases import F, F64, X32, X64, gravity, rot_inv

PAD_ROWS = 64
SENTINEL = np.uint32(0xA5A5A5A5)
SIZES = (1, 63, 64, 65, 129)

# the constants of the kernel the model is written from (tests/test_observe_edges.py holds each against the binding or the sources)
K = dict(ENV_BLOCK=64, OBS_BLOCK=256, GATHER=8, PLAN_UNITS=48, PLAN_OWNERS=8, HIST_SHIFT=8, MIXED_UNITS=5, CHAIN_OBS=2,
         MAX_ITEMS=24, MAX_WIDTH=256, MAX_EXT=16, MAX_COMMAND_VIEWS=4, MAX_CONTACT_VIEWS=4)
K_SOURCES = {   # constant -> (file under genesis-forge_amd/csrc, the text that defines it)
    "ENV_BLOCK": ("gf_launch.h", r"kEnvBlock = (\d+)"), "OBS_BLOCK": ("gf_obs_hist.h", r"kObsBlock = (\d+)"),
    "GATHER": ("gf_observe.hip", r"kObsGather = (\d+)"), "PLAN_UNITS": ("gf_observe.hip", r"kPlanUnits = (\d+)"),
    "PLAN_OWNERS": ("gf_observe.hip", r"kPlanOwners = (\d+)"), "HIST_SHIFT": ("gf_obs_hist.h", r"kObsShift = (\d+)"),
    "MIXED_UNITS": ("gf_obs_hist.h", r"constexpr int kU = (\d+)"), "CHAIN_OBS": ("gf_chain.hip", r"kChainObs = (\d+)")}
K_NATIVE = {"MAX_ITEMS": "GF_MAX_OBS_ITEMS", "MAX_WIDTH": "GF_MAX_OBS_WIDTH", "MAX_EXT": "GF_MAX_EXT",
            "MAX_COMMAND_VIEWS": "GF_MAX_COMMAND_VIEWS", "MAX_CONTACT_VIEWS": "GF_MAX_CONTACT_VIEWS"}

ROW_KINDS = ("dof_pos", "dof_vel", "dof_force", "actions", "raw")
BODY_KINDS = ("ang", "lin", "grav")
ROW_FIELD = {"dof_pos": "dof_pos", "dof_vel": "dof_vel", "dof_force": "dof_force", "actions": "targets", "raw": "env_actions"}

Item = collections.namedtuple("Item", "kind width scale noise stride off src")


def it(kind, width=None, scale=1.0, noise=0.0, stride=0, off=0):
    """One observation item.  ``width``: columns (DOF rows default to D, fixed-width kinds to their width); ``stride``: a command view's
    row stride (0 = dense); ``off``: floats of misalignment of an item-owned source (ext, cmd, norm)."""
    fixed = {"base_pos": 3, "base_quat": 4, "ang": 3, "lin": 3, "grav": 3}
    return Item(kind, fixed.get(kind, width), float(scale), float(noise), stride, off, None)


class Case:
    def __init__(self, name, n, items, D=12, H=1, ring=(), ring_slots=0, off=None, noise="philox", env_offset=0, stale=None, calls=None, data=None):
        self.name, self.n, self.D, self.H = name, n, D, H
        self.ring, self.ring_slots = tuple(ring), ring_slots     # ring: history_ring of each call (empty: no ring)
        self.off = dict(off or {})                               # buffer name -> floats of misalignment ("obs", "prev_obs", "dof_pos", …)
        self.noise, self.env_offset, self.stale = noise, env_offset, stale   # stale: None or (kind of stale_mask, kind of stale_mask2)
        self.seed, self.stream, self.data = 0x1234567887654321, (3 << 40) | 77, data
        slots = {"ext": 0, "cmd": 0, "norm": 0}
        self.items = []
        for x in items:
            w = x.width if x.width is not None else D
            src = x.kind
            if x.kind in slots:
                src = "%s.%d" % (x.kind, slots[x.kind])
                slots[x.kind] += 1
            self.items.append(x._replace(width=w, src=src))
        assert slots["ext"] <= K["MAX_EXT"] and slots["cmd"] <= K["MAX_COMMAND_VIEWS"] and slots["norm"] <= K["MAX_CONTACT_VIEWS"]
        assert 0 < len(self.items) <= K["MAX_ITEMS"]
        self.O = sum(x.width for x in self.items)
        assert 0 < self.O < K["MAX_WIDTH"]
        self.slots = (ring_slots or H) if self.ring else H
        self.calls = calls if calls is not None else (len(self.ring) if self.ring else (3 if H > 1 else 1))
        self.family = name.split("-")[0]

    # ---- geometry of the sources ---------------------------------------------------------------------------------------------------
    def stride_of(self, x):
        if x.kind == "ext":
            return x.width
        if x.kind == "cmd":
            return x.stride or x.width
        if x.kind == "norm":
            return 3 * x.width
        return {"base_pos": 3, "base_quat": 4}.get(x.kind, self.D)

    def off_of(self, name):
        for x in self.items:
            if x.src == name and x.kind in ("ext", "cmd", "norm"):
                return x.off
        return self.off.get(name, 0)

    def buffer_of(self, x):
        return {"base_pos": "pos", "base_quat": "quat"}.get(x.kind, x.src)

    def exact_columns(self):
        """Columns that are a copy or a copy times one scale: the kernel must give the float32 restatement's bits."""
        m, col = np.zeros(self.O, bool), 0
        for x in self.items:
            m[col:col + x.width] = x.kind not in BODY_KINDS + ("norm",) and x.noise == 0.0
            col += x.width
        return m

    def needs_body(self):
        return any(x.kind in BODY_KINDS for x in self.items)

    # ---- inputs ----------------------------------------------------------------------------------------------------------------------
    @functools.lru_cache(maxsize=None)
    def inputs(self, call=0):
        """name -> array, as call ``call`` finds them.  Every float source but the quaternions moves by 1 per call: a new frame each call."""
        if self.data is not None:   # a hand-written case: the same arrays every call
            return self.data
        n = self.n
        rng = np.random.default_rng(zlib.crc32(self.name.encode()))
        d, soft = {}, set()
        for x in self.items:
            if x.noise != 0.0 or x.kind == "norm":
                soft.add(self.buffer_of(x))
        shapes = {}
        for x in self.items:
            if x.kind in BODY_KINDS:
                continue
            shapes[self.buffer_of(x)] = (n, self.stride_of(x))
        for k, name in enumerate(sorted(shapes)):
            shape = shapes[name]
            if name == "quat":
                continue
            if name in soft:
                d[name] = rng.uniform(-2.0, 2.0, shape).astype(F)
            else:   # distinct integers: neighbours in a row differ by 7, buffers by a multiple of 131
                i = np.arange(shape[0] * shape[1], dtype=np.int64).reshape(shape)
                d[name] = ((i * 7 + k * 131) % 4093 - 2046).astype(F)
            d[name] = d[name] + F(call)
        if self.needs_body() or "quat" in shapes:
            q = rng.standard_normal((n, 4))
            d["quat"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)   # normalised on the host
        if self.needs_body():
            d["lin"] = rng.uniform(-2.0, 2.0, (n, 3)).astype(F) + F(call)
            d["ang"] = rng.uniform(-2.0, 2.0, (n, 3)).astype(F) + F(call)
            if self.stale is not None:
                q = rng.standard_normal((n, 4))
                d["stale_quat"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)
                for key, kind in zip(("stale_mask", "stale_mask2"), self.stale):
                    if kind is not None:
                        d[key] = _mask(rng, n, kind)
        if self.noise == "dense" and any(x.noise != 0.0 for x in self.items):
            d["noise_draws"] = rng.random((n, self.O)).astype(F)
        for v in d.values():
            v.setflags(write=False)
        return d

    def prev0(self):
        """What the first call of a history case finds in ``prev_obs``: integers, no two neighbours alike."""
        i = np.arange(self.n * self.H * self.O, dtype=np.int64)
        return ((i * 3) % 8191 - 4000).astype(F).reshape(self.n, self.H, self.O)


def _mask(rng, n, kind):
    m = np.zeros(n, np.uint8)
    if kind == "ones":
        m[:] = 1
    elif kind == "mixed":   # every byte value counts as set; env 0 and the last env differ between the two masks of a case
        r = rng.random(n)
        m[r < 0.3] = 1
        m[(r >= 0.3) & (r < 0.4)] = 0x80
        m[int(rng.integers(0, n))] = 0xFF
    else:
        assert kind == "zeros", kind
    return m


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def draws_of(case, d, col, width, call):
    """u of columns [col, col + width) of every env: the dense array, or Philox by global env id and column."""
    if "noise_draws" in d:
        return d["noise_draws"][:, col:col + width]
    genv = ((np.arange(case.n, dtype=np.uint64) + np.uint64(case.env_offset)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return philox.uniform_ids(case.seed, case.stream + call, genv, width, first_col=col)


def restate_frame(case, call, X):
    """[n, O] of number type ``X.dt``: observation_manager.py:232-256."""
    d = case.inputs(call)
    n = case.n
    quat = None
    if case.needs_body():   # entity_manager.py:189-195: the quaternion cached before this tick's reset, for the envs it reset
        quat = d["quat"]
        if "stale_quat" in d:
            m = np.zeros(n, bool)
            for key in ("stale_mask", "stale_mask2"):
                if key in d:
                    m |= d[key] != 0
            quat = np.where(m[:, None], d["stale_quat"], quat)
        quat = X.arr(quat)
    cols, col = [], 0
    for x in case.items:
        if x.kind == "ang":
            v = rot_inv(quat, X.arr(d["ang"]))
        elif x.kind == "lin":
            v = rot_inv(quat, X.arr(d["lin"]))
        elif x.kind == "grav":
            v = gravity(quat)
        elif x.kind == "norm":   # torch.norm(contacts, dim=-1)
            c = X.arr(d[x.src]).reshape(n, x.width, 3)
            v = X.norm3(c[:, :, 0], c[:, :, 1], c[:, :, 2])
        else:
            v = X.arr(d[case.buffer_of(x)][:, :x.width])
        v = np.array(v, X.dt)
        if x.scale != 1.0:
            v = v * X(x.scale)
        if x.noise != 0.0:
            u = X.arr(draws_of(case, d, col, x.width, call))
            v = v + (u * (X.dt(1.0) - X.dt(-1.0)) + X.dt(-1.0)) * X(x.noise)
        assert v.shape == (n, x.width) and v.dtype == X.dt
        cols.append(v)
        col += x.width
    return np.concatenate(cols, axis=1)


Want = collections.namedtuple("Want", "f32 f64 full")   # the new frame in both number types; the whole [n, slots, O] output (None for a ring)


@functools.lru_cache(maxsize=None)
def expected(name):
    """``expected_of`` a case of the table: built once, shared by the CPU and the GPU tests, never modified."""
    return expected_of(CASES[name])


def expected_of(case):
    """Per call: the restated frame and, for a history case, the restated output given the previous call's restated output."""
    out, prev = [], case.prev0() if case.H > 1 and not case.ring else None
    for c in range(case.calls):
        f32, f64 = restate_frame(case, c, X32), restate_frame(case, c, X64)
        full = None
        if not case.ring:
            full = f32[:, None, :] if case.H == 1 else np.concatenate([f32[:, None, :], prev[:, :-1, :]], axis=1)   # newest first
            prev = full
        for a in (f32, f64, full):
            if a is not None:
                a.setflags(write=False)
        out.append(Want(f32, f64, full))
    return out


# ---- the dispatch model (coverage only) -------------------------------------------------------------------------------------------------
Tile = collections.namedtuple("Tile", "rows U owners planned lgP gather_passes vec_units scalar_units flat V tail hist_batches mixed_passes")


def units_of(case):
    """(gather units, [(first column, floats per unit)], per-env items) as observe_body / observe_plan count them."""
    units, owners, col = [], 0, 0
    for x in case.items:
        if x.kind in BODY_KINDS:
            owners += 1
        else:
            rows = x.kind != "norm"
            vec = rows and x.width % 4 == 0 and case.stride_of(x) % 4 == 0 and case.off_of(case.buffer_of(x)) % 4 == 0
            units += [(col + 4 * j, 4) for j in range(x.width // 4)] if vec else [(col + j, 1) for j in range(x.width)]
        col += x.width
    return units, owners


def dispatch(case, chain=False):
    """One record per tile shape of the launch (a full tile, the partial last tile)."""
    units, owners = units_of(case)
    U, O, H = len(units), case.O, case.H
    ring = bool(case.ring)
    a_obs, a_prev = case.off.get("obs", 0) * 4 % 16, case.off.get("prev_obs", 0) * 4 % 16
    planned = (not chain) and 1 <= U <= K["PLAN_UNITS"] and owners <= K["PLAN_OWNERS"]
    lgP = (U - 1).bit_length() if U > 1 else 0
    grstep = K["OBS_BLOCK"] >> lgP
    hist = H > 1 and not ring
    flat = hist and O >= 4 and a_obs == 0
    V = 4 if O % 4 == 0 and a_obs == 0 and (not hist or a_prev == 0) else (2 if O % 2 == 0 and a_obs % 8 == 0 and (not hist or a_prev % 8 == 0) else 1)
    tiles = []
    for rows in sorted({min(case.n, K["ENV_BLOCK"]), case.n % K["ENV_BLOCK"] or K["ENV_BLOCK"]}):
        total = rows * O * H
        upr = ((O + 3) >> 2) + 1
        tiles.append(Tile(rows=rows, U=U, owners=owners, planned=planned, lgP=lgP,
                          gather_passes=-(-rows // (K["GATHER"] * grstep)) if U else 0,
                          vec_units=sum(1 for _c, w in units if w == 4), scalar_units=sum(1 for _c, w in units if w == 1),
                          flat=flat, V=V, tail=(total & 3) if flat else 0,
                          hist_batches=max(1, -(-(total >> 2) // (K["HIST_SHIFT"] * K["OBS_BLOCK"]))) if flat else 0,
                          mixed_passes=-(-rows * upr // (K["MIXED_UNITS"] * K["OBS_BLOCK"])) if flat else 0))
    return tiles


def edges_of(case):
    """The names of the dispatch edges a case reaches, for the coverage test and the profile."""
    e = set()
    units, _o = units_of(case)
    for t in dispatch(case):
        e.add("planned" if t.planned else "tables-in-LDS")
        e.add("U=%d" % t.U)
        e.add("owners=%d" % t.owners)
        e.add("lgP=%d" % t.lgP)
        e.add("gather-passes=%d" % t.gather_passes)
        if t.vec_units:
            e.add("vec-units")
        if t.scalar_units:
            e.add("scalar-units")
        if any(w == 4 and c % 4 for c, w in units):
            e.add("vec-unit-at-odd-column")
        e.add("rows=%d" % t.rows)
        if t.flat:
            e.add("flat")
            e.add("tail=%d" % t.tail)
            e.add("hist-batches=%d" % t.hist_batches)
            e.add("mixed-passes=%d" % t.mixed_passes)
            if case.off.get("prev_obs", 0) % 4:
                e.add("flat-prev-dword-aligned")
        elif case.H > 1 and not case.ring:
            e.add("element-history")
            e.add("element-history-V=%d" % t.V)
        if not t.flat:
            e.add("V=%d" % t.V)
        if case.ring:
            e.add("ring")
    return e


# ---- the case table ------------------------------------------------------------------------------------------------------------------------
CASES = {}


def _add(name, n, items, **kw):
    assert name not in CASES and n <= 193
    CASES[name] = Case(name, n, items, **kw)


def _split(total):
    """``total`` 1-float gather units out of external items: odd widths (never a 16-byte unit), two items where the total is even."""
    return [it("ext", total)] if total % 2 else ([it("ext", total // 2 - 1), it("ext", total // 2 + 1)] if total > 2 else [it("ext", 1), it("ext", 1)])


BODY = ("ang", "lin", "grav")
# plan / tables
_add("plan-units48", 65, [it("ext", 47), it("ext", 1)])
_add("plan-units49", 65, [it("ext", 49)])
_add("plan-owners8", 65, [it(BODY[i % 3], scale=(1.0, 0.5)[i & 1]) for i in range(8)] + [it("ext", 1)])
_add("plan-owners9", 65, [it(BODY[i % 3], scale=(1.0, 0.5)[i & 1]) for i in range(9)] + [it("ext", 1)])
_add("plan-nounits-h1", 65, [it("ang"), it("lin", scale=2.0), it("grav")])
_add("plan-nounits-h3", 65, [it("ang"), it("lin", scale=2.0), it("grav")], H=3)
_add("plan-oneunit", 65, [it("ext", 1)])
# lane mapping
LANE_UNITS = (2, 16, 17, 32, 33, 64, 65, 128, 129, 255)
for _u in LANE_UNITS:
    _add("lane-units%d" % _u, 65, _split(_u))
_add("lane-units129-n64", 64, _split(129))
# gather units
_add("gather-vec-stride12", 65, [it("dof_pos", 12, scale=0.5)], D=12)
_add("gather-vec-stride16", 65, [it("cmd", 12, stride=16)])
_add("gather-scalar-source4off", 65, [it("dof_pos", 12, scale=0.5)], D=12, off={"dof_pos": 1})
_add("gather-scalar-stride13", 65, [it("cmd", 12, stride=13)])
_add("gather-scalar-width14", 65, [it("cmd", 14, stride=16)])
_add("gather-interleaved", 65, [it("ext", 1), it("dof_pos", 12), it("base_pos", scale=0.25), it("dof_vel", 12, scale=0.05), it("ext", 3),
                                it("actions", 12), it("base_quat"), it("cmd", 3)], D=12)
_add("gather-norm1-last", 65, [it("dof_pos", 12), it("norm", 1)], D=12)
_add("gather-norm6-last", 65, [it("dof_pos", 12), it("norm", 6, scale=0.5)], D=12)
# write-out without history
WRITE_WIDTHS = (1, 2, 3, 4, 5, 6, 8, 255)
for _o in WRITE_WIDTHS:
    for _al, _off in ((16, 0), (8, 2), (4, 1)):
        _add("write-width%d-align%d" % (_o, _al), 65, [it("ext", _o)], off={"obs": _off})
# history, not a ring
HIST_SHAPES = ((1, 2), (3, 5), (4, 2), (5, 2), (7, 2), (8, 3), (62, 5), (76, 2), (255, 2), (255, 5))


def _hist_items(O):
    return [it("ext", O - 1), it("ext", 1, noise=0.02)] if O >= 4 else [it("ext", O)]


for _o, _h in HIST_SHAPES:
    for _n in (1, 63, 65):
        _add("hist-width%d-frames%d-n%d" % (_o, _h, _n), _n, _hist_items(_o), H=_h)
_add("hist-obs4off-width7", 65, _hist_items(7), H=2, off={"obs": 1})
_add("hist-obs4off-prev4off-width8", 65, _hist_items(8), H=3, off={"obs": 1, "prev_obs": 1})
_add("hist-obs8off-width6", 65, _hist_items(6), H=3, off={"obs": 2, "prev_obs": 2})
_add("hist-prev4off-width7", 65, _hist_items(7), H=2, off={"prev_obs": 1})
_add("hist-prev4off-width8", 65, _hist_items(8), H=3, off={"prev_obs": 1})
_add("hist-prev4off-width255", 63, _hist_items(255), H=5, off={"prev_obs": 3})
# ring: three calls, history_ring at 1, at the last slot and in the middle
for _o, _items in ((3, [it("ext", 3)]), (6, [it("ext", 5, scale=0.5), it("ext", 1, noise=0.02)]), (8, [it("ext", 8)])):
    for _slots in (0, 3, 6):
        _last = _slots or 3
        _add("ring-width%d-slots%d" % (_o, _slots), 65, _items, H=3, ring=(1, _last, (_last + 1) // 2 if _last > 3 else 2), ring_slots=_slots)
# noise
_NOISY = [it("ext", 5, noise=0.02), it("ext", 4, scale=0.5), it("dof_pos", 12, scale=2.0, noise=0.1), it("ext", 3), it("ext", 2, scale=0.25, noise=0.5)]
for _src in ("philox", "dense"):
    for _eo in (0, 1000, 2 ** 32 - 3):
        _add("noise-%s-offset%d" % (_src, _eo), 65, _NOISY, D=12, noise=_src, env_offset=_eo)
# stale quaternion
_BODY_FRAME = [it("ang"), it("ext", 4), it("lin", noise=0.02), it("grav", scale=0.5), it("dof_pos", 12), it("norm", 4)]
for _name, _stale in (("null", None), ("mask1", ("mixed", None)), ("mask2", (None, "mixed")), ("both", ("mixed", "mixed")),
                      ("nomasks", (None, None)), ("zeros", ("zeros", "zeros")), ("ones", ("ones", "ones"))):
    _add("stale-" + _name, 65, _BODY_FRAME, D=12, stale=_stale)
# frames of the chain tests only (two managers of one launch; sizes 65 and 130 are set by the test)
CHAIN_FRAMES = {
    "units49": lambda n: Case("chain-units49-n%d" % n, n, [it("ext", 49, scale=0.5)]),
    "nounits": lambda n: Case("chain-nounits-n%d" % n, n, [it("ang"), it("lin", scale=2.0), it("grav")], H=3, calls=1, stale=("mixed", "mixed")),
    "oddhist": lambda n: Case("chain-oddhist-n%d" % n, n, _hist_items(7), H=2, calls=1),
    "narrow": lambda n: Case("chain-narrow-n%d" % n, n, [it("dof_pos", 8)], D=8),
    "wide": lambda n: Case("chain-wide-n%d" % n, n, [it("ext", 197), it("lin"), it("ext", 51, noise=0.02)], off={"obs": 1}),
    "elemhist": lambda n: Case("chain-elemhist-n%d" % n, n, _hist_items(6), H=3, calls=1, off={"obs": 2, "prev_obs": 2}),
}
NAMES = sorted(CASES)


# ---- running a case through the raw C ABI ------------------------------------------------------------------------------------------------
class Spec:   # what reset_cases.run_ops reads of a launch
    fn = "observe"


class Launch:
    """One case's descriptor on guarded buffers of device ``dev``; ``want`` is ``expected(name)`` (or the same built for a chain frame)."""
    spec = Spec()

    def __init__(self, dev, case, want=None):
        import torch
        from genesis_forge_amd import _native as nat
        from guarded import Guarded
        self.dev, self.case, self.nat = dev, case, nat
        self.want = want if want is not None else (expected(case.name) if CASES.get(case.name) is case else expected_of(case))
        self.args = a = nat.GfObservationArgs()
        n, O = case.n, case.O
        a.num_envs, a.num_dofs, a.num_items, a.obs_width, a.history_len = n, case.D, len(case.items), O, case.H
        a.ring_slots, a.seed, a.env_offset = case.ring_slots, case.seed, case.env_offset
        self.src = {}
        for name, v in case.inputs(0).items():
            row = v.size // v.shape[0]
            dt = torch.uint8 if v.dtype == np.uint8 else torch.float32
            g = Guarded(v.size + PAD_ROWS * row, dt, dev, off=case.off_of(name))
            assert g.ptr % 16 == case.off_of(name) * 4 % 16
            self.src[name] = g
        ops = {"ext": nat.GF_O_EXTERNAL, "cmd": nat.GF_O_COMMAND, "norm": nat.GF_O_CONTACT_FORCE_NORM, "dof_pos": nat.GF_O_DOF_POS,
               "dof_vel": nat.GF_O_DOF_VEL, "dof_force": nat.GF_O_DOF_FORCE, "actions": nat.GF_O_ACTIONS, "raw": nat.GF_O_RAW_ACTIONS,
               "base_pos": nat.GF_O_BASE_POS, "base_quat": nat.GF_O_BASE_QUAT, "ang": nat.GF_O_ANG_VEL_BODY, "lin": nat.GF_O_LIN_VEL_BODY,
               "grav": nat.GF_O_PROJ_GRAVITY}
        for i, x in enumerate(case.items):
            t = a.items[i]
            t.op, t.width, t.scale, t.noise = ops[x.kind], x.width, x.scale, x.noise
            if x.kind in ("ext", "cmd", "norm"):
                slot = int(x.src.split(".")[1])
                t.i0 = slot
                if x.kind == "ext":
                    a.ext[slot] = self.src[x.src].ptr
                elif x.kind == "cmd":
                    a.command[slot].command, a.command[slot].width, a.command[slot].stride = self.src[x.src].ptr, x.width, x.stride
                else:
                    a.contact[slot].contacts, a.contact[slot].num_links = self.src[x.src].ptr, x.width
            elif x.kind in ROW_KINDS:
                setattr(a, ROW_FIELD[x.kind], self.src[x.kind].ptr)
        for name, field in (("pos", "pos"), ("quat", "quat"), ("lin", "lin_vel"), ("ang", "ang_vel")):
            if name in self.src:
                setattr(a.entity, field, self.src[name].ptr)
        for name in ("stale_quat", "stale_mask", "stale_mask2", "noise_draws"):
            if name in self.src:
                setattr(a, name, self.src[name].ptr)
        # outputs: [n + PAD_ROWS, slots, O]; a history case that is not a ring has two, used in turn
        numel = (n + PAD_ROWS) * case.slots * O
        self.out = [Guarded(numel, torch.float32, dev, off=case.off.get("obs", 0))]
        if case.H > 1 and not case.ring:
            self.out.append(Guarded(numel, torch.float32, dev, off=case.off.get("prev_obs", 0)))
            self.out[1].t[:n * case.H * O].copy_(torch.from_numpy(case.prev0().reshape(-1)))
        elif case.ring:   # recognisable content in every slot
            i = np.arange(numel, dtype=np.int64)
            self.out[0].t.copy_(torch.from_numpy(((i * 3) % 8191 - 4000).astype(F)))
        self.snap = None

    def _bits(self, g):
        return g.cpu().numpy().view(np.uint32).reshape(self.case.n + PAD_ROWS, self.case.slots, self.case.O)

    def prepare(self, call):
        """Upload the inputs of call ``call``, point the descriptor at this call's buffers and remember every byte."""
        import torch
        case, a = self.case, self.args
        for name, v in case.inputs(call).items():
            self.src[name].t[:v.size].copy_(torch.from_numpy(np.array(v).reshape(-1)))   # (a writable copy: the inputs are read-only)
        obs = self.out[call & 1] if len(self.out) == 2 else self.out[0]
        prev = self.out[(call + 1) & 1] if len(self.out) == 2 else None
        a.obs, a.prev_obs = obs.ptr, (prev.ptr if prev is not None else None)
        a.stream = case.stream + call
        a.history_ring = case.ring[call] if case.ring else 0
        self.snap = dict(src={k: g.raw.clone() for k, g in self.src.items()}, obs=obs, prev=prev, before=self._bits(obs).copy(),
                         prev_bits=self._bits(prev).copy() if prev is not None else None, prev_raw=prev.raw.clone() if prev is not None else None)

    def run(self, backend, call):
        from guarded import raw_call, sync
        self.prepare(call)
        rc = raw_call(backend, "observe", self.args)
        sync(self.dev)
        return rc

    def check(self, call, what=""):
        """Everything the call may and may not have written; returns (the launch's, the float32 restatement's) maximum error against
        float64 over the columns that are not exact, or None when every column is."""
        import torch
        case, s, w = self.case, self.snap, self.want[call]
        n, O = case.n, case.O
        what = f"{what or case.name}, call {call}"
        for k, g in self.src.items():
            assert torch.equal(g.raw, s["src"][k]), f"{what}: the launch changed its source {k} (or the guards around it)"
        if s["prev"] is not None:
            assert torch.equal(s["prev"].raw, s["prev_raw"]), f"{what}: the launch wrote to prev_obs"
        assert s["obs"].guards_ok(), f"{what}: the launch wrote outside the obs allocation's array"
        got = self._bits(s["obs"])
        exp = s["before"].copy()   # sentinel rows behind num_envs, ring slots not written: as they were
        slot = case.ring[call] - 1 if case.ring else 0
        if s["prev"] is not None:
            exp[:n, 1:, :] = s["prev_bits"][:n, :-1, :]   # the previous call's output, bit for bit
        exp[:n, slot, :] = w.f32.view(np.uint32)
        exact = case.exact_columns()
        diff = got != exp
        diff[:n, slot, ~exact] = False
        if diff.any():
            r, sl, c = (int(v[0]) for v in np.nonzero(diff))
            where = "a row past num_envs" if r >= n else ("the new frame" if sl == slot else "a slot that is not the new frame's")
            raise AssertionError(f"{what}: env {r}, slot {sl}, column {c} ({where}): got {got[r, sl, c:c + 1].view(F)[0]!r}, want "
                                 f"{exp[r, sl, c:c + 1].view(F)[0]!r}; {int(diff.sum())} floats differ")
        written = got[:n] if not case.ring else got[:n, slot:slot + 1]
        assert not (written == SENTINEL).any(), f"{what}: part of the output was left unwritten"
        if w.full is not None:   # … and against the restatement fed the previous call's RESTATED output
            assert np.array_equal(got[:n][:, :, exact], w.full.view(np.uint32)[:, :, exact]), f"{what}: the output differs from the restated history"
        if exact.all():
            return None
        g64 = got[:n, slot, :].view(F).astype(F64)
        e_got = float(np.abs(g64 - w.f64)[:, ~exact].max())
        e_f32 = float(np.abs(w.f32.astype(F64) - w.f64)[:, ~exact].max())
        return e_got, e_f32


def within(name, errs, factor=4.0):
    """The project's bound for arithmetic that is not bit-exact by construction: the launch's maximum error against float64 is at
    most ``factor`` x that of the numpy float32 restatement of the same inputs (printed before it is asserted)."""
    e_got, e_f32 = max(e[0] for e in errs), max(e[1] for e in errs)
    print(f"    OBSERVE-EDGE {name}: e_launch {e_got:.3e}  e_f32 {e_f32:.3e}  ratio {e_got / max(e_f32, 1e-300):.2f}")
    assert e_f32 > 0.0, f"{name}: the float32 restatement has no error against float64 — the bound would be vacuous"
    assert e_got <= factor * e_f32, f"{name}: e_launch {e_got:.3e} > {factor} x e_f32 {e_f32:.3e}"


def run_case(backend, dev, name):
    case = CASES[name]
    l = Launch(dev, case)
    errs = []
    for c in range(case.calls):
        assert l.run(backend, c) == 0, (name, c)
        e = l.check(c)
        if e is not None:
            errs.append(e)
    if errs:
        within(name, errs)
    return l


def constants_in_sources(root):
    """{constant: value} read from the kernel sources under ``root`` (genesis-forge_amd/csrc)."""
    import os
    out = {}
    for key, (fname, pat) in K_SOURCES.items():
        with open(os.path.join(root, fname)) as f:
            m = re.search(pat, f.read())
        out[key] = int(m.group(1)) if m else None
    return out
