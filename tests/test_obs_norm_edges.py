"""gf_obs_norm_update through its raw descriptor, at the decision points of its two launches (cases, the exact reference and the bound:
tests/norm_mirror_cases.py).

Every array the descriptor names — the segments, ``mean`` / ``var`` / ``std``, ``count`` and the workspace, sized exactly
``GF_OBS_NORM_WORKSPACE_BYTES`` — is a slice of a sentinel-filled ``tests/guarded.py`` buffer; after every launch the guards are
intact and the inputs have kept their bits.  Bit-for-bit comparisons are made on int32 views.

The accuracy bound.  The reference is the contract evaluated exactly (rationals) and rounded to float32 once; the kernel evaluates the
same formulas in float64 (u = 2⁻⁵³) and rounds once, so ``|got - exact| <= ulp32/2 + slop`` with slop the error of the float64
evaluation, to first order in u.  With N rows, D = max - min of the column, Δ = |mx - mean|, rate = N / count':

* a lane of launch 1 sums k rows of ``d = x - s`` (|d| <= D, each rounded: u·D): ``Σd`` is off by at most k²·u·D, its mean ``s + Σd/k``
  by (k + 2)·u·D + u·|mx|; the two merges (R lanes in LDS, P records in launch 2, around the first one's mean) add u·D per term.
  k, R (lanes that have rows) and P are each at most N:          ``e_mx = u·((3N + 8)·D + 2·|mx|)``;
* ``Σd²`` is off by (k² + 3k)·u·D² per lane, ``Σd² - (Σd)²/k`` by (3k² + 6k)·u·D²; over all lanes and divided by N that is
  (3k + 6)·u·D²; the between-lane terms ``n_b·(m_b - m0)²`` carry the means' own error, 2·D·((k + 2)·u·D + u·|mx|) each, and their
  sums (P + R)·u·D² more; counting every term generously:        ``e_vx = u·((16N + 32)·D² + 8·D·|mx|)``;
* ``mean' = mean + rate·(mx - mean)``: three roundings on top of rate·e_mx:
                                                                 ``slop_mean = rate·e_mx + u·(3·rate·Δ + |mean| + |mx|)``;
* ``var' = var + rate·(vx - var + d·(mx - mean'))`` with |d|, |mx - mean'| <= Δ, off by e_mx + u·Δ and e_mx + slop_mean + u·Δ:
                                ``slop_var = rate·(e_vx + 3·Δ·(e_mx + slop_mean)) + 8u·(var + rate·(vx + Δ²))``;
* from a fresh state (count = 0, mean = 0) rate is 1 and ``d = mx`` exactly, so ``mean' = mx`` and ``mx - mean'`` is exactly 0:
                                ``slop_mean = e_mx``,  ``slop_var = e_vx + 2u·(var + vx)``.

The half ulp is taken in the binade of ``|exact| + slop``.  The bound is a function of the inputs and the exact reference alone, and
the check applied is ``min(bound, ceiling)`` with the ceilings of tests/test_obs_norm.py (``2⁻²¹ (|mean'| + std')`` and ``2⁻²¹ var'``):
never looser than those.  On the benign class the derived bound itself is asserted to lie under the ceiling; where the ceiling is zero
(a constant or all-zero column from a fresh state) the result must be exactly zero."""
from fractions import Fraction

import numpy as np
import pytest

import norm_mirror_cases as nm
from rsl_rl_norm import RslRlEmpiricalNormalization

STATES = ("fresh", "warm")
SHAPES = nm.norm_shapes()


# ---- CPU: the case module itself -------------------------------------------------------------------------------------------------------------
def test_round_f32_is_round_half_even_with_overflow():
    f = nm.round_f32
    assert f(Fraction(1) + Fraction(1, 2 ** 24)) == 1.0 and f(Fraction(1) + Fraction(3, 2 ** 24)) == 1.0 + 2.0 ** -22   # ties to even
    assert f(Fraction(1) + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 80)) == 1.0 + 2.0 ** -23
    assert f(Fraction(1, 2 ** 150)) == 0.0 and f(Fraction(3, 2 ** 150)) == 2.0 ** -148 and f(-Fraction(1, 2 ** 149)) == -(2.0 ** -149)
    top = Fraction(2 ** 24 - 1) * 2 ** 104
    assert f(top) == float(np.finfo(np.float32).max) and f(top + 2 ** 102) == float(np.finfo(np.float32).max)
    assert f(top + 2 ** 103) == float("inf") and f(-Fraction(10) ** 77) == float("-inf")
    rng = np.random.default_rng(0)
    for v in rng.standard_normal(200) * 10.0 ** rng.integers(-30, 30, size=200):
        assert f(Fraction(float(v))) == float(np.float32(v))


@pytest.mark.parametrize("n,w", [(1, 1), (9, 2), (257, 48), (41, 86), (1025, 310), (65537, 5)])
def test_exact_reference_against_float64_and_rsl_rl(n, w):
    """On the benign class: the exact mean' / var' agree with a float64 numpy evaluation within 2⁻⁴⁰ relative (of ``|mean'| + std'`` and
    of ``var'``: a float64 two-pass evaluation on at most 65 537 rows is far inside that), and the float32 results agree with
    tests/rsl_rl_norm.py within that class's own f32 error — rsl_rl evaluates in float32 throughout: 2⁻²¹ + N·2⁻²⁴ of the same
    magnitudes is what a float32 pairwise mean, a two-pass variance and five more roundings stay under."""
    import torch

    for state in STATES:
        x, st, want = nm.norm_case(n, w, state)
        rot = (n + 3 * w) % len(nm.CLASSES)
        benign = np.array([nm.class_of(c, rot) == "benign" for c in range(w)])
        if not benign.any():
            continue
        x64 = x.astype(np.float64)
        mx, vx = x64.mean(axis=0), x64.var(axis=0)
        m, v = st[0].astype(np.float64), st[1].astype(np.float64)
        rate = n / (st[3] + n)
        m1 = m + rate * (mx - m)
        v1 = v + rate * (vx - v + (mx - m) * (mx - m1))
        mq, vq = np.array([float(q) for q in want["mean_q"]]), np.array([float(q) for q in want["var_q"]])
        assert (np.abs(m1 - mq)[benign] <= 2.0 ** -40 * (np.abs(mq) + np.sqrt(vq))[benign]).all()
        assert (np.abs(v1 - vq)[benign] <= 2.0 ** -40 * vq[benign]).all()
        ref = RslRlEmpiricalNormalization(int(benign.sum()))
        ref._mean.copy_(torch.from_numpy(st[0][benign])[None]), ref._var.copy_(torch.from_numpy(st[1][benign])[None]), ref.count.fill_(st[3])
        ref.update(torch.from_numpy(x[:, benign]))
        tol = 2.0 ** -21 + n * 2.0 ** -24
        assert int(ref.count) == want["count"]
        assert (np.abs(ref._mean[0].double().numpy() - mq[benign]) <= tol * (np.abs(m) + np.abs(mx) + np.sqrt(vq))[benign]).all()
        assert (np.abs(ref._var[0].double().numpy() - vq[benign]) <= tol * (v + vx + (mx - m) ** 2)[benign]).all()


@pytest.mark.parametrize("n,w,state", [(1, 3, "fresh"), (9, 7, "warm"), (41, 14, "big"), (300, 7, "warm")])
def test_the_integer_evaluation_is_the_contract_in_fractions(n, w, state):
    x, st = nm.norm_data(n, w), nm.state_of(state, w)
    want = nm.exact_update(st[0], st[1], st[3], x)
    mq, vq = nm.exact_update_fractions(st[0], st[1], st[3], x)
    assert want["mean_q"] == mq and want["var_q"] == vq and want["count"] == st[3] + n
    assert all(abs(float(a) - b) <= 2.0 ** -50 * abs(b) for a, b in zip(mq, [float(q) for q in want["mean_q"]]))


def test_data_classes_are_what_they_say():
    x, _st, want = nm.norm_case(257, 48, "fresh")
    rot = (257 + 3 * 48) % len(nm.CLASSES)
    kinds = [nm.class_of(c, rot) for c in range(48)]
    assert set(kinds) == set(nm.CLASSES)
    for c, kind in enumerate(kinds):
        col = x[:, c]
        if kind in ("constant", "zero"):
            assert want["var_q"][c] == 0 and want["var"][c] == 0.0 and want["std"][c] == 0.0 and (col == col[0]).all()
        if kind == "offset":   # a few ulps of the float32 grid at 10^6
            assert (np.abs(col - 1.0e6) <= 4 * np.spacing(np.float32(1.0e6))).all() and len(set(col.tolist())) > 2
        if kind == "huge":
            assert np.isposinf(want["var"][c]) and np.isposinf(want["std"][c]) and np.isfinite(want["mean"][c]) and np.abs(col).min() > 2.9e38
        if kind == "ramp":     # the block means are far from the first record's
            assert abs(float(col[:8].mean()) - float(col.mean())) > 10.0
        if kind == "alternating":
            assert set(col.tolist()) == {1024.0, -1024.0}
    big = nm.state_of("big", 3)
    assert big[3] == 2 ** 31 + 5 > 2 ** 31


def test_the_grid_has_a_case_on_each_side_of_every_threshold():
    """The thresholds come from the launch plan's formulas, not from a list."""
    widths = set(nm.norm_widths())
    one_seg = set(nm.WIDTHS)
    # launch 1: R = 256 // W changes 3 -> 2 -> 1; the one-column / four-column switch
    for r in (3, 2):
        w = nm.ON_BLOCK // r
        assert nm.lane_rows(w) == r and nm.lane_rows(w + 1) == r - 1 and {w, w + 1} <= one_seg, r
    assert nm.lane_rows(nm.ON_BLOCK) == 1 and nm.col_groups(nm.ON_BLOCK) == 1 and nm.col_groups(nm.ON_BLOCK + 1) == 2
    assert {nm.ON_BLOCK - 1, nm.ON_BLOCK, nm.ON_BLOCK + 1} <= one_seg
    # the four-column body: group q first has a live lane at W = 256 q + 1; a partly filled and a full last group for q = 1, 2, 3
    for q in (1, 2, 3):
        first = nm.ON_BLOCK * q + 1
        assert nm.col_groups(first - 1) == q and nm.col_groups(first) == q + 1 and {first - 1, first} <= one_seg, q
        assert any(nm.col_groups(w) == q + 1 and w % nm.ON_BLOCK != 0 for w in widths), f"no partly filled group {q}"
        assert any(nm.col_groups(w) == q + 1 and w % nm.ON_BLOCK == 0 for w in widths), f"no full group {q}"
    assert nm.ON_MAX_WIDTH in one_seg and nm.ON_MAX_WIDTH - 1 in one_seg and nm.col_groups(nm.ON_MAX_WIDTH) == 4
    # launch 2: J = 1024 // W changes 3 -> 2 -> 1
    for j in (3, 2):
        w = nm.ON_FIN_BLOCK // j
        assert nm.fin_lanes(w) == j and nm.fin_lanes(w + 1) == j - 1 and {w, w + 1} <= one_seg, j
    # the record loop b += J: P on J, J + 1 and 2J + 1 at the two wrap widths, and P > J in a wide-J configuration
    for w in nm.WRAP_WIDTHS:
        j = nm.fin_lanes(w)
        ps = {nm.partials(n) for n in nm.norm_rows_of(w)}
        assert j in (2, 3) and {j, j + 1, 2 * j + 1} <= ps, (w, j, sorted(ps))
    assert any(nm.partials(n) > nm.fin_lanes(w) >= 100 for w in nm.GRID_STRIDE_WIDTHS for n in nm.norm_rows_of(w))
    assert any(nm.partials(n) == nm.ON_MAX_PARTIALS and n > nm.ON_MAX_PARTIALS * nm.ON_TILE for w in nm.GRID_STRIDE_WIDTHS for n in nm.norm_rows_of(w))
    # the row loop: one row to either side of a lane's stride R·8 at every width; the tile and two tiles at the narrow widths
    for w in widths:
        s = nm.lane_rows(w) * nm.ON_UNROLL
        assert {s - 1, s, s + 1} - {0} <= set(nm.norm_rows_of(w)), w
    for w in nm.NARROW_WIDTHS:
        rows = set(nm.norm_rows_of(w))
        assert w <= 48 and {nm.ON_TILE - 1, nm.ON_TILE, nm.ON_TILE + 1, 2 * nm.ON_TILE - 1, 2 * nm.ON_TILE, 2 * nm.ON_TILE + 1} <= rows, w
    assert nm.lane_rows(48) * nm.ON_UNROLL == 40 and {39, 40, 41} <= set(nm.norm_rows_of(48))
    # segments: a width-1 segment first and last, on either side of the Q switch
    assert any(s[0] == 1 and s[-1] == 1 and sum(s) <= nm.ON_BLOCK for s in nm.SEGMENTS.values())
    assert any(s[0] == 1 and s[-1] == 1 and sum(s) > nm.ON_BLOCK for s in nm.SEGMENTS.values())
    assert all(sum(s) == w and 2 <= len(s) <= 4 for w, s in nm.SEGMENTS.items())
    assert max(n * w for n, w in SHAPES) <= 2 ** 20   # the largest cases: 65 537 x 5 (3.3·10^5 elements) and 1 793 x 342 (6.1·10^5)


# ---- GPU: the launch -----------------------------------------------------------------------------------------------------------------------------
class _Set:
    """One normaliser set on guarded buffers.  ``layout``: "contig" (one segment), "segs" (``widths``: a buffer per segment), "strided"
    (every segment a window of one NaN-filled row buffer, 3 gap columns in front of each and 2 behind the last), "off4" (one segment
    whose base is 4 bytes past a 16-byte boundary)."""

    def __init__(self, x, state, layout="contig", widths=None, until=-1):
        import torch
        from genesis_forge_amd import _native as nat
        from guarded import Guarded

        self.x = np.array(x, dtype=np.float32)   # (a copy: the shared case stays read-only)
        n, w = self.x.shape
        self.n, self.w, self.until = n, w, until
        widths = (w,) if widths is None or layout in ("contig", "off4") else tuple(widths)
        assert sum(widths) == w
        self.segments, self.inputs = [], []   # (ptr, width, row_stride), guarded input buffers
        if layout == "strided":
            stride = w + 3 * len(widths) + 2
            full = np.full((n, stride), np.nan, dtype=np.float32)
            at, col = 0, 0
            for ws in widths:
                col += 3
                full[:, col:col + ws] = self.x[:, at:at + ws]
                self.segments.append((col, ws, stride))
                at, col = at + ws, col + ws
            g = Guarded(n * stride, torch.float32, "cuda", init=torch.from_numpy(full))
            self.inputs.append(g)
            self.segments = [(g.ptr + 4 * c, ws, st) for c, ws, st in self.segments]
        else:
            at = 0
            for ws in widths:
                part = np.ascontiguousarray(self.x[:, at:at + ws])
                g = Guarded(n * ws, torch.float32, "cuda", off=1 if layout == "off4" else 0, init=torch.from_numpy(part))
                assert g.ptr % 16 == (4 if layout == "off4" else 0)
                self.inputs.append(g)
                self.segments.append((g.ptr, ws, 0))
                at += ws
        self.input_bits = [g.raw.clone() for g in self.inputs]
        mean, var, std, count = state
        f = lambda a: Guarded(w, torch.float32, "cuda", init=torch.from_numpy(np.ascontiguousarray(a)))
        self.mean, self.var, self.std = f(mean), f(var), f(std)
        self.count = Guarded(1, torch.int64, "cuda", init=torch.tensor([count], dtype=torch.int64))
        self.ws_bytes = nat.obs_norm_workspace_bytes(n, w)
        assert self.ws_bytes % 8 == 0
        self.workspace = Guarded(self.ws_bytes // 8, torch.float64, "cuda")
        self.state_bufs = (self.mean, self.var, self.std, self.count)

    def fill(self, st):
        st.num_inputs = len(self.segments)
        for seg, (ptr, ws, stride) in zip(st.inputs, self.segments):
            seg.rows, seg.width, seg.row_stride = ptr, ws, stride
        st.mean, st.var, st.std, st.count = self.mean.ptr, self.var.ptr, self.std.ptr, self.count.ptr
        st.until, st.workspace, st.workspace_bytes = self.until, self.workspace.ptr, self.ws_bytes

    def snapshot(self):
        return [g.raw.clone() for g in self.state_bufs]

    def same_as(self, snap):
        import torch

        return all(torch.equal(g.raw, s) for g, s in zip(self.state_bufs, snap))

    def check_silence(self, what):
        import torch

        for name, g in (("mean", self.mean), ("var", self.var), ("std", self.std), ("count", self.count), ("workspace", self.workspace)):
            assert g.guards_ok(), f"{what}: wrote outside {name}"
        for g, before in zip(self.inputs, self.input_bits):
            assert torch.equal(g.raw, before), f"{what}: an input buffer (or its guards) changed"

    def result(self):
        return self.mean.cpu().numpy(), self.var.cpu().numpy(), self.std.cpu().numpy(), int(self.count.cpu()[0])


def _launch(backend, sets, what=""):
    import torch
    from genesis_forge_amd import _native as nat
    from guarded import raw_call

    a = nat.GfObsNormArgs()
    a.num_rows, a.num_sets = sets[0].n, len(sets)
    for st, s in zip(a.sets, sets):
        assert s.n == sets[0].n
        s.fill(st)
    assert raw_call(backend, "obs_norm_update", a) == 0, what
    torch.cuda.synchronize()
    for s in sets:
        s.check_silence(what)
    return [s.result() for s in sets]


def _update(backend, x, state, **kw):
    return _launch(backend, [_Set(x, state, **kw)], str(kw))[0]


def _same_bits(a, b):
    return all(np.array_equal(nm.i32(p), nm.i32(q)) for p, q in zip(a[:3], b[:3])) and a[3] == b[3]


def _check_exact(got, x, st, want, what, rot):
    """Holds one result to the exact reference; returns {class: [worst |err| / bound of mean', of var', worst share of the slop used]}
    — the share is ``(|err| - ulp32/2) / slop`` where that is positive: how far past the final rounding the float64 evaluation went."""
    mean, var, std, count = got
    n, w = x.shape
    assert count == want["count"], f"{what}: count {count} vs {want['count']}"
    assert np.array_equal(nm.i32(std), nm.i32(nm.sqrt_f32(var))), f"{what}: std' is not the correctly rounded root of the returned var'"
    bm, bv, cm, cv, sm, sv = nm.norm_bounds(x, st, want)
    worst = {}
    for c in range(w):
        kind = nm.class_of(c, rot)
        ratios, share = [], 0.0
        for name, g, q, ref32, b, ceil, slop in (("mean'", mean[c], want["mean_q"][c], want["mean"][c], bm[c], cm[c], sm[c]),
                                                 ("var'", var[c], want["var_q"][c], want["var"][c], bv[c], cv[c], sv[c])):
            if not np.isfinite(ref32):   # the ±3e38 column: var' overflows float32 in the reference and in the kernel
                assert kind == "huge" and name == "var'" and g == ref32 == np.inf and std[c] == np.inf, f"{what}: column {c} ({kind}) {name} {g} vs {ref32}"
                continue
            assert np.isfinite(g), f"{what}: column {c} ({kind}) {name} = {g}, exact {float(q):.9g}"
            err = float(abs(Fraction(float(g)) - q))
            if kind == "benign" and ceil > 0.0:
                assert b <= ceil, f"{what}: column {c}: the derived bound {b:.3e} is looser than the 2^-21 ceiling {ceil:.3e} ({name})"
            if not np.isfinite(ceil) or ceil > 0.0:
                bound = min(b, ceil)
                assert err <= bound, f"{what}: column {c} ({kind}) {name} = {g!r}, exact {float(q):.17g}: off by {err:.3e}, bound {bound:.3e}"
                ratios.append(err / bound)
                share = max(share, (err - (b - slop)) / slop if slop > 0.0 else 0.0)
            else:
                assert g == 0.0, f"{what}: column {c} ({kind}) {name} = {g!r}, exactly 0 expected"
                ratios.append(0.0)
        if kind in ("constant", "zero") and st[3] == 0:
            assert var[c] == 0.0 and std[c] == 0.0, f"{what}: column {c} ({kind}): var' {var[c]!r}, std' {std[c]!r} from a fresh state"
        old = worst.get(kind, (0.0, 0.0, 0.0))
        ratios.append(0.0)   # (the ±3e38 column has no var' ratio)
        worst[kind] = (max(old[0], ratios[0]), max(old[1], ratios[1]), max(old[2], share))
    return worst


def _report(what, worst):
    print(f"NORM_EDGES {what}: " + " ".join(f"{k}={m:.4f}/{v:.4f}/{s:.2e}" for k, (m, v, s) in sorted(worst.items())) + "  (worst |err| / bound of mean' / var' / share of the slop used)")


def _exact_case(backend, n, w, state, **kw):
    x, st, want = nm.norm_case(n, w, state)
    got = _update(backend, x, st, **kw)
    what = f"N={n} W={w} {state} {kw or ''}"
    worst = _check_exact(got, x, st, want, what, (n + 3 * w) % len(nm.CLASSES))
    _report(what, worst)
    return got


# ---- GPU: accuracy against the exact reference -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,w", SHAPES, ids=[f"{n}x{w}" for n, w in SHAPES])
def test_update_equals_the_exact_reference(hip_backend, n, w):
    for state in STATES:
        _exact_case(hip_backend, n, w, state)


@pytest.mark.gpu
@pytest.mark.parametrize("w", sorted(nm.SEGMENTS))
def test_update_of_segments_with_nan_gaps_equals_the_exact_reference(hip_backend, w):
    """2 … 4 segments, windows of one row buffer whose gap columns hold NaN: a lane that read a gap would poison its column."""
    for n in sorted({1, nm.row_stride_of_a_lane(w) + 1, 257}):
        for state in STATES:
            got = _exact_case(hip_backend, n, w, state, layout="strided", widths=nm.SEGMENTS[w])
            x, st, _want = nm.norm_case(n, w, state)
            assert _same_bits(got, _update(hip_backend, x, st)), f"W={w} N={n} {state}: segments differ from one segment"


@pytest.mark.gpu
@pytest.mark.parametrize("n,w", [(1, 1), (9, 513), (257, 48), (41, 86), (65537, 5)])
def test_update_from_a_count_above_2_to_the_31(hip_backend, n, w):
    got = _exact_case(hip_backend, n, w, "big")
    assert got[3] == 2 ** 31 + 5 + n


# ---- GPU: the bitwise invariants ------------------------------------------------------------------------------------------------------------
def _permuted(state, pi):
    return state[0][pi], state[1][pi], state[2][pi], state[3]


@pytest.mark.gpu
@pytest.mark.parametrize("w", [86, 129, 257, 513, 769, 1024])
def test_a_column_permutation_of_the_input_permutes_the_state(hip_backend, w):
    """Every column gets the same lane arithmetic, wherever it sits: ``update(x[:, π])`` is ``update(x)[π]`` bit for bit — in one segment,
    and with π carrying columns across the boundaries of three segments (a width-1 segment first and last)."""
    n = 300   # two tiles, the second ragged
    x, st, _want = nm.norm_case(n, w, "warm")
    base = _update(hip_backend, x, st)
    pi = np.random.default_rng(w).permutation(w)
    assert not np.array_equal(pi, np.arange(w))
    want = (base[0][pi], base[1][pi], base[2][pi], base[3])
    xp = np.ascontiguousarray(x[:, pi])
    assert _same_bits(_update(hip_backend, xp, _permuted(st, pi)), want), "one segment"
    for layout in ("segs", "strided"):
        assert _same_bits(_update(hip_backend, xp, _permuted(st, pi), layout=layout, widths=(1, w - 2, 1)), want), layout
    shift = np.roll(np.arange(w), 1)   # every column moves one lane on; the last one wraps to lane 0
    got = _update(hip_backend, np.ascontiguousarray(x[:, shift]), _permuted(st, shift), layout="segs", widths=(w - 1, 1))
    assert _same_bits(got, (base[0][shift], base[1][shift], base[2][shift], base[3])), "rolled by one column"


@pytest.mark.gpu
@pytest.mark.parametrize("n,w,widths", [(41, 48, (1, 46, 1)), (257, 48, (5, 1, 41, 1)), (300, 257, (256, 1)), (9, 1024, (512, 1, 511)), (513, 342, (1, 340, 1))])
def test_four_layouts_and_a_repeat_give_the_same_bits(hip_backend, n, w, widths):
    for state in STATES:
        x, st, _want = nm.norm_case(n, w, state)
        base = _update(hip_backend, x, st)
        assert _same_bits(base, _update(hip_backend, x, st)), f"{state}: a second run differs"
        assert _same_bits(base, _update(hip_backend, x, st, layout="segs", widths=widths)), f"{state}: {widths} segments"
        assert _same_bits(base, _update(hip_backend, x, st, layout="strided", widths=widths)), f"{state}: strided {widths} with NaN gaps"
        assert _same_bits(base, _update(hip_backend, x, st, layout="strided")), f"{state}: one strided segment"
        assert _same_bits(base, _update(hip_backend, x, st, layout="off4")), f"{state}: base 4 bytes past a 16-byte boundary"


@pytest.mark.gpu
@pytest.mark.parametrize("wa,wb", [(256, 257), (257, 256), (48, 1024)])
def test_two_sets_in_one_call_equal_two_calls(hip_backend, wa, wb):
    n = 300
    (xa, sa, _), (xb, sb, _) = nm.norm_case(n, wa, "warm"), nm.norm_case(n, wb, "fresh")
    both = _launch(hip_backend, [_Set(xa, sa), _Set(xb, sb)], "two sets")
    assert _same_bits(both[0], _update(hip_backend, xa, sa)) and _same_bits(both[1], _update(hip_backend, xb, sb))


@pytest.mark.gpu
@pytest.mark.parametrize("frozen", [0, 1])
def test_a_frozen_set_is_untouched_while_the_other_updates(hip_backend, frozen):
    """``count >= until``: not one byte of the four state buffers (or of their guards) changes; the other set of the call updates."""
    n, widths = 300, (256, 257)
    cases = [nm.norm_case(n, w, "warm") for w in widths]
    sets = [_Set(x, st, until=st[3] if i == frozen else st[3] + 1) for i, (x, st, _w) in enumerate(cases)]
    snaps = [s.snapshot() for s in sets]
    got = _launch(hip_backend, sets, "frozen")
    assert sets[frozen].same_as(snaps[frozen]), "the frozen set changed"
    live = 1 - frozen
    x, st, want = cases[live]
    assert not sets[live].same_as(snaps[live])
    _check_exact(got[live], x, st, want, "the set that is not frozen", (n + 3 * widths[live]) % len(nm.CLASSES))
    assert _same_bits(got[live], _update(hip_backend, x, st))
    # until not reached yet (count = until - 1): the set updates once, and is frozen from then on
    again = _launch(hip_backend, sets, "frozen, second call")
    assert sets[frozen].same_as(snaps[frozen])
    assert again[live][3] == got[live][3], "count >= until after the first update: the second call must not count"
    assert _same_bits(again[live], got[live])


@pytest.mark.gpu
@pytest.mark.parametrize("w", [48, 300])
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_element_stays_in_its_column(hip_backend, w, bad):
    """One NaN / +inf element: its column's mean' / var' / std' are not finite, every other column keeps the bits of the clean run and
    count' advances — with the element in the first row (a lane's reference point ``s``), in the last row of the ragged second tile and
    in a row that a sub-lane > 0 owns (row 1 at W = 48, where a workgroup reads 5 rows at a time)."""
    n = 300
    x, st, _want = nm.norm_case(n, w, "warm")
    clean = _update(hip_backend, x, st)
    assert nm.lane_rows(48) > 1
    for row, col in ((0, 0), (n - 1, w - 1), (1, w // 2), (nm.ON_TILE + 1, 1)):
        y = x.copy()
        y[row, col] = bad
        got = _update(hip_backend, y, st)
        assert got[3] == clean[3] == st[3] + n
        others = np.arange(w) != col
        for name, g, c in zip(("mean'", "var'", "std'"), got[:3], clean[:3]):
            assert not np.isfinite(g[col]), f"{name}[{col}] = {g[col]} with x[{row}, {col}] = {bad}"
            assert np.array_equal(nm.i32(g)[others], nm.i32(c)[others]), f"{name}: another column changed with x[{row}, {col}] = {bad}"
