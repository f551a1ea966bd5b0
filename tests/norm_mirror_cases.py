"""Cases and references for tests/test_obs_norm_edges.py and tests/test_mirror_rows_edges.py.  No GPU, no kernel code: numpy and
Python integers only.

``gf_obs_norm_update``: the contract's formulas (include/gf_step.h: mx, vx biased, count', rate, mean', var') evaluated EXACTLY.  A
float32 is a dyadic rational, so a column scaled by the right power of two is a column of integers; Σx and Σx² are integer sums
(int64 where the bound below allows it, Python integers otherwise) and the update is integer arithmetic over a common denominator
from the f32 state (``exact_update``; ``exact_update_fractions`` states the same with ``fractions.Fraction`` and checks it).  mean' and var' are rounded to float32 once each (``round_f32``: round-half-even on the rational, overflow to ±inf); std' is
the correctly rounded root of the f32 var'.  The data are drawn on dyadic grids so that the integer sums stay in int64.

``gf_mirror_rows``: numpy indexing ``sign * x[:, perm]``, and for the normalised path float32 numpy, one rounding per operation.

The shape grids put a case on each side of every decision point of the two kernels; ``tests/test_*_edges.py`` prove that from the
formulas (``lane_rows`` = R, ``fin_lanes`` = J, ``col_groups``, ``partials`` = P, ``mirror_tile``)."""
import functools
import math
from fractions import Fraction

import numpy as np

# ---- the launch plan of gf_obs_norm_update, restated from include/gf_step.h and the kernel's header comment ------------------------------
ON_BLOCK = 256          # lanes of a workgroup of launch 1
ON_TILE = 256           # GF_OBS_NORM_TILE_ROWS
ON_UNROLL = 8           # rows of loads a lane has in flight
ON_FIN_BLOCK = 1024     # lanes of launch 2
ON_MAX_PARTIALS = 256   # GF_OBS_NORM_MAX_PARTIALS
ON_MAX_WIDTH = 1024     # GF_MLP_MAX_INPUT_WIDTH


def lane_rows(w):
    """R: the rows a workgroup of launch 1 reads at a time (a lane keeps one column while W <= 256, four column groups above)."""
    return ON_BLOCK // w if w <= ON_BLOCK else 1


def col_groups(w):
    """Column groups of ``ON_BLOCK`` columns with a live lane (1 in the one-column-per-lane body, up to 4 above 256 columns)."""
    return -(-w // ON_BLOCK)


def row_stride_of_a_lane(w):
    return lane_rows(w) * ON_UNROLL


def fin_lanes(w):
    """J: the lanes of launch 2 that share a column's records."""
    return ON_FIN_BLOCK // w


def partials(n):
    """P: workgroups (records) of launch 1."""
    return min(-(-n // ON_TILE), ON_MAX_PARTIALS)


# ---- exact rounding ------------------------------------------------------------------------------------------------------------------------
def round_f32(q):
    """The float32 nearest to the rational ``q`` (ties to even, ±inf past the largest finite), as a Python float."""
    q = Fraction(q)
    num, den = abs(q.numerator), q.denominator
    if num == 0:
        return 0.0
    sign = -1.0 if q < 0 else 1.0
    e = num.bit_length() - den.bit_length()                      # 2^(e-1) < q < 2^(e+1)
    if (num < (den << e)) if e >= 0 else ((num << -e) < den):
        e -= 1                                                   # 2^e <= q < 2^(e+1)
    if e >= 128:
        return sign * math.inf
    qe = max(e, -126) - 23                                       # the exponent of the float32 quantum at q
    nn, dd = (num, den << qe) if qe >= 0 else (num << -qe, den)
    k, r = divmod(nn, dd)
    if 2 * r > dd or (2 * r == dd and k & 1):
        k += 1
    if k >= 2 ** 24 and qe == 104:
        return sign * math.inf
    return sign * math.ldexp(float(k), qe)                       # (at most 24 bits: exact in a float64, denormals included)


def sqrt_f32(v):
    """The correctly rounded float32 root of float32 ``v``: the float64 root rounded once more (53 >= 2·24 + 2 bits: innocuous)."""
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.asarray(v, dtype=np.float32).astype(np.float64)).astype(np.float32)


# ---- exact column sums ---------------------------------------------------------------------------------------------------------------------
def _column_sums_slow(col, k):
    ints = [int(v) for v in np.ldexp(col.astype(np.float64), -k)]   # (a power-of-two scale: exact)
    c = ints[0]
    ys = [v - c for v in ints]
    return c, sum(ys), sum(v * v for v in ys)


def column_sums(x):
    """Per column of the float32 matrix ``x``: ``(k, c, S1, S2)`` with ``x_n = (c + y_n) · 2^k``, ``S1 = Σ y_n``, ``S2 = Σ y_n²`` — Python
    integers, exact.  ``2^k`` is the lowest set bit of the column, so the ``y_n`` are integers; the sums run in int64 where
    ``max|y|² · N < 2^62`` and over Python integers otherwise."""
    x = np.asarray(x, dtype=np.float32)
    assert np.isfinite(x).all()
    n = x.shape[0]
    x64 = x.astype(np.float64)
    m, e = np.frexp(x64)
    mant = np.abs(m * 2.0 ** 24).astype(np.int64)               # 24-bit integers (fewer bits for denormals: still integers)
    low = np.maximum(mant & -mant, 1)
    tz = np.frexp(low.astype(np.float64))[1] - 1
    k = np.where(mant != 0, e.astype(np.int64) - 24 + tz, 1 << 20).min(axis=0)
    k = np.where(k == 1 << 20, 0, k)                             # (an all-zero column)
    scaled = np.ldexp(x64, -k[None, :].astype(np.int32))
    small = np.abs(scaled).max(axis=0) < 2.0 ** 52
    xi = np.where(small[None, :], scaled, 0.0).astype(np.int64)
    y = xi - xi[0:1]
    top = np.abs(y).max(axis=0).astype(np.float64)
    fast = small & (top * top * n < 2.0 ** 62)
    s1, s2 = y.sum(axis=0), (y * y).sum(axis=0)                  # (wraps silently in a column that is not `fast`: not used there)
    out = []
    for c in range(x.shape[1]):
        if fast[c]:
            out.append((int(k[c]), int(xi[0, c]), int(s1[c]), int(s2[c])))
        else:
            out.append((int(k[c]),) + _column_sums_slow(x[:, c], int(k[c])))
    return out


def _pow2_ratio(f):
    """float -> (integer, exponent) with f = integer · 2^exponent."""
    num, den = float(f).as_integer_ratio()
    return num, -(den.bit_length() - 1)


def _scaled(num, den, p):
    """num / den · 2^p as a Fraction."""
    return Fraction(num << p, den) if p >= 0 else Fraction(num, den << -p)


def exact_update(mean, var, count, x):
    """The contract, column by column, exactly: every line below is a line of include/gf_step.h as a quotient of Python integers, in
    units of ``2^p`` (values) and ``4^p`` (variances), ``2^p`` a power of two that divides the column's elements, its mean and — squared —
    its variance.  ``mean`` / ``var``: float32 ``[W]``; ``x``: float32 ``[N, W]``.  Returns a dict: ``mean`` / ``var`` / ``std`` float32
    ``[W]`` (rounded once each), ``count``, the exact ``mean_q`` / ``var_q`` (Fractions) and ``mx`` / ``vx`` / ``delta`` = |mx - mean|
    (float64 roundings of the exact values, for the error bound)."""
    x = np.asarray(x, dtype=np.float32)
    N, w = x.shape
    C = int(count) + N                                            # count'
    mean_q, var_q, mxs, vxs, deltas = [], [], [], [], []
    for c, (k, c0, s1, s2) in enumerate(column_sums(x)):
        mn, me = _pow2_ratio(mean[c])
        vn, ve = _pow2_ratio(var[c])
        p = min(k, me, ve // 2)                                   # (// floors)
        a = (c0 * N + s1) << (k - p)                              # mx = a / N
        b = (N * s2 - s1 * s1) << (2 * (k - p))                   # vx = b / N²      (biased)
        mi = mn << (me - p)                                       # mean
        vi = vn << (ve - 2 * p)                                   # var
        dn = a - mi * N                                           # d = mx - mean = dn / N
        m1n = mi * C + dn                                         # mean' = mean + rate·d = m1n / C,   rate = N / C
        gn = a * C - N * m1n                                      # mx - mean' = gn / (N·C)
        hn = b * C - vi * N * N * C + dn * gn                     # vx - var + d·(mx - mean') = hn / (N²·C)
        v1n = vi * N * C * C + hn                                 # var' = var + rate·(…) = v1n / (N·C²)
        mean_q.append(_scaled(m1n, C, p)), var_q.append(_scaled(v1n, N * C * C, 2 * p))
        mxs.append(math.ldexp(a / N, p)), vxs.append(math.ldexp(b / (N * N), 2 * p)), deltas.append(math.ldexp(abs(dn) / N, p))
    m32 = np.array([round_f32(q) for q in mean_q], dtype=np.float32)
    v32 = np.array([round_f32(q) for q in var_q], dtype=np.float32)
    return dict(mean=m32, var=v32, std=sqrt_f32(v32), count=C, mean_q=mean_q, var_q=var_q, mx=np.array(mxs), vx=np.array(vxs),
                delta=np.array(deltas), rate=N / C)


def exact_update_fractions(mean, var, count, x):
    """The same contract, written with ``fractions.Fraction`` exactly as the header states it (slow: the check of ``exact_update``)."""
    x = np.asarray(x, dtype=np.float32)
    n, w = x.shape
    rate = Fraction(n, int(count) + n)
    out_m, out_v = [], []
    for c in range(w):
        col = [Fraction(float(v)) for v in x[:, c]]
        mx = sum(col) / n
        vx = sum((v - mx) ** 2 for v in col) / n
        m, v = Fraction(float(mean[c])), Fraction(float(var[c]))
        d = mx - m
        m1 = m + rate * d
        out_m.append(m1), out_v.append(v + rate * (vx - v + d * (mx - m1)))
    return out_m, out_v


# ---- data classes of the norm update -----------------------------------------------------------------------------------------------------
CLASSES = ("benign", "constant", "offset", "ramp", "alternating", "huge", "zero")
GRID = 2.0 ** -10


def class_of(c, rot):
    return CLASSES[(c + rot) % len(CLASSES)]


def norm_data(n, w, seed=0, rot=None):
    """float32 ``[n, w]``: column ``c`` is of class ``class_of(c, rot)`` — neighbouring lanes hold different classes.  Every value is
    exactly a float32 on a dyadic grid:

    * benign — ``round(randn · 2^e · 2^10) / 2^10 + offset`` with ``e`` in -3 … 5 and an offset within ±64 on the grid;
    * constant — one grid value; * zero — +0.0;
    * offset — ``10^6 + j / 16`` with ``j`` in -4 … 4: a spread of a few ulps of the float32 grid at 10^6 (ulp 1/16);
    * ramp — ``n / 8 - 3``;  * alternating — ``(-1)^n · 2^10``;
    * huge — ``± float32(3e38) · (1 - j · 2^-20)``, ``j`` in 0 … 7: var' overflows float32."""
    rot = (n + 3 * w) % len(CLASSES) if rot is None else rot
    rng = np.random.default_rng(100003 * seed + 1009 * n + w)
    x = np.empty((n, w), dtype=np.float32)
    rows = np.arange(n)
    for c in range(w):
        kind = class_of(c, rot)
        if kind == "benign":
            scale = 2.0 ** int(rng.integers(-3, 6))
            off = float(rng.integers(-65536, 65537)) * GRID
            col = np.round(rng.standard_normal(n).clip(-6, 6) * scale / GRID) * GRID + off
        elif kind == "constant":
            col = np.full(n, float(rng.integers(-65536, 65537)) * GRID)
        elif kind == "zero":
            col = np.zeros(n)
        elif kind == "offset":
            col = 1.0e6 + rng.integers(-4, 5, size=n) / 16.0
        elif kind == "ramp":
            col = rows / 8.0 - 3.0
        elif kind == "alternating":
            col = np.where(rows % 2 == 0, 1024.0, -1024.0)
        else:
            big = np.float64(np.float32(3e38))
            col = np.where(rng.integers(0, 2, size=n) == 0, 1.0, -1.0) * big * (1.0 - rng.integers(0, 8, size=n) * 2.0 ** -20)
        as32 = col.astype(np.float32)
        assert kind == "huge" or (as32.astype(np.float64) == col).all(), kind   # on the grid: nothing was rounded
        x[:, c] = as32
    return x


def warm_state(w, count=1000, seed=3):
    """A float32 state with ``count`` > 0: means within ±64 and variances 2^-4 … 2^4 on the grid."""
    rng = np.random.default_rng(7919 * seed + w)
    mean = (rng.integers(-65536, 65537, size=w) * GRID).astype(np.float32)
    var = (2.0 ** rng.integers(-4, 5, size=w) + rng.integers(0, 64, size=w) * GRID).astype(np.float32)
    return mean, var, sqrt_f32(var), int(count)


def fresh_state(w):
    """rsl_rl's initial buffers."""
    return np.zeros(w, dtype=np.float32), np.ones(w, dtype=np.float32), np.ones(w, dtype=np.float32), 0


BIG_COUNT = 2 ** 31 + 5


def state_of(kind, w):
    return {"fresh": lambda: fresh_state(w), "warm": lambda: warm_state(w), "big": lambda: warm_state(w, BIG_COUNT)}[kind]()


@functools.lru_cache(maxsize=None)
def norm_case(n, w, state):
    """``(x, state, exact)`` of one case; computed once per process and shared (nothing may write into it)."""
    x = norm_data(n, w)
    st = state_of(state, w)
    want = exact_update(st[0], st[1], st[3], x)
    x.setflags(write=False)
    return x, st, want


# ---- the shape grid of the norm update -----------------------------------------------------------------------------------------------------
WIDTHS = (1, 2, 85, 86, 127, 128, 129, 255, 256, 257, 341, 342, 511, 512, 513, 768, 769, 1023, 1024)
NARROW_WIDTHS = (1, 2, 5, 48)                      # W <= 48: the tile and grid-stride boundaries of the row loop
NARROW_ROWS = (1, 2, 255, 256, 257, 511, 512, 513)
WIDE_ROWS = (1, 7, 8, 9, 257)
GRID_STRIDE_ROWS = (65535, 65536, 65537)           # around ON_MAX_PARTIALS tiles: at W = 5, P = 256 > J = 204
GRID_STRIDE_WIDTHS = (1, 5)
WRAP_WIDTHS = (310, 342)                           # J = 3 and J = 2
WRAP_ROWS = (768, 769, 1025, 1537, 1793)           # P = 3, 4, 5, 7, 8
# widths as 2 … 4 segments, a width-1 segment first and last where there are three
SEGMENTS = {256: (1, 254, 1), 257: (256, 1), 1024: (512, 1, 511), 769: (1, 767, 1), 86: (1, 84, 1), 513: (1, 255, 256, 1), 129: (128, 1)}


def norm_rows_of(w):
    """The row counts of width ``w``: the fixed set of its side of the grid, and one row to either side of a lane's row stride."""
    s = row_stride_of_a_lane(w)
    rows = set(NARROW_ROWS if w <= 48 else WIDE_ROWS) | {s - 1, s, s + 1}
    if w in GRID_STRIDE_WIDTHS:
        rows |= set(GRID_STRIDE_ROWS)
    if w in WRAP_WIDTHS:
        rows |= set(WRAP_ROWS)
    return tuple(sorted(r for r in rows if r >= 1))


def norm_widths():
    return tuple(sorted(set(WIDTHS) | set(NARROW_WIDTHS) | set(WRAP_WIDTHS)))


def norm_shapes():
    """Every ``(n, w)`` of the grid."""
    return tuple((n, w) for w in norm_widths() for n in norm_rows_of(w))


# ---- the error bound of the norm update ---------------------------------------------------------------------------------------------------
U64 = 2.0 ** -53


def norm_bounds(x, state, want):
    """Per column: ``(bound_mean, bound_var, ceil_mean, ceil_var, slop_mean, slop_var)`` as float64 arrays — half a float32 ulp at the
    exact value plus the float64 slop derived in tests/test_obs_norm_edges.py, the 2^-21 ceilings of tests/test_obs_norm.py, and the
    slop alone.  Everything is computed
    from the inputs and the exact reference; nothing here has seen the kernel."""
    x = np.asarray(x, dtype=np.float32)
    n, w = x.shape
    mean, var, count = state[0].astype(np.float64), state[1].astype(np.float64), state[3]
    x64 = x.astype(np.float64)
    D = x64.max(axis=0) - x64.min(axis=0)
    mx, vx, delta, rate = np.abs(want["mx"]), want["vx"], want["delta"], want["rate"]
    e_mx = U64 * ((3 * n + 8) * D + 2 * mx)
    e_vx = U64 * ((16 * n + 32) * D * D + 8 * D * mx)
    if count == 0 and not mean.any():   # a fresh state: rate = 1 and d = mx exactly, so mean' = mx and var' = var + (vx - var)
        slop_mean = e_mx
        slop_var = e_vx + 2 * U64 * (var + vx)
    else:
        slop_mean = rate * e_mx + U64 * (3 * rate * delta + np.abs(mean) + mx)
        slop_var = rate * (e_vx + 3 * delta * (e_mx + slop_mean)) + 8 * U64 * (var + rate * (vx + delta * delta))
    m_q = np.array([abs(float(q)) for q in want["mean_q"]])
    v_q = np.array([abs(float(q)) for q in want["var_q"]])
    with np.errstate(over="ignore", invalid="ignore"):
        half_ulp = lambda a, s: 0.5 * np.spacing((a + s).astype(np.float32)).astype(np.float64)   # (the binade of the far end)
        bound_mean = half_ulp(m_q, slop_mean) + slop_mean
        bound_var = half_ulp(v_q, slop_var) + slop_var
        ceil_mean = 2.0 ** -21 * (m_q + np.sqrt(v_q))
        ceil_var = 2.0 ** -21 * v_q
    return bound_mean, bound_var, ceil_mean, ceil_var, slop_mean, slop_var


# ---- gf_mirror_rows ------------------------------------------------------------------------------------------------------------------------
MIRROR_MAX_WIDTH = 8192     # GF_MIRROR_MAX_WIDTH
MIRROR_MAX_TILE = 64
MIRROR_BLOCK = 256
MIRROR_UNITS = 4            # chunk loads a lane has in flight while staging
MIRROR_WIDTHS = (1, 3, 4, 5, 48, 128, 129, 132, 1024, 1028, 1365, 1366, 2048, 2049, 4096, 4097, 4100, 8191, 8192)
MIRROR_TABLES = ("identity", "reversal", "random")


def mirror_tile(w):
    return min(MIRROR_MAX_TILE, MIRROR_MAX_WIDTH // w)


def mirror_rows_of(w):
    t = mirror_tile(w)
    return tuple(sorted({r for r in (1, t - 1, t, t + 1, 2 * t + 1) if r >= 1}))


def mirror_vectorises(w, row_stride=0):
    """The 16-byte path, the pointers permitting."""
    return w % 4 == 0 and row_stride % 4 == 0


def mirror_tables(kind, w, seed=0):
    """``(perm int32 [w], sign float32 [w])``: the identity, the reversal, or a random signed involution (2-cycles with one sign on
    both ends, fixed points with a sign of their own)."""
    if kind == "identity":
        return np.arange(w, dtype=np.int32), np.ones(w, dtype=np.float32)
    if kind == "reversal":
        return np.arange(w - 1, -1, -1, dtype=np.int32), np.ones(w, dtype=np.float32)
    rng = np.random.default_rng(1009 * seed + w)
    order = rng.permutation(w)
    perm, sign = np.arange(w, dtype=np.int32), np.ones(w, dtype=np.float32)
    pairs = (w - w // 5) // 2
    for a, b in order[:2 * pairs].reshape(-1, 2):
        perm[a], perm[b] = b, a
        sign[a] = sign[b] = rng.choice((-1.0, 1.0))
    for a in order[2 * pairs:]:
        sign[a] = rng.choice((-1.0, 1.0))
    return perm, sign


SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x7F800000, 0xFF800000,
                     0x7F7FFFFF, 0xFF7FFFFF], dtype=np.uint32).view(np.float32)   # ±0, denormals, the least normal, ±inf, ±largest


def mirror_data(rows, w, seed=0):
    """float32 ``[rows, w]``: ordinary values with ±0.0, denormals, ±inf and the largest finite scattered through every row.  No NaN."""
    rng = np.random.default_rng(31 * rows + w + 7919 * seed)
    x = rng.standard_normal((rows, w)).astype(np.float32)
    hit = rng.random((rows, w)) < 0.25
    hit.reshape(-1)[:SPECIALS.size] = True          # every special value is there even in a one-row, narrow case …
    pick = rng.integers(0, SPECIALS.size, size=(rows, w))
    pick.reshape(-1)[:SPECIALS.size] = np.arange(SPECIALS.size)[:pick.size]
    return np.where(hit, SPECIALS[pick], x).astype(np.float32)


def mirror_ref(x, perm, sign):
    """``sign * x[:, perm]`` in float32: an exact product (-0.0 · -1 = +0.0, denormals, ±inf and the largest finite keep their bits up
    to the sign)."""
    with np.errstate(invalid="ignore"):
        return (sign[None, :] * x[:, perm]).astype(np.float32)


def normalise_ref(v, mean, std, eps):
    """``(v - mean) / (std + eps)`` in float32: one subtraction, one addition, one correctly rounded division."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        d = (std + np.float32(eps)).astype(np.float32)
        return ((v - mean[None, :]).astype(np.float32) / d[None, :]).astype(np.float32)


def norm_path_data(rows, w, seed=0):
    """Inputs of the normalised path, no non-finite value among them (``inf - inf`` would make a NaN whose sign is the platform's):
    ordinary columns; columns whose ``std + eps`` is 1e-30, so that quotients overflow to ±inf; columns whose mean is one denormal step
    from the value, so that ``v - mean`` is a denormal.  Returns ``(x, mean, std, eps)``."""
    rng = np.random.default_rng(523 * rows + w + 17 * seed)
    x = (rng.standard_normal((rows, w)) * 3.0 + 1.0).astype(np.float32)
    mean = rng.standard_normal(w).astype(np.float32)
    std = (rng.random(w) + 0.1).astype(np.float32)
    eps = np.float32(1e-30)
    kind = np.arange(w) % 3
    tiny = kind == 1
    std[tiny] = 0.0                                    # std + eps = 1e-30: |v - mean| above 3.4e8 · 1e-30 … overflows
    x[:, tiny] *= np.float32(1e9)
    den = kind == 2
    # values of the least normal binade, mean = the same value a few denormal steps away: the difference is a denormal
    base = (np.uint32(0x00800000) + rng.integers(0, 1 << 20, size=(rows, w)).astype(np.uint32)).view(np.float32)
    x[:, den] = base[:, den]
    mean[den] = (np.uint32(0x00800000) + rng.integers(0, 1 << 20, size=w).astype(np.uint32)).view(np.float32)[den]
    std[den] = 1.0
    return x, mean, std, eps


def i32(a):
    """The bits of a float32 array."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)
