"""gf_mirror_rows through its raw descriptor, over the whole range of its tile plan (cases and the numpy references:
tests/norm_mirror_cases.py).

``tile = min(64, 8192 // width)`` rows per workgroup: the widths run from 1 to 8 192, through the change 64 -> 63 rows at 128 | 129,
tiles of 8, 7, 6, 5, 4, 3 and 2 rows and the one-row tiles of every width above 4 096, on the 16-byte path (up to 2 048 chunks per
row) and on the element path (up to 8 191).  Every source, destination and table is a slice of a sentinel-filled
``tests/guarded.py`` buffer; the stride gaps of a source hold NaN; after every launch the guards are intact and the inputs have kept
their bits.  Every comparison is bit for bit on int32 views (in the normalised path NaN positions, not NaN bits: there the inputs are
chosen so that none arises)."""
import numpy as np
import pytest

import norm_mirror_cases as nm


# ---- CPU: the case module itself -------------------------------------------------------------------------------------------------------------
def test_the_widths_cover_the_tile_plan():
    """From ``tile = min(64, 8192 // w)``, computed here: both sides of every tile count the plan changes at among the widths named
    in the module, every tile of 8 … 1 rows, the largest width, and both paths above 1 024 columns."""
    tile = lambda w: min(nm.MIRROR_MAX_TILE, nm.MIRROR_MAX_WIDTH // w)
    assert all(nm.mirror_tile(w) == tile(w) for w in range(1, nm.MIRROR_MAX_WIDTH + 1))
    widths = set(nm.MIRROR_WIDTHS)
    last_full = nm.MIRROR_MAX_WIDTH // nm.MIRROR_MAX_TILE            # the widest field with 64-row tiles
    assert tile(last_full) == nm.MIRROR_MAX_TILE and tile(last_full + 1) == nm.MIRROR_MAX_TILE - 1 and {last_full, last_full + 1} <= widths
    one_row = nm.MIRROR_MAX_WIDTH // 2                               # above it a tile is one row
    assert tile(one_row) == 2 and tile(one_row + 1) == 1 and {one_row, one_row + 1, nm.MIRROR_MAX_WIDTH - 1, nm.MIRROR_MAX_WIDTH} <= widths
    assert {tile(w) for w in widths} >= set(range(1, 9)) | {nm.MIRROR_MAX_TILE - 1, nm.MIRROR_MAX_TILE}
    for t in (6, 4):                                                 # two more boundaries of the plan inside 1 025 … 8 192
        w = nm.MIRROR_MAX_WIDTH // t
        assert tile(w) == t and tile(w + 1) == t - 1 and {w, w + 1} <= widths
    assert any(tile(w) == 8 for w in widths) and any(tile(w) == 7 and nm.mirror_vectorises(w) for w in widths)
    for w in widths:
        t = tile(w)
        assert {r for r in (1, t - 1, t, t + 1, 2 * t + 1) if r >= 1} == set(nm.mirror_rows_of(w))
    # staging: a lane loads MIRROR_UNITS chunks a pass; more than one pass needs more than 1 024 chunk items in a tile
    items = lambda w: tile(w) * (w // 4 if nm.mirror_vectorises(w) else w)
    assert any(items(w) > nm.MIRROR_BLOCK * nm.MIRROR_UNITS and nm.mirror_vectorises(w) for w in widths)
    assert any(items(w) > nm.MIRROR_BLOCK * nm.MIRROR_UNITS and not nm.mirror_vectorises(w) for w in widths)
    assert any(w // 4 > 256 and nm.mirror_vectorises(w) for w in widths) and nm.MIRROR_MAX_WIDTH - 1 in widths   # 8 191 element chunks


@pytest.mark.parametrize("w", [1, 5, 48, 129, 1028])
def test_reference_is_an_involution_on_its_inputs(w):
    x = nm.mirror_data(7, w)
    for kind in nm.MIRROR_TABLES:
        perm, sign = nm.mirror_tables(kind, w, seed=3)
        assert sorted(perm.tolist()) == list(range(w)) and set(sign.tolist()) <= {1.0, -1.0}
        assert np.array_equal(perm[perm], np.arange(w)) and np.array_equal(sign[perm], sign)
        once = nm.mirror_ref(x, perm, sign)
        assert np.array_equal(nm.i32(nm.mirror_ref(once, perm, sign)), nm.i32(x)), kind
        if kind == "random" and w > 1:
            assert not np.array_equal(nm.i32(once), nm.i32(x))
    assert not np.isnan(x).any() and (nm.i32(x) == np.int32(-2 ** 31)).any()   # -0.0 is there
    if x.size >= nm.SPECIALS.size:
        assert set(nm.SPECIALS.view(np.uint32).tolist()) <= set(x.view(np.uint32).reshape(-1).tolist())   # and every other special value
    # -0.0 · -1 = +0.0, and a denormal, an inf and the largest finite keep their bits up to the sign
    m = nm.mirror_ref(nm.SPECIALS[None, :], np.arange(nm.SPECIALS.size), -np.ones(nm.SPECIALS.size, dtype=np.float32))
    assert np.array_equal(m.view(np.uint32), nm.SPECIALS.view(np.uint32)[None, :] ^ np.uint32(0x80000000))


def test_normalised_path_data_overflows_and_goes_denormal():
    x, mean, std, eps = nm.norm_path_data(9, 129)
    y = nm.normalise_ref(x, mean, std, eps)
    assert np.isfinite(x).all() and not np.isnan(y).any() and np.isinf(y).any()
    assert ((y != 0) & (np.abs(y) < np.finfo(np.float32).tiny)).any(), "no denormal quotient"
    assert (np.isfinite(y) & (np.abs(y) >= 1e-3)).any()


# ---- GPU: the launch -----------------------------------------------------------------------------------------------------------------------------
def _dev_bits(t):
    import torch

    return t.view(torch.int32).cpu().numpy()


class _Field:
    """One field on guarded buffers.  ``stride`` 0: contiguous rows; otherwise the source rows sit ``stride`` floats apart in a
    NaN-filled buffer.  ``src_off`` / ``perm_off``: elements past a 16-byte boundary.  ``joined``: the two destinations are the halves of
    one guarded ``[2·rows, w]`` buffer.  ``copy`` False: ``dst_copy`` is NULL (the buffer exists and must stay untouched)."""

    def __init__(self, x, perm, sign, stride=0, src_off=0, perm_off=0, joined=False, copy=True, norm=None):
        import torch
        from guarded import Guarded

        self.x, self.perm, self.sign, self.stride, self.copy, self.norm = x, perm, sign, stride, copy, norm
        rows, w = x.shape
        self.rows, self.w = rows, w
        full = x
        if stride:
            full = np.full((rows, stride), np.nan, dtype=np.float32)
            full[:, :w] = x
        f32 = lambda a, off=0: Guarded(a.size, torch.float32, "cuda", off=off, init=torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
        self.src = f32(full, src_off)
        self.perm_g = Guarded(w, torch.int32, "cuda", off=perm_off, init=torch.from_numpy(np.ascontiguousarray(perm, dtype=np.int32)))
        self.sign_g = f32(sign)
        self.inputs = [self.src, self.perm_g, self.sign_g]
        if norm is not None:
            self.mean_g, self.std_g = f32(norm[0]), f32(norm[1])
            self.inputs += [self.mean_g, self.std_g]
        if joined:
            self.both = Guarded(2 * rows * w, torch.float32, "cuda")
            self.outs = [self.both]
            self.copy_ptr, self.mirror_ptr = self.both.ptr, self.both.ptr + 4 * rows * w
        else:
            self.dc, self.dm = Guarded(rows * w, torch.float32, "cuda"), Guarded(rows * w, torch.float32, "cuda")
            self.outs = [self.dc, self.dm]
            self.copy_ptr, self.mirror_ptr = self.dc.ptr, self.dm.ptr
        self.joined = joined
        self.before = [g.raw.clone() for g in self.inputs]

    def fill(self, f):
        f.src, f.width, f.row_stride = self.src.ptr, self.w, self.stride
        f.dst_copy = self.copy_ptr if self.copy else None
        f.dst_mirror = self.mirror_ptr
        f.perm, f.sign = self.perm_g.ptr, self.sign_g.ptr
        if self.norm is not None:
            f.in_mean, f.in_std, f.in_eps = self.mean_g.ptr, self.std_g.ptr, float(self.norm[2])

    def check_silence(self, what):
        import torch

        for g in self.outs:
            assert g.guards_ok(), f"{what}: wrote outside a destination"
        for g, b in zip(self.inputs, self.before):
            assert torch.equal(g.raw, b), f"{what}: an input buffer (or its guards) changed"
        if not self.copy:
            assert not self.joined and self.dc.untouched(), f"{what}: dst_copy is NULL, yet the copy buffer was written"

    def result(self):
        """(copy bits or None, mirror bits), ``[rows, w]`` int32 each."""
        if self.joined:
            both = _dev_bits(self.both.t).reshape(2, self.rows, self.w)
            return both[0], both[1]
        return (_dev_bits(self.dc.t).reshape(self.rows, self.w) if self.copy else None), _dev_bits(self.dm.t).reshape(self.rows, self.w)

    def want(self):
        mirrored = nm.mirror_ref(self.x, self.perm, self.sign)
        if self.norm is None:
            return nm.i32(self.x), nm.i32(mirrored)
        return nm.i32(nm.normalise_ref(self.x, *self.norm)), nm.i32(nm.normalise_ref(mirrored, *self.norm))


def _launch(backend, fields, scalars=(), rows=None, what=""):
    """One gf_mirror_rows; ``scalars``: numpy ``[rows]`` arrays, each with a destination guarded at exactly ``2·rows``.  Returns the
    scalar destinations' bits."""
    import torch
    from genesis_forge_amd import _native as nat
    from guarded import Guarded, raw_call

    rows = fields[0].rows if rows is None else rows
    a = nat.GfMirrorRowsArgs()
    a.num_rows, a.num_fields, a.num_scalars = rows, len(fields), len(scalars)
    for f, d in zip(a.fields, fields):
        assert d.rows == rows
        d.fill(f)
    srcs, dsts = [], []
    for s, v in zip(a.scalars, scalars):
        src = Guarded(rows, torch.float32, "cuda", init=torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)))
        dst = Guarded(2 * rows, torch.float32, "cuda")
        s.src, s.dst = src.ptr, dst.ptr
        srcs.append((src, src.raw.clone())), dsts.append(dst)
    assert raw_call(backend, "mirror_rows", a) == 0, what
    torch.cuda.synchronize()
    for d in fields:
        d.check_silence(what)
    for (src, before), dst in zip(srcs, dsts):
        assert dst.guards_ok() and torch.equal(src.raw, before), f"{what}: a scalar wrote outside its 2·rows or changed its source"
    return [_dev_bits(d.t) for d in dsts]


def _run(backend, x, perm, sign, what, **kw):
    f = _Field(x, perm, sign, **kw)
    _launch(backend, [f], what=what)
    got, want = f.result(), f.want()
    if got[0] is not None:
        assert np.array_equal(got[0], want[0]), f"{what}: the copy half differs"
    assert np.array_equal(got[1], want[1]), f"{what}: the mirror half differs"
    return got


# ---- GPU: every width, row count and table ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w", nm.MIRROR_WIDTHS)
def test_every_width_rows_and_table_bit_for_bit(hip_backend, w):
    """rows in {1, tile - 1, tile, tile + 1, 2·tile + 1} x identity / reversal / random signed involution, two guarded destinations; the
    largest row count once more into the two halves of one guarded ``[2·rows, w]`` tensor and once with ``dst_copy == NULL``."""
    for rows in nm.mirror_rows_of(w):
        x = nm.mirror_data(rows, w)
        for kind in nm.MIRROR_TABLES:
            perm, sign = nm.mirror_tables(kind, w, seed=rows)
            got = _run(hip_backend, x, perm, sign, f"w={w} rows={rows} {kind}")
            if kind == "identity":
                assert np.array_equal(got[1], nm.i32(x))
    zero = nm.i32(x) == np.int32(-2 ** 31)   # -0.0 under sign -1 is +0.0
    flip = zero[:, perm] & (sign[None, :] < 0)
    assert (got[1][flip] == 0).all() and (w < 5 or rows < 3 or flip.any())
    assert np.array_equal(_run(hip_backend, x, perm, sign, f"w={w} rows={rows} joined halves", joined=True)[1], got[1])
    alone = _run(hip_backend, x, perm, sign, f"w={w} rows={rows} dst_copy NULL", copy=False)
    assert alone[0] is None and np.array_equal(alone[1], got[1])


@pytest.mark.gpu
@pytest.mark.parametrize("w", [1028, 4100])
def test_the_element_path_forced_three_ways_equals_the_vector_path(hip_backend, w):
    assert nm.mirror_vectorises(w)
    rows = 2 * nm.mirror_tile(w) + 1
    x = nm.mirror_data(rows, w, seed=1)
    perm, sign = nm.mirror_tables("random", w, seed=5)
    vec = _run(hip_backend, x, perm, sign, f"w={w} vector path")
    for what, kw in (("src 4 bytes off", dict(src_off=1)), ("perm 4 bytes off", dict(perm_off=1)), ("row_stride % 4 != 0", dict(stride=w + 1)),
                     ("row_stride % 4 == 0, strided vector path", dict(stride=w + 4))):
        got = _run(hip_backend, x, perm, sign, f"w={w} {what}", **kw)
        assert np.array_equal(got[0], vec[0]) and np.array_equal(got[1], vec[1]), what


@pytest.mark.gpu
@pytest.mark.parametrize("w", [129, 2049, 8192])
def test_strided_sources_with_nan_gaps(hip_backend, w):
    rows = 2 * nm.mirror_tile(w) + 1
    x = nm.mirror_data(rows, w, seed=2)
    for kind in ("reversal", "random"):
        perm, sign = nm.mirror_tables(kind, w, seed=7)
        base = _run(hip_backend, x, perm, sign, f"w={w} contiguous")
        for stride in (w + 3, 4 * w):
            got = _run(hip_backend, x, perm, sign, f"w={w} row_stride={stride}", stride=stride)
            assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])


# ---- GPU: the normalised path -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w", [3, 4, 129, 1028, 4097])
def test_the_normalised_path_is_float32_numpy_bit_for_bit(hip_backend, w):
    """``(v - mean[j]) / (std[j] + eps)`` at the destination column j — one subtraction, one addition, one correctly rounded division —
    on ordinary columns, on columns with ``std + eps`` = 1e-30 (quotients overflow to ±inf) and on columns where ``v - mean`` is a
    denormal (and so is the quotient).  Both halves against float32 numpy, NaN positions compared as positions (none arises)."""
    rows = 2 * nm.mirror_tile(w) + 1
    x, mean, std, eps = nm.norm_path_data(rows, w)
    perm, sign = nm.mirror_tables("random", w, seed=9)
    f = _Field(x, perm, sign, norm=(mean, std, eps))
    _launch(hip_backend, [f], what=f"normalised w={w}")
    got, want = f.result(), f.want()
    for half, g, wt in (("copy", got[0], want[0]), ("mirror", got[1], want[1])):
        gf, wf = g.view(np.float32), wt.view(np.float32)
        assert np.array_equal(np.isnan(gf), np.isnan(wf)), f"{half}: NaN positions"
        bad = (g != wt) & ~np.isnan(wf)
        if bad.any():
            r, c = np.argwhere(bad)[0]
            v = x[r, c] if half == "copy" else nm.mirror_ref(x, perm, sign)[r, c]
            raise AssertionError(f"{half} half, {int(bad.sum())} elements differ; first at [{r}, {c}]: v = {v!r} ({nm.i32(np.float32(v))!r}), mean = {mean[c]!r}, "
                                 f"std = {std[c]!r}, eps = {eps!r}: kernel {gf[r, c]!r}, numpy {wf[r, c]!r}")
    yc = nm.normalise_ref(x, mean, std, eps)
    assert np.isinf(yc).any() and ((yc != 0) & (np.abs(yc) < np.finfo(np.float32).tiny)).any()
    at_source = nm.mirror_ref(yc, perm, sign)   # what normalising at the SOURCE column perm[j] would give
    assert not np.array_equal(nm.i32(at_source), got[1]), "normalised at the destination, not the source, column"


# ---- GPU: one launch, fields of different tile counts, scalars ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_four_fields_of_different_tile_counts_and_four_scalars_in_one_launch(hip_backend):
    """rows = 130: 3 tiles of the 48-wide field, 19 of the 1 028-wide one and 130 one-row tiles of the 4 097- and 8 192-wide ones — most
    workgroups of the narrow fields' grid rows leave at once — and the scalars' single workgroup."""
    rows = 130
    widths = (48, 1028, 4097, 8192)
    assert len({-(-rows // nm.mirror_tile(w)) for w in widths}) == 3
    rng = np.random.default_rng(11)
    fields = []
    for i, w in enumerate(widths):
        perm, sign = nm.mirror_tables("random", w, seed=20 + i)
        fields.append(_Field(nm.mirror_data(rows, w, seed=3 + i), perm, sign, joined=i % 2 == 1))
    scalars = [rng.standard_normal(rows).astype(np.float32) for _ in range(4)]
    souts = _launch(hip_backend, fields, scalars, what="four fields")
    for f in fields:
        got, want = f.result(), f.want()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f.w
    for v, got in zip(scalars, souts):
        assert np.array_equal(got, nm.i32(np.concatenate([v, v])))


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1023, 1024, 1025])
def test_scalars_alone_around_one_workgroup_of_1024(hip_backend, rows):
    rng = np.random.default_rng(rows)
    scalars = [rng.standard_normal(rows).astype(np.float32) for _ in range(4)]
    scalars[1][:nm.SPECIALS.size] = nm.SPECIALS
    souts = _launch(hip_backend, [], scalars, rows=rows, what=f"scalars, {rows} rows")
    for i, (v, got) in enumerate(zip(scalars, souts)):
        assert np.array_equal(got[:rows], nm.i32(v)), f"scalar {i}: first half"
        assert np.array_equal(got[rows:], nm.i32(v)), f"scalar {i}: second half"
