"""gf_minibatch_gather at every tile of its launch plan, with ragged last tiles.

The host halves the tile from 256 rows while ``num_rows < tile * 1024``, down to 16 (csrc/gf_minibatch.hip): 16 below 32 768 rows, 32
below 65 536, 64 below 131 072, 128 below 262 144, 256 from there on.  The row counts here sit one row to either side of each
threshold, so every tile runs with a last tile of one row and with one of ``tile - 1`` rows, in the plain kernel (4-, 8- and 16-byte
chunks, one field normalised) and in the history kernel.  The reference is torch indexing (test_frame_rollout._rows_of), NaN rows where
the index is out of range; every destination has fill columns around the field and guard rows in front of row 0 and behind the last."""
import pytest
import torch

from test_frame_rollout import _ints, _rows_of, _same

ROWS = [32767, 32769, 65535, 65537, 131071, 131073, 262143, 262145]
EXTRA_ROWS = [17, 262399]    # tile 16 with a one-row last tile, tile 256 with one of 255 rows: the two the thresholds cannot give
T, N = 27, 37                # num_src_rows = 999
FILL, GUARD_ROWS = -3.0, 4   # (4 rows of any width keep the destination's 16-byte alignment)
EPS = 0.01


def _tile(rows):
    tile = 256
    while tile > 16 and rows < tile * 1024:
        tile //= 2
    return tile


def _last(rows):
    return rows - (-(-rows // _tile(rows)) - 1) * _tile(rows)


def test_tile_plan_on_known_values():
    known = {32767: 16, 32768: 32, 65535: 32, 65536: 64, 131071: 64, 131072: 128, 262143: 128, 262144: 256}
    assert {r: _tile(r) for r in known} == known
    assert _tile(1) == 16 and _tile(24576) == 16 and _tile(1048573) == 256


def test_rows_reach_every_tile_with_both_ragged_ends():
    seen = {(_tile(r), _last(r)) for r in ROWS + EXTRA_ROWS}
    assert seen >= {(t, k) for t in (16, 32, 64, 128, 256) for k in (1, t - 1)}, sorted(seen)
    assert {(_tile(r), _last(r)) for r in ROWS} >= {(t, k) for t in (32, 64, 128) for k in (1, t - 1)} | {(16, 15), (256, 1)}
    before = {_tile(r) for r in (1, 17, 255, 300, 1000, 4133, 8192, 1048573)}
    assert before == {16, 256}, "the tiles the suite reached before this file"


def _indices(rows, src_rows, g):
    """Random rows; -1 and ``src_rows`` in row 0, the last row and the rows tile - 1 and tile."""
    idx = torch.randint(0, src_rows, (rows,), generator=g)
    tile = _tile(rows)
    for at, bad in {tile - 1: src_rows, tile: -1, 0: -1, rows - 1: src_rows}.items():
        idx[at] = bad
    return idx


def test_indices_carry_the_out_of_range_rows():
    g = torch.Generator().manual_seed(0)
    for rows in ROWS + EXTRA_ROWS:
        idx, tile = _indices(rows, T * N, g), _tile(rows)
        bad = ((idx < 0) | (idx >= T * N)).nonzero()[:, 0].tolist()
        assert bad == sorted({0, tile - 1, tile, rows - 1}), rows
        assert {int(idx[i]) for i in bad} == {-1, T * N}


class _Dst:
    """``[rows, width]`` behind GUARD_ROWS fill rows and in front of as many; the field occupies ``[col, col + w)``."""

    def __init__(self, rows, width, col, w):
        self.buf = torch.full((GUARD_ROWS + rows + GUARD_ROWS, width), FILL, device="cuda")
        self.rows, self.width, self.col, self.w = rows, width, col, w
        self.t = self.buf[GUARD_ROWS:GUARD_ROWS + rows]

    def check(self, want, tag):
        assert _same(self.t[:, self.col:self.col + self.w], want), ("values", tag)
        assert bool((self.t[:, :self.col] == FILL).all()) and bool((self.t[:, self.col + self.w:] == FILL).all()), ("a column beside the field", tag)
        assert bool((self.buf[:GUARD_ROWS] == FILL).all()) and bool((self.buf[GUARD_ROWS + self.rows:] == FILL).all()), ("a guard row", tag)


def _launch(backend, rows, idx, fields):
    """``fields``: (src, dst, history_len, normaliser or None)."""
    from genesis_forge_amd import _native as nat

    a = nat.GfMinibatchArgs()
    a.num_rows, a.num_src_rows, a.indices, a.num_fields = rows, T * N, idx.data_ptr(), len(fields)
    for f, (src, dst, H, norm) in zip(a.fields, fields):
        f.src, f.dst, f.src_width, f.dst_width, f.dst_col = src.data_ptr(), dst.t.data_ptr(), src.shape[1], dst.width, dst.col
        f.history_len, f.frame_stride_rows = H, N if H > 1 else 0
        if norm is not None:
            f.mean, f.std, f.eps = norm[0].data_ptr(), norm[1].data_ptr(), EPS
    backend.minibatch_gather(a)


def _chunk_bytes(src, dst, H):
    """field_vec restated: the widest chunk the field's pointers, widths, column and frame stride allow."""
    p = src.data_ptr() | dst.t.data_ptr()
    w = src.shape[1] | dst.width | dst.col | (N * src.shape[1] if H > 1 else 0)
    return 16 if p % 16 == 0 and w % 4 == 0 else 8 if p % 8 == 0 and w % 2 == 0 else 4


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROWS + EXTRA_ROWS)
def test_plain_kernel_tiles_hip(hip_backend, rows):
    g = torch.Generator().manual_seed(rows)
    S = T * N
    idx = _indices(rows, S, g).cuda()
    valid = (idx >= 0) & (idx < S)
    s3, s4, s2 = _ints((S, 3), g, "cuda"), _ints((S, 4), g, "cuda"), _ints((S, 2), g, "cuda")
    norm = (_ints((4,), g, "cuda"), (torch.rand(4, generator=g) + 0.5).cuda())
    d3, d4, d2 = _Dst(rows, 5, 1, 3), _Dst(rows, 8, 4, 4), _Dst(rows, 4, 2, 2)
    assert [_chunk_bytes(s, d, 0) for s, d in ((s3, d3), (s4, d4), (s2, d2))] == [4, 16, 8]
    _launch(hip_backend, rows, idx, [(s3, d3, 0, None), (s4, d4, 0, norm), (s2, d2, 0, None)])
    d3.check(_rows_of(s3, idx, 1, N, valid), (rows, "width 3"))
    d4.check((_rows_of(s4, idx, 1, N, valid) - norm[0]) / (norm[1] + EPS), (rows, "width 4, normalised"))
    d2.check(_rows_of(s2, idx, 1, N, valid), (rows, "width 2"))
    assert int((~valid).sum()) == len({0, _tile(rows) - 1, _tile(rows), rows - 1}) and bool(torch.isnan(d4.t[~valid][:, 4:]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROWS + EXTRA_ROWS)
def test_history_kernel_tiles_hip(hip_backend, rows):
    g = torch.Generator().manual_seed(rows + 1)
    S = T * N
    idx = _indices(rows, S, g).cuda()
    valid = (idx >= 0) & (idx < S)
    fa, fb, plain = _ints(((T + 2) * N, 5), g, "cuda"), _ints(((T + 3) * N, 4), g, "cuda"), _ints((S, 3), g, "cuda")
    da, db, dp = _Dst(rows, 12, 1, 10), _Dst(rows, 16, 4, 12), _Dst(rows, 5, 1, 3)
    assert [_chunk_bytes(s, d, H) for s, d, H in ((fa, da, 2), (fb, db, 3), (plain, dp, 0))] == [4, 16, 4]
    _launch(hip_backend, rows, idx, [(fa, da, 2, None), (fb, db, 3, None), (plain, dp, 0, None)])
    da.check(_rows_of(fa, idx, 2, N, valid), (rows, "H = 2, O = 5"))
    db.check(_rows_of(fb, idx, 3, N, valid), (rows, "H = 3, O = 4"))
    dp.check(_rows_of(plain, idx, 1, N, valid), (rows, "plain"))
