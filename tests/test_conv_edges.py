"""gf_conv_encode and gf_conv_encode_banded through their raw descriptors, each against torch's float64 conv2d / elu / linear on its own
(cases, reference, data and buffers: tests/conv_cases.py).  No test here compares one form only with the other; where both are at
hand their bit-equality is asserted on top.

What the shapes reach:
  k7        dy, dx = 6, the top of the table word's 3-bit fields; stride 3; padding = kernel - 1; K = 49 (three whole chunks and a tail of one)
  low       an image lower than the kernel: two of the three tap rows are padding for every output
  c64       two full conv column blocks with K = 576; flat = 1024 (4 slabs, k1 == K on a slab border); four head blocks per wave; T = 7
  K1 … K48  the conv k loop's exits and prefetch guards: less than a chunk, a quad, one whole chunk, a chunk and one, a chunk and a
            quad, three whole chunks
  flat128 / 256 / 512   `flat` a multiple of the head's chunk and slab, head_nb 1, 2, 3, a latent one (five) past a 32-column block
  three     three layers, the middle activation (64 x 7 x 5) sizing a buffer, padding 4 of 5, stride 3 between strides of 1
  o33       a second conv column block with one live column; three latent blocks, so the fourth head wave has none
  depth     the 58 x 87 camera, the one shape that the plan bands by itself (R < 13)

Pruning.  Tile form: every N of {1, T-1, T, T+1, 2T+1} — five launches per shape, nothing pruned.  Banded form, of the product
band_rows {1, 2, h-1, h} x tile_envs {the plan's, 5, 32} x N {1, 31, 32, 33, 65} per shape: every N at (the second band setting,
tile_envs 5); every band setting at (the plan's tile, N = 33); tile_envs 32 at (the full band, N = 33) — at most ten launches.
Where the plan refuses a forced tile of 32 (c64: 7, three: 5, flat512: 15, o33: 30, flat256: 31) the largest tile it accepts is forced
instead.  N = 31 / 33 / 65 end
inside a 32-row block of the head while tiles of 5, 7 or the plan's end elsewhere.

Every launch of a shape asserts: GF_OK; torch.equal with the float64 reference; the guards of `out` and `feat`; no NaN left in `out`
(it starts as NaN, as `feat` does); banded only, feat[:N] equal to the reference's last activation."""
import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc
from genesis_forge_amd import _native as nat

FORMS = ("tile", "banded")
U = 2.0 ** -24


def _check(l, backend, want, what, last_act=None, prefix=None):
    assert l.run(backend) == cc.GF_OK, what
    got = l.result()
    assert not bool(torch.isnan(got).any()), f"{what}: an element of out was not written"
    if prefix is not None:
        assert torch.equal(got[:, :l.w1], prefix), f"{what}: the 1-D columns"
    bad = (got[:, l.w1:] != want.float()).nonzero()
    assert bad.numel() == 0, f"{what}: {len(bad)} elements differ from float64, first at {bad[0].tolist()}"
    assert l.out.guards_ok(), f"{what}: wrote outside out"
    assert l.feat.guards_ok(), f"{what}: wrote outside feat"
    if l.form == "banded":
        assert torch.equal(l.features(), last_act.flatten(1).float()), f"{what}: feat"
    else:
        assert bool(torch.isnan(l.feat.cpu()).all()), f"{what}: the tile form touched feat"
    return got


def _banded_runs(case):
    """(band_rows, tile_envs, n) of the module docstring's pruning."""
    bands = cc.band_settings(case)
    h = bands[-1]
    second = bands[min(1, len(bands) - 1)]
    runs = [(second, cc.forced_tile(case, second, 5), n) for n in (1, 31, 32, 33, 65)]
    runs += [(r, 0, 33) for r in bands]
    runs.append((h, cc.forced_tile(case, h, 32), 33))
    return runs


# ---- every shape, each form against float64 --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", cc.SHAPES, ids=lambda c: c.id)
def test_tile_form_is_exact_at_every_tile_edge(hip_backend, case):
    params, image, out, _acts = cc.exact_data(case)
    T = cc.tile_plan(case)[0]
    for n in sorted({1, T - 1, T, T + 1, 2 * T + 1} - {0}):
        _check(cc.Launch(case, params, image[:n], "cuda"), hip_backend, out[:n], f"{case.id} tile N={n} T={T}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", cc.SHAPES, ids=lambda c: c.id)
def test_banded_form_is_exact_at_every_band_tile_and_block_edge(hip_backend, case):
    params, image, out, acts = cc.exact_data(case)
    for band_rows, tile_envs, n in _banded_runs(case):
        plan = cc.banded_plan(case, band_rows, tile_envs)
        assert plan is not None and plan[1] == band_rows and (tile_envs == 0 or plan[0] == tile_envs)
        l = cc.Launch(case, params, image[:n], "cuda", form="banded", band_rows=band_rows, tile_envs=tile_envs)
        _check(l, hip_backend, out[:n], f"{case.id} banded R={band_rows} T={plan[0]} N={n}", acts[-1][:n])


@pytest.mark.gpu
def test_the_depth_camera_is_exact_in_the_plans_own_bands(hip_backend):
    case = cc.DEPTH
    params, image, out, acts = cc.exact_data(case, 3)
    T, R, bands, _lds, _flat = cc.banded_plan(case)
    assert R < cc.last_height(case) and bands > 1
    _check(cc.Launch(case, params, image, "cuda", form="banded"), hip_backend, out, f"depth banded R={R} T={T}", acts[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["three", "o33"])
def test_a_padded_image_and_strided_normalised_columns(hip_backend, name, form):
    """image_stride > C·H·W, one segment with row_stride > width and one contiguous, a normaliser, every input buffer off alignment:
    the gaps and the surroundings read as 3.4e38."""
    case = cc.BY_ID[name]
    params, image, out, acts = cc.exact_data(case)
    n, S = 33, image.shape[1]
    g = torch.Generator().manual_seed(11)
    s0, s1 = torch.randn(n, 5, generator=g), torch.randn(n, 2, generator=g)
    mean, std, eps = torch.randn(7, generator=g), torch.rand(7, generator=g) + 0.1, 1e-2
    kwargs = dict(form=form, image_stride=S + 3, segs=[(s0, 9), (s1, 0)], norm=(mean, std, eps), offs=dict(image=1, seg0=3, seg1=2, mean=1, std=2))
    if form == "banded":
        kwargs.update(band_rows=cc.band_settings(case)[0], tile_envs=3)
    l = cc.Launch(case, params, image[:n], "cuda", **kwargs)
    assert l.enc.image_stride > S and l.enc.inputs[0].row_stride > l.enc.inputs[0].width
    _check(l, hip_backend, out[:n], f"{name} {form} padded", acts[-1][:n], prefix=cc.columns((s0, s1), mean, std, eps))
    plain = cc.Launch(case, params, image[:n], "cuda", **dict(kwargs, norm=None, offs=dict(image=1, seg0=3, seg1=2)))   # no normaliser: copied
    _check(plain, hip_backend, out[:n], f"{name} {form} padded, copied", acts[-1][:n], prefix=torch.cat((s0, s1), dim=1))


# ---- alignment -------------------------------------------------------------------------------------------------------------------------
def _offsets(case, form):
    layers = range(len(case.channels))
    one = [{f"w{l}": o} for l in layers for o in (1, 2, 3)] + [dict(head_w=1), dict(image=1), dict(out=1)]
    everything = dict({f"w{l}": 3 for l in layers}, head_w=1, image=1, out=1, head_b=1, **{f"b{l}": 1 for l in layers})
    if form == "banded":
        one.append(dict(feat=1))
        everything["feat"] = 1
    return one + [everything]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["K16", "c64", "flat256"])
def test_misaligned_buffers_give_the_same_bits(hip_backend, name, form):
    """K % 4 == 0 and flat % 4 == 0 in all three: aligned, the layers and the head read 16 bytes at a time; 4, 8 or 12 bytes off they
    must fall back to the by-element path (the banded head for `feat` too) and give the same bits."""
    case = cc.BY_ID[name]
    params, image, out, acts = cc.exact_data(case)
    n = 33 if form == "banded" else cc.tile_plan(case)[0] + 1
    aligned = cc.Launch(case, params, image[:n], "cuda", form=form)
    assert all(b.ptr % 16 == 0 for b in aligned.bufs.values()) and aligned.out.ptr % 16 == 0 and aligned.feat.ptr % 16 == 0
    base = _check(aligned, hip_backend, out[:n], f"{name} {form} aligned", acts[-1][:n])
    for offs in _offsets(case, form):
        l = cc.Launch(case, params, image[:n], "cuda", form=form, offs=offs)
        for key, o in offs.items():
            buf = l.out if key == "out" else l.feat if key == "feat" else l.bufs[key]
            assert buf.ptr % 16 == 4 * o
        got = _check(l, hip_backend, out[:n], f"{name} {form} offsets {offs}", acts[-1][:n])
        assert torch.equal(got, base)


# ---- ELU's negative branch, element by element -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["k7", "o33"])
def test_elu_element_by_element_through_a_selector_head(hip_backend, name, form):
    """The head's row j holds a single 1 at flat index perm[j] and no bias: out[n, j] IS the stored activation at that index (1·x plus
    exact zeros), so a value at a wrong address shows as a wrong element.  Integer pre-activations: the non-negative ones must come back
    exactly; the negative ones within 4U relative of float64's expm1 — test_log_std's rule for a HIP float32 exponential: one float32
    ulp (up to 2U relative) documented for the device function, the rounding of the reference to float32 and 1U of slack."""
    case = cc.BY_ID[name]
    wt, b, image, pre, perm = cc.elu_data(case)
    flat, n = pre.shape[1], image.shape[0]
    want_all = F.elu(pre)
    assert 0.3 < float((pre < 0).float().mean()) < 0.7 and bool((pre == 0).any())
    seen, worst = torch.zeros(flat, dtype=torch.bool), 0.0
    for start in range(0, flat, nat.GF_CONV_MAX_LATENT):
        sel, params, idx = cc.selector(case, wt, b, perm, start)
        kwargs = dict(form="banded", band_rows=2, tile_envs=4) if form == "banded" else {}
        l = cc.Launch(sel, params, image, "cuda", **kwargs)
        assert l.run(hip_backend) == cc.GF_OK
        got, want, p = l.result().double(), want_all[:, idx], pre[:, idx]
        assert l.out.guards_ok() and l.feat.guards_ok() and not bool(torch.isnan(got).any())
        assert torch.equal(got[p >= 0], want[p >= 0]), f"{name} {form}: a non-negative activation is not the pre-activation"
        neg = p < 0
        spacing = torch.where(want[neg].abs() >= 0.5, U, U / 2)   # float32 spacing in [0.5, 1) and below: expm1 of an integer <= -1 is in (-1, -0.63]
        worst = max(worst, float(((got[neg] - want[neg]).abs() / spacing).max()))
        err = (got[neg] - want[neg]).abs()
        assert bool((err <= 4 * U * want[neg].abs()).all()), f"{name} {form}: expm1 off by {float((err / want[neg].abs()).max() / U):.2f} U"
        if form == "banded":
            assert torch.equal(l.features().double()[pre >= 0], want_all[pre >= 0])
        seen[idx] = True
    assert bool(seen.all())
    print(f"ELU {name} {form}: largest distance of a negative activation to float64's expm1 {worst:.2f} ulp")


# ---- refusals and the empty call ---------------------------------------------------------------------------------------------------------
def _clauses(table):
    return [pytest.param(form, apply, id=f"{form}-{name}") for name, forms, apply in table for form in forms]


@pytest.mark.parametrize("form,apply", _clauses(cc.RANGE_CLAUSES))
def test_the_plan_entry_refuses_each_range_clause(form, apply):
    args = cc.shape_args(cc.BASE, 3, form, widths=cc.BASE_WIDTHS)
    assert cc.plan_status(args) == cc.GF_OK
    apply(args)
    assert cc.plan_status(args) == cc.GF_E_RANGE


@pytest.mark.gpu
@pytest.mark.parametrize("num_envs", [3, 0], ids=["N=3", "N=0"])
@pytest.mark.parametrize("form,apply", _clauses(cc.RANGE_CLAUSES))
def test_the_launch_entry_refuses_each_range_clause_and_writes_nothing(hip_backend, form, apply, num_envs):
    """Valid pointers, one bad shape field: GF_E_RANGE — with num_envs == 0 too: the shape is judged first."""
    l = cc.base_launch("cuda", form)
    l.enc.num_envs = num_envs
    apply(l.args)
    assert l.run(hip_backend) == cc.GF_E_RANGE
    assert l.out.untouched() and l.feat.untouched()


@pytest.mark.gpu
@pytest.mark.parametrize("num_envs", [3, 0], ids=["N=3", "N=0"])
@pytest.mark.parametrize("form,apply", _clauses(cc.NULL_CLAUSES))
def test_the_launch_entry_refuses_each_missing_pointer_and_writes_nothing(hip_backend, form, apply, num_envs):
    """A valid shape, one pointer NULL: GF_E_NULL — with num_envs == 0 too: the pointers are judged before the empty call returns."""
    l = cc.base_launch("cuda", form)
    l.enc.num_envs = num_envs
    apply(l.args)
    assert l.run(hip_backend) == cc.GF_E_NULL
    assert l.out.untouched() and l.feat.untouched()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_a_bad_shape_wins_over_a_missing_pointer_and_the_empty_call_writes_nothing(hip_backend, form):
    l = cc.base_launch("cuda", form)
    l.enc.num_envs = 0
    assert l.run(hip_backend) == cc.GF_OK and l.out.untouched() and l.feat.untouched()
    l.enc.image = None
    l.enc.latent_dim = 0
    assert l.run(hip_backend) == cc.GF_E_RANGE and l.out.untouched() and l.feat.untouched()
    l.enc.latent_dim = cc.BASE.latent
    assert l.run(hip_backend) == cc.GF_E_NULL
    l.enc.image = l.bufs["image"].ptr
    l.enc.num_envs = 3   # the same descriptor, whole again, runs
    params, image, out, acts = cc.exact_data(cc.BASE)
    assert l.run(hip_backend) == cc.GF_OK and torch.equal(l.result()[:, l.w1:], out[:3].float()) and l.out.guards_ok() and l.feat.guards_ok()
