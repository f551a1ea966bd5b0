"""Shapes, the float64 reference, the raw descriptors and the data of tests/test_conv_edges.py: gf_conv_encode (csrc/gf_conv.hip) and
gf_conv_encode_banded (csrc/gf_conv_banded.hip) through their C ABI.

Reference: torch on the CPU in float64 — conv2d, elu, flatten, linear (``reference``); the 1-D columns follow the float32 rule
``(x - mean) / (std + eps)`` bit for bit (``columns``).  Nothing here is the other form of the kernel.

Signed-exact data (``exact_data``).  Conv and head weights are in {-1, 0, 1}, the image in {0 … vmax}, the head bias in {-3 … 3}; the
bias of conv output channel j is (the count of its -1 weights) x (the largest input value of that layer in the reference), the integer
that keeps every pre-activation >= 0: ELU is the identity and expm1f(0) == 0 on both of its branches.  While for every output element
of every layer ``|bias| + Σ|w·x| < 2^24`` (``exact_margin``, asserted for every case without a GPU), every partial sum of the kernel's
k-ascending fma chain is an integer below 2^24, so the float32 result is the float64 one: ``torch.equal`` is the check.  ``vmax`` and
the weights' density are per case so that the reference alone meets the condition.  One batch of ``NMAX`` envs is drawn per case and
its reference computed once; a run of n envs uses the first n rows of both.

Buffers (``Launch``).  Every array the descriptor names is a tests/guarded.py buffer with its own element offset.  guarded's sentinel
byte 0xA5 reads as the float -2.9e-16, which an integer sum swallows, so the bytes around (and in the row gaps of) every INPUT are
overwritten with 0x7F — the float 3.4e38 at any byte phase: one element read outside an input and not selected away shows in the
result.  Outputs keep guarded's sentinel and are checked with ``guards_ok`` / ``untouched``; ``out`` and ``feat`` start as NaN."""
import ctypes as C
import functools
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as F

import guarded
from genesis_forge_amd import _native as nat

GF_OK, GF_E_NULL, GF_E_RANGE = 0, -1, -2   # include/gf_step.h
NMAX = 65
LIMIT = 2.0 ** 24
INPUT_GUARD = 0x7F
KC, SLAB = 16, 256   # csrc/gf_conv.hip: kConvKC; csrc/gf_conv_banded.hip: kHeadSlab

Case = namedtuple("Case", "id image channels kernel stride padding latent vmax density")


def _case(id, image, channels, kernel, stride, padding, latent, vmax=2, density=2 / 3):
    n = len(channels)
    per = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v,) * n
    return Case(id, tuple(image), tuple(channels), per(kernel), per(stride), per(padding), latent, vmax, density)


# id | image (C, H, W) | channels | kernel | stride | padding | latent       (what each reaches: tests/test_conv_edges.py's docstring)
SHAPES = [
    _case("k7", (1, 9, 8), (5,), 7, 3, 6, 7),
    _case("low", (1, 1, 9), (3,), 3, 1, 2, 4),
    _case("c64", (64, 4, 4), (64,), 3, 1, 1, 512),
    _case("K1", (1, 3, 5), (2,), 1, 1, 0, 3),
    _case("K4", (1, 4, 5), (3,), 2, 1, 0, 3),
    _case("K16", (4, 4, 3), (5,), 2, 1, 0, 3),
    _case("K17", (17, 2, 3), (2,), 1, 1, 0, 3),
    _case("K20", (5, 3, 4), (3,), 2, 1, 0, 3),
    _case("K48", (3, 5, 6), (4,), 4, 1, 0, 3),
    _case("flat128", (1, 8, 16), (1,), 1, 1, 0, 5),
    _case("flat256", (1, 16, 16), (1,), 1, 1, 0, 129),
    _case("flat512", (2, 16, 16), (2,), 1, 1, 0, 257),
    _case("three", (2, 13, 9), (3, 64, 2), (3, 5, 3), (1, 3, 1), (2, 4, 0), 40, vmax=1, density=0.4),
    _case("o33", (3, 7, 6), (33,), 5, 2, 2, 96),
]
BY_ID = {c.id: c for c in SHAPES}
DEPTH = _case("depth", (1, 58, 87), (16, 32), (5, 3), 2, 0, 64, vmax=1, density=0.5)   # test_conv_banded.DEPTH
K_OF = dict(K1=1, K4=4, K16=16, K17=17, K20=20, K48=48)


def layer_shapes(case):
    """Per layer (cin, hin, win, cout, k, s, p, hout, wout, K), torch's Conv2d arithmetic."""
    c, h, w = case.image
    rows = []
    for o, k, s, p in zip(case.channels, case.kernel, case.stride, case.padding):
        ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        rows.append((c, h, w, o, k, s, p, ho, wo, c * k * k))
        c, h, w = o, ho, wo
    return rows


def flat_of(case):
    r = layer_shapes(case)[-1]
    return r[3] * r[7] * r[8]


def last_height(case):
    return layer_shapes(case)[-1][7]


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
Params = namedtuple("Params", "conv_w conv_b head_w head_b")   # float32 CPU tensors; conv_w / conv_b are tuples, one per layer


def reference(case, params, image):
    """float64: (out [n, latent], [the image, every activation])."""
    x = image.double().reshape(-1, *case.image)
    acts = [x]
    for w, b, s, p in zip(params.conv_w, params.conv_b, case.stride, case.padding):
        x = F.elu(F.conv2d(x, w.double(), b.double(), stride=s, padding=p))
        acts.append(x)
    return F.linear(x.flatten(1), params.head_w.double(), params.head_b.double()), acts


def exact_margin(case, params, image):
    """The largest ``|bias| + Σ|w·x|`` over every output element of every layer and the head, and the smallest conv pre-activation."""
    x = image.double().reshape(-1, *case.image)
    worst, low = 0.0, float("inf")
    for w, b, s, p in zip(params.conv_w, params.conv_b, case.stride, case.padding):
        worst = max(worst, float(F.conv2d(x.abs(), w.double().abs(), b.double().abs(), stride=s, padding=p).max()))
        pre = F.conv2d(x, w.double(), b.double(), stride=s, padding=p)
        low = min(low, float(pre.min()))
        x = F.elu(pre)
    worst = max(worst, float(F.linear(x.flatten(1).abs(), params.head_w.double().abs(), params.head_b.double().abs()).max()))
    return worst, low


def columns(segs, mean, std, eps):
    """The 1-D prefix of the row: float32, the kernel's staging arithmetic."""
    x = torch.cat(list(segs), dim=1)
    return x if mean is None else (x - mean) / (std + eps)


def _ternary(shape, density, g):
    u = torch.rand(shape, generator=g)
    return (u < density / 2).float() - ((u >= density / 2) & (u < density)).float()


@functools.lru_cache(maxsize=None)
def exact_data(case, n=NMAX, seed=0):
    """(params, image [n, C·H·W] float32, out float64, acts): the module docstring's signed-exact data and its reference, once per case."""
    g = torch.Generator().manual_seed(seed + 1000 * (sum(map(ord, case.id)) % 997))
    c, h, w = case.image
    image = torch.randint(0, case.vmax + 1, (n, c * h * w), generator=g).float()
    x = image.double().reshape(n, c, h, w)
    ws, bs = [], []
    for (cin, _h, _w, o, k, s, p, _ho, _wo, _K) in layer_shapes(case):
        wt = _ternary((o, cin, k, k), case.density, g)
        b = (wt == -1).flatten(1).sum(1).double() * float(x.max())
        x = F.elu(F.conv2d(x, wt.double(), b, stride=s, padding=p))
        ws.append(wt), bs.append(b.float())
    hw = _ternary((case.latent, flat_of(case)), case.density, g)
    hb = torch.randint(-3, 4, (case.latent,), generator=g).float()
    params = Params(tuple(ws), tuple(bs), hw, hb)
    out, acts = reference(case, params, image)
    return params, image, out, acts


@functools.lru_cache(maxsize=None)
def elu_data(case, n=9, seed=0):
    """One conv layer, everything signed: weights and image in {-2 … 2}, bias in {-3 … 3} — integer pre-activations, about half of them
    negative.  (params without a head, image, the float64 pre-activation [n, flat], a permutation of range(flat))."""
    assert len(case.channels) == 1
    g = torch.Generator().manual_seed(seed + 77)
    c, h, w = case.image
    cin, _h, _w, o, k, s, p, _ho, _wo, _K = layer_shapes(case)[0]
    image = torch.randint(-2, 3, (n, c * h * w), generator=g).float()
    wt = torch.randint(-2, 3, (o, cin, k, k), generator=g).float()
    b = torch.randint(-3, 4, (o,), generator=g).float()
    pre = F.conv2d(image.double().reshape(n, c, h, w), wt.double(), b.double(), stride=s, padding=p).flatten(1)
    return wt, b, image, pre, torch.randperm(flat_of(case), generator=g)


def selector(case, wt, b, perm, start):
    """The head that picks flat indices perm[start : start + L], L = min(flat, 512) (the tail wraps round): (case', params, indices)."""
    flat = flat_of(case)
    L = min(flat, nat.GF_CONV_MAX_LATENT)
    idx = perm[(torch.arange(L) + start) % flat]
    hw = torch.zeros(L, flat)
    hw[torch.arange(L), idx] = 1.0
    return case._replace(latent=L), Params((wt,), (b,), hw, torch.zeros(L)), idx


# ---- descriptors -----------------------------------------------------------------------------------------------------------------------
def shape_args(case, n=1, form="tile", band_rows=0, tile_envs=0, widths=(), row_strides=(), image_stride=0):
    """The descriptor's shape fields alone (every pointer NULL): what the plan entries look at."""
    args = nat.GfConvBandedArgs() if form == "banded" else nat.GfConvEncodeArgs()
    a = args.enc if form == "banded" else args
    a.num_envs, a.image_stride = n, image_stride
    a.channels, a.height, a.width = case.image
    a.num_layers, a.latent_dim = len(case.channels), case.latent
    for l, (o, k, s, p) in enumerate(zip(case.channels, case.kernel, case.stride, case.padding)):
        a.layers[l].out_channels, a.layers[l].kernel, a.layers[l].stride, a.layers[l].padding = o, k, s, p
    a.num_inputs = len(widths)
    for i, wd in enumerate(widths):
        a.inputs[i].width = wd
        a.inputs[i].row_stride = row_strides[i] if i < len(row_strides) else 0
    if form == "banded":
        args.band_rows, args.tile_envs = band_rows, tile_envs
    return args


def _plan_fn(form):
    lib = C.CDLL(nat.lib_path())
    f = lib.gf_conv_banded_plan if form == "banded" else lib.gf_conv_plan
    f.restype = C.c_int
    return f


def plan_status(args):
    """The plan entry's status code for a descriptor (host-only)."""
    banded = isinstance(args, nat.GfConvBandedArgs)
    out = [C.c_int(0) for _ in range(5 if banded else 3)]
    return _plan_fn("banded" if banded else "tile")(C.byref(args), *(C.byref(x) for x in out))


def tile_plan(case):
    """(T, lds_bytes, flat) of gf_conv_plan."""
    plan = nat.conv_plan(shape_args(case))
    assert plan is not None, case.id
    return plan


def banded_plan(case, band_rows=0, tile_envs=0):
    """(T, R, bands, lds_bytes, flat) of gf_conv_banded_plan, or None where it refuses."""
    return nat.conv_banded_plan(shape_args(case, form="banded", band_rows=band_rows, tile_envs=tile_envs))


def forced_tile(case, band_rows, want):
    """The largest tile_envs <= want that the banded plan accepts with this band."""
    for t in range(want, 0, -1):
        if banded_plan(case, band_rows, t) is not None:
            return t
    raise AssertionError(f"{case.id}: no tile fits a band of {band_rows} rows")


def band_settings(case):
    """band_rows in {1, 2, h - 1, h} where those differ, ascending."""
    h = last_height(case)
    return sorted({1, min(2, h), max(h - 1, 1), h})


def _input(data, dev, off, rows=None, width=None, stride=None):
    """An input on a guarded buffer whose surroundings (and row gaps) read as 3.4e38."""
    data = data.float()
    if rows is None:
        g = guarded.Guarded(data.numel(), torch.float32, dev, off=off)
        g.raw.fill_(INPUT_GUARD)
        g.t.copy_(data.reshape(-1))
        return g
    numel = (rows - 1) * stride + width if rows else 0
    g = guarded.Guarded(numel, torch.float32, dev, off=off)
    g.raw.fill_(INPUT_GUARD)
    if rows:
        torch.as_strided(g.t, (rows, width), (stride, 1)).copy_(data.reshape(rows, width))
    return g


class Launch:
    """A case on guarded buffers and its descriptor.  ``offs`` maps a buffer's name — image, w0 … w2, b0 … b2, head_w, head_b, seg0 …,
    mean, std, out, feat — to its element offset (0 … 3); ``segs`` is a list of ([n, width] float32, row_stride or 0); ``norm`` is
    (mean, std, eps) over the segments' columns.  ``poison=False`` leaves `out` / `feat` as the sentinel, for ``untouched``."""

    def __init__(self, case, params, image, dev, form="tile", band_rows=0, tile_envs=0, offs=None, image_stride=0, segs=(), norm=None, poison=True):
        offs = dict(offs or {})
        off = lambda name: offs.pop(name, 0)
        self.case, self.form, self.dev, self.n = case, form, dev, int(image.shape[0])
        n, S, flat = self.n, image.shape[1], flat_of(case)
        self.w1 = sum(s[0].shape[1] for s in segs)
        self.args = shape_args(case, n, form, band_rows, tile_envs, [s[0].shape[1] for s in segs], [s[1] for s in segs], image_stride)
        a = self.enc = self.args.enc if form == "banded" else self.args
        b = self.bufs = {}
        b["image"] = _input(image, dev, off("image"), n, S, image_stride or S)
        a.image = b["image"].ptr
        for l, (w, bias) in enumerate(zip(params.conv_w, params.conv_b)):
            b[f"w{l}"], b[f"b{l}"] = _input(w, dev, off(f"w{l}")), _input(bias, dev, off(f"b{l}"))
            a.layers[l].weight, a.layers[l].bias = b[f"w{l}"].ptr, b[f"b{l}"].ptr
        b["head_w"], b["head_b"] = _input(params.head_w, dev, off("head_w")), _input(params.head_b, dev, off("head_b"))
        a.head_weight, a.head_bias = b["head_w"].ptr, b["head_b"].ptr
        for i, (data, rs) in enumerate(segs):
            b[f"seg{i}"] = _input(data, dev, off(f"seg{i}"), n, data.shape[1], rs or data.shape[1])
            a.inputs[i].rows = b[f"seg{i}"].ptr
        if norm is not None:
            b["mean"], b["std"] = _input(norm[0], dev, off("mean")), _input(norm[1], dev, off("std"))
            a.in_mean, a.in_std, a.in_eps = b["mean"].ptr, b["std"].ptr, norm[2]
        self.out = guarded.Guarded(n * (self.w1 + case.latent), torch.float32, dev, off=off("out"))
        self.feat = guarded.Guarded(n * flat, torch.float32, dev, off=off("feat"))   # (the tile form never sees it)
        if poison:
            self.out.t.fill_(float("nan")), self.feat.t.fill_(float("nan"))
        a.out = self.out.ptr
        if form == "banded":
            self.args.feat = self.feat.ptr
        assert not offs, f"unknown buffers {sorted(offs)}"

    def run(self, backend) -> int:
        rc = guarded.raw_call(backend, "conv_encode_banded" if self.form == "banded" else "conv_encode", self.args)
        guarded.sync(self.dev)
        return rc

    def result(self):
        return self.out.cpu().reshape(self.n, self.w1 + self.case.latent)

    def features(self):
        return self.feat.cpu().reshape(self.n, flat_of(self.case))


def conv_args(case, params, image, dev, **kwargs):
    """The descriptor (GfConvEncodeArgs, or GfConvBandedArgs with form="banded") of a case on guarded buffers: ``Launch``'s, with the
    Launch that keeps the buffers alive."""
    l = Launch(case, params, image, dev, **kwargs)
    return l.args, l


# ---- the refusals: (id, forms, base shape keywords, what to break) ----------------------------------------------------------------------
BASE = _case("base", (2, 6, 5), (3, 4), (3, 2), (2, 1), (1, 0), 6)   # valid in both forms; two layers, two segments (3 and 2 wide)
BASE_WIDTHS = (3, 2)
BIG = 1 << 20


def _enc(args):
    return args.enc if isinstance(args, nat.GfConvBandedArgs) else args


def _set(path, value):
    def apply(args):
        a, names = _enc(args), path.split(".")
        for name in names[:-1]:
            a = getattr(a, name[:-3])[int(name[-2])] if name.endswith("]") else getattr(a, name)
        setattr(a, names[-1], value)
    return apply


def _top(field, value):
    return lambda args: setattr(args, field, value)


def _too_big(args):   # one env's activations: 64 x 128 x 128 floats
    a = _enc(args)
    a.channels, a.height, a.width, a.num_layers = 1, 128, 128, 1
    a.layers[0].out_channels, a.layers[0].kernel, a.layers[0].stride, a.layers[0].padding = 64, 3, 1, 1


def _one_row_band(args):   # a one-row band of one env: 3 x 4 096 image floats and 64 x 4 096 outputs
    _too_big(args)
    _enc(args).height, _enc(args).width = 8, 4096


def _depth(band_rows=0, tile_envs=0):
    def apply(args):   # the depth camera: 7 rows is the tallest band that fits one env, 13 the last layer's height
        a = _enc(args)
        a.channels, a.height, a.width, a.num_layers, a.latent_dim = 1, 58, 87, 2, 64
        for l, (o, k) in enumerate(((16, 5), (32, 3))):
            a.layers[l].out_channels, a.layers[l].kernel, a.layers[l].stride, a.layers[l].padding = o, k, 2, 0
        args.band_rows, args.tile_envs = band_rows, tile_envs
    return apply


BOTH, TILE, BANDED = ("tile", "banded"), ("tile",), ("banded",)
RANGE_CLAUSES = [
    ("num_envs<0", BOTH, _set("num_envs", -1)),
    ("layers=0", BOTH, _set("num_layers", 0)),
    ("layers=4", BOTH, _set("num_layers", nat.GF_CONV_MAX_LAYERS + 1)),
    ("channels=0", BOTH, _set("channels", 0)),
    ("channels=65", BOTH, _set("channels", nat.GF_CONV_MAX_CHANNELS + 1)),
    ("out_channels=0", BOTH, _set("layers[1].out_channels", 0)),
    ("out_channels=65", BOTH, _set("layers[0].out_channels", nat.GF_CONV_MAX_CHANNELS + 1)),
    ("height=0", BOTH, _set("height", 0)),
    ("width=4097", BOTH, _set("width", 4097)),
    ("kernel=0", BOTH, _set("layers[0].kernel", 0)),
    ("kernel=8", BOTH, _set("layers[0].kernel", nat.GF_CONV_MAX_KERNEL + 1)),
    ("stride=0", BOTH, _set("layers[1].stride", 0)),
    ("stride=4", BOTH, _set("layers[0].stride", nat.GF_CONV_MAX_STRIDE + 1)),
    ("padding=kernel", BOTH, _set("layers[0].padding", 3)),
    ("padding<0", BOTH, _set("layers[1].padding", -1)),
    ("output<1x1", BOTH, _set("layers[1].kernel", 4)),   # the second layer's input is 3 x 3
    ("latent=0", BOTH, _set("latent_dim", 0)),
    ("latent=513", BOTH, _set("latent_dim", nat.GF_CONV_MAX_LATENT + 1)),
    ("inputs<0", BOTH, _set("num_inputs", -1)),
    ("inputs=5", BOTH, _set("num_inputs", nat.GF_MLP_MAX_INPUTS + 1)),
    ("width<1", BOTH, _set("inputs[1].width", 0)),
    ("row_stride<width", BOTH, _set("inputs[0].row_stride", 2)),
    ("W1>1024", BOTH, _set("inputs[0].width", nat.GF_MLP_MAX_INPUT_WIDTH - 1)),   # 1023 + 2
    ("image_stride<size", BOTH, _set("image_stride", 2 * 6 * 5 - 1)),
    ("one-env-does-not-fit", TILE, _too_big),
    ("band_rows<0", BANDED, _top("band_rows", -1)),
    ("band_rows>height", BANDED, _top("band_rows", 3)),   # the last layer is 2 rows high
    ("tile_envs<0", BANDED, _top("tile_envs", -1)),
    ("tile_envs=33", BANDED, _top("tile_envs", nat.GF_CONV_MAX_TILE_ENVS + 1)),
    ("forced-band-does-not-fit", BANDED, _depth(band_rows=8)),
    ("forced-tile-does-not-fit", BANDED, _depth(tile_envs=32)),
    ("forced-pair-does-not-fit", BANDED, _depth(band_rows=7, tile_envs=2)),
    ("one-row-band-does-not-fit", BANDED, _one_row_band),
]
NULL_CLAUSES = [
    ("image", BOTH, _set("image", None)),
    ("out", BOTH, _set("out", None)),
    ("feat", BANDED, _top("feat", None)),
    ("head_weight", BOTH, _set("head_weight", None)),
    ("head_bias", BOTH, _set("head_bias", None)),
    ("weight0", BOTH, _set("layers[0].weight", None)),
    ("weight1", BOTH, _set("layers[1].weight", None)),
    ("bias0", BOTH, _set("layers[0].bias", None)),
    ("bias1", BOTH, _set("layers[1].bias", None)),
    ("rows0", BOTH, _set("inputs[0].rows", None)),
    ("rows1", BOTH, _set("inputs[1].rows", None)),
    ("mean-without-std", BOTH, _set("in_std", None)),
]


def base_launch(dev, form, n=3):
    """BASE with two segments and a normaliser on untouched (sentinel) outputs."""
    params, image, _out, _acts = exact_data(BASE)
    g = torch.Generator().manual_seed(5)
    segs = [(torch.randn(n, w, generator=g), 0) for w in BASE_WIDTHS]
    norm = (torch.randn(sum(BASE_WIDTHS), generator=g), torch.rand(sum(BASE_WIDTHS), generator=g) + 0.1, 1e-2)
    return Launch(BASE, params, image[:n], dev, form=form, segs=segs, norm=norm, poison=False)


# ---- CPU: the cases themselves ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SHAPES + [DEPTH, BASE], ids=lambda c: c.id)
def test_every_case_meets_the_exactness_condition(case):
    """|bias| + Σ|w·x| < 2^24 at every output element of every layer and the head, pre-activations >= 0, data in the stated sets."""
    params, image, out, acts = exact_data(case, 3 if case is DEPTH else NMAX)
    worst, low = exact_margin(case, params, image)
    print(f"{case.id}: largest |bias| + sum|w.x| = {worst:.0f} = 2^{torch.tensor(max(worst, 1.0)).log2():.1f}, smallest pre-activation {low:.0f}")
    assert worst < LIMIT and low >= 0.0
    assert set(image.unique().tolist()) <= set(range(case.vmax + 1)) and set(params.head_b.unique().tolist()) <= set(range(-3, 4))
    for w in params.conv_w + (params.head_w,):
        assert set(w.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert torch.equal(out.float().double(), out) and bool((out < 0).any()) and bool((out > 0).any())   # integers below 2^24, both signs
    for a in acts[1:]:
        assert float(a.min()) >= 0.0


def test_the_shapes_reach_what_they_are_for():
    """The table's arithmetic, from torch's Conv2d rule and the two plan entries."""
    ls = {c.id: layer_shapes(c) for c in SHAPES}
    assert ls["k7"][0][7:] == (5, 5, 49) and BY_ID["k7"].padding[0] == BY_ID["k7"].kernel[0] - 1 == 6
    assert BY_ID["low"].image[1] < BY_ID["low"].kernel[0] and ls["low"][0][7] == 3
    assert ls["c64"][0][9] == 576 and flat_of(BY_ID["c64"]) == 1024 and tile_plan(BY_ID["c64"])[0] == 7
    assert (BY_ID["c64"].latent + 31) // 32 // 4 == 4   # head_nb
    for name, K in K_OF.items():
        assert ls[name][0][9] == K and tile_plan(BY_ID[name])[0] == 32
    for name, flat, nb in (("flat128", 128, 1), ("flat256", 256, 2), ("flat512", 512, 3)):
        assert flat_of(BY_ID[name]) == flat and flat % SLAB in (0, 128) and ((BY_ID[name].latent + 31) // 32 + 3) // 4 == nb
        assert BY_ID[name].latent % 32 in (1, 5)
    assert [r[3] * r[7] * r[8] for r in ls["three"]] == [3 * 15 * 11, 64 * 7 * 5, 30] and BY_ID["three"].padding[1] == 4
    assert ls["o33"][0][3] == 33 and (BY_ID["o33"].latent + 31) // 32 == 3   # three column blocks: the fourth head wave has none
    for c in SHAPES:
        T, _lds, flat = tile_plan(c)
        assert flat == flat_of(c) and 2 * T + 1 <= NMAX and banded_plan(c)[1] == last_height(c)   # (whole images fit: the plan does not band)
    T, R, bands, lds, flat = banded_plan(DEPTH)
    assert R < last_height(DEPTH) == 13 and bands * R >= 13 and flat == 8320 and nat.conv_plan(shape_args(DEPTH)) is None
