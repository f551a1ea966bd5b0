"""gf_mlp_act through the raw descriptor at its block, chunk and pass boundaries (csrc/gf_mlp.hip).

The kernel picks ``mlp_layer<NB>`` by the output width (``NB = ceil(ceil(out / 32) / 4)``), walks k in chunks of ``mlp_kc(NB)`` =
128 / 64 / 32 columns — each loaded whole (``FULL``) or as a zero-filled tail, 16 bytes at a time (``VEC``: ``K % 4 == 0`` and a
16-byte aligned weight pointer) or by element — alternates two register sets for ``NB <= 2`` (its two ``break``s are taken after an
odd or an even number of chunks), and stages a first layer wider than 512 columns in two passes.  ``_dispatch`` restates those
choices in Python; ``test_grid_reaches_every_dispatch_path`` asserts that the cases below reach every combination of them.

* Integer nets (``_all_cases``): every partial sum is an integer below 2^24, hence an exact float32 in ANY summation order, and every
  hidden pre-activation is >= 0, so ELU is the identity: ``mean`` / ``values`` must be ``torch.equal`` to an int64 reference.  They
  are written between guard floats into sentinel-filled buffers.  The CPU twin of every case asserts the two conditions and that
  torch's float32 forward equals the reference: it guards the inputs, not the kernel.
* The element path forced onto ``K % 4 == 0`` by weights one float off their alignment: the same reference, bit for bit.
* Random nets where ELU is not the identity, under test_mlp_act's ``_bound`` (``e_hip <= 4 e_torch + 1e-7 max|ref|`` against the
  float64 twin), two of them also with both input normalisers.
* The sampling half at ``A`` in {3, 4, 5, 63, 64}: test_mlp_act.test_sampling_half's assertions, guard floats around every row."""
import collections
import copy
import functools
import itertools
import types

import pytest
import torch

from test_mlp_act import _bound, _obs, _one, _policy
from test_policy_act import _assert_fold, _np_normals
from test_policy_act import _raw as _raw_policy_act

SENTINEL = 1234.5   # no integer: never a result of the integer nets
GUARD = 8           # floats in front of and behind every output (32 bytes: the outputs keep their 16-byte alignment)
EXACT = 2 ** 24


# ---- the dispatch of csrc/gf_mlp.hip, restated ------------------------------------------------------------------------------------
def _nb(out):
    """32-column blocks per wave: mlp_act_kernel's ``nb``."""
    return -(-(-(-out // 32)) // 4)


def _kc(nb):
    """mlp_kc: k columns per chunk."""
    return 128 if nb == 1 else 64 if nb == 2 else 32


Path = collections.namedtuple("Path", "nb vec tail passes parity")


def _dispatch(K, out, aligned=True):
    """The path of one layer ``[K -> out]``: NB, the vector or the element loads, whether the last chunk is a tail
    (``k + KC > K``), the passes of 512 columns, and for ``NB <= 2`` the parity of the last pass's chunk count (the pass that may end
    in a tail; a first pass of a two-pass layer is 512 columns: 4 or 8 full chunks)."""
    nb = _nb(out)
    kc = _kc(nb)
    chunks = [-(-min(K - p0, 512) // kc) for p0 in range(0, K, 512)]
    return Path(nb, K % 4 == 0 and aligned, K % kc != 0, len(chunks), chunks[-1] % 2 if nb <= 2 else None)


def test_dispatch_model_on_known_layers():
    assert [_nb(o) for o in (1, 128, 129, 256, 257, 384, 385, 512)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert [_kc(n) for n in (1, 2, 3, 4)] == [128, 64, 32, 32]
    assert _dispatch(48, 512) == Path(4, True, True, 1, None)       # 32 + a tail of 16
    assert _dispatch(512, 256) == Path(2, True, False, 1, 0)        # 8 chunks
    assert _dispatch(310, 300) == Path(3, False, True, 1, None)
    assert _dispatch(1024, 64) == Path(1, True, False, 2, 0)        # 4 + 4 chunks
    assert _dispatch(641, 33) == Path(1, False, True, 2, 0)         # 4 + (1 full, 1 tail)
    assert _dispatch(576, 129) == Path(2, True, False, 2, 1)        # 8 + 1
    assert _dispatch(128, 12, aligned=False) == Path(1, False, False, 1, 1)


# ---- integer nets -------------------------------------------------------------------------------------------------------------------
# in_width -> widths[0] -> … -> widths[-1]: inputs in {0 … x_hi}, hidden weights in {0 … w_hi}, biases in {0 … b_hi}, the last layer's
# weights in {-last_hi … last_hi}
Net = collections.namedtuple("Net", "in_width widths x_hi w_hi b_hi last_hi seed")
# one launch: n rows, the actor's input cut into `segs` (the critic reads one segment), weights moved off their alignment or not
Case = collections.namedtuple("Case", "actor critic n segs misaligned")


def _first_net(k0, o, a=12):
    """First layer under test: |sum| <= 512 (1024 · 2 · 2 + 4) · 4 + 4 < 2^24."""
    return Net(k0, (o, a), 2, 2, 4, 4, 1000 * k0 + o)


def _hidden_net(k, o, a=12):
    """Hidden layer under test: |sum| <= 512 (512 · 9 + 1) · 3 + 1 < 2^24."""
    return Net(8, (k, o, a), 1, 1, 1, 3, 1000 * k + o + 7)


def _segmentations(k0):
    """The ways a first layer's input is handed over: one segment, the three of test_mlp_act._split, four — above 512 columns once with a
    boundary exactly at column 512 and once with a segment across it."""
    out = [(k0,)]
    if k0 >= 3:
        a, b = k0 // 3, k0 // 3 + max(1, k0 // 4)
        out.append((a, b - a, k0 - b))
    if k0 > 512:
        r = k0 - 512
        out.append((200, 312, r // 2, r - r // 2) if r >= 2 else (100, 100, 312, r))
        out.append((100, 400, 12 + r // 2, r - r // 2) if r >= 2 else (100, 300, 100, k0 - 500))
    elif k0 >= 4:
        q = k0 // 4
        out.append((1, q, k0 - 1 - 2 * q, q))
    assert all(sum(s) == k0 and min(s) >= 1 for s in out)
    return out


HIDDEN_K = [1, 3, 4, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 384, 385, 509, 511, 512]
HIDDEN_O = [1, 32, 33, 128, 129, 256, 257, 384, 385, 512]
# (644 and 708 are not asked for by the paths' edges: they are the two-pass vector layers whose second pass ends in a tail after an
# even number of chunks — 644 for NB = 1, 708 for NB = 1 and 2)
FIRST_K0 = [1, 5, 127, 128, 129, 511, 512, 513, 516, 543, 544, 545, 575, 576, 577, 639, 640, 641, 644, 708, 767, 768, 1023, 1024]
FIRST_O = [33, 129, 257, 385, 512]
LAST_K = [37, 128, 300]
LAST_A = [1, 2, 31, 32, 33, 63, 64]
ROWS = [1, 31, 32, 33, 65]
# NB of the layer under test: its (K, O).  (100, 256) is the grid's only one-pass vector layer under NB = 2 that ends in a tail after
# an even number of chunks: no K of HIDDEN_K between two multiples of 64 is a multiple of 4
ROW_NETS = {1: (193, 33), 2: (100, 256), 3: (33, 257), 4: (129, 512)}
# a one-layer net next to a four-layer one in one launch (grid.y = 2), both ways round
DEEP = (33, 129, 65)
BOTH = {
    "actor1-critic4": (Net(45, (12,), 2, 2, 4, 4, 11), Net(8, DEEP + (1,), 1, 1, 1, 3, 12)),
    "actor4-critic1": (Net(8, DEEP + (12,), 1, 1, 1, 3, 13), Net(45, (1,), 2, 2, 4, 4, 14)),
}
# K % 4 == 0 everywhere, the weights one float off their alignment: the element path without a tail — by one pass and by two, after
# an odd and an even number of chunks — which no K % 4 != 0 can reach (a layer without a tail has K % 32 == 0)
MISALIGNED = {
    "nb1-odd": _hidden_net(128, 33), "nb1-even": _hidden_net(256, 32), "nb2-odd": _hidden_net(64, 129), "nb2-even": _hidden_net(128, 256),
    "nb3": _hidden_net(96, 257), "nb4": _hidden_net(160, 512), "nb4-tail": _hidden_net(48, 385),
    "nb1-2pass-odd": _first_net(640, 33), "nb1-2pass-even": _first_net(1024, 128), "nb1-2pass-tail": _first_net(516, 64),
    "nb2-2pass-odd": _first_net(576, 129), "nb2-2pass-even": _first_net(640, 256), "nb3-2pass": _first_net(544, 257),
    "nb4-2pass": _first_net(1024, 512),
}


def _hidden_cases(k):
    return [Case(_hidden_net(k, o), None, 33, (8,), False) for o in HIDDEN_O]


def _first_cases(k0):
    return [Case(_first_net(k0, o), None, 33, s, False) for o in FIRST_O for s in _segmentations(k0)]


def _last_cases(k):
    return [Case(Net(8, (k, a), 1, 1, 1, 3, 100 * k + a), None, 33, (8,), False) for a in LAST_A]


def _row_cases(nb):
    k, o = ROW_NETS[nb]
    critic = _hidden_net(k, o, 1)._replace(seed=nb)
    return [Case(_hidden_net(k, o), critic, n, (8,), False) for n in ROWS]


def _both_cases(key):
    actor, critic = BOTH[key]
    return [Case(actor, critic, 33, s, False) for s in _segmentations(actor.in_width)[:2]]


def _misaligned_cases(key):
    net = MISALIGNED[key]
    return [Case(net, None, 33, (net.in_width,), m) for m in (False, True)]


def _all_cases():
    groups = [(_hidden_cases, HIDDEN_K), (_first_cases, FIRST_K0), (_last_cases, LAST_K), (_row_cases, ROW_NETS), (_both_cases, BOTH),
              (_misaligned_cases, MISALIGNED)]
    return [c for fn, keys in groups for k in keys for c in fn(k)]


@functools.lru_cache(maxsize=16)   # (a net holds up to 4 MB; the cases of one test share theirs)
def _int_net(net):
    """The net's integer data on the CPU (int64): the input for 65 rows and [(W, b)] — computed once, shared, never written.  A
    column of a hidden W that came out all zero gets a one, so that every k of every layer counts in some output."""
    g = torch.Generator().manual_seed(net.seed)
    x = torch.randint(0, net.x_hi + 1, (max(ROWS), net.in_width), generator=g)
    layers, k = [], net.in_width
    for i, o in enumerate(net.widths):
        if i == len(net.widths) - 1:
            w = torch.randint(-net.last_hi, net.last_hi + 1, (o, k), generator=g)
        else:
            w = torch.randint(0, net.w_hi + 1, (o, k), generator=g)
        dead = (w != 0).sum(0) == 0
        w[torch.randint(0, o, (k,), generator=g)[dead], torch.nonzero(dead)[:, 0]] = 1
        layers.append((w, torch.randint(0, net.b_hi + 1, (o,), generator=g)))
        k = o
    return x, tuple(layers)


@functools.lru_cache(maxsize=16)
def _int_reference(net, n):
    """The net's forward on its first ``n`` rows in int64 (ELU taken as the identity), with the two conditions under which a
    float32 evaluation in any order equals it: (output [n, out], max over the layers of max(|a| |W|^T + |b|), min over the hidden
    layers of the pre-activation)."""
    x, layers = _int_net(net)
    h, top, low = x[:n], 0, 0
    for i, (w, b) in enumerate(layers):
        top = max(top, int((h.abs() @ w.abs().T + b.abs()).max()))
        h = h @ w.T + b
        if i < len(layers) - 1:
            low = min(low, int(h.min()))
    return h, top, low


def _module(net, dtype=torch.float32):
    x, layers = _int_net(net)
    mods = []
    for w, b in layers:
        lin = torch.nn.Linear(w.shape[1], w.shape[0], dtype=dtype)
        with torch.no_grad():
            lin.weight.copy_(w)
            lin.bias.copy_(b)
        mods += [lin, torch.nn.ELU()]
    return torch.nn.Sequential(*mods[:-1])


# ---- CPU: the inputs and the coverage, without the kernel ---------------------------------------------------------------------------
def _check_case_on_cpu(case):
    for net in (case.actor, case.critic):
        if net is None:
            continue
        ref, top, low = _int_reference(net, case.n)
        assert top < EXACT, f"{net}: a sum of magnitudes reaches {top} >= 2^24"
        assert low >= 0, f"{net}: a hidden pre-activation is {low}: ELU is not the identity"
        with torch.no_grad():
            f32 = _module(net)(_int_net(net)[0][:case.n].float())
        assert f32.dtype == torch.float32 and torch.equal(f32.double(), ref.double()), f"{net}: torch's float32 forward differs"
        for w, _b in _int_net(net)[1]:
            assert bool(((w != 0).sum(0) > 0).all()), f"{net}: a weight column is all zero"


@pytest.mark.parametrize("k", HIDDEN_K)
def test_hidden_cases_are_exact_in_float32(k):
    for case in _hidden_cases(k):
        _check_case_on_cpu(case)


@pytest.mark.parametrize("k0", FIRST_K0)
def test_first_layer_cases_are_exact_in_float32(k0):
    for case in _first_cases(k0)[::len(_segmentations(k0))]:   # (the segmentations share the net and the rows)
        _check_case_on_cpu(case)


OTHER = ({f"last-{k}": _last_cases(k) for k in LAST_K} | {f"rows-nb{nb}": _row_cases(nb) for nb in ROW_NETS}
         | {k: _both_cases(k) for k in BOTH} | {k: _misaligned_cases(k)[:1] for k in MISALIGNED})


@pytest.mark.parametrize("key", list(OTHER))
def test_other_cases_are_exact_in_float32(key):
    for case in OTHER[key]:
        _check_case_on_cpu(case)


def _paths(cases):
    """{path: a case that takes it} over every layer of every net of ``cases``."""
    seen = {}
    for case in cases:
        for net in filter(None, (case.actor, case.critic)):
            for k, o in zip((net.in_width,) + net.widths, net.widths):
                seen.setdefault(_dispatch(k, o, not case.misaligned), case)
    return seen


def test_grid_reaches_every_dispatch_path():
    """NB x {vector, element} x {tail, none} x {1, 2} passes, and for NB <= 2 x {odd, even} chunk count of the last pass: no
    combination is unreachable — the element path without a tail exists only at a misaligned address (a layer without a tail has
    K % 32 == 0), which is what MISALIGNED's nets are for."""
    want = {Path(nb, vec, tail, passes, parity)
            for nb in (1, 2, 3, 4) for vec in (True, False) for tail in (True, False) for passes in (1, 2)
            for parity in ((0, 1) if nb <= 2 else (None,))}
    assert len(want) == 2 * 16 + 2 * 8
    seen = _paths(_all_cases())
    assert not want - set(seen), f"no case takes {sorted(want - set(seen), key=str)}"
    assert set(seen) == want
    # the aligned grid alone misses exactly the element path without a tail
    aligned = set(_paths(c for c in _all_cases() if not c.misaligned))
    assert want - aligned == {p for p in want if not p.vec and not p.tail}
    # every NB sees an output width on both sides of its block edges, every chunk length a K on both sides of a multiple
    outs = {o for c in _all_cases() for net in (c.actor, c.critic) if net for o in net.widths}
    assert {1, 32, 33, 128, 129, 256, 257, 384, 385, 512} <= outs
    hidden_k = {net.widths[0] for c in _all_cases() for net in (c.actor,) if len(net.widths) == 3}
    for kc, m in ((32, 2), (64, 3), (128, 3)):
        assert {kc - 1, kc, kc + 1, m * kc - 1, m * kc, m * kc + 1} <= hidden_k
    assert max(len(net.widths) for c in _all_cases() for net in (c.actor, c.critic) if net) == 4
    assert {c.n for c in _all_cases()} == set(ROWS)


# ---- GPU: the raw descriptor, outputs between guard floats ---------------------------------------------------------------------------
class _Out:
    """An ``[n, w]`` (w = 0: ``[n]``) output in a sentinel-filled buffer with GUARD floats in front of it and behind it."""

    def __init__(self, n, w, dev):
        self.buf = torch.full((2 * GUARD + n * max(w, 1),), SENTINEL, device=dev)
        self.view = self.buf[GUARD:GUARD + n * max(w, 1)].view((n, w) if w else (n,))
        self.ptr = self.buf.data_ptr() + 4 * GUARD
        assert self.buf.data_ptr() % 16 == 0

    def check(self, what):
        guards = torch.cat([self.buf[:GUARD], self.buf[-GUARD:]])
        assert bool((guards == SENTINEL).all()), f"{what}: a float outside the output was written"
        return self.view


def _off_alignment(net, layers, keep):
    """Point the descriptor's weights at copies one float off 16-byte alignment."""
    for lay, (w, _b) in zip(net.layers, layers):
        buf = torch.full((w.numel() + 4,), SENTINEL, device=w.device)
        buf[1:1 + w.numel()].copy_(w.detach().reshape(-1))
        assert buf.data_ptr() % 16 == 0 and lay.weight == w.data_ptr()
        lay.weight = buf.data_ptr() + 4
        keep.append(buf)


def _launch(backend, fwd, n, obs=None, cobs=None, misaligned=False, std=None, noise=None, seed=1, stream=0, env_offset=0):
    """gf_mlp_act through the binding: {name: guarded output}, checked.  ``std``: the sampling half with all five storage rows."""
    dev = (obs or cobs)[0].device
    a = fwd._fill(n, obs, cobs)
    a.std = a.noise = a.mean = a.values = a.actions = a.actions_out = a.mu_out = a.sigma_out = a.values_out = a.log_prob_out = None
    a.seed, a.stream, a.env_offset, a.std_per_env = seed, stream, env_offset, 0
    keep, o = [], {}
    if misaligned:
        for net, layers, x in ((a.actor, fwd.actor, obs), (a.critic, fwd.critic, cobs)):
            if x is not None:
                _off_alignment(net, layers, keep)
    if obs is not None:
        A = int(fwd.actor[-1][0].shape[0])
        o["mean"] = _Out(n, A, dev)
        a.mean = o["mean"].ptr
        if std is not None:
            for k in ("actions", "actions_out", "mu_out", "sigma_out"):
                o[k] = _Out(n, A, dev)
                setattr(a, k, o[k].ptr)
            o["log_prob_out"] = _Out(n, 0, dev)
            a.log_prob_out, a.std = o["log_prob_out"].ptr, std.data_ptr()
            a.noise = None if noise is None else noise.data_ptr()
    if cobs is not None:
        o["values"] = _Out(n, 0, dev)
        a.values = o["values"].ptr
        if std is not None:
            o["values_out"] = _Out(n, 0, dev)
            a.values_out = o["values_out"].ptr
    backend.mlp_act(a)
    torch.cuda.synchronize()
    return {k: v.check(k) for k, v in o.items()}


@functools.lru_cache(maxsize=8)
def _forward_of(actor, critic):
    from genesis_forge_amd.learner import PolicyForward

    policy = types.SimpleNamespace(actor=None if actor is None else _module(actor).cuda(), critic=None if critic is None else _module(critic).cuda())
    return PolicyForward(policy)


def _cut(x, widths):
    at = list(itertools.accumulate((0,) + tuple(widths)))
    return tuple(x[:, i:j].contiguous() for i, j in zip(at, at[1:]))


def _run_case(backend, case):
    fwd = _forward_of(case.actor, case.critic)
    obs = _cut(_int_net(case.actor)[0][:case.n].float().cuda(), case.segs)
    cobs = None if case.critic is None else (_int_net(case.critic)[0][:case.n].float().cuda(),)
    got = _launch(backend, fwd, case.n, obs, cobs, case.misaligned)
    what = f"{case.actor}, {case.n} rows, segments {case.segs}" + (", weights off their alignment" if case.misaligned else "")
    mean = got["mean"].cpu()
    ref = _int_reference(case.actor, case.n)[0]
    assert mean.shape == ref.shape and torch.equal(mean.double(), ref.double()), f"mean: {what}: {int((mean.double() != ref.double()).sum())} of {ref.numel()} differ"
    if case.critic is not None:
        values = got["values"].cpu()
        ref = _int_reference(case.critic, case.n)[0][:, 0]
        assert values.shape == ref.shape and torch.equal(values.double(), ref.double()), f"values: {case.critic} next to {what}"
    return mean


@pytest.mark.gpu
@pytest.mark.parametrize("k", HIDDEN_K)
def test_hidden_layer_is_exact_on_integer_nets(hip_backend, k):
    """[8 -> k -> O -> 12] for every O: the layer [k -> O] under NB(O), and with it [8 -> k] under NB(k) and [O -> 12] under NB = 1."""
    for case in _hidden_cases(k):
        _run_case(hip_backend, case)


@pytest.mark.gpu
@pytest.mark.parametrize("k0", FIRST_K0)
def test_first_layer_is_exact_on_integer_nets(hip_backend, k0):
    """[k0 -> O -> 12] for every O, the input as one, three and four segments: one pass or two, the second one of 1 … 512 columns."""
    for case in _first_cases(k0):
        _run_case(hip_backend, case)


@pytest.mark.gpu
@pytest.mark.parametrize("k", LAST_K)
def test_last_layer_is_exact_on_integer_nets(hip_backend, k):
    for case in _last_cases(k):
        _run_case(hip_backend, case)


@pytest.mark.gpu
@pytest.mark.parametrize("nb", list(ROW_NETS))
def test_rows_of_a_partial_tile_are_exact(hip_backend, nb):
    """1, 31, 32, 33 and 65 rows (a tile of one row, a full one, a full one and a row) with both nets in the launch."""
    for case in _row_cases(nb):
        _run_case(hip_backend, case)


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(BOTH))
def test_nets_of_different_depth_in_one_launch(hip_backend, key):
    for case in _both_cases(key):
        _run_case(hip_backend, case)


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(MISALIGNED))
def test_element_path_forced_by_address(hip_backend, key):
    aligned, moved = (_run_case(hip_backend, case) for case in _misaligned_cases(key))
    assert torch.equal(aligned, moved)


# ---- GPU: accuracy where ELU is not the identity ------------------------------------------------------------------------------------
ACCURACY = [   # (input segments, hidden widths, A)
    ((48,), (129, 257, 385), 12),
    ((45,), (33, 511), 12),
    ((516,), (193,), 12),
    ((512, 1, 511), (257, 129), 12),
    ((48,), (64, 129, 33, 385, 64), 12),   # six Linear
]
NORMALIZED = [(1024,), (512, 1, 511)]
_ids = lambda s: "-".join(map(str, s[0] + s[1] + (s[2],)))


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("shape", ACCURACY, ids=_ids)
def test_accuracy_against_float64_at_the_edges(hip_backend, shape, scale):
    from genesis_forge_amd.learner import PolicyForward

    segs, hidden, A = shape
    n = 1000
    policy = _policy(segs, hidden, A, "cuda", seed=2, scale=scale)
    ref64 = copy.deepcopy(policy).double()
    fwd = PolicyForward(policy)
    obs = _obs(segs, n, "cuda", scale=scale)
    x = _one(obs)
    print(f"  segments {segs} hidden {hidden} A {A} rows {n} scale x{scale}")
    got = _launch(hip_backend, fwd, n, obs, obs)
    with torch.no_grad():
        _bound("mean ", got["mean"], policy.act_mean(x), ref64.act_mean(x.double()))
        _bound("value", got["values"], policy.evaluate(x)[:, 0], ref64.evaluate(x.double())[:, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("widths", NORMALIZED, ids=lambda s: "+".join(map(str, s)))
def test_two_pass_nets_normalize_as_they_stage(hip_backend, widths):
    """test_obs_norm.test_mlp_act_normalizes_as_it_stages' rule on a two-pass first layer under NB = 3 (then NB = 2): the launch that
    normalises equals, bit for bit, the launch on the input the CPU normalised in float32; and both keep ``_bound``."""
    from genesis_forge_amd.learner import ActorCriticMLP, PolicyForward
    from test_obs_norm import _data, _normalized_on_cpu, _warm
    from test_obs_norm import _split as _split_widths

    n, w, A = 1000, sum(widths), 12
    torch.manual_seed(w)
    policy = ActorCriticMLP(w, A, (257, 129), (257, 129), init_noise_std=0.7, actor_obs_normalization=True, critic_obs_normalization=True).to("cuda")
    _warm(policy.actor_obs_normalizer, 3), _warm(policy.critic_obs_normalizer, 4)
    plain = types.SimpleNamespace(actor=policy.actor, critic=policy.critic, std=policy.std)
    fwd, fwd_plain = PolicyForward(policy), PolicyForward(plain)
    x = _data(n, w, seed=2)
    raw = tuple(p.cuda() for p in _split_widths(x, widths))
    xa = tuple(p.cuda() for p in _split_widths(_normalized_on_cpu(policy.actor_obs_normalizer, x), widths))
    xc = tuple(p.cuda() for p in _split_widths(_normalized_on_cpu(policy.critic_obs_normalizer, x), widths))
    assert not torch.equal(xa[0], xc[0])
    noise = torch.randn(n, A, generator=torch.Generator().manual_seed(n)).cuda()
    std = policy.std.detach()
    got = _launch(hip_backend, fwd, n, raw, raw, std=std, noise=noise)
    want = _launch(hip_backend, fwd_plain, n, xa, xc, std=std, noise=noise)
    assert set(got) == set(want) and "log_prob_out" in got and "values_out" in got
    for k in got:
        assert torch.equal(got[k], want[k]), f"{k}: the fused normalisation differs from the launch on the normalised input"
    assert torch.equal(fwd.mean(raw), got["mean"]) and torch.equal(fwd.value(raw)[:, 0], got["values"])
    ref64 = copy.deepcopy(policy).double()
    xd = x.cuda()
    with torch.no_grad():
        _bound("mean ", got["mean"], policy.act_mean(xd), ref64.act_mean(xd.double()))
        _bound("value", got["values"], policy.evaluate(xd)[:, 0], ref64.evaluate(xd.double())[:, 0])


# ---- GPU: the sampling half at the action-width edges ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("A", [3, 4, 5, 63, 64])
def test_sampling_half_at_the_action_width_edges(hip_backend, A):
    """test_mlp_act.test_sampling_half's assertions where the last quad of a row ends at, before or past A (A % 4 == 0: the vector
    policy_act_row), every output between guard floats."""
    from genesis_forge_amd.learner import PolicyForward

    segs, hidden, n = (48,), (64,), 257
    policy = _policy(segs, hidden, A, "cuda", seed=4)
    fwd = PolicyForward(policy)
    obs = _obs(segs, n, "cuda", seed=5)
    std = (torch.rand(A, generator=torch.Generator().manual_seed(6)) * 1.5 + 0.05).cuda()
    noise = torch.randn(n, A, generator=torch.Generator().manual_seed(7)).cuda()
    assert std.data_ptr() % 16 == 0 and noise.data_ptr() % 16 == 0
    o = _launch(hip_backend, fwd, n, obs, obs, std=std, noise=noise)
    assert torch.equal(o["mu_out"], o["mean"]) and torch.equal(o["values_out"], o["values"])
    assert torch.equal(o["mean"], fwd.mean(obs)) and torch.equal(o["values"], fwd.value(obs)[:, 0]), "each net alone gives the same bits"
    assert torch.equal(o["sigma_out"], std.expand(n, A))
    assert torch.equal(o["actions"], o["mu_out"] + std * noise) and torch.equal(o["actions_out"], o["actions"])
    _assert_fold(o["log_prob_out"], o["actions"], o["mu_out"], std)
    # Philox mode
    seed, stream, off = 1234, 5, 17
    p = _launch(hip_backend, fwd, n, obs, obs, std=std, seed=seed, stream=stream, env_offset=off)
    assert torch.equal(p["mean"], o["mean"])
    eps = torch.from_numpy(_np_normals(seed, stream, off, n, A)).cuda()
    assert float((p["actions"] - p["mu_out"] - std * eps).abs().max()) <= 1e-6
    q = _raw_policy_act(hip_backend, p["mean"].contiguous(), std, p["values"].contiguous(), seed=seed, stream=stream, env_offset=off)
    for mine, theirs in zip((p["actions"], p["actions_out"], p["mu_out"], p["sigma_out"], p["values_out"], p["log_prob_out"]), q):
        assert torch.equal(mine, theirs), "gf_policy_act draws the same from the same mean"
    _assert_fold(p["log_prob_out"], p["actions"], p["mu_out"], std)
    # mean only: nothing is drawn, nothing else is written
    m = _launch(hip_backend, fwd, n, obs, None)
    assert torch.equal(m["mean"], o["mean"])
