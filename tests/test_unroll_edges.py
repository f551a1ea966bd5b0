"""gf_history_unroll at the edges of its index arithmetic (cases and reference: tests/unroll_cases.py).

Every case runs on the GPU (``gf_history_unroll`` / ``gf_run_ops``) and, unmarked, on the CPU oracle (``gfo_history_unroll`` /
``gfo_run_ops``), both against the numpy restatement, bit for bit on int32 views.  Ring, ``out`` and ``out2`` are slices of guarded
buffers (tests/guarded.py): nothing outside an exactly sized destination may change, and a NULL ``out2`` leaves its buffer alone."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import unroll_cases as uc
from genesis_forge_amd import _native as nat
from guarded import Guarded, raw_call, sync


@functools.lru_cache(maxsize=3)
def _ring(n, O, H):
    return uc.make_ring(n, O, H)


@functools.lru_cache(maxsize=3)
def _want(n, O, H, k):
    return torch.from_numpy(np.ascontiguousarray(uc.want(_ring(n, O, H), k))).reshape(-1)


class Gather:
    """One gather's descriptor with its guarded buffers."""

    def __init__(self, dev, n, O, H, slot, two, ring_off=0, out_off=0, out2_off=0):
        self.dev, self.shape, self.slot, self.two = dev, (n, O, H), slot, two
        total = n * O * H
        self.ring = Guarded(total, torch.int32, dev, off=ring_off, init=torch.from_numpy(_ring(n, O, H)))
        self.out = Guarded(total, torch.int32, dev, off=out_off)
        self.out2 = Guarded(total, torch.int32, dev, off=out2_off)
        a = self.args = nat.GfHistoryUnrollArgs()
        a.ring, a.out, a.out2 = self.ring.ptr, self.out.ptr, (self.out2.ptr if two else None)
        a.num_envs, a.frame_width, a.history_len, a.ring_slot = n, O, H, slot

    def check(self, what=""):
        n, O, H = self.shape
        w = _want(n, O, H, self.slot - 1).to(self.dev)
        tag = (what, self.shape, self.slot, self.two)
        assert torch.equal(self.out.t, w), ("out differs", tag)
        assert self.out.guards_ok() and self.ring.guards_ok(), ("wrote outside out", tag)
        assert torch.equal(self.ring.t.cpu().reshape(n, H, O), torch.from_numpy(_ring(n, O, H))), ("the ring changed", tag)
        if self.two:
            assert torch.equal(self.out2.t, w), ("out2 differs", tag)
            assert self.out2.guards_ok(), ("wrote outside out2", tag)
        else:
            assert self.out2.untouched(), ("out2 is NULL, its buffer changed", tag)

    def check_untouched(self, what=""):
        assert self.out.untouched() and self.out2.untouched(), (what, self.shape)


def _single(backend, dev, n, O, H, slots, two=None, ring_off=0):
    """One call per slot; ``two`` None alternates the second destination with the slot."""
    for slot in slots:
        g = Gather(dev, n, O, H, slot, (slot % 2 == 1) if two is None else two, ring_off=ring_off)
        assert raw_call(backend, "history_unroll", g.args) == 0
        sync(dev)
        g.check()


def _run_ops(backend, gathers):
    ops = (nat.GfOp * len(gathers))()
    for i, g in enumerate(gathers):
        ops[i].phase, ops[i].args = nat.GF_PHASE_UNROLL, C.addressof(g.args)
    failed = C.c_int(-1)
    if backend.name == "hip":
        rc = backend.lib.gf_run_ops(ops, len(gathers), backend._stream(), C.byref(failed))
    else:
        rc = backend.lib.gfo_run_ops(ops, len(gathers), C.byref(failed))
    sync(gathers[0].dev)
    return rc, failed.value


# ---- the groups, once per backend ---------------------------------------------------------------------------------------------------
def _all_slots(backend, dev, n, O, H):
    _single(backend, dev, n, O, H, uc.slots_all(H))


def _long_rows(backend, dev, n, O, H):
    _single(backend, dev, n, O, H, uc.slots_all(H) if H <= 7 else uc.slots_few(H) + [H - 1])


def _range_edge(backend, dev, n, O, H):
    _single(backend, dev, n, O, H, uc.slots_few(H))


def _ring_offset(backend, dev, shape, off):
    _single(backend, dev, *shape, uc.slots_all(shape[2]), ring_off=off)


def _streaming(backend, dev, n, O, H, two):
    _single(backend, dev, n, O, H, [1, H], two=two)


def _pair(backend, dev, sa, sb, two_a=False, two_b=False):
    """a and b through gf_run_ops == two single calls == the restatement."""
    for slot_a, slot_b in ((1, sb[2]), (sa[2], 1)):
        pair = [Gather(dev, *sa, slot_a, two_a), Gather(dev, *sb, slot_b, two_b)]
        assert _run_ops(backend, pair) == (0, -1)
        alone = [Gather(dev, *sa, slot_a, two_a), Gather(dev, *sb, slot_b, two_b)]
        for g in alone:
            assert raw_call(backend, "history_unroll", g.args) == 0
        sync(dev)
        for p, s in zip(pair, alone):
            p.check("pair")
            s.check("alone")
            assert torch.equal(p.out.raw, s.out.raw) and torch.equal(p.out2.raw, s.out2.raw)


def _pair_cases(backend, dev):
    _pair(backend, dev, (70, 62, 5), (70, 3, 2))
    _pair(backend, dev, (70, 3, 2), (70, 62, 5))
    _pair(backend, dev, (257, 7, 6), (1, 1, 1), two_a=True)
    # three adjacent ops: the first two share a launch, the third runs alone
    three = [Gather(dev, 70, 62, 5, 2, False), Gather(dev, 70, 3, 2, 2, True), Gather(dev, 33, 7, 6, 4, True)]
    assert _run_ops(backend, three) == (0, -1)
    for g in three:
        g.check("three ops")
    # b refused (misaligned out): a is written, the failure is b's
    a, b = Gather(dev, 70, 62, 5, 3, True), Gather(dev, 70, 3, 2, 1, False, out_off=1)
    assert _run_ops(backend, [a, b]) == (uc.GF_E_UNSUPPORTED, 1)
    a.check("in front of a refused op")
    b.check_untouched("refused")
    # a has no envs: nothing of it is launched, b is
    a, b = Gather(dev, 5, 3, 4, 1, True), Gather(dev, 130, 16, 5, 5, True)
    a.args.num_envs = 0
    assert _run_ops(backend, [a, b]) == (0, -1)
    a.check_untouched("num_envs = 0")
    b.check("behind an empty op")


def _pair_streaming(backend, dev, n):
    pair = [Gather(dev, n, 62, 5, 2, True), Gather(dev, n, 62, 5, 5, True)]
    assert _run_ops(backend, pair) == (0, -1)
    for g in pair:
        g.check("pair at the streaming rule")


GROUPS = {
    "narrow": (_all_slots, uc.NARROW + uc.NARROW_CHUNK),
    "wide_small": (_all_slots, uc.WIDE_SMALL),
    "long_rows": (_long_rows, uc.LONG_ROWS),
    "range_edge": (_range_edge, uc.RANGE_EDGE),
    "ring_offset": (_ring_offset, uc.RING_OFFSETS),
    "streaming": (_streaming, [c[:4] for c in uc.STREAMING]),
    "pair_streaming": (_pair_streaming, [(n,) for n, _s in uc.PAIR_STREAMING]),
}
ALL = [pytest.param(name, case, id=f"{name}-{'x'.join(str(x) for x in case)}".replace(" ", "")) for name, (_f, cases) in GROUPS.items() for case in cases]


@pytest.mark.parametrize("group,case", ALL)
def test_unroll_edges_oracle(oracle_backend, group, case):
    GROUPS[group][0](oracle_backend, "cpu", *case)


@pytest.mark.gpu
@pytest.mark.parametrize("group,case", ALL)
def test_unroll_edges_hip(hip_backend, group, case):
    GROUPS[group][0](hip_backend, "cuda", *case)


def test_unroll_pairs_oracle(oracle_backend):
    _pair_cases(oracle_backend, "cpu")


@pytest.mark.gpu
def test_unroll_pairs_hip(hip_backend):
    _pair_cases(hip_backend, "cuda")


# ---- refusals: no launch, so both libraries answer without a GPU --------------------------------------------------------------------
def test_unroll_edge_refusals(oracle_lib_path):
    hip, orc = C.CDLL(nat.lib_path()), C.CDLL(oracle_lib_path)
    calls = (lambda a: hip.gf_history_unroll(C.byref(a), None), lambda a: orc.gfo_history_unroll(C.byref(a)))
    for call in calls:
        for O, H in uc.RANGE_REFUSED:   # O*H = 2^17: the first product outside the divisions' exact range
            g = Gather("cpu", 1, 1, 1, 1, True)
            g.args.frame_width, g.args.history_len = O, H
            assert call(g.args) == uc.GF_E_RANGE
            g.args.num_envs = 0
            assert call(g.args) == uc.GF_E_RANGE, "the range is checked before the empty launch returns"
            g.check_untouched()
        g = Gather("cpu", 70, 62, 5, 1, True, out2_off=1)   # out2 4 bytes off
        assert call(g.args) == uc.GF_E_UNSUPPORTED
        g.check_untouched()
        g = Gather("cpu", 70, 62, 5, 1, False, out_off=2)
        assert call(g.args) == uc.GF_E_UNSUPPORTED
        g.check_untouched()


# ---- the divisions' model -----------------------------------------------------------------------------------------------------------
def test_mulshift_divisions_are_exact_for_every_legal_divisor():
    """UnrollMap.src divides by O*H (ec < O*H + 2 056) and by O (c < O*H < 2^17) with ceil(2^40 / d): floor division is a step
    function, so exactness at k*d - 1 and k*d for every multiple in range is exactness everywhere in range."""
    for limit in (lambda d: d + uc.EC_SPAN, lambda d: np.full_like(d, uc.RANGE_LIMIT)):
        d, m = uc.multiples_up_to(limit)
        assert d.min() == 1 and d.max() == uc.RANGE_LIMIT - 1 and np.unique(d).size == uc.RANGE_LIMIT - 1
        assert np.array_equal(uc.mulshift_div(m, d), (m // d).astype(np.uint64))
        assert np.array_equal(uc.mulshift_div(m - 1, d), ((m - 1) // d).astype(np.uint64))
    for oh in (131071, 130048, 131070):   # the range-limit cases, every i the kernel can form
        i = np.arange(oh + uc.EC_SPAN + 1, dtype=np.int64)
        assert np.array_equal(uc.mulshift_div(i, np.full_like(i, oh)), (i // oh).astype(np.uint64))
