"""gf_observe through its raw descriptor, at its plan, gather, write-out and history edges (cases, numpy restatement and dispatch
model: tests/observe_cases.py).

Every case of the table runs twice against the restatement: on the CPU oracle (``gfo_observe``, unmarked — this is what holds the
restatement and the oracle to each other before a GPU is touched) and on the GPU (``gf_observe``).  Per call:

* columns of copied and scale-only items equal the float32 restatement bit for bit (integer views; a single multiply cannot be
  contracted), history slots equal the previous call's output bit for bit, and the whole output equals the restatement fed the
  previous call's restated output in those columns;
* noise, body-frame and norm columns: the launch's maximum error against the float64 restatement is at most 4 x the numpy float32
  restatement's own (``observe_cases.within``; both are printed, the measured ratios are in profiles/observe_edges.md) — and the
  float32 restatement's error is not zero, so the bound says something;
* every sentinel survives — the 64 rows behind ``num_envs``, the guards, every ring slot that is not written —, every source
  buffer is unchanged byte for byte, and no output float is left at its sentinel.

The chain: the ops [masked reset, observe] and [masked reset, command(masked), observe, observe] through ``gf_run_ops`` with
GF_OPT_CHAIN on fold into ``chain_b_kernel`` — its observe phase builds the tables in LDS always, takes the write-out width at run
time, reads each manager's items at its own offset of the argument segment and reuses one LDS tile for both managers — and with
the option off run launch by launch; both must equal the restatement.  The first observation manager of the four-op runs reads the
command rows the masked command op of the same run writes.

No case is skipped or filtered: the table is fixed."""
import os

import numpy as np
import pytest

import observe_cases as oc
import reset_cases as rc
from genesis_forge_amd import _native as nat
from observe_cases import Case, it

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "genesis-forge_amd", "csrc")
CHAIN_SIZES = (65, 130)
CHAIN_RUNS = {   # name -> (a masked command op between the reset and the observations, the frames of observe_cases.CHAIN_FRAMES)
    "reset-units49": (False, ("units49",)),
    "reset-nounits": (False, ("nounits",)),
    "reset-oddhist": (False, ("oddhist",)),
    "reset-command-narrow-wide": (True, ("narrow", "wide")),
    "reset-command-wide-narrow": (True, ("wide", "narrow")),
    "reset-command-elemhist-units49": (True, ("elemhist", "units49")),
    "reset-command-nounits-oddhist": (True, ("nounits", "oddhist")),
}


# ---- CPU: the model's constants, the restatement's pins, the coverage of the table -----------------------------------------------------
def test_model_constants_are_the_kernels():
    for key, name in oc.K_NATIVE.items():
        assert oc.K[key] == getattr(nat, name), key
    for key, value in oc.constants_in_sources(CSRC).items():
        assert value == oc.K[key], f"{key}: the model says {oc.K[key]}, the sources {value}"
    import ctypes
    assert ctypes.sizeof(nat.GfObsItem) == 24 and nat.GfObsItem.scale.offset == 16 and nat.GfObsItem.noise.offset == 20


def _hand(items, data, **kw):
    n = next(iter(data.values())).shape[0]
    return Case("hand", n, items, data={k: np.asarray(v) for k, v in data.items()}, **kw)


def test_restatement_pins():
    F = np.float32
    # scale, then noise: 3 * 0.5 + (2 * 0.75 - 1) * 0.5 = 1.75; u = 0 is the lower end, -noise; a noise-free neighbour stays
    c = _hand([it("ext", 2, scale=0.5, noise=0.5), it("ext", 1)],
              {"ext.0": np.array([[3.0, 3.0]], F), "ext.1": np.array([[7.0]], F), "noise_draws": np.array([[0.75, 0.0, 0.25]], F)}, noise="dense")
    assert oc.restate_frame(c, 0, oc.X32).tolist() == [[1.75, 1.0, 7.0]]
    # the dense draws are indexed [n, frame column], not [n, column of the item]
    c = _hand([it("ext", 1), it("ext", 1, noise=1.0)], {"ext.0": np.array([[5.0], [6.0]], F), "ext.1": np.zeros((2, 1), F),
                                                       "noise_draws": np.array([[0.0, 0.5], [1.0, 0.75]], F)}, noise="dense")
    assert oc.restate_frame(c, 0, oc.X32).tolist() == [[5.0, 0.0], [6.0, 0.5]]
    # torch.norm of (3, 4, 12) and of (0, 0, 0), link by link
    c = _hand([it("norm", 2, scale=0.5)], {"norm.0": np.array([[3.0, 4.0, 12.0, 0.0, 0.0, 0.0]], F)})
    assert oc.restate_frame(c, 0, oc.X32).tolist() == [[6.5, 0.0]]
    # body frame: a quarter turn about x takes the world's -z to the body's -y, a world +y velocity to the body's -z … and the
    # stale quaternion (identity here) is used exactly where either mask byte is set
    h = np.sqrt(0.5)
    data = {"quat": np.array([[h, h, 0, 0]] * 4, F), "stale_quat": np.array([[1, 0, 0, 0]] * 4, F), "lin": np.array([[0, 1, 0]] * 4, F),
            "ang": np.array([[2, 0, 0]] * 4, F), "stale_mask": np.array([0, 1, 0, 0x80], np.uint8), "stale_mask2": np.array([0, 0, 0xFF, 1], np.uint8)}
    c = _hand([it("grav"), it("lin"), it("ang")], data, stale=("mixed", "mixed"))
    got = oc.restate_frame(c, 0, oc.X64)
    np.testing.assert_allclose(got[0], [0, -1, 0, 0, 0, -1, 2, 0, 0], atol=2e-7)
    for row in (1, 2, 3):
        assert got[row].tolist() == [0, 0, -1, 0, 1, 0, 2, 0, 0]
    # Philox by GLOBAL env id modulo 2^32 and frame column: local env 3 at offset 2^32 - 3 is env 0
    import philox
    c = Case("hand", 5, [it("ext", 2), it("ext", 3, noise=1.0)], env_offset=2 ** 32 - 3)
    u = oc.draws_of(c, {}, 2, 3, 1)
    assert np.array_equal(u[3:5], philox.uniform(c.seed, c.stream + 1, 2, 5)[:, 2:5]) and not np.array_equal(u[0], u[3])
    # history: newest first; the first call's older frames are what it found in prev_obs
    c = oc.CASES["hist-width3-frames5-n1"]
    w = oc.expected(c.name)
    assert np.array_equal(w[0].full[:, 0], w[0].f32) and np.array_equal(w[0].full[:, 1:], c.prev0()[:, :-1])
    assert np.array_equal(w[2].full[:, 2], w[0].f32) and np.array_equal(w[2].full[:, 1], w[1].f32) and np.array_equal(w[2].full[:, 4], c.prev0()[:, 1])
    assert not np.array_equal(w[1].f32, w[0].f32)


def test_the_float32_restatement_errs_where_the_bound_is_used():
    """The 4 x bound is relative to the float32 restatement's own error: that error is not zero in any case that uses it, and the
    copied columns hold integers (times one scale), so a dropped or shifted column is off by far more than a rounding."""
    for name in oc.NAMES:
        case, exact = oc.CASES[name], oc.CASES[name].exact_columns()
        for w in oc.expected(name):
            if not exact.all():
                assert np.abs(w.f32.astype(np.float64) - w.f64)[:, ~exact].max() > 0.0, name
            assert np.array_equal(w.f32[:, exact].astype(np.float64), w.f64[:, exact].astype(np.float32).astype(np.float64)), name
        col = 0
        for x in case.items:
            if exact[col] and x.scale == 1.0 and x.kind != "base_quat":   # (a copied unit quaternion is no integer)
                v = oc.expected(name)[0].f32[:, col:col + x.width]
                assert np.array_equal(v, np.rint(v)), (name, x)
            col += x.width


def _tiles():
    return [(c, t) for c in oc.CASES.values() for t in oc.dispatch(c)]


def test_the_table_reaches_every_named_edge():
    tiles = _tiles()
    C = oc.CASES

    def some(what, pred):
        assert any(pred(c, t) for c, t in tiles), f"no case reaches: {what}"

    assert set(c.n for c in C.values()) <= set(oc.SIZES) and max(c.n for c in C.values()) <= 193
    # plan / tables
    some("48 units, planned", lambda c, t: t.U == 48 and t.planned)
    some("49 units, tables in LDS", lambda c, t: t.U == 49 and not t.planned)
    some("8 per-env items, planned", lambda c, t: t.owners == 8 and t.planned)
    some("9 per-env items, tables in LDS", lambda c, t: t.owners == 9 and t.U >= 1 and not t.planned)
    some("no gather unit, H = 1", lambda c, t: t.U == 0 and c.H == 1 and not t.planned)
    some("no gather unit, H = 3", lambda c, t: t.U == 0 and c.H == 3 and t.flat)
    some("one unit", lambda c, t: t.U == 1 and t.planned)
    # lane mapping
    for u in oc.LANE_UNITS:
        some(f"U = {u} one-float units, a second tile of one row", lambda c, t: t.U == u and t.scalar_units == u and c.O == u and c.n == 65 and t.rows == 1)
    assert {t.lgP for _c, t in tiles} >= {0, 1, 4, 5, 6, 7, 8}
    some("eight gather passes over a full tile at U = 129", lambda c, t: t.U == 129 and c.n == 64 and t.rows == 64 and t.gather_passes == 8)
    for p in (1, 2, 4, 8):
        some(f"{p} gather passes", lambda c, t: t.gather_passes == p)
    # gather units
    unit = lambda name: oc.units_of(C[name])[0]
    assert [w for _c, w in unit("gather-vec-stride12")] == [4] * 3 and [w for _c, w in unit("gather-vec-stride16")] == [4] * 3
    for name, n_units in (("gather-scalar-source4off", 12), ("gather-scalar-stride13", 12), ("gather-scalar-width14", 14)):
        assert [w for _c, w in unit(name)] == [1] * n_units, name
    assert C["gather-scalar-source4off"].off == {"dof_pos": 1} and C["gather-scalar-stride13"].items[0].stride == 13
    assert C["gather-scalar-width14"].items[0].stride == 16 and C["gather-vec-stride16"].items[0].stride == 16 and C["gather-vec-stride12"].D == 12
    mixed = unit("gather-interleaved")
    assert any(w == 4 and c % 4 for c, w in mixed) and any(w == 1 for _c, w in mixed) and "vec-unit-at-odd-column" in oc.edges_of(C["gather-interleaved"])
    for links in (1, 6):
        last = C["gather-norm%d-last" % links].items[-1]
        assert last.kind == "norm" and last.width == links
    # write-out without history
    for o in oc.WRITE_WIDTHS:
        for off in (0, 2, 1):
            some(f"O = {o}, H = 1, obs {off} floats off", lambda c, t: c.O == o and c.H == 1 and not c.ring and c.off.get("obs", 0) == off)
    for v in (4, 2, 1):
        some(f"V = {v} without history", lambda c, t: c.H == 1 and t.V == v and c.family == "write")
    # history, not a ring
    for o, h in oc.HIST_SHAPES:
        for n in (1, 63, 65):
            some(f"(O, H) = ({o}, {h}) at n = {n}, three calls", lambda c, t: (c.O, c.H, c.n, c.calls) == (o, h, n, 3) and not c.ring and not c.off)
    for tail in (1, 2, 3):
        some(f"tail = {tail}", lambda c, t: t.flat and t.tail == tail and c.family == "hist")
    some("three history batches or more", lambda c, t: t.hist_batches >= 3)
    some("two passes of write_mixed_units or more", lambda c, t: t.mixed_passes >= 2)
    some("exactly one full pass of write_mixed_units", lambda c, t: t.mixed_passes == 1 and t.rows * (((c.O + 3) >> 2) + 1) == oc.K["MIXED_UNITS"] * oc.K["OBS_BLOCK"])
    some("O (H - 1) = 4 on the flat path", lambda c, t: t.flat and c.O * (c.H - 1) == 4)
    some("element history, V = 1, obs 4 bytes off", lambda c, t: c.H > 1 and not c.ring and not t.flat and t.V == 1 and c.off.get("obs") == 1)
    some("element history, V = 2, obs 8 bytes off, even O", lambda c, t: c.H > 1 and not c.ring and not t.flat and t.V == 2 and c.off.get("obs") == 2 and c.O % 2 == 0)
    some("element history of a frame narrower than 4", lambda c, t: c.H > 1 and not c.ring and not t.flat and c.O < 4 and not c.off)
    some("flat path, prev_obs dword aligned only", lambda c, t: t.flat and c.off.get("prev_obs", 0) % 4 != 0 and c.off.get("obs", 0) == 0)
    # ring
    for o in (3, 6, 8):
        for slots in (0, 3, 6):
            last = slots or 3
            some(f"ring, O = {o}, ring_slots = {slots}: slot 1, the last and one between",
                 lambda c, t: c.ring and c.O == o and c.ring_slots == slots and c.H == 3 and c.ring[0] == 1 and c.ring[1] == last and 1 < c.ring[2] < last)
    # noise
    for src in ("philox", "dense"):
        for eo in (0, 1000, 2 ** 32 - 3):
            some(f"{src} noise at env_offset {eo}", lambda c, t: c.family == "noise" and c.noise == src and c.env_offset == eo and c.n == 65
                 and ("noise_draws" in c.inputs(0)) == (src == "dense"))
    items = C["noise-philox-offset0"].items
    assert any(a.noise != 0 and b.noise == 0 for a, b in zip(items, items[1:])) and any(a.noise == 0 and b.noise != 0 for a, b in zip(items, items[1:]))
    assert any(x.scale == 1.0 and x.noise != 0 for x in items) and any(x.scale != 1.0 and x.noise == 0 for x in items)
    assert any(x.noise != 0 and w == 4 for x in items for w in [oc.units_of(Case("one", 65, [x]))[0][0][1]])   # … and through a 16-byte unit
    # stale quaternion
    has = lambda name: {k for k in ("stale_quat", "stale_mask", "stale_mask2") if k in C[name].inputs(0)}
    assert has("stale-null") == set() and has("stale-mask1") == {"stale_quat", "stale_mask"} and has("stale-mask2") == {"stale_quat", "stale_mask2"}
    assert has("stale-both") == has("stale-zeros") == has("stale-ones") == {"stale_quat", "stale_mask", "stale_mask2"} and has("stale-nomasks") == {"stale_quat"}
    d = C["stale-both"].inputs(0)
    m1, m2 = d["stale_mask"] != 0, d["stale_mask2"] != 0
    assert (m1 & ~m2).any() and (m2 & ~m1).any() and (~m1 & ~m2).any()   # the union differs from either mask
    assert not C["stale-zeros"].inputs(0)["stale_mask"].any() and C["stale-ones"].inputs(0)["stale_mask2"].all()
    for name in oc.NAMES:
        if name.startswith("stale-"):
            assert C[name].n == 65 and C[name].needs_body()
    # the chain's frames
    for n in CHAIN_SIZES:
        runs = {run: [(c, oc.dispatch(c, chain=True)[0]) for c in _chain_cases(n, run)] for run in CHAIN_RUNS}
        every = [ct for cts in runs.values() for ct in cts]
        assert not any(t.planned for _c, t in every)
        assert any(t.U == 49 for _c, t in every) and any(t.U == 0 and c.H == 3 for c, t in every)
        assert any(t.flat and c.O % 2 == 1 for c, t in every) and any(c.H > 1 and not t.flat and t.V == 2 for c, t in every)
        (c0, t0), (c1, t1) = runs["reset-command-narrow-wide"]
        assert c0.O < c1.O and (t0.V, t1.V) == (4, 1) and c0.H == c1.H == 1
        (c0, t0), (c1, t1) = runs["reset-command-wide-narrow"]
        assert c0.O > c1.O and (t0.V, t1.V) == (1, 4) and c0.O == oc.K["MAX_WIDTH"] - 1
    assert max(len(frames) for _cmd, frames in CHAIN_RUNS.values()) == oc.K["CHAIN_OBS"]


# ---- both backends ----------------------------------------------------------------------------------------------------------------------
def _chain_cases(n, run, command_rows=None):
    """The observation managers of a run.  In a run with a command op the first manager's first item is that op's [n, 4] command
    rows as this very run resamples them (``command_rows``: the restated rows; None: zeros, for the dispatch model)."""
    with_command, frames = CHAIN_RUNS[run]
    cases = [oc.CHAIN_FRAMES[f](n) for f in frames]
    if with_command:
        first = cases[0]
        data = dict(first.inputs(0))
        data["cmd.0"] = command_rows if command_rows is not None else np.zeros((n, 4), np.float32)
        cases[0] = Case(first.name, n, [it("cmd", 4, scale=0.5)] + [x._replace(src=None) for x in first.items], D=first.D, H=first.H, off=first.off,
                        stale=first.stale, calls=1, data=data)
    return cases


def _chain(backend, dev, n, run):
    with_command, frames = CHAIN_RUNS[run]
    reset = rc.reset_spec(n, D=12, T=5, mask="three_groups", spawn=True)
    command = rc.command_spec(n, R=4, mode=rc.CMD_MASKED, mask="three_groups")
    specs = [reset] + ([command] if with_command else [])
    wants = [rc.restate(s) for s in specs]
    cases = _chain_cases(n, run, wants[1][0]["command"] if with_command else None)
    expect = [oc.expected_of(c) for c in cases]
    for chain in (1, 0):
        if backend.name == "hip":
            backend.set_option(nat.GF_OPT_CHAIN, chain)
        try:
            ls = [rc.Launch(dev, s) for s in specs]
            obs = [oc.Launch(dev, c, w) for c, w in zip(cases, expect)]
            for o in obs:
                o.prepare(0)
            if with_command:
                obs[0].args.command[0].command = ls[1].bufs["command"].ptr
                del obs[0].src["cmd.0"], obs[0].snap["src"]["cmd.0"]   # (the command launch owns and checks that buffer)
            assert rc.run_ops(backend, ls + obs) == (0, -1)
        finally:
            if backend.name == "hip":
                backend.set_option(nat.GF_OPT_CHAIN, 1)
        for i, (l, (w, st)) in enumerate(zip(ls, wants)):
            l.check(w, st, f"op {i} of {run}, chain option {chain}, {n} envs")
        for f, o in zip(frames, obs):
            e = o.check(0, f"{run}: frame {f}, chain option {chain}, {n} envs")
            if e is not None:
                oc.within(f"chain-{f} ({run}, option {chain}, n {n})", [e])
        if backend.name != "hip":
            break


@pytest.mark.parametrize("name", oc.NAMES)
def test_oracle_equals_the_restatement(oracle_backend, name):
    oc.run_case(oracle_backend, "cpu", name)


@pytest.mark.parametrize("run", sorted(CHAIN_RUNS))
@pytest.mark.parametrize("n", CHAIN_SIZES)
def test_oracle_runs_the_ops_like_the_restatement(oracle_backend, n, run):
    _chain(oracle_backend, "cpu", n, run)


@pytest.mark.gpu
@pytest.mark.parametrize("name", oc.NAMES)
def test_kernel_equals_the_restatement(hip_backend, name):
    oc.run_case(hip_backend, "cuda", name)


@pytest.mark.gpu
@pytest.mark.parametrize("run", sorted(CHAIN_RUNS))
@pytest.mark.parametrize("n", CHAIN_SIZES)
def test_chain_and_separate_launches_equal_the_restatement(hip_backend, n, run):
    _chain(hip_backend, "cuda", n, run)
