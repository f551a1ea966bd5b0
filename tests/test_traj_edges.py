"""gf_traj_table and gf_traj_gather through the raw C ABI, at the sizes where the scan, the segment walk and the grid-stride loops take
another shape (tests/traj_cases.py has the cases, the plain-loop reference and the launch restated).

* the table at N around a wave (63 / 64 / 65), a chunk of 256 envs (255 / 256 / 257) and several chunks (511 / 512 / 513, 1 025), with
  dones patterns whose counts differ from lane to lane and one "hot" env on either side of a wave and of a chunk;
* the gather on a table that comes from the reference (a gather failure is not a table failure): strided segments whose gap columns
  hold NaN, one / two / four segments, widths up to GF_MLP_MAX_INPUT_WIDTH, hidden sizes up to GF_MLP_MAX_HIDDEN, every combination of
  absent / LSTM / GRU the two slots are used with, minibatches with env_start > 0, and the three grid-stride loops past the 4 096 x 256
  lanes of the capped launch;
* every output a slice of a guarded, sentinel-filled buffer (tests/guarded.py): each element equals the reference bit for bit — so
  nothing is left unwritten and padding is +0.0 — and no guard byte changes.
The CPU twins check the reference itself against rsl_rl's lines (tests/rsl_rl_recurrent.py)."""
import functools

import pytest
import torch

import rsl_rl_recurrent as R
import traj_cases as tc
from genesis_forge_amd import _native as nat
from guarded import FILL, Guarded, raw_call, sync

GATHER_NAMES = [c.name for c in tc.GATHER_CASES]


def _bits(x):
    return x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ---- the reference against rsl_rl's lines (CPU) ---------------------------------------------------------------------------------------
def test_constants_are_the_headers():
    assert (tc.MAX_INPUTS, tc.MAX_WIDTH, tc.MAX_HIDDEN) == (nat.GF_MLP_MAX_INPUTS, nat.GF_MLP_MAX_INPUT_WIDTH, nat.GF_MLP_MAX_HIDDEN)


@pytest.mark.parametrize("N", tc.TABLE_N)
def test_reference_table_is_rsl_rls_split(N):
    """counts, offsets and (env, t0, len) of the loop reference against the done indices rsl_rl's split_and_pad_trajectories cuts at."""
    for T in tc.TABLE_T:
        for pattern in tc.patterns_of(N):
            dones, counts, offsets, table = tc.table_case(T, N, pattern)
            d = dones.clone().bool()
            d[-1] = True
            ends = d.transpose(1, 0).reshape(-1).nonzero()[:, 0]
            starts = torch.cat([torch.zeros(1, dtype=torch.int64), ends[:-1] + 1])
            assert torch.equal(table, torch.stack([starts // T, starts % T, ends - starts + 1], dim=1).to(torch.int32)), (T, pattern)
            assert torch.equal(counts, d.sum(0).to(torch.int32)) and int(offsets[0]) == 0
            assert torch.equal(offsets[1:].long(), counts.long().cumsum(0)), (T, pattern)
            _padded, masks = R.split_and_pad_trajectories(torch.zeros(T, N, 1), dones.bool())
            assert torch.equal(masks.sum(0).to(torch.int32), table[:, 2]) and masks.shape[1] == int(offsets[N])


def test_table_patterns_are_what_they_claim():
    T, N = 24, 513
    ramp = tc.make_dones(T, N, "ramp")
    assert ramp.sum(0).tolist() == [n % T for n in range(N)]
    counts = tc.table_case(T, N, "ramp")[1]
    assert bool((counts[1:] != counts[:-1]).all()), "neighbouring counts differ"
    for chunk in (0, 1):   # (n % T repeats every 192 envs at T = 24, so the first and the last wave of a chunk agree: ramp7 is for the waves)
        waves = tc.table_case(T, N, "ramp7")[1][256 * chunk:256 * chunk + 256].view(4, 64).sum(1).tolist()
        assert len(set(waves)) == 4, "the four wave totals of a chunk differ"
    for k in tc.HOT_ENVS:
        d = tc.make_dones(T, N, f"hot{k}")
        assert int(d.sum()) == T and bool(d[:, k].all())
    assert [p for p in tc.patterns_of(64) if p.startswith("hot")] == ["hot63"] and len(tc.patterns_of(257)) == len(tc.PATTERNS)
    assert 0 < int(tc.make_dones(T, N, "random0.1").sum()) < int(tc.make_dones(T, N, "random0.5").sum()) < T * N


@functools.lru_cache(maxsize=None)
def _ref(name, mb):
    """The reference outputs of one minibatch of a case: computed once, shared, never written."""
    return tc.ref_gather(tc.build(name), *mb)


def _saved(start, dones):
    """rsl_rl's per-step [T, 1, N, H]: the rollout-start state, zeros behind a done, anything elsewhere."""
    T, N = dones.shape
    g = torch.Generator().manual_seed(9)
    x = torch.randn(T, 1, N, start.shape[1], generator=g)
    x[0, 0] = start
    x[1:, 0][dones[:-1].bool()] = 0.0
    return x


@pytest.mark.parametrize("name", GATHER_NAMES)
def test_reference_gather_is_rsl_rl(name):
    """The loop reference against split_and_pad_trajectories (padded values, masks), recurrent_mini_batches fed per-step saved states
    (h0, c0, each minibatch's trajectory range) and unpad_trajectories (index_select with the reference's index)."""
    inp = tc.build(name)
    T, N, dones = inp.T, inp.N, inp.dones.bool()
    obs = [None if gr is None else tc.observations(inp, k) for k, gr in enumerate(inp.groups)]
    assert all(o is None or not bool(torch.isnan(o).any()) for o in obs), "no gap column is part of an observation"
    assert all(st is None or bool((st.h_start != 0).all()) for st in inp.states)
    saved = [() if st is None else tuple(_saved(s, dones) for s in (st.h_start, st.c_start) if s is not None) for st in inp.states]
    g = torch.Generator().manual_seed(2)
    for M in inp.case.splits:
        want = list(R.recurrent_mini_batches(obs[0], obs[0] if obs[1] is None else obs[1], dones, saved[0], saved[1], M, 1))
        bounds, offs = tc.bounds_of(N, M), inp.offsets.tolist()
        assert len(want) == M
        for i, w in enumerate(want):
            e0, e1 = bounds[i], bounds[i + 1]
            assert (w.env_start, w.env_stop) == (e0, e1)
            mb = (e0, e1, offs[e0], offs[e1] - offs[e0])
            assert mb in tc.minibatches(inp)
            ref = _ref(name, mb)
            assert _same_bits(ref["dst0"], w.obs), (name, M, i)
            if obs[1] is not None:
                assert _same_bits(ref["dst1"], w.critic_obs), (name, M, i)
            assert torch.equal(ref["masks"].bool(), w.masks) and set(ref["masks"].unique().tolist()) <= {0, 1}
            for k, (st, hid) in enumerate(zip(inp.states, (w.hid_a, w.hid_c))):
                if st is None:
                    continue
                assert _same_bits(ref[f"h0_{k}"], hid[0][0]) and (st.c_start is None or _same_bits(ref[f"c0_{k}"], hid[1][0])), (name, M, i, k)
                assert (f"c0_{k}" in ref) == (st.kind == "lstm") and len(hid) == (2 if st.kind == "lstm" else 1)
            index = ref["unpad_index"]
            assert int(index.min()) >= 0 and index.unique().numel() == (e1 - e0) * T, "every step of every env, once"
            x = torch.randn(T, mb[3], 2, generator=g)
            assert torch.equal(x.transpose(1, 0).reshape(-1, 2).index_select(0, index).view(-1, T, 2).transpose(1, 0), R.unpad_trajectories(x, w.masks))


def test_cases_reach_every_path():
    """From the cases themselves and the launch restated in traj_cases.gather_plan."""
    seen = set()
    for c in tc.GATHER_CASES:
        inp = tc.build(c.name)
        for mb in tc.minibatches(inp):
            seen |= tc.paths_of(inp, *mb)
    assert tc.REQUIRED_PATHS <= seen, sorted(tc.REQUIRED_PATHS - seen)
    floor = tc.CAP * tc.LANES
    assert floor == 1048576
    for name, job in tc.STRIDE_CASES.items():
        inp = tc.build(name)
        (mb,) = tc.minibatches(inp)
        J = mb[3]
        jobs, blocks, strided = tc.gather_plan(inp.T, J, [0 if g is None else g.W for g in inp.groups], [0 if s is None else s.H for s in inp.states])
        assert blocks == min(-(-max(jobs.values()) // 256), 4096) == 4096
        assert jobs[job] == max(jobs.values()) > floor and job in strided, (name, jobs)
    obs = tc.build("stride-observations")
    assert 8 * obs.table.shape[0] * 1024 >= 1064960 == 8 * 130 * 1024
    assert 24 * tc.build("stride-rows").table.shape[0] == 1048896 and tc.build("stride-states").table.shape[0] * 512 == 1075200
    # before this file the largest launch was a third of 1 025 envs with all 24 steps done, W = 8 and 7, H = 6 and 4: the observation loops
    # strode there (on contiguous rows), the loop over the masks and the index and the loops over the states never did
    assert tc.gather_plan(24, 342 * 24, [8, 7], [6, 4])[2] == {"obs0", "obs1"}


# ---- gf_traj_table, raw ----------------------------------------------------------------------------------------------------------------
def _table_launch(backend, dev, dones_dev, T, N):
    counts, offsets, table = Guarded(N, torch.int32, dev), Guarded(N + 1, torch.int32, dev), Guarded(T * N * 3, torch.int32, dev)
    a = nat.GfTrajTableArgs()
    a.num_steps, a.num_envs, a.dones = T, N, dones_dev.data_ptr()
    a.counts, a.offsets, a.table = counts.ptr, offsets.ptr, table.ptr
    assert raw_call(backend, "traj_table", a) == 0
    sync(dev)
    return counts, offsets, table


def _check_table(got, want, T, N, tag):
    counts, offsets, table = got
    _dones, wc, wo, wt = want
    J = wt.shape[0]
    assert counts.guards_ok() and offsets.guards_ok() and table.guards_ok(), ("a guard", tag)
    assert torch.equal(counts.cpu(), wc), ("counts", tag)
    assert torch.equal(offsets.cpu(), wo), ("offsets", tag)
    rows = table.cpu().view(T * N, 3)
    assert torch.equal(rows[:J], wt), ("table", tag)
    assert bool((rows[J:].contiguous().view(torch.uint8) == FILL).all()), ("a table row from offsets[N] on was written", tag)


@pytest.mark.gpu
@pytest.mark.parametrize("N", tc.TABLE_N)
def test_traj_table_hip(hip_backend, N):
    for T in tc.TABLE_T:
        for pattern in tc.patterns_of(N):
            want = tc.table_case(T, N, pattern)
            dones = want[0].cuda()
            first = _table_launch(hip_backend, "cuda", dones, T, N)
            _check_table(first, want, T, N, (T, N, pattern))
            again = _table_launch(hip_backend, "cuda", dones, T, N)
            assert all(torch.equal(x.raw, y.raw) for x, y in zip(first, again)), ("two launches differ", T, N, pattern)


# ---- gf_traj_gather, raw ---------------------------------------------------------------------------------------------------------------
class _Sources:
    """The inputs of a case on the device, uploaded once per case."""

    def __init__(self, inp, dev):
        self.segs = [None if gr is None else [s.wide.to(dev) for s in gr.segs] for gr in inp.groups]
        self.norm = [None if gr is None or gr.store is None else tuple(x.to(dev) for x in gr.store) for gr in inp.groups]
        self.states = [None if st is None else (st.h_start.to(dev), None if st.c_start is None else st.c_start.to(dev)) for st in inp.states]


def _gather_launch(backend, dev, inp, src, mb, table_dev, table_rows):
    """One launch into fresh guarded buffers: {name: Guarded}."""
    e0, e1, j0, J = mb
    T = inp.T
    a = nat.GfTrajGatherArgs()
    a.num_steps, a.num_envs, a.first_traj, a.num_traj, a.env_start, a.num_mb_envs = T, inp.N, j0, J, e0, e1 - e0
    a.table, a.table_rows = table_dev, table_rows
    out = {}
    for k, gr in enumerate(inp.groups):
        if gr is None:
            continue
        d = a.groups[k]
        d.num_inputs, d.width = len(gr.segs), gr.W
        for seg, s, t in zip(d.inputs, gr.segs, src.segs[k]):
            seg.rows, seg.width, seg.row_stride = t.data_ptr() + 4 * s.off, s.width, s.row_stride
        if gr.mean is not None:
            off = 4 if gr.sliced else 0
            d.mean, d.std, d.eps = src.norm[k][0].data_ptr() + off, src.norm[k][1].data_ptr() + off, gr.eps
        out[f"dst{k}"] = Guarded(T * J * gr.W, torch.float32, dev)
        d.dst = out[f"dst{k}"].ptr
    for k, st in enumerate(inp.states):
        if st is None:
            continue
        d = a.states[k]
        d.hidden, d.h_start = st.H, src.states[k][0].data_ptr()
        out[f"h0_{k}"] = Guarded(J * st.H, torch.float32, dev)
        d.h0 = out[f"h0_{k}"].ptr
        if st.kind == "lstm":
            d.c_start = src.states[k][1].data_ptr()
            out[f"c0_{k}"] = Guarded(J * st.H, torch.float32, dev)
            d.c0 = out[f"c0_{k}"].ptr
    out["masks"], out["unpad_index"] = Guarded(T * J, torch.uint8, dev), Guarded((e1 - e0) * T, torch.int64, dev)
    a.masks, a.unpad_index = out["masks"].ptr, out["unpad_index"].ptr
    assert raw_call(backend, "traj_gather", a) == 0
    sync(dev)
    return out


def _check_gather(got, ref, tag):
    assert set(got) == set(ref), tag
    for k, want in ref.items():
        assert got[k].guards_ok(), ("a guard of " + k, tag)
        have = got[k].cpu().view(want.shape)
        if k == "masks":
            assert set(have.unique().tolist()) <= {0, 1}, ("masks holds a byte other than 0 and 1", tag)
        assert torch.equal(_bits(have), _bits(want)), (k, tag, f"{int((_bits(have) != _bits(want)).sum())} of {want.numel()} elements differ")


def _run_gather_case(backend, dev, name):
    inp = tc.build(name)
    src = _Sources(inp, dev)
    rows = inp.table.shape[0]
    table = Guarded(rows * 3, torch.int32, dev, init=inp.table)   # exactly table_rows rows: nothing behind them to read
    for mb in tc.minibatches(inp):
        ref = _ref(name, mb)
        first = _gather_launch(backend, dev, inp, src, mb, table.ptr, rows)
        _check_gather(first, ref, (name, mb))
        again = _gather_launch(backend, dev, inp, src, mb, table.ptr, rows)
        assert all(torch.equal(first[k].raw, again[k].raw) for k in first), ("two launches differ", name, mb)
    assert table.guards_ok() and torch.equal(table.cpu().view(-1, 3), inp.table), "the table changed"
    for k, gr in enumerate(inp.groups):
        for s, t in zip(gr.segs if gr else (), src.segs[k] or ()):
            assert torch.equal(_bits(t.cpu()), _bits(s.wide)), "a source changed"


@pytest.mark.gpu
@pytest.mark.parametrize("name", GATHER_NAMES)
def test_traj_gather_hip(hip_backend, name):
    _run_gather_case(hip_backend, "cuda", name)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [65, 257])
def test_table_then_gather_hip(hip_backend, N):
    """gf_traj_table, then gf_traj_gather on its output: the table is asserted against the reference before the gather is launched."""
    name = {65: "four-segments", 257: "ramp"}[N]
    inp = tc.build(name)
    assert (inp.T, inp.N) == (24, N)
    got = _table_launch(hip_backend, "cuda", inp.dones.cuda(), inp.T, N)
    _check_table(got, (inp.dones, inp.counts, inp.offsets, inp.table), inp.T, N, name)
    src = _Sources(inp, "cuda")
    for mb in tc.minibatches(inp):
        _check_gather(_gather_launch(hip_backend, "cuda", inp, src, mb, got[2].ptr, int(inp.offsets[N])), _ref(name, mb), (name, mb))


# ---- through the storage ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_storage_generator_is_rsl_rl_hip(hip_backend):
    """recurrent_mini_batch_generator on the HIP path at N = 257, T = 24, M = 3 — groups of width 48 and 235 (three segments, one shared),
    a 256-unit LSTM actor and GRU critic, both groups normalised — against rsl_rl's generator fed per-step saved states."""
    from genesis_forge_amd.learner import EmpiricalNormalization
    from test_recurrent import _stub_storage

    T, N, M, H = 24, 257, 3, 256
    g = torch.Generator().manual_seed(5)
    dones = tc.make_dones(T, N, "random0.1", seed=3).bool()
    rows = {k: torch.randn(T, N, w, generator=g) for k, w in (("a", 41), ("b", 7), ("c", 194))}
    groups = {"policy": ["a", "b"], "critic": ["a", "c"]}
    nz = lambda: torch.randn(N, H, generator=g).abs() + 0.25
    start = {"actor": (nz(), nz()), "critic": (nz(), None)}
    norms, cpu_norms = [], []
    for w in (48, 235):
        stats = torch.randn(w, generator=g), torch.rand(w, generator=g) + 0.5
        for dev, into in (("cuda", norms), ("cpu", cpu_norms)):
            norm = EmpiricalNormalization(w).to(dev)
            with torch.no_grad():
                norm._mean.copy_(stats[0])
                norm._std.copy_(stats[1])
            into.append(norm)
    eps = [torch.tensor(n.eps, dtype=torch.float32) for n in cpu_norms]
    obs = (torch.cat([rows["a"], rows["b"]], -1) - cpu_norms[0]._mean) / (cpu_norms[0]._std + eps[0])
    cobs = (torch.cat([rows["a"], rows["c"]], -1) - cpu_norms[1]._mean) / (cpu_norms[1]._std + eps[1])
    saved = lambda state: tuple(_saved(s, dones) for s in state if s is not None)
    want = list(R.recurrent_mini_batches(obs, cobs, dones, saved(start["actor"]), saved(start["critic"]), M, 1))
    st = _stub_storage(hip_backend, "cuda", T, N, dones, rows, groups, start)
    got = list(st.recurrent_mini_batch_generator(M, 1, tuple(norms)))
    assert len(got) == len(want) == M
    tn = (torch.arange(T) * N)[:, None] + torch.arange(N)[None, :]
    for b, w in zip(got, want):
        assert b.masks.dtype == torch.bool and torch.equal(b.masks.cpu(), w.masks)
        assert _same_bits(b.obs.cpu(), w.obs) and _same_bits(b.critic_obs.cpu(), w.critic_obs)
        assert _same_bits(b.hid_a[0].cpu(), w.hid_a[0]) and _same_bits(b.hid_a[1].cpu(), w.hid_a[1]) and _same_bits(b.hid_c.cpu(), w.hid_c[0])
        assert torch.equal(b.rows.cpu(), tn[:, w.env_start:w.env_stop].reshape(-1))
        x = torch.randn(T, w.masks.shape[1], 2, generator=g)
        assert torch.equal(x.transpose(1, 0).reshape(-1, 2).index_select(0, b.unpad_index.cpu()).view(-1, T, 2).transpose(1, 0), R.unpad_trajectories(x, w.masks))
