"""contact_tile() (gf_contact_tile.h) at its tile-size, mask-word and slot-loop boundaries: the stand-alone launch (gf_contact.hip),
the contact phase of the fused post-physics launch (gf_post.hip / gf_post_ws.h) and the oracle's gfo_contact_step against a plain
numpy restatement of the reference (tests/contact_cases.py), which two CPU tests anchor to recorded reference outputs.

* exact leg: integer forces and positions, Hurwitz quaternions, dt = 1/64 — float32 arithmetic is exact, so every output must EQUAL
  the restatement (by value: -0 == +0), whatever the tile size, the path the slot ids take into LDS and the number of mask words.
  The shapes are the table CASES; _plan() below restates contact_launch()'s choice of tile and thread count, and a CPU test
  asserts that the table still reaches every class it was chosen for.
* accuracy leg: random floats against the float64 restatement, within bounds counted from the operations
  (contact_cases.accuracy_bounds).
* the non-finite flag: raised if and only if a slot that a manager includes held a non-finite force component.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import contact_cases as cc
import helpers
from genesis_forge_amd import _native as nat

GUARD = 3            # rows behind the last env of every output buffer; they must survive a launch
AIR_POISON = -7.0    # guard rows of the air-time arrays (their first N rows are state)
AIR = ("last_air_time", "current_air_time", "last_contact_time", "current_contact_time")


# ----------------------------------------------------------------------------------------------------
# contact_launch()'s launch plan (gf_contact.hip) and the case table
# ----------------------------------------------------------------------------------------------------
def _plan(num_envs, C_, total):
    """What contact_launch() (gf_contact.hip) launches for num_envs envs, C_ slots per env and ``total`` tracked links, and what the
    workgroups then do in contact_tile(): None where the launch is refused."""
    c1 = C_ if C_ > 0 else 1
    lds = lambda e: e * (c1 + (c1 + 31) // 32) * 4
    blocks = lambda e: (num_envs + e - 1) // e
    E = max(1, min(64, 256 // total))
    while E > 1 and lds(E) > 16 * 1024:
        E -= 1
    if lds(E) > 48 * 1024:
        return None
    e_max = E
    while E > 8 and blocks(E) < 512:
        E >>= 1
    if C_ > 0:
        q, c = 32, C_
        while q > 1 and c % 2 == 0:
            q, c = q >> 1, c >> 1
        al = (e_max // q) * q
        while al > q and blocks(al) < 512:
            al -= q
        if al >= 1 and 4 * al >= 3 * E and blocks(al) >= 512:
            E = al
    threads = min(256, (E * total + 63) // 64 * 64)
    grid, lpp = blocks(E), threads // E
    paths, tails, loops = set(), set(), 0
    for b in range(grid):
        n0 = b * E
        here = min(E, num_envs - n0)
        vec = C_ > 0 and (n0 * C_) % 4 == 0
        slots4 = here * C_ // 4 if vec else 0
        paths.add("vector" if vec else "scalar")
        tails.add(here * C_ - 4 * slots4 if vec else 0)
        loops = max(loops, -(-slots4 // threads))
    tail_slots = [(min(num_envs, b * E + E) - 1, s) for b in range(grid) if C_ > 0 and (b * E * C_) % 4 == 0
                  for s in range(C_ - (min(E, num_envs - b * E) * C_) % 4, C_)]   # (env, slot) staged by the scalar loop behind a vector copy
    return dict(tail_slots=tail_slots, E=E, threads=threads, grid=grid, words=(C_ + 31) // 32, lpp=lpp, passes=-(-total // lpp), unit_loops=loops, paths=paths, tails=tails,
                idle_lanes=(threads - 1) // lpp >= E, last_envs=num_envs - (grid - 1) * E, lds=lds(E), lds_cut=e_max < min(64, 256 // total))


# (envs, C, tracked links, managers, what contact_launch() must make of it)
CASES = [
    (257, 9, 13, "auto", dict(E=4, threads=64, words=1, last_envs=1)),
    (300, 5, 17, "auto", dict(E=7, threads=128, idle_lanes=True, paths={"vector", "scalar"}, has_tail=3)),
    (200, 7, 40, "auto", dict(E=6, threads=256, has_tail=2)),
    (200, 7, 64, "four", dict(E=4, threads=256)),
    (130, 33, 4, "auto", dict(words=2, unit_loops=2)),
    (130, 65, 5, "auto", dict(words=3, E=6, has_tail=2)),
    (65, 64, 32, "one", dict(words=2)),
    (70, 300, 4, "auto", dict(lds_cut=True, words=10, unit_loops=8)),
    (40, 1000, 3, "auto", dict(E=3, words=32)),
    (20, 4095, 2, "auto", dict(E=1, words=128, has_tail=3, lds_over_16k=True)),
    (100, 0, 4, "auto", dict(words=0)),
    (8197, 8, 4, "auto", dict(E=16)),
    (16385, 30, 13, "auto", dict(E=16, threads=256)),
    (32771, 8, 4, "auto", dict(E=64, threads=256)),
    (32771, 12, 1, "auto", dict(E=64, threads=64, lpp=1, unit_loops=3)),
]
HIGH_IDS = 9   # this case's links go up to num_scene_links - 1 = 32 766
IDS = [f"{n}x{c}x{t}" for n, c, t, _, _ in CASES]


@functools.lru_cache(maxsize=None)
def _case(i):
    n, c, t, mode, _ = CASES[i]
    hi = dict(num_links=32767, id_max=32766) if i == HIGH_IDS else {}
    case = cc.make_case(n, c, t, seed=100 + i, mode=mode, **hi)
    return case, cc.expected_exact(case)


def test_case_table_reaches_every_dispatch_class():
    for (n, c, t, _, want), name in zip(CASES, IDS):
        p = _plan(n, c, t)
        for k, v in want.items():
            if k == "has_tail":
                assert v in p["tails"], (name, p)
            elif k == "lds_over_16k":
                assert p["lds"] > 16 * 1024, (name, p)
            elif k == "paths":
                assert p["paths"] >= v, (name, p)
            else:
                assert p[k] == v, (name, k, p)
        assert p["passes"] == 1, "the stand-alone launch sizes its workgroups for one pass"
    plans = [_plan(n, c, t) for n, c, t, _, _ in CASES]
    assert {1, 3, 4, 6, 7, 16, 64} <= {p["E"] for p in plans} and {64, 128, 256} == {p["threads"] for p in plans}
    assert {0, 1, 2, 3, 10, 32, 128} <= {p["words"] for p in plans}
    assert _plan(2, 12000, 1) is None and _plan(2, 11000, 1)["E"] == 1, "rows of one env beyond 48 KiB are refused"
    for i in range(len(CASES)):   # every case mixes the kinds of slots, and the non-finite components sit in included slots
        if CASES[i][1] == 0:
            continue
        case, want = _case(i)
        la, lb = case["inp"]["link_a"], case["inp"]["link_b"]
        tracked = np.concatenate([m["targets"] for m in case["mgrs"]])
        ta, tb = np.isin(la, tracked), np.isin(lb, tracked)
        assert (ta & ~tb).any() and (tb & ~ta).any() and (ta & (la == lb)).any(), IDS[i]
        assert ((la < 0) ^ (lb < 0)).any() and ((la < 0) & (lb < 0)).any() and any(m["withs"] is not None for m in case["mgrs"]), IDS[i]
        included = {(int(n), c) for m in case["mgrs"] for c, n_idx, _, _ in cc.matched_slots(la, lb, m["targets"], m["withs"]) for n in n_idx}
        p = _plan(*CASES[i][:3])
        assert not p["tail_slots"] or included & set(p["tail_slots"]), IDS[i] + ": no included contact in a scalar tail"
        assert p["unit_loops"] < 2 or any((n % p["E"]) * CASES[i][1] + c >= 4 * p["threads"] for n, c in included), IDS[i] + ": no included contact behind the first unit loop"
        assert p["words"] < 2 or {c >> 5 for _, c in included} >= {0, p["words"] - 1}, IDS[i] + ": first or last mask word without an included contact"
        assert want[0]["flag"] and all((w["position_counts"] > 0).any() for w in want), IDS[i]
    assert _case(HIGH_IDS)[0]["mgrs"][0]["targets"][0] == 32766


# ----------------------------------------------------------------------------------------------------
# the anchors: the restatement against recorded reference outputs
# ----------------------------------------------------------------------------------------------------
def test_restatement_matches_the_reference_on_the_contact_kernel_fixture(oracle_backend):
    """tests/golden/contact_kernel.npz: every step, all three managers, the tolerances of tests/test_contact_kernel.py."""
    import test_contact_kernel as tk

    fix = helpers.load("contact_kernel")
    env, _ = tk._env(int(fix["n"]), int(fix["C"]), "cpu")
    mgrs = []
    for cm in env.cms:
        a = cm._args
        mgrs.append(dict(targets=list(a.target_link_ids[:a.num_targets]), withs=list(a.with_link_ids[:a.num_with]) if a.has_with_filter else None,
                         threshold=a.air_time_threshold, dt=env.dt,
                         air=tuple(np.zeros((int(fix["n"]), a.num_targets), np.float32) for _ in range(4)) if a.track_air_time else None))
    assert [m["withs"] is not None for m in mgrs] == [False, True, True] and [m["air"] is not None for m in mgrs] == [True, False, True]
    for t in range(int(fix["steps"])):
        inp = {k: fix[k][t] for k in ("force", "position", "link_a", "link_b", "links_quat")}
        flags = []
        for k, m in enumerate(mgrs):
            r = cc.restate(inp, m["targets"], m["withs"], m["threshold"], m["air"], m["dt"])
            np.testing.assert_allclose(r["forces"], fix[f"m{k}_contacts"][t], atol=1e-5, rtol=0, err_msg=f"manager {k} forces, step {t}")
            np.testing.assert_allclose(r["positions"], fix[f"m{k}_contact_positions"][t], atol=1e-5, rtol=0, err_msg=f"manager {k} positions, step {t}")
            if m["air"] is not None:
                np.testing.assert_allclose(np.stack(r["air"]), fix[f"m{k}_air"][t], atol=1e-6, rtol=0, err_msg=f"manager {k} air time, step {t}")
                m["air"] = tuple(x.astype(np.float32) for x in r["air"])
            flags.append(r["flag"])
        assert any(flags) == (t == 2)


def test_restatement_matches_the_reference_on_the_contact_edges_fixture():
    """tests/golden/contact_edges.npz (tools/gen_golden.py contact_edges): 130 slots per env with self-contacts, one-sided and empty
    slots and non-finite forces, with and without the filter.  Evaluated in float32 the restatement takes the reference's steps in
    the reference's order (one rounding per operation, slots in slot order), so it reproduces the recorded float32 outputs bit for
    bit; in float64 it stays within the accuracy leg's bounds of them."""
    fix = helpers.load("contact_edges")
    inp = {k: fix[k] for k in ("force", "position", "link_a", "link_b", "links_quat")}
    assert inp["link_a"].shape[1] > 64
    for filt in (0, 1):
        withs = list(fix["withs"]) if filt else None
        want = {k: fix[f"f{filt}_{k}"] for k in ("contacts", "contact_positions", "counts")}
        r32 = cc.restate(inp, list(fix["targets"]), withs, dtype=np.float32)
        assert np.array_equal(r32["forces"], want["contacts"]) and np.array_equal(r32["positions"], want["contact_positions"])
        r = cc.restate(inp, list(fix["targets"]), withs)
        fb, pb, _ = cc.accuracy_bounds(r, 0.0)
        assert np.array_equal(r["counts"], want["counts"]) and r["flag"]
        assert (np.abs(r["forces"] - want["contacts"]) <= fb).all() and (np.abs(r["positions"] - want["contact_positions"]) <= pb).all()
        assert np.abs(want["contacts"]).max() > 30


# ----------------------------------------------------------------------------------------------------
# running a case through a backend
# ----------------------------------------------------------------------------------------------------
def _alloc(case, dev, misalign_ids=False, stats=None):
    """The case's arrays on ``dev`` and one GfContactArgs per manager: outputs poisoned, GUARD rows behind the last env."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    inp, N, Cn = case["inp"], case["N"], case["C"]
    bufs = {k: t(inp[k]) for k in ("force", "position", "links_quat", "links_vel", "links_pos")}
    for k in ("link_a", "link_b"):
        if misalign_ids:   # a view that starts 4 bytes behind a 16-byte boundary: every workgroup stages its ids one by one
            raw = torch.full((N * Cn + 8,), -1, dtype=torch.int32, device=dev)
            raw[1:1 + N * Cn] = t(inp[k]).reshape(-1)
            bufs[k + "_raw"], bufs[k] = raw, raw[1:1 + N * Cn]
            assert bufs[k].data_ptr() % 16 == 4
        else:
            bufs[k] = t(inp[k])
    mgrs = []
    for j, m in enumerate(case["mgrs"]):
        L = len(m["targets"])
        nan3 = lambda: torch.full((N + GUARD, L, 3), float("nan"), device=dev)
        out = dict(contacts=nan3(), contact_positions=nan3(), position_counts=torch.full((N + GUARD, L), -1.0, device=dev), link_vel=nan3(), link_pos=nan3())
        air = [torch.cat([torch.from_numpy(x), torch.full((GUARD, L), AIR_POISON)]).to(dev) for x in m["air"]]
        a = nat.GfContactArgs()
        a.num_envs, a.num_contacts, a.num_scene_links, a.num_targets = N, Cn, case["NL"], L
        a.num_with, a.has_with_filter, a.track_air_time = (len(m["withs"]), 1, 1) if m["withs"] is not None else (0, 0, 1)
        for k in ("force", "position", "link_a", "link_b", "links_quat", "links_vel", "links_pos"):
            setattr(a, k, bufs[k].data_ptr())
        a.link_vel_out, a.link_pos_out = out["link_vel"].data_ptr(), out["link_pos"].data_ptr()
        for w, x in enumerate(m["targets"]):
            a.target_link_ids[w] = x
        for w, x in enumerate(m["withs"] or ()):
            a.with_link_ids[w] = x
        a.air_time_threshold, a.dt = m["threshold"], case["dt"]
        a.contacts, a.contact_positions, a.position_counts = (out[k].data_ptr() for k in ("contacts", "contact_positions", "position_counts"))
        for k, x in zip(AIR, air):
            setattr(a, k, x.data_ptr())
        a.stats = stats[j] if stats is not None else None
        mgrs.append(dict(args=a, out=out, air=air))
    return dict(bufs=bufs, mgrs=mgrs, N=N)


def _step(backend, a):
    """gf_contact_step / gfo_contact_step; returns the status."""
    f = backend._fn["contact_step"]
    return f(C.byref(a), backend._stream()) if backend.name == "hip" else f(C.byref(a))


def _launch(backend, run):
    """One manager: the entry point itself; several: consecutive contact ops of one gf_run_ops (folded into as few launches as
    kContactMaxTargets allows)."""
    if len(run["mgrs"]) == 1:
        assert _step(backend, run["mgrs"][0]["args"]) == 0
    else:
        ops = (nat.GfOp * len(run["mgrs"]))()
        for k, m in enumerate(run["mgrs"]):
            ops[k].phase, ops[k].args = nat.GF_PHASE_CONTACT, C.addressof(m["args"])
        backend.run_ops(ops, len(run["mgrs"]))
    if backend.name == "hip":
        torch.cuda.synchronize()


def _check(run, want, what):
    N = run["N"]
    for j, (m, w) in enumerate(zip(run["mgrs"], want)):
        for k, x in m["out"].items():
            got = x.cpu().numpy()
            assert np.array_equal(got[:N], w[k]), f"{what}: manager {j} {k}: {int((got[:N] != w[k]).sum())} values differ, first at {np.argwhere(got[:N] != w[k])[:3].tolist()}"
            assert (np.isnan(got[N:]) if k != "position_counts" else got[N:] == -1.0).all(), f"{what}: manager {j} {k}: wrote behind the last env"
        for k, x, wa in zip(AIR, m["air"], w["air"]):
            got = x.cpu().numpy()
            assert np.array_equal(got[:N], wa), f"{what}: manager {j} {k}: {int((got[:N] != wa).sum())} values differ"
            assert (got[N:] == AIR_POISON).all(), f"{what}: manager {j} {k}: wrote behind the last env"


def _check_untouched(run, case, what):
    for m, cm in zip(run["mgrs"], case["mgrs"]):
        for k, x in m["out"].items():
            got = x.cpu().numpy()
            assert (np.isnan(got) if k != "position_counts" else got == -1.0).all(), f"{what}: {k} was written"
        for x, before in zip(m["air"], cm["air"]):
            assert np.array_equal(x.cpu().numpy()[:run["N"]], before), f"{what}: the air-time state changed"


def _flag(stats_t):
    return _stats_mod().sum_shards(stats_t.cpu().numpy().tobytes()).contact_flags


def _stats_mod():
    from genesis_forge_amd import _stats
    return _stats


# ----------------------------------------------------------------------------------------------------
# exact leg: the oracle (runs without a GPU) and the stand-alone launch
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_exact_oracle(oracle_backend, i):
    case, want = _case(i)
    run = _alloc(case, "cpu")
    _launch(oracle_backend, run)
    _check(run, want, "oracle " + IDS[i])


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_exact_standalone_hip(hip_backend, i):
    case, want = _case(i)
    run = _alloc(case, "cuda")
    _launch(hip_backend, run)
    _check(run, want, "hip " + IDS[i])


@pytest.mark.gpu
def test_exact_standalone_hip_slot_ids_off_16_byte_alignment(hip_backend):
    """link_a / link_b as views 4 bytes behind a 16-byte boundary: no workgroup may take the 16-byte path, the results are the same."""
    i = IDS.index("300x5x17")
    case, want = _case(i)
    run = _alloc(case, "cuda", misalign_ids=True)
    _launch(hip_backend, run)
    _check(run, want, "hip, slot ids off alignment")


def _split_case():
    return cc.make_case(150, 11, 90, seed=77, num_links=120, mode=[30, 30, 30])


def test_exact_oracle_three_managers_of_30_links(oracle_backend):
    case = _split_case()
    run = _alloc(case, "cpu")
    _launch(oracle_backend, run)
    _check(run, cc.expected_exact(case), "oracle, 90 links")


@pytest.mark.gpu
def test_exact_run_ops_splits_more_than_64_tracked_links(hip_backend):
    """Three consecutive managers of 30 links: 90 > kContactMaxTargets, so gf_run_ops launches twice (60 + 30) — same outputs."""
    case = _split_case()
    assert sum(len(m["targets"]) for m in case["mgrs"]) > 64
    run = _alloc(case, "cuda")
    _launch(hip_backend, run)
    _check(run, cc.expected_exact(case), "hip, 90 links")


@pytest.mark.gpu
def test_standalone_refusals_write_nothing(hip_backend):
    """What contact_launch() cannot stage is refused before anything is launched: the poisoned outputs and the air-time state stay."""
    case = cc.make_case(2, 12000, 1, seed=5)
    assert _plan(2, 12000, 1) is None
    run = _alloc(case, "cuda")
    a = run["mgrs"][0]["args"]
    assert _step(hip_backend, a) == -2, "rows of one env beyond 48 KiB of LDS: GF_E_RANGE"
    a.num_contacts = 11000   # (the same arrays read as shorter rows: accepted)
    assert _step(hip_backend, a) == 0
    torch.cuda.synchronize()
    case = cc.make_case(9, 6, 3, seed=6)
    run = _alloc(case, "cuda")
    for m in run["mgrs"]:
        m["args"].num_scene_links = 32768
        assert _step(hip_backend, m["args"]) == -2, "slot ids are staged as 16-bit pairs: 32 768 links is GF_E_RANGE"
        m["args"].num_scene_links = case["NL"]
    quat = torch.zeros(9 * case["NL"] * 4 + 4, device="cuda")
    quat[1:-3] = run["bufs"]["links_quat"].reshape(-1)
    for m in run["mgrs"]:
        m["args"].links_quat = quat[1:].data_ptr()
        assert m["args"].links_quat % 16 == 4 and _step(hip_backend, m["args"]) == -5, "links_quat off 16-byte alignment: GF_E_UNSUPPORTED"
        m["args"].links_quat = run["bufs"]["links_quat"].data_ptr()
    torch.cuda.synchronize()
    _check_untouched(run, case, "refused launches")
    _launch(hip_backend, run)
    _check(run, cc.expected_exact(case), "the same descriptors, accepted")


# ----------------------------------------------------------------------------------------------------
# exact leg: the contact phase of the fused post-physics launch
# ----------------------------------------------------------------------------------------------------
_HOSTS = {}


def _host(n):
    """A small fusable env of n envs whose post-physics launch carries the contact phase (any fusable step will do)."""
    if n not in _HOSTS:
        import envs

        host = envs.Go2CommandDirectionEnv(num_envs=n, max_episode_length_s=1, cmd_resample_s=0.3, contacts=True, scene_kwargs=dict(ang_noise=0.3, seed=3))
        host.build(); host.seed(3); host.reset()
        g = torch.Generator().manual_seed(0)
        for _ in range(6):
            host.step(torch.randn(n, 12, generator=g).to("cuda"))
        assert host._trace.post_refs is not None
        _HOSTS[n] = host
    return _HOSTS[n]


def _fused(backend, n, run, variant=2):
    """gf_post_physics_step_contacts with the run's managers folded regardless of size (GF_OPT_FOLD_CONTACT = 2); returns the status."""
    refs = _host(n)._trace.post_refs
    backend.set_option(nat.GF_OPT_FOLD_CONTACT, 2)
    backend.set_option(nat.GF_OPT_POST_VARIANT, variant)
    try:
        if variant == 0:
            assert backend.post_describe(refs).split(":")[0] == "program 0 (interpreter)"
        rc = backend.post_step_contacts(refs, [m["args"] for m in run["mgrs"]])
        torch.cuda.synchronize()
        return rc
    finally:
        backend.set_option(nat.GF_OPT_FOLD_CONTACT, 1)
        backend.set_option(nat.GF_OPT_POST_VARIANT, 2)


FUSED = [(1, 1), (31, 4), (32, 5), (33, 16), (64, 17), (65, 20), (128, 32)]


@functools.lru_cache(maxsize=None)
def _fused_case(n, c, t):
    case = cc.make_case(n, c, t, seed=1000 + 7 * c + n, num_links=255, id_max=254)
    if t >= 17:   # LPP = 4 in the 64-env tile: links 16 … land in passes >= 4, whose air-time state is read late
        assert sum(len(m["targets"]) for m in case["mgrs"][:-1]) <= 16 < t and all(m["air"] is not None for m in case["mgrs"])
    assert max(max(m["targets"]) for m in case["mgrs"]) == 254 and max(max(m["withs"]) for m in case["mgrs"] if m["withs"]) == 254
    return case, cc.expected_exact(case)


@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("c,t", FUSED, ids=[f"{c}x{t}" for c, t in FUSED])
def test_exact_oracle_fused_shapes(oracle_backend, n, c, t):
    case, want = _fused_case(n, c, t)
    run = _alloc(case, "cpu")
    _launch(oracle_backend, run)
    _check(run, want, f"oracle {n}x{c}x{t}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("c,t", FUSED, ids=[f"{c}x{t}" for c, t in FUSED])
def test_exact_fused_hip(hip_backend, n, c, t):
    case, want = _fused_case(n, c, t)
    run = _alloc(case, "cuda")
    assert _fused(hip_backend, n, run) == 0, "not folded"
    _check(run, want, f"fused {n}x{c}x{t}")
    stand = _alloc(case, "cuda")
    _launch(hip_backend, stand)
    _check(stand, want, f"stand-alone {n}x{c}x{t}")


@pytest.mark.gpu
@pytest.mark.parametrize("n,c,t", [(65, 65, 20), (130, 128, 32)])
def test_exact_fused_hip_table_interpreter(hip_backend, n, c, t):
    """GF_OPT_POST_VARIANT = 0 (= 1): the table interpreter keeps its descriptor in LDS and stages the slot ids behind it."""
    case, want = _fused_case(n, c, t)
    run = _alloc(case, "cuda")
    assert _fused(hip_backend, n, run, variant=0) == 0, "not folded"
    _check(run, want, f"fused, interpreter {n}x{c}x{t}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 130])
def test_exact_fused_hip_largest_slot_count_and_refusals(hip_backend, n):
    """The largest C the fold accepts with 32 tracked links (found by asking: the tile's slot ids, masks and tables must fit its LDS
    next to the descriptor — a little over 200), one more slot, and link ids beyond a byte: refused with nothing written."""
    probe = _alloc(cc.make_case(n, 512, 32, seed=3, num_links=255), "cuda")
    for b in ("link_a", "link_b"):
        probe["bufs"][b].fill_(-1)   # (read with other row lengths below: no slot holds a contact)

    def accepted(c):
        for m in probe["mgrs"]:
            m["args"].num_contacts = c
        rc = _fused(hip_backend, n, probe)
        assert rc in (0, -5), nat.GF_ERRORS.get(rc, rc)
        return rc == 0

    lo, hi = 128, 512
    assert accepted(lo) and not accepted(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if accepted(mid) else (lo, mid)
    print(f"fused, {n} envs, 32 links: the largest slot count the fold accepts is {lo}")
    assert 200 < lo < 240, lo
    case = cc.make_case(n, lo, 32, seed=4, num_links=255, id_max=254)
    run = _alloc(case, "cuda")
    assert _fused(hip_backend, n, run) == 0
    _check(run, cc.expected_exact(case), f"fused {n}x{lo}x32")
    case = cc.make_case(n, lo + 1, 32, seed=5, num_links=255, id_max=254)
    run = _alloc(case, "cuda")
    assert _fused(hip_backend, n, run) == -5
    _check_untouched(run, case, "one slot more than fits")
    case, want = _fused_case(n, 32, 5)
    run = _alloc(case, "cuda")
    a = run["mgrs"][0]["args"]
    assert a.target_link_ids[0] == 254
    a.target_link_ids[0] = 255
    assert _fused(hip_backend, n, run) == -5, "a tracked link id beyond 254"
    a.target_link_ids[0] = 254
    b = run["mgrs"][1]["args"]
    keep = b.with_link_ids[0]
    b.with_link_ids[0] = 255
    assert _fused(hip_backend, n, run) == -5, "a with-filter link id beyond 254"
    b.with_link_ids[0] = keep
    for m in run["mgrs"]:
        m["args"].num_scene_links = 256
    assert _fused(hip_backend, n, run) == -5, "more than 255 scene links"
    for m in run["mgrs"]:
        m["args"].num_scene_links = 255
    _check_untouched(run, case, "refused folds")
    assert _fused(hip_backend, n, run) == 0
    _check(run, want, "the same descriptors, accepted")


# ----------------------------------------------------------------------------------------------------
# the non-finite flag
# ----------------------------------------------------------------------------------------------------
def _flag_cases():
    """(a) non-finite components in slots that manager 0 includes and manager 1 does not; (b) the same values only where no manager
    includes them: an empty slot, a pair of untracked links, and a link of the filtered manager against a link its filter lacks."""
    a = cc.make_case(130, 40, 8, seed=9, num_links=60)
    b = cc.make_case(130, 40, 8, seed=9, num_links=60)
    f, la, lb = b["inp"]["force"], b["inp"]["link_a"], b["inp"]["link_b"]
    f[~np.isfinite(f)] = 1.0
    tracked = np.concatenate([m["targets"] for m in b["mgrs"]])
    free = [x for x in range(60) if x not in tracked and x not in b["mgrs"][1]["withs"]]
    for env, slot, comp, val, pair in ((0, 3, 0, np.nan, (-1, -1)), (64, 39, 1, np.inf, (free[0], free[1])), (129, 20, 2, -np.inf, (b["mgrs"][1]["targets"][0], free[0]))):
        f[env, slot, comp], la[env, slot], lb[env, slot] = val, pair[0], pair[1]
    wa, wb = cc.expected_exact(a), cc.expected_exact(b)
    assert [w["flag"] for w in wa] == [True, False] and [w["flag"] for w in wb] == [False, False]
    return (a, wa), (b, wb)


def _flags_standalone(backend, dev):
    """The reference warns when a non-finite force sits ANYWHERE in the scene's array (contact_manager.py:401); the kernels raise
    contact_flags only for slots that a manager includes — pinned here."""
    st = _stats_mod()
    for (case, want), expect in zip(_flag_cases(), ([1, 0], [0, 0])):
        blocks = [torch.zeros(st.STATS_BYTES, dtype=torch.uint8, device=dev) for _ in case["mgrs"]]
        run = _alloc(case, dev, stats=[b.data_ptr() for b in blocks])
        _launch(backend, run)   # (one launch for both managers on the GPU: the flag is per manager even then)
        _check(run, want, "flag case")
        assert [_flag(b) for b in blocks] == expect


def test_non_finite_flag_only_for_included_slots_oracle(oracle_backend):
    _flags_standalone(oracle_backend, "cpu")


@pytest.mark.gpu
def test_non_finite_flag_only_for_included_slots_hip(hip_backend):
    _flags_standalone(hip_backend, "cuda")


@pytest.mark.gpu
def test_non_finite_flag_of_a_folded_launch(hip_backend):
    """Folded, every manager counts into the step's one statistics block: raised iff some manager included such a slot."""
    host = _host(130)
    ptr = C.cast(host._trace.post_refs.termination, C.POINTER(nat.GfTerminationArgs)).contents.stats
    block = None
    for t in (host.stats.dev, getattr(host.stats, "ring", None)):   # the step's block: the env's own, or a slot of its ring
        if t is not None and 0 <= ptr - t.data_ptr() <= t.numel() - _stats_mod().STATS_BYTES:
            block = t.view(-1)[ptr - t.data_ptr():][:_stats_mod().STATS_BYTES]
    assert block is not None
    for (case, want), expect in zip(_flag_cases(), (1, 0)):
        block.zero_()
        run = _alloc(case, "cuda", stats=[ptr] * 2)   # (the fold accepts managers that count into the step's own block only)
        assert _fused(hip_backend, 130, run) == 0, "not folded"
        _check(run, want, "folded flag case")
        assert _flag(block) == expect


# ----------------------------------------------------------------------------------------------------
# accuracy leg
# ----------------------------------------------------------------------------------------------------
ACCURACY = [(257, 9, 13, None), (70, 300, 4, None), (130, 128, 32, 255)]   # one mask word; ten words and eight unit loops; the fused tile's limit of links
ACC_IDS = ["257x9x13", "70x300x4", "130x128x32-fused"]


@functools.lru_cache(maxsize=None)
def _accuracy_case(i):
    n, c, t, nl = ACCURACY[i]
    case = cc.make_float_case(n, c, t, seed=500 + i, num_links=nl, id_max=254 if nl else None)
    ref = []
    excluded = total = 0
    for m in case["mgrs"]:
        r = cc.restate(case["inp"], m["targets"], m["withs"], m["threshold"], m["air"], case["dt"])
        r["bounds"] = cc.accuracy_bounds(r, m["threshold"])
        excluded, total = excluded + int((~r["bounds"][2]).sum()), total + r["bounds"][2].size
        ref.append(r)
    assert excluded <= 0.01 * total, "too many norms within their bound of the threshold to compare air time"
    return case, ref


def _accuracy_check(run, case, ref, what, limit=1.0):
    """Every output of a float32 implementation within ``limit`` times the bounds of contact_cases.accuracy_bounds (module docstring
    there); returns the worst error over its bound."""
    N, worst = run["N"], 0.0
    for j, (m, r, cm) in enumerate(zip(run["mgrs"], ref, case["mgrs"])):
        fb, pb, decided = r["bounds"]
        o = {k: x.cpu().numpy() for k, x in m["out"].items()}
        tg = np.asarray(cm["targets"])
        assert np.array_equal(o["position_counts"][:N], r["counts"]), f"{what}: manager {j} counts"
        assert np.array_equal(o["link_vel"][:N], case["inp"]["links_vel"][:, tg]) and np.array_equal(o["link_pos"][:N], case["inp"]["links_pos"][:, tg])
        for k, want, bound in (("contacts", r["forces"], fb), ("contact_positions", r["positions"], pb)):
            err = np.abs(o[k][:N].astype(np.float64) - want)
            ratio = float((err / np.where(bound > 0, bound, 1.0))[bound > 0].max(initial=0.0))
            print(f"{what}: manager {j} {k}: worst error {err.max():.3e}, worst error / bound {ratio:.3f}")
            assert (err <= limit * bound).all(), f"{what}: manager {j} {k}: error / bound up to {ratio:.3f}"
            assert np.isnan(o[k][N:]).all()
            worst = max(worst, ratio)
        for k, x, wa in zip(AIR, m["air"], r["air"]):
            got = x.cpu().numpy()
            assert np.array_equal(got[:N][decided], wa.astype(np.float32)[decided]), f"{what}: manager {j} {k}"
            assert (got[N:] == AIR_POISON).all()
    print(f"{what}: worst error / bound {worst:.3f}")
    return worst


@pytest.mark.parametrize("i", range(len(ACCURACY)), ids=ACC_IDS)
def test_accuracy_bounds_hold_with_margin_on_the_cpu(oracle_backend, i):
    """The guard of the bounds: the restatement evaluated in float32 in the same slot order, and the oracle, stay below HALF of them."""
    case, ref = _accuracy_case(i)
    for m, r in zip(case["mgrs"], ref):
        r32 = cc.restate(case["inp"], m["targets"], m["withs"], m["threshold"], m["air"], case["dt"], dtype=np.float32)
        fb, pb, decided = r["bounds"]
        assert (np.abs(r32["forces"] - r["forces"]) <= 0.5 * fb).all() and (np.abs(r32["positions"] - r["positions"]) <= 0.5 * pb).all()
        assert np.array_equal(r32["is_contact"][decided], r["is_contact"][decided])
        assert (fb > 0).mean() > 0.1 and decided.mean() >= 0.99
    run = _alloc(case, "cpu")
    _launch(oracle_backend, run)
    _accuracy_check(run, case, ref, "oracle " + ACC_IDS[i], limit=0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(ACCURACY)), ids=ACC_IDS)
def test_accuracy_hip(hip_backend, i):
    """Forces: 5u of the magnitudes that enter rot_inv per matched slot plus (k - 1) u sum |term| for the float32 sum of k slots; mean
    position: (k - 1) u sum |p| plus u |mean|; air time wherever the float64 norm is further than its bound from the threshold (at least 99 % of the
    pairs, asserted from the reference alone) — derivation: contact_cases.accuracy_bounds.  Measured: profiles/contact_edges.md."""
    case, ref = _accuracy_case(i)
    run = _alloc(case, "cuda")
    if ACCURACY[i][3]:
        assert _fused(hip_backend, ACCURACY[i][0], run) == 0, "not folded"
    else:
        _launch(hip_backend, run)
    _accuracy_check(run, case, ref, "hip " + ACC_IDS[i])
