"""Every mask-valued decision at its boundary, against the reference (tests/golden/mask_edges.npz, recorded by
``tools/gen_golden.py mask_edges``; tests/mask_edges_cases.py holds the env, the config and the block layout).

A block of rows per probed decision — a force norm against 1.0 / 5.0 / 8.0 / 1.7 on axis-aligned forces one float32 step either side
of the threshold and on ≥ 2 000 oblique forces within a few steps of it, has_contact's count at min_contacts − 1 … + 1, the grace
periods at grace − 1 … + 1, the xy command norm against 0.06 and 0.1, bad_orientation swept about oblique axes, base height, the four
terrain bounds, the timeout, has_made_contact's two comparisons, feet_air_time's clamp — with everything else far from firing.

Three ways through the package must give the reference's bits: the per-term functions (every link set: 1, 4, 5, 9 and 17 links), one
TerminationManager.step() + RewardManager.step() of a config of the mask terms (five variants, see mask_edges_cases), and — GPU — the
fused post-physics launch of the same env, under the table interpreter and under a static program compiled for the config.
Masks, pure norms and the manager totals are compared exactly; float sums keep the 1e-5 rule of test_terms_golden.

CPU: oracle backend.  GPU (-m gpu): HIP kernels."""
import numpy as np
import pytest
import torch

import helpers
import mask_edges_cases as mc

_FIX = []
_ENVS = {}
VARIANT_IDS = list(range(len(mc.VARIANTS)))


def _fixture() -> mc.Fixture:
    if not _FIX:
        _FIX.append(mc.Fixture(helpers.load("mask_edges")))
    return _FIX[0]


def _env(dev: str, variant: int):
    """One built env per device and variant for the whole module (the state of every block is loaded into it in place)."""
    key = (dev, variant)
    if key not in _ENVS:
        env = mc.make_env(mc.package_api(), variant)
        env.build()
        _ENVS[key] = env
    return _ENVS[key]


def _to(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _flips(what: str, block: str, got: np.ndarray, want: np.ndarray) -> list:
    """[] when equal, else one line naming the term, the block and how many rows differ."""
    if got.shape == want.shape and np.array_equal(got, want):
        return []
    bad = int((got != want).reshape(got.shape[0], -1).any(axis=1).sum()) if got.shape == want.shape else -1
    return [f"{what} on block {block}: {bad} of {want.shape[0]} rows differ"]


def test_oblique_blocks_tell_the_norm_formulas_apart():
    """The sensitivity condition, from the fixture alone: in every oblique block at least 50 rows are ones where plain float32
    products summed left to right land on the other side of the mask the reference recorded — so the blocks fail a norm that is
    not torch's.  (A condition on the inputs: nothing of the package runs here.)"""
    fix = _fixture()
    oblique = [b for b in fix.blocks if b.endswith("_oblique")]
    assert len(oblique) == len(mc.THRESHOLDS) + len(mc.CMD_THRESHOLDS)
    for b in oblique:
        assert fix.n(b) >= 2000
        rows = mc.sensitive_rows(fix, b)
        print(f"{b}: {rows} of {fix.n(b)} rows tell the formulas apart")
        assert rows >= mc.MIN_SENSITIVE_ROWS, f"{b}: only {rows} sensitive rows"
    # the axis-aligned rows pin `>` and the float32 cast of the threshold: exactly the rows one step above fire
    for thr in mc.THRESHOLDS:
        b = f"c3_{thr}_axis"
        want = fix.call_expected(b)["term_contact_force_L5"][1]
        lengths = np.abs(fix.a["in_force"][fix.rows(b)][:, 0]).max(axis=1)
        assert np.array_equal(want, lengths > np.float32(thr)) and 0 < want.sum() < want.size


def _check_call_path(dev):
    fix, api = _fixture(), mc.package_api()
    env = _env(dev, 0)
    bad = []
    for block in fix.blocks:
        n = fix.n(block)
        mc.load_state(env, fix.state(block), _to(dev))
        got = mc.call_terms(api, env, fix.thr(block), fix.limit(block))
        want = fix.call_expected(block)
        assert set(got) == set(want)
        for term, (kind, val) in got.items():
            g, w = val.cpu().numpy()[:n], want[term][1]
            if kind == "mask":
                assert g.dtype == np.bool_ or np.all((g == 0) | (g == 1)), f"{term} is not 0 / 1"
                bad += _flips(term, block, g != 0, w)
            elif kind == "norm":
                bad += _flips(term, block, g, w)
            else:   # a float sum: the 1e-5 rule, scaled as in test_terms_golden
                tol = 1e-5 * max(1.0, float(np.abs(w).max()))
                if not np.allclose(g, w, atol=tol, rtol=0):
                    bad.append(f"{term} on block {block}: {int((np.abs(g - w) > tol).sum())} of {n} rows off by more than {tol:g}")
    assert not bad, "\n".join(bad)


def _manager_step(env):
    env._begin_step()
    try:
        term, trunc = env.termination_manager.step()
        rew = env.reward_manager.step()
        return term.cpu().numpy().copy(), trunc.cpu().numpy().copy(), rew.cpu().numpy().copy()
    finally:
        env._end_step()


def _reward_names(got: np.ndarray, want: np.ndarray) -> str:
    """Which terms of the config a wrong total points at: the weights are distinct powers of two times dt."""
    d = np.unique(np.round((got - want)[got != want] / np.float32(mc.DT)).astype(np.int64))[:4]
    return ", ".join(f"Δ={int(x)}·dt" for x in d) + f" (weights {mc.WEIGHTS})"


def _check_manager_path(dev, variant):
    fix = _fixture()
    env = _env(dev, variant)
    bad, seen = [], 0
    for block in fix.blocks:
        if variant not in fix.variants(block):
            continue
        seen += 1
        n = fix.n(block)
        mc.load_state(env, fix.state(block), _to(dev))
        term, trunc, rew = _manager_step(env)
        want = fix.manager_expected(block, variant)
        bad += _flips("terminated", block, term[:n], want["terminated"])
        bad += _flips("truncated", block, trunc[:n], want["truncated"])
        r = _flips("reward", block, rew[:n], want["reward"])
        bad += [r[0] + ": " + _reward_names(rew[:n], want["reward"])] if r else []
    assert seen > 10
    assert not bad, f"variant {variant} {mc.VARIANTS[variant]}:\n" + "\n".join(bad)


def _check_contact_step(dev, variant):
    """ContactManager.step()'s is_contact at the variant's threshold: the block's feet forces go in as one scene contact per foot
    (identity link quaternions: local == world), the four air-time arrays after one step from the known state must be the reference's."""
    fix = _fixture()
    env = _env(dev, variant)
    feet, sc = env.cms[mc.FEET], env.scene
    ids = feet.link_ids.to(torch.int32)
    bad, seen = [], 0
    for block in fix.blocks:
        want = fix.manager_expected(block, variant)
        if variant not in fix.variants(block) or "air" not in want:
            continue
        seen += 1
        n = fix.n(block)
        st = fix.state(block)
        mc.load_state(env, st, _to(dev))
        sc.contact_force[:] = 0.0
        sc.contact_force[:, :4] = _to(dev)(st[f"contacts{mc.FEET}"])
        sc.contact_pos[:] = 0.0
        sc.link_a[:] = -1
        sc.link_b[:] = -1
        sc.link_a[:, :4] = 0
        sc.link_b[:, :4] = ids
        sc.links_quat[:] = torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev)
        feet.step()
        bad += _flips("contacts", block, feet.contacts.cpu().numpy()[:n], st[f"contacts{mc.FEET}"][:n])
        got = np.stack([x.cpu().numpy() for x in (feet.last_air_time, feet.current_air_time, feet.last_contact_time, feet.current_contact_time)])
        for k, name in enumerate(("last_air_time", "current_air_time", "last_contact_time", "current_contact_time")):
            bad += _flips(name, block, got[k][:n], want["air"][k])
    assert seen == 4
    assert not bad, f"variant {variant} (air_time_contact_threshold {mc.VARIANTS[variant]['thr']}):\n" + "\n".join(bad)


def test_call_path_cpu_oracle(oracle_backend):
    _check_call_path("cpu")


@pytest.mark.parametrize("variant", VARIANT_IDS)
def test_manager_path_cpu_oracle(oracle_backend, variant):
    _check_manager_path("cpu", variant)


@pytest.mark.parametrize("variant", VARIANT_IDS)
def test_contact_step_cpu_oracle(oracle_backend, variant):
    _check_contact_step("cpu", variant)


@pytest.mark.gpu
def test_call_path_hip(hip_backend):
    _check_call_path("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANT_IDS)
def test_manager_path_hip(hip_backend, variant):
    _check_manager_path("cuda", variant)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANT_IDS)
def test_contact_step_hip(hip_backend, variant):
    _check_contact_step("cuda", variant)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANT_IDS)
@pytest.mark.parametrize("post_variant", [1, 2])
def test_fused_path_hip(hip_backend, post_variant, variant):
    """The same env's fused post-physics launch (termination → reward → … in one kernel) on every block of the variant: its reward
    and termination buffers must be the manager path's and the fixture's, bit for bit.  GF_OPT_POST_VARIANT 1: the table interpreter;
    2: a static program — none of the built-in ones matches this config, so the env compiles its own (jit_programs = "sync")."""
    from genesis_forge_amd import _native as nat

    fix = _fixture()
    dev = "cuda"
    env = mc.make_env(mc.package_api(), variant)
    if post_variant == 2:
        env.jit_programs = "sync"
    env.build()
    env.seed(3)
    env.reset()
    for _ in range(6):
        env.step(torch.zeros(env.num_envs, 12, device=dev))
    refs = env._trace.post_refs
    assert refs is not None, "the config's step is not recorded with a fused post-physics launch"
    tm, rm = env.termination_manager, env.reward_manager
    hip_backend.set_option(nat.GF_OPT_POST_VARIANT, post_variant)
    try:
        what = hip_backend.post_describe(refs)
        assert what.startswith("program 0 (interpreter)") == (post_variant == 1), f"{what} (compile: {env._program_info})"
        bad = []
        blocks = [b for b in fix.blocks if variant in fix.variants(b)]
        fused = {}
        # every fused launch first: a manager's own step() hands its descriptor the statistics block of a phase-by-phase step, and
        # the recorded descriptors then no longer agree on one (the launch would be refused, not wrong)
        for block in blocks:
            mc.load_state(env, fix.state(block), _to(dev))
            rc = hip_backend.post_step_contacts(refs, [])
            assert rc == 0, nat.GF_ERRORS.get(rc, rc)
            torch.cuda.synchronize()
            fused[block] = (tm._terminated_buf.cpu().numpy().copy(), tm._truncated_buf.cpu().numpy().copy(), rm._reward_buf.cpu().numpy().copy())
        for block in blocks:
            n = fix.n(block)
            mc.load_state(env, fix.state(block), _to(dev))   # (the launch reset the envs that were done)
            phased = _manager_step(env)
            want = fix.manager_expected(block, variant)
            for name, f, p in zip(("terminated", "truncated", "reward"), fused[block], phased):
                bad += _flips(f"fused {name} against the fixture", block, f[:n], want[name])
                bad += _flips(f"fused {name} against the manager path", block, f[:n], p[:n])
        assert not bad, f"variant {variant} {mc.VARIANTS[variant]}, {what.split(':')[0]}:\n" + "\n".join(bad)
    finally:
        hip_backend.set_option(nat.GF_OPT_POST_VARIANT, 2)
