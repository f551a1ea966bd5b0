"""The action phase folded into the scene-tick launch of a recorded step (gf_run_ops: an action op directly in front of a scene op
runs as one launch) against the two launches it replaces (GF_FOLD_ACTION=0), bit for bit.

* Raw C ABI: ``gf_run_ops([ACTION, SCENE])`` on cloned state for three ticks — partial last tiles, D = 12 and 28, both action
  modes, per-link / contact outputs, the 16-env tiles below 32 768 envs and the 64-env tiles at 65 536, the optional bookkeeping
  buffers present and absent, non-finite raw actions, ``actions_in`` aliasing ``env_actions``.  Everything either op writes is
  compared through an int32 view, and so is the statistics ring (the shard an action flag lands in may differ, the OR over the
  shards and the folded rows may not).
* Fall-backs: pairs the fold does not cover give the same results with the switch in either position (and, where the entry points
  are called one by one, the same as those).  The launch count itself is not visible through the ABI; a kernel trace shows it.
* Errors: an invalid op is reported with its own index and return code and nothing is enqueued.
* Environment level: recorded steps of the benchmark config and of the gait config, fold on against fold off, with resets."""
import ctypes as C
import os

import pytest

from genesis_forge_amd import _native as nat

pytestmark = pytest.mark.gpu

STATS_WORDS = C.sizeof(nat.GfStepStats) // 4
FLAGS_WORD = nat.GfStepStats.action_flags.offset // 4
VECTOR_LEN = nat.GF_MAX_TERM_TERMS + 5 + nat.GF_MAX_TERMS + nat.GF_MAX_GAITS
SLOTS = 3
L, CN = 14, 6


def _lib():
    lib = C.CDLL(nat.lib_path())
    lib.gf_run_ops.restype = C.c_int
    lib.gf_run_ops.argtypes = [C.POINTER(nat.GfOp), C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    lib.gf_action_step.restype = C.c_int
    lib.gf_action_step.argtypes = [C.POINTER(nat.GfActionArgs), C.c_void_p]
    lib.gf_synth_scene_step.restype = C.c_int
    lib.gf_synth_scene_step.argtypes = [C.POINTER(nat.GfSynthSceneArgs), C.c_void_p]
    return lib


def _state(torch, n, d, links=False, contacts=False, misalign=0, keep=True, episode=True, bad=False, alias=False, steps=3):
    g = torch.Generator().manual_seed(1000 * n + 10 * d + links + 2 * contacts)
    q = torch.randn(n, 4, generator=g)
    q = q / q.norm(dim=1, keepdim=True)

    def rows(k):   # misalign = 1: the joint rows start 4 B past a 16-byte boundary
        return torch.randn(n * k + misalign, generator=g)
    raw = torch.randn(steps, n, d, generator=g) * 2.0
    if bad:   # a handful of non-finite and huge raw actions per tick, spread over the tiles
        flat = raw.view(steps, -1)
        for t in range(steps):
            idx = torch.randperm(n * d, generator=g)[:4]
            for j, v in zip(idx.tolist(), (float("nan"), float("inf"), float("-inf"), 1e9)):
                if t != 1 or v == 1e9 or v != v:   # tick 1 carries no Inf: the two flag bits must differ between the folded rows
                    flat[t, j] = v
    lo = -torch.rand(d, generator=g) - 0.2
    st = {"pos": torch.randn(n, 3, generator=g) + torch.tensor([0.0, 0.0, 0.3]), "quat": q,
          "lin_vel": torch.randn(n, 3, generator=g), "ang_vel": torch.randn(n, 3, generator=g),
          "targets": rows(d), "dof_pos": rows(d), "dof_vel": torch.zeros(n * d + misalign),
          "raw": raw, "scale": torch.rand(d, generator=g) + 0.1, "offset": torch.randn(d, generator=g) * 0.3,
          "clip_lo": lo, "clip_hi": lo + torch.rand(d, generator=g) * 2.0 + 0.1,
          "stats": torch.randint(0, 50, (SLOTS, nat.GF_STATS_SHARDS, STATS_WORDS), generator=g, dtype=torch.int32),
          "rows": torch.zeros(steps, VECTOR_LEN, dtype=torch.float64), "last_reset": torch.zeros(VECTOR_LEN, dtype=torch.float64)}
    st["stats"][0, :, FLAGS_WORD] = 0   # tick 0 ORs into slot 0 without anybody having zeroed it
    if keep:
        st["env_actions"] = torch.randn(n, d, generator=g)
        st["env_last_actions"] = torch.randn(n, d, generator=g)
    if alias:   # the policy wrote straight into the env's action buffer
        st["raw"][0] = st["env_actions"]
    if episode:
        st["episode_length"] = torch.randint(0, 500, (n,), generator=g, dtype=torch.int32)
    if links:
        st["links_quat_out"] = torch.zeros(n, L, 4)
        st["links_vel_out"] = torch.zeros(n, L, 3)
        st["links_pos_out"] = torch.zeros(n, L, 3)
    if contacts:
        st["contact_force_out"] = torch.zeros(n, CN, 3)
        st["contact_pos_out"] = torch.zeros(n, CN, 3)
        st["link_a_out"] = torch.zeros(n, CN, dtype=torch.int32)
        st["link_b_out"] = torch.zeros(n, CN, dtype=torch.int32)
    return {k: v.to("cuda") for k, v in st.items()}


def _args(st, n, d, mode, misalign=0, contacts=False, alias=False, split_targets=None):
    a = nat.GfActionArgs()
    a.num_envs, a.num_dofs, a.mode, a.check_finite = n, d, mode, 1
    for k in ("scale", "offset", "clip_lo", "clip_hi", "env_actions", "env_last_actions", "episode_length"):
        if k in st:
            setattr(a, k, st[k].data_ptr())
    a.targets = st["targets"].data_ptr() + 4 * misalign
    s = nat.GfSynthSceneArgs()
    s.num_envs, s.num_dofs = n, d
    s.num_contacts = CN if contacts else 0
    s.num_scene_links = L
    s.dt, s.joint_rate, s.ang_noise, s.lin_noise, s.height_target = 0.02, 8.0, 0.3, 0.05, 0.3
    s.contact_prob, s.contact_force, s.foot_contact_prob = 0.3, 40.0, 0.5
    s.seed, s.env_offset = 0x1234_5678_9ABC, 777
    s.foot_link_mask = (1 << 5) | (1 << 9) if contacts else 0
    for k in ("pos", "quat", "lin_vel", "ang_vel", "targets", "dof_pos", "dof_vel", "links_quat_out", "links_vel_out", "links_pos_out",
              "contact_force_out", "contact_pos_out", "link_a_out", "link_b_out"):
        if k in st:
            setattr(s, k, st[k].data_ptr() + (4 * misalign if k in ("targets", "dof_pos", "dof_vel") else 0))
    if split_targets is not None:   # the scene reads other targets than the action phase writes
        s.targets = split_targets.data_ptr()
    return a, s


def _per_tick(st, a, s, t, alias=False):
    a.actions_in = st["env_actions"].data_ptr() if (alias and t == 0) else st["raw"][t].data_ptr()
    slot = lambda k: st["stats"][k % SLOTS].data_ptr()
    a.stats, a.stats_zero, a.stats_fold_src = slot(t), slot(t + 1), slot(t + SLOTS - 1)
    a.stats_fold_dst = st["rows"][t].data_ptr()
    a.stats_last_reset = st["last_reset"].data_ptr()
    s.tick = (5 << 32) + t


def _run(torch, lib, st, a, s, fold, steps=3, alias=False, legacy=False, entry_points=False):
    ops = (nat.GfOp * 2)()
    ops[0].phase, ops[0].args = nat.GF_PHASE_ACTION, C.addressof(a)
    ops[1].phase, ops[1].args = nat.GF_PHASE_SCENE, C.addressof(s)
    if fold:
        os.environ.pop("GF_FOLD_ACTION", None)
    else:
        os.environ["GF_FOLD_ACTION"] = "0"
    if legacy:
        os.environ["GF_SCENE_LEGACY"] = "1"
    try:
        for t in range(steps):
            _per_tick(st, a, s, t, alias)
            if entry_points:
                assert lib.gf_action_step(C.byref(a), None) == 0
                assert lib.gf_synth_scene_step(C.byref(s), None) == 0
            else:
                failed = C.c_int(-1)
                assert lib.gf_run_ops(ops, 2, None, C.byref(failed)) == 0, failed.value
        torch.cuda.synchronize()
    finally:
        os.environ.pop("GF_FOLD_ACTION", None)
        os.environ.pop("GF_SCENE_LEGACY", None)


def _assert_same(torch, new, old, what):
    for k in new:
        x, y = new[k].cpu(), old[k].cpu()
        if k == "stats":   # the flags may sit in other shards: their OR per slot, and every other word as it is
            fx, fy = x[:, :, FLAGS_WORD], y[:, :, FLAGS_WORD]
            for bit in (1, 2):
                assert torch.equal((fx & bit).amax(dim=1), (fy & bit).amax(dim=1)), f"action flag bit {bit}: {what}"
            x, y = x.clone(), y.clone()
            x[:, :, FLAGS_WORD] = 0
            y[:, :, FLAGS_WORD] = 0
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{k}: {what}"


def _compare(torch, n, d, mode, steps=3, **kw):
    lib = _lib()
    run_kw = {k: kw.pop(k) for k in ("legacy", "entry_points") if k in kw}
    arg_kw = {k: kw[k] for k in ("misalign", "contacts", "alias") if k in kw}
    new = _state(torch, n, d, steps=steps, **kw)
    old = {k: v.clone() for k, v in new.items()}
    alias = kw.get("alias", False)
    a, s = _args(new, n, d, mode, **arg_kw)
    _run(torch, lib, new, a, s, True, steps, alias, legacy=run_kw.get("legacy", False))
    a, s = _args(old, n, d, mode, **arg_kw)
    _run(torch, lib, old, a, s, False, steps, alias, **run_kw)
    _assert_same(torch, new, old, "the folded launch differs from the two launches")
    return new


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("no GPU")
    return torch


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4103, 65536])
@pytest.mark.parametrize("d", [12, 28])
@pytest.mark.parametrize("mode", [nat.GF_ACTION_POSITION, nat.GF_ACTION_WITHIN_LIMITS])
@pytest.mark.parametrize("links,contacts", [(False, False), (True, False), (False, True), (True, True)])
def test_fold_matches_two_launches(n, d, mode, links, contacts):
    torch = _torch()
    st = _compare(torch, n, d, mode, links=links, contacts=contacts)
    assert int(st["stats"][1].abs().sum()) == 0, "the next step's slot was not zeroed"


@pytest.mark.parametrize("n", [65, 4103, 65536])
@pytest.mark.parametrize("d", [12, 28])
@pytest.mark.parametrize("keep,episode", [(True, False), (False, True), (False, False)])
@pytest.mark.parametrize("tile", [False, True])
def test_fold_optional_buffers(n, d, keep, episode, tile):
    _compare(_torch(), n, d, nat.GF_ACTION_POSITION, keep=keep, episode=episode, links=tile, contacts=tile)


@pytest.mark.parametrize("n", [65, 4103, 65536])
@pytest.mark.parametrize("d", [12, 28])
@pytest.mark.parametrize("mode", [nat.GF_ACTION_POSITION, nat.GF_ACTION_WITHIN_LIMITS])
def test_fold_nonfinite_actions(n, d, mode):
    torch = _torch()
    st = _compare(torch, n, d, mode, bad=True, contacts=(n == 4103))
    rows = st["rows"].cpu()
    nan_col, inf_col = nat.GF_MAX_TERM_TERMS + 1, nat.GF_MAX_TERM_TERMS + 2
    if mode == nat.GF_ACTION_POSITION:   # row t is the fold of tick t - 1: tick 0 had NaN and Inf, tick 1 NaN only
        assert rows[1, nan_col] == 1.0 and rows[1, inf_col] == 1.0
        assert rows[2, nan_col] == 1.0 and rows[2, inf_col] == 0.0
    else:   # within-limits managers do not scan (position_within_limits.py)
        assert rows[1:, nan_col].sum() == 0.0 and rows[1:, inf_col].sum() == 0.0
    assert not torch.isfinite(st["targets"]).all()   # NaN goes through both clamps


@pytest.mark.parametrize("n", [65, 4103, 65536])
@pytest.mark.parametrize("d", [12, 28])
def test_fold_actions_alias_env_actions(n, d):
    _compare(_torch(), n, d, nat.GF_ACTION_POSITION, alias=True, links=(n == 4103))


@pytest.mark.parametrize("n", [65, 4103])
@pytest.mark.parametrize("what", ["d5", "misaligned_rows", "legacy"])
def test_fall_back_two_launches(n, what):
    torch = _torch()
    if what == "d5":
        _compare(torch, n, 5, nat.GF_ACTION_POSITION, contacts=True, entry_points=True)
    elif what == "misaligned_rows":
        _compare(torch, n, 12, nat.GF_ACTION_POSITION, misalign=1, entry_points=True)
    else:
        _compare(torch, n, 12, nat.GF_ACTION_POSITION, links=True, legacy=True)


@pytest.mark.parametrize("n", [65, 4103])
def test_fall_back_other_targets(n):
    """scene.targets != action.targets: the scene must read ITS targets (which nobody writes here), not the action phase's."""
    torch = _torch()
    lib = _lib()
    new = _state(torch, n, 12)
    new["scene_targets"] = torch.randn(n, 12, generator=torch.Generator().manual_seed(n)).to("cuda")
    old = {k: v.clone() for k, v in new.items()}
    for st, fold in ((new, True), (old, False)):
        a, s = _args(st, n, 12, nat.GF_ACTION_POSITION, split_targets=st["scene_targets"])
        _run(torch, lib, st, a, s, fold, entry_points=not fold)
    _assert_same(torch, new, old, "differs from the entry points called one by one")


@pytest.mark.parametrize("n", [65, 65536])
@pytest.mark.parametrize("which", ["null_actions", "misaligned_quat"])
def test_invalid_op_reports_its_index_and_enqueues_nothing(n, which):
    torch = _torch()
    lib = _lib()
    st = _state(torch, n, 12)
    before = {k: v.clone() for k, v in st.items()}
    a, s = _args(st, n, 12, nat.GF_ACTION_POSITION)
    _per_tick(st, a, s, 0)
    if which == "null_actions":
        a.actions_in = None
        want_rc, want_index = -1, 0   # GF_E_NULL from the action op
    else:
        s.quat = st["quat"].data_ptr() + 4
        want_rc, want_index = -5, 1   # GF_E_UNSUPPORTED from the scene op
    ops = (nat.GfOp * 2)()
    ops[0].phase, ops[0].args = nat.GF_PHASE_ACTION, C.addressof(a)
    ops[1].phase, ops[1].args = nat.GF_PHASE_SCENE, C.addressof(s)
    failed = C.c_int(-1)
    os.environ.pop("GF_FOLD_ACTION", None)
    assert lib.gf_run_ops(ops, 2, None, C.byref(failed)) == want_rc
    assert failed.value == want_index
    torch.cuda.synchronize()
    for k in st:
        assert torch.equal(st[k].view(torch.int32), before[k].view(torch.int32)), f"{k}: a failed gf_run_ops call modified a buffer"


def _make_env(kind, n):
    from genesis_forge_amd import tasks

    if kind == "bench":
        env = tasks.bench_env(n, max_episode_length_s=0.4)
    else:
        env = tasks.Go2GaitTrainingEnv(num_envs=n, max_episode_length_s=0.4, scene_kwargs=dict(ang_noise=0.3, seed=3, contact_prob=0.05))
    env.build()
    return env


@pytest.mark.parametrize("kind,n", [("bench", 1000), ("bench", 65536), ("gait", 4096)])
def test_recorded_env_fold_on_equals_fold_off(hip_backend, kind, n):
    import torch

    envs = {"on": _make_env(kind, n), "off": _make_env(kind, n)}
    try:
        for env in envs.values():
            env.seed(7)
            env.reset()
        g = torch.Generator().manual_seed(1)
        d = envs["on"].action_space.shape[0]
        dones = 0
        for k in range(60):
            act = torch.randn(n, d, generator=g).to("cuda")
            out = {}
            for name, env in envs.items():
                if name == "on":
                    os.environ.pop("GF_FOLD_ACTION", None)
                else:
                    os.environ["GF_FOLD_ACTION"] = "0"
                out[name] = env.step(act.clone())
            (o1, r1, t1, u1, e1), (o2, r2, t2, u2, e2) = out["on"], out["off"]
            assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)), f"observations differ at step {k}"
            assert torch.equal(r1.view(torch.int32), r2.view(torch.int32)), f"reward differs at step {k}"
            assert torch.equal(t1, t2) and torch.equal(u1, u2), f"masks differ at step {k}"
            assert set(e1["episode"]) == set(e2["episode"])
            for key in e1["episode"]:
                x, y = torch.as_tensor(e1["episode"][key]).double().cpu(), torch.as_tensor(e2["episode"][key]).double().cpu()
                assert torch.equal(x.view(torch.int64), y.view(torch.int64)), f"episode log {key} differs at step {k}"
            a1, a2 = envs["on"], envs["off"]
            for what, x, y in (("actions", a1.actions, a2.actions), ("last_actions", a1.last_actions, a2.last_actions),
                               ("episode_length", a1.episode_length, a2.episode_length),
                               ("targets", a1.action_manager.get_actions(), a2.action_manager.get_actions()),
                               ("raw_actions", a1.action_manager.raw_actions, a2.action_manager.raw_actions)):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{what} differs at step {k}"
            dones += int((t1 | u1).sum())
        assert dones > 0, "no env reset in 60 steps"
        assert envs["on"]._trace is not None and envs["off"]._trace is not None, "the step was not recorded"
    finally:
        os.environ.pop("GF_FOLD_ACTION", None)
