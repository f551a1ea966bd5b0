"""A recorded step on the stand-in scene as ONE launch (gf_run_ops: action op, scene op, fused post-physics op in a row — the
tick of the workgroup's tile runs as the post-physics kernel's prologue) against the two launches it replaces (GF_FOLD_STEP=0),
bit for bit.  The switch is read per call, so one process runs both sides; ``gf_step_fold_count`` says whether a call folded.

* Environment level: ``tasks.bench_env(n, dofs=d)`` and the simple Go2 config, fold on against fold off over 40 recorded steps:
  everything ``step()`` returns, the env's state buffers and the statistics as the log shows them, through int32 / int64 views.
  n covers a lane-starved tile, a full tile, a partial last tile and a tile index beyond the upkeep workgroups; d = 12 with the
  static program, 12 and 28 with the table interpreter; logging on and off; observation output ``fresh`` and ``static``; one
  case with non-finite raw actions.  The step's statistics slot is read on both sides too: the OR of the action-flag word over the
  shards is equal, and with non-finite actions it is NaN | Inf (the shard a flag lands in may differ, the other counters are summed
  over the shards).  A recorded single-process step always carries the statistics ring, so the upkeep workgroups are present in
  every one of these cases whatever the logging switch says.
* Without upkeep workgroups: the recorded ops of an env, the ring fields of the action descriptor cleared, through ``gf_run_ops``
  with the switch on and off — the folded launch whose grid is the tile count.
  Every case asserts that inside the compared window at least one env was reset and at least one was not.  The episodes are
  0.4 s (20 steps ± 10 %), so in 40 steps every env times out and most steps of an env reset nothing (checked with the oracle
  backend on the CPU for every case of the table before the first GPU run).
* Against the oracle: the folded step at n = 130, d = 12 for 30 steps, compared the way ``smoke()`` compares.
* Fall-backs give the same results with the switch in either position and do not fold: ``[ACTION, SCENE]`` alone, a step with
  contact ops between the scene and the post-physics op, a scene with contact slots directly in front of a valid post-physics op
  (the BASELINE ``simple`` config: the peephole launches the pair's tile kernel itself), a profiled POST phase.
* Errors: an invalid post-physics op behind a valid pair gives the same return code, failed index and buffers either way."""
import ctypes as C
import os

import pytest

from genesis_forge_amd import _native as nat

import test_action_fold as taf

pytestmark = pytest.mark.gpu

STEPS = 40
N_BEYOND_UPKEEP = 64 * (24 + 1) + 37   # kActionUpkeepBlocks = 24: tile 25 sits behind more tiles than there are upkeep workgroups


def _count():
    lib = C.CDLL(nat.lib_path())
    lib.gf_step_fold_count.restype = C.c_long
    return int(lib.gf_step_fold_count())


def _switch(on):
    if on:
        os.environ.pop("GF_FOLD_STEP", None)
    else:
        os.environ["GF_FOLD_STEP"] = "0"


def _make(kind, n, d=12, logging=True, output="fresh"):
    from genesis_forge_amd import tasks

    if kind == "simple_slots":   # BASELINE config 1 as it is: contact slots in the scene, no ContactManager
        env = tasks.Go2SimpleEnv(num_envs=n, max_episode_length_s=0.4, scene_kwargs=dict(tasks._SC))
    elif kind == "simple":
        # (the BASELINE config's scene has contact slots, which keep the tile kernel's launch: here without them)
        env = tasks.Go2SimpleEnv(num_envs=n, max_episode_length_s=0.4, scene_kwargs=dict(tasks._SC, max_collision_pairs=0))
    elif kind == "contacts":
        env = tasks.Go2CommandDirectionEnv(num_envs=n, max_episode_length_s=0.4, contacts=True, scene_kwargs=dict(ang_noise=0.3, seed=3))
    else:
        env = tasks.bench_env(n, max_episode_length_s=0.4, dofs=d)
    env.build()
    if not logging:
        env.managers["reward"].logging_enabled = False
        env.managers["termination"].logging_enabled = False
    if output != "fresh":
        for om in env.managers["observation"]:
            om.output = output
    return env


def _state_of(env):
    r, am = env.robot, env.action_manager
    st = {"pos": r.pos, "quat": r.quat, "lin_vel": r.lin_vel, "ang_vel": r.ang_vel, "dof_pos": r.dof_pos, "dof_vel": r.dof_vel,
          "targets": am.get_actions(), "raw_actions": am.raw_actions, "actions": env.actions, "last_actions": env.last_actions,
          "episode_length": env.episode_length}
    rm = env.managers["reward"]
    st["episode_sums"], st["episode_seconds"] = rm._episode_sums, rm._episode_seconds
    for c, cmd in enumerate(env.managers["command"]):
        st[f"command{c}"] = cmd._command
    return st


INT_WORDS = 24   # GfStepStats starts with its int32 counters: term_fired[16], reset_count, action_flags, contact_flags, resample_count, gait_count[4]


def _slot_counters(torch, env, slot=None):
    """(OR of the action flags over the shards, the other int32 counters summed over the shards) of a statistics ring slot — by
    default the one the last recorded step counted into, which no later step has folded or zeroed yet."""
    slot = env.stats._ring_prev if slot is None else slot
    words = env.stats.ring[slot].view(torch.int32).view(nat.GF_STATS_SHARDS, taf.STATS_WORDS)[:, :INT_WORDS].cpu()
    flags = 0
    for v in words[:, taf.FLAGS_WORD].tolist():
        flags |= v
    words[:, taf.FLAGS_WORD] = 0
    return flags, words.sum(dim=0)


def _same_bits(torch, x, y, what):
    x, y = torch.as_tensor(x), torch.as_tensor(y)
    if x.dtype == torch.bool or x.dtype == torch.uint8:
        assert torch.equal(x, y), what
    elif x.dtype in (torch.float64, torch.int64):
        assert torch.equal(x.view(torch.int64), y.view(torch.int64)), what
    else:
        assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)), what


def _compare_envs(torch, kind, n, d=12, logging=True, output="fresh", bad=False, expect_fold=True, steps=STEPS, program=None):
    """Two envs of the same seed, the same actions: one steps with the fold, one with GF_FOLD_STEP=0."""
    envs = {"on": _make(kind, n, d, logging, output), "off": _make(kind, n, d, logging, output)}
    try:
        for env in envs.values():
            env.seed(7)
            env.reset()
        g = torch.Generator().manual_seed(1000 * n + d)
        width = envs["on"].action_space.shape[0]
        done_steps = torch.zeros(0, n, dtype=torch.bool)
        compared = 0
        for k in range(steps + 6):
            act = torch.randn(n, width, generator=g)
            if bad:   # a few non-finite raw actions per step: the action flags of the step are non-zero
                flat = act.view(-1)
                for j, v in zip(torch.randperm(n * width, generator=g)[:3].tolist(), (float("nan"), float("inf"), float("-inf"))):
                    flat[j] = v
            act = act.to("cuda")
            recorded = all(e._trace is not None for e in envs.values())
            out = {}
            for name, env in envs.items():
                _switch(name == "on")
                c0 = _count()
                out[name] = env.step(act.clone())
                folded = _count() - c0
                if recorded:
                    assert folded == (1 if (name == "on" and expect_fold) else 0), f"step {k}, switch {name}: {folded} folded launches"
            (o1, r1, t1, u1, e1), (o2, r2, t2, u2, e2) = out["on"], out["off"]
            _same_bits(torch, o1, o2, f"observations differ at step {k}")
            _same_bits(torch, r1, r2, f"reward differs at step {k}")
            assert torch.equal(t1, t2) and torch.equal(u1, u2), f"masks differ at step {k}"
            assert set(e1["episode"]) == set(e2["episode"])
            for key in e1["episode"]:
                _same_bits(torch, torch.as_tensor(e1["episode"][key]).double().cpu(), torch.as_tensor(e2["episode"][key]).double().cpu(),
                           f"episode log {key} differs at step {k}")
            s1, s2 = _state_of(envs["on"]), _state_of(envs["off"])
            for key in s1:
                _same_bits(torch, s1[key], s2[key], f"{key} differs at step {k}")
            if recorded:
                (f1, c1), (f2, c2) = _slot_counters(torch, envs["on"]), _slot_counters(torch, envs["off"])
                assert f1 == f2, f"action flags differ at step {k}: {f1} folded, {f2} in two launches"
                assert torch.equal(c1, c2), f"statistics counters differ at step {k}"
                assert f1 == (3 if bad else 0), f"action flags {f1} at step {k}"
                done_steps = torch.cat([done_steps, (t1 | u1).cpu().view(1, n)])
                compared += 1
                if compared == steps:
                    break
        assert compared == steps, "the step was not recorded in time"
        if program is not None:   # which kernel the fused launch selects: "program <id> (<name>): <signature>"
            what = nat.get_backend().post_describe(envs["on"]._trace.post_refs)
            assert what.startswith(f"program {program} "), what
        assert bool(done_steps.any()), "no env was reset inside the compared window"
        assert bool((~done_steps).any()), "no env went on without a reset inside the compared window"
    finally:
        _switch(True)


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("no GPU")
    return torch


VARIANTS = [(12, "static"), (12, "interp"), (28, "interp")]


def _with_variant(hip_backend, variant, fn):
    if variant == "interp":
        hip_backend.set_option(nat.GF_OPT_POST_VARIANT, 1)
    try:
        fn()
    finally:
        hip_backend.set_option(nat.GF_OPT_POST_VARIANT, 2)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, N_BEYOND_UPKEEP])
@pytest.mark.parametrize("d,variant", VARIANTS)
def test_folded_step_equals_two_launches(hip_backend, n, d, variant):
    torch = _torch()
    program = 1 if variant == "static" else 0
    _with_variant(hip_backend, variant, lambda: _compare_envs(torch, "bench", n, d, program=program))


@pytest.mark.parametrize("n", [65, N_BEYOND_UPKEEP])
@pytest.mark.parametrize("d,variant", VARIANTS)
@pytest.mark.parametrize("logging,output", [(False, "fresh"), (True, "static"), (False, "static")])
def test_folded_step_logging_and_output(hip_backend, n, d, variant, logging, output):
    torch = _torch()
    _with_variant(hip_backend, variant, lambda: _compare_envs(torch, "bench", n, d, logging=logging, output=output))


@pytest.mark.parametrize("n", [130, N_BEYOND_UPKEEP])
def test_folded_step_second_static_program(hip_backend, n):
    _compare_envs(_torch(), "simple", n, program=2)


@pytest.mark.parametrize("d,variant", VARIANTS)
def test_folded_step_nonfinite_actions(hip_backend, d, variant):
    torch = _torch()
    _with_variant(hip_backend, variant, lambda: _compare_envs(torch, "bench", 130, d, bad=True))


@pytest.mark.parametrize("n", [65, N_BEYOND_UPKEEP])
@pytest.mark.parametrize("d,variant", VARIANTS)
def test_folded_step_without_upkeep_workgroups(hip_backend, n, d, variant):
    """The recorded ops of two envs in the same state through gf_run_ops, the statistics ring's fields of the action descriptor
    cleared (nothing to zero, nothing to fold: no upkeep workgroup, grid = tiles), fold on against fold off: the same buffers, the
    same counters in the slot both count into (envs time out and are reset inside the raw ticks), non-zero action flags."""
    torch = _torch()
    lib = taf._lib()

    def run():
        envs = {"on": _make("bench", n, d), "off": _make("bench", n, d)}
        g = torch.Generator().manual_seed(n + d)
        keep = []
        for env in envs.values():
            env.seed(7)
            env.reset()
        for k in range(17):   # recorded, and up to the step before the first time-outs (episodes of 18 … 22 steps)
            act = torch.randn(n, d, generator=g).to("cuda")
            keep.append([env.step(act.clone()) for env in envs.values()])   # (the descriptors point into what the last step returned)
        assert all(e._trace is not None and e._trace.n_ops == 3 for e in envs.values())
        for t in range(6):   # … so that envs are reset inside these ticks
            act = torch.randn(n, d, generator=g)
            flat = act.view(-1)
            for j, v in zip(torch.randperm(n * d, generator=g)[:2].tolist(), (float("nan"), float("-inf"))):
                flat[j] = v
            act = act.to("cuda")
            for name, env in envs.items():
                tr = env._trace
                a = tr.action_args
                a.actions_in = act.data_ptr()
                a.stats_zero = a.stats_fold_src = a.stats_fold_dst = a.stats_last_reset = None
                _switch(name == "on")
                c0 = _count()
                failed = C.c_int(-1)
                assert lib.gf_run_ops(tr.ops, tr.n_ops, None, C.byref(failed)) == 0, failed.value
                assert _count() - c0 == (1 if name == "on" else 0), f"tick {t}, switch {name}"
            torch.cuda.synchronize()
            s1, s2 = _state_of(envs["on"]), _state_of(envs["off"])
            for key in s1:
                _same_bits(torch, s1[key], s2[key], f"{key} differs at raw tick {t}")
            for x, y in zip(keep[-1][0][:4], keep[-1][1][:4]):   # observations, reward, masks: written in place of the last step's
                _same_bits(torch, x, y, f"a step output differs at raw tick {t}")
            (f1, c1), (f2, c2) = _slot_counters(torch, envs["on"]), _slot_counters(torch, envs["off"])
            assert f1 == f2 == 3, f"action flags {f1} / {f2} at raw tick {t}"
            assert torch.equal(c1, c2), f"statistics counters differ at raw tick {t}"
        assert int(c1[nat.GF_MAX_TERM_TERMS]) > 0, "no env was reset inside the raw ticks"

    try:
        _with_variant(hip_backend, variant, run)
    finally:
        _switch(True)


def test_folded_step_against_oracle(hip_backend, oracle_lib_path):
    torch = _torch()
    from genesis_forge_amd import gs, tasks
    from oracle_backend import OracleBackend

    n, steps = 130, 30

    def run(dev):
        env = tasks.bench_env(n, max_episode_length_s=0.4)
        env.build()
        env.seed(123)
        env.reset()
        g = torch.Generator().manual_seed(0)
        outs = []
        for _ in range(steps):
            o, r, t, u, ex = env.step(torch.randn(n, 12, generator=g).to(dev))
            outs.append((o.cpu().clone(), r.cpu().clone(), t.cpu().clone(), u.cpu().clone(), dict(ex["episode"])))
        return outs

    _switch(True)
    c0 = _count()
    hip = run("cuda")
    torch.cuda.synchronize()
    assert _count() - c0 >= steps - 6, "the steps did not fold"
    try:
        gs.set_device("cpu")
        nat.set_backend(OracleBackend(oracle_lib_path))
        ref = run("cpu")
    finally:
        nat.set_backend(None)
        gs.set_device("cuda:0")
    dones = 0
    for t, (a, b) in enumerate(zip(hip, ref)):
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]), f"done masks differ at step {t}"
        assert torch.allclose(a[0], b[0], atol=1e-5, rtol=0), f"obs differ at step {t}: {(a[0] - b[0]).abs().max()}"
        assert torch.allclose(a[1], b[1], atol=1e-5, rtol=0), f"reward differs at step {t}: {(a[1] - b[1]).abs().max()}"
        assert set(a[4]) == set(b[4]), f"log keys differ at step {t}"
        dones += int(a[2].sum()) + int(a[3].sum())
    assert dones > 0, "the trajectory never reset an env"


# ---- fall-backs ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [65, N_BEYOND_UPKEEP])
def test_fall_back_pair_alone(n):
    """[ACTION, SCENE] with nothing behind it: the pair's own launch, whatever GF_FOLD_STEP says."""
    torch = _torch()
    lib = taf._lib()
    new = taf._state(torch, n, 12)
    old = {k: v.clone() for k, v in new.items()}
    c0 = _count()
    try:
        for st, on in ((new, True), (old, False)):
            _switch(on)
            a, s = taf._args(st, n, 12, nat.GF_ACTION_POSITION)
            taf._run(torch, lib, st, a, s, True)
    finally:
        _switch(True)
    assert _count() == c0
    taf._assert_same(torch, new, old, "GF_FOLD_STEP changed a step without a post-physics op")


def test_fall_back_contact_ops_and_link_rows(hip_backend):
    """[ACTION, SCENE, CONTACT …, POST] over a scene with per-link outputs and contact slots."""
    _compare_envs(_torch(), "contacts", 130, expect_fold=False)


@pytest.mark.parametrize("n", [130, N_BEYOND_UPKEEP])
def test_fall_back_contact_slots_in_front_of_a_valid_post_op(hip_backend, n):
    """The scene has contact slots: the pair runs as the tile kernel's launch, the post-physics op behind it as its own."""
    _compare_envs(_torch(), "simple_slots", n, expect_fold=False, program=2)


def test_fall_back_profiled_post_phase(hip_backend):
    """A profiled POST phase keeps the plain post-physics kernel in a launch of its own."""
    torch = _torch()
    hip_backend.profile_begin(nat.GF_PHASE_POST, 4 * (STEPS + 6))
    try:
        _compare_envs(torch, "bench", 130, expect_fold=False)
    finally:
        _, samples = hip_backend.profile_end()
    assert samples > 0, "no post-physics launch was profiled"


# ---- errors --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("links", [False, True])
def test_invalid_post_op_behind_a_valid_pair(links):
    """The pair's launch is enqueued, the post-physics op fails with its own index — with per-link outputs too, where the pair folds
    into the tile kernel and the step never would."""
    torch = _torch()
    lib = taf._lib()
    n = 130
    res = {}
    c0 = _count()
    try:
        for on in (True, False):
            _switch(on)
            st = taf._state(torch, n, 12, links=links)
            a, s = taf._args(st, n, 12, nat.GF_ACTION_POSITION)
            taf._per_tick(st, a, s, 0)
            refs = nat.GfPostRefs()   # no termination descriptor: GF_E_NULL
            ops = (nat.GfOp * 3)()
            ops[0].phase, ops[0].args = nat.GF_PHASE_ACTION, C.addressof(a)
            ops[1].phase, ops[1].args = nat.GF_PHASE_SCENE, C.addressof(s)
            ops[2].phase, ops[2].args = nat.GF_OP_POST_PHYSICS, C.addressof(refs)
            failed = C.c_int(-1)
            rc = lib.gf_run_ops(ops, 3, None, C.byref(failed))
            torch.cuda.synchronize()
            res[on] = (rc, failed.value, st)
    finally:
        _switch(True)
    assert _count() == c0
    assert res[True][0] == res[False][0] == -1 and res[True][1] == res[False][1] == 2
    taf._assert_same(torch, res[True][2], res[False][2], "a failed step left other buffers with the fold switched on")
    assert not torch.equal(res[True][2]["dof_pos"], taf._state(torch, n, 12, links=links)["dof_pos"]), "the pair's launch was not enqueued"
