"""The fused post-physics launch at its table limits and one entry past them (configs: tests/post_capacity_cases.py).

At a limit the recorded step must be ONE launch of the fused kernel and equal the phase-by-phase step bit for bit; one entry past it
the step must leave the kernel by the rule of exactly that limit — onto the phase chains, or, for a third observation manager, with
the surplus manager observing behind a fused launch of the first two — and still equal the phase-by-phase step.

The CPU half needs no kernel: the oracle computes, the HIP library's host-only entry points (gf_post_physics_check / _describe /
_lds_bytes) decide and describe.  Two limits are not reachable through an env and are pinned on copies of recorded descriptors: a
256-wide frame (the ObservationManager raises at build()) and a third command manager (the recorder keeps the chains before it asks).

The dynamic LDS of the launch grows with the frame width: 86 912 B for a 255-wide frame at 32 DOF, more than the 64 KiB most kernels
stop at.  profiles/post_capacity.md records that a plain launch on an MI355X takes it (sharedMemPerBlock is 160 KiB); DEVICE_LDS_BYTES
is that measured limit, and no descriptor pack() admits may ask for more.
"""
import os
import re
import subprocess
import sys

import ctypes as C

import pytest
import torch

import post_capacity_cases as pc
from genesis_forge_amd import _native as nat

DEVICE_LDS_BYTES = 160 * 1024   # hipDeviceProp_t::sharedMemPerBlock of the MI355X (profiles/post_capacity.md)
N_CPU, STEPS = 33, 40
# what the packed descriptor of an at-limit config must say (gf_post_physics_describe): the table really is full
SAYS = {
    "term8": ["n_term = 8;"], "rew16": ["n_rew = 16;"], "rew16of24": ["n_rew = 16;"],
    "items12": ["width 91 history 2 items {{"], "width255": ["DV = 8;", "obs[0]: width 255 history 2"], "width255_dof12": ["DV = 3;", "obs[0]: width 255 history 2"],
    "obs2": ["n_obs = 2;"], "cmd2": ["n_cmd = 2;"], "ranges4": ["cmd_width = {4, 1}"],
    "everything28": ["DV = 7;", "n_term = 8;", "n_rew = 16;", "n_cmd = 2;", "cmd_width = {3, 4}", "n_obs = 2;", "obs[0]: width 255 history 2"],
    "everything32": ["DV = 8;", "n_term = 8;", "n_rew = 16;", "n_cmd = 2;", "cmd_width = {3, 4}", "n_obs = 2;", "obs[0]: width 255 history 2"],
}


@pytest.fixture()
def pack_oracle(oracle_lib_path):
    """The oracle as compute backend with the HIP library's pack() deciding what fuses, GF_OPT_POST_VARIANT = 1 (the interpreter)."""
    from genesis_forge_amd import gs

    old_dev = gs.device
    gs.set_device("cpu")
    b = pc.pack_checked_backend(oracle_lib_path)
    nat.set_backend(b)
    b.hip.set_option(nat.GF_OPT_POST_VARIANT, 1)
    yield b
    b.hip.set_option(nat.GF_OPT_POST_VARIANT, 2)
    nat.set_backend(None)
    gs.device = old_dev


_ordinary = {}   # (case, device, n) -> the phase-by-phase run: computed once, read by every test that compares against it


def _reference(name, spec, dev, n):
    key = (name, dev, n)
    if key not in _ordinary:
        _ordinary[key] = pc.run(spec, dev, "ordinary", n, STEPS)[0]
    return _ordinary[key]


def _fused_kind(env):
    tr = env._trace
    assert tr is not None, f"the step was not recorded: {getattr(env, '_untraceable', None)}"
    return tr.post_refs


def _count_items(text, m):
    """Items of observation manager ``m`` in a describe() signature."""
    body = text.split(f"obs[{m}]:")[1].split("items {")[1].split("};")[0]
    return body.count("{")


# ---- CPU: the decision, the rule, the inputs, oracle parity ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.AT))
def test_at_limit_fuses_and_equals_phase_by_phase_cpu(pack_oracle, name):
    spec = pc.AT[name]
    fused, env = pc.run(spec, "cpu", "fused", N_CPU, STEPS)
    refs = _fused_kind(env)
    assert refs is not None, "a config AT the limit must take the fused kernel"
    text = pack_oracle.hip.post_describe(refs)
    assert text.startswith("program 0 (interpreter)"), text[:60]
    for want in SAYS.get(name, []):
        assert want in text, (want, text)
    if name.startswith(("items12", "width255", "everything")):
        assert _count_items(text, 0) == 12, text
    if name in ("items12x2", "everything28", "everything32"):
        assert _count_items(text, 1) == 12, text
    if name in ("rew16of24", "everything28", "everything32"):
        rw = C.cast(refs.reward, C.POINTER(nat.GfRewardArgs)).contents
        rs = C.cast(refs.reset, C.POINTER(nat.GfResetArgs)).contents
        assert rw.num_terms == 16 and max(rw.terms[k].row for k in range(16)) == 23 and rs.num_reward_terms == 24
        assert bin(rs.reward_log_mask).count("1") == 16 and rs.reward_logging == 1
    if name == "views4":
        assert env.reward_manager._program.slots.cmds.__len__() == 4
    if name == "contacts4":
        assert len(env.managers["contact"]) == 4
    ref = _reference(name, spec, "cpu", N_CPU)
    pc.same(ref, fused, name)
    assert pc.resets(ref) > 0, "no env reset: the reset path went untested"


@pytest.mark.parametrize("name", list(pc.PAST))
def test_one_past_leaves_the_fused_kernel_and_equals_phase_by_phase_cpu(pack_oracle, name):
    spec, _rule, how = pc.PAST[name]
    rec, env = pc.run(spec, "cpu", "fused", N_CPU, STEPS)
    refs = _fused_kind(env)
    if how == "chains":
        assert refs is None, "one entry past the limit the step must run on the phase chains"
    else:   # a third observation manager: the first two stay in the fused launch, the third observes behind it
        assert refs is not None and refs.num_observe == nat.GF_POST_MAX_OBS and len(env.obs_managers) == nat.GF_POST_MAX_OBS + 1
    ref = _reference(name, spec, "cpu", N_CPU)
    pc.same(ref, rec, name)
    assert pc.resets(ref) > 0


def test_a_256_wide_frame_is_refused_at_build_and_by_pack(pack_oracle):
    """The one-past side of the width limit: the ObservationManager refuses the config before a step exists, and pack() refuses the
    same width on descriptors (as it does a third observation / command manager, which the recorder never sends)."""
    with pytest.raises(ValueError, match="wider than 255"):
        pc.run(pc.WIDTH256, "cpu", "fused", 4, steps=1)
    _seq, env = pc.run(pc.AT["width255"], "cpu", "fused", 4, steps=3)
    hip = pack_oracle.hip
    assert hip.post_check(nat.GfPostRefs.from_buffer_copy(env._trace.post_refs)), "the unchanged copy must pack"
    for which in pc.RAW_RULE:
        refs, _keep = pc.raw_past_refs(env, which)
        assert not hip.post_check(refs), which
        assert hip.lib.gf_post_physics_describe(C.byref(refs), C.create_string_buffer(64), 64) == -5   # GF_E_UNSUPPORTED


def test_one_past_means_exactly_one_rule():
    """GF_POST_WHY names the rule that kept a step off the fused kernel (read once per process: a fresh child).  Every refusal of a
    one-past config must be the rule of the limit under test — an earlier rule would mean the config misses its limit."""
    env = dict(os.environ, GF_POST_WHY="1")
    env.pop("GF_NO_FUSE", None)
    p = subprocess.run([sys.executable, pc.__file__, "why"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    seen, fused, case = {}, {}, None
    for line in p.stderr.splitlines():
        if line.startswith("case "):
            case = line.split()[1]
            seen[case] = []
        elif line.startswith("fused "):
            fused[line.split()[1]] = line.split()[2] == "True"
        else:
            m = re.match(r"gf_post_physics: not fusable \(.*gf_post\.hip:\d+\): (.*)$", line)
            if m and case:
                seen[case].append(m.group(1))
    for name, (_spec, rule, how) in pc.PAST.items():
        assert fused[name] == (how == "late"), name
        want = [] if rule is None else [pc.RULE[rule]]   # (obs3 / cmd3: the recorder never sends the surplus manager)
        assert sorted(set(seen[name])) == want, (name, seen[name])
    for which, rule in pc.RAW_RULE.items():
        assert not fused["raw_" + which]
        assert sorted(set(seen["raw_" + which])) == [pc.RULE[rule]], (which, seen["raw_" + which])


@pytest.mark.parametrize("name", list(pc.DECISIVE))
def test_the_last_table_entry_is_decisive_cpu(oracle_backend, name):
    """Guards the INPUTS, phase by phase on the oracle: the config's last table entry — the one a kernel that stops one short would
    lose — changes the outputs."""
    spec, what = pc.AT[name], pc.DECISIVE[name]
    full = _reference(name, spec, "cpu", N_CPU)
    less = pc.run(spec, "cpu", "ordinary", N_CPU, STEPS, drop=what)[0]
    assert pc.resets(full) > 0
    if what == "term":
        assert any(not torch.equal(a["terminated"], b["terminated"]) or not torch.equal(a["truncated"], b["truncated"]) for a, b in zip(full, less))
    elif what == "rew":
        assert not torch.equal(full[0]["reward"], less[0]["reward"]), "the sixteenth reward term adds nothing at step 0"
        assert full[-1]["episode_sums"].shape[0] == less[-1]["episode_sums"].shape[0] + 1
    else:
        frame, short = full[0]["obs"].shape[1] // spec.history, less[0]["obs"].shape[1] // spec.history
        assert frame > short
        assert any(bool((s["obs"][:, short:frame] != 0).any()) for s in full), "the last item's columns are zero on every env and step"


def test_no_admitted_descriptor_asks_for_more_lds_than_a_workgroup_has(pack_oracle):
    """post_launch() hands the launch its dynamic LDS unchecked, so the bound must hold by construction: the interpreter's request at
    the widest admitted frame — any DOF count, with a gait manager, the tick variant's handed rows included — stays under the
    device's limit; and the at-limit configs ask for what the bound says."""
    lib = pack_oracle.hip.lib
    worst = max(lib.gf_post_interp_lds_bytes(d, nat.GF_MAX_OBS_WIDTH - 1, g, t) for d in range(1, 33) for g in (0, 1) for t in (0, 1))
    assert worst == lib.gf_post_interp_lds_bytes(32, nat.GF_MAX_OBS_WIDTH - 1, 1, 1)
    assert 64 * 1024 < worst <= DEVICE_LDS_BYTES, worst
    for name, dofs in (("width255", 32), ("width255_dof12", 12), ("everything28", 28), ("everything32", 32)):
        _seq, env = pc.run(pc.AT[name], "cpu", "fused", 4, steps=3)
        got = pack_oracle.hip.post_lds_bytes(env._trace.post_refs)
        assert got == lib.gf_post_interp_lds_bytes(dofs, 255, 0, 0) and 64 * 1024 < got <= worst, (name, got)
    # 16 reward rows + 21 exchange rows + 4 rows per float4 chunk of a DOF row + the 256-column tile, 64 envs of 4 bytes each
    assert lib.gf_post_interp_lds_bytes(32, 255, 0, 0) - lib.gf_post_interp_lds_bytes(32, 0, 0, 0) == 255 * 256
    assert lib.gf_post_interp_lds_bytes(32, 0, 0, 0) - lib.gf_post_interp_lds_bytes(4, 0, 0, 0) == 28 * 256


def _plugin_for(hip, refs):
    """Compile (or find cached) and register the static program of these descriptors; returns (id, the plugin's own LDS size function)."""
    from genesis_forge_amd import _programs

    hip.set_option(nat.GF_OPT_POST_VARIANT, 1)
    sig = hip.post_describe(refs)
    hip.set_option(nat.GF_OPT_POST_VARIANT, 2)
    so, _secs = _programs.compile_sync(sig)
    fn = C.CDLL(so).gfp_lds_bytes
    fn.restype, fn.argtypes = C.c_size_t, [C.c_int, C.c_int]
    return hip.register_program(so), fn


def test_a_compiled_program_that_needs_more_lds_than_a_workgroup_has_is_passed_over(pack_oracle):
    """Host-only (signature -> hipcc -> register -> select): a static program parks one LDS row per link of its contact-force-norm
    items.  For two managers of 255 norm columns that is 510 rows on top of the tile, more than the device's 160 KiB — launching it
    would fail in the middle of env.step().  The library must keep such a step on the interpreter; a wide frame whose program fits
    (width255: 19 norm rows) still gets its program."""
    from genesis_forge_amd import _programs

    if _programs.hipcc() is None:
        pytest.skip("no hipcc")
    hip = pack_oracle.hip
    try:
        _seq, env = pc.run(pc.AT["norms255x2"], "cpu", "fused", 4, steps=3)
        refs = env._trace.post_refs
        pid, plugin_lds = _plugin_for(hip, refs)
        assert pid >= 100 and plugin_lds(255, 0) > DEVICE_LDS_BYTES, plugin_lds(255, 0)
        assert hip.post_describe(refs).startswith("program 0 (interpreter)"), "the step selected a program that cannot be launched"
        assert hip.post_lds_bytes(refs) == hip.lib.gf_post_interp_lds_bytes(12, 255, 0, 0) <= DEVICE_LDS_BYTES
        _seq, env = pc.run(pc.AT["width255"], "cpu", "fused", 4, steps=3)
        refs = env._trace.post_refs
        pid, plugin_lds = _plugin_for(hip, refs)
        assert hip.post_describe(refs).startswith(f"program {pid} (jit_")
        assert hip.post_lds_bytes(refs) == plugin_lds(255, 0) <= DEVICE_LDS_BYTES
    finally:
        hip.set_option(nat.GF_OPT_POST_VARIANT, 1)   # (the fixture's state)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def post_variant(hip_backend, request):
    hip_backend.set_option(nat.GF_OPT_POST_VARIANT, request.param)
    yield request.param
    hip_backend.set_option(nat.GF_OPT_POST_VARIANT, 2)


def _direct_launch(hip_backend, refs):
    rc = hip_backend.post_step_contacts(refs, [])
    assert rc == 0, nat.GF_ERRORS.get(rc, rc)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("post_variant", [1], indirect=True)
def test_a_launch_with_more_than_64k_of_lds_is_accepted_hip(hip_backend, post_variant):
    """The narrowest run that settles it: the 255-wide frame at 32 DOF, 65 envs, ONE direct launch, its status asserted."""
    _seq, env = pc.run(pc.AT["width255"], "cuda", "fused", 65, steps=3)
    refs = _fused_kind(env)
    assert refs is not None
    lds = hip_backend.post_lds_bytes(refs)
    limit = torch.cuda.get_device_properties(0).shared_memory_per_block
    print(f"post_capacity: width255 at 32 DOF asks for {lds} B of dynamic LDS; sharedMemPerBlock = {limit} B")
    assert 64 * 1024 < lds <= limit
    _direct_launch(hip_backend, refs)
    print("post_capacity: the launch returned GF_OK")
    worst = hip_backend.lib.gf_post_interp_lds_bytes(32, nat.GF_MAX_OBS_WIDTH - 1, 1, 1)
    assert worst <= limit and limit == DEVICE_LDS_BYTES, (worst, limit)


@pytest.mark.gpu
@pytest.mark.parametrize("post_variant", [1], indirect=True)
@pytest.mark.parametrize("n", [1, 65, 130])
@pytest.mark.parametrize("name", list(pc.AT))
def test_at_limit_fused_equals_unfused_equals_ordinary_hip(hip_backend, post_variant, name, n):
    spec = pc.AT[name]
    a = _reference(name, spec, "cuda", n)
    b, env_b = pc.run(spec, "cuda", "unfused", n, STEPS)
    c, env_c = pc.run(spec, "cuda", "fused", n, STEPS)
    assert env_b._trace is not None and env_b._trace.post_refs is None
    refs = _fused_kind(env_c)
    assert refs is not None, "a config AT the limit must take the fused kernel"
    assert hip_backend.post_describe(refs).startswith("program 0 (interpreter)")
    pc.same(a, b, f"{name} chains")
    pc.same(a, c, f"{name} fused")
    if n > 1:
        assert pc.resets(a) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("post_variant", [1], indirect=True)
@pytest.mark.parametrize("n", [1, 65, 130])
@pytest.mark.parametrize("name", list(pc.PAST))
def test_one_past_runs_the_chains_and_equals_ordinary_hip(hip_backend, post_variant, name, n):
    spec, _rule, how = pc.PAST[name]
    a = _reference(name, spec, "cuda", n)
    b, env = pc.run(spec, "cuda", "fused", n, STEPS)
    refs = _fused_kind(env)
    if how == "chains":
        assert refs is None, "one entry past the limit the step must run on the phase chains"
    else:
        assert refs is not None and refs.num_observe == nat.GF_POST_MAX_OBS
    pc.same(a, b, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["everything28", "width255", "rew16"])
def test_static_program_at_the_limits_hip(hip_backend, name):
    """GF_OPT_POST_VARIANT 2 with a program compiled for exactly this structure (jit_programs = "sync"): arrays of the table sizes
    (vals[kPostMaxReward], item[GF_POST_MAX_OBS][kPostMaxItems]) filled to the last entry."""
    spec, n = pc.AT[name], 65
    a = _reference(name, spec, "cuda", n)
    c, env = pc.run(spec, "cuda", "fused", n, STEPS, jit="sync")
    refs = _fused_kind(env)
    assert refs is not None
    what = hip_backend.post_describe(refs).split(":")[0]
    assert re.match(r"program [1-9]\d\d \(jit_[0-9a-f]+\)", what), f"{what} (compile: {env._program_info})"
    pc.same(a, c, f"{name} static program")


@pytest.mark.gpu
def test_a_config_whose_compiled_program_would_not_fit_runs_the_interpreter_hip(hip_backend):
    """jit_programs = "sync" compiles and registers the program of the 2 x 255 norm-column config; the step must run — on the
    interpreter — and equal the phase-by-phase step."""
    spec, n = pc.AT["norms255x2"], 65
    a = _reference("norms255x2", spec, "cuda", n)
    c, env = pc.run(spec, "cuda", "fused", n, STEPS, jit="sync")
    refs = _fused_kind(env)
    assert refs is not None
    assert hip_backend.post_describe(refs).startswith("program 0 (interpreter)"), env._program_info
    pc.same(a, c, "norms255x2 with its program registered")


SENTINEL = -12345.0


@pytest.mark.gpu
@pytest.mark.parametrize("post_variant", [1], indirect=True)
@pytest.mark.parametrize("n", [65, 130])
@pytest.mark.parametrize("name", ["width255", "everything32"])
def test_rows_behind_the_last_env_survive_a_launch_hip(hip_backend, post_variant, name, n):
    """One direct launch into buffers of the test's own with three sentinel rows behind env N-1 of every observation, the reward
    and the episode sums: the last tile's idle lanes (63 of 64 at N = 65) and the rows past the table must store nothing."""
    _seq, env = pc.run(pc.AT[name], "cuda", "fused", n, steps=3)
    refs = _fused_kind(env)
    assert refs is not None
    rw = C.cast(refs.reward, C.POINTER(nat.GfRewardArgs)).contents
    rs = C.cast(refs.reset, C.POINTER(nat.GfResetArgs)).contents
    obs = [C.cast(refs.observe[m], C.POINTER(nat.GfObservationArgs)).contents for m in range(refs.num_observe)]
    old = (rw.reward, rw.episode_sums, rs.episode_sums, [o.obs for o in obs])
    rows = rs.num_reward_terms
    assert rows == env.reward_manager._episode_sums.shape[0] and not any(o.ring_slots for o in obs)
    dev = "cuda"
    reward = torch.full((n + 3,), SENTINEL, device=dev)
    sums = torch.full((rows + 3, n), SENTINEL, device=dev)
    sums[:rows] = env.reward_manager._episode_sums
    frames = [torch.full((n + 3, o.obs_width * o.history_len), SENTINEL, device=dev) for o in obs]
    try:
        rw.reward, rw.episode_sums, rs.episode_sums = reward.data_ptr(), sums.data_ptr(), sums.data_ptr()
        for o, t in zip(obs, frames):
            o.obs = t.data_ptr()
        _direct_launch(hip_backend, refs)
    finally:
        rw.reward, rw.episode_sums, rs.episode_sums = old[0], old[1], old[2]
        for o, p in zip(obs, old[3]):
            o.obs = p
    assert bool((reward[n:] == SENTINEL).all()) and bool((reward[:n] != SENTINEL).all())
    assert bool((sums[rows:] == SENTINEL).all()) and bool((sums[:rows] != SENTINEL).all())
    for m, t in enumerate(frames):
        assert bool((t[n:] == SENTINEL).all()), f"observation manager {m}: a row behind env {n - 1} was written"
        width = obs[m].obs_width
        # (a history kept as a ring takes the new frame in the slot of this step, any other layout every column)
        assert bool(((t[:n] != SENTINEL).sum(dim=1) >= width).all()), f"observation manager {m}: the launch left columns of the new frame unwritten"
