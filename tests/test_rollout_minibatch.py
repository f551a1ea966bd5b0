"""RolloutStorage as the whole rsl_rl storage of a PPO update: observation-group rows and minibatches.

* ``obs_groups`` (rsl_rl's dict form): the gait trainer's asymmetric critic reads ``["policy", "critic"]``.  Every distinct member
  manager gets time-major rows written by the step's own launches; they must equal a torch ``copy_`` storage of
  ``extras["observations"][name]`` bit for bit, on the ordinary, recorded, fused and Python-tail steps.
* ``mini_batch_generator``: rsl_rl's semantics (one ``randperm`` per call shared by the epochs, remainder rows never drawn,
  ``x.flatten(0, 1)[indices]`` per field); on the GPU each minibatch is one ``gf_minibatch_gather`` launch, compared with torch
  indexing bit for bit, and the raw ABI is checked against ``src[indices]``."""
import ctypes as C

import pytest
import torch

GAIT_GROUPS = {"policy": ["policy"], "critic": ["policy", "critic"]}


def _env(kind, n, trace=True, fuse=True, output="fresh"):
    from genesis_forge_amd import tasks
    from genesis_forge_amd.managers import ObservationManager

    old, ObservationManager.default_output = ObservationManager.default_output, output
    try:   # (the managers are created by env.config(), i.e. inside build())
        if kind == "gait":
            env = tasks.Go2GaitTrainingEnv(num_envs=n, max_episode_length_s=0.4, scene_kwargs=dict(ang_noise=0.3, seed=3, contact_prob=0.05))
        elif kind == "gait_curriculum":
            env = tasks.Go2GaitTrainingCurriculumEnv(num_envs=n, max_episode_length_s=0.4, scene_kwargs=dict(ang_noise=0.3, seed=3, contact_prob=0.05))
        elif kind == "go2_hist":
            env = tasks.Go2CommandDirectionEnv(num_envs=n, max_episode_length_s=0.4, cmd_resample_s=0.2, history=3, contacts=True, obs_noise=True,
                                               scene_kwargs=dict(ang_noise=0.3, seed=3))
        else:
            raise KeyError(kind)
        env.trace_enabled = trace
        env.fuse_post_physics = fuse
        env.build()
    finally:
        ObservationManager.default_output = old
    env.seed(7)
    return env


def _check_group_rows(dev, kind, n, trace, fuse=True, output="fresh", horizon=5, steps=13):
    """Steps the env with a group storage attached; after every step the rows equal torch copy_ storages of what the step returned."""
    from genesis_forge_amd.learner import RolloutStorage

    env = _env(kind, n, trace, fuse, output)
    obs, extras = env.reset()
    store = RolloutStorage(env, horizon, obs_groups=GAIT_GROUPS).attach()
    store.begin(obs, extras)
    assert store.group_rows["policy"] is store.observations and set(store.group_rows) == {"policy", "critic"}
    Wc = env.managers["observation"][1].observation_space.shape[0]
    assert store.group_rows["critic"].shape == (horizon + 1, n, Wc)
    ref = {k: torch.zeros(horizon + 1, n, store.group_rows[k].shape[2], device=dev) for k in ("policy", "critic")}
    for k in ref:
        ref[k][0].copy_(extras["observations"][k])
    g = torch.Generator().manual_seed(1)
    d = env.action_space.shape[0]
    dones = 0
    for k in range(steps):
        t = k % horizon
        if t == 0 and k > 0:
            for r in ref.values():
                r[0].copy_(r[horizon])
        obs, rew, term, trunc, extras = env.step(torch.randn(n, d, generator=g).to(dev))
        for name, r in ref.items():
            r[t + 1].copy_(extras["observations"][name])
        assert torch.equal(extras["observations"]["policy"], obs)
        dones += int((term | trunc).sum())
        assert torch.equal(store.observations[: t + 2], ref["policy"][: t + 2]), f"policy rows differ at step {k}"
        assert torch.equal(store.group_rows["critic"][: t + 2], ref["critic"][: t + 2]), f"critic rows differ at step {k}"
    assert dones > 0
    return env, store


@pytest.mark.parametrize("kind,trace,output", [("gait", False, "fresh"), ("gait", True, "fresh"), ("gait_curriculum", True, "fresh"),
                                               ("gait", True, "static"), ("gait", False, "static")])
def test_group_rows_cpu(oracle_backend, kind, trace, output):
    env, _ = _check_group_rows("cpu", kind, 70, trace, output=output)
    assert (env._trace is not None) == trace


def _op_phases(env):
    tr = env._trace
    return [tr.ops[i].phase for i in range(tr.n_ops)]


def _post_shape(env):
    r = env._trace.post_refs
    if r is None:
        return None
    return (bool(r.termination), bool(r.reward), bool(r.reset), r.num_command, r.num_observe, r.num_gait, r.flags, bool(r.rollout))


@pytest.mark.parametrize("output", ["fresh", "static"])
def test_default_groups_record_the_same_step(oracle_backend, output):
    """obs_groups=None: no extra rows, no extra launch — the recorded step is the one a storage built without the argument records."""
    from genesis_forge_amd.learner import RolloutStorage

    env = _env("go2_hist", 70, output=output)
    obs, extras = env.reset()
    shapes = []
    for kw in ({}, {"obs_groups": None}):
        st = RolloutStorage(env, 4, **kw).attach()
        st.begin(obs)
        for _ in range(4):
            obs, *_ = env.step(torch.zeros(70, 12))
        assert env._trace is not None
        assert st.group_rows == {"policy": st.observations} and not st._group_writers
        assert st.obs_groups == {"policy": ["policy"], "critic": ["policy"]}
        shapes.append((_op_phases(env), _post_shape(env), len(env._trace.native), len(env._trace.patches)))
        st.detach()
    assert shapes[0] == shapes[1]


def _fill_policy(env, store, steps, dev, seed=11):
    """A PPO-style collection: env.step → add_policy for ``steps`` transitions, then compute_returns (random policy outputs)."""
    g = torch.Generator().manual_seed(seed)
    n, A = env.num_envs, env.action_space.shape[0]
    for _ in range(steps):
        mu = torch.randn(n, A, generator=g).to(dev)
        sigma = (torch.rand(n, A, generator=g) + 0.5).to(dev)
        actions = mu + sigma * torch.randn(n, A, generator=g).to(dev)
        values = torch.randn(n, 1, generator=g).to(dev)
        logp = torch.randn(n, generator=g).to(dev)
        _obs, _rew, _term, trunc, _ = env.step(actions)
        store.add_policy(actions, values, logp, mu, sigma, time_outs=trunc)
    store.compute_returns(torch.randn(n, 1, generator=g).to(dev))


def _rsl_rl_batches(store, indices, num_mini_batches, num_epochs):
    """rsl_rl's RolloutStorage.mini_batch_generator, expression for expression (critic input: torch.cat of its group's members)."""
    T = store.num_steps
    mb = indices.numel() // num_mini_batches
    flat = {name: r[:T].flatten(0, 1) for name, r in store.group_rows.items()}
    cat = lambda names: torch.cat([flat[m] for m in names], dim=-1)
    obs_all, critic_all = cat(store.obs_groups["policy"]), cat(store.obs_groups["critic"])
    for _ in range(num_epochs):
        for i in range(num_mini_batches):
            b = indices[i * mb:(i + 1) * mb]
            yield (obs_all[b], critic_all[b], store.actions.flatten(0, 1)[b], store.values.flatten(0, 1)[b], store.advantages.flatten(0, 1)[b],
                   store.returns.flatten(0, 1)[b], store.actions_log_prob.flatten(0, 1)[b], store.mu.flatten(0, 1)[b], store.sigma.flatten(0, 1)[b])


def _check_generator(store, num_mini_batches, num_epochs, seed, dev):
    T, n = store.num_steps, store.env.num_envs
    mb = T * n // num_mini_batches
    batches = list(store.mini_batch_generator(num_mini_batches, num_epochs, generator=torch.Generator(device=dev).manual_seed(seed)))
    assert len(batches) == num_mini_batches * num_epochs
    want_idx = torch.randperm(num_mini_batches * mb, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
    got_idx = torch.cat([b.indices for b in batches[:num_mini_batches]])
    assert torch.equal(got_idx, want_idx), "one randperm(num_mini_batches * mb) per call, sliced in order"
    for e in range(1, num_epochs):
        assert torch.equal(torch.cat([b.indices for b in batches[e * num_mini_batches:(e + 1) * num_mini_batches]]), want_idx), \
            "every epoch reuses the permutation"
    if T * n % num_mini_batches:
        assert int(want_idx.max()) < num_mini_batches * mb, "the remainder rows are never drawn"
    for b, want in zip(batches, _rsl_rl_batches(store, want_idx, num_mini_batches, num_epochs)):
        for name, x, y in zip(b._fields, b, want):
            assert x.dtype == torch.float32 and x.shape == y.shape, name
            assert torch.equal(x, y), f"minibatch field {name} differs from rsl_rl's indexing"
    ptrs = {b.obs.data_ptr() for b in batches}
    assert len(ptrs) == len(batches), "every batch is a fresh tensor"
    return batches


def test_generator_semantics_cpu(oracle_backend):
    from genesis_forge_amd.learner import RolloutStorage

    env = _env("gait", 70)
    obs, extras = env.reset()
    store = RolloutStorage(env, 5, obs_groups=GAIT_GROUPS).attach()
    store.begin(obs, extras)
    _fill_policy(env, store, 5, "cpu")
    batches = _check_generator(store, 4, 5, seed=3, dev="cpu")   # 350 transitions: mb = 87, two rows never drawn
    assert batches[0].critic_obs.shape[1] == store.obs_width + store.group_rows["critic"].shape[2]
    assert batches[0].critic_obs is not batches[0].obs

    env2 = _env("go2_hist", 70)
    obs, _ = env2.reset()
    st2 = RolloutStorage(env2, 6).attach()
    st2.begin(obs)
    _fill_policy(env2, st2, 6, "cpu")
    for b in _check_generator(st2, 4, 2, seed=5, dev="cpu"):
        assert b.critic_obs is b.obs, "default groups: the critic input is the policy input, gathered once"


def test_refusals(oracle_backend):
    from genesis_forge_amd.learner import RolloutStorage

    env = _env("gait", 20)
    obs, extras = env.reset()
    with pytest.raises(ValueError, match="no ObservationManager"):
        RolloutStorage(env, 4, obs_groups={"policy": ["policy"], "critic": ["policy", "privileged"]})
    st = RolloutStorage(env, 4, obs_groups=GAIT_GROUPS)
    with pytest.raises(ValueError, match="extras"):
        st.begin(obs)
    with pytest.raises(RuntimeError, match="compute_returns"):
        st.mini_batch_generator(4, 5)
    critic = next(m for m in env.managers["observation"] if m.name == "critic")
    critic.output = "window"
    with pytest.raises(ValueError, match="window"):
        RolloutStorage(env, 4, obs_groups=GAIT_GROUPS)


# -- GPU --------------------------------------------------------------------------------------------------------------------------
def _args(num_rows, num_src_rows, indices, fields):
    from genesis_forge_amd import _native as nat

    a = nat.GfMinibatchArgs()
    a.num_rows, a.num_src_rows, a.indices, a.num_fields = num_rows, num_src_rows, indices, len(fields)
    for f, (src, dst, sw, dw, col) in zip(a.fields, fields):
        f.src, f.dst, f.src_width, f.dst_width, f.dst_col = src, dst, sw, dw, col
    return a


def _gather(b, idx, num_src_rows, fields):
    """fields: (src [R, w] tensor, dst [m, W] tensor, dst_col)."""
    a = _args(idx.numel(), num_src_rows, idx.data_ptr(), [(s.data_ptr(), d.data_ptr(), s.shape[1], d.shape[1], col) for s, d, col in fields])
    b.minibatch_gather(a)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("width,rows", [(w, r) for w in (1, 3, 12, 48, 310, 390) for r in (1, 255)] + [(1, 1048573), (48, 1048573)])
def test_gather_abi_widths(hip_backend, width, rows):
    g = torch.Generator(device="cuda").manual_seed(width * 7 + rows)
    R = max(rows + 17, 5000)
    src = torch.randn(R, width, device="cuda", generator=g)
    idx = torch.randint(0, R, (rows,), device="cuda", generator=g)
    dst = torch.full((rows, width), 7.0, device="cuda")
    _gather(hip_backend, idx, R, [(src, dst, 0)])
    assert torch.equal(dst, src[idx])


@pytest.mark.gpu
def test_gather_abi_columns_alignment_and_size(hip_backend):
    g = torch.Generator(device="cuda").manual_seed(0)
    R, m = 9000, 4097
    idx = torch.randint(0, R, (m,), device="cuda", generator=g)
    # two members of a concatenated group side by side in one [m, 390] output (the gait critic: 310 + 80)
    a, c = torch.randn(R, 310, device="cuda", generator=g), torch.randn(R, 80, device="cuda", generator=g)
    dst = torch.zeros(m, 390, device="cuda")
    _gather(hip_backend, idx, R, [(a, dst, 0), (c, dst, 310)])
    assert torch.equal(dst, torch.cat([a, c], dim=-1)[idx])
    # a dst_col offset inside a wider row; the other columns are left alone
    s = torch.randn(R, 5, device="cuda", generator=g)
    dst = torch.full((m, 11), -3.0, device="cuda")
    _gather(hip_backend, idx, R, [(s, dst, 3)])
    assert torch.equal(dst[:, 3:8], s[idx]) and bool((dst[:, :3] == -3).all()) and bool((dst[:, 8:] == -3).all())
    # misaligned base pointers: source and destination start one float into their allocations
    for w in (12, 48, 2):
        sbuf = torch.randn(R * w + 1, device="cuda", generator=g)
        dbuf = torch.zeros(m * w + 3, device="cuda")
        src, dst = sbuf[1:1 + R * w].view(R, w), dbuf[1:1 + m * w].view(m, w)
        _gather(hip_backend, idx, R, [(src, dst, 0)])
        assert torch.equal(dst, src[idx])
        assert float(dbuf[0]) == 0 and bool((dbuf[1 + m * w:] == 0).all())
    # Go2's 65 536 x 24 rollout at width 48: 302 MB of source, past the Infinity Cache; and every field width of a minibatch at once
    R = 65536 * 24
    src = torch.randn(R, 48, device="cuda", generator=g)
    idx = torch.randperm(R, device="cuda", generator=g)[: R // 4]
    outs = [torch.empty(R // 4, 48, device="cuda")]
    small = [torch.randn(R, w, device="cuda", generator=g) for w in (12, 1, 1, 1, 1, 12, 12)]
    outs += [torch.empty(R // 4, s.shape[1], device="cuda") for s in small]
    _gather(hip_backend, idx, R, [(src, outs[0], 0)] + [(s, o, 0) for s, o in zip(small, outs[1:])])
    for s, o in zip([src] + small, outs):
        assert torch.equal(o, s[idx])


@pytest.mark.gpu
def test_gather_abi_out_of_range_indices_are_nan(hip_backend):
    """The source has 8 rows of slack past the num_src_rows passed: indices into the slack (and -1) must give NaN rows and no load."""
    g = torch.Generator(device="cuda").manual_seed(1)
    R = 1000
    src = torch.randn(R + 8, 48, device="cuda", generator=g)
    s1 = torch.randn(R + 8, 1, device="cuda", generator=g)
    idx = torch.randint(0, R, (300,), device="cuda", generator=g)
    bad = torch.tensor([3, 50, 51, 299, 120], device="cuda")
    idx[bad] = torch.tensor([R, R + 3, R + 7, -1, R + 1], device="cuda")
    dst, d1 = torch.zeros(300, 48, device="cuda"), torch.zeros(300, 1, device="cuda")
    _gather(hip_backend, idx, R, [(src, dst, 0), (s1, d1, 0)])
    ok = torch.ones(300, dtype=torch.bool, device="cuda")
    ok[bad] = False
    assert torch.equal(dst[ok], src[idx[ok]]) and torch.equal(d1[ok], s1[idx[ok]])
    assert bool(torch.isnan(dst[~ok]).all()) and bool(torch.isnan(d1[~ok]).all())


@pytest.mark.gpu
def test_gather_abi_refusals(hip_backend):
    from genesis_forge_amd import _native as nat

    lib = hip_backend.lib
    src, dst = torch.zeros(10, 4, device="cuda"), torch.zeros(5, 4, device="cuda")
    idx = torch.zeros(5, dtype=torch.int64, device="cuda")
    ok = (src.data_ptr(), dst.data_ptr(), 4, 4, 0)
    call = lambda a: lib.gf_minibatch_gather(C.byref(a), None)
    assert lib.gf_sizeof(nat.GF_SIZEOF_MINIBATCH) == C.sizeof(nat.GfMinibatchArgs)
    assert call(_args(5, 10, idx.data_ptr(), [ok])) == 0
    assert call(_args(5, 10, None, [ok])) == -1
    assert call(_args(5, 10, idx.data_ptr(), [(None, dst.data_ptr(), 4, 4, 0)])) == -1
    assert call(_args(5, 10, idx.data_ptr(), [(src.data_ptr(), None, 4, 4, 0)])) == -1
    assert call(_args(5, 10, idx.data_ptr(), [])) == -2
    a = _args(5, 10, idx.data_ptr(), [ok] * 12)
    a.num_fields = 13
    assert call(a) == -2
    assert call(_args(5, 10, idx.data_ptr(), [(src.data_ptr(), dst.data_ptr(), 0, 4, 0)])) == -2
    assert call(_args(5, 10, idx.data_ptr(), [(src.data_ptr(), dst.data_ptr(), 4, 0, 0)])) == -2
    assert call(_args(5, 10, idx.data_ptr(), [(src.data_ptr(), dst.data_ptr(), 4, 4, 1)])) == -2
    assert call(_args(5, 0, idx.data_ptr(), [ok])) == -2
    dst.fill_(5.0)
    torch.cuda.synchronize()
    assert call(_args(0, 10, idx.data_ptr(), [ok])) == 0
    torch.cuda.synchronize()
    assert bool((dst == 5).all()), "num_rows == 0 launches nothing"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1000, 8192])
@pytest.mark.parametrize("fuse,output", [(True, "fresh"), (False, "fresh"), (True, "static"), (False, "static")])
def test_group_rows_hip(hip_backend, n, fuse, output):
    _check_recorded_shape("cuda", n, fuse, output)


@pytest.mark.parametrize("fuse,output", [(True, "fresh"), (True, "static")])
def test_group_rows_recorded_shape_cpu(oracle_backend, fuse, output):
    _check_recorded_shape("cpu", 70, fuse, output)


def _check_recorded_shape(dev, n, fuse, output):
    from genesis_forge_amd.learner import RolloutStorage

    env, store = _check_group_rows(dev, "gait", n, True, fuse=fuse, output=output)
    tr = env._trace
    assert tr is not None
    with_group = (_op_phases(env), _post_shape(env))
    # the same env with a default storage: the group rows add no op (fresh: the gathers store them) or at most one (static)
    store.detach()
    obs, _ = env.reset()
    st = RolloutStorage(env, 5).attach()
    st.begin(obs)
    for _ in range(4):
        env.step(torch.zeros(n, env.action_space.shape[0], device=dev))
    plain = (_op_phases(env), _post_shape(env))
    if fuse:
        assert with_group[1] is not None and with_group[1] == plain[1], "the fused launch is kept"
        extra = len(with_group[0]) - len(plain[0])
        assert extra == 0 if output == "fresh" else 0 <= extra <= 1, (with_group[0], plain[0])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [("gait", 1000), ("go2_hist", 4096)])
def test_full_rollout_minibatches_hip(hip_backend, kind, n):
    """One rollout of 24 transitions, compute_returns, then 4 minibatches x 5 epochs: every HIP batch equals torch indexing."""
    from genesis_forge_amd.learner import RolloutStorage

    env = _env(kind, n)
    obs, extras = env.reset()
    store = RolloutStorage(env, 24, obs_groups=GAIT_GROUPS if kind == "gait" else None).attach()
    store.begin(obs, extras)
    _fill_policy(env, store, 24, "cuda")
    assert env._trace is not None
    batches = _check_generator(store, 4, 5, seed=9, dev="cuda")
    if kind == "gait":
        assert batches[0].critic_obs.shape[1] == 390 and batches[0].obs.shape[1] == 310
    else:
        assert all(b.critic_obs is b.obs for b in batches)
