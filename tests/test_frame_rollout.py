"""RolloutStorage(history="frames"): a history observation is stored once per frame, the minibatch gather rebuilds the rows.

* rows through frames: after every step ``observation_rows()`` equals torch copies of what the steps returned — ``fresh`` / ``static`` /
  ``window`` outputs, recorded and ordinary steps, across storage wraps (also the overlapping wrap copy of H > T);
* the minibatches of a ``frames`` + ``window`` rollout are bit for bit those of its ``rows`` + ``fresh`` twin (also normalised);
* refusals and defaults;
* GPU, raw ABI: ``gf_minibatch_gather`` history fields against torch indexing, ``gf_rollout_frame_write`` against torch slicing;
* one collection and PPO update on ``frames`` + ``window`` ends with the parameters of the ``rows`` + ``fresh`` twin.

Every comparison is a pure copy or the same arithmetic on the same values: ``torch.equal`` throughout."""
import ctypes as C

import pytest
import torch

GAIT_GROUPS = {"policy": ["policy"], "critic": ["policy", "critic"]}
E_NULL, E_RANGE = -1, -2


def _env(kind, n, trace=True, fuse=True, output="fresh"):
    from genesis_forge_amd import tasks
    from genesis_forge_amd.managers import ObservationManager

    old, ObservationManager.default_output = ObservationManager.default_output, output
    try:   # (the managers are created by env.config(), i.e. inside build())
        if kind == "gait":
            env = tasks.Go2GaitTrainingEnv(num_envs=n, max_episode_length_s=0.4, scene_kwargs=dict(ang_noise=0.3, seed=3, contact_prob=0.05))
        elif kind == "go2_hist":
            env = tasks.Go2CommandDirectionEnv(num_envs=n, max_episode_length_s=0.4, cmd_resample_s=0.2, history=3, contacts=True, obs_noise=True,
                                               scene_kwargs=dict(ang_noise=0.3, seed=3))
        elif kind == "go2":
            env = tasks.Go2CommandDirectionEnv(num_envs=n, max_episode_length_s=0.4, cmd_resample_s=0.2, scene_kwargs=dict(ang_noise=0.3, seed=3))
        else:
            raise KeyError(kind)
        env.trace_enabled = trace
        env.fuse_post_physics = fuse
        env.build()
    finally:
        ObservationManager.default_output = old
    assert all(m._output == output for m in env.managers["observation"])
    env.seed(7)
    return env


def _groups(kind):
    return GAIT_GROUPS if kind == "gait" else None


# ---- 1. rows through frames ---------------------------------------------------------------------------------------------------------
def _check_frames(dev, kind, n, trace, output, fuse=True, horizon=5, steps=17):
    """The shape of test_learner._check_rollout: the reference side is plain torch copies of what step() returned."""
    from genesis_forge_amd.learner import RolloutStorage

    env = _env(kind, n, trace, fuse, output)
    obs, extras = env.reset()
    store = RolloutStorage(env, horizon, obs_groups=_groups(kind), history="frames").attach()
    store.begin(obs, extras)
    names = sorted({m for members in store.obs_groups.values() for m in members})
    assert set(store.frames) == set(names) and not store.group_rows and store.observations is None
    for name in names:
        om = next(m for m in env.managers["observation"] if m.name == name)
        W = om.observation_space.shape[0]
        assert store.frames[name].shape == (horizon + om._history_len, n, W // om._history_len) and store.frames[name].is_contiguous()
    ref = {name: torch.zeros(horizon + 1, n, extras["observations"][name].shape[1], device=dev) for name in names}
    for name in names:
        ref[name][0].copy_(extras["observations"][name])
        assert torch.equal(store.observation_rows(name, 0), ref[name][0])
    ref_rew = torch.zeros(horizon, n, device=dev)
    ref_done = torch.zeros(horizon, n, dtype=torch.bool, device=dev)
    g = torch.Generator().manual_seed(1)
    d = env.action_space.shape[0]
    dones = 0
    for k in range(steps):
        t = k % horizon
        if t == 0 and k > 0:
            for r in ref.values():
                r[0].copy_(r[horizon])
        obs, rew, term, trunc, extras = env.step(torch.randn(n, d, generator=g).to(dev))
        assert torch.equal(extras["observations"]["policy"], obs)
        for name in names:
            ref[name][t + 1].copy_(extras["observations"][name])
        ref_rew[t].copy_(rew)
        ref_done[t].copy_(term | trunc)
        dones += int((term | trunc).sum())
        assert store.step == t + 1 and store.full == (t + 1 == horizon)
        for name in names:
            assert torch.equal(store.observation_rows(name, t + 1), extras["observations"][name]), f"row {t + 1} of '{name}' differs at step {k}"
            assert torch.equal(store.observation_rows(name)[: t + 2], ref[name][: t + 2]), f"the rows of '{name}' differ from the torch copies at step {k}"
        assert torch.equal(store.observation_rows(None, t + 1), obs)
        assert torch.equal(store.rewards[: t + 1], ref_rew[: t + 1]), f"rewards differ from the torch copy_ storage at step {k}"
        assert torch.equal(store.dones[: t + 1], ref_done[: t + 1]), f"dones differ from the torch copy_ storage at step {k}"
    assert dones > 0
    assert (env._trace is not None) == trace, getattr(env, "_untraceable", None)
    return env, store


OUTPUTS = ("fresh", "static", "window")


@pytest.mark.parametrize("output", OUTPUTS)
@pytest.mark.parametrize("trace", [True, False])
@pytest.mark.parametrize("kind", ["go2_hist", "gait"])
def test_frames_hold_the_rows_cpu(oracle_backend, kind, trace, output):
    _check_frames("cpu", kind, 70, trace, output)


@pytest.mark.parametrize("output", OUTPUTS)
@pytest.mark.parametrize("trace", [True, False])
def test_frames_wrap_copy_overlaps_cpu(oracle_backend, trace, output):
    """Horizon 2 with the gait task's H = 5: the wrap copy frames[0:H] <- frames[T:T+H] overlaps itself."""
    _check_frames("cpu", "gait", 70, trace, output, horizon=2)


@pytest.mark.gpu
@pytest.mark.parametrize("output", OUTPUTS)
@pytest.mark.parametrize("trace,fuse", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("kind", ["go2_hist", "gait"])
def test_frames_hold_the_rows_hip(hip_backend, kind, trace, fuse, output):
    _check_frames("cuda", kind, 1000, trace, output, fuse=fuse)


@pytest.mark.gpu
@pytest.mark.parametrize("output", OUTPUTS)
@pytest.mark.parametrize("trace", [True, False])
def test_frames_wrap_copy_overlaps_hip(hip_backend, trace, output):
    _check_frames("cuda", "gait", 1000, trace, output, horizon=2)


# ---- 2. same minibatches ------------------------------------------------------------------------------------------------------------
def _fill_policy(env, store, steps, dev, seed=11):
    """A PPO-style collection: env.step -> add_policy for ``steps`` transitions, then compute_returns (random policy outputs)."""
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


def _normalizer(width, dev, seed):
    from genesis_forge_amd.learner import EmpiricalNormalization

    norm = EmpiricalNormalization(width)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        norm._mean.copy_(torch.randn(1, width, generator=g) * 0.3)
        norm._std.copy_(torch.rand(1, width, generator=g) + 0.5)
        norm._var.copy_(norm._std ** 2)
    return norm.to(dev).eval()


def _check_same_minibatches(dev, kind, n, T=6):
    from genesis_forge_amd.learner import RolloutStorage

    stores = []
    for history, output in (("rows", "fresh"), ("frames", "window")):
        env = _env(kind, n, output=output)
        obs, extras = env.reset()
        st = RolloutStorage(env, T, obs_groups=_groups(kind), history=history).attach()
        st.begin(obs, extras)
        _fill_policy(env, st, T + 2, dev)   # (two steps into the second rollout: the gathered rows have been through a wrap)
        _fill_policy(env, st, T - 2, dev, seed=12)
        assert st.full
        stores.append(st)
    rows, frames = stores
    assert set(frames.frames) == {m for members in frames.obs_groups.values() for m in members} and frames.observations is None
    for k in ("actions", "values", "returns", "advantages", "actions_log_prob", "mu", "sigma", "rewards", "dones"):
        assert torch.equal(getattr(rows, k), getattr(frames, k)), f"the twins' {k} differ: the comparison below would mean nothing"
    wp = sum(rows.group_rows[m].shape[2] for m in rows.obs_groups["policy"])
    wc = sum(rows.group_rows[m].shape[2] for m in rows.obs_groups["critic"])
    for norms in ({}, {"obs_normalizer": _normalizer(wp, dev, 1), "critic_obs_normalizer": _normalizer(wc, dev, 2)}):
        a, b = (list(st.mini_batch_generator(4, 2, generator=torch.Generator(device=dev).manual_seed(5), **norms)) for st in stores)
        assert len(a) == len(b) == 8
        for x, y in zip(a, b):
            for name, u, v in zip(x._fields, x, y):
                assert u.shape == v.shape and u.dtype == v.dtype, name
                assert torch.equal(u, v), f"minibatch field {name} of the frame-stored rollout differs from the row-stored twin's"
            assert (y.critic_obs is y.obs) == (x.critic_obs is x.obs)
            assert not bool(torch.isnan(y.obs).any()) and not bool(torch.isnan(y.critic_obs).any())


@pytest.mark.parametrize("kind", ["go2_hist", "gait"])
def test_same_minibatches_cpu(oracle_backend, kind):
    _check_same_minibatches("cpu", kind, 70)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["go2_hist", "gait"])
def test_same_minibatches_hip(hip_backend, kind):
    _check_same_minibatches("cuda", kind, 1000)


# ---- 3. refusals and defaults -------------------------------------------------------------------------------------------------------
def test_refusals_and_defaults(oracle_backend):
    from genesis_forge_amd.learner import RolloutStorage

    env = _env("gait", 20, output="ring")
    with pytest.raises(ValueError, match="ring"):
        RolloutStorage(env, 4, obs_groups=GAIT_GROUPS, history="frames")
    with pytest.raises(ValueError, match="history"):
        RolloutStorage(env, 4, history="slots")
    # a manager without a history keeps its rows; with no history anywhere "frames" is "rows"
    env = _env("go2", 20)
    st = RolloutStorage(env, 4, history="frames")
    assert st.frames == {} and st.observations is not None and st.group_rows == {"policy": st.observations} and not st._frame_parts
    # exactly the frame-stored names in `frames`, exactly the others in `group_rows`
    env = _env("gait", 20, output="window")
    st = RolloutStorage(env, 4, obs_groups=GAIT_GROUPS, history="frames")
    hist = {m.name for m in env.managers["observation"] if m._history_len > 1}
    assert hist == {"policy", "critic"} and set(st.frames) == hist and set(st.group_rows) == set()
    st = RolloutStorage(env, 4, obs_groups={"policy": ["policy"]}, history="frames")
    assert set(st.frames) == {"policy"} and st.group_rows == {} and st.observations is None
    with pytest.raises(ValueError, match="extras"):
        RolloutStorage(env, 4, obs_groups=GAIT_GROUPS, history="frames").begin(env.reset()[0])
    with pytest.raises(ValueError):
        st.observation_rows("critic")
    with pytest.raises(ValueError):
        st.observation_rows("policy", 5)
    # a manager switched to the slot-ordered ring after the storage was made is refused at the step that would store its frame
    env = _env("go2_hist", 20)
    st = RolloutStorage(env, 4, history="frames").attach()
    st.begin(*env.reset())
    env.step(torch.zeros(20, 12))
    env.observation_manager.output = "ring"
    with pytest.raises(ValueError, match="ring"):
        env.step(torch.zeros(20, 12))
    env = _env("gait", 20)
    st = RolloutStorage(env, 4, obs_groups=GAIT_GROUPS)
    assert st.history == "rows" and st.frames == {} and set(st.group_rows) == {"policy", "critic"}
    obs, extras = env.reset()
    st.begin(obs, extras)
    assert torch.equal(st.observation_rows("critic", 0), extras["observations"]["critic"]) and st.observation_rows().shape == st.observations.shape


# ---- 4. gf_minibatch_gather history fields, raw ABI ---------------------------------------------------------------------------------
def _ints(shape, g, dev):
    return torch.randint(-99, 100, shape, generator=g).to(torch.float32).to(dev)


def _rows_of(frames, idx, H, N, valid):
    """torch indexing of the flattened frames [(T+H)·N, O]: row i is frames idx + (H-1-j)·N, j = 0 … H-1 side by side; NaN where invalid."""
    safe = torch.where(valid, idx, torch.zeros_like(idx))
    out = torch.cat([frames[safe + (H - 1 - j) * N] for j in range(H)], dim=-1)
    out[~valid] = float("nan")
    return out


def _same(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


@pytest.mark.gpu
@pytest.mark.parametrize("N", [37, 64])
@pytest.mark.parametrize("H", [1, 2, 5])
@pytest.mark.parametrize("O", [1, 2, 4, 16, 45, 78])
def test_gather_history_fields_hip(hip_backend, O, H, N):
    from genesis_forge_amd import _native as nat

    dev, T = "cuda", 3
    g = torch.Generator().manual_seed(O * 100 + H * 10 + N)
    src_rows = T * N
    OB, HB, WP = 16, 3, 5   # the second history field and the plain one
    fa, fb = _ints(((T + H) * N, O), g, dev), _ints(((T + HB) * N, OB), g, dev)
    plain = _ints((src_rows, WP), g, dev)
    mean, std = _ints((H * O,), g, dev), (torch.rand(H * O, generator=g) + 0.5).to(dev)
    for m in (1, 17, 300):
        idx = torch.randint(0, src_rows, (m,), generator=g).to(dev)
        if m >= 17:
            idx[3], idx[m - 1], idx[7] = -1, src_rows, src_rows - 1
        valid = (idx >= 0) & (idx < src_rows)
        # an aligned destination (column 4, a width that is a multiple of 4) lets the field move in the widest chunks its source allows:
        # 16 bytes for O in {4, 16} (O = 4: one chunk per frame), 8 for O in {2, 78}, 4 for O in {1, 45}; column 3 forces 4-byte chunks
        for normed, col_a in ((False, 4), (True, 4), (False, 3)) if m == 300 else ((False, 4), (False, 3)) if m == 17 else ((False, 4),):
            col_b = 4
            wa = col_a + H * O + 2 if col_a == 3 else col_a + H * O + 4 + (-(H * O)) % 4
            da = torch.full((m, wa), -3.0, device=dev)
            db = torch.full((m, col_b + HB * OB + 4), -3.0, device=dev)
            dp = torch.full((m, WP), -3.0, device=dev)
            a = nat.GfMinibatchArgs()
            a.num_rows, a.num_src_rows, a.indices, a.num_fields = m, src_rows, idx.data_ptr(), 3
            for f, (s, d, w, col, h) in zip(a.fields, ((fa, da, O, col_a, H), (plain, dp, WP, 0, 0), (fb, db, OB, col_b, HB))):
                f.src, f.dst, f.src_width, f.dst_width, f.dst_col, f.history_len, f.frame_stride_rows = s.data_ptr(), d.data_ptr(), w, d.shape[1], col, h, N
            if normed:
                a.fields[0].mean, a.fields[0].std, a.fields[0].eps = mean.data_ptr(), std.data_ptr(), 0.01
            hip_backend.minibatch_gather(a)
            want_a = _rows_of(fa, idx, H, N, valid)
            if normed:
                want_a = (want_a - mean) / (std + 0.01)
            assert _same(da[:, col_a:col_a + H * O], want_a), f"history field O={O} H={H} N={N} rows={m} normed={normed}"
            assert _same(db[:, col_b:col_b + HB * OB], _rows_of(fb, idx, HB, N, valid))
            assert _same(dp, _rows_of(plain, idx, 1, N, valid))
            assert bool(torch.isnan(da[~valid][:, col_a:col_a + H * O]).all()) and bool(torch.isnan(db[~valid][:, col_b:col_b + HB * OB]).all())
            for d, lo, hi in ((da, col_a, col_a + H * O), (db, col_b, col_b + HB * OB)):   # the columns around a field are not touched
                assert bool((d[:, :lo] == -3).all()) and bool((d[:, hi:] == -3).all())
        if H == 1:   # the same field alone: the plain kernel (history_len 0 and 1 are the plain field)
            for h, col in ((0, 4), (1, 4), (1, 3)):
                wa = col + O + (-(col + O)) % 4
                da = torch.full((m, wa), -3.0, device=dev)
                a = nat.GfMinibatchArgs()
                a.num_rows, a.num_src_rows, a.indices, a.num_fields = m, src_rows, idx.data_ptr(), 1
                f = a.fields[0]
                f.src, f.dst, f.src_width, f.dst_width, f.dst_col, f.history_len, f.frame_stride_rows = fa.data_ptr(), da.data_ptr(), O, wa, col, h, 0
                hip_backend.minibatch_gather(a)
                assert _same(da[:, col:col + O], _rows_of(fa, idx, 1, N, valid))
                assert bool((da[:, :col] == -3).all()) and bool((da[:, col + O:] == -3).all())


def test_gather_history_refusals():
    """Every refusal returns its code before anything is launched (no device is touched: the pointers are never dereferenced)."""
    from genesis_forge_amd import _native as nat

    lib = C.CDLL(nat.lib_path())
    lib.gf_sizeof.argtypes, lib.gf_sizeof.restype = [C.c_int], C.c_int
    assert lib.gf_sizeof(nat.GF_SIZEOF_MINIBATCH) == C.sizeof(nat.GfMinibatchArgs) and C.sizeof(nat.GfMinibatchField) == 56
    lib.gf_minibatch_gather.argtypes, lib.gf_minibatch_gather.restype = [C.POINTER(nat.GfMinibatchArgs), C.c_void_p], C.c_int
    PTR = 0x1000

    def args(**kw):
        a = nat.GfMinibatchArgs()
        a.num_rows, a.num_src_rows, a.indices, a.num_fields = 0, 100, PTR, 1   # (num_rows 0: a call that passes is a no-op)
        f = a.fields[0]
        f.src, f.dst, f.src_width, f.dst_width, f.dst_col, f.history_len, f.frame_stride_rows = PTR, PTR, 6, 33, 3, 5, 10
        for k, v in kw.items():
            setattr(f, k, v)
        return a

    assert lib.gf_minibatch_gather(C.byref(args()), None) == 0
    assert lib.gf_minibatch_gather(C.byref(args(history_len=-1)), None) == E_RANGE
    assert lib.gf_minibatch_gather(C.byref(args(frame_stride_rows=0)), None) == E_RANGE
    assert lib.gf_minibatch_gather(C.byref(args(frame_stride_rows=-4)), None) == E_RANGE
    assert lib.gf_minibatch_gather(C.byref(args(dst_width=32)), None) == E_RANGE      # dst_col + H·O = 33
    assert lib.gf_minibatch_gather(C.byref(args(history_len=6)), None) == E_RANGE
    assert lib.gf_minibatch_gather(C.byref(args(history_len=1, frame_stride_rows=0, dst_width=9)), None) == 0   # a plain field never reads the stride
    assert lib.gf_minibatch_gather(C.byref(args(history_len=0, frame_stride_rows=0, dst_width=9)), None) == 0
    assert lib.gf_minibatch_gather(C.byref(args(history_len=0, dst_width=8)), None) == E_RANGE
    assert lib.gf_minibatch_gather(C.byref(args(src=None)), None) == E_NULL
    assert lib.gf_minibatch_gather(C.byref(args(dst=None)), None) == E_NULL
    assert lib.gf_minibatch_gather(C.byref(args(mean=PTR)), None) == E_NULL           # mean without std


# ---- 5. gf_rollout_frame_write, raw ABI ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nseg", [1, 4])
@pytest.mark.parametrize("n", [1, 1000])
def test_frame_write_hip(hip_backend, n, nseg):
    from genesis_forge_amd import _native as nat

    dev = "cuda"
    g = torch.Generator().manual_seed(n + nseg)
    widths = (1, 2, 16, 78)
    for strides in (lambda w: w, lambda w: w + 3, lambda w: 5 * w):
        for lead in (0, 1, 2):   # the source starts 0, 4 and 8 bytes into its allocation
            for first in range(0, 4, nseg):
                a = nat.GfRolloutFrameArgs()
                a.num_envs, a.num_segs = n, nseg
                keep = []
                for seg, w in zip(a.segs, widths[first:first + nseg]):
                    s = strides(w)
                    buf = _ints((lead + n * s,), g, dev)
                    src = torch.as_strided(buf, (n, w), (s, 1), lead)
                    dst = torch.full((n + 2, w), -3.0, device=dev)   # (a guard row on either side)
                    seg.src, seg.dst, seg.width, seg.src_stride = src.data_ptr(), dst[1].data_ptr(), w, s
                    keep.append((src, dst))
                hip_backend.rollout_frame_write(a)
                for src, dst in keep:
                    assert torch.equal(dst[1:n + 1], src), f"width {src.shape[1]} stride {src.stride(0)} lead {lead} n {n} segs {nseg}"
                    assert bool((dst[0] == -3).all()) and bool((dst[n + 1] == -3).all()), "a store outside the frame"
    a.num_envs = 0   # a no-op: nothing is launched, nothing is written
    before = [d.clone() for _, d in keep]
    for seg in a.segs:
        seg.src = 0x1000
    hip_backend.rollout_frame_write(a)
    torch.cuda.synchronize()
    assert all(torch.equal(x, d) for x, (_, d) in zip(before, keep))


def test_frame_write_refusals():
    from genesis_forge_amd import _native as nat

    lib = C.CDLL(nat.lib_path())
    lib.gf_sizeof.argtypes, lib.gf_sizeof.restype = [C.c_int], C.c_int
    assert nat.GF_SIZEOF_ROLLOUT_FRAME == 30 and lib.gf_sizeof(30) == C.sizeof(nat.GfRolloutFrameArgs) == 16 + 4 * 24
    assert nat.GF_ROLLOUT_FRAME_MAX == 4
    lib.gf_abi_version.restype = C.c_int
    assert lib.gf_abi_version() == nat.GF_ABI_VERSION
    assert "rollout_frame_write" not in nat.PHASE_FUNCS and nat.GfRolloutFrameArgs not in nat.ABI_STRUCTS
    lib.gf_rollout_frame_write.argtypes, lib.gf_rollout_frame_write.restype = [C.POINTER(nat.GfRolloutFrameArgs), C.c_void_p], C.c_int
    PTR = 0x1000

    def args(num_envs=0, num_segs=2, **kw):
        a = nat.GfRolloutFrameArgs()
        a.num_envs, a.num_segs = num_envs, num_segs   # (num_envs 0: a call that passes is a no-op)
        for seg in a.segs:
            seg.src, seg.dst, seg.width, seg.src_stride = PTR, PTR, 16, 80
        for k, v in kw.items():
            setattr(a.segs[1], k, v)
        return a

    assert lib.gf_rollout_frame_write(C.byref(args()), None) == 0
    assert lib.gf_rollout_frame_write(None, None) == E_NULL
    assert lib.gf_rollout_frame_write(C.byref(args(src=None)), None) == E_NULL
    assert lib.gf_rollout_frame_write(C.byref(args(dst=None)), None) == E_NULL
    assert lib.gf_rollout_frame_write(C.byref(args(num_envs=-1)), None) == E_RANGE
    assert lib.gf_rollout_frame_write(C.byref(args(num_segs=0)), None) == E_RANGE
    assert lib.gf_rollout_frame_write(C.byref(args(num_segs=5)), None) == E_RANGE
    assert lib.gf_rollout_frame_write(C.byref(args(width=0)), None) == E_RANGE
    assert lib.gf_rollout_frame_write(C.byref(args(src_stride=15)), None) == E_RANGE
    assert lib.gf_rollout_frame_write(C.byref(args(src_stride=16)), None) == 0
    a = args(num_segs=1, src=None, width=0)   # (only the first num_segs segments are read)
    assert lib.gf_rollout_frame_write(C.byref(a), None) == 0


# ---- 7. one collection and update ---------------------------------------------------------------------------------------------------
ALGO = dict(clip_param=0.2, desired_kl=0.01, entropy_coef=0.01, gamma=0.99, lam=0.95, learning_rate=0.001, max_grad_norm=1.0,
            num_learning_epochs=2, num_mini_batches=4, schedule="adaptive", use_clipped_value_loss=True, value_loss_coef=1.0)


def _collect_and_update(dev, n, T, history, output, noise_gen=None):
    from genesis_forge_amd.learner import PPO, ActorCriticMLP, EpisodeStatistics, PolicyForward, RolloutStorage

    env = _env("gait", n, output=output)
    obs, extras = env.reset()
    st = RolloutStorage(env, T, obs_groups=GAIT_GROUPS, history=history).attach()
    st.begin(obs, extras)
    st.seed(5)
    A = env.action_space.shape[0]
    wp, wc = (sum(m.observation_space.shape[0] for m in env.managers["observation"] if m.name in st.obs_groups[k]) for k in ("policy", "critic"))
    torch.manual_seed(0)
    policy = ActorCriticMLP(wp, A, (64, 32), (64, 32), init_noise_std=0.8, num_critic_obs=wc,
                            actor_obs_normalization=True, critic_obs_normalization=True).to(dev)
    fwd, ppo, stats = PolicyForward(policy), PPO(policy, st, **ALGO), EpisodeStatistics(n)
    cobs_of = lambda extras: tuple(extras["observations"][m] for m in st.obs_groups["critic"])
    for _ in range(T):
        noise = None if noise_gen is None else torch.randn(n, A, generator=noise_gen).to(dev)
        actions = st.act_policy(fwd, obs, critic_obs=cobs_of(extras), noise=noise)
        obs, _r, _te, trunc, extras = env.step(actions)
        if output == "window":
            assert not obs.is_contiguous(), "the learner is handed the window view itself"
        policy.update_normalization(obs, cobs_of(extras))
        st.process_env_step(trunc, gamma=ppo.gamma, episodes=stats)
    ppo.compute_returns(torch.cat(cobs_of(extras), dim=-1))
    losses = ppo.update(generator=torch.Generator(device=dev).manual_seed(3))
    assert all(v == v and abs(v) != float("inf") for v in losses.values()), losses
    flat = torch.cat([p.detach().reshape(-1) for p in policy.parameters()])
    assert bool(torch.isfinite(flat).all())
    norms = torch.cat([b.reshape(-1).to(torch.float32) for b in policy.buffers()])
    return flat, norms, losses, env


def _check_collect_and_update(dev, n, T, noise_seed=None):
    gen = lambda: None if noise_seed is None else torch.Generator().manual_seed(noise_seed)
    rows = _collect_and_update(dev, n, T, "rows", "fresh", gen())
    frames = _collect_and_update(dev, n, T, "frames", "window", gen())
    assert frames[3]._trace is not None, "the window-mode env with a frame-stored rollout runs as a recorded step"
    # two runs of one form are compared bit for bit (tests/test_ppo_update.py::test_update_is_bitwise_deterministic): so are the two forms
    assert torch.equal(rows[1], frames[1]), "the normalisers' statistics differ"
    assert torch.equal(rows[0], frames[0]), "the parameters after the update differ from the row-stored twin's"
    assert rows[2] == frames[2]


def test_collect_and_update_cpu(oracle_backend):
    _check_collect_and_update("cpu", 70, 6, noise_seed=4)


@pytest.mark.gpu
def test_collect_and_update_hip(hip_backend):
    _check_collect_and_update("cuda", 256, 6)
