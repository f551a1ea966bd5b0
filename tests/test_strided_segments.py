"""Row-strided input segments of ``gf_mlp_act`` and ``gf_obs_norm_update`` (``GfMlpSegment.row_stride``): rows ``row_stride`` floats apart
give the bits of their ``.contiguous()`` copy, and the learner's entry points take the strided view an ``output="window"``
ObservationManager hands out as it is — and still no other strided tensor."""
import ctypes as C

import pytest
import torch

E_NULL, E_RANGE = -1, -2


def _policy(in_w, critic_w, hidden, A, dev, norm=False, seed=0):
    from genesis_forge_amd.learner import ActorCriticMLP

    torch.manual_seed(seed)
    return ActorCriticMLP(in_w, A, hidden, hidden, init_noise_std=0.7, num_critic_obs=critic_w,
                          actor_obs_normalization=norm, critic_obs_normalization=norm).to(dev)


def _strided(x, stride, lead=0):
    """The rows of ``x`` ``stride`` floats apart inside a larger allocation (the gaps hold other numbers)."""
    n, w = x.shape
    buf = torch.full((lead + n * stride,), 1.0e6, device=x.device)
    v = torch.as_strided(buf, (n, w), (stride, 1), lead)
    v.copy_(x)
    assert not v.is_contiguous() or n == 1 or stride == w
    return v


def _mlp_raw(backend, fwd, n, parts, cparts, strides, cstrides, std, noise):
    """gf_mlp_act through the binding into fresh outputs: mean, values, actions and the five storage rows."""
    A, dev = fwd.num_actions, parts[0].device
    a = fwd._fill(n, tuple(p.contiguous() for p in parts), tuple(p.contiguous() for p in cparts))   # (the descriptor's shape)
    for net, ps, ss in ((a.actor, parts, strides), (a.critic, cparts, cstrides)):
        for seg, p, s in zip(net.inputs, ps, ss):
            seg.rows, seg.width, seg.row_stride = p.data_ptr(), p.shape[1], s
    new = lambda *s: torch.full(s, 7.0, device=dev)
    o = {k: new(n, A) for k in ("mean", "actions", "actions_out", "mu_out", "sigma_out")}
    o.update({k: new(n) for k in ("values", "values_out", "log_prob_out")})
    for k, t in o.items():
        setattr(a, k, t.data_ptr())
    a.std, a.noise, a.std_per_env = std.data_ptr(), noise.data_ptr(), 0
    a.seed, a.stream, a.env_offset = 1, 0, 0
    backend.mlp_act(a)
    torch.cuda.synchronize()
    return o


@pytest.mark.gpu
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("segs", [(48,), (20, 28)])
def test_mlp_act_strided_rows_hip(hip_backend, segs, norm):
    """Actor + critic, 48 -> 64 -> 12 / 1: every output and every storage row from strided rows equals the contiguous call's."""
    from genesis_forge_amd.learner import PolicyForward

    dev, n, A = "cuda", 1000, 12
    policy = _policy(48, 48, (64,), A, dev, norm)
    if norm:
        g = torch.Generator().manual_seed(3)
        for m in (policy.actor_obs_normalizer, policy.critic_obs_normalizer):
            m._mean.copy_(torch.randn(1, 48, generator=g) * 0.2)
            m._std.copy_(torch.rand(1, 48, generator=g) + 0.5)
    fwd = PolicyForward(policy)
    g = torch.Generator().manual_seed(7)
    parts = tuple(torch.randn(n, w, generator=g).to(dev) for w in segs)
    cparts = tuple(torch.randn(n, w, generator=g).to(dev) for w in segs)
    std, noise = policy.std.detach(), torch.randn(n, A, generator=g).to(dev)
    want = _mlp_raw(hip_backend, fwd, n, parts, cparts, [0] * len(segs), [0] * len(segs), std, noise)
    assert not any(bool((t == 7.0).all()) for t in want.values())
    explicit = _mlp_raw(hip_backend, fwd, n, parts, cparts, list(segs), list(segs), std, noise)   # row_stride == width is 0's meaning
    for k in want:
        assert torch.equal(explicit[k], want[k]), k
    for mult in (lambda w: w + 3, lambda w: 4 * w):
        sp = tuple(_strided(p, mult(p.shape[1]), lead=i) for i, p in enumerate(parts))
        sc = tuple(_strided(p, mult(p.shape[1])) for p in cparts)
        got = _mlp_raw(hip_backend, fwd, n, sp, sc, [p.stride(0) for p in sp], [p.stride(0) for p in sc], std, noise)
        for k in want:
            assert torch.equal(got[k], want[k]), f"{k} from rows {[p.stride(0) for p in sp]} floats apart differs from the contiguous rows'"


@pytest.mark.gpu
@pytest.mark.parametrize("segs", [(48,), (20, 28), (300,)])
def test_obs_norm_strided_rows_hip(hip_backend, segs):
    from genesis_forge_amd.learner import EmpiricalNormalization

    dev, n, W = "cuda", 1000, sum(segs)
    g = torch.Generator().manual_seed(5)
    parts = tuple((torch.randn(n, w, generator=g) * 2 + 1).to(dev) for w in segs)

    def run(ps, strides):
        norm = EmpiricalNormalization(W).to(dev)
        a = norm._scratch.args
        a.num_rows, a.num_sets = n, 1
        norm._fill(a.sets[0], tuple(p.contiguous() for p in ps))
        for seg, p, s in zip(a.sets[0].inputs, ps, strides):
            seg.rows, seg.width, seg.row_stride = p.data_ptr(), p.shape[1], s
        hip_backend.obs_norm_update(a)
        hip_backend.obs_norm_update(a)   # (a second batch: the update from a non-trivial state)
        torch.cuda.synchronize()
        return norm._mean.clone(), norm._var.clone(), norm._std.clone(), norm.count.clone()

    want = run(parts, [0] * len(segs))
    assert int(want[3]) == 2 * n and not torch.equal(want[0], torch.zeros_like(want[0]))
    for mult in (lambda w: w, lambda w: w + 3, lambda w: 4 * w):
        sp = tuple(_strided(p, mult(p.shape[1]), lead=i) for i, p in enumerate(parts))
        got = run(sp, [p.stride(0) if n > 1 else mult(p.shape[1]) for p in sp])
        for name, x, y in zip(("mean", "var", "std", "count"), got, want):
            assert torch.equal(x, y), f"{name} from strided rows differs from the contiguous rows'"


def test_row_stride_refusals():
    """A non-zero row_stride smaller than the width is refused before anything is launched, by both entry points."""
    from genesis_forge_amd import _native as nat

    lib = C.CDLL(nat.lib_path())
    lib.gf_sizeof.argtypes, lib.gf_sizeof.restype = [C.c_int], C.c_int
    assert C.sizeof(nat.GfMlpSegment) == 16
    assert lib.gf_sizeof(nat.GF_SIZEOF_MLP_ACT) == C.sizeof(nat.GfMlpActArgs) and lib.gf_sizeof(nat.GF_SIZEOF_OBS_NORM) == C.sizeof(nat.GfObsNormArgs)
    lib.gf_mlp_act.argtypes, lib.gf_mlp_act.restype = [C.POINTER(nat.GfMlpActArgs), C.c_void_p], C.c_int
    lib.gf_obs_norm_update.argtypes, lib.gf_obs_norm_update.restype = [C.POINTER(nat.GfObsNormArgs), C.c_void_p], C.c_int
    PTR = 0x1000

    def mlp(stride):
        a = nat.GfMlpActArgs()
        a.num_envs = 0   # (a call that passes is a no-op)
        a.actor.num_layers, a.actor.num_inputs = 1, 2
        for seg in a.actor.inputs[:2]:
            seg.rows, seg.width = PTR, 24
        a.actor.inputs[1].row_stride = stride
        a.actor.layers[0].weight, a.actor.layers[0].bias, a.actor.layers[0].out_width = PTR, PTR, 12
        a.mean = PTR
        return a

    assert lib.gf_mlp_act(C.byref(mlp(0)), None) == 0
    assert lib.gf_mlp_act(C.byref(mlp(24)), None) == 0 and lib.gf_mlp_act(C.byref(mlp(240)), None) == 0
    assert lib.gf_mlp_act(C.byref(mlp(23)), None) == E_RANGE
    assert lib.gf_mlp_act(C.byref(mlp(-24)), None) == E_RANGE

    def norm(stride):
        a = nat.GfObsNormArgs()
        a.num_rows, a.num_sets = 0, 1
        st = a.sets[0]
        st.num_inputs = 2
        for seg in st.inputs[:2]:
            seg.rows, seg.width = PTR, 24
        st.inputs[1].row_stride = stride
        st.mean = st.var = st.std = st.count = st.workspace = PTR
        st.until, st.workspace_bytes = -1, 1 << 20
        return a

    assert lib.gf_obs_norm_update(C.byref(norm(0)), None) == 0
    assert lib.gf_obs_norm_update(C.byref(norm(24)), None) == 0 and lib.gf_obs_norm_update(C.byref(norm(100)), None) == 0
    assert lib.gf_obs_norm_update(C.byref(norm(23)), None) == E_RANGE
    assert lib.gf_obs_norm_update(C.byref(norm(-1)), None) == E_RANGE


def _window_env(n):
    from genesis_forge_amd import tasks
    from genesis_forge_amd.managers import ObservationManager

    old, ObservationManager.default_output = ObservationManager.default_output, "window"
    try:
        env = tasks.Go2CommandDirectionEnv(num_envs=n, max_episode_length_s=0.4, cmd_resample_s=0.2, history=3, contacts=True, obs_noise=True,
                                           scene_kwargs=dict(ang_noise=0.3, seed=3))
        env.build()
    finally:
        ObservationManager.default_output = old
    env.seed(7)
    return env


def _check_window_view(dev, n):
    from genesis_forge_amd.learner import EmpiricalNormalization, PolicyForward

    env = _window_env(n)
    env.reset()
    g = torch.Generator().manual_seed(2)
    for _ in range(4):
        view, *_ = env.step(torch.randn(n, 12, generator=g).to(dev))
    W = view.shape[1]
    assert not view.is_contiguous() and view.stride(1) == 1 and view.stride(0) > W
    policy = _policy(W, W, (64, 32), 12, dev, norm=True)
    fwd = PolicyForward(policy)
    flat = view.contiguous()
    assert torch.equal(fwd.mean(view), fwd.mean(flat))          # (at the parent commit: ValueError — the view is not contiguous)
    assert torch.equal(fwd.value(view), fwd.value(flat))
    a, b = EmpiricalNormalization(W).to(dev), EmpiricalNormalization(W).to(dev)
    a.update(view)
    b.update(flat)
    for x, y in zip(a.buffers(), b.buffers()):
        assert torch.equal(x, y)
    twin = _policy(W, W, (64, 32), 12, dev, norm=True)
    policy.update_normalization(view)
    twin.update_normalization(flat)
    for x, y in zip(policy.buffers(), twin.buffers()):
        assert torch.equal(x, y)
    # what was refused stays refused: a strided tensor that is not a manager's window, a window cut up by the caller
    other = torch.zeros(n, 2 * W, device=dev)[:, :W]
    for bad in (other, view[:, :W - 1], view[:, 1:], torch.zeros(n, 2 * W, device=dev)[:, ::2]):
        with pytest.raises(ValueError):
            fwd.mean(bad)
    with pytest.raises(ValueError, match="strided view"):
        a.update(other)
    with pytest.raises(ValueError):
        policy.update_normalization(other)


def test_window_view_is_read_in_place_cpu(oracle_backend):
    _check_window_view("cpu", 70)


@pytest.mark.gpu
def test_window_view_is_read_in_place_hip(hip_backend):
    _check_window_view("cuda", 1000)
