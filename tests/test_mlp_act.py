"""gf_mlp_act — the actor and critic MLP forward of a collection step and gf_policy_act's sampling in ONE launch on the f32 matrix
cores — with its way up: ``learner.PolicyForward`` and ``RolloutStorage.act_policy``.

* CPU: the ABI size and every refusal through the raw entry point (they return before any launch), the oracle backend's path
  (bit-identical to ``act`` on torch's forward), ``PolicyForward`` / ``act_policy`` input refusals;
* GPU: the layout pinned without a tolerance (integer-valued data: every summation order gives the same f32), accuracy against the
  float64 module with torch's own f32 forward as the yardstick (``e_hip <= 4 e_torch + 1e-7 max|ref|``), the sampling half relative
  to the kernel's own mean, row independence and determinism, the storage rows, live weights across ``PPO.update``."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from test_policy_act import _assert_fold, _go2, _np_normals
from test_policy_act import _raw as _raw_policy_act

SHAPES = [   # (input segments, hidden widths, A)
    ((48,), (512, 256, 128), 12),
    ((45,), (512, 256, 128), 12),
    ((37,), (64,), 1),
    ((310,), (300, 37), 28),
    ((48,), (), 37),
]
CRITIC_ONLY = ((250, 60), (512, 256, 128), 12)
SIZES = [1000, 4133]


def _policy(segs, hidden, A, dev, seed=0, scale=1.0, critic_segs=None):
    from genesis_forge_amd.learner import ActorCriticMLP

    torch.manual_seed(seed)
    policy = ActorCriticMLP(sum(segs), A, hidden, hidden, init_noise_std=0.7)
    if critic_segs is not None:
        policy.critic = ActorCriticMLP(sum(critic_segs), A, hidden, hidden).critic
    if scale != 1.0:
        with torch.no_grad():
            for p in list(policy.actor.parameters()) + list(policy.critic.parameters()):
                p.mul_(scale)
    return policy.to(dev)


def _obs(segs, n, dev, seed=1, scale=1.0):
    g = torch.Generator().manual_seed(seed * 7919 + n + sum(segs))
    return tuple((torch.randn(n, w, generator=g) * scale).to(dev) for w in segs)


def _one(parts):
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=-1)


def _raw(backend, fwd, n, obs=None, cobs=None, std=None, noise=None, seed=1, stream=0, env_offset=0, sample=True, rows=True):
    """gf_mlp_act through the binding into fresh outputs: dict of mean, values, actions and the five storage rows."""
    A = fwd.num_actions
    dev = (obs or cobs)[0].device
    o = {}
    a = fwd._fill(n, obs, cobs)
    a.std = a.noise = a.mean = a.values = a.actions = a.actions_out = a.mu_out = a.sigma_out = a.values_out = a.log_prob_out = None
    a.seed, a.stream, a.env_offset, a.std_per_env = seed, stream, env_offset, 0
    new = lambda *s: torch.full(s, 7.0, device=dev)
    if obs is not None:
        o["mean"] = new(n, A)
        a.mean = o["mean"].data_ptr()
        if sample:
            o["actions"] = new(n, A)
            a.actions, a.std = o["actions"].data_ptr(), std.data_ptr()
            a.noise = None if noise is None else noise.data_ptr()
            if rows:
                for k in ("actions_out", "mu_out", "sigma_out"):
                    o[k] = new(n, A)
                    setattr(a, k, o[k].data_ptr())
                o["log_prob_out"] = new(n)
                a.log_prob_out = o["log_prob_out"].data_ptr()
    if cobs is not None:
        o["values"] = new(n)
        a.values = o["values"].data_ptr()
        if rows:
            o["values_out"] = new(n)
            a.values_out = o["values_out"].data_ptr()
    backend.mlp_act(a)
    torch.cuda.synchronize()
    return o


# ---- CPU: ABI, refusals -------------------------------------------------------------------------------------------------------------
def test_abi_size_and_raw_refusals():
    from genesis_forge_amd import _native as nat

    lib = C.CDLL(nat.lib_path())
    lib.gf_sizeof.argtypes, lib.gf_sizeof.restype = [C.c_int], C.c_int
    assert lib.gf_sizeof(nat.GF_SIZEOF_MLP_ACT) == C.sizeof(nat.GfMlpActArgs)
    lib.gf_mlp_act.argtypes, lib.gf_mlp_act.restype = [C.POINTER(nat.GfMlpActArgs), C.c_void_p], C.c_int
    assert (nat.GF_MLP_MAX_LAYERS, nat.GF_MLP_MAX_INPUTS, nat.GF_MLP_MAX_HIDDEN, nat.GF_MLP_MAX_INPUT_WIDTH, nat.GF_MLP_MAX_ACTIONS) == (6, 4, 512, 1024, 64)
    E_NULL, E_RANGE, E_UNSUPPORTED = -1, -2, -5
    PTR = 0x1000   # never dereferenced: every call below returns before a launch

    def net(inputs, widths):
        m = nat.GfMlpNet()
        m.num_layers, m.num_inputs = len(widths), len(inputs)
        for seg, w in zip(m.inputs, inputs):
            seg.rows, seg.width = PTR, w
        for lay, w in zip(m.layers, widths):
            lay.weight, lay.bias, lay.out_width = PTR, PTR, w
        return m

    def args(actor=((48,), (512, 256, 128, 12)), critic=((48,), (512, 256, 128, 1)), **kw):
        a = nat.GfMlpActArgs()
        a.num_envs = 0   # (a valid descriptor then returns GF_OK without a launch)
        if actor is not None:
            a.actor = net(*actor) if isinstance(actor, tuple) else actor
            a.std, a.actions, a.mean = PTR, PTR, PTR
        if critic is not None:
            a.critic = net(*critic) if isinstance(critic, tuple) else critic
            a.values = PTR
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    call = lambda a: lib.gf_mlp_act(C.byref(a), None)
    assert lib.gf_mlp_act(None, None) == E_NULL
    assert call(args()) == 0, "num_envs == 0 is a no-op"
    assert call(args(critic=None)) == 0 and call(args(actor=None)) == 0, "either net may be absent"
    assert call(args(actor=None, critic=None)) == E_UNSUPPORTED
    broken = net((48,), (64, 12))
    broken.layers[1].weight = None
    assert call(args(actor=broken)) == E_NULL
    broken = net((48,), (64, 12))
    broken.inputs[0].rows = None
    assert call(args(actor=broken)) == E_NULL
    assert call(args(actor=((48,), (513, 12)))) == E_RANGE and call(args(actor=((48,), (512, 12)))) == 0
    assert call(args(actor=((1000, 25), (64, 12)))) == E_RANGE and call(args(actor=((1000, 24), (64, 12)))) == 0
    five = net((8, 8, 8, 8), (64, 12))
    five.num_inputs = 5
    assert call(args(actor=five)) == E_RANGE
    seven = net((48,), (64,) * 5 + (12,))
    assert call(args(actor=seven)) == 0
    seven.num_layers = 7
    assert call(args(actor=seven)) == E_RANGE
    assert call(args(actor=((48,), (64, 65)))) == E_RANGE and call(args(actor=((48,), (64, 64)))) == 0
    assert call(args(critic=((48,), (64, 2)))) == E_UNSUPPORTED
    assert call(args(std=None)) == E_NULL, "actions need a std"
    assert call(args(std=None, actions=None)) == 0, "mean only draws nothing"
    assert call(args(critic=None, values_out=PTR)) == E_NULL and call(args(critic=None, values=PTR)) == E_NULL
    assert call(args(actor=None, mean=PTR)) == E_NULL
    assert call(args(num_envs=-1)) == E_RANGE and call(args(std_per_env=2)) == E_RANGE


# ---- CPU: the oracle backend is today's path ------------------------------------------------------------------------------------------
def _twin_storages(n, T, groups=None):
    from genesis_forge_amd.learner import RolloutStorage

    out = []
    for _ in range(2):
        env = _go2(n, trace=False)
        obs, extras = env.reset()
        st = RolloutStorage(env, T, obs_groups=groups).attach()
        st.begin(obs, extras)
        out.append((env, st, obs))
    return out


def test_oracle_act_policy_is_act_on_the_torch_forward(oracle_backend):
    from genesis_forge_amd.learner import PolicyForward

    n, A = 70, 12
    (env, st, obs), (_env2, st2, obs2) = _twin_storages(n, 3)
    policy = _policy((st.obs_width,), (64, 32), A, "cpu")
    fwd = PolicyForward(policy)
    z = torch.randn(n, A, generator=torch.Generator().manual_seed(3))
    with pytest.raises(RuntimeError, match="noise"):
        st.act_policy(fwd, obs)
    st._act_stream = 0
    actions = st.act_policy(fwd, obs, noise=z)
    with torch.no_grad():
        want = st2.act(policy.act_mean(obs2), policy.std.detach(), policy.evaluate(obs2), noise=z)
    assert torch.equal(actions, want)
    for k in ("actions", "mu", "sigma", "values", "actions_log_prob"):
        assert torch.equal(getattr(st, k), getattr(st2, k)), k
    assert st._act_stream == st2._act_stream == 1 and st._pol_serial == st2._pol_serial
    # two critic segments are their concatenation
    wide = _policy((st.obs_width,), (64, 32), A, "cpu", critic_segs=(st.obs_width, 9))
    fwd = PolicyForward(wide)
    extra = torch.randn(n, 9, generator=torch.Generator().manual_seed(4))
    a1 = st.act_policy(fwd, obs, critic_obs=(obs, extra), noise=z)
    with torch.no_grad():
        a2 = st2.act(wide.act_mean(obs2), wide.std.detach(), wide.evaluate(torch.cat([obs2, extra], dim=-1)), noise=z)
    assert torch.equal(a1, a2)
    for k in ("actions", "mu", "sigma", "values", "actions_log_prob"):
        assert torch.equal(getattr(st, k), getattr(st2, k)), k
    assert torch.equal(fwd.mean(obs), wide.act_mean(obs)) and torch.equal(fwd.value((obs, extra)), wide.evaluate(torch.cat([obs, extra], dim=-1)))


# ---- CPU / GPU: refusals of the public interface --------------------------------------------------------------------------------------
def test_policy_forward_refuses_what_the_kernel_cannot_run():
    from genesis_forge_amd.learner import ActorCriticMLP, PolicyForward

    nn = torch.nn
    ok = ActorCriticMLP(48, 12, (64, 32), (64, 32))
    PolicyForward(ok)
    bad = copy.deepcopy(ok)
    bad.actor[1] = nn.Tanh()
    with pytest.raises(ValueError, match="Tanh"):
        PolicyForward(bad)
    bad = copy.deepcopy(ok)
    bad.actor[1] = nn.ELU(alpha=0.5)
    with pytest.raises(ValueError, match="alpha=0.5"):
        PolicyForward(bad)
    with pytest.raises(ValueError, match="float64"):
        PolicyForward(copy.deepcopy(ok).double())
    with pytest.raises(ValueError, match="1024"):
        PolicyForward(ActorCriticMLP(48, 12, (1024, 32), (64, 32)))
    bad = copy.deepcopy(ok)
    bad.critic[-1] = nn.Linear(32, 2)
    with pytest.raises(ValueError, match="2 outputs"):
        PolicyForward(bad)
    with pytest.raises(ValueError, match="65 outputs"):
        PolicyForward(ActorCriticMLP(48, 65, (64,), (64,)))
    with pytest.raises(ValueError, match="1025"):
        PolicyForward(ActorCriticMLP(1025, 12, (64,), (64,)))
    bad = copy.deepcopy(ok)
    bad.actor = nn.Sequential(*list(ok.actor) + [nn.ELU()])
    with pytest.raises(ValueError, match="activation"):
        PolicyForward(bad)
    bad = copy.deepcopy(ok)
    bad.actor[0].weight = nn.Parameter(torch.zeros(48, 64).T)
    with pytest.raises(ValueError, match="contiguous"):
        PolicyForward(bad)


def _check_act_policy_refusals(dev):
    from genesis_forge_amd.learner import PolicyForward, RolloutStorage

    n, A = 64, 12
    env = _go2(n, trace=False)
    obs, _ = env.reset()
    store = RolloutStorage(env, 4).attach()
    store.begin(obs)
    W = store.obs_width
    fwd = PolicyForward(_policy((W,), (64, 32), A, dev))
    wide = PolicyForward(_policy((W,), (64, 32), A, dev, critic_segs=(W, 9)))
    good, extra = torch.zeros(n, W, device=dev), torch.zeros(n, 9, device=dev)
    z = torch.zeros(n, A, device=dev)
    other = "cpu" if dev != "cpu" else "meta"
    bad = [
        good.double(), good[:, :W - 1], good[:-1], torch.zeros(n, 2 * W, device=dev)[:, ::2], torch.zeros(W, n, device=dev).T, good.to(other),
        good.reshape(-1), (good[:, :20], good[:, 20:]), (good[:, :20].contiguous(), good[:, 20:W - 1].contiguous()),
        (good,) * 5, (), "obs",
    ]
    for x in bad:
        with pytest.raises(ValueError):
            store.act_policy(fwd, x, noise=z)
    for c in (extra, (good, extra.double()), (good, extra[:-1]), (good, extra, extra), (good, torch.zeros(n, 18, device=dev)[:, ::2])):
        with pytest.raises(ValueError):
            store.act_policy(wide, good, critic_obs=c, noise=z)
    with pytest.raises(ValueError):
        store.act_policy(wide, good, noise=z)   # the critic reads obs: 48 columns are not the 57 its first layer reads
    for zz in (z.double(), torch.zeros(n, A + 1, device=dev)):
        with pytest.raises(ValueError):
            store.act_policy(fwd, good, noise=zz)
    with pytest.raises(ValueError):
        store.act_policy(fwd.policy, good, noise=z)
    assert store._act_stream == 0, "a refused call draws nothing"
    store.act_policy(fwd, good, noise=z)
    store.act_policy(wide, (good[:, :20].contiguous(), good[:, 20:].contiguous()), critic_obs=(good, extra), noise=z)
    assert store._act_stream == 2


def test_act_policy_refuses_bad_inputs_cpu(oracle_backend):
    _check_act_policy_refusals("cpu")


@pytest.mark.gpu
def test_act_policy_refuses_bad_inputs(hip_backend):
    _check_act_policy_refusals("cuda")


# ---- GPU: layout, exactly --------------------------------------------------------------------------------------------------------------
class _Single(torch.nn.Module):
    """One Linear as both nets: actor [in -> out]; the critic is present only when out == 1."""

    def __init__(self, w, b):
        super().__init__()
        lin = torch.nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(w)
            lin.bias.copy_(b)
        self.actor = torch.nn.Sequential(lin)
        self.critic = torch.nn.Sequential(copy.deepcopy(lin)) if w.shape[0] == 1 else None
        self.std = torch.nn.Parameter(torch.ones(w.shape[0]))


def _split(x, parts):
    if parts == 1 or x.shape[1] < 3:
        return (x,)
    a, b = x.shape[1] // 3, x.shape[1] // 3 + max(1, x.shape[1] // 4)
    return tuple(t.contiguous() for t in (x[:, :a], x[:, a:b], x[:, b:]))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 1000])
@pytest.mark.parametrize("width", [1, 3, 37, 48, 310, 512, 1024])
def test_layout_is_exact_on_integer_data(hip_backend, n, width):
    from genesis_forge_amd.learner import PolicyForward

    lim = 2 if width > 512 else 4   # |sum| <= 1024 * 2 * 4 + 4 < 2^24: every partial sum is an exact f32
    for out in (1, 12, 37, 64):
        for parts in (1, 3):
            g = torch.Generator().manual_seed(width * 131 + out * 7 + n + parts)
            x = torch.randint(-lim, lim + 1, (n, width), generator=g).float()
            w = torch.randint(-4, 5, (out, width), generator=g).float()
            b = torch.randint(-4, 5, (out,), generator=g).float()
            ref = x.double() @ w.double().T + b.double()
            fwd = PolicyForward(_Single(w, b).cuda())
            segs = _split(x.cuda(), parts)
            mean = fwd.mean(segs if len(segs) > 1 else segs[0])
            torch.cuda.synchronize()
            assert torch.equal(mean.double().cpu(), ref), f"mean: in {width} ({len(segs)} segments), out {out}, {n} rows"
            if out == 1:
                v = fwd.value(segs)
                torch.cuda.synchronize()
                assert tuple(v.shape) == (n, 1) and torch.equal(v.double().cpu(), ref), f"value: in {width}, {n} rows"


# ---- GPU: accuracy against float64 ---------------------------------------------------------------------------------------------------
def _bound(name, out, f32, ref):
    """Bound 5 of the issue: e_hip <= 4 e_torch + 1e-7 max|ref| (printed before it is asserted)."""
    e_hip, e_torch, top = float((out.double() - ref).abs().max()), float((f32.double() - ref).abs().max()), float(ref.abs().max())
    print(f"    {name}: e_hip {e_hip:.3e}  e_torch {e_torch:.3e}  ratio {e_hip / max(e_torch, 1e-300):.2f}  max|ref| {top:.3e}")
    assert e_hip <= 4 * e_torch + 1e-7 * top, f"{name}: e_hip {e_hip:.3e} > 4 x e_torch {e_torch:.3e} + 1e-7 x {top:.3e}"


def _accuracy(backend, segs, hidden, A, n, scale, critic_only=False):
    from genesis_forge_amd.learner import PolicyForward

    policy = _policy((48,) if critic_only else segs, hidden, A, "cuda", seed=2, scale=scale, critic_segs=segs if critic_only else None)
    ref64 = copy.deepcopy(policy).double()
    fwd = PolicyForward(policy)
    obs = _obs(segs, n, "cuda", scale=scale)
    x = _one(obs)
    print(f"  segments {segs} hidden {hidden} A {A} rows {n} scale x{scale}")
    with torch.no_grad():
        if not critic_only:
            _bound("mean ", fwd.mean(obs), policy.act_mean(x), ref64.act_mean(x.double()))
        _bound("value", fwd.value(obs), policy.evaluate(x), ref64.evaluate(x.double()))


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s[0] + s[1] + (s[2],))))
def test_accuracy_against_float64(hip_backend, shape, n, scale):
    _accuracy(hip_backend, *shape, n, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("n", SIZES)
def test_accuracy_against_float64_critic_two_segments(hip_backend, n, scale):
    _accuracy(hip_backend, *CRITIC_ONLY, n, scale, critic_only=True)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 3.0])
def test_accuracy_against_float64_65536(hip_backend, scale):
    _accuracy(hip_backend, *SHAPES[0], 65536, scale)


# ---- GPU: the sampling half --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s[0] + s[1] + (s[2],))))
def test_sampling_half(hip_backend, shape, n):
    from genesis_forge_amd.learner import PolicyForward

    segs, hidden, A = shape
    policy = _policy(segs, hidden, A, "cuda", seed=4)
    fwd = PolicyForward(policy)
    obs = _obs(segs, n, "cuda", seed=5)
    std = (torch.rand(A, generator=torch.Generator().manual_seed(6)) * 1.5 + 0.05).cuda()
    noise = torch.randn(n, A, generator=torch.Generator().manual_seed(7)).cuda()
    o = _raw(hip_backend, fwd, n, obs, obs, std, noise)
    assert torch.equal(o["mu_out"], o["mean"]) and torch.equal(o["values_out"], o["values"])
    assert torch.equal(o["mean"], fwd.mean(obs)) and torch.equal(o["values"], fwd.value(obs)[:, 0]), "each net alone gives the same bits"
    assert torch.equal(o["sigma_out"], std.expand(n, A))
    assert torch.equal(o["actions"], o["mu_out"] + std * noise) and torch.equal(o["actions_out"], o["actions"])
    _assert_fold(o["log_prob_out"], o["actions"], o["mu_out"], std)
    # Philox mode
    seed, stream, off = 1234, 5, 17
    p = _raw(hip_backend, fwd, n, obs, obs, std, None, seed=seed, stream=stream, env_offset=off)
    assert torch.equal(p["mean"], o["mean"])
    eps = torch.from_numpy(_np_normals(seed, stream, off, n, A)).cuda()
    assert float((p["actions"] - p["mu_out"] - std * eps).abs().max()) <= 1e-6
    q = _raw_policy_act(hip_backend, p["mean"], std, p["values"], seed=seed, stream=stream, env_offset=off)
    for mine, theirs in zip((p["actions"], p["actions_out"], p["mu_out"], p["sigma_out"], p["values_out"], p["log_prob_out"]), q):
        assert torch.equal(mine, theirs), "gf_policy_act draws the same from the same mean"
    _assert_fold(p["log_prob_out"], p["actions"], p["mu_out"], std)
    # mean only: nothing is drawn, nothing else is written
    m = _raw(hip_backend, fwd, n, obs, None, sample=False)
    assert torch.equal(m["mean"], o["mean"])


# ---- GPU: row independence, determinism ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rows_are_independent_and_deterministic(hip_backend):
    from genesis_forge_amd.learner import PolicyForward

    segs, hidden, A = SHAPES[0]
    n = 4133
    policy = _policy(segs, hidden, A, "cuda", seed=8)
    fwd = PolicyForward(policy)
    obs = _obs(segs, n, "cuda", seed=9)
    std = torch.full((A,), 0.6, device="cuda")
    keys = ("mean", "values", "actions", "log_prob_out", "mu_out", "values_out")
    full = _raw(hip_backend, fwd, n, obs, obs, std, seed=77, stream=3)
    again = _raw(hip_backend, fwd, n, obs, obs, std, seed=77, stream=3)
    for k in full:
        assert torch.equal(full[k], again[k]), f"two calls: {k}"
    for k0 in (1, 1000, 2049):
        part_obs = tuple(x[k0:].contiguous() for x in obs)
        part = _raw(hip_backend, fwd, n - k0, part_obs, part_obs, std, seed=77, stream=3, env_offset=k0)
        for k in keys:
            assert torch.equal(part[k], full[k][k0:]), f"rows {k0}… alone with env_offset={k0}: {k}"
    head_obs = tuple(x[:1000].contiguous() for x in obs)
    head = _raw(hip_backend, fwd, 1000, head_obs, head_obs, std, seed=77, stream=3)
    for k in keys:
        assert torch.equal(head[k], full[k][:1000]), f"the first 1000 rows alone: {k}"


# ---- GPU: through the storage ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_storage_act_policy_rows_streams_and_env_draws(hip_backend):
    from genesis_forge_amd.learner import PolicyForward, RolloutStorage

    n, T = 1000, 3
    env, twin = _go2(n), _go2(n)
    obs, _ = env.reset()
    twin.reset()
    store = RolloutStorage(env, T).attach()
    store.begin(obs)
    A = env.action_space.shape[0]
    policy = _policy((store.obs_width,), (64, 32), A, "cuda", seed=10)
    fwd = PolicyForward(policy)
    first = None
    obs0 = obs.clone()
    for k in range(2 * T + 1):
        t = 0 if store.full else store.step
        rng = env._rng_stream
        actions = store.act_policy(fwd, obs)
        assert env._rng_stream == rng, "act_policy() never advances the env's stream"
        mean, values = fwd.mean(obs), fwd.value(obs)
        torch.cuda.synchronize()
        assert torch.equal(store.actions[t], actions) and torch.equal(store.mu[t], mean) and torch.equal(store.values[t], values[:, 0])
        assert torch.equal(store.sigma[t], policy.std.detach().expand(n, A))
        eps = torch.from_numpy(_np_normals(env._rng_seed, k, 0, n, A)).cuda()
        assert float((actions - (mean + policy.std.detach() * eps)).abs().max()) <= 1e-6
        _assert_fold(store.actions_log_prob[t], actions, mean, policy.std.detach())
        if first is None:
            first = actions.clone()
        fixed = torch.zeros(n, A, device="cuda")
        out = env.step(fixed)
        out2 = twin.step(fixed)
        store.process_env_step(out[3])
        assert env._rng_stream == twin._rng_stream
        for x, y in zip(out[:4], out2[:4]):
            assert torch.equal(x, y), "the env's trajectory does not depend on act_policy()"
        obs = out[0]
    store.seed(env._rng_seed)
    assert torch.equal(store.act_policy(fwd, obs0), first), "seed() restarts the stream"


@pytest.mark.gpu
def test_gait_critic_segments_from_the_group_rows(hip_backend):
    from genesis_forge_amd import tasks
    from genesis_forge_amd.learner import PolicyForward, RolloutStorage

    n, T = 384, 4
    env = tasks.Go2GaitTrainingEnv(num_envs=n, max_episode_length_s=0.4, scene_kwargs=dict(ang_noise=0.3, seed=3, contact_prob=0.05))
    env.build()
    env.seed(7)
    obs, extras = env.reset()
    groups = {"policy": ["policy"], "critic": ["policy", "critic"]}
    st = RolloutStorage(env, T, obs_groups=groups).attach()
    st.begin(obs, extras)
    A = env.action_space.shape[0]
    widths = tuple(st.group_rows[m].shape[2] for m in groups["critic"])
    policy = _policy((st.obs_width,), (128, 64), A, "cuda", seed=11, critic_segs=widths)
    ref64 = copy.deepcopy(policy).double()
    fwd = PolicyForward(policy)
    for _ in range(T):
        t = st.step
        cseg = tuple(st.group_rows[m][t] for m in groups["critic"])   # the rows the step's own launches stored
        actions = st.act_policy(fwd, st.observations[t], critic_obs=cseg)
        x = torch.cat(cseg, dim=-1)
        with torch.no_grad():
            _bound("value", st.values[t], policy.evaluate(x)[:, 0], ref64.evaluate(x.double())[:, 0])
            _bound("mean ", st.mu[t], policy.act_mean(st.observations[t]), ref64.act_mean(st.observations[t].double()))
        assert torch.equal(st.actions[t], actions)
        _o, _r, _te, tr, _ex = env.step(actions)
        st.process_env_step(tr)


# ---- GPU: live weights, no host synchronisation ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_forward_reads_the_live_weights_and_never_synchronises(hip_backend):
    from genesis_forge_amd.learner import PPO, EpisodeStatistics, PolicyForward, RolloutStorage
    from test_ppo_update import ALGO

    n, T = 256, 24
    env = _go2(n)
    obs, extras = env.reset()
    st = RolloutStorage(env, T).attach()
    st.begin(obs, extras)
    st.seed(5)
    A = env.action_space.shape[0]
    policy = _policy((st.obs_width,), (64, 32), A, "cuda", seed=12)
    fwd = PolicyForward(policy)   # before the PPO re-seats every p.data
    before_ptr = policy.actor[0].weight.data_ptr()
    ppo = PPO(policy, st, **ALGO)
    assert policy.actor[0].weight.data_ptr() != before_ptr, "PPO moved the parameters into its flat buffer"
    stats = EpisodeStatistics(n)
    probe = obs.clone()
    before = fwd.mean(probe).clone()
    torch.cuda.synchronize()
    honoured = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(1, device="cuda").item()
    except RuntimeError:
        honoured = True
    finally:
        torch.cuda.set_sync_debug_mode(0)
    if honoured:
        torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(T):
            actions = st.act_policy(fwd, obs)
            obs, _r, _te, tr, _ex = env.step(actions)
            st.process_env_step(tr, gamma=ppo.gamma, episodes=stats)
        last = fwd.value(obs)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    st.compute_returns(last, gamma=ppo.gamma, lam=ppo.lam)
    ppo.update(generator=torch.Generator(device="cuda").manual_seed(0))
    after = fwd.mean(probe)
    ref64 = copy.deepcopy(policy).double()
    with torch.no_grad():
        _bound("mean after update ", after, policy.act_mean(probe), ref64.act_mean(probe.double()))
        _bound("value after update", fwd.value(probe), policy.evaluate(probe), ref64.evaluate(probe.double()))
    assert not torch.equal(after, before), "the forward follows the optimiser's in-place updates"
