"""Empirical observation normalisation of the PPO learner (rsl_rl ``EmpiricalNormalization``): ``gf_obs_norm_update`` — the running
statistics of up to two normalisers in two launches — the normalisation folded into ``gf_mlp_act``'s input staging and into
``gf_minibatch_gather``, and the way up: ``learner.EmpiricalNormalization``, ``ActorCriticMLP``'s two options and
``from_train_cfg``, ``PolicyForward``, ``RolloutStorage.mini_batch_generator`` and ``PPO``.

* CPU: the torch path against rsl_rl's class restated (tests/rsl_rl_norm.py), bit for bit; ``until`` and eval mode; rsl_rl's
  ``state_dict``; the training dict's three spellings of the switch; the ABI size and every refusal of the three entry points (they
  return before any launch); ``PPO.update`` on the oracle backend against the restated rsl_rl update.
* GPU: the update kernel against float64 (``|Δmean| <= 2⁻²¹ (|mean| + std)``, ``|Δvar| <= 2⁻²¹ var``: four f32 epsilons — the
  float64 evaluation's own error can only move a result across an f32 rounding boundary), ``_std == sqrt(_var)`` and ``count``
  exact, freezing, set independence, determinism, no host read; the two consumers bitwise against the CPU's f32
  ``(x - mean) / (std + eps)``; ``PPO.update`` against the torch path; a collection loop."""
import contextlib
import copy
import ctypes as C
import types

import pytest
import torch

from rsl_rl_norm import RslRlEmpiricalNormalization
from rsl_rl_ppo import RslRlPPO
from test_ppo_update import ALGO, GAIT_GROUPS, _env, _flat

BOUND = 2.0 ** -21


@contextlib.contextmanager
def host_reads():
    """Counts the calls that read a tensor back to the host (or wait for the device): Tensor.item / tolist / cpu / __bool__ /
    __float__ and torch.cuda.synchronize (the witness of tests/test_ppo_update.py)."""
    count = [0]
    T = torch.Tensor
    saved = {n: getattr(T, n) for n in ("item", "tolist", "cpu", "__bool__", "__float__")}
    saved_sync = torch.cuda.synchronize

    def wrap(f):
        def g(*a, **k):
            count[0] += 1
            return f(*a, **k)
        return g

    try:
        for n, f in saved.items():
            setattr(T, n, wrap(f))
        torch.cuda.synchronize = wrap(saved_sync)
        yield count
    finally:
        for n, f in saved.items():
            setattr(T, n, f)
        torch.cuda.synchronize = saved_sync


# ---- data ---------------------------------------------------------------------------------------------------------------------------
def _data(n, w, t=0, seed=0):
    """``x = randn·exp(2·randn_c) + 50·randn_c + 0.1·t``: every column its own scale (e^±4 and beyond) and offset."""
    g = torch.Generator().manual_seed(1000 * seed + w)
    scale, offset = torch.exp(2 * torch.randn(w, generator=g)), 50 * torch.randn(w, generator=g)
    gx = torch.Generator().manual_seed(7919 * n + 31 * w + t + 17 * seed)
    return (torch.randn(n, w, generator=gx) * scale + offset + 0.1 * t).contiguous()


def _split(x, widths):
    if widths is None:
        return x
    out, at = [], 0
    for w in widths:
        out.append(x[:, at:at + w].contiguous())
        at += w
    return tuple(out)


def _warm(norm, seed=3):
    """A state with count > 0."""
    g = torch.Generator().manual_seed(seed + norm.width)
    with torch.no_grad():
        norm._mean.copy_((20 * torch.randn(1, norm.width, generator=g)).to(norm._mean.device))
        norm._var.copy_(torch.exp(2 * torch.randn(1, norm.width, generator=g)).to(norm._mean.device))
        norm._std.copy_(torch.sqrt(norm._var))
        norm.count.fill_(1000)
    return norm


def _state(norm):
    return norm._mean.detach().cpu().clone(), norm._var.detach().cpu().clone(), norm._std.detach().cpu().clone(), int(norm.count.cpu())


def _ref_update(state, x):
    """The contract's formulas in float64 from the f32 inputs and the f32 state; mean' and var' rounded to f32 once each."""
    mean, var, _std, count = state
    x = x.double()
    n = x.shape[0]
    mx, vx = x.mean(dim=0, keepdim=True), x.var(dim=0, unbiased=False, keepdim=True)
    count1 = count + n
    rate = n / count1
    m, v = mean.double(), var.double()
    d = mx - m
    m1 = m + rate * d
    v1 = v + rate * (vx - v + d * (mx - m1))
    v1 = v1.float()
    return m1.float(), v1, torch.sqrt(v1), count1


def _check_state(norm, want, what):
    mean, var, std, count = _state(norm)
    wm, wv, ws, wc = want
    em = float(((mean.double() - wm.double()).abs() / (wm.double().abs() + ws.double())).nan_to_num(0.0).max())
    ev = float(((var.double() - wv.double()).abs() / wv.double()).nan_to_num(0.0).max())
    print(f"{what}: max |dmean| / (|mean| + std) = {em:.3e}, max |dvar| / var = {ev:.3e} (bound {BOUND:.3e})")
    assert count == wc, f"{what}: count {count} vs {wc}"
    assert bool(((mean.double() - wm.double()).abs() <= BOUND * (wm.double().abs() + ws.double())).all()), f"{what}: mean off by {em:.3e} of |mean| + std"
    assert bool(((var.double() - wv.double()).abs() <= BOUND * wv.double()).all()), f"{what}: var off by {ev:.3e}"
    # rsl_rl's line where the buffers live, and the correctly rounded root by a second route: the float64 root rounded to f32 (53 >=
    # 2·24 + 2 bits: the double rounding is innocuous).  Not torch.sqrt on a CPU copy: on some hosts its f32 root is an ulp off.
    assert torch.equal(std, torch.sqrt(norm._var).cpu()), f"{what}: _std is not torch.sqrt(_var) bit for bit"
    assert torch.equal(std, torch.sqrt(var.double()).float()), f"{what}: _std is not the correctly rounded root of _var"


# ---- CPU: the module ----------------------------------------------------------------------------------------------------------------
def test_torch_path_is_rsl_rl_bit_for_bit():
    from genesis_forge_amd.learner import EmpiricalNormalization

    for w, widths in ((37, None), (310, (250, 60)), (1, None)):
        a, b = EmpiricalNormalization(w), RslRlEmpiricalNormalization(w)
        for t, n in enumerate((1, 63, 257, 5, 1000)):
            x = _data(n, w, t)
            a.update(_split(x, widths))
            b.update(x)
            for k in ("_mean", "_var", "_std", "count"):
                assert torch.equal(getattr(a, k), getattr(b, k)), (w, t, k)
        y = _data(9, w, 99)
        assert torch.equal(a(y), b(y)) and torch.equal(a.inverse(y), b.inverse(y))
        assert torch.equal(a.mean, b.mean) and torch.equal(a.std, b.std) and a.mean.shape == (w,)


def test_until_and_eval_mode_freeze():
    from genesis_forge_amd.learner import EmpiricalNormalization

    a, b = EmpiricalNormalization(5, until=100), RslRlEmpiricalNormalization(5, until=100)
    for t in range(4):   # counts 0, 40, 80 update; 120 >= 100 does not
        x = _data(40, 5, t)
        a.update(x)
        b.update(x)
    assert int(a.count) == 120 == int(b.count)
    before = _state(a)
    a.update(_data(40, 5, 9))
    assert all(torch.equal(p, q) for p, q in zip(before[:3], _state(a)[:3])) and int(a.count) == 120
    assert torch.equal(a._mean, b._mean) and torch.equal(a._var, b._var)
    c = EmpiricalNormalization(5).eval()
    c.update(_data(40, 5, 0))
    assert int(c.count) == 0 and torch.equal(c._mean, torch.zeros(1, 5)) and torch.equal(c._var, torch.ones(1, 5))
    c.train()
    c.update(_data(40, 5, 0))
    assert int(c.count) == 40


def test_state_dict_is_rsl_rl_s():
    from genesis_forge_amd.learner import EmpiricalNormalization

    a, b = EmpiricalNormalization(12), RslRlEmpiricalNormalization(12)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) == ["_mean", "_var", "_std", "count"]
    assert all(sa[k].shape == sb[k].shape and sa[k].dtype == sb[k].dtype for k in sa)
    assert sa["_mean"].shape == (1, 12) and sa["count"].shape == () and sa["count"].dtype == torch.int64
    for t in range(3):
        b.update(_data(50, 12, t))
    a.load_state_dict(b.state_dict())
    x = _data(7, 12, 5)
    assert torch.equal(a(x), b(x)) and int(a.count) == 150
    with pytest.raises(ValueError):
        EmpiricalNormalization((3, 4))


def test_update_refuses_what_it_would_have_to_cast_or_copy():
    from genesis_forge_amd.learner import EmpiricalNormalization

    a = EmpiricalNormalization(6)
    with pytest.raises(ValueError, match="float32"):
        a.update(torch.zeros(4, 6, dtype=torch.float64))
    with pytest.raises(ValueError, match="strided view"):
        a.update(torch.zeros(4, 12)[:, :6])
    with pytest.raises(ValueError, match="wide"):
        a.update(torch.zeros(4, 5))
    with pytest.raises(ValueError, match="1 to 4"):
        a.update([torch.zeros(4, 1)] * 6)
    with pytest.raises(ValueError):
        a.update((torch.zeros(4, 3), torch.zeros(5, 3)))
    assert int(a.count) == 0


def test_actor_critic_options_and_train_cfg():
    from genesis_forge_amd.learner import ActorCriticMLP, EmpiricalNormalization

    torch.manual_seed(0)
    plain = ActorCriticMLP(10, 3, (16, 8), (16, 8))
    keys = ["std"] + [f"{net}.{i}.{p}" for net in ("actor", "critic") for i in (0, 2, 4) for p in ("weight", "bias")]
    assert list(plain.state_dict()) == keys and [n for n, _ in plain.named_parameters()] == keys
    assert isinstance(plain.actor_obs_normalizer, torch.nn.Identity) and isinstance(plain.critic_obs_normalizer, torch.nn.Identity)
    torch.manual_seed(0)
    both = ActorCriticMLP(10, 3, (16, 8), (16, 8), num_critic_obs=14, actor_obs_normalization=True, critic_obs_normalization=True)
    assert [n for n, _ in both.named_parameters()] == keys   # the flat bucket's order is unchanged
    assert torch.equal(both.actor[0].weight, plain.actor[0].weight) and both.critic[0].weight.shape == (16, 14)
    assert both.actor_obs_normalizer.width == 10 and both.critic_obs_normalizer.width == 14
    obs, cobs = _data(20, 10), _data(20, 14)
    both.update_normalization(obs, cobs)
    ref_a, ref_c = RslRlEmpiricalNormalization(10), RslRlEmpiricalNormalization(14)
    ref_a.update(obs), ref_c.update(cobs)
    assert torch.equal(both.actor_obs_normalizer._mean, ref_a._mean) and torch.equal(both.critic_obs_normalizer._var, ref_c._var)
    assert torch.equal(both.act_mean(obs), both.actor(ref_a(obs))) and torch.equal(both.evaluate(cobs), both.critic(ref_c(cobs)))
    assert torch.equal(plain.act_mean(obs), plain.actor(obs))

    cfg = {"policy": {"activation": "elu", "actor_hidden_dims": [32, 16], "critic_hidden_dims": [24], "init_noise_std": 0.5, "class_name": "ActorCritic"},
           "empirical_normalization": None, "obs_groups": {"policy": ["policy"], "critic": ["policy"]}}
    is_norm = lambda p: (isinstance(p.actor_obs_normalizer, EmpiricalNormalization), isinstance(p.critic_obs_normalizer, EmpiricalNormalization))
    p = ActorCriticMLP.from_train_cfg(cfg, 10, 3)
    assert is_norm(p) == (False, False) and p.actor[0].weight.shape == (32, 10) and p.critic[0].weight.shape == (24, 10) and float(p.std.detach()[0]) == 0.5
    assert is_norm(ActorCriticMLP.from_train_cfg(dict(cfg, empirical_normalization=False), 10, 3)) == (False, False)
    assert is_norm(ActorCriticMLP.from_train_cfg(dict(cfg, empirical_normalization=True), 10, 3, num_critic_obs=14)) == (True, True)
    assert is_norm(ActorCriticMLP.from_train_cfg(dict(cfg, policy=dict(cfg["policy"], actor_obs_normalization=True)), 10, 3)) == (True, False)
    assert is_norm(ActorCriticMLP.from_train_cfg(dict(cfg, policy=dict(cfg["policy"], critic_obs_normalization=True)), 10, 3)) == (False, True)
    with pytest.raises(ValueError, match="activation"):
        ActorCriticMLP.from_train_cfg(dict(cfg, policy=dict(cfg["policy"], activation="relu")), 10, 3)
    with pytest.raises(ValueError, match="rnn_type"):
        ActorCriticMLP.from_train_cfg(dict(cfg, policy=dict(cfg["policy"], rnn_type="lstm")), 10, 3)


def test_policy_forward_refuses_a_foreign_normalizer():
    from genesis_forge_amd.learner import ActorCriticMLP, EmpiricalNormalization, PolicyForward

    policy = ActorCriticMLP(10, 3, (16,), (16,), actor_obs_normalization=True)
    PolicyForward(policy)
    policy.critic_obs_normalizer = None
    PolicyForward(policy)
    policy.actor_obs_normalizer = EmpiricalNormalization(11)
    with pytest.raises(ValueError, match="actor_obs_normalizer"):
        PolicyForward(policy)
    policy.actor_obs_normalizer = torch.nn.LayerNorm(10)
    with pytest.raises(ValueError, match="LayerNorm"):
        PolicyForward(policy)


# ---- CPU: ABI, refusals -------------------------------------------------------------------------------------------------------------
def test_abi_size_and_raw_refusals():
    from genesis_forge_amd import _native as nat

    lib = C.CDLL(nat.lib_path())
    lib.gf_sizeof.argtypes, lib.gf_sizeof.restype = [C.c_int], C.c_int
    assert nat.GF_SIZEOF_OBS_NORM == 29 and lib.gf_sizeof(29) == C.sizeof(nat.GfObsNormArgs)
    assert lib.gf_sizeof(nat.GF_SIZEOF_MLP_ACT) == C.sizeof(nat.GfMlpActArgs) and lib.gf_sizeof(nat.GF_SIZEOF_MINIBATCH) == C.sizeof(nat.GfMinibatchArgs)
    assert (nat.GF_OBS_NORM_MAX_SETS, nat.GF_OBS_NORM_TILE_ROWS, nat.GF_OBS_NORM_MAX_PARTIALS) == (2, 256, 256)
    assert nat.obs_norm_workspace_bytes(1, 3) == 7 * 8 and nat.obs_norm_workspace_bytes(257, 48) == 2 * 97 * 8
    assert nat.obs_norm_workspace_bytes(256 * 256 + 1, 3) == nat.obs_norm_workspace_bytes(10 ** 9, 3) == 256 * 7 * 8
    E_NULL, E_RANGE = -1, -2
    PTR = 0x1000   # never dereferenced: every call below returns before a launch

    # gf_obs_norm_update
    lib.gf_obs_norm_update.argtypes, lib.gf_obs_norm_update.restype = [C.POINTER(nat.GfObsNormArgs), C.c_void_p], C.c_int

    def args(widths=((48,), (250, 60)), num_rows=0, sets=None, **kw):
        a = nat.GfObsNormArgs()
        a.num_rows, a.num_sets = num_rows, len(widths) if sets is None else sets
        for st, ws in zip(a.sets, widths):
            st.num_inputs = len(ws)
            for seg, w in zip(st.inputs, ws):
                seg.rows, seg.width = PTR, w
            st.mean = st.var = st.std = st.count = st.workspace = PTR
            st.until, st.workspace_bytes = -1, nat.obs_norm_workspace_bytes(max(num_rows, 0), sum(ws))
        for k, v in kw.items():
            setattr(a.sets[0], k, v)
        return a

    call = lambda a: lib.gf_obs_norm_update(C.byref(a), None)
    assert lib.gf_obs_norm_update(None, None) == E_NULL
    assert call(args()) == 0 and call(args(widths=((1024,),))) == 0, "num_rows == 0 is a no-op"
    assert call(args(num_rows=-1)) == E_RANGE
    assert call(args(sets=0)) == E_RANGE and call(args(sets=3)) == E_RANGE
    for field in ("mean", "var", "std", "count", "workspace"):
        assert call(args(**{field: None})) == E_NULL, field
    broken = args()
    broken.sets[1].inputs[1].rows = None
    assert call(broken) == E_NULL
    assert call(args(num_inputs=0)) == E_RANGE and call(args(num_inputs=5)) == E_RANGE
    assert call(args(widths=((0,),))) == E_RANGE and call(args(widths=((1000, 25),))) == E_RANGE and call(args(widths=((1000, 24),))) == 0
    small = args(num_rows=300)
    small.sets[1].workspace_bytes -= 8
    assert call(small) == E_RANGE, "a workspace too small"
    assert call(args(num_rows=300, workspace=PTR + 4)) == E_RANGE and call(args(num_rows=300, count=PTR + 4)) == E_RANGE

    # gf_mlp_act: in_mean without in_std
    lib.gf_mlp_act.argtypes, lib.gf_mlp_act.restype = [C.POINTER(nat.GfMlpActArgs), C.c_void_p], C.c_int

    def mlp(**kw):
        a = nat.GfMlpActArgs()
        for net, out in ((a.actor, 12), (a.critic, 1)):
            net.num_layers, net.num_inputs = 2, 1
            net.inputs[0].rows, net.inputs[0].width = PTR, 48
            for lay, w in zip(net.layers, (64, out)):
                lay.weight, lay.bias, lay.out_width = PTR, PTR, w
        a.std = a.actions = a.mean = a.values = PTR
        for k, v in kw.items():
            net, field = k.split("__")
            setattr(getattr(a, net), field, v)
        return a

    mcall = lambda a: lib.gf_mlp_act(C.byref(a), None)
    assert mcall(mlp()) == 0
    assert mcall(mlp(actor__in_mean=PTR, actor__in_std=PTR, critic__in_mean=PTR, critic__in_std=PTR)) == 0
    assert mcall(mlp(actor__in_mean=PTR)) == E_NULL and mcall(mlp(critic__in_mean=PTR)) == E_NULL
    assert mcall(mlp(actor__in_std=PTR)) == 0, "a std without a mean is not read"

    # gf_minibatch_gather: mean without std
    lib.gf_minibatch_gather.argtypes, lib.gf_minibatch_gather.restype = [C.POINTER(nat.GfMinibatchArgs), C.c_void_p], C.c_int

    def mb(**kw):
        a = nat.GfMinibatchArgs()
        a.num_rows, a.num_src_rows, a.indices, a.num_fields = 0, 10, PTR, 2
        for f in a.fields[:2]:
            f.src, f.dst, f.src_width, f.dst_width, f.dst_col = PTR, PTR, 5, 5, 0
        for k, v in kw.items():
            setattr(a.fields[1], k, v)
        return a

    gcall = lambda a: lib.gf_minibatch_gather(C.byref(a), None)
    assert gcall(mb()) == 0 and gcall(mb(mean=PTR, std=PTR)) == 0
    assert gcall(mb(mean=PTR)) == E_NULL


# ---- PPO with normalisers -----------------------------------------------------------------------------------------------------------
def _norm_setup(kind, n, T, dev, hidden=(64, 32)):
    from genesis_forge_amd.learner import ActorCriticMLP, RolloutStorage

    env = _env(kind, n)
    obs, extras = env.reset()
    st = RolloutStorage(env, T, obs_groups=GAIT_GROUPS if kind == "gait" else None).attach()
    st.begin(obs, extras)
    st.seed(5)
    A = env.action_space.shape[0]
    critic_w = sum(st.group_rows[m].shape[2] for m in st.obs_groups["critic"])
    torch.manual_seed(0)
    policy = ActorCriticMLP(st.obs_width, A, hidden, hidden, init_noise_std=0.8, num_critic_obs=critic_w,
                            actor_obs_normalization=True, critic_obs_normalization=True).to(dev)
    return env, st, policy, [obs, extras]


def _norm_collect(env, st, policy, state, noise_gen=None):
    """One rollout of the documented loop: act_policy -> env.step -> update_normalization -> process_env_step."""
    from genesis_forge_amd.learner import PolicyForward

    fwd = PolicyForward(policy)
    obs, extras = state
    n, A = env.num_envs, env.action_space.shape[0]
    critic = st.obs_groups["critic"]
    cobs_of = lambda obs, extras: obs if critic == st.obs_groups["policy"] else tuple(extras["observations"][m] for m in critic)
    for _ in range(st.num_steps):
        noise = None if noise_gen is None else torch.randn(n, A, generator=noise_gen).to(obs.device)
        actions = st.act_policy(fwd, obs, cobs_of(obs, extras), noise=noise)
        obs, _r, _te, tr, extras = env.step(actions)
        policy.update_normalization(obs, cobs_of(obs, extras))
        st.process_env_step(tr)
    state[0], state[1] = obs, extras
    c = cobs_of(obs, extras)
    return c if isinstance(c, torch.Tensor) else torch.cat(c, dim=-1)


def test_update_with_normalizers_is_rsl_rl_on_normalized_batches_cpu(oracle_backend):
    """The oracle-backend path with normalisers against rsl_rl's update restated: its ``policy.act_mean(b.obs)`` IS
    ``actor(normalizer(obs))`` on the raw batch.  Bounds: those of test_ppo_update._end_to_end for the same pair without normalisers."""
    from genesis_forge_amd.learner import PPO

    env, st, policy, state = _norm_setup("go2", 70, 8, "cpu")
    last = _norm_collect(env, st, policy, state, torch.Generator().manual_seed(4))
    assert int(policy.actor_obs_normalizer.count) == 8 * 70 == int(policy.critic_obs_normalizer.count)
    ref_policy = copy.deepcopy(policy)
    ppo, ref = PPO(policy, st, **ALGO), RslRlPPO(ref_policy, st, **ALGO)
    ppo.compute_returns(last)
    # the batches come out normalised, the storage keeps the raw rows
    b = next(st.mini_batch_generator(4, 1, generator=torch.Generator().manual_seed(1), obs_normalizer=policy.actor_obs_normalizer,
                                     critic_obs_normalizer=policy.critic_obs_normalizer))
    raw = st.observations[:8].reshape(-1, st.obs_width)[b.indices]
    assert torch.equal(b.obs, policy.actor_obs_normalizer(raw)) and torch.equal(b.critic_obs, policy.critic_obs_normalizer(raw))
    assert b.critic_obs is not b.obs
    shared = next(st.mini_batch_generator(4, 1, generator=torch.Generator().manual_seed(1), obs_normalizer=policy.actor_obs_normalizer,
                                          critic_obs_normalizer=policy.actor_obs_normalizer))
    assert shared.critic_obs is shared.obs
    with pytest.raises(ValueError, match="obs_normalizer"):
        st.mini_batch_generator(4, 1, obs_normalizer=torch.nn.LayerNorm(st.obs_width))
    want = ref.update(generator=torch.Generator().manual_seed(10))
    got = ppo.update(generator=torch.Generator().manual_seed(10))
    for k in ("value_function", "surrogate", "entropy"):
        assert abs(got[k] - want[k]) <= 1e-4 * max(abs(want[k]), 1e-6), f"{k} {got[k]} vs {want[k]}"
    assert ppo.learning_rate == ref.learning_rate
    a, r = _flat(policy), _flat(ref_policy)
    d = (a - r).abs()
    assert float((d <= 1e-4 + 1e-3 * r.abs()).float().mean()) >= 0.995 and float(d.max()) <= 2 * 3.2 * 1e-2 * 20
    for k in ("_mean", "_var", "_std", "count"):   # the statistics are frozen during an update
        assert torch.equal(getattr(policy.actor_obs_normalizer, k), getattr(ref_policy.actor_obs_normalizer, k))


# ---- GPU: gf_obs_norm_update against float64 ------------------------------------------------------------------------------------------
ROWS = [1, 63, 257, 4133]
WIDTHS = [1, 3, 37, 48, 310, 1024]
SEGMENTS = {310: (250, 60), 37: (5, 1, 30, 1)}


def _gpu_norm(w, warm):
    from genesis_forge_amd.learner import EmpiricalNormalization

    norm = EmpiricalNormalization(w).to("cuda")
    return _warm(norm) if warm else norm


def _one_update(n, w, warm, widths=None):
    norm = _gpu_norm(w, warm)
    x = _data(n, w)
    want = _ref_update(_state(norm), x)
    norm.update(_split(x.cuda(), widths))
    _check_state(norm, want, f"N={n} W={w} {'warm' if warm else 'fresh'} {widths or ''}")


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True], ids=["fresh", "warm"])
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("n", ROWS)
def test_update_kernel_against_float64(hip_backend, n, w, warm):
    _one_update(n, w, warm)


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True], ids=["fresh", "warm"])
@pytest.mark.parametrize("w", sorted(SEGMENTS))
@pytest.mark.parametrize("n", ROWS)
def test_update_kernel_against_float64_segments(hip_backend, n, w, warm):
    _one_update(n, w, warm, SEGMENTS[w])


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True], ids=["fresh", "warm"])
def test_update_kernel_grid_stride_wraps(hip_backend, warm):
    from genesis_forge_amd import _native as nat

    _one_update(nat.GF_OBS_NORM_MAX_PARTIALS * nat.GF_OBS_NORM_TILE_ROWS + 1, 3, warm)


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True], ids=["fresh", "warm"])
@pytest.mark.parametrize("n,w,widths", [(1, 3, None), (63, 310, (250, 60)), (257, 37, (5, 1, 30, 1)), (4133, 48, None), (257, 1024, None), (4133, 1, None)])
def test_update_kernel_chain_of_24(hip_backend, n, w, widths, warm):
    norm = _gpu_norm(w, warm)
    ref = _state(norm)
    for t in range(24):
        x = _data(n, w, t)
        ref = _ref_update(ref, x)
        norm.update(_split(x.cuda(), widths))
    _check_state(norm, ref, f"chain N={n} W={w}")
    assert ref[3] == 24 * n + (1000 if warm else 0)


@pytest.mark.gpu
def test_frozen_set_is_untouched_while_the_other_updates(hip_backend):
    from genesis_forge_amd.learner import ActorCriticMLP

    policy = ActorCriticMLP(48, 12, (16,), (16,), num_critic_obs=310, actor_obs_normalization=True, critic_obs_normalization=True).to("cuda")
    _warm(policy.actor_obs_normalizer), _warm(policy.critic_obs_normalizer)
    policy.actor_obs_normalizer.until = 1000   # count == 1000 already: frozen
    before = [getattr(policy.actor_obs_normalizer, k).clone() for k in ("_mean", "_var", "_std", "count")]
    obs, cobs = _data(300, 48), _data(300, 310)
    want = _ref_update(_state(policy.critic_obs_normalizer), cobs)
    policy.update_normalization(obs.cuda(), _split(cobs.cuda(), SEGMENTS[310]))
    for k, b in zip(("_mean", "_var", "_std", "count"), before):
        assert torch.equal(getattr(policy.actor_obs_normalizer, k), b), k
    _check_state(policy.critic_obs_normalizer, want, "the other set")
    policy.actor_obs_normalizer.until = 1001   # not reached yet: updates, then freezes
    want = _ref_update(_state(policy.actor_obs_normalizer), obs)
    policy.update_normalization(obs.cuda(), cobs.cuda())
    _check_state(policy.actor_obs_normalizer, want, "until not reached")
    frozen = _state(policy.actor_obs_normalizer)
    policy.update_normalization(obs.cuda(), cobs.cuda())
    assert all(torch.equal(a, b) for a, b in zip(frozen[:3], _state(policy.actor_obs_normalizer)[:3])) and int(policy.actor_obs_normalizer.count) == 1300
    assert int(policy.critic_obs_normalizer.count) == 1900
    policy.eval()
    policy.update_normalization(obs.cuda(), cobs.cuda())
    assert int(policy.critic_obs_normalizer.count) == 1900


@pytest.mark.gpu
@pytest.mark.parametrize("n", [63, 4133])
def test_two_sets_equal_two_calls_and_runs_repeat_bitwise(hip_backend, n):
    from genesis_forge_amd.learner import ActorCriticMLP

    policy = ActorCriticMLP(48, 12, (16,), (16,), num_critic_obs=1024, actor_obs_normalization=True, critic_obs_normalization=True).to("cuda")
    _warm(policy.actor_obs_normalizer), _warm(policy.critic_obs_normalizer)
    single, again = copy.deepcopy(policy), copy.deepcopy(policy)
    obs, cobs = _data(n, 48).cuda(), _data(n, 1024).cuda()
    policy.update_normalization(obs, cobs)
    single.actor_obs_normalizer.update(obs)
    single.critic_obs_normalizer.update(cobs)
    again.update_normalization(obs, cobs)
    for name in ("actor_obs_normalizer", "critic_obs_normalizer"):
        for k in ("_mean", "_var", "_std", "count"):
            got = getattr(getattr(policy, name), k)
            assert torch.equal(got, getattr(getattr(single, name), k)), f"{name}.{k}: two sets in one call differ from two calls"
            assert torch.equal(got, getattr(getattr(again, name), k)), f"{name}.{k}: the same update on a clone differs"


@pytest.mark.gpu
def test_update_reads_nothing_back(hip_backend):
    from genesis_forge_amd.learner import ActorCriticMLP

    policy = ActorCriticMLP(48, 12, (16,), (16,), actor_obs_normalization=True, critic_obs_normalization=True).to("cuda")
    policy.actor_obs_normalizer.until = 500
    obs = _data(256, 48).cuda()
    policy.update_normalization(obs)   # (the workspaces are allocated)
    with host_reads() as c:
        for _ in range(3):
            policy.update_normalization(obs)
            policy.critic_obs_normalizer.update(obs)
    assert c[0] == 0, f"update read the device {c[0]} times"
    assert int(policy.actor_obs_normalizer.count) == 512 and int(policy.critic_obs_normalizer.count) == 7 * 256


# ---- GPU: the normalisation inside gf_mlp_act -----------------------------------------------------------------------------------------
def _normalized_on_cpu(norm, x):
    """rsl_rl's forward in f32 on the CPU: one subtraction, one addition, one correctly rounded division."""
    return ((x.cpu() - norm._mean.cpu()) / (norm._std.cpu() + norm.eps)).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("widths", [(37,), (48,), (600,), (1024,), (250, 60), (5, 1, 30, 1), (512, 1, 511)], ids=lambda s: "+".join(map(str, s)))
@pytest.mark.parametrize("n", [1, 63, 1000])
def test_mlp_act_normalizes_as_it_stages(hip_backend, n, widths):
    from genesis_forge_amd.learner import ActorCriticMLP, PolicyForward
    from test_mlp_act import _raw

    w, A = sum(widths), 12
    torch.manual_seed(w)
    policy = ActorCriticMLP(w, A, (128, 64), (128, 64), init_noise_std=0.7, actor_obs_normalization=True, critic_obs_normalization=True).to("cuda")
    _warm(policy.actor_obs_normalizer, 3), _warm(policy.critic_obs_normalizer, 4)
    plain = types.SimpleNamespace(actor=policy.actor, critic=policy.critic, std=policy.std)
    fwd, fwd_plain = PolicyForward(policy), PolicyForward(plain)
    x = _data(n, w, seed=2)
    raw = tuple(p.cuda() for p in _split(x, widths))
    xa = tuple(p.cuda() for p in _split(_normalized_on_cpu(policy.actor_obs_normalizer, x), widths))
    xc = tuple(p.cuda() for p in _split(_normalized_on_cpu(policy.critic_obs_normalizer, x), widths))
    assert not torch.equal(xa[0], xc[0])
    noise = torch.randn(n, A, generator=torch.Generator().manual_seed(n)).cuda()
    std = policy.std.detach()
    got = _raw(hip_backend, fwd, n, raw, raw, std, noise)
    want = _raw(hip_backend, fwd_plain, n, xa, xc, std, noise)
    assert set(got) == set(want) and "log_prob_out" in got and "values_out" in got
    for k in got:
        assert torch.equal(got[k], want[k]), f"{k}: the fused normalisation differs from the launch on the normalised input"
    assert torch.equal(fwd.mean(raw), fwd_plain.mean(xa)) and torch.equal(fwd.value(raw), fwd_plain.value(xc))
    assert torch.equal(fwd.mean(raw), got["mean"])


# ---- GPU: the normalisation inside gf_minibatch_gather --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mb", [1, 255, 4133])
def test_minibatch_gather_normalizes_on_the_way(hip_backend, mb):
    from genesis_forge_amd import _native as nat
    from genesis_forge_amd.learner import EmpiricalNormalization

    rows = 5000
    g = torch.Generator().manual_seed(mb)
    idx = torch.randint(0, rows, (mb,), generator=g)
    idx[mb // 2] = rows + 3   # out of range: a NaN row in every field
    # (source width, destination width, first column, normaliser key): 37 / 310 / 48 take the 4-, 8- and 16-byte chunk paths; the
    # two-member group (5 + 44 under one 49-wide normaliser) puts the second member at an odd column; the last field is a pure copy
    layout = [(37, 37, 0, "a"), (310, 310, 0, "b"), (48, 48, 0, "c"), (5, 49, 0, "g"), (44, 49, 5, "g"), (48, 48, 0, None)]
    norms = {k: _warm(EmpiricalNormalization(w), seed=i) for i, (k, w) in enumerate((("a", 37), ("b", 310), ("c", 48), ("g", 49)))}
    dev_norms = {k: copy.deepcopy(v).to("cuda") for k, v in norms.items()}
    srcs = [_data(rows, sw, seed=5 + i) for i, (sw, _dw, _c, _k) in enumerate(layout)]
    dsts = {}
    a = nat.GfMinibatchArgs()
    a.num_rows, a.num_src_rows, a.num_fields = mb, rows, len(layout)
    dev_idx, dev_srcs = idx.cuda(), [s.cuda() for s in srcs]
    a.indices = dev_idx.data_ptr()
    for f, (sw, dw, col, key), src in zip(a.fields, layout, dev_srcs):
        dst = dsts.setdefault((key, dw), torch.full((mb, dw), 7.0, device="cuda"))
        f.src, f.dst, f.src_width, f.dst_width, f.dst_col = src.data_ptr(), dst.data_ptr(), sw, dw, col
        if key is not None:
            f.mean, f.std, f.eps = dev_norms[key]._mean.data_ptr() + 4 * col, dev_norms[key]._std.data_ptr() + 4 * col, dev_norms[key].eps
    hip_backend.minibatch_gather(a)
    torch.cuda.synchronize()
    ok = idx < rows
    assert int((~ok).sum()) == 1
    safe = idx.clamp(max=rows - 1)
    for (sw, dw, col, key), src in zip(layout, srcs):
        got = dsts[(key, dw)].cpu()[:, col:col + sw]
        want = src[safe]
        if key is not None:
            n = norms[key]
            want = (want - n._mean[:, col:col + sw]) / (n._std[:, col:col + sw] + n.eps)
        assert torch.equal(got[ok], want[ok]), f"field {sw}@{col} of {dw} ({key})"
        assert bool(got[~ok].isnan().all()), f"field {sw}@{col}: the out-of-range row is not NaN"


@pytest.mark.gpu
def test_mini_batch_generator_normalizes_the_groups(hip_backend):
    """The gait task's groups (critic = policy + critic rows) through the storage: one launch per batch, raw rows kept."""
    env, st, policy, state = _norm_setup("gait", 96, 6, "cuda")
    last = _norm_collect(env, st, policy, state)
    with torch.no_grad():
        st.compute_returns(policy.evaluate(last))
    an, cn = policy.actor_obs_normalizer, policy.critic_obs_normalizer
    seed = lambda: torch.Generator(device="cuda").manual_seed(2)
    plain = list(st.mini_batch_generator(3, 1, generator=seed()))
    normed = list(st.mini_batch_generator(3, 1, generator=seed(), obs_normalizer=an, critic_obs_normalizer=cn))
    for p, q in zip(plain, normed):
        assert torch.equal(p.indices, q.indices) and torch.equal(p.actions, q.actions) and torch.equal(p.returns, q.returns)
        assert torch.equal(q.obs.cpu(), _normalized_on_cpu(an, p.obs)) and torch.equal(q.critic_obs.cpu(), _normalized_on_cpu(cn, p.critic_obs))
    assert float(an._var.min()) >= 0.0 and int(an.count) == 6 * 96


# ---- GPU: end to end ------------------------------------------------------------------------------------------------------------------
class _TorchPath:
    """A backend with none of the learner's entry points: PPO and the storage then run their torch expressions (the path of the
    test-only oracle backend) on whatever device the tensors live on."""
    name, device_type = "torch-path", "cuda"


@pytest.mark.gpu
def test_update_with_normalizers_hip_against_the_torch_path(hip_backend):
    """``PPO.update`` with both normalisers: the HIP path against the oracle-backend (torch) path on the same rollout, the same
    minibatch stream and the same starting weights.  rtol=1e-6, atol=1e-7 on the parameters and the Adam state; one host read."""
    from genesis_forge_amd import _native as nat
    from genesis_forge_amd.learner import PPO

    env, st, policy, state = _norm_setup("go2", 256, 24, "cuda")
    last = _norm_collect(env, st, policy, state)
    ref_policy = copy.deepcopy(policy)
    ppo, ref = PPO(policy, st, **ALGO), PPO(ref_policy, st, **ALGO)
    ppo.compute_returns(last)
    with host_reads() as c:
        got = ppo.update(generator=torch.Generator(device="cuda").manual_seed(10))
    assert c[0] == 1, f"PPO.update read the device {c[0]} times"
    nat.set_backend(_TorchPath())
    try:
        want = ref.update(generator=torch.Generator(device="cuda").manual_seed(10))
    finally:
        nat.set_backend(hip_backend)
    print("losses", got, want, "lr", ppo.learning_rate, ref.learning_rate)
    for name, a, b in (("params", ppo.params, ref.params), ("exp_avg", ppo.exp_avg, ref.exp_avg), ("exp_avg_sq", ppo.exp_avg_sq, ref.exp_avg_sq)):
        d = (a - b).abs()
        print(f"{name}: max |d| = {float(d.max()):.3e}, max |d| / (1e-7 + 1e-6 |ref|) = {float((d / (1e-7 + 1e-6 * b.abs())).max()):.3f}")
    for name, a, b in (("params", ppo.params, ref.params), ("exp_avg", ppo.exp_avg, ref.exp_avg), ("exp_avg_sq", ppo.exp_avg_sq, ref.exp_avg_sq)):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7, msg=lambda m, name=name: f"{name}: {m}")


@pytest.mark.gpu
def test_collection_loop_with_normalizers(hip_backend):
    """act_policy -> env.step -> update_normalization -> process_env_step on a Go2 env: the statistics count every row, and the
    stored ``mu`` of every transition is the forward of the observation normalised with the statistics of that moment."""
    from genesis_forge_amd.learner import PolicyForward

    n, T = 256, 8
    env, st, policy, state = _norm_setup("go2", n, T, "cuda")
    fwd = PolicyForward(policy)
    fwd_plain = PolicyForward(types.SimpleNamespace(actor=policy.actor, critic=policy.critic, std=policy.std))
    obs, _extras = state
    want_mu, want_v = [], []
    for _ in range(T):
        want_mu.append(fwd_plain.mean(_normalized_on_cpu(policy.actor_obs_normalizer, obs).cuda()))
        want_v.append(fwd_plain.value(_normalized_on_cpu(policy.critic_obs_normalizer, obs).cuda()))
        actions = st.act_policy(fwd, obs)
        obs, _r, _te, tr, _extras = env.step(actions)
        policy.update_normalization(obs)
        st.process_env_step(tr)
    assert int(policy.actor_obs_normalizer.count) == T * n == int(policy.critic_obs_normalizer.count)
    for t in range(T):
        assert torch.equal(st.mu[t], want_mu[t]), f"mu of transition {t}"
        assert torch.equal(st.values[t], want_v[t].reshape(-1)), f"value of transition {t}"
    assert not torch.equal(policy.actor_obs_normalizer._mean, torch.zeros_like(policy.actor_obs_normalizer._mean))
