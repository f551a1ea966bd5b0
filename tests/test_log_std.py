"""rsl_rl's ``noise_std_type="log"`` through every layer: the ``log_std`` flag of gf_policy_act, gf_mlp_act and gf_ppo_loss, and
``ActorCriticMLP`` / ``PolicyForward`` / ``RolloutStorage.act`` / ``PPO`` on a policy that holds ``log_std``.

* CPU: the flag's refusals through the raw ABI (no device), the policy and its config key, the self-check of the float32 bounds
  the GPU loss test uses (torch's float32 autograd of the log-mode expression against float64, no kernel), and ``PPO.update`` on the
  oracle backend against tests/rsl_rl_ppo.py run on a copy of the policy whose ``std`` is ``exp(log_std)``.
* GPU: every kernel in log mode against the SAME kernel in scalar mode fed the sigma the log call stored — one shared ``expf``
  (``policy_sigma``), so the two are related bit for bit, ``grad_log_std == grad_sigma * sigma`` in float32 included — sigma itself
  within 4U of the float64 ``exp``, the loss within the float32 bounds of the float64 reference, and the update end to end."""
import contextlib
import copy
import ctypes as C
import functools
import types

import pytest
import torch

from rsl_rl_ppo import RslRlPPO
from test_learner_edges import CE, CLIP, CV, GRADS, SCALARS, U, _error_over_bound, _loss_bounds, _loss_outputs, _offset_view, _report
from test_mlp_act import _obs, _policy
from test_mlp_edges import _launch as _launch_mlp
from test_ppo_update import ALGO, _env, _flat, _synthetic, _torch_loss, host_reads

E_RANGE = -2


# ---- CPU: the flag's refusals (no device is touched: every call returns before a launch, no pointer is dereferenced) -----------------
def test_flag_refusals_raw_abi():
    from genesis_forge_amd import _native as nat

    assert "std_is_log" in dict(nat.GfPolicyActArgs._fields_) and "std_is_log" in dict(nat.GfMlpActArgs._fields_)
    assert "sigma_is_log" in dict(nat.GfPpoLossArgs._fields_)
    lib = C.CDLL(nat.lib_path())
    lib.gf_sizeof.argtypes, lib.gf_sizeof.restype = [C.c_int], C.c_int
    for idx, st, f in ((nat.GF_SIZEOF_POLICY_ACT, nat.GfPolicyActArgs, lib.gf_policy_act), (nat.GF_SIZEOF_PPO_LOSS, nat.GfPpoLossArgs, lib.gf_ppo_loss),
                       (nat.GF_SIZEOF_MLP_ACT, nat.GfMlpActArgs, lib.gf_mlp_act)):
        assert lib.gf_sizeof(idx) == C.sizeof(st)
        f.restype, f.argtypes = C.c_int, [C.POINTER(st), C.c_void_p]
    lib.gf_abi_version.restype = C.c_int
    assert lib.gf_abi_version() == nat.GF_ABI_VERSION
    PTR = 1 << 20   # (16-byte aligned; never dereferenced)

    def act(**kw):
        a = nat.GfPolicyActArgs()
        a.num_envs, a.num_actions, a.mean, a.std, a.actions = 100, 12, PTR, PTR, PTR
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.gf_policy_act(C.byref(a), None)

    assert act(std_is_log=2) == E_RANGE and act(std_is_log=2, num_envs=0) == E_RANGE
    assert act(std_is_log=1, num_envs=0) == 0 and act(std_is_log=1, std_per_env=1, num_envs=0) == 0

    def loss(**kw):
        a = nat.GfPpoLossArgs()
        a.num_rows, a.num_actions, a.use_clipped_value_loss = 300, 12, 1
        for k in ("mu", "sigma", "value", "actions", "old_log_prob", "advantages", "target_values", "returns", "old_mu", "old_sigma",
                  "grad_mu", "grad_value", "grad_sigma", "out", "workspace"):
            setattr(a, k, PTR)
        a.workspace_bytes = nat.ppo_loss_workspace_bytes(300, 12)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.gf_ppo_loss(C.byref(a), None)

    assert loss(sigma_is_log=2) == E_RANGE and loss(sigma_is_log=-1) == E_RANGE and loss(sigma_is_log=2, num_rows=0) == E_RANGE
    assert loss(sigma_is_log=1, num_rows=0) == 0

    def mlp(**kw):
        a = nat.GfMlpActArgs()
        a.num_envs = 0
        for net, out in ((a.actor, 12), (a.critic, 1)):
            net.num_layers, net.num_inputs = 2, 1
            net.inputs[0].rows, net.inputs[0].width = PTR, 8
            for lay, w in zip(net.layers, (16, out)):
                lay.weight, lay.bias, lay.out_width = PTR, PTR, w
        a.std, a.actions, a.mean, a.values = PTR, PTR, PTR, PTR
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.gf_mlp_act(C.byref(a), None)

    assert mlp(std_is_log=2) == E_RANGE and mlp(std_is_log=-1) == E_RANGE and mlp(std_is_log=2, num_envs=100) == E_RANGE
    assert mlp(std_is_log=1) == 0 and mlp(std_is_log=1, std=None, actions=None) == 0
    assert mlp(std_is_log=1, std_per_env=2) == E_RANGE, "std_per_env keeps its range"


# ---- CPU: the policy ---------------------------------------------------------------------------------------------------------------
def test_policy_log_std_parameter_and_config():
    from genesis_forge_amd.learner import ActorCriticMLP, PolicyForward

    cfg = {"policy": {"class_name": "ActorCritic", "activation": "elu", "actor_hidden_dims": [32, 16], "critic_hidden_dims": [32, 16],
                      "init_noise_std": 0.8, "noise_std_type": "log"}}
    log = ActorCriticMLP.from_train_cfg(cfg, 48, 12)
    scalar = ActorCriticMLP.from_train_cfg({"policy": dict(cfg["policy"], noise_std_type="scalar")}, 48, 12)
    assert log.noise_std_type == "log" and scalar.noise_std_type == "scalar"
    assert isinstance(log.log_std, torch.nn.Parameter) and torch.equal(log.log_std.detach(), torch.log(0.8 * torch.ones(12)))
    assert not hasattr(log, "std") and not hasattr(scalar, "log_std")
    names_log, names_scalar = [k for k, _ in log.named_parameters()], [k for k, _ in scalar.named_parameters()]
    assert names_log == ["log_std" if k == "std" else k for k in names_scalar] and "log_std" in names_log
    assert [tuple(p.shape) for p in log.parameters()] == [tuple(p.shape) for p in scalar.parameters()]
    assert "log_std" in log.state_dict() and "std" not in log.state_dict()
    assert torch.equal(log.action_std, log.log_std.detach().exp()) and not log.action_std.requires_grad
    assert torch.equal(scalar.action_std, scalar.std.detach()) and torch.allclose(log.action_std, scalar.action_std, rtol=1e-6, atol=0)
    assert ActorCriticMLP(48, 12).noise_std_type == "scalar"
    for bad in ("exp", "LOG", None):
        with pytest.raises(ValueError, match="noise_std_type"):
            ActorCriticMLP.from_train_cfg({"policy": dict(cfg["policy"], noise_std_type=bad)}, 48, 12)
        with pytest.raises(ValueError, match="noise_std_type"):
            ActorCriticMLP(48, 12, noise_std_type=bad)
    with pytest.raises(ValueError, match="activation"):   # (the other refusals stay)
        ActorCriticMLP.from_train_cfg({"policy": dict(cfg["policy"], activation="relu")}, 48, 12)
    # PolicyForward picks the parameter by the policy's type — a foreign policy with rsl_rl's attribute names too
    assert PolicyForward(log).std_param() == (log.log_std, True) and PolicyForward(log).num_actions == 12
    assert PolicyForward(scalar).std_param() == (scalar.std, False)
    foreign = types.SimpleNamespace(actor=log.actor, critic=log.critic, log_std=torch.zeros(12), noise_std_type="log")
    p, is_log = PolicyForward(foreign).std_param()
    assert p is foreign.log_std and is_log and PolicyForward(foreign).num_actions == 12
    with pytest.raises(ValueError, match="log_std"):
        PolicyForward(types.SimpleNamespace(actor=log.actor, critic=log.critic, log_std=torch.zeros(11), noise_std_type="log"))


# ---- gf_ppo_loss in log mode: the float64 reference and the float32 bounds -------------------------------------------------------------
def _torch_loss_log(inp, log_std, clipped):
    """test_ppo_update._torch_loss with ``sigma = exp(log_std)`` inside the graph: rsl_rl's noise_std_type="log" expression."""
    mu = inp["mu"].clone().requires_grad_(True)
    value = inp["value"].clone().requires_grad_(True)
    ls = log_std.clone().requires_grad_(True)
    sigma = torch.exp(ls).expand_as(mu)
    d = torch.distributions.Normal(mu, sigma, validate_args=False)
    logp = d.log_prob(inp["actions"]).sum(dim=-1)
    ent = d.entropy().sum(dim=-1)
    with torch.no_grad():
        kl = torch.sum(torch.log(sigma / inp["old_sigma"] + 1.0e-5) + (torch.square(inp["old_sigma"]) + torch.square(inp["old_mu"] - mu))
                       / (2.0 * torch.square(sigma)) - 0.5, axis=-1).mean()
    ratio = torch.exp(logp - inp["old_log_prob"])
    adv = inp["advantages"]
    surr = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP)).mean()
    if clipped:
        vc = inp["target_values"] + (value - inp["target_values"]).clamp(-CLIP, CLIP)
        vl = torch.max((value - inp["returns"]).pow(2), (vc - inp["returns"]).pow(2)).mean()
    else:
        vl = (inp["returns"] - value).pow(2).mean()
    loss = surr + CV * vl - CE * ent.mean()
    loss.backward()
    return dict(surrogate=surr.detach(), value_loss=vl.detach(), entropy=ent.mean().detach(), kl_mean=kl, loss=loss.detach(),
                grad_mu=mu.grad, grad_value=value.grad, grad_sigma=ls.grad, ratio=ratio.detach())


@functools.lru_cache(maxsize=2)   # (the largest case holds some 30 MB)
def _log_case(mb, A, clipped):
    """One shape's float32 inputs (CPU) with ``log_std = sigma.log()`` in float32, the float64 reference of the case whose sigma is
    ``exp(log_std)`` evaluated in float64, and the bounds: test_learner_edges._loss_bounds on those float64 inputs, the grad_sigma
    bound replaced by that of ``grad_log_std = grad_sigma * sigma`` — the scalar bound times sigma, plus 8U of the result (the
    float32 ``expf``, up to 2U, enters the product once and the reciprocals of the sum's terms up to three times; one rounding of the
    product) and 4U·CE (the entropy term ``-CE / sigma * sigma`` of magnitude CE).  Computed once, shared, never written."""
    inp = _synthetic(mb, A, "cpu", seed=1)
    log_std = inp["sigma"].log()
    assert log_std.dtype == torch.float32
    inp64 = {k: v.double() for k, v in inp.items()}
    inp64["sigma"] = log_std.double().exp()
    ref = _torch_loss(inp64, clipped)
    ref["grad_sigma"] = ref["grad_sigma"] * inp64["sigma"]   # d loss / d log_std
    via_graph = _torch_loss_log(inp64, log_std.double(), clipped)["grad_sigma"]
    assert torch.allclose(ref["grad_sigma"], via_graph, rtol=1e-9, atol=1e-12 * float(via_graph.abs().max())), "exp's backward"
    assert all(ref[k].dtype == torch.float64 for k in SCALARS + GRADS)
    r = ref["ratio"]
    assert float(torch.minimum((r - (1 - CLIP)).abs(), (r - (1 + CLIP)).abs()).min()) > 1e-4, "a ratio within 1e-4 of 1 ± clip"
    assert float(((inp64["value"] - inp64["target_values"]).abs() - CLIP).abs().min()) > 1e-4, "a |v - tv| within 1e-4 of clip"
    if mb >= 255:
        assert bool((r < 1 - CLIP).any()) and bool((r > 1 + CLIP).any()) and bool(((r > 1 - CLIP) & (r < 1 + CLIP)).any())
    b = _loss_bounds(inp64, ref, clipped)
    b["grad_sigma"] = b["grad_sigma"] * inp64["sigma"] + 8 * U * ref["grad_sigma"].abs() + 4 * U * CE
    return inp, log_std, ref, b


@pytest.mark.parametrize("A", [1, 3, 4, 13, 16, 37, 64])
@pytest.mark.parametrize("mb", [1, 255, 256, 257, 16385])
@pytest.mark.parametrize("clipped", [True, False])
def test_log_loss_bounds_hold_torch_f32_cpu(A, mb, clipped):
    """The self-check of the bounds and the inputs the GPU test below uses (no kernel runs): torch's float32 autograd of the log-mode
    expression stays at or below half of every bound."""
    inp, log_std, ref, bounds = _log_case(mb, A, clipped)
    worst = _error_over_bound(_torch_loss_log(inp, log_std, clipped), ref, bounds)
    _report("log_std torch_f32", mb, A, clipped, worst)
    for k, v in worst.items():
        assert v <= 0.5, f"A={A} mb={mb} clipped={clipped}: torch f32 {k} at {v:.3f} of its bound"


# ---- PPO.update on a log_std policy against rsl_rl's loop ----------------------------------------------------------------------------
def _as_rsl_rl(policy):
    """A deep copy of a log_std policy for tests/rsl_rl_ppo.py: its ``std`` is ``exp(log_std)`` — what rsl_rl's distribution update
    computes — so autograd reaches log_std."""
    class _StdFromLog(type(policy)):
        std = property(lambda self: self.log_std.exp())

    ref = copy.deepcopy(policy)
    ref.__class__ = _StdFromLog
    return ref


@contextlib.contextmanager
def _recorded_kl(into):
    """Records the float32 ``kl_mean`` of every minibatch of an RslRlPPO.update: its ``torch.mean(kl)`` is the update's only call of
    the function ``torch.mean`` (the losses use the method)."""
    saved = torch.mean

    def mean(*a, **k):
        out = saved(*a, **k)
        into.append(float(out))
        return out

    torch.mean = mean
    try:
        yield
    finally:
        torch.mean = saved


def _log_end_to_end(dev, n, T, iterations=2, noise_gen=None, check=True):
    """test_ppo_update._end_to_end on a noise_std_type="log" policy: collect (``act`` with the given noise on a backend that cannot
    draw, ``act_policy`` otherwise), update the policy with PPO and its copy with rsl_rl's loop on the same minibatch stream; the
    same tolerances.  Returns (the flat parameters, PPO.update's host reads per iteration)."""
    from genesis_forge_amd.learner import PPO, ActorCriticMLP, PolicyForward, RolloutStorage

    env = _env("go2", n)
    obs, extras = env.reset()
    st = RolloutStorage(env, T).attach()
    st.begin(obs, extras)
    st.seed(5)
    A = env.action_space.shape[0]
    torch.manual_seed(0)
    policy = ActorCriticMLP(st.obs_width, A, (64, 32), (64, 32), init_noise_std=0.8, noise_std_type="log").to(dev)
    ref_policy = _as_rsl_rl(policy)
    fwd = PolicyForward(policy)
    ppo, ref = PPO(policy, st, **ALGO), RslRlPPO(ref_policy, st, **ALGO)
    reads = []
    for it in range(iterations):
        for _ in range(T):
            if noise_gen is None:
                actions = st.act_policy(fwd, obs)
            else:
                with torch.no_grad():
                    mean, values = policy.act_mean(obs), policy.evaluate(obs)
                actions = st.act(mean, policy.log_std.detach(), values, noise=torch.randn(n, A, generator=noise_gen).to(dev), std_is_log=True)
            obs, _r, _te, tr, extras = env.step(actions)
            st.process_env_step(tr)
        # the sigma rows hold std, never log_std (rsl_rl's action_std): the last transition's row
        sigma_row = st.sigma[T - 1]
        assert torch.allclose(sigma_row, policy.action_std.expand_as(sigma_row), rtol=4 * U, atol=0) and bool((sigma_row > 0).all())
        ppo.compute_returns(obs)
        if check:
            kls = []
            with _recorded_kl(kls):
                want = ref.update(generator=torch.Generator(device=dev).manual_seed(10 + it))
            assert len(kls) == ALGO["num_learning_epochs"] * ALGO["num_mini_batches"]
            # equal learning rates need every KL clear of the schedule's two thresholds
            for kl in kls:
                for edge in (2.0 * ALGO["desired_kl"], ALGO["desired_kl"] / 2.0):
                    assert abs(kl - edge) > 1e-3 * edge, f"iteration {it}: a minibatch KL of the reference run ({kl}) within 1e-3 of {edge}: pick another seed"
        with host_reads() as c:
            got = ppo.update(generator=torch.Generator(device=dev).manual_seed(10 + it))
        reads.append(c[0])
        if check:
            for k in ("value_function", "surrogate", "entropy"):
                assert abs(got[k] - want[k]) <= 1e-4 * max(abs(want[k]), 1e-6), f"iteration {it}: {k} {got[k]} vs {want[k]}"
            assert ppo.learning_rate == ref.learning_rate, f"iteration {it}: lr {ppo.learning_rate} vs {ref.learning_rate}"
    if check:   # test_ppo_update._end_to_end's parameter criteria, on all parameters and on log_std alone
        steps = iterations * ALGO["num_learning_epochs"] * ALGO["num_mini_batches"]
        assert not torch.equal(policy.log_std.detach(), torch.log(0.8 * torch.ones(A, device=dev))), "log_std was trained"
        for what, a, b in (("all", _flat(policy), _flat(ref_policy)), ("log_std", policy.log_std.detach(), ref_policy.log_std.detach())):
            d = (a - b).abs()
            bulk = float((d <= 1e-4 + 1e-3 * b.abs()).float().mean())
            assert bulk >= 0.995, f"{what}: only {bulk:.4f} of the parameters agree to 1e-4 + 1e-3|p| (max diff {float(d.max())})"
            assert float(d.max()) <= 2 * 3.2 * 1e-2 * steps, what
    st.detach()
    return _flat(policy).clone(), reads


def test_log_std_update_end_to_end_cpu(oracle_backend):
    _params, reads = _log_end_to_end("cpu", 70, 8, noise_gen=torch.Generator().manual_seed(4))
    assert reads == [1, 1], f"PPO.update read the host {reads} times"


def test_ppo_takes_either_parameter_and_refuses_neither(oracle_backend):
    from genesis_forge_amd.learner import PPO, ActorCriticMLP, RolloutStorage

    env = _env("go2", 16)
    st = RolloutStorage(env, 4)
    policy = ActorCriticMLP(st.obs_width, 12, (16,), (16,), noise_std_type="log")
    ppo = PPO(policy, st, **ALGO)
    assert ppo.num_actions == 12 and policy.log_std.data_ptr() >= ppo.params.data_ptr(), "log_std lives in the flat buffer"
    assert policy.log_std.data_ptr() < ppo.params.data_ptr() + 4 * ppo.params.numel()
    for broken in (types.SimpleNamespace(noise_std_type="log", std=torch.ones(12)), types.SimpleNamespace(log_std=torch.zeros(12)), types.SimpleNamespace()):
        with pytest.raises(ValueError, match="log_std"):
            PPO(broken, st, **ALGO)


# ---- GPU: gf_policy_act ---------------------------------------------------------------------------------------------------------------
def _act_raw(backend, mean, std, values, noise, is_log):
    """gf_policy_act through the raw ABI into fresh outputs: (actions, actions_out, mu, sigma, values, log_prob)."""
    from genesis_forge_amd import _native as nat

    n, A = mean.shape
    outs = [torch.full((n, A), 7.0, device=mean.device) for _ in range(4)] + [torch.full((n,), 7.0, device=mean.device) for _ in range(2)]
    a = nat.GfPolicyActArgs()
    a.num_envs, a.num_actions, a.std_per_env, a.std_is_log = n, A, 1 if std.dim() == 2 else 0, int(is_log)
    a.mean, a.std, a.values, a.noise = mean.data_ptr(), std.data_ptr(), values.data_ptr(), noise.data_ptr()
    a.seed, a.stream, a.env_offset = 1, 0, 0
    a.actions, a.actions_out, a.mu_out, a.sigma_out, a.values_out, a.log_prob_out = (o.data_ptr() for o in outs)
    backend.policy_act(a)
    torch.cuda.synchronize()
    return outs


def _log_std_values(shape, zero_col, seed):
    """Uniform in [-5, 2] (sigma from 0.007 to 7.4), column ``zero_col`` exactly 0."""
    ls = torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 7.0 - 5.0
    ls[..., zero_col] = 0.0
    return ls.cuda()


def _assert_sigma(sigma, log_std, zero_col):
    """Within 4U relative of the float64 exp: one float32 ulp — up to 2U relative — for expf's documented error, the rounding of the
    reference to float32 spacing and slack of 1U; exp(0) is exact."""
    want = log_std.double().exp().expand_as(sigma)
    assert bool(((sigma.double() - want).abs() <= 4 * U * want).all()), f"sigma off exp(log_std) by {float(((sigma.double() - want).abs() / want).max() / U):.2f} U"
    assert bool((sigma[..., zero_col] == 1.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("A,misaligned", [(3, False), (4, False), (12, False), (4, True)])
@pytest.mark.parametrize("std_rows", [False, True])
def test_policy_act_log_mode(hip_backend, n, A, misaligned, std_rows):
    g = torch.Generator().manual_seed(100 * n + A)
    mean, values, noise = (torch.randn(s, generator=g).cuda() for s in ((n, A), (n,), (n, A)))
    zero_col = A // 2
    log_std = _log_std_values((n, A) if std_rows else (A,), zero_col, seed=n + A)
    keep = None
    if misaligned:   # (the scalar kernel on a shape the vector kernel normally takes)
        keep, log_std = _offset_view(log_std)
    else:
        assert log_std.data_ptr() % 16 == 0
    got = _act_raw(hip_backend, mean, log_std, values, noise, True)
    sigma = got[3]
    _assert_sigma(sigma, log_std, zero_col)
    assert torch.equal(got[2], mean) and torch.equal(got[4], values) and torch.equal(got[0], got[1])
    assert bool(torch.isfinite(got[5]).all()) and bool((got[5] != 7.0).all())
    # scalar mode fed that sigma: the same bits everywhere
    std = sigma.contiguous() if std_rows else sigma[0].contiguous()
    if not std_rows:
        assert torch.equal(sigma, std.expand(n, A)), "every row holds the same sigma"
    again = _act_raw(hip_backend, mean, std, values, noise, False)
    for name, x, y in zip(("actions", "actions_out", "mu_out", "sigma_out", "values_out", "log_prob_out"), got, again):
        assert torch.equal(x, y), name
    if misaligned:
        aligned = _act_raw(hip_backend, mean, log_std.clone(), values, noise, True)
        for x, y in zip(got, aligned):
            assert torch.equal(x, y), "the scalar and the vector kernel exponentiate alike"
        assert float(keep[0]) == 7.0 and bool((keep[1 + log_std.numel():] == 7.0).all())


# ---- GPU: gf_mlp_act --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("A", [3, 12])
@pytest.mark.parametrize("both", [True, False])
def test_mlp_act_log_mode(hip_backend, A, both):
    """33 rows: two tiles, one of a single row.  The descriptor is PolicyForward's own (test_mlp_edges._launch leaves the flag as it
    finds it), every output between guard floats."""
    from genesis_forge_amd.learner import PolicyForward

    n, segs = 33, (8,)
    fwd = PolicyForward(_policy(segs, (16,), A, "cuda", seed=2))
    obs = _obs(segs, n, "cuda", seed=3)
    cobs = obs if both else None
    zero_col = A // 2
    log_std = _log_std_values((A,), zero_col, seed=A)
    noise = torch.randn(n, A, generator=torch.Generator().manual_seed(8)).cuda()
    try:
        fwd._args.std_is_log = 1
        got = _launch_mlp(hip_backend, fwd, n, obs, cobs, std=log_std, noise=noise)
        mean_only = _launch_mlp(hip_backend, fwd, n, obs, None)   # actions == NULL with the flag set: the mean, nothing drawn
    finally:
        fwd._args.std_is_log = 0
    _assert_sigma(got["sigma_out"], log_std, zero_col)
    assert torch.equal(got["sigma_out"], got["sigma_out"][0].expand(n, A))
    assert torch.equal(mean_only["mean"], got["mean"]) and set(mean_only) == {"mean"}
    again = _launch_mlp(hip_backend, fwd, n, obs, cobs, std=got["sigma_out"][0].contiguous(), noise=noise)
    assert set(got) == set(again) and ("values" in got) == both
    for k in got:
        assert torch.equal(got[k], again[k]), k
    # gf_policy_act in log mode on the kernel's own mean: the same row code
    values = got["values"] if both else torch.zeros(n, device="cuda")
    q = _act_raw(hip_backend, got["mean"].contiguous(), log_std, values.contiguous(), noise, True)
    for k, x in zip(("actions", "actions_out", "mu_out", "sigma_out"), q):
        assert torch.equal(got[k], x), k
    assert torch.equal(got["log_prob_out"], q[5])


# ---- GPU: gf_ppo_loss ---------------------------------------------------------------------------------------------------------------------
def _loss_raw(backend, t, mb, A, clipped, is_log):
    """gf_ppo_loss on the tensors of ``t`` as they lie (grad_* may be missing: NULL)."""
    from genesis_forge_amd import _native as nat

    ws = torch.empty(max(1, nat.ppo_loss_workspace_bytes(mb, A) // 8), device=t["mu"].device, dtype=torch.float64)
    a = nat.GfPpoLossArgs()
    a.num_rows, a.num_actions, a.use_clipped_value_loss, a.sigma_is_log = mb, A, int(clipped), int(is_log)
    for k in ("mu", "sigma", "value", "actions", "old_log_prob", "advantages", "target_values", "returns", "old_mu", "old_sigma", "out"):
        setattr(a, k, t[k].data_ptr())
    for k in GRADS:
        setattr(a, k, t[k].data_ptr() if k in t else None)
    a.clip_param, a.value_loss_coef, a.entropy_coef = CLIP, CV, CE
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 8
    backend.ppo_loss(a)
    torch.cuda.synchronize()


def _as_dict(t):
    o = t["out"]
    return dict(surrogate=o[0], value_loss=o[1], entropy=o[2], kl_mean=o[3], loss=o[4], **{k: t[k] for k in GRADS if k in t})


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 3, 4, 13, 16, 64])
@pytest.mark.parametrize("mb", [1, 257, 16385])
@pytest.mark.parametrize("clipped", [True, False])
def test_loss_kernel_log_mode(hip_backend, A, mb, clipped):
    inp, log_std, ref, bounds = _log_case(mb, A, clipped)
    dev = {k: v.cuda() for k, v in inp.items()}
    log_std = log_std.cuda()
    assert log_std.data_ptr() % 16 == 0
    # (a) within the float32 bounds of the float64 reference; the workspace is only scratch: a second call gives the same bits
    got = _loss_outputs(mb, A)
    _loss_raw(hip_backend, {**dev, "sigma": log_std, **got}, mb, A, clipped, True)
    worst = _error_over_bound(_as_dict(got), ref, bounds)
    _report("log_std kernel", mb, A, clipped, worst)
    for k, v in worst.items():
        assert v <= 1.0, f"A={A} mb={mb} clipped={clipped}: {k} at {v:.3f} of its bound"
    again = _loss_outputs(mb, A)
    _loss_raw(hip_backend, {**dev, "sigma": log_std, **again}, mb, A, clipped, True)
    for k in ("out",) + GRADS:
        assert torch.equal(got[k], again[k]), k
    # (b) scalar mode on the kernel's own sigma (a one-env gf_policy_act log call stores it): the same bits, and exp's backward
    # is one float32 product
    one = torch.zeros(1, A, device="cuda")
    sigma = _act_raw(hip_backend, one, log_std, torch.zeros(1, device="cuda"), one, True)[3][0].contiguous()
    scalar = _loss_outputs(mb, A)
    _loss_raw(hip_backend, {**dev, "sigma": sigma, **scalar}, mb, A, clipped, False)
    for k in ("out", "grad_mu", "grad_value"):
        assert torch.equal(got[k], scalar[k]), k
    assert torch.equal(got["grad_sigma"], scalar["grad_sigma"] * sigma), "grad_log_std == grad_sigma * sigma in float32"
    # (c) loss-only mode: the same five scalars
    only = _loss_outputs(mb, A, grads=False)
    _loss_raw(hip_backend, {**dev, "sigma": log_std, **only}, mb, A, clipped, True)
    assert torch.equal(only["out"], got["out"])
    # (d) a misaligned log_std on A = 4: the scalar kernel, the same bits
    if A == 4:
        keep, off = _offset_view(log_std)
        mis = _loss_outputs(mb, A)
        _loss_raw(hip_backend, {**dev, "sigma": off, **mis}, mb, A, clipped, True)
        for k in ("out",) + GRADS:
            assert torch.equal(got[k], mis[k]), k
        assert float(keep[0]) == 7.0 and bool((keep[1 + A:] == 7.0).all())


# ---- GPU: end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_log_std_update_end_to_end_hip(hip_backend):
    """Collection through act_policy (gf_mlp_act), PPO.update through gf_ppo_loss / gf_adam_step, against rsl_rl's loop; one host read
    per update; a second identical run (without the reference) ends on the same bits."""
    first, reads = _log_end_to_end("cuda", 384, 24)
    assert reads == [1, 1], f"PPO.update read the host {reads} times"
    second, _ = _log_end_to_end("cuda", 384, 24, check=False)
    assert torch.equal(first, second)
