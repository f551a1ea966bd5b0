"""learner.PPO — rsl_rl's PPO.update with the loss, its gradient, the adaptive lr, clip_grad_norm_ and Adam in HIP (gf_ppo_loss,
gf_adam_step), and no host synchronisation per minibatch.

* gf_ppo_loss against torch autograd of rsl_rl's expression (real Go2 minibatches and synthetic rows with ratios outside both
  clip bounds and |v - target| on both sides of eps; vector and scalar column paths);
* gf_adam_step against clip_grad_norm_ + torch.optim.Adam(foreach=True), and its lr schedule bit for bit against rsl_rl's rule;
* PPO.update end to end against tests/rsl_rl_ppo.py on the same minibatch stream, its host reads, determinism, a one-rank RCCL
  group; on the CPU oracle backend the same arithmetic runs in torch (schedule, end to end, host reads, two gloo ranks)."""
import contextlib
import ctypes as C
import math
import os
import socket
import tempfile

import pytest
import torch
import torch.multiprocessing as mp

from rsl_rl_ppo import RslRlPPO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGO = dict(class_name="PPO", clip_param=0.2, desired_kl=0.01, entropy_coef=0.01, gamma=0.99, lam=0.95, learning_rate=0.001, max_grad_norm=1.0,
            num_learning_epochs=5, num_mini_batches=4, schedule="adaptive", use_clipped_value_loss=True, value_loss_coef=1.0)   # examples/*/train.py
GAIT_GROUPS = {"policy": ["policy"], "critic": ["policy", "critic"]}


# ---- host-read witness ------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def host_reads():
    """Counts the calls that read a tensor back to the host (or wait for the device): Tensor.item / tolist / cpu / __bool__ /
    __float__ and torch.cuda.synchronize."""
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


# ---- rollouts -----------------------------------------------------------------------------------------------------------------------
def _env(kind, n):
    from genesis_forge_amd import tasks

    if kind == "go2":
        env = tasks.Go2CommandDirectionEnv(num_envs=n, max_episode_length_s=0.4, cmd_resample_s=0.2, scene_kwargs=dict(ang_noise=0.3, seed=3))
    else:
        env = tasks.Go2GaitTrainingEnv(num_envs=n, max_episode_length_s=0.4, scene_kwargs=dict(ang_noise=0.3, seed=3, contact_prob=0.05))
    env.build()
    env.seed(7)
    return env


def _setup(kind, n, T, dev, hidden=(64, 32), seed=0):
    from genesis_forge_amd.learner import ActorCriticMLP, RolloutStorage

    env = _env(kind, n)
    obs, extras = env.reset()
    groups = GAIT_GROUPS if kind == "gait" else None
    st = RolloutStorage(env, T, obs_groups=groups).attach()
    st.begin(obs, extras)
    st.seed(5)
    A = env.action_space.shape[0]
    critic_w = sum(st.group_rows[m].shape[2] for m in st.obs_groups["critic"])
    torch.manual_seed(seed)
    policy = ActorCriticMLP(st.obs_width, A, hidden, hidden, init_noise_std=0.8).to(dev)
    if critic_w != st.obs_width:   # the asymmetric critic reads the concatenated group
        policy.critic = ActorCriticMLP(critic_w, A, hidden, hidden).critic.to(dev)
    return env, st, policy, [obs, extras]


def _collect(env, st, policy, state, noise_gen=None):
    """One rollout: act -> env.step -> process_env_step, T times (noise from ``noise_gen`` on backends that cannot draw)."""
    obs, extras = state
    n, A = env.num_envs, env.action_space.shape[0]
    critic = st.obs_groups["critic"]
    for _ in range(st.num_steps):
        with torch.no_grad():
            cobs = obs if critic == st.obs_groups["policy"] else torch.cat([extras["observations"][m] for m in critic], dim=-1)
            mean, values = policy.act_mean(obs), policy.evaluate(cobs)
        noise = None if noise_gen is None else torch.randn(n, A, generator=noise_gen).to(mean.device)
        actions = st.act(mean, policy.std.detach(), values, noise=noise)
        obs, _r, _te, tr, extras = env.step(actions)
        st.process_env_step(tr)
    state[0], state[1] = obs, extras
    cobs = obs if critic == st.obs_groups["policy"] else torch.cat([extras["observations"][m] for m in critic], dim=-1)
    return cobs


def _flat(policy):
    return torch.cat([p.detach().reshape(-1) for p in policy.parameters()])


# ---- gf_ppo_loss vs torch autograd ----------------------------------------------------------------------------------------------
def _torch_loss(inp, clipped, clip=0.2, cv=1.0, ce=0.01):
    mu = inp["mu"].clone().requires_grad_(True)
    value = inp["value"].clone().requires_grad_(True)
    std = inp["sigma"].clone().requires_grad_(True)
    sigma = std.expand_as(mu)
    d = torch.distributions.Normal(mu, sigma, validate_args=False)
    logp = d.log_prob(inp["actions"]).sum(dim=-1)
    ent = d.entropy().sum(dim=-1)
    with torch.no_grad():
        kl = torch.sum(torch.log(sigma / inp["old_sigma"] + 1.0e-5) + (torch.square(inp["old_sigma"]) + torch.square(inp["old_mu"] - mu))
                       / (2.0 * torch.square(sigma)) - 0.5, axis=-1).mean()
    ratio = torch.exp(logp - inp["old_log_prob"])
    adv = inp["advantages"]
    surr = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)).mean()
    if clipped:
        vc = inp["target_values"] + (value - inp["target_values"]).clamp(-clip, clip)
        vl = torch.max((value - inp["returns"]).pow(2), (vc - inp["returns"]).pow(2)).mean()
    else:
        vl = (inp["returns"] - value).pow(2).mean()
    loss = surr + cv * vl - ce * ent.mean()
    loss.backward()
    return dict(surrogate=surr.detach(), value_loss=vl.detach(), entropy=ent.mean().detach(), kl_mean=kl, loss=loss.detach(),
                grad_mu=mu.grad, grad_value=value.grad, grad_sigma=std.grad, ratio=ratio.detach())


def _raw_loss(backend, inp, clipped, clip=0.2, cv=1.0, ce=0.01, sums=None):
    from genesis_forge_amd import _native as nat

    mb, A = inp["mu"].shape
    dev = inp["mu"].device
    out = {"grad_mu": torch.full((mb, A), 7.0, device=dev), "grad_value": torch.full((mb,), 7.0, device=dev),
           "grad_sigma": torch.full((A,), 7.0, device=dev), "out": torch.zeros(5, device=dev)}
    ws = torch.empty(max(1, nat.ppo_loss_workspace_bytes(mb, A) // 8), device=dev, dtype=torch.float64)
    a = nat.GfPpoLossArgs()
    a.num_rows, a.num_actions, a.use_clipped_value_loss = mb, A, int(clipped)
    for k in ("mu", "sigma", "value", "actions", "old_log_prob", "advantages", "target_values", "returns", "old_mu", "old_sigma"):
        setattr(a, k, inp[k].data_ptr())
    a.clip_param, a.value_loss_coef, a.entropy_coef = clip, cv, ce
    a.grad_mu, a.grad_value, a.grad_sigma, a.out = (out[k].data_ptr() for k in ("grad_mu", "grad_value", "grad_sigma", "out"))
    a.sums = None if sums is None else sums.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 8
    backend.ppo_loss(a)
    o = out["out"]
    return dict(surrogate=o[0], value_loss=o[1], entropy=o[2], kl_mean=o[3], loss=o[4], **{k: out[k] for k in ("grad_mu", "grad_value", "grad_sigma")})


def _synthetic(mb, A, dev, seed):
    """Rows whose ratio lies well outside both clip bounds (and inside), |v - target| on both sides of eps, advantages of both signs."""
    g = torch.Generator().manual_seed(seed * 7919 + mb * 31 + A)
    mu, old_mu = torch.randn(mb, A, generator=g), torch.randn(mb, A, generator=g) * 0.3
    sigma = torch.rand(A, generator=g) * 0.9 + 0.2
    old_sigma = (sigma + torch.rand(mb, A, generator=g) * 0.2 - 0.1).clamp_min(0.05)
    actions = mu + sigma * torch.randn(mb, A, generator=g)
    logp = torch.distributions.Normal(mu, sigma.expand_as(mu), validate_args=False).log_prob(actions).sum(-1)
    r = torch.rand(mb, generator=g) * 1.2 + 0.4                                  # ratios in [0.4, 1.6]: both bounds crossed
    r = torch.where((r - 0.8).abs() < 1e-3, r + 3e-3, r)
    r = torch.where((r - 1.2).abs() < 1e-3, r + 3e-3, r)                          # (kept clear of the bounds by 1e-3)
    tv = torch.randn(mb, generator=g)
    dv = torch.rand(mb, generator=g) * 1.0 - 0.5                                 # |v - target| up to 0.5 on both sides of eps = 0.2
    dv = torch.where((dv.abs() - 0.2).abs() < 1e-3, dv * 1.02, dv)
    inp = dict(mu=mu, sigma=sigma, value=tv + dv, actions=actions, old_log_prob=logp - torch.log(r), advantages=torch.randn(mb, generator=g),
               target_values=tv, returns=tv + torch.randn(mb, generator=g) * 0.5, old_mu=old_mu + mu, old_sigma=old_sigma)
    return {k: v.to(dev).contiguous() for k, v in inp.items()}


def _check_loss(got, want, clip=0.2, what=""):
    for k in ("surrogate", "value_loss", "entropy", "kl_mean", "loss"):
        a, b = float(got[k]), float(want[k])
        assert abs(a - b) <= 1e-5 * max(abs(b), 1e-6), f"{what}{k}: {a} vs {b}"
    # rows whose ratio is within 1e-6 of a clip bound may take the other side of the clamp in one of the two log-prob folds:
    # they are left out of the elementwise check (and the column sums are only checked when there is none)
    near = ((want["ratio"] - (1 - clip)).abs() <= 1e-6) | ((want["ratio"] - (1 + clip)).abs() <= 1e-6)
    keep = ~near
    for k in ("grad_mu", "grad_value"):
        a, b = got[k].reshape(keep.shape[0], -1)[keep], want[k].reshape(keep.shape[0], -1)[keep]
        scale = float(want[k].abs().max())
        assert float((a - b).abs().max()) <= 1e-5 * scale, f"{what}{k}: {(a - b).abs().max()} vs scale {scale}"
    if not bool(near.any()):
        scale = float(want["grad_sigma"].abs().max())
        assert float((got["grad_sigma"] - want["grad_sigma"]).abs().max()) <= 1e-5 * scale, f"{what}grad_sigma"
    return int(near.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("A", [12, 5, 1])
@pytest.mark.parametrize("mb", [1, 255, 24576])
@pytest.mark.parametrize("clipped", [True, False])
def test_loss_kernel_synthetic_rows(hip_backend, A, mb, clipped):
    inp = _synthetic(mb, A, "cuda", seed=1)
    got, want = _raw_loss(hip_backend, inp, clipped), _torch_loss(inp, clipped)
    _check_loss(got, want, what=f"A={A} mb={mb}: ")
    if mb > 1:
        r = want["ratio"]
        assert bool((r < 0.8).any()) and bool((r > 1.2).any()) and bool(((r > 0.8) & (r < 1.2)).any())
    # the workspace is only scratch: a second call gives the same bits
    again = _raw_loss(hip_backend, inp, clipped)
    for k in ("grad_mu", "grad_value", "grad_sigma", "loss"):
        assert torch.equal(got[k], again[k])


_GO2_MB = {}


def _go2_minibatch(dev):
    """A real Go2 rollout (1 024 envs x 24 steps = one minibatch of 24 576 rows) and a policy a few Adam steps away from the one
    that collected it (ratios off 1, the clip engaged on some rows)."""
    if dev not in _GO2_MB:
        env, st, policy, state = _setup("go2", 1024, 24, dev, hidden=(128, 64))
        last = _collect(env, st, policy, state)
        with torch.no_grad():
            st.compute_returns(policy.evaluate(last))
            for p in policy.parameters():
                p.add_(torch.randn_like(p) * 0.02)
        b = next(iter(st.mini_batch_generator(1, 1, generator=torch.Generator(device=dev).manual_seed(0))))
        with torch.no_grad():
            mu, value = policy.act_mean(b.obs), policy.evaluate(b.critic_obs).reshape(-1)
        _GO2_MB[dev] = dict(mu=mu.contiguous(), sigma=policy.std.detach().clone(), value=value.contiguous(), actions=b.actions,
                            old_log_prob=b.old_log_prob, advantages=b.advantages, target_values=b.values, returns=b.returns, old_mu=b.old_mu,
                            old_sigma=b.old_sigma)
    return _GO2_MB[dev]


@pytest.mark.gpu
@pytest.mark.parametrize("mb", [1, 255, 24576])
@pytest.mark.parametrize("clipped", [True, False])
def test_loss_kernel_go2_minibatch(hip_backend, mb, clipped):
    full = _go2_minibatch("cuda")
    inp = {k: (v if k == "sigma" else v[:mb].contiguous()) for k, v in full.items()}
    got, want = _raw_loss(hip_backend, inp, clipped), _torch_loss(inp, clipped)
    _check_loss(got, want, what=f"go2 mb={mb}: ")
    if mb == 24576:
        r = want["ratio"]
        assert bool(((r < 0.8) | (r > 1.2)).any()), "the perturbed policy should engage the clip on some rows"
        assert abs(float(got["kl_mean"]) - float(want["kl_mean"])) <= 1e-6 * abs(float(want["kl_mean"]))


# ---- gf_adam_step vs clip_grad_norm_ + torch.optim.Adam ------------------------------------------------------------------------
def _adam_args(params, grads, m, v, state, ws, parity, kl=None, desired=0.01, max_norm=1.0):
    from genesis_forge_amd import _native as nat

    a = nat.GfAdamArgs()
    a.numel = params.numel()
    a.params, a.grads, a.exp_avg, a.exp_avg_sq, a.state = (t.data_ptr() for t in (params, grads, m, v, state))
    a.kl_mean = None if kl is None else kl.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 8
    a.desired_kl = desired if kl is not None else 0.0
    a.beta1, a.beta2, a.eps, a.max_grad_norm = 0.9, 0.999, 1e-8, max_norm
    a.schedule = nat.GF_ADAM_SCHEDULE_ADAPTIVE if kl is not None else nat.GF_ADAM_SCHEDULE_FIXED
    a.parity = parity
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("clip_active", [True, False])
@pytest.mark.parametrize("offset", [0, 1])
def test_adam_step_matches_torch(hip_backend, clip_active, offset):
    """10 steps on the flat parameters of an ActorCriticMLP (offset 1: a buffer that is not 16-byte aligned and not a multiple of
    four, the scalar path)."""
    from genesis_forge_amd import _native as nat
    from genesis_forge_amd.learner import ActorCriticMLP

    torch.manual_seed(0)
    net = ActorCriticMLP(48, 12).cuda()
    ref = [p.detach().clone().requires_grad_(True) for p in net.parameters()]
    n = sum(p.numel() for p in ref) - offset
    buf = torch.zeros(n + 8, device="cuda")
    params = buf[offset:offset + n]
    params.copy_(torch.cat([p.detach().reshape(-1) for p in ref])[:n])
    if offset:   # (the reference drops the same last element)
        ref[-1] = ref[-1].detach()[:-offset].clone().requires_grad_(True)
    gbuf = torch.zeros(n + 8, device="cuda")
    grads = gbuf[offset:offset + n]
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    state = torch.zeros(4, device="cuda", dtype=torch.int64)
    state.view(torch.float64)[0] = 1e-3
    ws = torch.zeros(max(1, nat.adam_workspace_bytes(n) // 8), device="cuda", dtype=torch.float64)
    opt = torch.optim.Adam(ref, lr=1e-3, foreach=True)
    g = torch.Generator(device="cuda").manual_seed(3)
    for it in range(10):
        gr = torch.randn(n, device="cuda", generator=g) * (0.05 if clip_active else 1e-4) * (1 + it % 3)
        grads.copy_(gr)
        off = 0
        for p in ref:
            p.grad = gr[off:off + p.numel()].view_as(p).clone()
            off += p.numel()
        norm = torch.nn.utils.clip_grad_norm_(ref, 1.0)
        assert (float(norm) > 1.0) == clip_active
        opt.step()
        hip_backend.adam_step(_adam_args(params, grads, m, v, state, ws, it & 1))
        cat = lambda xs: torch.cat([x.reshape(-1) for x in xs])
        torch.testing.assert_close(grads, cat(p.grad for p in ref), rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(params, cat(ref), rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(m, cat(opt.state[p]["exp_avg"] for p in ref), rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(v, cat(opt.state[p]["exp_avg_sq"] for p in ref), rtol=1e-6, atol=1e-7)
    assert int(state[2 * (10 & 1) + 1]) == 10 and float(state.view(torch.float64)[2 * (10 & 1)]) == 1e-3


def _rsl_rl_rule(lr, kl, desired):
    """rsl_rl's lines, with the float32 kl_mean as a tensor (torch compares it with the Python float in float32)."""
    kl_mean = torch.tensor(kl, dtype=torch.float32)
    if kl_mean > desired * 2.0:
        lr = max(1e-5, lr / 1.5)
    elif kl_mean < desired / 2.0 and kl_mean > 0.0:
        lr = min(1e-2, lr * 1.5)
    return lr


def _schedule_kls(desired):
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    kls = [f32(desired / 2.0), f32(desired * 2.0), 0.0, -0.01, f32(desired), 0.05, 0.001]   # ties at both thresholds, kl <= 0
    kls += [1e-4] * 14                  # up to the 1e-2 cap
    kls += [0.5] * 30                   # down to the 1e-5 floor
    kls += [f32(desired / 2.0), 0.003, f32(desired / 2.0) * (1 - 2 ** -20), f32(desired * 2.0) * (1 + 2 ** -20)]
    return kls


@pytest.mark.gpu
def test_adam_lr_schedule_bitwise(hip_backend):
    """gf_adam_step's lr sequence against rsl_rl's rule bit for bit: both thresholds (kl == float32(desired / 2) must NOT raise the
    lr — a comparison in double would), both caps, kl <= 0; and kl == float32(desired / 2) is indeed below desired / 2 in double."""
    from genesis_forge_amd import _native as nat

    desired = 0.01
    f32half = float(torch.tensor(desired / 2.0, dtype=torch.float32))
    assert f32half < desired / 2.0, "the tie case must tell a float32 comparison from a double one"
    n = 1000
    params, grads, m, v = (torch.zeros(n, device="cuda") for _ in range(4))
    state = torch.zeros(4, device="cuda", dtype=torch.int64)
    state.view(torch.float64)[0] = 1e-3
    ws = torch.zeros(max(1, nat.adam_workspace_bytes(n) // 8), device="cuda", dtype=torch.float64)
    kl_t = torch.zeros(1, device="cuda")
    lr = 1e-3
    seen = set()
    for i, kl in enumerate(_schedule_kls(desired)):
        kl_t.fill_(kl)
        hip_backend.adam_step(_adam_args(params, grads, m, v, state, ws, i & 1, kl=kl_t, desired=desired))
        lr = _rsl_rl_rule(lr, kl, desired)
        got = float(state.view(torch.float64)[2 * (1 - (i & 1))])
        assert got == lr, f"call {i} (kl {kl!r}): lr {got!r} vs rsl_rl {lr!r}"
        seen.add(lr)
    assert 1e-2 in seen and 1e-5 in seen


def _ppo_schedule(dev, kind, n, T, schedule, noise_gen=None):
    """PPO minibatch by minibatch: the lr after each equals rsl_rl's rule applied to the kernel's own kl_mean."""
    from genesis_forge_amd.learner import PPO

    env, st, policy, state = _setup(kind, n, T, dev)
    last = _collect(env, st, policy, state, noise_gen)
    ppo = PPO(policy, st, **dict(ALGO, schedule=schedule, learning_rate=0.003))
    ppo.compute_returns(last)
    lr, lrs = 0.003, []
    gen = torch.Generator(device=dev).manual_seed(1)
    for b in st.mini_batch_generator(ppo.num_mini_batches, ppo.num_learning_epochs, generator=gen):
        ppo._minibatch(b)
        kl = float(ppo._out[3])
        if schedule == "adaptive":
            lr = _rsl_rl_rule(lr, kl, 0.01)
        assert ppo.learning_rate == lr
        lrs.append(lr)
    return lrs


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", ["adaptive", "fixed"])
def test_ppo_lr_schedule_hip(hip_backend, schedule):
    lrs = _ppo_schedule("cuda", "go2", 256, 24, schedule)
    if schedule == "fixed":
        assert set(lrs) == {0.003}


@pytest.mark.parametrize("schedule", ["adaptive", "fixed"])
def test_ppo_lr_schedule_cpu(oracle_backend, schedule):
    lrs = _ppo_schedule("cpu", "go2", 70, 8, schedule, noise_gen=torch.Generator().manual_seed(2))
    if schedule == "fixed":
        assert set(lrs) == {0.003}


# ---- PPO.update end to end ------------------------------------------------------------------------------------------------------
def _end_to_end(dev, kind, n, T, iterations=2, noise_gen=None):
    """Collect with the fused policy, then update it with PPO and a copy of it with rsl_rl's loop, on the same rollout and the same
    minibatch stream; two iterations (the second rollout comes from the PPO-updated policy; both updates read it)."""
    import copy

    from genesis_forge_amd.learner import PPO

    env, st, policy, state = _setup(kind, n, T, dev)
    ref_policy = copy.deepcopy(policy)
    ppo, ref = PPO(policy, st, **ALGO), RslRlPPO(ref_policy, st, **ALGO)
    out = []
    for it in range(iterations):
        last = _collect(env, st, policy, state, noise_gen)
        ppo.compute_returns(last)
        want = ref.update(generator=torch.Generator(device=dev).manual_seed(10 + it))
        got = ppo.update(generator=torch.Generator(device=dev).manual_seed(10 + it))
        out.append((got, want, ppo.learning_rate, ref.learning_rate))
        for k in ("value_function", "surrogate", "entropy"):
            assert abs(got[k] - want[k]) <= 1e-4 * max(abs(want[k]), 1e-6), f"iteration {it}: {k} {got[k]} vs {want[k]}"
        assert ppo.learning_rate == ref.learning_rate, f"iteration {it}: lr {ppo.learning_rate} vs {ref.learning_rate}"
    # Parameters.  Adam's first steps move every weight by about lr·sign(g); where a gradient is near zero, the last-bit
    # difference of the two loss gradients can flip that sign, so single weights may differ by up to ~2·lr per step.  Bound: the
    # bulk (99.5 %) within 1e-4 + 1e-3·|p|, and no weight further than 2·3.2·Σ lr (3.2 ≈ the largest |m̂| / sqrt(v̂) of Adam's early
    # steps) — far below the ~0.05 spread of the weights themselves.
    a, b = _flat(policy), _flat(ref_policy)
    d = (a - b).abs()
    bulk = float((d <= 1e-4 + 1e-3 * b.abs()).float().mean())
    assert bulk >= 0.995, f"only {bulk:.4f} of the parameters agree to 1e-4 + 1e-3|p| (max diff {float(d.max())})"
    steps = iterations * ALGO["num_learning_epochs"] * ALGO["num_mini_batches"]
    assert float(d.max()) <= 2 * 3.2 * 1e-2 * steps
    return out, ppo


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["go2", "gait"])
def test_update_end_to_end_hip(hip_backend, kind):
    _end_to_end("cuda", kind, 384, 24)


def test_update_end_to_end_cpu(oracle_backend):
    _end_to_end("cpu", "go2", 70, 8, noise_gen=torch.Generator().manual_seed(4))


# ---- host reads -----------------------------------------------------------------------------------------------------------------
def _host_reads(dev, n, T, noise_gen=None):
    import copy

    from genesis_forge_amd.learner import PPO

    env, st, policy, state = _setup("go2", n, T, dev)
    last = _collect(env, st, policy, state, noise_gen)
    ref_policy = copy.deepcopy(policy)
    ppo, ref = PPO(policy, st, **ALGO), RslRlPPO(ref_policy, st, **ALGO)
    ppo.compute_returns(last)
    batches = ALGO["num_learning_epochs"] * ALGO["num_mini_batches"]
    with host_reads() as c:
        ref.update(generator=torch.Generator(device=dev).manual_seed(0))
    assert c[0] >= 4 * batches, f"the torch restatement read {c[0]} times"
    for _ in range(2):
        with host_reads() as c:
            ppo.update(generator=torch.Generator(device=dev).manual_seed(0))
        assert c[0] == 1, f"PPO.update read the device {c[0]} times"
    return ppo, st


@pytest.mark.gpu
def test_update_has_one_host_read_hip(hip_backend):
    ppo, st = _host_reads("cuda", 256, 24)
    # the sync debug mode, if this build honours it (positive control first): the minibatches never synchronise
    honoured = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(1, device="cuda").item()
    except RuntimeError:
        honoured = True
    finally:
        torch.cuda.set_sync_debug_mode(0)
    if honoured:
        batches = ppo.storage.mini_batch_generator(4, 5, generator=torch.Generator(device="cuda").manual_seed(0))
        torch.cuda.set_sync_debug_mode("error")
        try:
            for b in batches:
                ppo._minibatch(b)
        finally:
            torch.cuda.set_sync_debug_mode(0)


def test_update_has_one_host_read_cpu(oracle_backend):
    _host_reads("cpu", 70, 8, noise_gen=torch.Generator().manual_seed(4))


# ---- determinism, one-rank RCCL group --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_update_is_bitwise_deterministic(hip_backend):
    from genesis_forge_amd.learner import PPO

    env, st, policy, state = _setup("go2", 512, 24, "cuda", hidden=(256, 128))
    last = _collect(env, st, policy, state)
    ppo = PPO(policy, st, **ALGO)
    ppo.compute_returns(last)
    snap = [t.clone() for t in (ppo.params, ppo.exp_avg, ppo.exp_avg_sq, ppo._state)]
    runs = []
    for _ in range(2):
        for t, s in zip((ppo.params, ppo.exp_avg, ppo.exp_avg_sq, ppo._state), snap):
            t.copy_(s)
        ppo._calls = 0
        losses = ppo.update(generator=torch.Generator(device="cuda").manual_seed(3))
        runs.append((ppo.params.clone(), ppo.learning_rate, losses, ppo.grad_sync.bucket.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][3], runs[1][3])
    assert runs[0][1] == runs[1][1] and runs[0][2] == runs[1][2]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.gpu
def test_update_on_rccl_group_of_one(hip_backend):
    """A forced one-rank RCCL group runs the KL all-reduce and the bucket all-reduce of every minibatch: the sum over one rank is
    the identity, so the update equals the one without a group bit for bit."""
    import torch.distributed as dist
    from genesis_forge_amd.learner import PPO, GradientAllReduce

    env, st, policy, state = _setup("go2", 256, 24, "cuda")
    last = _collect(env, st, policy, state)
    init = [p.detach().clone() for p in policy.parameters()]

    def run(force):
        with torch.no_grad():
            for p, q in zip(policy.parameters(), init):
                p.data = q.clone()
        sync = GradientAllReduce(policy.parameters(), force=force)
        ppo = PPO(policy, st, grad_sync=sync, **ALGO)
        ppo.compute_returns(last)
        losses = ppo.update(generator=torch.Generator(device="cuda").manual_seed(2))
        return ppo.params.clone(), ppo.learning_rate, losses

    want = run(False)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        got = run(True)
    finally:
        dist.destroy_process_group()
    assert torch.equal(want[0], got[0]) and want[1] == got[1] and want[2] == got[2]


# ---- two gloo ranks (CPU) ---------------------------------------------------------------------------------------------------------
def _gloo_worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "genesis-forge_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from genesis_forge_amd import _native as nat
    from genesis_forge_amd import gs
    from genesis_forge_amd.learner import PPO, GradientAllReduce
    from oracle_backend import OracleBackend

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    gs.set_device("cpu")
    nat.set_backend(OracleBackend(os.path.join(ROOT, "oracle", "libgf_oracle.so")))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    env, st, policy, state = _setup("go2", 40 + 6 * rank, 8, "cpu")   # every rank its own shard of envs, the same initial policy
    last = _collect(env, st, policy, state, torch.Generator().manual_seed(20 + rank))
    ppo = PPO(policy, st, grad_sync=GradientAllReduce(policy.parameters()), **dict(ALGO, learning_rate=0.004))
    ppo.compute_returns(last)
    losses = ppo.update(generator=torch.Generator().manual_seed(rank))
    torch.save({"params": ppo.params.clone(), "lr": ppo.learning_rate, "losses": losses}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_update_two_gloo_ranks_stay_identical(oracle_lib_path):
    ctx = mp.get_context("spawn")
    with tempfile.TemporaryDirectory() as d:
        port = _free_port()
        procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, d)) for r in range(2)]
        for q in procs:
            q.start()
        for q in procs:
            q.join(240)
            assert q.exitcode == 0
        r0, r1 = (torch.load(os.path.join(d, f"rank{r}.pt")) for r in range(2))
    assert torch.equal(r0["params"], r1["params"]), "replicas diverged"
    assert r0["lr"] == r1["lr"]
    assert r0["losses"] != r1["losses"], "the ranks should have trained on different shards"


# ---- the algorithm dict, the ABI ----------------------------------------------------------------------------------------------------
def test_algorithm_dict_refusals(oracle_backend):
    from genesis_forge_amd.learner import PPO

    env, st, policy, _state = _setup("go2", 16, 4, "cpu")
    PPO(policy, st, **ALGO)   # the reference's dict as written
    for bad, word in ((dict(rnd_cfg={"weight": 1.0}), "rnd_cfg"), (dict(symmetry_cfg={"use_data_augmentation": True}), "symmetry_cfg"),
                      (dict(normalize_advantage_per_mini_batch=True), "normalize_advantage_per_mini_batch"), (dict(schedule="linear"), "schedule"),
                      (dict(learnig_rate=1e-3), "learnig_rate"), (dict(max_grad_norm=0.0), "max_grad_norm")):
        with pytest.raises(ValueError, match=word):
            PPO(policy, st, **dict(ALGO, **bad))
    PPO(policy, st, **dict(ALGO, normalize_advantage_per_mini_batch=False, rnd_cfg=None, symmetry_cfg=None))


def test_abi_sizes_and_refusals():
    """gf_sizeof 26 / 27 against the binding, and every refusal returns its code without launching (no device is touched: every
    call below returns before a launch, the non-NULL pointers are never dereferenced)."""
    from genesis_forge_amd import _native as nat

    lib = C.CDLL(nat.lib_path())
    lib.gf_sizeof.restype = C.c_int
    assert lib.gf_sizeof(nat.GF_SIZEOF_PPO_LOSS) == C.sizeof(nat.GfPpoLossArgs)
    assert lib.gf_sizeof(nat.GF_SIZEOF_ADAM) == C.sizeof(nat.GfAdamArgs)
    for f, st in ((lib.gf_ppo_loss, nat.GfPpoLossArgs), (lib.gf_adam_step, nat.GfAdamArgs)):
        f.restype, f.argtypes = C.c_int, [C.POINTER(st), C.c_void_p]
    E_NULL, E_RANGE = -1, -2
    FAKE = 1 << 20   # (16-byte aligned; never dereferenced)

    def loss_args(**kw):
        a = nat.GfPpoLossArgs()
        a.num_rows, a.num_actions, a.use_clipped_value_loss = 300, 12, 1
        for k in ("mu", "sigma", "value", "actions", "old_log_prob", "advantages", "target_values", "returns", "old_mu", "old_sigma",
                  "grad_mu", "grad_value", "grad_sigma", "out", "workspace"):
            setattr(a, k, FAKE)
        a.workspace_bytes = nat.ppo_loss_workspace_bytes(300, 12)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    call = lambda a: lib.gf_ppo_loss(C.byref(a), None)
    assert lib.gf_ppo_loss(None, None) == E_NULL
    for k in ("mu", "sigma", "value", "actions", "old_log_prob", "advantages", "target_values", "returns", "old_mu", "old_sigma", "out", "workspace"):
        assert call(loss_args(**{k: None})) == E_NULL, k
    assert call(loss_args(target_values=None, use_clipped_value_loss=0, num_rows=0)) == 0   # (the targets are read by the clipped loss only)
    for k in ("grad_mu", "grad_value", "grad_sigma"):
        assert call(loss_args(**{k: None})) == E_NULL, f"half a gradient set ({k} missing)"
    assert call(loss_args(num_rows=-1)) == E_RANGE
    assert call(loss_args(num_actions=0)) == E_RANGE
    assert call(loss_args(use_clipped_value_loss=2)) == E_RANGE
    assert call(loss_args(workspace_bytes=nat.ppo_loss_workspace_bytes(300, 12) - 8)) == E_RANGE
    assert call(loss_args(workspace=FAKE + 4)) == E_RANGE
    assert call(loss_args(num_rows=0, workspace_bytes=0)) == 0
    assert nat.ppo_loss_workspace_bytes(300, 12) == 2 * 15 * 8

    def adam_args(**kw):
        a = nat.GfAdamArgs()
        a.numel = 5000
        for k in ("params", "grads", "exp_avg", "exp_avg_sq", "state", "kl_mean", "workspace"):
            setattr(a, k, FAKE)
        a.workspace_bytes = nat.adam_workspace_bytes(5000)
        a.desired_kl, a.beta1, a.beta2, a.eps, a.max_grad_norm = 0.01, 0.9, 0.999, 1e-8, 1.0
        a.schedule, a.parity = nat.GF_ADAM_SCHEDULE_ADAPTIVE, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    acall = lambda a: lib.gf_adam_step(C.byref(a), None)
    assert lib.gf_adam_step(None, None) == E_NULL
    for k in ("params", "grads", "exp_avg", "exp_avg_sq", "state", "kl_mean", "workspace"):
        assert acall(adam_args(**{k: None})) == E_NULL, k
    assert acall(adam_args(schedule=nat.GF_ADAM_SCHEDULE_FIXED)) == E_NULL, "a KL given to the fixed schedule: half a set"
    assert acall(adam_args(numel=-1)) == E_RANGE
    assert acall(adam_args(schedule=2)) == E_RANGE
    assert acall(adam_args(parity=2)) == E_RANGE
    assert acall(adam_args(max_grad_norm=0.0)) == E_RANGE
    assert acall(adam_args(desired_kl=0.0)) == E_RANGE
    assert acall(adam_args(beta2=1.0)) == E_RANGE
    assert acall(adam_args(workspace_bytes=nat.adam_workspace_bytes(5000) - 8)) == E_RANGE
    assert acall(adam_args(workspace=FAKE + 4)) == E_RANGE
    assert acall(adam_args(numel=0, workspace_bytes=0)) == 0
    assert acall(adam_args(kl_mean=None, schedule=nat.GF_ADAM_SCHEDULE_FIXED, numel=0)) == 0
    assert nat.adam_workspace_bytes(5000) == 5 * 8 and nat.adam_workspace_bytes(10 ** 9) == 1024 * 8
