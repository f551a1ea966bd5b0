"""Random network distillation: ``gf_rnd_reward``, ``learner.RandomNetworkDistillation`` / ``EmpiricalDiscountedVariationNormalization`` /
``RndForward``, ``RolloutStorage.intrinsic_reward`` / ``group_rows_batch``, ``learner.PPO(rnd_cfg=...)`` and the runner's RND lines,
against rsl_rl's module and update restated in torch (tests/rsl_rl_rnd.py).

* CPU (oracle backend): the ``rnd_cfg`` refusals; the module against the restatement bit for bit (both normalisers, the three weight
  schedules at their boundary steps, the ``until`` freeze, eval mode); the exact-zero branch of the reward normaliser; ``PPO.update``
  with RND against the restated loop (once with symmetry augmentation); the runner's log keys, checkpoint keys and an exact resume;
  the entry point's refusals through the raw ABI; the self-check of the reward normaliser's float32 bound.
* GPU: the raw reward within 1 float32 ulp of ``(float)sqrt(Σ (double)(t−p)²)`` of two ``gf_mlp_act`` launches (and ``torch.equal``
  to an int64 reference on integer nets); the row add and the accumulators; the reward normaliser over five calls against a float64
  restatement within a derived bound, at 1, 2 and 257 tile records; the refusals with nothing written; a storage collection, one
  ``PPO.update`` and ``group_rows_batch`` end to end."""
import copy
import ctypes as C
import math
import os

import pytest
import torch

import test_ppo_update as tpu
from rsl_rl_rnd import RslRlDiscountedVariationNormalization, RslRlRND, RslRlRndPPO, rnd_state_rows
from test_log_std import _recorded_kl
from test_symmetry import _go2_symmetry

ALGO = tpu.ALGO
U = 2.0 ** -24   # unit roundoff of float32
E_NULL, E_RANGE, E_UNSUPPORTED = -1, -2, -5
FAKE = 1 << 20   # (16-byte aligned; never dereferenced)
RND_GROUPS = {"policy": ["policy"], "critic": ["policy"], "rnd_state": ["policy"]}
RND_CFG = dict(num_outputs=5, predictor_hidden_dims=[24, 16], target_hidden_dims=[20], weight=0.5, state_normalization=True,
               reward_normalization=True, learning_rate=2e-3)


# ---- CPU 1: the algorithm dict --------------------------------------------------------------------------------------------------------
def _storage(n=16, T=4, groups=RND_GROUPS, kind="go2", history="rows", env=None):
    from genesis_forge_amd.learner import RolloutStorage

    env = tpu._env(kind, n) if env is None else env
    obs, extras = env.reset()
    st = RolloutStorage(env, T, obs_groups=groups, history=history).attach()
    st.begin(obs, extras)
    st.seed(5)
    return env, st, [obs, extras]


def _policy(st, env, dev, hidden=(32, 16)):
    from genesis_forge_amd.learner import ActorCriticMLP

    torch.manual_seed(0)
    return ActorCriticMLP(st.obs_width, env.action_space.shape[0], hidden, hidden, init_noise_std=0.8).to(dev)


def test_rnd_cfg_is_accepted_and_its_refusals_name_it(oracle_backend):
    from genesis_forge_amd.learner import PPO, EmpiricalDiscountedVariationNormalization, EmpiricalNormalization, RandomNetworkDistillation

    env, st, _ = _storage()
    policy = _policy(st, env, "cpu")
    ppo = PPO(policy, st, **dict(ALGO, rnd_cfg=dict(RND_CFG, weight_schedule={"mode": "step", "final_step": 10, "final_value": 0.1})))
    rnd = ppo.rnd
    assert isinstance(rnd, RandomNetworkDistillation) and rnd.num_states == st.obs_width and rnd.num_outputs == 5
    assert isinstance(rnd.state_normalizer, EmpiricalNormalization) and rnd.state_normalizer.until == 10 ** 8
    assert isinstance(rnd.reward_normalizer, EmpiricalDiscountedVariationNormalization) and rnd.reward_normalizer.emp_norm.until == 10 ** 8
    assert (rnd.reward_normalizer.emp_norm.eps, rnd.reward_normalizer.gamma) == (1e-2, 0.99)
    assert not rnd.target.training and all(not p.requires_grad for p in rnd.target.parameters())
    assert all(p.requires_grad for p in rnd.predictor.parameters())
    assert [m.out_features for m in rnd.predictor if isinstance(m, torch.nn.Linear)] == [24, 16, 5]
    assert ppo._rnd_opt.learning_rate == 2e-3 and ppo.learning_rate == ALGO["learning_rate"]
    assert PPO(_policy(st, env, "cpu"), st, **dict(ALGO, rnd_cfg=None)).rnd is None
    minus = PPO(_policy(st, env, "cpu"), st, **dict(ALGO, rnd_cfg=dict(RND_CFG, predictor_hidden_dims=[-1, 8]))).rnd
    assert minus.predictor[0].out_features == st.obs_width, "a hidden width of -1 means num_states"
    lin = {"mode": "linear", "initial_step": 2, "final_step": 6, "final_value": 1.0}
    for bad, word in ((dict(weight=1.0), "num_outputs"), ({k: v for k, v in RND_CFG.items() if k != "predictor_hidden_dims"}, "predictor_hidden_dims"),
                      ({k: v for k, v in RND_CFG.items() if k != "target_hidden_dims"}, "target_hidden_dims"),
                      (dict(RND_CFG, num_state=3), "num_state"), (dict(RND_CFG, activation="relu"), "relu"),
                      (dict(RND_CFG, weight_schedule={"mode": "cosine"}), "weight_schedule"),
                      (dict(RND_CFG, weight_schedule={"mode": "step", "final_step": 3}), "final_value"),
                      (dict(RND_CFG, weight_schedule=dict(lin, final_step=2)), "final_step"),
                      (dict(RND_CFG, weight_schedule=dict(lin, power=2)), "power"), ("rnd", "dict")):
        with pytest.raises(ValueError, match="rnd_cfg") as e:
            PPO(_policy(st, env, "cpu"), st, **dict(ALGO, rnd_cfg=bad))
        assert word in str(e.value), f"{word!r} not in {e.value}"
    env2, plain, _ = _storage(groups=None)
    with pytest.raises(ValueError, match="rnd_cfg") as e:
        PPO(_policy(plain, env2, "cpu"), plain, **dict(ALGO, rnd_cfg=RND_CFG))
    assert "rnd_state" in str(e.value)

    class TwoRanks:   # what PPO reads of a multi-rank GradientAllReduce before it refuses
        world = 2
    with pytest.raises(ValueError, match="rnd_cfg") as e:
        PPO(_policy(st, env, "cpu"), st, grad_sync=TwoRanks(), **dict(ALGO, rnd_cfg=RND_CFG))
    assert "rank" in str(e.value)
    with pytest.raises(ValueError, match="normalize_advantage_per_mini_batch"):   # still out of scope
        PPO(_policy(st, env, "cpu"), st, **dict(ALGO, rnd_cfg=RND_CFG, normalize_advantage_per_mini_batch=True))


# ---- CPU 2: the module against the restatement ---------------------------------------------------------------------------------------------
def _pair(num_states=11, schedule=None, weight=0.5, state_norm=True, reward_norm=True, seed=3):
    from genesis_forge_amd.learner import RandomNetworkDistillation

    kw = dict(num_outputs=6, predictor_hidden_dims=[16, -1], target_hidden_dims=[12], weight=weight, state_normalization=state_norm,
              reward_normalization=reward_norm, weight_schedule=schedule)
    torch.manual_seed(seed)
    ours = RandomNetworkDistillation(num_states, **kw)
    ref = RslRlRND(num_states, **kw)
    ref.load_state_dict(ours.state_dict())   # (the same key names: rsl_rl's)
    return ours, ref


def _same_state(ours, ref, what):
    a, b = ours.state_dict(), ref.state_dict()
    assert list(a) == list(b), what
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k}"
    ra, rb = ours.reward_normalizer, ref.reward_normalizer
    if not isinstance(ra, torch.nn.Identity):
        assert (ra.avg is None) == (rb.avg is None), what
        assert ra.avg is None or torch.equal(ra.avg, rb.avg), f"{what}: avg"


def test_module_is_the_restatement_bit_for_bit():
    ours, ref = _pair()
    assert set(ours.state_dict()) >= {"predictor.0.weight", "target.0.bias", "state_normalizer._mean", "state_normalizer.count",
                                      "reward_normalizer.emp_norm._mean", "reward_normalizer.emp_norm._var", "reward_normalizer.emp_norm._std",
                                      "reward_normalizer.emp_norm.count"}
    g = torch.Generator().manual_seed(1)
    for step in range(7):
        x = torch.randn(40, 11, generator=g) * (1 + step) + step
        ours.update_normalization(x)
        ref.update_normalization(x)
        got, want = ours.get_intrinsic_reward(x), ref.get_intrinsic_reward(x)
        assert got.shape == (40,) and not got.requires_grad and torch.equal(got, want), f"step {step}"
        assert (ours.update_counter, ours.weight) == (ref.update_counter, ref.weight) == (step + 1, 0.5)
        _same_state(ours, ref, f"step {step}")
    assert int(ours.state_normalizer.count) == int(ours.reward_normalizer.emp_norm.count) == 7 * 40
    # eval mode: nothing is updated, the division by the running std stays
    ours.eval(), ref.eval()
    before = copy.deepcopy(ours.state_dict())
    avg = ours.reward_normalizer.avg.clone()
    x = torch.randn(40, 11, generator=g)
    ours.update_normalization(x), ref.update_normalization(x)
    assert torch.equal(ours.get_intrinsic_reward(x), ref.get_intrinsic_reward(x))
    for k, v in ours.state_dict().items():
        assert torch.equal(v, before[k]), f"eval mode changed {k}"
    assert torch.equal(ours.reward_normalizer.avg, avg)
    ours.train()
    assert not ours.target.training and ours.predictor.training, "the target stays in eval mode"


def test_until_freezes_both_normalisers():
    ours, ref = _pair()
    for m in (ours, ref):
        m.state_normalizer.until = 80
        m.reward_normalizer.emp_norm.until = 80
    g = torch.Generator().manual_seed(2)
    for step in range(5):
        x = torch.randn(40, 11, generator=g) + step
        ours.update_normalization(x), ref.update_normalization(x)
        assert torch.equal(ours.get_intrinsic_reward(x), ref.get_intrinsic_reward(x))
        _same_state(ours, ref, f"step {step}")
    assert int(ours.state_normalizer.count) == int(ours.reward_normalizer.emp_norm.count) == 80, "two batches, then frozen"


@pytest.mark.parametrize("schedule,expected", [
    (None, [0.5] * 8), ({"mode": "constant"}, [0.5] * 8),
    ({"mode": "step", "final_step": 4, "final_value": 2.0}, [0.5, 0.5, 0.5, 2.0, 2.0, 2.0, 2.0, 2.0]),      # counter 1 … 8: 0.5 while < 4
    ({"mode": "linear", "initial_step": 2, "final_step": 6, "final_value": 2.5}, [0.5, 0.5, 1.0, 1.5, 2.0, 2.5, 2.5, 2.5]),
], ids=["none", "constant", "step", "linear"])
def test_weight_schedules_at_their_boundary_steps(schedule, expected):
    ours, ref = _pair(schedule=schedule, state_norm=False, reward_norm=False)
    x = torch.randn(9, 11, generator=torch.Generator().manual_seed(0))
    raw = torch.linalg.norm(ref.target(x) - ref.predictor(x), dim=1).detach()
    for step, w in enumerate(expected):
        got, want = ours.get_intrinsic_reward(x), ref.get_intrinsic_reward(x)
        assert torch.equal(got, want) and torch.equal(got, raw * w), f"call {step + 1}"
        assert ours.weight == ref.weight == w, f"call {step + 1}: weight {ours.weight}"


# ---- CPU 3: the exact-zero branch ---------------------------------------------------------------------------------------------------------
def test_a_predictor_equal_to_the_target_gives_exact_zeros(oracle_backend):
    from genesis_forge_amd.learner import RandomNetworkDistillation, RndForward

    torch.manual_seed(0)
    rnd = RandomNetworkDistillation(9, 4, [8], [8], weight=2.0, reward_normalization=True)
    rnd.predictor.load_state_dict(rnd.target.state_dict())
    x = torch.randn(20, 9)
    rewards = torch.randn(20)
    before = rewards.clone()
    acc = torch.zeros(2, 20, dtype=torch.float64)
    for _ in range(2):
        out = RndForward(rnd).reward(x, rewards, acc[0], acc[1])
        assert torch.equal(out, torch.zeros(20)) and torch.equal(rewards, before), "r == 0, std == 0: the reward itself, no NaN"
    emp = rnd.reward_normalizer.emp_norm
    assert float(emp._std) == 0.0 and float(emp._var) == 0.0 and int(emp.count) == 40
    assert torch.equal(acc[1], torch.zeros(20, dtype=torch.float64)) and torch.equal(acc[0], 2 * before.double())


# ---- the reward normaliser in float64, with the bound of a float32 evaluation -----------------------------------------------------------------
def _normaliser_reference(rs, weight, gamma=0.99, until=None, dr=None):
    """rsl_rl's EmpiricalDiscountedVariationNormalization (training mode, fresh state) over the calls ``rs`` (float32 ``[N]`` each) in
    float64, the result scaled by ``weight`` — and first-order bounds of a float32 evaluation of the same lines, from float32's unit
    roundoff U and the roundings on the path.  ``gamma`` is the float32 the module multiplies with.  ``dr[k]``: a bound of the error
    the caller's ``rs[k]`` already carries (0: taken as exact).  Per call k:
      avg:   one multiply and one add                          dA_k = gamma dA_{k-1} + 2 U max|avg_k| + dr_k      (the first call copies)
      batch moments, the update lines, the count's division: torch's float32 lines take a pairwise sum over N (log2 N roundings) and
      about eight more operations each for the mean and the variance; the kernel takes them in float64 and rounds once — c = log2 N + 8
      covers both:
      mean:  a convex combination                              dM_k = (1-rate) dM_{k-1} + rate dA_k + c U (|mx| + |mean| + |mean'|)
      var' = (1-rate) var + rate vx + rate (1-rate) d²:        dV_k = (1-rate) dV_{k-1} + rate (2 sd_x dA_k + dA_k²)
                                                                      + rate (1-rate) 2 |d| (dA_k + dM_{k-1}) + c U (vx + var + d² + var')
      std = sqrt(var'), one rounding                           dS_k = dV_k / (2 std) + U std
      i = r / std · weight: the division, the product and the conversion of the weight round once each
                                                               dI_k = |i| (dS_k / std + 3 U) + |weight| dr_k / std
    Returns one dict per call: i, avg, mean, var, std, count and the bounds dI (per env), dA, dM, dV, dS."""
    g = float(torch.tensor(gamma, dtype=torch.float32))
    mean, var, std, count = 0.0, 1.0, 1.0, 0
    avg, dA, dM, dV, dS = None, 0.0, 0.0, 0.0, 0.0
    out = []
    for k, r in enumerate(rs):
        r64 = r.double()
        d_r = 0.0 if dr is None else float(dr[k])
        if avg is None:
            avg, dA = r64.clone(), d_r
        else:
            avg = avg * g + r64
            dA = g * dA + 2 * U * float(avg.abs().max()) + d_r
        n = r.numel()
        c = math.log2(n) + 8
        if until is None or count < until:
            mx, vx = float(avg.mean()), float(avg.var(unbiased=False))
            count += n
            rate = n / count
            d = mx - mean
            mean1 = mean + rate * d
            var1 = var + rate * (vx - var + d * (mx - mean1))
            dM1 = (1 - rate) * dM + rate * dA + c * U * (abs(mx) + abs(mean) + abs(mean1))
            dV = ((1 - rate) * dV + rate * (2 * math.sqrt(vx) * dA + dA * dA) + rate * (1 - rate) * 2 * abs(d) * (dA + dM)
                  + c * U * (vx + var + d * d + var1))
            dM, mean, var = dM1, mean1, var1
            std = math.sqrt(var)
            dS = dV / (2 * std) + U * std
        i = (r64 / std if std > 0 else r64) * weight
        dI = i.abs() * (dS / std + 3 * U) + abs(weight) * d_r / std
        out.append(dict(i=i, avg=avg.clone(), mean=mean, var=var, std=std, count=count, dI=dI, dA=dA, dM=dM, dV=dV, dS=dS))
    return out


def _distances(n, calls=5, seed=11, K=24, E=8, dev="cpu"):
    """Fixed random nets and ``calls`` different inputs whose distances spread over the envs (the running std stays far from 0):
    (target, predictor, [x_k])."""
    from genesis_forge_amd.learner import _mlp

    torch.manual_seed(seed)
    target, predictor = _mlp([K, 32, E]), _mlp([K, 24, E])
    g = torch.Generator().manual_seed(seed + 1)
    xs = [(torch.randn(n, K, generator=g) * (0.5 + 0.5 * k) * torch.linspace(0.2, 2.0, n).unsqueeze(1)).to(dev) for k in range(calls)]
    return target.to(dev), predictor.to(dev), xs


NORMALISER_SIZES = [32, 64, 8224]   # 1, 2 and 257 tile records: the scale launch's fold takes one record per lane, then a second round


@pytest.mark.parametrize("n", NORMALISER_SIZES)
def test_normaliser_bound_holds_torch_f32_cpu(n):
    """The self-check of the bound and the inputs (no kernel runs): rsl_rl's float32 lines stay within the bound of the float64 ones,
    and the running std stays well away from 0."""
    target, predictor, xs = _distances(n)
    with torch.no_grad():
        rs = [torch.linalg.norm(target(x) - predictor(x), dim=1) for x in xs]
    ref = _normaliser_reference(rs, 0.5)
    f32 = RslRlDiscountedVariationNormalization(until=10 ** 8)
    worst = 0.0
    for k, (r, want) in enumerate(zip(rs, ref)):
        got = f32(r) * 0.5
        q = float(((got.double() - want["i"]).abs() / want["dI"]).max())
        worst = max(worst, q)
        assert want["std"] > 0.05 * float(want["avg"].abs().mean()), f"call {k}: std {want['std']} too close to 0 for these inputs"
        assert abs(float(f32.emp_norm._std) - want["std"]) <= want["dS"], f"call {k}: std"
        assert abs(float(f32.emp_norm._mean) - want["mean"]) <= want["dM"], f"call {k}: mean"
        assert float((f32.avg.double() - want["avg"]).abs().max()) <= want["dA"] or k == 0, f"call {k}: avg"
        assert q <= 1.0, f"n={n} call {k}: torch f32 at {q:.3f} of the bound"
    print(f"    n={n}: torch f32 at most {worst:.3f} of the bound; relative bound {float((ref[-1]['dI'] / ref[-1]['i'].abs()).max()):.2e}")


# ---- CPU 4: PPO.update with RND against the restated loop -------------------------------------------------------------------------------------
def _collect_with_rnd(env, st, policy, rnd, state, dev, noise_gen, fwd=None):
    """One rollout with rsl_rl's RND lines: act -> env.step -> rnd.update_normalization -> intrinsic_reward -> process_env_step."""
    obs, extras = state
    n, A = env.num_envs, env.action_space.shape[0]
    rows = []
    for _ in range(st.num_steps):
        with torch.no_grad():
            mean, values = policy.act_mean(obs), policy.evaluate(obs)
        actions = st.act(mean, policy.std.detach(), values, noise=torch.randn(n, A, generator=noise_gen).to(dev))
        obs, _r, _te, tr, extras = env.step(actions)
        rnd.update_normalization(obs)
        rows.append(st.intrinsic_reward(rnd if fwd is None else fwd, obs))
        st.process_env_step(tr)
    state[0], state[1] = obs, extras
    return torch.stack(rows)


def _reference_rnd(ppo, st, cfg):
    kw = {k: v for k, v in cfg.items() if k != "learning_rate"}
    ref = RslRlRND(st.obs_width, **kw).to(ppo.params.device)
    ref.load_state_dict(ppo.rnd.state_dict())
    return ref


def _update_vs_restatement(dev, augment, seed, n=70, T=5):
    from genesis_forge_amd.learner import PPO

    env, st, state = _storage(n, T)
    policy = _policy(st, env, dev)
    ref_policy = copy.deepcopy(policy)
    sym = None
    if augment:
        sym = dict(use_data_augmentation=True, use_mirror_loss=True, mirror_loss_coeff=0.5, data_augmentation_func=_go2_symmetry(env))
    torch.manual_seed(8)
    ppo = PPO(policy, st, **dict(ALGO, rnd_cfg=RND_CFG, symmetry_cfg=sym))
    intrinsic = _collect_with_rnd(env, st, policy, ppo.rnd, state, dev, torch.Generator().manual_seed(4))
    assert float(intrinsic.abs().min()) > 0.0 and ppo.rnd.update_counter == T
    with torch.no_grad():
        st.compute_returns(policy.evaluate(state[0]), gamma=ALGO["gamma"], lam=ALGO["lam"])
    ref_rnd = _reference_rnd(ppo, st, RND_CFG)
    ref = RslRlRndPPO(ref_policy, st, ref_rnd, rnd_learning_rate=RND_CFG["learning_rate"], symmetry_cfg=sym, **ALGO)
    before, before_pred = tpu._flat(policy).clone(), tpu._flat(ppo.rnd.predictor).clone()
    target_before = tpu._flat(ppo.rnd.target).clone()
    kls = []
    with _recorded_kl(kls):
        want = ref.update(generator=torch.Generator(device=dev).manual_seed(seed))
    steps = ALGO["num_learning_epochs"] * ALGO["num_mini_batches"]
    assert len(kls) == steps
    for kl in kls:   # equal learning rates need every KL clear of the schedule's two thresholds
        for edge in (2.0 * ALGO["desired_kl"], ALGO["desired_kl"] / 2.0):
            assert abs(kl - edge) > 1e-3 * edge, f"a minibatch KL of the reference run ({kl}) within 1e-3 of {edge}: pick another seed"
    with tpu.host_reads() as c:
        got = ppo.update(generator=torch.Generator(device=dev).manual_seed(seed))
    assert c[0] == 1, f"PPO.update read the device {c[0]} times"
    print(f"    augment={augment}: got {got}\n    want {want}  lr {ppo.learning_rate} vs {ref.learning_rate}")
    keys = {"value_function", "surrogate", "entropy", "rnd"} | ({"symmetry"} if augment else set())
    assert set(got) == keys
    for k in sorted(keys):   # test_ppo_update._end_to_end's tolerances
        assert abs(got[k] - want[k]) <= 1e-4 * max(abs(want[k]), 1e-6), f"{k} {got[k]} vs {want[k]}"
    assert got["rnd"] > 1e-6
    assert ppo.learning_rate == ref.learning_rate, f"lr {ppo.learning_rate} vs {ref.learning_rate}"
    assert ppo._rnd_opt._calls == steps and ppo._rnd_opt.learning_rate == RND_CFG["learning_rate"], "the predictor's Adam: one step per minibatch, fixed lr"
    for name, a, b, a0 in (("policy", tpu._flat(policy), tpu._flat(ref_policy), before),
                           ("predictor", tpu._flat(ppo.rnd.predictor), tpu._flat(ref_rnd.predictor), before_pred)):
        d = (a - b).abs()
        bulk = float((d <= 1e-4 + 1e-3 * b.abs()).float().mean())
        print(f"    {name}: bulk {bulk:.4f}, max diff {float(d.max()):.3e}, moved {float((a - a0).abs().max()):.3e}")
        assert bulk >= 0.995, f"{name}: only {bulk:.4f} of the parameters agree to 1e-4 + 1e-3|p| (max diff {float(d.max())})"
        assert float(d.max()) <= 2 * 3.2 * 1e-2 * steps
        assert float((a - a0).abs().max()) > 1e-3, f"the update moved the {name}"
    assert torch.equal(tpu._flat(ppo.rnd.target), target_before), "the target is frozen"
    st.detach()
    return got


@pytest.mark.parametrize("augment", [False, True], ids=["plain", "augmented"])
def test_update_with_rnd_matches_the_restatement_cpu(oracle_backend, augment):
    _update_vs_restatement("cpu", augment, seed=12 if augment else 10)


def test_intrinsic_reward_belongs_between_the_step_and_process_env_step(oracle_backend):
    from genesis_forge_amd.learner import RandomNetworkDistillation

    env, st, (obs, _extras) = _storage(8, 3)
    policy = _policy(st, env, "cpu")
    torch.manual_seed(1)
    rnd = RandomNetworkDistillation(st.obs_width, 4, [8], [8], weight=1.0)
    with pytest.raises(RuntimeError, match="follows the env.step"):
        st.intrinsic_reward(rnd, obs)
    with torch.no_grad():
        actions = st.act(policy.act_mean(obs), policy.std.detach(), policy.evaluate(obs), noise=torch.zeros(8, env.action_space.shape[0]))
    obs, rew, _te, tr, _ex = env.step(actions)
    raw = st.rewards[0].clone()
    out = st.intrinsic_reward(rnd, obs)
    assert torch.equal(st.rewards[0], raw + out) and float(out.min()) > 0
    assert torch.equal(st.rnd_sums[0], raw.double()) and torch.equal(st.rnd_sums[1], out.double())
    with pytest.raises(RuntimeError, match="already hold"):
        st.intrinsic_reward(rnd, obs)
    st.process_env_step(tr)
    with pytest.raises(ValueError, match="RndForward or a RandomNetworkDistillation"):
        st.intrinsic_reward(policy, obs)
    actions = st.act(policy.act_mean(obs).detach(), policy.std.detach(), policy.evaluate(obs).detach(), noise=torch.zeros(8, env.action_space.shape[0]))
    obs, _rew, _te, tr, _ex = env.step(actions)
    st.process_env_step(tr)
    with pytest.raises(RuntimeError, match="before process_env_step"):
        st.intrinsic_reward(rnd, obs)


# ---- CPU 5: the runner ------------------------------------------------------------------------------------------------------------------------
def _runner_cfg(reward_normalization, **rnd):
    import test_runner as tr

    cfg = tr._cfg("go2")
    cfg["obs_groups"] = {k: list(v) for k, v in RND_GROUPS.items()}
    cfg["algorithm"]["rnd_cfg"] = dict(RND_CFG, reward_normalization=reward_normalization,
                                       weight_schedule={"mode": "linear", "initial_step": 2, "final_step": 40, "final_value": 0.05}, **rnd)
    return cfg


def _rnd_runner(cfg, dev, log_dir=None, forward="hip", noise_seed=2):
    import test_runner as tr

    return tr._runner(tr._built("go2"), copy.deepcopy(cfg), dev, log_dir=log_dir, forward=forward, noise_seed=noise_seed)


def _run_and_resume(dev, tmp_path, noise_seed=2):
    import test_runner as tr
    from genesis_forge_amd.runner import OnPolicyRunner

    cfg = _runner_cfg(False)
    path = os.path.join(str(tmp_path), "rnd.pt")
    a = _rnd_runner(cfg, dev, noise_seed=noise_seed)
    a.learn(2)
    log = a.last_log
    assert {"rnd", "mean_intrinsic_reward", "mean_extrinsic_reward", "rnd_weight"} <= set(log), sorted(log)
    steps = 2 * tr.T
    assert a.alg.rnd.update_counter == steps and log["rnd_weight"] == a.alg.rnd.weight == a.alg.rnd._scheduled_weight()
    assert log["rnd"] > 0 and log["mean_intrinsic_reward"] > 0 and math.isfinite(log["mean_extrinsic_reward"])
    a.save(path)
    saved = torch.load(path, weights_only=False)
    assert {"rnd_state_dict", "rnd_optimizer_state_dict"} <= set(saved) and saved["genesis_forge_amd"]["rnd_update_counter"] == steps
    assert saved["genesis_forge_amd"]["version"] == 1
    assert set(saved["rnd_optimizer_state_dict"]) == {"state", "param_groups"} and len(saved["rnd_optimizer_state_dict"]["state"]) == 6
    a.learn(1)
    env = tr._built("go2")
    tr._runner(env, copy.deepcopy(cfg), dev, noise_seed=noise_seed).learn(2)   # (the env is where run A's was at the save)
    torch.manual_seed(999)
    other = None if noise_seed is None else torch.Generator().manual_seed(noise_seed + 5)
    b = OnPolicyRunner(env, dict(copy.deepcopy(cfg), seed=77), None, device=dev, action_noise=other)
    assert not torch.equal(tpu._flat(b.alg.rnd.predictor), tpu._flat(a.alg.rnd.predictor))
    assert b.load(path) is None
    for k, v in saved["rnd_state_dict"].items():
        assert torch.equal(b.alg.rnd.state_dict()[k].cpu(), v.cpu()), k
    got, want = b.alg.rnd_optimizer_state_dict(), saved["rnd_optimizer_state_dict"]
    assert got["param_groups"] == want["param_groups"]
    for i, s in want["state"].items():
        for k, v in s.items():
            assert torch.equal(got["state"][i][k].cpu(), v.cpu()), (i, k)
    assert b.alg.rnd.update_counter == steps
    b.learn(1)
    for k in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(b.alg, k), getattr(a.alg, k)), f"policy {k}"
        assert torch.equal(getattr(b.alg._rnd_opt, k), getattr(a.alg._rnd_opt, k)), f"predictor {k}"
    for k, v in a.alg.rnd.state_dict().items():
        assert torch.equal(b.alg.rnd.state_dict()[k], v), k
    for k in ("iteration", "value_function", "surrogate", "entropy", "rnd", "mean_intrinsic_reward", "mean_extrinsic_reward", "rnd_weight",
              "learning_rate", "mean_reward"):
        assert b.last_log[k] == a.last_log[k], k
    return a


def test_runner_logs_saves_and_resumes_with_rnd_cpu(oracle_backend, tmp_path):
    _run_and_resume("cpu", tmp_path)


def test_runner_files_without_rnd_keep_their_keys(oracle_backend, tmp_path):
    import test_runner as tr

    plain = tr._runner(tr._built("go2"), tr._cfg("go2"), "cpu", noise_seed=2)
    plain.learn(1)
    assert not {"rnd", "mean_intrinsic_reward", "mean_extrinsic_reward", "rnd_weight"} & set(plain.last_log)
    path = os.path.join(str(tmp_path), "plain.pt")
    plain.save(path)
    saved = torch.load(path, weights_only=False)
    assert "rnd_state_dict" not in saved and "rnd_update_counter" not in saved["genesis_forge_amd"]
    again = tr._runner(tr._built("go2"), tr._cfg("go2"), "cpu", noise_seed=2)
    assert again.load(path) is None
    with_rnd = _rnd_runner(_runner_cfg(True), "cpu")
    with pytest.raises(ValueError, match="rnd_state_dict"):
        with_rnd.load(path)
    with_rnd.learn(1)   # (both normalisers on: the torch lines of the oracle backend)
    assert int(with_rnd.alg.rnd.reward_normalizer.emp_norm.count) == tr.T * tr.N
    with_rnd.save(path)
    assert again.load(path) is None, "a runner without RND reads a file with the RND keys"


# ---- the raw ABI ------------------------------------------------------------------------------------------------------------------------------
def _lib():
    from genesis_forge_amd import _native as nat

    lib = C.CDLL(nat.lib_path())
    lib.gf_sizeof.restype = C.c_int
    lib.gf_sizeof.argtypes = [C.c_int]
    lib.gf_rnd_reward.restype = C.c_int
    lib.gf_rnd_reward.argtypes = [C.c_void_p, C.c_void_p]
    return lib, nat


def _fake_args(nat, n=40, E=5, normalize=1, **over):
    a = nat.GfRndRewardArgs()
    a.num_envs = n
    for net, hidden in ((a.target, 16), (a.predictor, 24)):
        net.num_layers, net.num_inputs = 2, 1
        net.inputs[0].rows, net.inputs[0].width, net.inputs[0].row_stride = FAKE, 12, 0
        net.layers[0].weight, net.layers[0].bias, net.layers[0].out_width = FAKE, FAKE, hidden
        net.layers[1].weight, net.layers[1].bias, net.layers[1].out_width = FAKE, FAKE, E
    a.weight, a.gamma, a.normalize, a.update, a.first = 1.0, 0.99, normalize, normalize, 0
    a.avg = a.mean = a.var = a.std = a.count = FAKE if normalize else None
    a.until = -1
    a.rewards = a.intrinsic = a.acc_extrinsic = a.acc_intrinsic = a.workspace = FAKE
    a.workspace_bytes = nat.rnd_workspace_bytes(n)
    for k, v in over.items():
        obj, names = a, k.split("__")
        for name in names[:-1]:
            obj = getattr(obj, name) if not name.isdigit() else obj[int(name)]
        setattr(obj, names[-1], v)
    return a


REFUSALS = [
    (dict(intrinsic=None), E_NULL), (dict(workspace=None), E_NULL), (dict(avg=None), E_NULL), (dict(mean=None), E_NULL),
    (dict(var=None), E_NULL), (dict(std=None), E_NULL), (dict(count=None), E_NULL),
    (dict(target__layers__0__weight=None), E_NULL), (dict(predictor__layers__1__bias=None), E_NULL),
    (dict(target__inputs__0__rows=None), E_NULL), (dict(predictor__in_mean=FAKE), E_NULL),                    # in_mean without in_std
    (dict(num_envs=-1), E_RANGE), (dict(normalize=2), E_RANGE), (dict(update=-1), E_RANGE), (dict(first=2), E_RANGE),
    (dict(target__num_layers=7), E_RANGE), (dict(predictor__num_inputs=0), E_RANGE), (dict(target__layers__0__out_width=513), E_RANGE),
    (dict(predictor__layers__1__out_width=65, target__layers__1__out_width=65), E_RANGE), (dict(target__inputs__0__width=1025, predictor__inputs__0__width=1025), E_RANGE),
    (dict(target__inputs__0__row_stride=5, predictor__inputs__0__row_stride=5), E_RANGE),
    (dict(predictor__layers__1__out_width=6), E_RANGE),                                                           # output widths differ
    (dict(predictor__inputs__0__rows=FAKE + 16), E_RANGE), (dict(predictor__inputs__0__row_stride=16), E_RANGE),  # segment sets differ
    (dict(predictor__num_inputs=2, predictor__inputs__1__rows=FAKE, predictor__inputs__1__width=3), E_RANGE),
    (dict(workspace_bytes=8 * (4 + 3 * 2) - 1), E_RANGE), (dict(workspace=FAKE + 4), E_RANGE), (dict(count=FAKE + 4), E_RANGE),
    (dict(target__num_layers=0), E_UNSUPPORTED), (dict(predictor__num_layers=0), E_UNSUPPORTED),
]


def test_abi_size_and_refusals():
    """Every refusal through the raw descriptor, with pointers that are never dereferenced: nothing is launched."""
    lib, nat = _lib()
    assert lib.gf_sizeof(nat.GF_SIZEOF_RND_REWARD) == C.sizeof(nat.GfRndRewardArgs) and nat.GF_SIZEOF_RND_REWARD == 35
    assert nat.GF_ABI_VERSION == 11 and nat.GF_OBS_NORM_MAX_SETS == 2
    assert nat.rnd_workspace_bytes(40) == 8 * (4 + 3 * 2) and nat.rnd_workspace_bytes(0) == 32
    assert lib.gf_rnd_reward(None, None) == E_NULL
    for over, code in REFUSALS:
        assert lib.gf_rnd_reward(C.byref(_fake_args(nat, **over)), None) == code, over
    for over in (dict(avg=None, mean=None, var=None, std=None, count=None), dict(rewards=None, acc_extrinsic=None, acc_intrinsic=None)):
        assert lib.gf_rnd_reward(C.byref(_fake_args(nat, normalize=0, num_envs=0, **over)), None) == 0, "optional without the normaliser; no rows: a no-op"
    assert lib.gf_rnd_reward(C.byref(_fake_args(nat, num_envs=0)), None) == 0


# ---- GPU: the kernel through the raw descriptor ---------------------------------------------------------------------------------------------------
SENTINEL = 1234.5


def _views(x, how):
    """``x`` ``[n, K]`` as the segments the kernel reads: "one", "two" (the second on a base pointer 4 bytes off a 16-byte boundary),
    "strided" (two segments, the first a view of wider rows)."""
    n, K = x.shape
    if how == "one" or K < 2:
        return (x.contiguous(),)
    a = K // 3 or 1
    if how == "two":
        flat = torch.empty(n * (K - a) + 1, device=x.device)
        second = flat[1:].view(n, K - a)
        second.copy_(x[:, a:])
        assert second.data_ptr() % 16 == 4 and second.is_contiguous()
        return (x[:, :a].contiguous(), second)
    wide = torch.full((n, a + 7), SENTINEL, device=x.device)
    wide[:, 3:3 + a] = x[:, :a]
    return (wide[:, 3:3 + a], x[:, a:].contiguous())


def _fill(nat, a_net, net, segs, norm=None):
    from genesis_forge_amd.learner import _fill_net, _walk_mlp

    _fill_net(a_net, _walk_mlp(net, "net", nat.GF_MLP_MAX_ACTIONS, "test"), segs, norm)


def _embedding(backend, nat, net, segs, norm=None):
    """The ``mean`` of a gf_mlp_act launch with ``net`` as its actor."""
    n = segs[0].shape[0]
    out = torch.empty((n, net[-1].out_features), device="cuda")
    a = nat.GfMlpActArgs()
    a.num_envs = n
    _fill(nat, a.actor, net, segs, norm)
    a.critic.num_layers = 0
    a.mean = out.data_ptr()
    backend.mlp_act(a)
    return out


class _Call:
    """One gf_rnd_reward descriptor over device buffers with guard floats; ``run()`` launches and returns the intrinsic rewards."""

    def __init__(self, backend, nat, target, predictor, segs, norm=None, weight=1.0, rewards=None, normalizer=None, accumulate=False):
        n = segs[0].shape[0]
        self.backend, self.n = backend, n
        self.a = a = nat.GfRndRewardArgs()
        a.num_envs = n
        _fill(nat, a.target, target, segs, norm)
        _fill(nat, a.predictor, predictor, segs, norm)
        a.weight, a.gamma, a.until = weight, 0.99, -1
        self.buf = torch.full((n + 16,), SENTINEL, device="cuda")
        self.out = self.buf[8:8 + n]
        a.intrinsic = self.out.data_ptr()
        self.rewards = rewards
        a.rewards = None if rewards is None else rewards.data_ptr()
        self.acc = torch.zeros((2, n), device="cuda", dtype=torch.float64) if accumulate else None
        if accumulate:
            a.acc_extrinsic, a.acc_intrinsic = self.acc[0].data_ptr(), self.acc[1].data_ptr()
        self.ws = torch.zeros(nat.rnd_workspace_bytes(n) // 8, device="cuda", dtype=torch.float64)
        a.workspace, a.workspace_bytes = self.ws.data_ptr(), self.ws.numel() * 8
        if normalizer is not None:   # dict(avg, mean, var, std, count)
            a.normalize, a.update = 1, 1
            a.avg, a.mean, a.var, a.std, a.count = (normalizer[k].data_ptr() for k in ("avg", "mean", "var", "std", "count"))
        self.keep = (target, predictor, segs, norm, normalizer)

    def run(self, **fields):
        for k, v in fields.items():
            setattr(self.a, k, v)
        self.backend.rnd_reward(self.a)
        assert float(self.buf[:8].min()) == float(self.buf[-8:].max()) == SENTINEL, "a write outside intrinsic"
        return self.out.clone()


def _random_nets(K, hidden, E, seed):
    from genesis_forge_amd.learner import _mlp

    torch.manual_seed(seed)
    return _mlp([K, *hidden, E]).cuda(), _mlp([K, *[h + 8 for h in hidden], E]).cuda()


def _integer_nets(K, hidden, E, seed):
    """Nets and inputs of small integers with non-negative hidden pre-activations (ELU is the identity) and every partial sum below
    2^24: the float32 embeddings and their difference are exact in any order."""
    from genesis_forge_amd.learner import _mlp

    g = torch.Generator().manual_seed(seed)
    nets = []
    for extra in (0, 8):
        net = _mlp([K, *[h + extra for h in hidden], E])
        linears = [m for m in net if isinstance(m, torch.nn.Linear)]
        with torch.no_grad():
            for i, m in enumerate(linears):
                last = i == len(linears) - 1
                m.weight.copy_(torch.randint(-3 if last else 0, 4 if last else 2, m.weight.shape, generator=g).float())
                m.bias.copy_(torch.randint(-2 if last else 0, 3 if last else 2, m.bias.shape, generator=g).float())
        nets.append(net)
    return nets[0].cuda(), nets[1].cuda()


def _int64_forward(net, x):
    h = x.long()
    for m in net:
        if isinstance(m, torch.nn.Linear):
            h = h @ m.weight.long().T + m.bias.long()
            assert int(h.abs().max()) < 2 ** 24
    return h


def _ulps(a, b):
    """|a - b| in units of the last place of positive float32 values."""
    return (a.view(torch.int32).long() - b.view(torch.int32).long()).abs()


RAW_CASES = (
    [(n, 5, 48, (64,), "one", False) for n in (1, 31, 32, 33, 65)]
    + [(33, E, 7, (40, 24), "two", False) for E in (1, 5, 33, 64)]
    + [(65, 33, K, hidden, how, False) for K, how in ((7, "strided"), (48, "two"), (516, "strided")) for hidden in ((), (64,), (40, 24))]
    + [(33, 64, 516, (64,), "two", True), (65, 5, 48, (40, 24), "strided", True), (31, 1, 7, (), "one", True)]
)


@pytest.mark.gpu
@pytest.mark.parametrize("n,E,K,hidden,how,normed", RAW_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_raw_reward_is_the_distance_of_two_mlp_act_embeddings(hip_backend, n, E, K, hidden, how, normed):
    from genesis_forge_amd import _native as nat
    from genesis_forge_amd.learner import EmpiricalNormalization

    target, predictor = _random_nets(K, hidden, E, seed=K + E)
    x = torch.randn(n, K, generator=torch.Generator().manual_seed(n)).cuda() * 2 + 0.5
    segs = _views(x, how)
    norm = None
    if normed:
        norm = EmpiricalNormalization(K).cuda()
        norm.update(x), norm.update(x * 0.5 - 1)
    t, p = _embedding(hip_backend, nat, target, segs, norm), _embedding(hip_backend, nat, predictor, segs, norm)
    d = (t - p).double()
    s = torch.zeros(n, device="cuda", dtype=torch.float64)
    for j in range(E):   # j ascending
        s = s + d[:, j] * d[:, j]
    want = torch.sqrt(s).float()
    got = _Call(hip_backend, nat, target, predictor, segs, norm).run()
    worst = int(_ulps(got, want).max())
    print(f"    n={n} E={E} K={K} hidden={hidden} {how} normed={normed}: {worst} ulp (bit-equal: {torch.equal(got, want)})")
    assert worst <= 1, f"{worst} ulp from (float)sqrt(sum (double)(t-p)^2)"
    with torch.no_grad():   # and it is the module's quantity: within float32 rounding of torch's forward
        xn = x if norm is None else norm(x)
        ref = torch.linalg.norm(target.double()(xn.double()) - predictor.double()(xn.double()), dim=1)
    assert float((got.double() - ref).abs().max()) <= 1e-4 * float(ref.abs().max()) + 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("n,E,K,hidden,how", [(65, 33, 516, (40, 24), "strided"), (33, 64, 48, (64,), "two"), (32, 5, 7, (), "one"), (1, 1, 48, (64,), "one")],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_raw_reward_on_integer_nets_is_exact(hip_backend, n, E, K, hidden, how):
    from genesis_forge_amd import _native as nat

    target, predictor = _integer_nets(K, hidden, E, seed=K * 7 + E)
    x = torch.randint(0, 3, (n, K), generator=torch.Generator().manual_seed(n + 1)).float()
    d = _int64_forward(target.cpu(), x) - _int64_forward(predictor.cpu(), x)
    want = torch.sqrt((d * d).sum(1).double()).float()
    assert int((d * d).sum(1).max()) < 2 ** 53 and float(want.max()) > 0
    got = _Call(hip_backend, nat, target.cuda(), predictor.cuda(), _views(x.cuda(), how)).run()
    assert torch.equal(got.cpu(), want), f"max diff {float((got.cpu() - want).abs().max())}"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [33, 300])
def test_row_add_and_accumulators(hip_backend, n):
    from genesis_forge_amd import _native as nat

    target, predictor = _random_nets(24, (32,), 8, seed=5)
    x = torch.randn(n, 24, generator=torch.Generator().manual_seed(3)).cuda()
    rewards = torch.randn(n, generator=torch.Generator().manual_seed(4)).cuda()
    before = rewards.clone()
    call = _Call(hip_backend, nat, target, predictor, (x,), weight=0.75, rewards=rewards, accumulate=True)
    i1 = call.run()
    assert torch.equal(rewards, before + i1) and float(i1.min()) > 0
    raw = _Call(hip_backend, nat, target, predictor, (x,), weight=1.0).run()
    assert torch.equal(i1, raw * 0.75), "the weight is one float32 multiplication"
    i2 = call.run()
    assert torch.equal(i2, i1) and torch.equal(rewards, (before + i1) + i2)
    assert torch.equal(call.acc[0], before.double() + (before + i1).double()), "acc_extrinsic takes the row before the add"
    assert torch.equal(call.acc[1], i1.double() + i2.double())
    # rewards == NULL: only intrinsic (and its accumulator) is written
    alone = _Call(hip_backend, nat, target, predictor, (x,), weight=0.75, accumulate=True)
    assert torch.equal(alone.run(), i1)
    assert torch.equal(alone.acc[0], torch.zeros(n, device="cuda", dtype=torch.float64)) and torch.equal(alone.acc[1], i1.double())
    assert torch.equal(rewards, (before + i1) + i2)


def _normaliser_state(n):
    z = lambda v: torch.full((1, 1), v, device="cuda")
    return dict(avg=torch.full((n,), SENTINEL, device="cuda"), mean=z(0.0), var=z(1.0), std=z(1.0), count=torch.zeros((), device="cuda", dtype=torch.int64))


def _five_calls(backend, nat, n, until=-1):
    """Five consecutive normalised calls from a fresh state; returns (state, [intrinsic_k], [r_k]): r_k from launches without the
    normaliser — the same chains, the same bits."""
    target, predictor, xs = _distances(n, dev="cuda")
    state = _normaliser_state(n)
    outs, rs = [], []
    for k, x in enumerate(xs):
        rs.append(_Call(backend, nat, target, predictor, (x,)).run())
        outs.append(_Call(backend, nat, target, predictor, (x,), weight=0.5, normalizer=state).run(first=1 if k == 0 else 0, until=until))
    return state, outs, rs


@pytest.mark.gpu
@pytest.mark.parametrize("n", NORMALISER_SIZES)
def test_reward_normaliser_against_float64(hip_backend, n):
    from genesis_forge_amd import _native as nat

    state, outs, rs = _five_calls(hip_backend, nat, n)
    ref = _normaliser_reference([r.cpu() for r in rs], 0.5)
    worst = 0.0
    for k, (got, want) in enumerate(zip(outs, ref)):
        q = float(((got.cpu().double() - want["i"]).abs() / want["dI"]).max())
        worst = max(worst, q)
        assert q <= 1.0, f"n={n} call {k}: at {q:.3f} of the bound"
    last = ref[-1]
    print(f"    n={n}: at most {worst:.3f} of the bound; std {float(state['std']):.6f} vs {last['std']:.6f} (bound {last['dS']:.2e})")
    assert float((state["avg"].cpu().double() - last["avg"]).abs().max()) <= last["dA"]
    assert abs(float(state["mean"]) - last["mean"]) <= last["dM"] and abs(float(state["var"]) - last["var"]) <= last["dV"]
    assert abs(float(state["std"]) - last["std"]) <= last["dS"] and int(state["count"]) == 5 * n
    assert float(state["std"]) == math.sqrt(float(state["var"])) or float(state["std"]) == float(torch.sqrt(state["var"])), "std = sqrtf(var)"
    again, outs2, _ = _five_calls(hip_backend, nat, n)   # identical state, identical inputs: identical bits
    for a, b in zip(outs, outs2):
        assert torch.equal(a, b)
    for k in state:
        assert torch.equal(state[k], again[k]), k


@pytest.mark.gpu
def test_reward_normaliser_until_update_flag_and_exact_zero(hip_backend):
    from genesis_forge_amd import _native as nat

    n = 64
    state, outs, rs = _five_calls(hip_backend, nat, n, until=2 * n)   # two batches, then frozen: avg goes on, the statistics do not
    ref = _normaliser_reference([r.cpu() for r in rs], 0.5, until=2 * n)
    assert int(state["count"]) == 2 * n
    for k, (got, want) in enumerate(zip(outs, ref)):
        assert float(((got.cpu().double() - want["i"]).abs() / want["dI"]).max()) <= 1.0, f"call {k}"
    assert abs(float(state["std"]) - ref[1]["std"]) <= ref[1]["dS"] and float((state["avg"].cpu().double() - ref[-1]["avg"]).abs().max()) <= ref[-1]["dA"]
    # update = 0 (eval mode): r / std · weight from the statistics as they are; avg and the statistics untouched, one launch
    target, predictor, xs = _distances(n, dev="cuda")
    frozen = {k: v.clone() for k, v in state.items()}
    got = _Call(hip_backend, nat, target, predictor, (xs[0],), weight=0.5, normalizer=state).run(update=0)
    assert torch.equal(got, rs[0] / state["std"].reshape(()) * 0.5)
    for k in state:
        assert torch.equal(state[k], frozen[k]), k
    # the exact-zero case: predictor = target, r == 0, the first update leaves var = std = 0 and the reward is r itself
    zero = _normaliser_state(n)
    rewards = torch.randn(n, generator=torch.Generator().manual_seed(9)).cuda()
    before = rewards.clone()
    for first in (1, 0):
        out = _Call(hip_backend, nat, target, target, (xs[1],), weight=2.0, rewards=rewards, normalizer=zero).run(first=first)
        assert torch.equal(out, torch.zeros(n, device="cuda")) and torch.equal(rewards, before)
    assert float(zero["std"]) == 0.0 and float(zero["var"]) == 0.0 and int(zero["count"]) == 2 * n
    assert torch.equal(zero["avg"], torch.zeros(n, device="cuda"))


@pytest.mark.gpu
def test_refusals_write_nothing(hip_backend):
    from genesis_forge_amd import _native as nat

    lib = hip_backend.lib
    n = 40
    target, predictor = _random_nets(12, (16,), 5, seed=1)
    x = torch.randn(n, 12).cuda()
    state = _normaliser_state(n)
    rewards = torch.full((n,), SENTINEL, device="cuda")
    call = _Call(hip_backend, nat, target, predictor, (x,), rewards=rewards, normalizer=state, accumulate=True)
    saved = {f: getattr(call.a, f) for f, _ in call.a._fields_ if f not in ("target", "predictor")}

    def attempt(over):
        a = call.a
        undo = []
        for k, v in over.items():
            obj, names = a, k.split("__")
            for name in names[:-1]:
                obj = getattr(obj, name) if not name.isdigit() else obj[int(name)]
            undo.append((obj, names[-1], getattr(obj, names[-1])))
            setattr(obj, names[-1], v)
        rc = lib.gf_rnd_reward(C.byref(a), None)
        for obj, name, v in reversed(undo):
            setattr(obj, name, v)
        return rc

    real = [(o, c) for o, c in REFUSALS if all(v is None or v < FAKE for v in o.values())]   # (the rest are built on fake addresses)
    assert len(real) >= 22
    real += [(dict(predictor__in_mean=state["mean"].data_ptr()), E_NULL), (dict(workspace=call.ws.data_ptr() + 4), E_RANGE),
             (dict(count=state["count"].data_ptr() + 4), E_RANGE), (dict(predictor__inputs__0__rows=x.data_ptr() + 16), E_RANGE),
             (dict(predictor__num_inputs=2, predictor__inputs__1__rows=x.data_ptr(), predictor__inputs__1__width=3), E_RANGE)]
    for over, code in real:
        assert attempt(over) == code, over
    assert attempt(dict(num_envs=0)) == 0
    torch.cuda.synchronize()
    for f, v in saved.items():
        assert getattr(call.a, f) == v, f
    assert float(call.buf.min()) == float(call.buf.max()) == SENTINEL and float(rewards.min()) == float(rewards.max()) == SENTINEL
    assert float(state["avg"].min()) == SENTINEL and int(state["count"]) == 0 and float(call.acc.abs().max()) == 0.0


# ---- GPU: end to end ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_collection_with_rnd_forward_against_the_module(hip_backend):
    """T = 8 steps at N = 64: the storage's rewards and the intrinsic rows through RndForward against the module's torch lines on the
    GPU, within the normaliser's bound fed with the error the distances themselves may carry: 4 x torch's own float32 error against
    float64 + 1e-7 max|r| (test_mlp_act's bound of the forward)."""
    from genesis_forge_amd.learner import RandomNetworkDistillation, RndForward

    n, T = 64, 8
    runs = []
    for which in ("hip", "torch"):
        env, st, state = _storage(n, T)
        policy = _policy(st, env, "cuda")
        torch.manual_seed(6)
        rnd = RandomNetworkDistillation(st.obs_width, 8, [48, 24], [32], weight=0.5, state_normalization=True, reward_normalization=True).cuda()
        fwd = RndForward(rnd) if which == "hip" else None
        raw, states = [], []
        obs, extras = state
        g = torch.Generator().manual_seed(4)
        rows = []
        for _ in range(T):
            with torch.no_grad():
                mean, values = policy.act_mean(obs), policy.evaluate(obs)
            actions = st.act(mean, policy.std.detach(), values, noise=torch.randn(n, env.action_space.shape[0], generator=g).cuda())
            obs, _r, _te, tr, extras = env.step(actions)
            rnd.update_normalization(obs)
            raw.append(st.rewards[st.step - 1].clone())
            states.append((obs.clone(), copy.deepcopy(rnd.state_normalizer)))
            rows.append(st.intrinsic_reward(rnd if fwd is None else fwd, obs))
            st.process_env_step(None)
        runs.append(dict(rnd=rnd, st=st, raw=torch.stack(raw), rows=torch.stack(rows), states=states))
        st.detach()
    hip, ref = runs
    assert torch.equal(hip["raw"], ref["raw"]), "the two envs ran the same steps"
    rnd = ref["rnd"]
    t64, p64 = copy.deepcopy(rnd.target).double(), copy.deepcopy(rnd.predictor).double()
    rs, dr = [], []
    with torch.no_grad():
        for x, norm in ref["states"]:
            r32 = torch.linalg.norm(rnd.target(norm(x)) - rnd.predictor(norm(x)), dim=1)
            xn = (x.double() - norm._mean.double()) / (norm._std.double() + norm.eps)
            r64 = torch.linalg.norm(t64(xn) - p64(xn), dim=1)
            rs.append(r64.cpu())
            dr.append(4 * float((r32.double() - r64).abs().max()) + 1e-7 * float(r64.abs().max()))
    want = _normaliser_reference([r.float() for r in rs], 0.5, dr=[d + U * float(r.abs().max()) for d, r in zip(dr, rs)])
    worst = 0.0
    for k in range(T):
        for name, run in (("hip", hip), ("torch", ref)):
            q = float(((run["rows"][k].cpu().double() - want[k]["i"]).abs() / want[k]["dI"]).max())
            worst = max(worst, q) if name == "hip" else worst
            assert q <= 1.0, f"step {k}: the {name} intrinsic reward at {q:.3f} of the bound"
        assert torch.equal(hip["st"].rewards[k], hip["raw"][k] + hip["rows"][k]), f"step {k}: rewards = raw + intrinsic"
        assert float((hip["st"].rewards[k] - ref["st"].rewards[k]).abs().max()) <= 2 * float(want[k]["dI"].max()) + 2 * U * float(ref["st"].rewards[k].abs().max())
    print(f"    the HIP rows at most {worst:.3f} of the bound")
    assert hip["rnd"].update_counter == ref["rnd"].update_counter == T
    assert int(hip["rnd"].reward_normalizer.emp_norm.count) == T * n
    assert abs(float(hip["rnd"].reward_normalizer.emp_norm._std) - want[-1]["std"]) <= want[-1]["dS"]
    sums = hip["st"].rnd_sums
    assert torch.equal(sums[0], hip["raw"].double().sum(0)) and torch.equal(sums[1], hip["rows"].double().sum(0))


@pytest.mark.gpu
@pytest.mark.parametrize("augment", [False, True], ids=["plain", "augmented"])
def test_update_with_rnd_matches_the_restatement_hip(hip_backend, augment):
    _update_vs_restatement("cuda", augment, seed=12 if augment else 10, n=384, T=8)


@pytest.mark.gpu
@pytest.mark.parametrize("history", ["rows", "frames"])
def test_group_rows_batch_is_indexing(hip_backend, history):
    import test_frame_rollout as tfr
    from genesis_forge_amd.learner import EmpiricalNormalization, RolloutStorage

    n, T = 48, 6
    env = tfr._env("gait", n)
    groups = dict(tpu.GAIT_GROUPS, rnd_state=["critic", "policy"])
    obs, extras = env.reset()
    st = RolloutStorage(env, T, obs_groups=groups, history=history).attach()
    st.begin(obs, extras)
    assert (history == "frames") == bool(st.frames)
    A = env.action_space.shape[0]
    g = torch.Generator().manual_seed(0)
    for _ in range(T):
        env.step(torch.randn(n, A, generator=g).cuda() * 0.3)
    idx = torch.randperm(T * n, generator=g)[:101].cuda()
    rows = torch.cat([st.observation_rows(m)[:T].reshape(T * n, -1) for m in groups["rnd_state"]], dim=-1)
    got = st.group_rows_batch("rnd_state", idx)
    assert got.shape == (101, rows.shape[1]) and torch.equal(got, rows[idx])
    norm = EmpiricalNormalization(rows.shape[1]).cuda()
    norm.update(rows)
    assert torch.equal(st.group_rows_batch("rnd_state", idx, norm), norm(rows[idx])), "the gather's normalisation is forward() bit for bit"
    assert torch.equal(st.group_rows_batch("policy", idx), st.observation_rows("policy")[:T].reshape(T * n, -1)[idx])
    with pytest.raises(ValueError, match="no observation group"):
        st.group_rows_batch("teacher", idx)
    st.detach()


@pytest.mark.gpu
def test_runner_with_rnd_hip(hip_backend, tmp_path):
    """``learn`` with a complete rnd_cfg on the HIP forward: the log keys, the checkpoint and an exact resume — and no host read in a
    collection step (both normalisers on)."""
    a = _run_and_resume("cuda", tmp_path, noise_seed=None)
    assert a._rnd_fwd is not None
    runner = _rnd_runner(_runner_cfg(True), "cuda", noise_seed=None)
    runner.learn(1)   # (allocations and first-call paths)
    env, base, store = runner.env, runner.env.unwrapped, runner.storage
    from genesis_forge_amd.learner import EpisodeStatistics

    obs, extras = env.get_observations(), base.extras
    stats = EpisodeStatistics(base.num_envs)
    with tpu.host_reads() as c:
        runner._collect(obs, extras, stats)
    assert c[0] == 0, f"a collection with RND read the device {c[0]} times"
