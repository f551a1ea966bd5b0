"""Teacher–student distillation: learner.StudentTeacherMLP / DistillForward / RolloutStorage.act_distill / Distillation, the
DistillationRunner, and the two entry points gf_mlp_distill_act and gf_bc_loss.

* StudentTeacherMLP's load rule, frozen teacher and eval mode;
* Distillation.update against tests/rsl_rl_distillation.py (gradient_length on both sides of T, both losses, clipping, the student's
  normaliser, a log-std policy), the dropped-tail rule, the refusals;
* DistillationRunner: a PPO teacher loaded from an OnPolicyRunner's checkpoint, an exact resume, the log record;
* the refusals of the two entry points without a device;
* on the GPU: gf_mlp_distill_act equals two gf_mlp_act launches bit for bit, gf_bc_loss equals gf_mirror_loss (mse) and float64
  within derived bounds, act_distill's rows, Distillation.update and the runner's two forwards.

Shapes: 70 envs (no multiple of the 32-row MLP tile or of a wave), 5 steps per env, hidden dims (32, 16), as tests/test_runner.py."""
import copy
import ctypes as C
import json
import os

import pytest
import torch

from rsl_rl_distillation import RslRlDistillation
from test_ppo_update import _env, host_reads

N, T, HIDDEN = 70, 5, (32, 16)
U = 2.0 ** -24
GROUPS = {"policy": ["policy"], "teacher": ["policy", "critic"]}       # the student reads the gait env's policy rows, the teacher its critic's too
TEACHER_GROUPS = {"policy": ["policy", "critic"], "critic": ["policy", "critic"]}   # the PPO run whose actor becomes the teacher


# ---- a distillation rollout ---------------------------------------------------------------------------------------------------------
def _setup(dev, n=N, steps=T, norm=False, std_type="scalar", seed=0):
    from genesis_forge_amd.learner import DistillForward, RolloutStorage, StudentTeacherMLP

    env = _env("gait", n)
    obs, extras = env.reset()
    st = RolloutStorage(env, steps, obs_groups=GROUPS).attach()
    st.begin(obs, extras)
    st.seed(5)
    A = env.action_space.shape[0]
    width = lambda g: sum(st._widths[m] for m in st.obs_groups[g])
    torch.manual_seed(seed)
    policy = StudentTeacherMLP(width("policy"), width("teacher"), A, HIDDEN, HIDDEN, init_noise_std=0.3, student_obs_normalization=norm,
                               noise_std_type=std_type).to(dev)
    return env, st, policy, DistillForward(policy), [obs, extras]


def _collect(env, st, policy, fwd, state, noise_gen=None):
    """One rollout: act_distill -> env.step -> update_normalization -> process_env_step(None, episodes)."""
    from genesis_forge_amd.learner import EpisodeStatistics

    obs, extras = state
    stats = EpisodeStatistics(env.num_envs)
    n, A = env.num_envs, env.action_space.shape[0]
    policy.train()
    for _ in range(st.num_steps):
        noise = None if noise_gen is None else torch.randn(n, A, generator=noise_gen).to(obs.device)
        actions = st.act_distill(fwd, obs, (obs, extras["observations"]["critic"]), noise=noise)
        obs, _r, _te, _tr, extras = env.step(actions)
        policy.update_normalization(obs)
        st.process_env_step(None, episodes=stats)
    state[0], state[1] = obs, extras
    return stats


def _flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()])


def _std(policy):
    return (policy.log_std if policy.noise_std_type == "log" else policy.std).detach()


def _update_vs_restatement(dev, gradient_length, loss_type, max_grad_norm, norm, std_type, noise_gen=None, epochs=2):
    """Distillation.update against the restatement on the same rollout.  The comparison of tests/test_ppo_update.py: the logged mean
    within 1e-4 relative, every student parameter within 1e-4 + 1e-3·|p|; the teacher and std keep their bits."""
    from genesis_forge_amd.learner import Distillation

    env, st, policy, fwd, state = _setup(dev, norm=norm, std_type=std_type)
    _collect(env, st, policy, fwd, state, noise_gen)
    if norm:
        assert int(policy.student_obs_normalizer.count) == N * T
    ref_policy = copy.deepcopy(policy)
    cfg = dict(num_learning_epochs=epochs, gradient_length=gradient_length, learning_rate=1e-3, max_grad_norm=max_grad_norm, loss_type=loss_type)
    alg, ref = Distillation(policy, st, class_name="Distillation", **cfg), RslRlDistillation(ref_policy, st, **cfg)
    teacher, std = _flat(policy.teacher).clone(), _std(policy).clone()
    before = _flat(policy.student).clone()
    for it in range(2):
        want = ref.update()
        got = alg.update()
        assert set(got) == {"behavior"}
        print(f"    update {it}: behavior {got['behavior']!r} vs {want['behavior']!r}")
        assert abs(got["behavior"] - want["behavior"]) <= 1e-4 * max(abs(want["behavior"]), 1e-6)
    steps = (epochs * T) // gradient_length
    assert alg._calls == ref.num_steps == 2 * steps
    a, b = _flat(policy.student), _flat(ref_policy.student)
    d = (a - b).abs()
    print(f"    student parameters: max |diff| {float(d.max()):.3e}, moved by up to {float((a - before).abs().max()):.3e}")
    assert bool((d <= 1e-4 + 1e-3 * b.abs()).all()), f"max diff {float(d.max())}"
    assert (steps == 0) == torch.equal(a, before)
    assert torch.equal(_flat(policy.teacher), teacher) and torch.equal(_std(policy), std), "the teacher and std are never stepped"
    std_param = policy.log_std if policy.noise_std_type == "log" else policy.std
    assert all(p.grad is None for p in policy.teacher.parameters()) and std_param.grad is None
    return alg


CASES = [(1, "mse", None, False, "scalar"), (3, "mse", None, False, "scalar"), (7, "mse", None, False, "scalar"),
         (3, "huber", None, False, "scalar"), (7, "huber", 0.5, False, "scalar"), (3, "mse", 0.5, False, "scalar"),
         (3, "mse", None, True, "scalar"), (7, "huber", 0.5, True, "scalar"), (3, "mse", None, False, "log")]
CASE_IDS = ["-".join(str(x) for x in c) for c in CASES]


# ---- 1. StudentTeacherMLP -----------------------------------------------------------------------------------------------------------------
def test_student_teacher_load_rule():
    from genesis_forge_amd.learner import ActorCriticMLP, StudentTeacherMLP

    torch.manual_seed(1)
    ppo_policy = ActorCriticMLP(20, 6, HIDDEN, HIDDEN, actor_obs_normalization=True)
    with torch.no_grad():
        ppo_policy.actor_obs_normalizer._mean.add_(0.5)
        ppo_policy.actor_obs_normalizer.count.add_(9)
    st = StudentTeacherMLP(11, 20, 6, (24,), HIDDEN, teacher_obs_normalization=True)
    assert st.loaded_teacher is False
    assert isinstance(st.student, torch.nn.Sequential) and isinstance(st.teacher, torch.nn.Sequential)
    assert [n for n, _ in st.named_parameters() if not n.startswith(("student.", "teacher."))] == ["std"]
    assert all(not p.requires_grad for p in st.teacher.parameters()) and all(p.requires_grad for p in st.student.parameters())
    student = {k: v.clone() for k, v in st.student.state_dict().items()}
    assert st.load_state_dict(ppo_policy.state_dict()) is False and st.loaded_teacher is True
    for k, v in ppo_policy.actor.state_dict().items():
        assert torch.equal(st.teacher.state_dict()[k], v), k
    for k, v in ppo_policy.actor_obs_normalizer.state_dict().items():
        assert torch.equal(st.teacher_obs_normalizer.state_dict()[k], v), k
    for k, v in st.student.state_dict().items():
        assert torch.equal(v, student[k]), "a PPO checkpoint leaves the student alone"
    # its own state dict round-trips into a policy built from other weights
    other = StudentTeacherMLP(11, 20, 6, (24,), HIDDEN, teacher_obs_normalization=True)
    assert other.load_state_dict(st.state_dict()) is True and other.loaded_teacher is True
    for k, v in st.state_dict().items():
        assert torch.equal(other.state_dict()[k], v), k
    with pytest.raises(ValueError, match="actor"):
        other.load_state_dict({"critic.0.weight": torch.zeros(1)})
    # the teacher stays in eval mode; act_mean / evaluate / action_std / the log-std variant
    st.train()
    assert st.training and st.student.training and not st.teacher.training and not st.teacher_obs_normalizer.training
    st.eval()
    st.train(True)
    assert not st.teacher.training
    x, tx = torch.randn(5, 11), torch.randn(5, 20)
    assert torch.equal(st.act_mean(x), st.student(x)) and not st.evaluate(tx).requires_grad
    assert torch.equal(st.evaluate(tx), st.teacher(st.teacher_obs_normalizer(tx)))
    log = StudentTeacherMLP(11, 20, 6, noise_std_type="log", init_noise_std=0.25)
    assert not hasattr(log, "std") and torch.allclose(log.action_std, torch.full((6,), 0.25))
    assert [m.out_features for m in log.student if isinstance(m, torch.nn.Linear)] == [256, 256, 256, 6]


def test_from_train_cfg_and_refusals():
    from genesis_forge_amd.learner import StudentTeacherMLP

    cfg = {"policy": {"class_name": "StudentTeacher", "activation": "elu", "student_hidden_dims": [24, 8], "teacher_hidden_dims": [32],
                      "init_noise_std": 0.2, "noise_std_type": "log", "student_obs_normalization": True}}
    p = StudentTeacherMLP.from_train_cfg(cfg, 11, 20, 6)
    assert [m.out_features for m in p.student if isinstance(m, torch.nn.Linear)] == [24, 8, 6] and p.teacher[0].in_features == 20
    assert hasattr(p, "log_std") and isinstance(p.teacher_obs_normalizer, torch.nn.Identity) and p.student_obs_normalizer.width == 11
    for bad, word in ((dict(actor_hidden_dims=[8]), "actor_hidden_dims"), (dict(activation="relu"), "activation"),
                      (dict(class_name="ActorCritic"), "class_name"), (dict(noise_std_type="gsde"), "noise_std_type")):
        with pytest.raises(ValueError, match=word):
            StudentTeacherMLP.from_train_cfg({"policy": dict(cfg["policy"], **bad)}, 11, 20, 6)


# ---- 2. Distillation.update ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gl,loss_type,clip,norm,std_type", CASES, ids=CASE_IDS)
def test_update_matches_the_restatement_cpu(oracle_backend, gl, loss_type, clip, norm, std_type):
    _update_vs_restatement("cpu", gl, loss_type, clip, norm, std_type, noise_gen=torch.Generator().manual_seed(4))


def test_the_pending_tail_is_dropped(oracle_backend):
    """T = 5, gradient_length = 3, one epoch: exactly one Adam step — after step 3; steps 4 and 5 leave the parameters where it put them,
    and their gradient does not reach the next update either."""
    from genesis_forge_amd.learner import Distillation

    env, st, policy, fwd, state = _setup("cpu")
    _collect(env, st, policy, fwd, state, torch.Generator().manual_seed(4))
    twin = copy.deepcopy(policy)
    alg = Distillation(policy, st, num_learning_epochs=1, gradient_length=3)
    alg.update()
    assert alg._calls == 1
    after = _flat(policy.student).clone()
    # the same single step from the first three time steps alone
    opt = torch.optim.Adam(twin.student.parameters(), lr=1e-3)
    loss = 0
    for t, (obs, target) in enumerate(st.step_batches()):
        if t < 3:
            loss = loss + torch.nn.functional.mse_loss(twin.act_mean(obs), target)
    loss.backward()
    opt.step()
    d = (after - _flat(twin.student)).abs()
    assert bool((d <= 1e-6 + 1e-5 * after.abs()).all()), float(d.max())
    assert not bool(alg.grad_sync.bucket.any()), "what was pending is gone"


def test_step_batches_of_a_frame_stored_group(oracle_backend):
    """A policy group of two managers, the first a history observation stored once per frame: a step's observation is the group's
    members side by side, the frame-stored one rebuilt by ``observation_rows(name, t)``."""
    from genesis_forge_amd.learner import DistillForward, RolloutStorage, StudentTeacherMLP

    env = _env("gait", 9)
    obs, extras = env.reset()
    st = RolloutStorage(env, 3, obs_groups={"policy": ["policy", "critic"], "teacher": ["critic"]}, history="frames").attach()
    assert "policy" in st.frames and st.observations is None, "the gait policy observation is a history: frame-stored"
    st.begin(obs, extras)
    with pytest.raises(RuntimeError, match="act_distill"):
        next(st.step_batches())
    A = env.action_space.shape[0]
    policy = StudentTeacherMLP(st._widths["policy"] + st._widths["critic"], st._widths["critic"], A, (8,), (8,))
    fwd, g, seen = DistillForward(policy), torch.Generator().manual_seed(0), []
    for _ in range(3):
        cobs = extras["observations"]["critic"]
        seen.append((torch.cat([obs, cobs], dim=-1).clone(), policy.evaluate(cobs).clone()))
        obs, _r, _te, _tr, extras = env.step(st.act_distill(fwd, (obs, cobs), cobs, noise=torch.randn(9, A, generator=g)))
        st.process_env_step(None)
    for (x, target), (want_x, want_t) in zip(st.step_batches(), seen):
        assert torch.equal(x, want_x) and torch.equal(target, want_t)


def test_distillation_refusals(oracle_backend, tmp_path):
    from genesis_forge_amd.learner import Distillation
    from genesis_forge_amd.runner import DistillationRunner

    env, st, policy, _fwd, _state = _setup("cpu")
    Distillation(policy, st, class_name="Distillation", num_learning_epochs=2, gradient_length=2, learning_rate=1e-4, max_grad_norm=1.0, loss_type="huber")
    for bad, word in ((dict(clip_param=0.2), "clip_param"), (dict(loss_type="l1"), "loss_type"), (dict(gradient_length=0), "gradient_length"),
                      (dict(num_learning_epochs=0), "num_learning_epochs"), (dict(max_grad_norm=0.0), "max_grad_norm"),
                      (dict(max_grad_norm=-1.0), "max_grad_norm")):
        with pytest.raises(ValueError, match=word):
            Distillation(policy, st, **bad)
    with pytest.raises(ValueError, match="grad_sync"):
        Distillation(policy, st, grad_sync=None)   # (single rank: there is no such argument)
    env2 = _built()
    with pytest.raises(ValueError, match="teacher"):
        DistillationRunner(env2, _cfg(obs_groups={"policy": ["policy"]}), None, device="cpu")
    runner = _runner(_built(), "cpu", noise_seed=1)
    with pytest.raises(ValueError, match="teacher"):
        runner.learn(1)


# ---- 3. DistillationRunner -------------------------------------------------------------------------------------------------------------------
def _cfg(**top):
    cfg = {"algorithm": {"class_name": "Distillation", "num_learning_epochs": 2, "gradient_length": 3, "learning_rate": 1e-3,
                         "max_grad_norm": 1.0, "loss_type": "mse"},
           "policy": {"class_name": "StudentTeacher", "activation": "elu", "student_hidden_dims": list(HIDDEN), "teacher_hidden_dims": list(HIDDEN),
                      "init_noise_std": 0.3, "student_obs_normalization": True, "teacher_obs_normalization": True},
           "obs_groups": {k: list(v) for k, v in GROUPS.items()}, "seed": 1, "num_steps_per_env": T, "save_interval": 2}
    cfg.update(top)
    return cfg


def _built():
    env = _env("gait", N)
    env.reset()
    return env


def _runner(env, dev, log_dir=None, forward="hip", noise_seed=None, cfg=None):
    from genesis_forge_amd.runner import DistillationRunner

    torch.manual_seed(0)
    noise = None if noise_seed is None else torch.Generator().manual_seed(noise_seed)
    return DistillationRunner(env, cfg or _cfg(), log_dir, device=dev, forward=forward, action_noise=noise)


def _teacher_checkpoint(dev, tmp_path, noise_seed=3):
    """A PPO teacher trained for two iterations on the privileged group; returns (checkpoint path, the PPO runner)."""
    from genesis_forge_amd.runner import OnPolicyRunner

    cfg = {"algorithm": dict(class_name="PPO", clip_param=0.2, desired_kl=0.01, entropy_coef=0.01, gamma=0.99, lam=0.95, learning_rate=0.001,
                             max_grad_norm=1.0, num_learning_epochs=2, num_mini_batches=4, schedule="adaptive", use_clipped_value_loss=True,
                             value_loss_coef=1.0),
           "policy": {"activation": "elu", "actor_hidden_dims": list(HIDDEN), "critic_hidden_dims": list(HIDDEN), "init_noise_std": 0.8,
                      "class_name": "ActorCritic"},
           "obs_groups": {k: list(v) for k, v in TEACHER_GROUPS.items()}, "seed": 1, "num_steps_per_env": T, "save_interval": 100,
           "empirical_normalization": True}
    torch.manual_seed(7)
    noise = None if noise_seed is None else torch.Generator().manual_seed(noise_seed)
    ppo = OnPolicyRunner(_built(), cfg, os.path.join(str(tmp_path), "teacher"), device=dev, action_noise=noise)
    ppo.learn(2)
    return os.path.join(str(tmp_path), "teacher", "model_1.pt"), ppo


def _runner_flow(dev, tmp_path, noise_seed):
    path, ppo = _teacher_checkpoint(dev, tmp_path, None if noise_seed is None else noise_seed + 1)
    log_dir = os.path.join(str(tmp_path), "student")

    def fresh(env, log=None, seed=noise_seed):
        r = _runner(env, dev, log, noise_seed=seed)
        student = _flat(r.alg.policy.student).clone()
        assert r.load(path) is None
        assert r.current_learning_iteration == 0 and r.alg._calls == 0, "a PPO checkpoint gives the teacher only"
        assert torch.equal(_flat(r.alg.policy.student), student)
        for k, v in ppo.alg.policy.actor.state_dict().items():
            assert torch.equal(r.alg.policy.teacher.state_dict()[k], v), k
        assert torch.equal(r.alg.policy.teacher_obs_normalizer._mean, ppo.alg.policy.actor_obs_normalizer._mean)
        return r

    a = fresh(_built(), log_dir)
    a.learn(2)
    ck = os.path.join(str(tmp_path), "a.pt")
    a.save(ck)
    a.learn(1)
    lines = [json.loads(l) for l in open(os.path.join(log_dir, "progress.jsonl"))]
    assert [l["iteration"] for l in lines] == [0, 1, 1] and all("behavior" in l and "surrogate" not in l for l in lines)
    assert set(lines[0]) == {"iteration", "behavior", "learning_rate", "mean_action_std", "mean_reward", "mean_episode_length",
                             "steps_per_second", "collection_time", "learn_time"}
    assert "model_0.pt" in os.listdir(log_dir)
    # an uninterrupted learn(3)
    whole = fresh(_built())
    whole.learn(3)
    # resumed in a fresh runner, on an env that is where run A's was at the save
    env = _built()
    fresh(env).learn(2)
    torch.manual_seed(1234)
    b = _runner(env, dev, noise_seed=None if noise_seed is None else noise_seed + 777, cfg=_cfg(seed=99))
    assert b.load(ck) is None and b.current_learning_iteration == 1 and b.alg.policy.loaded_teacher
    b.learn(1)
    for other, what in ((a, "continued"), (whole, "uninterrupted")):
        for x, y in zip((b.alg.params, b.alg.exp_avg, b.alg.exp_avg_sq), (other.alg.params, other.alg.exp_avg, other.alg.exp_avg_sq)):
            assert torch.equal(x, y), f"resumed vs {what} run"
        assert b.alg._calls == other.alg._calls == 3 * ((2 * T) // 3)
        for k, v in other.alg.policy.state_dict().items():
            assert torch.equal(b.alg.policy.state_dict()[k], v), k
    assert b.last_log["behavior"] == a.last_log["behavior"]
    # the inference policy is the student's mean
    act = b.get_inference_policy()
    obs = env.get_observations()
    with torch.no_grad():
        want = b.alg.policy.act_mean(obs)
    assert not b.alg.policy.training and act(obs).shape == want.shape
    return b, act(obs), want


def test_runner_teacher_resume_and_log_cpu(oracle_backend, tmp_path):
    import genesis_forge_amd
    from genesis_forge_amd.runner import DistillationRunner

    assert genesis_forge_amd.DistillationRunner is DistillationRunner
    _b, got, want = _runner_flow("cpu", tmp_path, noise_seed=21)
    assert torch.equal(got, want)


def test_runner_forwards_agree_bitwise_cpu(oracle_backend, tmp_path):
    """On the oracle backend both forwards are the same torch expressions."""
    path, _ppo = _teacher_checkpoint("cpu", tmp_path)
    out = []
    for forward in ("hip", "torch"):
        r = _runner(_built(), "cpu", forward=forward, noise_seed=11)
        r.load(path)
        r.learn(2)
        out.append((r.alg.params.clone(), r.last_log["behavior"]))
    assert torch.equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]


# ---- 4. the ABI, without a device ---------------------------------------------------------------------------------------------------------
def test_abi_sizes_and_refusals():
    """gf_sizeof 33 / 34 against the binding, and every refusal returns its code without launching (no device is touched: every call
    below returns before a launch, the non-NULL pointers are never dereferenced)."""
    from genesis_forge_amd import _native as nat

    lib = C.CDLL(nat.lib_path())
    lib.gf_sizeof.restype = C.c_int
    assert lib.gf_sizeof(nat.GF_SIZEOF_MLP_DISTILL) == C.sizeof(nat.GfMlpDistillArgs)
    assert lib.gf_sizeof(nat.GF_SIZEOF_BC_LOSS) == C.sizeof(nat.GfBcLossArgs)
    for f, st in ((lib.gf_mlp_distill_act, nat.GfMlpDistillArgs), (lib.gf_bc_loss, nat.GfBcLossArgs)):
        f.restype, f.argtypes = C.c_int, [C.POINTER(st), C.c_void_p]
    E_NULL, E_RANGE, E_UNSUPPORTED = -1, -2, -5
    FAKE = 1 << 20   # (16-byte aligned; never dereferenced)

    def net(n, widths, inputs=(48,)):
        n.num_layers, n.num_inputs = len(widths), len(inputs)
        for seg, w in zip(n.inputs, inputs):
            seg.rows, seg.width, seg.row_stride = FAKE, w, 0
        for lay, w in zip(n.layers, widths):
            lay.weight, lay.bias, lay.out_width = FAKE, FAKE, w

    def args(edit=None, **kw):
        a = nat.GfMlpDistillArgs()
        a.num_envs = 100
        net(a.student, (64, 32, 12))
        net(a.teacher, (96, 64, 32, 12), inputs=(48, 13))
        a.std = a.actions = a.teacher_actions = FAKE
        for k, v in kw.items():
            setattr(a, k, v)
        if edit is not None:
            edit(a)
        return a

    call = lambda a: lib.gf_mlp_distill_act(C.byref(a), None)
    assert lib.gf_mlp_distill_act(None, None) == E_NULL
    for k in ("std", "actions", "teacher_actions"):
        assert call(args(**{k: None})) == E_NULL, k
    assert call(args(num_envs=0, mean=FAKE, noise=FAKE, actions_out=FAKE, teacher_actions_out=FAKE, std_is_log=1)) == 0

    def edit(path, value):
        def f(a):
            obj, names = a, path.split(".")
            for nm in names[:-1]:
                obj = getattr(obj, nm[:-3])[int(nm[-2])] if nm.endswith("]") else getattr(obj, nm)
            setattr(obj, names[-1], value)
        return f

    for which in ("student", "teacher"):
        for path in ("layers[1].weight", "layers[0].bias", "inputs[0].rows"):
            assert call(args(edit(f"{which}.{path}", None))) == E_NULL, f"{which}.{path}"
        assert call(args(edit(f"{which}.in_mean", FAKE))) == E_NULL, "in_mean without in_std"
        for path, v in (("num_layers", 7), ("num_layers", -1), ("num_inputs", 0), ("num_inputs", 5), ("inputs[0].width", 0),
                        ("inputs[0].row_stride", 40), ("inputs[0].width", 1025), ("layers[0].out_width", 513), ("layers[0].out_width", 0)):
            assert call(args(edit(f"{which}.{path}", v))) == E_RANGE, f"{which}.{path} = {v}"
        assert call(args(edit(f"{which}.num_layers", 0))) == E_UNSUPPORTED, f"{which} absent"
    assert call(args(edit("student.layers[2].out_width", 65))) == E_RANGE
    assert call(args(edit("teacher.layers[3].out_width", 11))) == E_RANGE, "output widths differ"
    assert call(args(std_is_log=2)) == E_RANGE and call(args(std_is_log=-1)) == E_RANGE
    assert call(args(num_envs=-1)) == E_RANGE

    def bc(**kw):
        a = nat.GfBcLossArgs()
        a.num_rows, a.num_actions, a.loss_type = 300, 12, 1
        a.mu = a.target = a.grad = a.out = a.sums = a.workspace = FAKE
        a.workspace_bytes = nat.bc_loss_workspace_bytes(300)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    bcall = lambda a: lib.gf_bc_loss(C.byref(a), None)
    assert lib.gf_bc_loss(None, None) == E_NULL
    for k in ("mu", "target", "out", "workspace"):
        assert bcall(bc(**{k: None})) == E_NULL, k
    for kw in (dict(num_rows=-1), dict(num_actions=0), dict(loss_type=2), dict(loss_type=-1),
               dict(workspace_bytes=nat.bc_loss_workspace_bytes(300) - 8), dict(workspace=FAKE + 4)):
        assert bcall(bc(**kw)) == E_RANGE, kw
    assert bcall(bc(num_rows=0, workspace_bytes=0, grad=None, sums=None)) == 0
    assert nat.bc_loss_workspace_bytes(300) == 2 * 8 and nat.bc_loss_workspace_bytes(256) == 8 and nat.bc_loss_workspace_bytes(257) == 16


# ---- GPU: gf_mlp_distill_act == two gf_mlp_act launches -------------------------------------------------------------------------------------
def _mlp(sizes, g):
    """[(weight, bias)] on the GPU, torch.nn.Linear's layout."""
    return [((torch.randn(o, i, generator=g) / i ** 0.5).cuda(), (torch.randn(o, generator=g) * 0.1).cuda()) for i, o in zip(sizes[:-1], sizes[1:])]


def _fill(net, layers, parts, norm):
    """``parts``: [(tensor, width, row_stride)]; ``norm``: (mean, std, eps) or None."""
    net.num_layers, net.num_inputs = len(layers), len(parts)
    for seg, (x, w, stride) in zip(net.inputs, parts):
        seg.rows, seg.width, seg.row_stride = x.data_ptr(), w, stride
    for lay, (w, b) in zip(net.layers, layers):
        lay.weight, lay.bias, lay.out_width = w.data_ptr(), b.data_ptr(), w.shape[0]
    if norm is not None:
        net.in_mean, net.in_std, net.in_eps = norm[0].data_ptr(), norm[1].data_ptr(), norm[2]


def _inputs(n, width, split, stride, g):
    """The input of a net as segments: one tensor, two side by side (``split``), or a strided view of a wider tensor (``stride``)."""
    if stride:
        base = torch.randn(n, stride, generator=g).cuda()
        return [(base, width, stride)]
    if split:
        return [(torch.randn(n, split, generator=g).cuda(), split, 0), (torch.randn(n, width - split, generator=g).cuda(), width - split, 0)]
    return [(torch.randn(n, width, generator=g).cuda(), width, 0)]


def _norm(width, g):
    return (torch.randn(width, generator=g).cuda(), (torch.rand(width, generator=g) + 0.5).cuda(), 1e-2)


def _distill_case(backend, n, student, teacher, snorm=False, tnorm=False, is_log=0, philox=False, split=0, stride=0, seed=0):
    from genesis_forge_amd import _native as nat

    g = torch.Generator().manual_seed(1000 * seed + n)
    A = student[-1]
    sl, tl = _mlp(student, g), _mlp(teacher, g)
    sp, tp = _inputs(n, student[0], split, stride, g), _inputs(n, teacher[0], 0, 0, g)
    sn, tn = (_norm(student[0], g) if snorm else None), (_norm(teacher[0], g) if tnorm else None)
    std = (torch.rand(A, generator=g) * 0.5 + 0.1).cuda()
    if is_log:
        std = std.log()
    noise = None if philox else torch.randn(n, A, generator=g).cuda()
    new = lambda: torch.full((n, A), 7.0, device="cuda")
    key = dict(seed=0x1234ABCD5678, stream=3, env_offset=5)

    got = {k: new() for k in ("mean", "actions", "actions_out", "teacher_actions", "teacher_actions_out")}
    a = nat.GfMlpDistillArgs()
    a.num_envs = n
    _fill(a.student, sl, sp, sn)
    _fill(a.teacher, tl, tp, tn)
    a.std, a.std_is_log, a.noise = std.data_ptr(), is_log, None if noise is None else noise.data_ptr()
    a.seed, a.stream, a.env_offset = key["seed"], key["stream"], key["env_offset"]
    for k, v in got.items():
        setattr(a, k, v.data_ptr())
    backend.mlp_distill_act(a)

    want = {k: new() for k in ("mean", "actions", "actions_out", "teacher_actions")}
    b = nat.GfMlpActArgs()   # the student as gf_mlp_act's actor: sampled
    b.num_envs = n
    _fill(b.actor, sl, sp, sn)
    b.std, b.std_is_log, b.noise = std.data_ptr(), is_log, None if noise is None else noise.data_ptr()
    b.seed, b.stream, b.env_offset = key["seed"], key["stream"], key["env_offset"]
    b.mean, b.actions, b.actions_out = (want[k].data_ptr() for k in ("mean", "actions", "actions_out"))
    backend.mlp_act(b)
    c = nat.GfMlpActArgs()   # the teacher as gf_mlp_act's actor: mean only
    c.num_envs = n
    _fill(c.actor, tl, tp, tn)
    c.mean = want["teacher_actions"].data_ptr()
    backend.mlp_act(c)
    want["teacher_actions_out"] = want["teacher_actions"]
    for k in got:
        assert torch.isfinite(got[k]).all() and not bool((got[k] == 7.0).all()), k
        assert torch.equal(got[k], want[k]), f"{k}: max diff {float((got[k] - want[k]).abs().max())}"
    assert not torch.equal(got["actions"], got["mean"]), "the student is sampled"
    # loss of the optional destinations changes nothing else
    a.mean = a.actions_out = a.teacher_actions_out = None
    keep = {k: got[k].clone() for k in ("actions", "teacher_actions")}
    for k in keep:
        got[k].fill_(7.0)
    backend.mlp_distill_act(a)
    assert all(torch.equal(got[k], keep[k]) for k in keep)


STUDENT, TEACHER = (48, 64, 32, 12), (61, 96, 64, 32, 12)   # the teacher: another depth, and K % 4 != 0 — the element path


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 31, 32, 33, 70])
def test_distill_act_equals_two_mlp_act_launches(hip_backend, n):
    _distill_case(hip_backend, n, STUDENT, TEACHER)
    _distill_case(hip_backend, n, STUDENT, TEACHER, philox=True, is_log=1, seed=1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["A3", "A64", "student-normalised", "teacher-normalised", "log-std", "philox", "two-segments", "row-stride", "widest"])
def test_distill_act_paths(hip_backend, case):
    kw = dict(student=STUDENT, teacher=TEACHER)
    if case == "A3":
        kw.update(student=(48, 64, 32, 3), teacher=(61, 96, 64, 32, 3))
    elif case == "A64":
        kw.update(student=(48, 64, 32, 64), teacher=(61, 96, 64, 32, 64), philox=True)
    elif case == "student-normalised":
        kw.update(snorm=True)
    elif case == "teacher-normalised":
        kw.update(tnorm=True, philox=True)
    elif case == "log-std":
        kw.update(is_log=1)
    elif case == "philox":
        kw.update(philox=True)
    elif case == "two-segments":
        kw.update(split=20, snorm=True)
    elif case == "row-stride":
        kw.update(stride=240)
    else:   # a 600-wide first layer (two passes of the k loop) into hidden width 512 (four blocks per wave)
        kw.update(student=(600, 512, 12), teacher=(61, 96, 64, 32, 12), tnorm=True)
    _distill_case(hip_backend, 70, seed=2, **kw)


# ---- GPU: gf_bc_loss ---------------------------------------------------------------------------------------------------------------------------
def _bc_loss(backend, mu, target, loss_type, grad, sums=None):
    from genesis_forge_amd import _native as nat

    n, A = mu.shape
    out = torch.full((1,), 7.0, device="cuda")
    ws = torch.empty(max(1, nat.bc_loss_workspace_bytes(n) // 8), device="cuda", dtype=torch.float64)
    a = nat.GfBcLossArgs()
    a.num_rows, a.num_actions, a.loss_type = n, A, loss_type
    a.mu, a.target = mu.data_ptr(), target.data_ptr()
    a.grad = None if grad is None else grad.data_ptr()
    a.out, a.sums = out.data_ptr(), None if sums is None else sums.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 8
    backend.bc_loss(a)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("A", [3, 12, 64])
def test_bc_loss_and_gradient(hip_backend, A):
    """Rows around the workgroup (256) and two of them (513).

    mse equals gf_mirror_loss with identity tables, coeff 1 and a zeroed gradient, bit for bit (the same operation order).

    Bounds against float64 on the same float32 inputs, derived as tests/test_symmetry.py derives gf_mirror_loss's.  d is one float32
    rounding of the exact difference (relative 2^-24).
      mse    loss: d² carries 2·2^-24, the sum is double, the mean is rounded once: within 2^-22 relative.
             gradient: 1 / (N·A) and the product with 2·d are two more roundings: within 4·2^-24 relative.
      huber  loss: the quadratic branch as mse; the linear branch |d| - 0.5 with |d| >= 1 has absolute error 2^-24·|d| <= 2·2^-24 of
             its value; an element whose rounded d falls on the other side of 1 changes by 0.5·(|d| - 1)² <= 2^-49 (the branches
             meet with equal slope).  The sum is double, the mean is rounded once: within 2^-22 relative, as mse.
             gradient: inv · clamp(d, -1, 1) — inside, d's rounding, inv's and the product's: within 4·2^-24 relative; clamped, ±1 is
             exact: 2·2^-24; across the flip clamp moves by at most 2^-24 relative.  Within 4·2^-24 relative throughout."""
    from test_symmetry import _mirror_loss

    perm, sign = torch.arange(A, dtype=torch.int32, device="cuda"), torch.ones(A, device="cuda")
    for n in (1, 255, 256, 257, 513):
        g = torch.Generator().manual_seed(n + A)
        mu, target = torch.randn(n, A, generator=g), torch.randn(n, A, generator=g) * 1.5
        # |d| exactly 1, just inside and just outside, both signs (target 0: the differences below are exact in float32)
        one = torch.tensor(1.0)
        edge = [1.0, -1.0, float(torch.nextafter(one, one * 0)), -float(torch.nextafter(one, one * 0)), float(torch.nextafter(one, one * 2)),
                -float(torch.nextafter(one, one * 2))]
        k = min(len(edge), n * A)
        target.view(-1)[:k] = 0.0
        mu.view(-1)[:k] = torch.tensor(edge[:k])
        mu, target = mu.cuda(), target.cuda()
        if k == len(edge):
            assert (mu - target).view(-1)[:k].tolist() == edge
        d64 = mu.double() - target.double()
        for loss_type in (0, 1):
            if loss_type == 0:
                loss64, grad64 = float((d64 * d64).mean()), 2.0 * d64 / (n * A)
            else:
                e = torch.where(d64.abs() < 1, 0.5 * d64 * d64, d64.abs() - 0.5)
                loss64, grad64 = float(e.mean()), d64.clamp(-1, 1) / (n * A)
                ref = torch.nn.functional.huber_loss(mu.double(), target.double())
                assert abs(float(ref) - loss64) <= 1e-14 * loss64, "the float64 reference is torch's huber_loss"
            grad = torch.full((n, A), 7.0, device="cuda")
            sums = torch.tensor([1.5], dtype=torch.float64, device="cuda")
            out = _bc_loss(hip_backend, mu, target, loss_type, grad, sums)
            e_loss = abs(float(out[0]) - loss64) / loss64
            e_grad = float(((grad.double() - grad64).abs() / grad64.abs().clamp_min(1e-300)).max())
            print(f"    A={A} n={n} type={loss_type}: loss rel err {e_loss:.3e}, grad rel err {e_grad:.3e} (bounds {4 * U:.3e})")
            assert e_loss <= 4 * U, f"loss {float(out[0])} vs {loss64}"
            assert bool(((grad.double() - grad64).abs() <= 4 * U * grad64.abs()).all()), f"gradient: max rel err {e_grad}"
            assert float(sums[0]) == 1.5 + float(out[0]), "the running sum takes the float32 loss"
            if loss_type == 0:
                zero = torch.zeros(n, A, device="cuda")
                mir = _mirror_loss(hip_backend, mu, target, perm, sign, 1.0, zero)
                assert torch.equal(mir, out) and torch.equal(zero, grad), "mse is gf_mirror_loss's operation order"
            # written, not added; bitwise reproducible; loss only writes nothing but out / sums
            again = torch.full((n, A), -3.0, device="cuda")
            assert torch.equal(_bc_loss(hip_backend, mu, target, loss_type, again), out) and torch.equal(again, grad)
            assert torch.equal(_bc_loss(hip_backend, mu, target, loss_type, None, sums), out)
            assert float(sums[0]) == (1.5 + float(out[0])) + float(out[0])


# ---- GPU: act_distill's rows, the update, the runner ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_act_distill_writes_its_rows(hip_backend):
    env, st, policy, fwd, state = _setup("cuda", steps=3)
    obs, extras = state
    seen = []
    for i in range(5):   # rows 0, 1, 2 = T-1, then the wrap into the next rollout: 0, 1
        tobs = (obs, extras["observations"]["critic"])
        stream = st._act_stream
        actions = st.act_distill(fwd, obs, tobs)
        t = i % 3
        want_a, want_t = fwd.act(obs, tobs, seed=5, stream=stream, env_offset=0)
        assert torch.equal(actions, want_a), "the launch's own Philox draws: seed and stream as act_policy's"
        assert torch.equal(st.actions[t], actions) and torch.equal(st.privileged_actions[t], want_t), f"call {i}: row {t}"
        seen.append((t, actions.clone(), want_t.clone()))
        obs, _r, _te, _tr, extras = env.step(actions)
        st.process_env_step(None)
    assert st.values is None and st.mu is None and st.actions_log_prob is None, "no PPO rows"
    assert torch.equal(st.actions[2], seen[2][1]) and torch.equal(st.privileged_actions[2], seen[2][2]), "row T-1 of the first rollout stays"
    assert torch.equal(st.actions[0], seen[3][1]) and not torch.equal(seen[3][1], seen[0][1])
    batches = list(st.step_batches())
    assert len(batches) == 3 and all(b[1].data_ptr() == st.privileged_actions[t].data_ptr() for t, b in enumerate(batches)), "views, no gather"
    assert batches[1][0].data_ptr() == st.observations[1].data_ptr()
    # the teacher's stored actions are the teacher's output within float32 rounding of torch's forward
    with torch.no_grad():
        ref = copy.deepcopy(policy.teacher).double()(torch.cat(tobs, dim=-1).double())
    assert float((seen[4][2].double() - ref).abs().max()) <= 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("gl,loss_type,clip,norm,std_type", [(3, "mse", None, False, "scalar"), (7, "mse", 0.5, True, "scalar"),
                                                              (3, "huber", 0.5, True, "log"), (7, "huber", None, False, "scalar")])
def test_update_matches_the_restatement_hip(hip_backend, gl, loss_type, clip, norm, std_type):
    alg = _update_vs_restatement("cuda", gl, loss_type, clip, norm, std_type)
    with host_reads() as c:
        alg.update()
    assert c[0] == 1, f"Distillation.update read the device {c[0]} times"


@pytest.mark.gpu
def test_runner_hip_and_torch_forwards_agree(hip_backend, tmp_path):
    """learn(2) with forward="hip" and forward="torch" from the same seed and the same given noise: the two forwards differ by float32
    rounding only, the logged behaviour loss agrees within 1e-4 relative."""
    path, _ppo = _teacher_checkpoint("cuda", tmp_path, noise_seed=None)
    logs = []
    for forward in ("hip", "torch"):
        r = _runner(_built(), "cuda", forward=forward, noise_seed=11)
        r.load(path)
        r.learn(2)
        assert r.alg._calls == 2 * ((2 * T) // 3) and r.storage.privileged_actions is not None
        logs.append(r.last_log["behavior"])
    print(f"    behavior: hip {logs[0]!r}, torch {logs[1]!r}, relative difference {abs(logs[0] - logs[1]) / abs(logs[1]):.3e}")
    assert abs(logs[0] - logs[1]) <= 1e-4 * abs(logs[1])


@pytest.mark.gpu
def test_runner_resume_is_exact_hip(hip_backend, tmp_path):
    """The CPU flow with the kernels' own Philox draws: the PPO teacher, learn / save / resume, the inference policy (one launch)."""
    b, got, want = _runner_flow("cuda", tmp_path, noise_seed=None)
    assert float((got - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))
    assert torch.equal(got, b._fwd.mean(b.env.get_observations()))
