"""Distillation with a recurrent student: ``learner.StudentTeacherRecurrent`` against rsl_rl's restated
(tests/rsl_rl_distillation_recurrent.py), the one-launch step ``gf_mlp_recurrent_distill_act`` against the separate launches it joins
(``gf_mlp_recurrent_act`` / ``gf_mlp_act``, bit for bit) and against float64, ``RecurrentDistillForward`` /
``RolloutStorage.act_distill_recurrent``, ``Distillation.update`` by truncated back-propagation through time against the restated
loop, and the ``DistillationRunner``.

Shapes: the update and the runner run 12 / 70 envs of the Go2 task with episodes of four steps, so that every rollout of six steps
has dones before its last step; the kernel cases are listed at ``CELL_CASES`` / ``SHAPE_CASES``."""
import copy
import ctypes as C
import os

import pytest
import torch

import rsl_rl_distillation_recurrent as RD
import test_recurrent as TR
from test_ppo_update import host_reads

FAKE = 0x10000
E_NULL, E_RANGE, E_UNSUPPORTED = -1, -2, -5
SENTINEL = TR.SENTINEL
KINDS = ("lstm", "gru")


def _states(s):
    return () if s is None else (tuple(s) if isinstance(s, tuple) else (s,))


# ---- CPU: the module ------------------------------------------------------------------------------------------------------------------
def _pair(kind, teacher_recurrent, S=11, P=14, A=3, H=16, hidden=(24, 12), seed=0, noise_std_type="scalar"):
    """``(ours, rsl_rl's)`` with the same weights."""
    from genesis_forge_amd.learner import StudentTeacherRecurrent

    torch.manual_seed(seed)
    ours = StudentTeacherRecurrent(S, P, A, hidden, hidden, 0.7, rnn_type=kind, rnn_hidden_dim=H, teacher_recurrent=teacher_recurrent,
                                   noise_std_type=noise_std_type)
    ref = RD.RslRlStudentTeacherRecurrent(S, P, A, hidden, hidden, 0.3, rnn_type=kind, rnn_hidden_dim=H, teacher_recurrent=teacher_recurrent,
                                          noise_std_type=noise_std_type)
    ref.load_state_dict(ours.state_dict())
    return ours, ref


@pytest.mark.parametrize("teacher_recurrent", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_module_is_the_restatement_in_step_mode(kind, teacher_recurrent):
    ours, ref = _pair(kind, teacher_recurrent)
    assert ours.is_recurrent is True and ours.teacher[0].in_features == (16 if teacher_recurrent else 14) and ours.student[0].in_features == 16
    g = torch.Generator().manual_seed(1)
    n = 5
    for t in range(6):
        obs, tobs = torch.randn(n, 11, generator=g), torch.randn(n, 14, generator=g)
        mu, mu_ref = ours.act_mean(obs), ref.act_mean(obs)
        assert mu.requires_grad and torch.equal(mu, mu_ref), t
        te = ours.evaluate(tobs)
        assert not te.requires_grad and torch.equal(te, ref.evaluate(tobs)), t
        for a, b in zip(ours.get_hidden_states(), ref.get_hidden_states()):
            assert TR._states_equal(a, b)
        assert (ours.get_hidden_states()[1] is None) == (not teacher_recurrent)
        assert all(x.requires_grad for x in _states(ours.get_hidden_states()[0])), "act_mean keeps a graph when grad is enabled"
        assert all(not x.requires_grad for x in _states(ours.get_hidden_states()[1])), "evaluate runs under no_grad"
        ours.detach_hidden_states()
        ref.detach_hidden_states()
        assert all(not x.requires_grad for x in _states(ours.get_hidden_states()[0]))
        if t in (1, 2, 4):
            dones = None if t == 4 else torch.rand(n, generator=g) < 0.5
            ours.reset(dones)
            ref.reset(dones)
            if dones is None:
                assert ours.get_hidden_states() == (None, None)
            else:
                for s in ours.get_hidden_states():
                    for x in _states(s):
                        assert float(x[0, dones].abs().sum()) == 0.0
    given = copy.deepcopy(ours.get_hidden_states())
    ours.reset()
    ours.reset(hidden_states=given)
    for a, b in zip(ours.get_hidden_states(), given):
        assert TR._states_equal(a, b)
    with torch.no_grad():   # no graph under no_grad
        ours.act_mean(torch.randn(n, 11, generator=g))
    assert all(not x.requires_grad for x in _states(ours.get_hidden_states()[0]))


@pytest.mark.parametrize("teacher_recurrent", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_keys_and_frozen_teacher(kind, teacher_recurrent):
    ours, ref = _pair(kind, teacher_recurrent, noise_std_type="log")
    rnn = lambda m: [f"memory_{m}.rnn.{p}_l0" for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    want = rnn("s") + (rnn("t") if teacher_recurrent else [])
    want += [f"{net}.{i}.{p}" for net in ("student", "teacher") for i in (0, 2, 4) for p in ("weight", "bias")] + ["log_std"]
    ours.act_mean(torch.zeros(2, 11))   # (a hidden state exists: it must not show up)
    assert sorted(ours.state_dict().keys()) == sorted(want) == sorted(ref.state_dict().keys())
    assert hasattr(ours, "memory_t") == teacher_recurrent
    frozen = [n for n, p in ours.named_parameters() if not p.requires_grad]
    assert sorted(frozen) == sorted(k for k in want if k.startswith(("teacher.", "memory_t.")))
    ours.train()
    assert ours.training and ours.student.training and ours.memory_s.training and not ours.teacher.training
    assert not teacher_recurrent or not ours.memory_t.training
    from genesis_forge_amd.learner import StudentTeacherRecurrent

    normed = StudentTeacherRecurrent(11, 14, 3, (8,), (8,), rnn_type=kind, rnn_hidden_dim=8, student_obs_normalization=True,
                                     teacher_obs_normalization=True, teacher_recurrent=teacher_recurrent)
    normed.train()
    assert normed.student_obs_normalizer.training and not normed.teacher_obs_normalizer.training
    assert {k.split(".")[0] for k in normed.state_dict()} >= {"student_obs_normalizer", "teacher_obs_normalizer"}
    normed.update_normalization(torch.randn(6, 11))
    assert int(normed.student_obs_normalizer.count) == 6 and int(normed.teacher_obs_normalizer.count) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_the_four_load_cases(kind):
    from genesis_forge_amd.learner import ActorCriticMLP, ActorCriticRecurrent, StudentTeacherRecurrent

    torch.manual_seed(3)
    H, hid = 16, (24, 12)
    rec = ActorCriticRecurrent(14, 3, hid, hid, rnn_type=kind, rnn_hidden_dim=H, actor_obs_normalization=True)
    mlp = ActorCriticMLP(14, 3, hid, hid, actor_obs_normalization=True)
    with torch.no_grad():
        for p in (rec, mlp):
            p.actor_obs_normalizer._mean.add_(0.5)
    make = lambda tr: StudentTeacherRecurrent(11, 14, 3, hid, hid, rnn_type=kind, rnn_hidden_dim=H, teacher_recurrent=tr, teacher_obs_normalization=True)
    # 1. a recurrent PPO checkpoint into teacher_recurrent=True: the teacher, its normaliser and memory_t
    st = make(True)
    student = {k: v.clone() for k, v in st.state_dict().items() if k.startswith(("student.", "memory_s."))}
    assert st.loaded_teacher is False and st.load_state_dict(rec.state_dict()) is False and st.loaded_teacher is True
    for k, v in rec.actor.state_dict().items():
        assert torch.equal(st.teacher.state_dict()[k], v), k
    for k, v in rec.memory_a.state_dict().items():
        assert torch.equal(st.memory_t.state_dict()[k], v), k
    assert torch.equal(st.teacher_obs_normalizer._mean, rec.actor_obs_normalizer._mean)
    for k, v in student.items():
        assert torch.equal(st.state_dict()[k], v), "a PPO checkpoint leaves the student and its memory alone"
    assert not st.teacher.training and not st.memory_t.training
    x = torch.randn(4, 14)
    with torch.no_grad():
        rec.eval()
        assert torch.equal(st.evaluate(x), rec.act_mean(x)), "the recurrent teacher is the PPO actor behind its memory"
    # 2. a feed-forward PPO checkpoint into teacher_recurrent=False
    sf = make(False)
    assert sf.load_state_dict(mlp.state_dict()) is False and sf.loaded_teacher
    for k, v in mlp.actor.state_dict().items():
        assert torch.equal(sf.teacher.state_dict()[k], v), k
    # 3. a distillation checkpoint loads whole
    other = make(True)
    assert other.load_state_dict(st.state_dict()) is True and other.loaded_teacher
    for k, v in st.state_dict().items():
        assert torch.equal(other.state_dict()[k], v), k
    # 4. the mismatches name teacher_recurrent
    with pytest.raises(ValueError, match="teacher_recurrent"):
        make(False).load_state_dict(rec.state_dict())
    with pytest.raises(ValueError, match="teacher_recurrent"):
        make(True).load_state_dict(mlp.state_dict())
    with pytest.raises(ValueError, match="actor"):
        make(True).load_state_dict({"critic.0.weight": torch.zeros(1)})


def test_from_train_cfg_and_refusals_name_their_key():
    from genesis_forge_amd.learner import StudentTeacherMLP, StudentTeacherRecurrent

    cfg = {"policy": {"class_name": "StudentTeacherRecurrent", "rnn_type": "gru", "rnn_hidden_dim": 32, "rnn_num_layers": 1, "teacher_recurrent": True,
                      "student_hidden_dims": [16], "teacher_hidden_dims": [8], "activation": "elu", "init_noise_std": 0.5,
                      "student_obs_normalization": True}}
    p = StudentTeacherRecurrent.from_train_cfg(cfg, 10, 12, 4)
    assert isinstance(p.memory_s.rnn, torch.nn.GRU) and p.memory_s.rnn.input_size == 10 and p.memory_t.rnn.input_size == 12
    assert p.memory_s.rnn.hidden_size == 32 and p.student[0].in_features == 32 and p.teacher[0].in_features == 32 and float(p.std.detach()[0]) == 0.5
    assert p.student_obs_normalizer.width == 10 and isinstance(p.teacher_obs_normalizer, torch.nn.Identity)
    d = StudentTeacherRecurrent.from_train_cfg({"policy": {"class_name": "StudentTeacherRecurrent"}}, 10, 12, 4)
    assert isinstance(d.memory_s.rnn, torch.nn.LSTM) and d.memory_s.rnn.hidden_size == 256 and not d.teacher_recurrent and d.teacher[0].in_features == 12
    for over, key in ((dict(rnn_num_layers=2), "rnn_num_layers"), (dict(rnn_type="rnn"), "rnn_type"), (dict(rnn_hidden_dim=513), "rnn_hidden_dim"),
                      (dict(rnn_hidden_dim=0), "rnn_hidden_dim"), (dict(activation="relu"), "activation"), (dict(class_name="StudentTeacher"), "class_name"),
                      (dict(actor_hidden_dims=[8]), "actor_hidden_dims"), (dict(noise_std_type="gsde"), "noise_std_type")):
        with pytest.raises(ValueError, match=key):
            StudentTeacherRecurrent.from_train_cfg({"policy": dict(cfg["policy"], **over)}, 10, 12, 4)
    with pytest.raises(ValueError, match="class_name"):   # the MLP policy still takes "StudentTeacher" only
        StudentTeacherMLP.from_train_cfg({"policy": {"class_name": "StudentTeacherRecurrent"}}, 10, 12, 4)
    with pytest.raises(ValueError, match="rnn_type"):     # … and knows nothing of the rnn keys
        StudentTeacherMLP.from_train_cfg({"policy": {"rnn_type": "lstm"}}, 10, 12, 4)
    for kw, key in ((dict(rnn_num_layers=2), "rnn_num_layers"), (dict(rnn_type="rnn"), "rnn_type"), (dict(rnn_hidden_dim=513), "rnn_hidden_dim")):
        with pytest.raises(ValueError, match=key):
            StudentTeacherRecurrent(10, 12, 4, **kw)


# ---- the raw ABI, without a device --------------------------------------------------------------------------------------------------
def _lib():
    from genesis_forge_amd import _native as nat

    lib = C.CDLL(nat.lib_path())
    lib.gf_sizeof.restype = C.c_int
    lib.gf_sizeof.argtypes = [C.c_int]
    lib.gf_mlp_recurrent_distill_act.restype = C.c_int
    lib.gf_mlp_recurrent_distill_act.argtypes = [C.c_void_p, C.c_void_p]
    return lib, nat


def _fake_args(nat, n=40, **over):
    """An LSTM student and a GRU teacher on fake addresses."""
    ra = nat.GfMlpRecurrentDistillArgs()
    a = ra.act
    a.num_envs = n
    for net in (a.student, a.teacher):
        net.num_layers, net.num_inputs = 2, 1
        net.inputs[0].rows, net.inputs[0].width, net.inputs[0].row_stride = FAKE, 12, 0
        net.layers[0].weight, net.layers[0].bias, net.layers[0].out_width = FAKE, FAKE, 16
        net.layers[1].weight, net.layers[1].bias, net.layers[1].out_width = FAKE, FAKE, 5
    a.std = a.actions = a.teacher_actions = FAKE
    for cell, kind in ((ra.student_cell, nat.GF_RNN_LSTM), (ra.teacher_cell, nat.GF_RNN_GRU)):
        cell.type, cell.hidden = kind, 24
        cell.w_ih = cell.w_hh = cell.b_ih = cell.b_hh = cell.h = FAKE
        cell.c = FAKE if kind == nat.GF_RNN_LSTM else None
    TR._set(ra, over)
    return ra


REFUSALS = [
    # rnn_check_cell's, per cell
    (dict(student_cell__w_ih=None), E_NULL), (dict(teacher_cell__w_hh=None), E_NULL), (dict(student_cell__b_ih=None), E_NULL),
    (dict(teacher_cell__b_hh=None), E_NULL), (dict(student_cell__h=None), E_NULL), (dict(teacher_cell__h=None), E_NULL),
    (dict(student_cell__c=None), E_NULL),                                                # an LSTM without c
    (dict(teacher_cell__c=FAKE), E_NULL), (dict(teacher_cell__c_save=FAKE), E_NULL),     # c with a GRU
    (dict(student_cell__type=0, student_cell__h_save=FAKE), E_NULL), (dict(teacher_cell__type=0, teacher_cell__h_save=FAKE), E_NULL),
    (dict(student_cell__type=0, student_cell__c_save=FAKE), E_NULL),
    (dict(student_cell__hidden=0), E_RANGE), (dict(teacher_cell__hidden=513), E_RANGE), (dict(student_cell__type=3), E_RANGE),
    (dict(teacher_cell__type=-1), E_RANGE),
    (dict(student_cell__type=0, teacher_cell__type=0, student_cell__h_save=None, student_cell__c_save=None, teacher_cell__h_save=None),
     E_UNSUPPORTED),                                                                     # gf_mlp_distill_act's launch
    # gf_mlp_distill_act's own, with its codes
    (dict(act__num_envs=-1), E_RANGE), (dict(act__std=None), E_NULL), (dict(act__actions=None), E_NULL), (dict(act__teacher_actions=None), E_NULL),
    (dict(act__student__layers__0__weight=None), E_NULL), (dict(act__teacher__layers__1__bias=None), E_NULL), (dict(act__teacher__inputs__0__rows=None), E_NULL),
    (dict(act__student__in_mean=FAKE), E_NULL), (dict(act__student__inputs__0__width=1025), E_RANGE), (dict(act__teacher__num_layers=7), E_RANGE),
    (dict(act__teacher__layers__0__out_width=513), E_RANGE), (dict(act__student__layers__1__out_width=65), E_RANGE),
    (dict(act__teacher__layers__1__out_width=4), E_RANGE),                               # output widths differ
    (dict(act__std_is_log=2), E_RANGE), (dict(act__student__num_layers=0), E_UNSUPPORTED), (dict(act__teacher__num_layers=0), E_UNSUPPORTED),
]


def test_abi_size_and_refusals():
    """Every refusal through the raw descriptor, with pointers that are never dereferenced: nothing is launched."""
    lib, nat = _lib()
    assert nat.GF_SIZEOF_MLP_RECURRENT_DISTILL == 40
    assert lib.gf_sizeof(40) == C.sizeof(nat.GfMlpRecurrentDistillArgs) == C.sizeof(nat.GfMlpDistillArgs) + 2 * C.sizeof(nat.GfRnnCell)
    assert lib.gf_sizeof(41) == -1
    assert callable(nat.HipBackend.mlp_recurrent_distill_act)
    assert lib.gf_mlp_recurrent_distill_act(None, None) == E_NULL
    for over, code in REFUSALS:
        assert lib.gf_mlp_recurrent_distill_act(C.byref(_fake_args(nat, **over)), None) == code, over
    assert lib.gf_mlp_recurrent_distill_act(C.byref(_fake_args(nat, n=0)), None) == 0, "no rows: a no-op"
    assert lib.gf_mlp_recurrent_distill_act(C.byref(_fake_args(nat, n=0, student_cell__h_save=FAKE, student_cell__c_save=FAKE, teacher_cell__type=0,
                                                               teacher_cell__h=None)), None) == 0


# ---- a distillation rollout with a recurrent student -----------------------------------------------------------------------------------
T_ROLLOUT = 6


def _env(n):
    from genesis_forge_amd import tasks

    # (episodes of four steps, and falls besides: every rollout has dones before its last step)
    env = tasks.Go2CommandDirectionEnv(num_envs=n, max_episode_length_s=0.08, cmd_resample_s=0.04, scene_kwargs=dict(ang_noise=0.6, seed=3))
    env.build()
    env.seed(7)
    return env


def _setup(kind, dev, n=12, T=T_ROLLOUT, teacher_recurrent=False, seed=0, hidden=(32, 16), H=24):
    from genesis_forge_amd.learner import RecurrentDistillForward, RolloutStorage, StudentTeacherRecurrent

    env = _env(n)
    obs, extras = env.reset()
    st = RolloutStorage(env, T).attach()
    st.begin(obs, extras)
    st.seed(5)
    A = env.action_space.shape[0]
    torch.manual_seed(seed)
    policy = StudentTeacherRecurrent(st.obs_width, st.obs_width, A, hidden, hidden, init_noise_std=0.3, rnn_type=kind, rnn_hidden_dim=H,
                                     teacher_recurrent=teacher_recurrent).to(dev)
    ref = RD.RslRlStudentTeacherRecurrent(st.obs_width, st.obs_width, A, hidden, hidden, rnn_type=kind, rnn_hidden_dim=H,
                                          teacher_recurrent=teacher_recurrent).to(dev)
    ref.load_state_dict(policy.state_dict())
    return env, st, policy, ref, RecurrentDistillForward(policy), {"obs": obs}


def _collect(env, st, fwd, state, noise_gen, dev, others=()):
    """One rollout through act_distill_recurrent; ``others`` (modules fed the same observations and resets) step along in torch.
    Returns, per step, the student state the step started from (after the reset) and what the others computed."""
    n, A = env.num_envs, env.action_space.shape[0]
    obs, starts, seen = state["obs"], [], []
    for t in range(st.num_steps):
        noise = None if noise_gen is None else torch.randn(n, A, generator=noise_gen).to(dev)
        pend = fwd._pending["student"]
        before = [x.clone() for x in fwd.state("student", n, dev) if x is not None]
        if pend is not None:
            for x in before:
                x[:, pend.bool()] = 0.0
        starts.append(before)
        actions = st.act_distill_recurrent(fwd, obs, noise=noise)
        with torch.no_grad():
            seen.append([(p.act_mean(obs.to(p.student[0].weight.dtype)), p.evaluate(obs.to(p.student[0].weight.dtype))) for p in others])
        obs, _r, _te, _tr, _extras = env.step(actions)
        st.process_env_step(None)
        fwd.reset(st.dones[t])
        for p in others:
            p.reset(st.dones[t])
            p.detach_hidden_states()
    state["obs"] = obs
    return starts, seen


@pytest.mark.parametrize("teacher_recurrent", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_act_distill_recurrent_keeps_the_start_state_cpu(oracle_backend, kind, teacher_recurrent):
    """Two rollouts on the oracle backend with rsl_rl's module stepped alongside: the teacher's stored actions and both hidden states
    bit for bit, and ``rnn_start["student"]`` is the state the rollout's first step started from, after the reset."""
    n = 12
    env, st, policy, ref, fwd, state = _setup(kind, "cpu", n, teacher_recurrent=teacher_recurrent)
    g = torch.Generator().manual_seed(4)
    with pytest.raises(RuntimeError, match="noise"):
        st.act_distill_recurrent(fwd, state["obs"])
    with pytest.raises(ValueError, match="RecurrentDistillForward"):
        st.act_distill_recurrent(object(), state["obs"])
    for rollout in range(2):
        starts, seen = _collect(env, st, fwd, state, g, "cpu", others=(ref,))
        for t in range(T_ROLLOUT):
            assert torch.equal(st.privileged_actions[t], seen[t][0][1]), (rollout, t)
        for a, b in zip(policy.get_hidden_states(), ref.get_hidden_states()):
            assert TR._states_equal(a, b)
        assert set(st.rnn_start) == {"student"}, "the teacher's start state is not kept"
        h, c = st.rnn_start["student"]
        assert torch.equal(h, starts[0][0][0]) and (c is None) == (kind == "gru") and (c is None or torch.equal(c, starts[0][1][0]))
        assert bool(st.dones[:-1].any())
        if rollout == 1:
            assert float(h.abs().max()) > 0 and bool((h[st.dones[-1]] == 0).all()), "after the reset: the rows done at the last step start from zeros"
    batches = list(st.step_batches(with_dones=True))
    assert len(batches) == T_ROLLOUT and all(len(b) == 3 for b in batches) and all(len(b) == 2 for b in st.step_batches())
    assert all(torch.equal(b[2], st.dones[t]) and b[1].data_ptr() == st.privileged_actions[t].data_ptr() for t, b in enumerate(batches))


# ---- Distillation.update against the restated loop ---------------------------------------------------------------------------------------
def _trained(policy):
    return torch.cat([p.detach().reshape(-1) for p in list(policy.student.parameters()) + list(policy.memory_s.parameters())])


def _frozen(policy):
    mods = [policy.teacher] + ([policy.memory_t] if policy.teacher_recurrent else [])
    std = policy.log_std if policy.noise_std_type == "log" else policy.std
    return torch.cat([p.detach().reshape(-1) for m in mods for p in m.parameters()] + [std.detach().reshape(-1)])


LR = 1e-3


def _update_vs_restatement(dev, kind, gl, loss_type, clip, teacher_recurrent=False, epochs=2, noise_gen=None, n=12):
    """Two collections, each followed by the restated update and ``Distillation.update`` on the same rollout, under the issue's
    bounds: the logged mean within 1e-4 relative; at least 0.995 of the trained parameters within 1e-4 + 1e-3·|p| and every one
    within Adam's per-step bound 2 · 3.2 · lr · (optimizer steps); the end state of ``memory_s`` within the first bound; the
    teacher, ``memory_t``, ``std`` and the teacher's state keep their bits."""
    from genesis_forge_amd.learner import Distillation

    env, st, policy, ref_policy, fwd, state = _setup(kind, dev, n, teacher_recurrent=teacher_recurrent)
    cfg = dict(num_learning_epochs=epochs, gradient_length=gl, learning_rate=LR, max_grad_norm=clip, loss_type=loss_type)
    alg, ref = Distillation(policy, st, class_name="Distillation", **cfg), RD.RslRlRecurrentDistillation(ref_policy, st, **cfg)
    assert alg.recurrent and alg.params.numel() == _trained(policy).numel() and any("memory_s" in k for k, p in policy.named_parameters() if p.requires_grad)
    lo, hi = alg.params.data_ptr(), alg.params.data_ptr() + 4 * alg.params.numel()
    assert all(lo <= p.data_ptr() < hi for p in policy.memory_s.parameters()), "memory_s lives in the flat buffer"
    frozen, before = _frozen(policy).clone(), _trained(policy).clone()
    steps = 0
    for it in range(2):
        _collect(env, st, fwd, state, noise_gen, dev)
        assert bool(st.dones[:-1].any()), "the rollout contains dones before its last step"
        teacher_state = [x.clone() for x in _states(policy.get_hidden_states()[1])]
        want = ref.update()
        got = alg.update()
        assert set(got) == {"behavior"}
        print(f"    {kind} gl={gl} {loss_type} clip={clip} update {it}: behavior {got['behavior']!r} vs {want['behavior']!r}")
        assert abs(got["behavior"] - want["behavior"]) <= 1e-4 * max(abs(want["behavior"]), 1e-6)
        steps += (epochs * T_ROLLOUT) // gl
        assert alg._calls == ref.num_steps == steps
        mine, theirs = _states(policy.get_hidden_states()[0]), _states(ref_policy.get_hidden_states()[0])
        assert len(mine) == len(theirs) == (2 if kind == "lstm" else 1)
        for x, y in zip(mine, theirs):
            assert not x.requires_grad and x.is_contiguous() and x.grad_fn is None and tuple(x.shape) == (1, n, 24)
            d = (x - y).abs()
            print(f"      end state: max |diff| {float(d.max()):.3e}")
            assert bool((d <= 1e-4 + 1e-3 * y.abs()).all()), float(d.max())
            assert bool((x[0, st.dones[-1]] == 0).all()), "the last dones are applied"
        for x, y in zip(_states(policy.get_hidden_states()[1]), teacher_state):
            assert torch.equal(x, y), "update() never touches the teacher's memory"
    a, b = _trained(policy), _trained(ref_policy)
    d = (a - b).abs()
    bulk = float((d <= 1e-4 + 1e-3 * b.abs()).float().mean())
    print(f"    trained parameters: share within 1e-4 + 1e-3|p| {bulk:.4f}, max |diff| {float(d.max()):.3e}, moved by up to {float((a - before).abs().max()):.3e}")
    assert bulk >= 0.995, f"only {bulk:.4f} of the parameters agree to 1e-4 + 1e-3|p| (max diff {float(d.max())})"
    assert float(d.max()) <= 2 * 3.2 * LR * steps
    assert float((a - before).abs().max()) > 0 and not torch.equal(_trained(policy)[-10:], before[-10:]), "memory_s is trained too"
    assert torch.equal(_frozen(policy), frozen), "the teacher, memory_t and std are never stepped"
    return alg, env, st, fwd, state


UPDATE_CASES = [("lstm", 1, "mse", None), ("lstm", 3, "mse", None), ("lstm", 7, "mse", None), ("gru", 1, "huber", None), ("gru", 3, "huber", 0.5),
                ("gru", 7, "mse", 0.5), ("lstm", 3, "huber", 0.5), ("lstm", 7, "huber", None), ("gru", 3, "mse", None), ("lstm", 1, "mse", 0.5)]
UPDATE_IDS = ["-".join(str(x) for x in c) for c in UPDATE_CASES]


@pytest.mark.parametrize("kind,gl,loss_type,clip", UPDATE_CASES, ids=UPDATE_IDS)
def test_update_matches_the_restatement_cpu(oracle_backend, kind, gl, loss_type, clip):
    _update_vs_restatement("cpu", kind, gl, loss_type, clip, noise_gen=torch.Generator().manual_seed(4))


def test_update_with_a_recurrent_teacher_cpu(oracle_backend):
    _update_vs_restatement("cpu", "gru", 3, "mse", None, teacher_recurrent=True, noise_gen=torch.Generator().manual_seed(4))


def test_the_pending_tail_is_dropped_but_advances_the_state(oracle_backend):
    """T = 6, gradient_length = 4, one epoch: exactly one Adam step — after step 4; steps 5 and 6 leave the parameters where it put them
    and no gradient behind, but the state ``memory_s`` is left with is that of all six steps."""
    from genesis_forge_amd.learner import Distillation

    env, st, policy, _ref, fwd, state = _setup("lstm", "cpu")
    _collect(env, st, fwd, state, torch.Generator().manual_seed(4), "cpu")
    twin = copy.deepcopy(policy)
    alg = Distillation(policy, st, num_learning_epochs=1, gradient_length=4)
    alg.update()
    assert alg._calls == 1
    after = _trained(policy).clone()
    # the same single step from the first four time steps alone, then all six steps of the stepped parameters' state
    opt = torch.optim.Adam(list(twin.student.parameters()) + list(twin.memory_s.parameters()), lr=1e-3)
    twin.reset(hidden_states=(tuple(x[None].clone() for x in st.rnn_start["student"]), None))
    loss = 0
    for t, (obs, target, dones) in enumerate(st.step_batches(with_dones=True)):
        if t < 4:
            loss = loss + torch.nn.functional.mse_loss(twin.act_mean(obs), target)
        if t == 3:
            loss.backward()
            opt.step()
            twin.detach_hidden_states()
        if t >= 4:
            with torch.no_grad():
                twin.act_mean(obs)
        twin.memory_s.hidden_states = tuple(torch.where(dones[None, :, None], 0.0, x) for x in twin.memory_s.hidden_states)
    d = (after - _trained(twin)).abs()
    assert bool((d <= 1e-6 + 1e-5 * after.abs()).all()), float(d.max())
    assert not bool(alg.grad_sync.bucket.any()), "what was pending is gone"
    for x, y in zip(policy.memory_s.hidden_states, twin.memory_s.hidden_states):
        assert float((x - y).abs().max()) <= 1e-5, "the tail advanced the state"


def test_recurrent_distillation_refusals(oracle_backend):
    from genesis_forge_amd.learner import Distillation, RecurrentDistillForward, StudentTeacherMLP

    env, st, policy, _ref, fwd, state = _setup("gru", "cpu", n=4, T=2)
    alg = Distillation(policy, st, gradient_length=2)
    with pytest.raises((ValueError, RuntimeError), match="act_distill"):
        alg.update()   # nothing collected
    g = torch.Generator().manual_seed(0)
    _collect(env, st, fwd, state, g, "cpu")
    st.rnn_start = {}
    with pytest.raises(ValueError, match="rnn_start"):
        alg.update()
    st.rnn_start = None
    with pytest.raises(ValueError, match="rnn_start"):
        alg.update()
    st.history = "frames"
    with pytest.raises(ValueError, match="frames"):
        alg.update()
    with pytest.raises(ValueError, match="memory_s"):
        RecurrentDistillForward(StudentTeacherMLP(5, 5, 3))   # (a feed-forward student: DistillForward's)
    with pytest.raises(ValueError, match="critic"):
        fwd.value(state["obs"])


# ---- the runner ----------------------------------------------------------------------------------------------------------------------
N_RUN = 70
GROUPS = {"policy": ["policy"], "teacher": ["policy"]}


def _cfg(kind="lstm", teacher_recurrent=False, **top):
    cfg = {"algorithm": {"class_name": "Distillation", "num_learning_epochs": 2, "gradient_length": 4, "learning_rate": 1e-3,
                         "max_grad_norm": 1.0, "loss_type": "mse"},
           "policy": {"class_name": "StudentTeacherRecurrent", "activation": "elu", "student_hidden_dims": [32, 16], "teacher_hidden_dims": [32, 16],
                      "init_noise_std": 0.3, "student_obs_normalization": True, "teacher_obs_normalization": True, "rnn_type": kind,
                      "rnn_hidden_dim": 24, "rnn_num_layers": 1, "teacher_recurrent": teacher_recurrent},
           "obs_groups": {k: list(v) for k, v in GROUPS.items()}, "seed": 1, "num_steps_per_env": T_ROLLOUT, "save_interval": 100}
    cfg.update(top)
    return cfg


def _built():
    env = _env(N_RUN)
    env.reset()
    return env


def _runner(env, dev, cfg, log_dir=None, forward="hip", noise_seed=None):
    from genesis_forge_amd.runner import DistillationRunner

    torch.manual_seed(0)
    noise = None if noise_seed is None else torch.Generator().manual_seed(noise_seed)
    return DistillationRunner(env, cfg, log_dir, device=dev, forward=forward, action_noise=noise)


def _teacher_checkpoint(dev, tmp_path, kind, recurrent, noise_seed=3):
    """A PPO teacher (recurrent or not) trained for one iteration on the same observations; returns the checkpoint's path."""
    from genesis_forge_amd.runner import OnPolicyRunner

    pol = {"activation": "elu", "actor_hidden_dims": [32, 16], "critic_hidden_dims": [32, 16], "init_noise_std": 0.8, "class_name": "ActorCritic"}
    if recurrent:
        pol.update(class_name="ActorCriticRecurrent", rnn_type=kind, rnn_hidden_dim=24, rnn_num_layers=1)
    cfg = {"algorithm": dict(TR.ALGO), "policy": pol, "seed": 1, "num_steps_per_env": T_ROLLOUT, "save_interval": 100, "empirical_normalization": True}
    torch.manual_seed(7)
    noise = None if noise_seed is None else torch.Generator().manual_seed(noise_seed)
    log = os.path.join(str(tmp_path), "teacher")
    OnPolicyRunner(_built(), cfg, log, device=dev, action_noise=noise).learn(1)
    return os.path.join(log, "model_0.pt")


def _state_of(r):
    alg = r.alg
    return [alg.params.clone(), alg.exp_avg.clone(), alg.exp_avg_sq.clone()] + [b.clone().to(torch.float32) for b in alg.policy.buffers()]


def _resume_flow(dev, tmp_path, kind, teacher_recurrent, noise_seed, forward="hip"):
    """Learn 2, save, learn 2 — against a fresh runner that loads the file on an env in the same place and learns 2: bit for bit,
    both hidden states included (they travel in this package's block of the checkpoint)."""
    path = _teacher_checkpoint(dev, tmp_path, kind, teacher_recurrent, None if noise_seed is None else noise_seed + 1)
    cfg = _cfg(kind, teacher_recurrent)

    def fresh(env):
        r = _runner(env, dev, copy.deepcopy(cfg), forward=forward, noise_seed=noise_seed)
        assert r.load(path) is None and r.current_learning_iteration == 0 and r.alg._calls == 0, "a PPO checkpoint gives the teacher only"
        return r

    a = fresh(_built())
    assert a.alg.recurrent and type(a.alg.policy).__name__ == "StudentTeacherRecurrent" and hasattr(a.alg.policy, "memory_t") == teacher_recurrent
    a.learn(2)
    logs = [a.last_log["behavior"]]
    ck = os.path.join(str(tmp_path), "a.pt")
    a.save(ck)
    a.learn(2)
    logs.append(a.last_log["behavior"])
    print(f"    behavior after 2 / 4 iterations: {logs[0]!r} / {logs[1]!r}")
    assert logs[1] < logs[0], "the student learns"
    env = _built()
    fresh(env).learn(2)   # (the env is where run A's was at the save)
    torch.manual_seed(1234)
    b = _runner(env, dev, _cfg(kind, teacher_recurrent, seed=99), forward=forward, noise_seed=None if noise_seed is None else noise_seed + 777)
    assert not torch.equal(b.alg.params, a.alg.params)
    assert b.load(ck) is None and b.current_learning_iteration == 1 and b.alg.policy.loaded_teacher
    b.learn(2)
    for i, (x, y) in enumerate(zip(_state_of(b), _state_of(a))):
        assert torch.equal(x, y), f"resumed run: tensor {i} differs by {float((x - y).abs().max())}"
    for x, y in zip(a.alg.policy.get_hidden_states(), b.alg.policy.get_hidden_states()):
        assert TR._states_equal(x, y)
    assert b.alg._calls == a.alg._calls == 4 * ((2 * T_ROLLOUT) // 4) and b.last_log["behavior"] == a.last_log["behavior"]
    saved = torch.load(ck, weights_only=False)
    mem = "st" if teacher_recurrent else "s"
    assert sorted(k for k in saved["model_state_dict"] if "memory" in k) == sorted(
        f"memory_{m}.rnn.{p}_l0" for m in mem for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
    hs = saved["genesis_forge_amd"]["hidden_states"]
    assert len(hs) == 2 and hs[0] is not None and (hs[1] is not None) == teacher_recurrent
    return a


@pytest.mark.parametrize("kind,teacher_recurrent", [("lstm", True), ("gru", False)])
def test_runner_learns_saves_and_resumes_exactly_cpu(oracle_backend, tmp_path, kind, teacher_recurrent):
    a = _resume_flow("cpu", tmp_path, kind, teacher_recurrent, noise_seed=21)
    # the inference policy keeps a hidden state of its own; reset(dones) zeroes rows, reset() all
    policy = a.get_inference_policy()
    before = [x.clone() for x in _states(a.alg.policy.get_hidden_states()[0])]
    g = torch.Generator().manual_seed(3)
    n, W = N_RUN, a.storage.obs_width
    xs = [torch.randn(n, W, generator=g) for _ in range(2)]
    first, second = policy(xs[0]), policy(xs[1])
    assert tuple(first.shape) == (n, a.alg.num_actions) and not a.alg.policy.training
    dones = torch.zeros(n, dtype=torch.bool)
    dones[::2] = True
    policy.reset(dones)
    third = policy(xs[0])
    assert torch.equal(third[dones], first[dones]) and not torch.equal(third[~dones], first[~dones]), "reset rows start over, the others go on"
    policy.reset()
    assert torch.equal(policy(xs[0]), first) and torch.equal(policy(xs[1]), second)
    for x, y in zip(before, _states(a.alg.policy.get_hidden_states()[0])):
        assert torch.equal(x, y), "the training state is untouched"


def test_runner_forwards_agree_bitwise_cpu(oracle_backend, tmp_path):
    """On the oracle backend both forwards are the module's torch step: the same parameters and loss after 2 iterations."""
    path = _teacher_checkpoint("cpu", tmp_path, "lstm", True)
    out = []
    for forward in ("hip", "torch"):
        r = _runner(_built(), "cpu", _cfg("lstm", True), forward=forward, noise_seed=11)
        r.load(path)
        r.learn(2)
        out.append((r.alg.params.clone(), r.last_log["behavior"], r.alg.policy.get_hidden_states()))
    assert torch.equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    for x, y in zip(out[0][2], out[1][2]):
        assert TR._states_equal(x, y)


def test_runner_refuses_a_mismatched_teacher(oracle_backend, tmp_path):
    path = _teacher_checkpoint("cpu", tmp_path, "gru", True)
    r = _runner(_built(), "cpu", _cfg("gru", False), noise_seed=1)
    with pytest.raises(ValueError, match="teacher"):
        r.learn(1)
    with pytest.raises(ValueError, match="teacher_recurrent"):
        r.load(path)


# ---- GPU: the kernel through the raw descriptor ---------------------------------------------------------------------------------------
class _Plain:
    """A net without a cell: the MLP alone (``kind`` "none"), as ``test_recurrent._Net`` otherwise."""

    def __init__(self, in_w, hidden, out, seed=0, norm=False):
        torch.manual_seed(seed)
        self.kind, self.in_w, self.H, self.out = "none", in_w, None, out
        self.mlp = TR._mlp([in_w, *hidden, out])
        self.norm = (torch.randn(in_w) * 0.5, torch.rand(in_w) + 0.5, 1e-2) if norm else None


class _PlainSpec:
    def __init__(self, net, x, views="1"):
        from types import SimpleNamespace

        self.net, self.n = net, x.shape[0]
        self.layers = [(m.weight.detach().cuda(), m.bias.detach().cuda()) for m in net.mlp if isinstance(m, torch.nn.Linear)]
        self.segs = TR._views(x, views)
        self.norm = None if net.norm is None else SimpleNamespace(_mean=net.norm[0].cuda(), _std=net.norm[1].cuda(), eps=net.norm[2])
        self.h = self.c = self.h_save = self.c_save = None


def _net(kind, in_w, H, hidden, out, seed, norm=False):
    return _Plain(in_w, hidden, out, seed, norm) if kind == "none" else TR._Net(kind, in_w, H, hidden, out, seed=seed, norm=norm)


def _spec(net, n, seed, views="1", reset=False, save=False, pad=0, misalign=False):
    """The same net, inputs, state and reset flags every time it is called with the same arguments: one for each launch compared."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, net.in_w, generator=g)
    if net.kind == "none":
        return _PlainSpec(net, x, views)
    h = torch.randn(n, net.H, generator=g) * 0.5
    c = torch.randn(n, net.H, generator=g) if net.kind == "lstm" else None
    flags = (torch.rand(n, generator=g) < 0.4) if reset else None
    return TR._Spec(net, x, h, c, views=views, reset=flags, save=save, misalign=misalign, pad=pad)


def _point_cell(nat, cell, spec):
    if spec.net.kind == "none":
        cell.type = nat.GF_RNN_NONE
        return
    cell.type, cell.hidden = (nat.GF_RNN_LSTM if spec.net.kind == "lstm" else nat.GF_RNN_GRU), spec.net.H
    cell.w_ih, cell.w_hh, cell.b_ih, cell.b_hh = (t.data_ptr() for t in spec.w)
    cell.h, cell.c = spec.h.data_ptr(), None if spec.c is None else spec.c.data_ptr()
    cell.reset = None if spec.reset is None else spec.reset.data_ptr()
    cell.h_save = None if spec.h_save is None else spec.h_save.data_ptr()
    cell.c_save = None if spec.c_save is None else spec.c_save.data_ptr()


def _sample_args(a, std, noise, is_log):
    a.std, a.std_is_log, a.noise = std.data_ptr(), is_log, None if noise is None else noise.data_ptr()
    a.seed, a.stream, a.env_offset = 0x1234ABCD5678, 3, 5


def _buffers(names, n, A, pad):
    return {k: torch.full((n + pad, A), SENTINEL, device="cuda") for k in names}


def _joined(backend, nat, n, student, teacher, std, noise, is_log, pad=0, optional=True, launch=True):
    """ONE gf_mlp_recurrent_distill_act launch; returns its outputs (``optional=False``: without mean and the two storage rows) and the
    descriptor (``launch=False``: the descriptor alone is built)."""
    from genesis_forge_amd.learner import _fill_net

    A = student.net.out
    ra = nat.GfMlpRecurrentDistillArgs()
    a = ra.act
    a.num_envs = n
    _fill_net(a.student, student.layers, student.segs, student.norm)
    _fill_net(a.teacher, teacher.layers, teacher.segs, teacher.norm)
    _point_cell(nat, ra.student_cell, student)
    _point_cell(nat, ra.teacher_cell, teacher)
    _sample_args(a, std, noise, is_log)
    names = ("mean", "actions", "actions_out", "teacher_actions", "teacher_actions_out") if optional else ("actions", "teacher_actions")
    out = _buffers(names, n, A, pad)
    for k, v in out.items():
        setattr(a, k, v.data_ptr())
    if launch:
        backend.mlp_recurrent_distill_act(ra)
        torch.cuda.synchronize()
    return out, ra


def _alone(backend, nat, n, spec, std=None, noise=None, is_log=0, pad=0):
    """``spec`` as the actor of a launch of its own — gf_mlp_recurrent_act, or gf_mlp_act for a net without a cell; sampled when ``std``
    is given.  Returns mean (and actions, actions_out)."""
    from genesis_forge_amd.learner import _fill_net

    A = spec.net.out
    if spec.net.kind == "none":
        ra = a = nat.GfMlpActArgs()
        a.num_envs = n
        _fill_net(a.actor, spec.layers, spec.segs, spec.norm)
        a.critic.num_layers = 0
        fn = backend.mlp_act
    else:
        ra = TR._fill_launch(nat, n, actor=spec)
        a = ra.act
        fn = backend.mlp_recurrent_act
    out = _buffers(("mean",) + (("actions", "actions_out") if std is not None else ()), n, A, pad)
    if std is not None:
        _sample_args(a, std, noise, is_log)
    for k, v in out.items():
        setattr(a, k, v.data_ptr())
    fn(ra)
    torch.cuda.synchronize()
    return out


def _state_tensors(spec):
    return {k: getattr(spec, k) for k in ("h", "c", "h_save", "c_save") if getattr(spec, k) is not None}


def _equal_to_separate_launches(backend, cells, n, Hs, in_ws, views, reset, save, norm, is_log, philox, seed):
    from genesis_forge_amd import _native as nat

    A, pad = 12, 3
    student = _net(cells[0], in_ws[0], Hs[0], (40, 36), A, seed=seed + 1, norm=norm[0])
    teacher = _net(cells[1], in_ws[1], Hs[1], (130, 24), A, seed=seed + 2, norm=norm[1])
    mk = lambda: (_spec(student, n, seed + 3, views[0], reset, save, pad), _spec(teacher, n, seed + 4, views[1], reset, save, pad, misalign=True))
    g = torch.Generator().manual_seed(seed + 5)
    std = torch.rand(A, generator=g) * 0.5 + 0.1
    std = (std.log() if is_log else std).cuda()
    noise = None if philox else torch.randn(n, A, generator=g).cuda()

    s1, t1 = mk()
    got, _ra = _joined(backend, nat, n, s1, t1, std, noise, is_log, pad)
    s2, t2 = mk()
    want = _alone(backend, nat, n, s2, std, noise, is_log, pad)
    teacher_mean = _alone(backend, nat, n, t2, pad=pad)["mean"]
    want["teacher_actions"] = want["teacher_actions_out"] = teacher_mean
    assert sorted(got) == sorted(want)
    for k in got:
        assert torch.equal(got[k], want[k]), f"{k}: max diff {float((got[k] - want[k]).abs().max())}"
        assert torch.isfinite(got[k][:n]).all() and float(got[k][:n].abs().max()) != SENTINEL, k
        assert float(got[k][n:].min()) == float(got[k][n:].max()) == SENTINEL, f"{k}: rows past num_envs are never written"
    assert not torch.equal(got["actions"], got["mean"]), "the student is sampled"
    for name, mine, theirs in (("student", s1, s2), ("teacher", t1, t2)):
        a, b = _state_tensors(mine), _state_tensors(theirs)
        want_keys = {"none": [], "gru": ["h"] + (["h_save"] if save else []), "lstm": ["c", "h"] + (["c_save", "h_save"] if save else [])}[mine.net.kind]
        assert sorted(a) == sorted(b) == sorted(want_keys)
        for k in a:
            assert torch.equal(a[k], b[k]), f"{name} {k}"
            assert float(a[k][n:].min()) == float(a[k][n:].max()) == SENTINEL, f"{name} {k}: rows past num_envs are never written"
        if mine.net.kind != "none":
            assert not torch.equal(a["h"][:n], _spec(mine.net, n, seed + (3 if name == "student" else 4), "1").h[:n]), "the state advanced"
            if reset and save:
                flags = mine.reset.bool()
                assert float(a["h_save"][:n][flags].abs().sum()) == 0.0, "h_save is the state after the reset"
    # without the optional destinations the required ones keep their bits
    s3, t3 = mk()
    bare, _ = _joined(backend, nat, n, s3, t3, std, noise, is_log, pad, optional=False)
    assert torch.equal(bare["actions"], got["actions"]) and torch.equal(bare["teacher_actions"], got["teacher_actions"])


CELL_CASES = [("lstm", "none"), ("gru", "none"), ("lstm", "lstm"), ("gru", "lstm"), ("none", "gru")]
# per cell case: N, (student H, teacher H), (student input width, teacher input width), (student segments, teacher segments) — every N,
# every H (128 / 129: one round / two; 160: idle waves in round two), every width (5: scalar loads, 48: vector loads, 516: two x passes)
# and both segmentations meet every cell case's student or teacher at least once across the rotation below
SHAPE_CASES = [(1, (1, 160), (5, 516), ("1", "3")), (31, (33, 129), (48, 5), ("3", "1")), (32, (128, 33), (516, 48), ("1", "3")),
               (33, (129, 1), (5, 48), ("3", "3")), (65, (160, 128), (48, 516), ("3", "1"))]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", range(len(SHAPE_CASES)), ids=lambda i: "n{}-H{}_{}-in{}_{}".format(SHAPE_CASES[i][0], *SHAPE_CASES[i][1], *SHAPE_CASES[i][2]))
@pytest.mark.parametrize("cells", CELL_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_one_launch_equals_the_separate_launches(hip_backend, cells, shape):
    """Every output and state of the one launch against gf_mlp_recurrent_act / gf_mlp_act launches of the student and of the teacher:
    ``torch.equal``, a sentinel behind row N.  Mixed reset flags; h_save / c_save given in the even shape cases; the given-noise and
    the Philox path, std and log_std by turns; the teacher's cell weights 4 bytes off a 16-byte boundary."""
    n, Hs, in_ws, views = SHAPE_CASES[shape]
    k = CELL_CASES.index(cells)
    _equal_to_separate_launches(hip_backend, cells, n, Hs, in_ws, views, reset=True, save=shape % 2 == 0, norm=(k % 2 == 0, shape % 2 == 1),
                                is_log=(k + shape) % 2, philox=(k + shape) % 3 == 0, seed=100 * k + shape)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 31, 32, 33, 65])
def test_every_n_without_resets_and_rows_alone(hip_backend, n):
    """No reset flags, no save: the bits of the separate launches again at every N, and row n depends on row n only — the last row
    launched alone (N = 1) equals the same row of the full launch."""
    from genesis_forge_amd import _native as nat

    _equal_to_separate_launches(hip_backend, ("lstm", "gru"), n, (160, 96), (48, 52), ("1", "1"), reset=False, save=False, norm=(True, False),
                                is_log=0, philox=False, seed=n)
    student, teacher = _net("gru", 48, 129, (64,), 12, seed=1, norm=True), _net("lstm", 52, 33, (32,), 12, seed=2)
    std, noise = torch.full((12,), 0.5).cuda(), torch.zeros(n, 12).cuda()
    s, t = _spec(student, n, 3), _spec(teacher, n, 4)
    full, _ = _joined(hip_backend, nat, n, s, t, std, noise, 0)
    s1, t1 = _spec(student, n, 3), _spec(teacher, n, 4)
    for sp in (s1, t1):   # the last row as a launch of one
        sp.segs = tuple(x[n - 1:].contiguous() for x in sp.segs)
        sp.h = sp.h[n - 1:].contiguous()
        sp.c = None if sp.c is None else sp.c[n - 1:].contiguous()
    one, _ = _joined(hip_backend, nat, 1, s1, t1, std, noise[n - 1:].contiguous(), 0)
    for k in full:
        assert torch.equal(one[k], full[k][n - 1:]), k
    assert torch.equal(s1.h, s.h[n - 1:]) and torch.equal(t1.h, t.h[n - 1:]) and torch.equal(t1.c, t.c[n - 1:])


@pytest.mark.gpu
def test_refusals_write_nothing(hip_backend):
    from genesis_forge_amd import _native as nat

    lib = hip_backend.lib
    lib.gf_mlp_recurrent_distill_act.restype, lib.gf_mlp_recurrent_distill_act.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    n = 40
    student, teacher = _net("lstm", 12, 24, (16,), 5, seed=1), _net("gru", 12, 24, (16,), 5, seed=2)
    s, t = _spec(student, n, 3, save=True), _spec(teacher, n, 4, save=True)
    before = [x.clone() for x in (s.h, s.c, t.h)]
    std, noise = torch.ones(5).cuda(), torch.zeros(n, 5).cuda()
    out, ra = _joined(hip_backend, nat, n, s, t, std, noise, 0, launch=False)

    def attempt(over):
        undo = TR._set(ra, over)
        rc = lib.gf_mlp_recurrent_distill_act(C.byref(ra), None)
        for obj, name, v in reversed(undo):
            setattr(obj, name, v)
        return rc

    real = [(o, c) for o, c in REFUSALS if all(v is None or v < FAKE for v in o.values())]   # (the rest are built on fake addresses)
    assert len(real) >= 22
    real += [(dict(teacher_cell__c=s.c.data_ptr()), E_NULL), (dict(student_cell__type=0, student_cell__c=None, student_cell__c_save=None), E_NULL)]
    for over, code in real:
        assert attempt(over) == code, over
    assert attempt(dict(act__num_envs=0)) == 0
    torch.cuda.synchronize()
    for x in list(out.values()) + [s.h_save, s.c_save, t.h_save]:
        assert float(x.min()) == float(x.max()) == SENTINEL
    for x, b in zip((s.h, s.c, t.h), before):
        assert torch.equal(x, b)


def _within(name, got, f32, ref, factor=4.0):
    """The issue's bound (``tests/test_recurrent.py``'s): the kernel's max error against float64 is at most 4 x that of torch's own
    float32 CPU run of the same inputs (printed before it is asserted)."""
    e_hip, e_torch = TR._err(got, ref), TR._err(f32, ref)
    print(f"    {name}: e_hip {e_hip:.3e}  e_torch {e_torch:.3e}  ratio {e_hip / max(e_torch, 1e-300):.2f}")
    assert e_hip <= factor * e_torch, f"{name}: e_hip {e_hip:.3e} > {factor} x e_torch {e_torch:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_accuracy_against_float64(hip_backend, kind, norm):
    """256 units, input width 48, N = 65: h', c', the student's mean and the teacher's output within 4 x torch's own float32 error."""
    from genesis_forge_amd import _native as nat

    n = 65
    student = TR._Net(kind, 48, 256, (256, 256, 256), 12, seed=1, norm=norm)
    teacher = TR._Net(kind, 48, 256, (256, 256, 256), 12, seed=2, norm=norm)
    xs, xt = TR._inputs(student, n, 3), TR._inputs(teacher, n, 4)
    s, t = TR._Spec(student, *xs), TR._Spec(teacher, *xt)
    out, _ = _joined(hip_backend, nat, n, s, t, torch.ones(12).cuda(), torch.zeros(n, 12).cuda(), 0)
    print(f"  {kind} norm={norm}")
    for name, net, spec, x, y in (("student", student, s, xs, out["mean"]), ("teacher", teacher, t, xt, out["teacher_actions"])):
        h64, c64, y64 = net.reference(*x, torch.float64)
        h32, c32, y32 = net.reference(*x, torch.float32)
        _within(f"{name} h'", spec.h, h32, h64)
        if kind == "lstm":
            _within(f"{name} c'", spec.c, c32, c64)
        _within(f"{name} {'mean' if name == 'student' else 'output'}", y, y32, y64)


# ---- GPU: the storage, the update, the runner -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,teacher_recurrent", [("lstm", True), ("gru", False)])
def test_act_distill_recurrent_writes_its_rows_and_the_start_state(hip_backend, kind, teacher_recurrent):
    """Eight steps over a storage of three rows (the wrap into later rollouts) against ``RecurrentDistillForward.act`` of a twin policy
    stepped from copies of the states: the sample (the launch's own Philox draws: seed and stream as act_policy's), both rows, both
    states, and at row 0 the start state — the pre-step state with the pending reset applied."""
    from genesis_forge_amd.learner import RecurrentDistillForward

    n = 45
    env, st, policy, _ref, fwd, state = _setup(kind, "cuda", n, T=3, teacher_recurrent=teacher_recurrent)
    twin = copy.deepcopy(policy)
    fwd2 = RecurrentDistillForward(twin)
    f64 = copy.deepcopy(policy).double()
    obs, resets = state["obs"], 0
    for i in range(8):
        t = i % 3
        for name in fwd._memory:   # the twin starts the step where the policy does
            twin_m, hs = fwd2._memory[name], fwd._memory[name].hidden_states
            twin_m.hidden_states = None if hs is None else (tuple(x.clone() for x in hs) if isinstance(hs, tuple) else hs.clone())
            fwd2._pending[name] = None if fwd._pending[name] is None else fwd._pending[name].clone()
        pend = fwd._pending["student"]
        hs = _states(policy.memory_s.hidden_states)
        start = [x[0].clone() for x in hs] if hs else [torch.zeros(n, 24, device="cuda") for _ in range(2 if kind == "lstm" else 1)]
        if pend is not None:
            for x in start:
                x[pend.bool()] = 0.0
        stream = st._act_stream
        actions = st.act_distill_recurrent(fwd, obs)
        want_a, want_t = fwd2.act(obs, seed=5, stream=stream, env_offset=0)
        assert torch.equal(actions, want_a) and torch.equal(st.actions[t], actions) and torch.equal(st.privileged_actions[t], want_t), f"call {i}: row {t}"
        for a, b in zip(policy.get_hidden_states(), twin.get_hidden_states()):
            assert TR._states_equal(a, b)
        assert all(v is None for v in fwd._pending.values()), "the launch consumed the pending resets"
        if t == 0:
            kept = [x for x in st.rnn_start["student"] if x is not None]
            assert set(st.rnn_start) == {"student"} and len(kept) == len(start) and all(torch.equal(a, b) for a, b in zip(kept, start)), f"call {i}"
        with torch.no_grad():
            want64 = f64.evaluate(obs.double())
        assert float((want_t.double() - want64).abs().max()) <= 1e-4, "the stored teacher actions are the module's within float32 rounding"
        obs, _r, _te, _tr, _extras = env.step(actions)
        st.process_env_step(None)
        fwd.reset(st.dones[t])
        f64.reset(st.dones[t])
        resets += int(st.dones[t].sum())
    assert resets > 0 and st.values is None and st.mu is None, "resets happened; no PPO rows"


@pytest.mark.gpu
@pytest.mark.parametrize("kind,gl,loss_type,clip,teacher_recurrent", [("lstm", 3, "mse", None, False), ("gru", 7, "huber", 0.5, True),
                                                                      ("lstm", 1, "huber", 0.5, True), ("gru", 3, "mse", None, False)])
def test_update_matches_the_restatement_hip(hip_backend, kind, gl, loss_type, clip, teacher_recurrent):
    alg, env, st, fwd, state = _update_vs_restatement("cuda", kind, gl, loss_type, clip, teacher_recurrent=teacher_recurrent, n=45)
    _collect(env, st, fwd, state, None, "cuda")
    with host_reads() as c:
        alg.update()
    assert c[0] == 1, f"Distillation.update read the device {c[0]} times"
    st.act_distill_recurrent(fwd, state["obs"])   # the state update() left is one the next launch steps in place


@pytest.mark.gpu
def test_runner_resume_is_exact_hip(hip_backend, tmp_path):
    a = _resume_flow("cuda", tmp_path, "lstm", True, noise_seed=None)
    policy = a.get_inference_policy()
    n, W = N_RUN, a.storage.obs_width
    x = torch.randn(n, W, generator=torch.Generator().manual_seed(3)).cuda()
    first, second = policy(x), policy(x)
    dones = torch.zeros(n, dtype=torch.bool, device="cuda")
    dones[::2] = True
    policy.reset(dones)
    third = policy(x)
    assert torch.equal(third[dones], first[dones]) and not torch.equal(third[~dones], first[~dones])
    policy.reset()
    assert torch.equal(policy(x), first) and torch.equal(policy(x), second)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,teacher_recurrent", [("gru", True), ("lstm", False)])
def test_runner_hip_and_torch_forwards_agree(hip_backend, tmp_path, kind, teacher_recurrent):
    """learn(2) with forward="hip" and forward="torch" from the same seed and the same given noise: the two forwards differ by float32
    rounding only, the logged behaviour loss agrees within 1e-4 relative (``tests/test_distillation.py``'s comparison)."""
    path = _teacher_checkpoint("cuda", tmp_path, kind, teacher_recurrent, noise_seed=None)
    logs = []
    for forward in ("hip", "torch"):
        r = _runner(_built(), "cuda", _cfg(kind, teacher_recurrent), forward=forward, noise_seed=11)
        r.load(path)
        r.learn(2)
        assert r.alg._calls == 2 * ((2 * T_ROLLOUT) // 4) and r.storage.privileged_actions is not None
        logs.append(r.last_log["behavior"])
    print(f"    behavior: hip {logs[0]!r}, torch {logs[1]!r}, relative difference {abs(logs[0] - logs[1]) / abs(logs[1]):.3e}")
    assert abs(logs[0] - logs[1]) <= 1e-4 * abs(logs[1])
