"""Teacher–student distillation at the go2_cmd shapes: the collection step's forward in three forms, and one update in two.

usage: python tools/bench_distill.py [--sizes 4096,16384,65536] [--steps 24] [--gradient-length 15] [--reps 7] [--calls 50]
                                     [--parts collect,update] [--out FILE]
                                     [--policy mlp|recurrent] [--rnn-type lstm|gru] [--teacher-recurrent]

The student reads a 5-frame history of the 48-wide go2_cmd observation (240 columns), the teacher the newest frame and 187 terrain
heights (235 columns); both are the reference's 512-256-128 ELU MLPs with 12 actions.  Inputs are random rows — no env: every launch
between two synchronisations belongs to the form being timed.

collect — per collection step, what produces the sampled student actions, the teacher's actions and the two storage rows:
  distill_act   ONE gf_mlp_distill_act launch (learner.DistillForward.act)
  two_mlp_act   two gf_mlp_act launches: the student with sampling and its storage row, the teacher mean-only into its row
  torch         policy.act_mean + policy.evaluate in torch, gf_policy_act for the sample and a copy_ of the teacher's actions
update — one update over T stored steps (``gradient_length`` 15, one epoch, mse):
  fused         learner.Distillation.update (gf_bc_loss + gf_adam_step, one host read)
  rsl_rl        tests/rsl_rl_distillation.py (torch.optim.Adam, an .item() per step)
Every rep runs each form once, alternating, after one warm-up per form; a rep is timed with the host clock between two device
synchronisations (``--calls`` collection steps per rep).  Prints one JSON line per size, part and form: best and median.

``--policy recurrent`` (a 256-unit LSTM / GRU in front of the student's MLP, with ``--teacher-recurrent`` in front of the teacher's too;
the default ``mlp`` and its output are unchanged) times the same two parts; its lines carry ``policy``, ``rnn_type``,
``teacher_recurrent`` and, as the spread of the repeats, the slowest rep beside best and median:
collect
  recurrent_distill_act   ONE gf_mlp_recurrent_distill_act launch (learner.RecurrentDistillForward.act)
  two_launches            gf_mlp_recurrent_act for the student (sampling, its storage row) + gf_mlp_act for the teacher, or a second
                          gf_mlp_recurrent_act where the teacher is recurrent
  torch                   the module's torch step (act_mean + evaluate), gf_policy_act for the sample and a copy_ of the teacher's actions
update (2 % of the stored steps are dones)
  fused                   learner.Distillation.update: one backward per window of ``gradient_length`` steps, gf_bc_loss + gf_adam_step
  restated                tests/rsl_rl_distillation_recurrent.py (torch.optim.Adam, an .item() per step)"""
import argparse
import copy
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genesis-forge_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))   # the torch restatement of rsl_rl's update is test infrastructure

import torch  # noqa: E402

STUDENT_W, TEACHER_W, A, HIDDEN = 5 * 48, 48 + 187, 12, (512, 256, 128)
RNN_HIDDEN = 256


def timed(fn, calls: int) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def run_forms(forms: dict, reps: int, calls: int) -> dict:
    for fn in forms.values():   # one warm-up per form
        timed(fn, 1)
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            times[k].append(timed(fn, calls))
    return {k: (min(v), statistics.median(v), max(v)) for k, v in times.items()}


def collect_forms(n: int):
    from genesis_forge_amd import _native as nat
    from genesis_forge_amd.learner import DistillForward, StudentTeacherMLP, _fill_net

    backend = nat.get_backend()
    torch.manual_seed(0)
    policy = StudentTeacherMLP(STUDENT_W, TEACHER_W, A, HIDDEN, HIDDEN).cuda()
    fwd = DistillForward(policy)
    g = torch.Generator(device="cuda").manual_seed(1)
    obs, tobs = torch.randn(n, STUDENT_W, device="cuda", generator=g), torch.randn(n, TEACHER_W, device="cuda", generator=g)
    row_a, row_t = torch.zeros(n, A, device="cuda"), torch.zeros(n, A, device="cuda")
    stream = [0]

    def distill_act():
        stream[0] += 1
        return fwd.act(obs, tobs, seed=3, stream=stream[0], actions_out=row_a, teacher_actions_out=row_t, backend=backend)

    sa, ta = nat.GfMlpActArgs(), nat.GfMlpActArgs()
    actions = torch.empty(n, A, device="cuda")
    for a, layers, x in ((sa, fwd.student, obs), (ta, fwd.teacher, tobs)):
        a.num_envs = n
        _fill_net(a.actor, layers, (x,), None)
    sa.std, sa.seed, sa.actions, sa.actions_out = policy.std.data_ptr(), 3, actions.data_ptr(), row_a.data_ptr()
    ta.mean = row_t.data_ptr()

    def two_mlp_act():
        stream[0] += 1
        sa.stream = stream[0]
        backend.mlp_act(sa)
        backend.mlp_act(ta)

    pa = nat.GfPolicyActArgs()
    pa.num_envs, pa.num_actions, pa.seed = n, A, 3
    pa.std, pa.actions, pa.actions_out = policy.std.data_ptr(), actions.data_ptr(), row_a.data_ptr()

    def torch_forward():
        stream[0] += 1
        with torch.no_grad():
            mean, teacher = policy.act_mean(obs), policy.evaluate(tobs)
        pa.mean, pa.stream = mean.data_ptr(), stream[0]
        backend.policy_act(pa)
        row_t.copy_(teacher)

    return {"distill_act": distill_act, "two_mlp_act": two_mlp_act, "torch": torch_forward}


def update_forms(n: int, T: int, gradient_length: int):
    from genesis_forge_amd import _native as nat
    from genesis_forge_amd.learner import Distillation, RolloutStorage, StudentTeacherMLP
    from rsl_rl_distillation import RslRlDistillation

    mk = lambda name, w: SimpleNamespace(name=name, observation_space=SimpleNamespace(shape=(w,)), output="fresh", _history_len=1, _unrolled=False)
    env = SimpleNamespace(num_envs=n, managers={"observation": [mk("policy", STUDENT_W)]}, backend=nat.get_backend())
    st = RolloutStorage(env, T, obs_groups={"policy": ["policy"]})
    st._ensure_distill_rows(A)
    g = torch.Generator(device="cuda").manual_seed(0)
    for t in (st.observations, st.privileged_actions):
        t.copy_(torch.randn(t.shape, device="cuda", generator=g))
    torch.manual_seed(0)
    policy = StudentTeacherMLP(STUDENT_W, TEACHER_W, A, HIDDEN, HIDDEN).cuda()
    ref_policy = copy.deepcopy(policy)
    cfg = dict(num_learning_epochs=1, gradient_length=gradient_length, learning_rate=1e-3, max_grad_norm=None, loss_type="mse")
    alg = Distillation(policy, st, **cfg)
    start, ref_start = alg.params.clone(), copy.deepcopy(ref_policy.state_dict())
    out = {}

    def fused():
        alg.params.copy_(start)   # the initial weights and a fresh optimizer state, without a host read
        alg.exp_avg.zero_(), alg.exp_avg_sq.zero_(), alg._state.zero_()
        alg._state_lr[0] = cfg["learning_rate"]
        alg._calls = 0
        out["fused"] = alg.update()

    def rsl_rl():
        ref_policy.load_state_dict(ref_start)
        out["rsl_rl"] = RslRlDistillation(ref_policy, st, **cfg).update()

    return {"fused": fused, "rsl_rl": rsl_rl}, out


def _recurrent_policy(rnn_type: str, teacher_recurrent: bool):
    from genesis_forge_amd.learner import StudentTeacherRecurrent

    torch.manual_seed(0)
    return StudentTeacherRecurrent(STUDENT_W, TEACHER_W, A, HIDDEN, HIDDEN, rnn_type=rnn_type, rnn_hidden_dim=RNN_HIDDEN,
                                   teacher_recurrent=teacher_recurrent).cuda()


def recurrent_collect_forms(n: int, rnn_type: str, teacher_recurrent: bool):
    from genesis_forge_amd import _native as nat
    from genesis_forge_amd.learner import RecurrentDistillForward, _fill_net

    backend = nat.get_backend()
    policy = _recurrent_policy(rnn_type, teacher_recurrent)
    fwd = RecurrentDistillForward(policy)
    g = torch.Generator(device="cuda").manual_seed(1)
    obs, tobs = torch.randn(n, STUDENT_W, device="cuda", generator=g), torch.randn(n, TEACHER_W, device="cuda", generator=g)
    row_a, row_t = torch.zeros(n, A, device="cuda"), torch.zeros(n, A, device="cuda")
    stream = [0]

    def recurrent_distill_act():
        stream[0] += 1
        return fwd.act(obs, tobs, seed=3, stream=stream[0], actions_out=row_a, teacher_actions_out=row_t, backend=backend)

    # the two launches step states of their own
    actions = torch.empty(n, A, device="cuda")
    keep = []

    def cell_of(cell, rnn):
        h = torch.zeros(n, RNN_HIDDEN, device="cuda")
        c = torch.zeros(n, RNN_HIDDEN, device="cuda") if rnn_type == "lstm" else None
        keep.append((h, c))
        cell.type, cell.hidden = (nat.GF_RNN_LSTM if rnn_type == "lstm" else nat.GF_RNN_GRU), RNN_HIDDEN
        cell.w_ih, cell.w_hh, cell.b_ih, cell.b_hh = (getattr(rnn, p).data_ptr() for p in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"))
        cell.h, cell.c = h.data_ptr(), None if c is None else c.data_ptr()

    sa = nat.GfMlpRecurrentActArgs()
    sa.act.num_envs = n
    _fill_net(sa.act.actor, fwd.student, (obs,), None)
    cell_of(sa.actor_cell, policy.memory_s.rnn)
    sa.act.std, sa.act.seed, sa.act.actions, sa.act.actions_out = policy.std.data_ptr(), 3, actions.data_ptr(), row_a.data_ptr()
    if teacher_recurrent:
        ta = nat.GfMlpRecurrentActArgs()
        ta.act.num_envs = n
        _fill_net(ta.act.actor, fwd.teacher, (tobs,), None)
        cell_of(ta.actor_cell, policy.memory_t.rnn)
        ta.act.mean = row_t.data_ptr()
        teacher_launch = lambda: backend.mlp_recurrent_act(ta)
    else:
        ta = nat.GfMlpActArgs()
        ta.num_envs = n
        _fill_net(ta.actor, fwd.teacher, (tobs,), None)
        ta.mean = row_t.data_ptr()
        teacher_launch = lambda: backend.mlp_act(ta)

    def two_launches():
        stream[0] += 1
        sa.act.stream = stream[0]
        backend.mlp_recurrent_act(sa)
        teacher_launch()

    pa = nat.GfPolicyActArgs()
    pa.num_envs, pa.num_actions, pa.seed = n, A, 3
    pa.std, pa.actions, pa.actions_out = policy.std.data_ptr(), actions.data_ptr(), row_a.data_ptr()
    module = copy.deepcopy(policy)   # (a module of its own: its memories hold torch's state tensors)

    def torch_forward():
        stream[0] += 1
        with torch.no_grad():
            mean, teacher = module.act_mean(obs), module.evaluate(tobs)
        pa.mean, pa.stream = mean.data_ptr(), stream[0]
        backend.policy_act(pa)
        row_t.copy_(teacher)

    return {"recurrent_distill_act": recurrent_distill_act, "two_launches": two_launches, "torch": torch_forward}


def recurrent_update_forms(n: int, T: int, gradient_length: int, rnn_type: str, teacher_recurrent: bool):
    from genesis_forge_amd import _native as nat
    from genesis_forge_amd.learner import Distillation, RolloutStorage
    from rsl_rl_distillation_recurrent import RslRlRecurrentDistillation, RslRlStudentTeacherRecurrent

    mk = lambda name, w: SimpleNamespace(name=name, observation_space=SimpleNamespace(shape=(w,)), output="fresh", _history_len=1, _unrolled=False)
    env = SimpleNamespace(num_envs=n, managers={"observation": [mk("policy", STUDENT_W)]}, backend=nat.get_backend())
    st = RolloutStorage(env, T, obs_groups={"policy": ["policy"]})
    st._ensure_distill_rows(A)
    g = torch.Generator(device="cuda").manual_seed(0)
    for t in (st.observations, st.privileged_actions):
        t.copy_(torch.randn(t.shape, device="cuda", generator=g))
    st.dones.copy_(torch.rand(st.dones.shape, device="cuda", generator=g) < 0.02)
    state = lambda: torch.randn(n, RNN_HIDDEN, device="cuda", generator=g) * 0.1
    st.rnn_start = {"student": (state(), state() if rnn_type == "lstm" else None)}
    policy = _recurrent_policy(rnn_type, teacher_recurrent)
    ref_policy = RslRlStudentTeacherRecurrent(STUDENT_W, TEACHER_W, A, HIDDEN, HIDDEN, rnn_type=rnn_type, rnn_hidden_dim=RNN_HIDDEN,
                                              teacher_recurrent=teacher_recurrent).cuda()
    ref_policy.load_state_dict(policy.state_dict())
    cfg = dict(num_learning_epochs=1, gradient_length=gradient_length, learning_rate=1e-3, max_grad_norm=None, loss_type="mse")
    alg = Distillation(policy, st, **cfg)
    start, ref_start = alg.params.clone(), copy.deepcopy(ref_policy.state_dict())
    out = {}

    def fused():
        alg.params.copy_(start)   # the initial weights and a fresh optimizer state, without a host read
        alg.exp_avg.zero_(), alg.exp_avg_sq.zero_(), alg._state.zero_()
        alg._state_lr[0] = cfg["learning_rate"]
        alg._calls = 0
        out["fused"] = alg.update()

    def restated():
        ref_policy.load_state_dict(ref_start)
        out["restated"] = RslRlRecurrentDistillation(ref_policy, st, **cfg).update()

    return {"fused": fused, "restated": restated}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,65536")
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--gradient-length", type=int, default=15)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--parts", default="collect,update")
    ap.add_argument("--out", default=None)
    ap.add_argument("--policy", default="mlp", choices=("mlp", "recurrent"))
    ap.add_argument("--rnn-type", default="lstm", choices=("lstm", "gru"))
    ap.add_argument("--teacher-recurrent", action="store_true")
    args = ap.parse_args()
    recurrent = args.policy == "recurrent"
    tag = {"policy": "recurrent", "rnn_type": args.rnn_type, "teacher_recurrent": args.teacher_recurrent} if recurrent else {}
    spread = lambda worst, scale, unit: {f"max_{unit}": worst * scale} if recurrent else {}
    from genesis_forge_amd import gs

    gs.set_device("cuda:0")
    lines = []
    for n in (int(x) for x in args.sizes.split(",")):
        if "collect" in args.parts.split(","):
            forms = recurrent_collect_forms(n, args.rnn_type, args.teacher_recurrent) if recurrent else collect_forms(n)
            for form, (best, med, worst) in run_forms(forms, args.reps, args.calls).items():
                lines.append({"part": "collect", "envs": n, **tag, "form": form, "best_us_per_step": best * 1e6, "median_us_per_step": med * 1e6,
                              **spread(worst, 1e6, "us_per_step")})
                print(json.dumps(lines[-1]), flush=True)
        if "update" in args.parts.split(","):
            if recurrent:
                forms, out = recurrent_update_forms(n, args.steps, args.gradient_length, args.rnn_type, args.teacher_recurrent)
            else:
                forms, out = update_forms(n, args.steps, args.gradient_length)
            for form, (best, med, worst) in run_forms(forms, args.reps, 1).items():
                lines.append({"part": "update", "envs": n, **tag, "steps": args.steps, "gradient_length": args.gradient_length, "form": form,
                              "best_ms_per_update": best * 1e3, "median_ms_per_update": med * 1e3, **spread(worst, 1e3, "ms_per_update"),
                              "behavior": out[form]["behavior"]})
                print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
