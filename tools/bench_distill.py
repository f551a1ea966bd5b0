"""Teacher–student distillation at the go2_cmd shapes: the collection step's forward in three forms, and one update in two.

usage: python tools/bench_distill.py [--sizes 4096,16384,65536] [--steps 24] [--gradient-length 15] [--reps 7] [--calls 50]
                                     [--parts collect,update] [--out FILE]

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
synchronisations (``--calls`` collection steps per rep).  Prints one JSON line per size, part and form: best and median."""
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
    return {k: (min(v), statistics.median(v)) for k, v in times.items()}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,65536")
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--gradient-length", type=int, default=15)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--parts", default="collect,update")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genesis_forge_amd import gs

    gs.set_device("cuda:0")
    lines = []
    for n in (int(x) for x in args.sizes.split(",")):
        if "collect" in args.parts.split(","):
            for form, (best, med) in run_forms(collect_forms(n), args.reps, args.calls).items():
                lines.append({"part": "collect", "envs": n, "form": form, "best_us_per_step": best * 1e6, "median_us_per_step": med * 1e6})
                print(json.dumps(lines[-1]), flush=True)
        if "update" in args.parts.split(","):
            forms, out = update_forms(n, args.steps, args.gradient_length)
            for form, (best, med) in run_forms(forms, args.reps, 1).items():
                lines.append({"part": "update", "envs": n, "steps": args.steps, "gradient_length": args.gradient_length, "form": form,
                              "best_ms_per_update": best * 1e3, "median_ms_per_update": med * 1e3, "behavior": out[form]["behavior"]})
                print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
