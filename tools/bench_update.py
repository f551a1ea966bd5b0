"""One PPO update (num_learning_epochs x num_mini_batches = 5 x 4 minibatches) of the reference's training configs: rsl_rl's
PPO.update restated in torch (tests/rsl_rl_ppo.py: torch.optim.Adam, clip_grad_norm_, the .item() calls) against learner.PPO
(gf_ppo_loss + gf_adam_step, one host read per update).

usage: python tools/bench_update.py [--sizes go2_cmd:4096,go2_cmd:16384,go2_cmd:65536,gait:4096] [--steps 24] [--reps 7]
                                    [--forms rsl_rl,fused] [--out FILE] [--noise-std-type scalar|log]
                                    [--symmetry none|augment|mirror|both] [--rnd]
                                    [--policy mlp|recurrent] [--rnn-type lstm|gru] [--rnn-hidden-dim 256]

Per size: one rollout of T steps is collected with act / process_env_step by the reference policy (ELU MLPs 512-256-128, as
examples/*/train.py) and its returns computed; then every rep runs each form once, alternating, from the same initial weights,
a fresh optimizer state and the same minibatch stream (the generator's seed), so only the update differs.  A rep is timed with
the host clock from a device synchronise to the device synchronise that ends it.  ``gait`` uses the gait trainer's asymmetric
critic (obs_groups {"policy": ["policy"], "critic": ["policy", "critic"]}).  Prints one JSON line per size and form: best and
median ms per update over the reps (after one warm-up update per form), and the losses of the last rep.
``--synthetic``: random storage rows instead of a rollout — two such runs of one form under ``rocprofv3 --kernel-trace --stats``
that differ only in ``--reps`` differ by exactly that many updates, which gives the dispatches per minibatch.
``--noise-std-type log``: the policy holds ``log_std`` (the torch restatement reads ``std = exp(log_std)`` through a property).
``--symmetry``: both forms get rsl_rl's ``symmetry_cfg`` with the Go2 left/right mirror (``go2_mirror``) — ``augment``: data
augmentation, ``mirror``: the mirror loss, ``both``; the torch form is then tests/rsl_rl_symmetry.py.
``--rnd``: both forms get rsl_rl's ``rnd_cfg`` (``rnd_state`` = the policy observation, a 256-128 predictor and target with 16
outputs, both normalisers on): every minibatch also trains the predictor; the torch form is then tests/rsl_rl_rnd.py.
``--policy recurrent [--rnn-type lstm|gru] [--rnn-hidden-dim 256]``: an ``ActorCriticRecurrent`` policy, its rollout collected with
``act_recurrent``; ``fused`` is ``learner.PPO`` on the trajectory minibatches (gf_traj_table, gf_traj_gather), ``rsl_rl`` is
tests/rsl_rl_recurrent.py (``split_and_pad_trajectories`` once per update, the per-step saved hidden states)."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genesis-forge_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))   # the torch restatement of rsl_rl's update is test infrastructure

import torch  # noqa: E402

ALGO = dict(class_name="PPO", clip_param=0.2, desired_kl=0.01, entropy_coef=0.01, gamma=0.99, lam=0.95, learning_rate=0.001, max_grad_norm=1.0,
            num_learning_epochs=5, num_mini_batches=4, schedule="adaptive", use_clipped_value_loss=True, value_loss_coef=1.0)
GAIT_GROUPS = {"policy": ["policy"], "critic": ["policy", "critic"]}
RND_CFG = dict(num_outputs=16, predictor_hidden_dims=[256, 128], target_hidden_dims=[256, 128], weight=0.1, state_normalization=True,
               reward_normalization=True, learning_rate=1e-3)


def obs_groups(config: str, rnd: bool):
    """The storage's observation groups: the gait trainer's asymmetric critic, and the policy observation as ``rnd_state`` with --rnd."""
    groups = dict(GAIT_GROUPS) if config == "gait" else ({"policy": ["policy"], "critic": ["policy"]} if rnd else None)
    if rnd:
        groups["rnd_state"] = ["policy"]
    return groups


def make_policy(num_obs: int, A: int, noise_std_type: str):
    """ActorCriticMLP; for "log" with a ``std`` property = ``exp(log_std)``, which is what rsl_rl's distribution update computes and
    what tests/rsl_rl_ppo.py reads (autograd reaches log_std through it)."""
    from genesis_forge_amd.learner import ActorCriticMLP

    if noise_std_type != "log":
        return ActorCriticMLP(num_obs, A)

    class LogStdPolicy(ActorCriticMLP):
        std = property(lambda self: self.log_std.exp())

    return LogStdPolicy(num_obs, A, noise_std_type="log")


def rollout(config: str, n: int, T: int, noise_std_type: str = "scalar", rnd: bool = False):
    from genesis_forge_amd.learner import ActorCriticMLP, RolloutStorage
    from genesis_forge_amd.tasks import BASELINE_CONFIGS

    env = BASELINE_CONFIGS[config][1](n)
    env.build()
    env.seed(1)
    obs, extras = env.reset()
    st = RolloutStorage(env, T, obs_groups=obs_groups(config, rnd)).attach()
    st.begin(obs, extras)
    st.seed(2)
    A = env.action_space.shape[0]
    critic = st.obs_groups["critic"]
    critic_w = sum(st.group_rows[m].shape[2] for m in critic)
    torch.manual_seed(0)
    policy = make_policy(st.obs_width, A, noise_std_type).cuda()
    is_log = noise_std_type == "log"
    if critic_w != st.obs_width:
        policy.critic = ActorCriticMLP(critic_w, A).critic.cuda()
    cat = lambda o, ex: o if critic == st.obs_groups["policy"] else torch.cat([ex["observations"][m] for m in critic], dim=-1)
    for _ in range(T):
        with torch.no_grad():
            mean, values = policy.act_mean(obs), policy.evaluate(cat(obs, extras))
        actions = st.act(mean, (policy.log_std if is_log else policy.std).detach(), values, std_is_log=is_log)
        obs, _r, _te, tr, extras = env.step(actions)
        st.process_env_step(tr)
    with torch.no_grad():
        st.compute_returns(policy.evaluate(cat(obs, extras)), gamma=ALGO["gamma"], lam=ALGO["lam"])
    return env, st, policy


def recurrent_rollout(config: str, n: int, T: int, rnn_type: str, hidden: int):
    """A rollout of an ActorCriticRecurrent policy through act_recurrent, and rsl_rl's per-step saved hidden states next to it."""
    from genesis_forge_amd.learner import ActorCriticRecurrent, RecurrentForward, RolloutStorage
    from genesis_forge_amd.tasks import BASELINE_CONFIGS

    env = BASELINE_CONFIGS[config][1](n)
    env.build()
    env.seed(1)
    obs, extras = env.reset()
    st = RolloutStorage(env, T).attach()
    st.begin(obs, extras)
    st.seed(2)
    torch.manual_seed(0)
    policy = ActorCriticRecurrent(st.obs_width, env.action_space.shape[0], rnn_type=rnn_type, rnn_hidden_dim=hidden).cuda()
    fwd = RecurrentForward(policy)
    saved, prev = {"actor": [], "critic": []}, None
    for t in range(T):
        for name in saved:
            parts = [x.clone() for x in fwd.state(name, n, "cuda") if x is not None]
            if prev is not None:
                for x in parts:
                    x[:, prev] = 0.0
            saved[name].append(parts)
        actions = st.act_recurrent(fwd, obs)
        obs, _r, _te, tr, extras = env.step(actions)
        st.process_env_step(tr)
        prev = st.dones[t].clone()
        fwd.reset(st.dones[t])
    st.compute_returns(fwd.value(obs), gamma=ALGO["gamma"], lam=ALGO["lam"])
    stack = lambda steps: tuple(torch.stack([s[i] for s in steps]) for i in range(len(steps[0])))
    return env, st, policy, (stack(saved["actor"]), stack(saved["critic"]))


def synthetic(config: str, n: int, T: int, noise_std_type: str = "scalar", rnd: bool = False):
    """A storage of random rows with the shapes of ``config`` and no env behind it (the dispatch-count runs: every launch of the
    process then belongs to the set-up or to an update)."""
    from types import SimpleNamespace

    from genesis_forge_amd import _native as nat
    from genesis_forge_amd.learner import ActorCriticMLP, RolloutStorage

    obs_w, critic_w, A = (48, 0, 12) if config == "go2_cmd" else (52, 12, 12)   # (widths of the go2_cmd and gait configs' managers)
    mk = lambda name, w: SimpleNamespace(name=name, observation_space=SimpleNamespace(shape=(w,)), output="fresh", _history_len=1, _unrolled=False)
    mgrs = [mk("policy", obs_w)] + ([mk("critic", critic_w)] if critic_w else [])
    env = SimpleNamespace(num_envs=n, managers={"observation": mgrs}, backend=nat.get_backend())
    st = RolloutStorage(env, T, obs_groups=obs_groups("gait" if critic_w else "go2_cmd", rnd))
    st._ensure_policy_rows(A)
    g = torch.Generator(device="cuda").manual_seed(0)
    for t in [st.observations, *st.group_rows.values(), st.actions, st.values, st.advantages, st.returns, st.actions_log_prob, st.mu]:
        t.copy_(torch.randn(t.shape, device="cuda", generator=g))
    st.sigma.fill_(1.0)
    st._returns_ready = True
    torch.manual_seed(0)
    policy = make_policy(obs_w, A, noise_std_type).cuda()
    if critic_w:
        policy.critic = ActorCriticMLP(obs_w + critic_w, A).critic.cuda()
    return env, st, policy


# Go2's left/right mirror.  Joints are ordered FL, FR, RL, RR x (hip, thigh, calf): legs swap sides, the hip (abduction) changes sign.
# Under the reflection y -> -y a velocity / the gravity direction flips y, an angular velocity (a pseudo-vector) flips x and z, and
# the command (vx, vy, yaw rate) flips vy and the yaw rate.
GO2_JOINT_MIRROR = ([3, 4, 5, 0, 1, 2, 9, 10, 11, 6, 7, 8], [-1, 1, 1] * 4)
GO2_ITEM_MIRROR = {"velocity_cmd": ([0, 1, 2], [1, -1, -1]), "angle_velocity": ([0, 1, 2], [-1, 1, -1]), "linear_velocity": ([0, 1, 2], [1, -1, 1]),
                   "projected_gravity": ([0, 1, 2], [1, -1, 1]), "dof_position": GO2_JOINT_MIRROR, "dof_velocity": GO2_JOINT_MIRROR,
                   "actions": GO2_JOINT_MIRROR}


def go2_mirror(st):
    """The MirrorSymmetry of a storage's observation groups: the Go2 tables for the items a manager has (any other item maps onto
    itself); a storage without real managers (``--synthetic``) gets a column reversal of every width."""
    from genesis_forge_amd import MirrorSymmetry

    managers = {m.name: m for m in st.env.managers["observation"]}

    def tables(group):
        members = [managers[name] for name in st.obs_groups[group]]
        if not all(getattr(m, "_plan", None) for m in members):
            w = sum(st._widths[name] for name in st.obs_groups[group])
            return list(range(w - 1, -1, -1)), [1.0] * w
        have = {name for m in members for name, *_ in m._plan}
        items = {k: v for k, v in GO2_ITEM_MIRROR.items() if k in have and all(w == len(v[0]) for m in members for n, _c, _s, w in m._plan if n == k)}
        return MirrorSymmetry.item_tables(members, items)

    (op, os_), (cp, cs) = tables("policy"), tables("critic")
    return MirrorSymmetry(op, os_, *GO2_JOINT_MIRROR, critic_obs_perm=cp, critic_obs_sign=cs)


def recurrent_update(config: str, n: int, args, forms) -> list:
    """--policy recurrent: one size, the forms alternated per rep from the same initial weights."""
    import rsl_rl_recurrent as R
    from genesis_forge_amd.learner import PPO

    env, st, policy0, (saved_a, saved_c) = recurrent_rollout(config, n, args.steps, args.rnn_type, args.rnn_hidden_dim)
    init = copy.deepcopy(policy0.state_dict())
    obs = st.observation_rows()[:args.steps]
    A = env.action_space.shape[0]
    times, last = {f: [] for f in forms}, {}
    for rep in range(args.reps + 1):   # rep 0: warm-up
        for form in forms:
            if form == "fused":
                policy = copy.deepcopy(policy0)
                policy.load_state_dict(init)
                policy.reset()
                algo = PPO(policy, st, **ALGO)
                update = algo.update
            else:
                policy = R.RslRlActorCriticRecurrent(st.obs_width, A, (512, 256, 128), (512, 256, 128), rnn_type=args.rnn_type,
                                                     rnn_hidden_dim=args.rnn_hidden_dim).cuda()
                policy.load_state_dict(init)
                algo = R.RslRlRecurrentPPO(policy, st, **ALGO)
                update = lambda: algo.update(obs, obs, saved_a, saved_c)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            losses = update()
            torch.cuda.synchronize()
            if rep:
                times[form].append((time.perf_counter() - t0) * 1e3)
            last[form] = (losses, algo.learning_rate)
    rows = []
    for form in forms:
        row = dict(config=config, num_envs=n, steps=args.steps, form=form, reps=args.reps, policy="recurrent", rnn_type=args.rnn_type,
                   rnn_hidden_dim=args.rnn_hidden_dim, trajectories=int(st.dones[:-1].sum()) + n,
                   best_ms=round(min(times[form]), 3) if times[form] else None,
                   median_ms=round(statistics.median(times[form]), 3) if times[form] else None,
                   all_ms=[round(x, 3) for x in times[form]], losses=last[form][0], lr=last[form][1], device=torch.cuda.get_device_name(0))
        rows.append(row)
        print(json.dumps(row), flush=True)
    del env, st, policy0
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="go2_cmd:4096,go2_cmd:16384,go2_cmd:65536,gait:4096")
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--forms", default="rsl_rl,fused")
    ap.add_argument("--out", default=None)
    ap.add_argument("--synthetic", action="store_true", help="random storage rows, no env (dispatch counts under rocprofv3)")
    ap.add_argument("--noise-std-type", default="scalar", choices=["scalar", "log"], help="the policy's std parameter: std, or log_std")
    ap.add_argument("--symmetry", default="none", choices=["none", "augment", "mirror", "both"], help="rsl_rl's symmetry_cfg with the Go2 mirror")
    ap.add_argument("--rnd", action="store_true", help="rsl_rl's rnd_cfg: every minibatch also trains the RND predictor")
    ap.add_argument("--policy", default="mlp", choices=["mlp", "recurrent"], help="recurrent: ActorCriticRecurrent on trajectory minibatches")
    ap.add_argument("--rnn-type", default="lstm", choices=["lstm", "gru"])
    ap.add_argument("--rnn-hidden-dim", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_update.py measures on a ROCm GPU: none is visible")
    from genesis_forge_amd.learner import PPO
    from rsl_rl_ppo import RslRlPPO
    from rsl_rl_rnd import RslRlRND, RslRlRndPPO
    from rsl_rl_symmetry import RslRlSymmetryPPO

    forms = args.forms.split(",")
    lines = []
    for spec in args.sizes.split(","):
        config, n = spec.split(":")
        if args.policy == "recurrent":
            lines += recurrent_update(config, int(n), args, forms)
            continue
        env, st, policy0 = (synthetic if args.synthetic else rollout)(config, int(n), args.steps, args.noise_std_type, args.rnd)
        init = copy.deepcopy(policy0.state_dict())
        algo_cfg = dict(ALGO)
        if args.symmetry != "none":
            algo_cfg["symmetry_cfg"] = dict(use_data_augmentation=args.symmetry in ("augment", "both"), use_mirror_loss=args.symmetry in ("mirror", "both"),
                                            mirror_loss_coeff=0.5, data_augmentation_func=go2_mirror(st))
        times = {f: [] for f in forms}
        last = {}
        for rep in range(args.reps + 1):   # rep 0: warm-up
            for form in forms:
                policy = copy.deepcopy(policy0)
                policy.load_state_dict(init)
                if form == "fused":
                    algo = PPO(policy, st, **dict(algo_cfg, rnd_cfg=RND_CFG if args.rnd else None))
                elif args.rnd:
                    ref_rnd = RslRlRND(st.obs_width, **{k: v for k, v in RND_CFG.items() if k != "learning_rate"}).cuda()
                    algo = RslRlRndPPO(policy, st, ref_rnd, rnd_learning_rate=RND_CFG["learning_rate"], **algo_cfg)
                else:
                    algo = (RslRlSymmetryPPO if args.symmetry != "none" else RslRlPPO)(policy, st, **algo_cfg)
                gen = torch.Generator(device="cuda").manual_seed(rep)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                losses = algo.update(generator=gen)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if rep:
                    times[form].append(dt * 1e3)
                last[form] = (losses, algo.learning_rate)
        mb = st.num_steps * st.env.num_envs // ALGO["num_mini_batches"]
        for form in forms:
            row = dict(config=config, num_envs=int(n), steps=args.steps, minibatch=mb, form=form, reps=args.reps,
                       noise_std_type=args.noise_std_type, symmetry=args.symmetry, rnd=args.rnd,
                       best_ms=round(min(times[form]), 3) if times[form] else None,
                       median_ms=round(statistics.median(times[form]), 3) if times[form] else None,
                       losses=last[form][0], lr=last[form][1], device=torch.cuda.get_device_name(0))
            lines.append(row)
            print(json.dumps(row), flush=True)
        del env, st, policy0
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
