"""Configs at the fused post-physics launch's table limits and one entry past them (tests/test_post_capacity.py).

``pack()`` (csrc/gf_post.hip) admits a recorded step to the one-launch kernel only inside tables smaller than the phase kernels':
8 termination terms, 16 reward terms (rows < 24), 12 items per observation manager, a 255-wide frame, 2 observation managers,
2 stepped command managers of up to 4 ranges, 4 command buffers and 4 ContactManagers over all phases, 1 … 32 DOF.  A ``Spec`` names
one point of that space; ``make_env`` builds it on the synthetic scene from catalogues that repeat an op with other parameters where
the ops run out.  ``AT`` holds the config at every limit, ``PAST`` the one an entry past it with what happens there.

Run as a script (``python post_capacity_cases.py why``) it prints, for every refused config, the rules GF_POST_WHY names — the
variable is read once per process, so the test starts this file as a child.
"""
import ctypes as C
import os
import sys
from dataclasses import dataclass, replace
from typing import Optional

import torch

D3 = ("cmd0", "ang", "grav", "lin")                                               # the 3-wide items
DW = ("dof_pos", "dof_vel", "actions", "dof_force", "raw", "dof_pos*", "dof_vel*", "actions*")   # the DOF-wide ones (*: rescaled repeat)
GO2_POLICY = ("cmd0", "ang", "grav", "dof_pos", "dof_vel", "actions")
GO2_CRITIC = ("lin", "norm:feet", "dof_force", "raw")
# thirteen items; the twelfth (the last of an at-limit manager) is a rescaled projected gravity: never zero
ITEMS13 = ("cmd0", "ang", "grav", "lin", "dof_pos", "dof_vel", "actions", "dof_force", "raw", "norm:feet", "dof_vel*", "grav*", "ang*")


NORM255 = ("norm:wide32", "norm:wide32*") * 3 + ("norm:wide32", "norm:wide31")   # 7·32 + 31 columns in eight items


def wide_items(dofs: int, width: int) -> tuple:
    """Twelve items whose widths add up to ``width``: DOF-wide and 3-wide items and contact-force norms over
    ``wide<k>`` ContactManagers of k links — the last item is a norm, so dropping it narrows the frame by its links."""
    if dofs == 32:      # 7·32 + 4·3 + 19
        head, rest = DW[:7] + D3, width - 7 * 32 - 12
    elif dofs == 28:    # 8·28 + 3·3 + 22
        head, rest = DW[:8] + D3[:3], width - 8 * 28 - 9
    elif dofs == 12:    # 6·12 + 5·32 + 23: the norm items share one 32-link manager
        head, rest = DW[:6] + ("norm:wide32", "norm:wide32*", "norm:wide32", "norm:wide32*", "norm:wide32"), width - 72 - 160
    else:
        raise ValueError(dofs)
    assert 1 <= rest <= 32
    return head + (f"norm:wide{rest}",)


@dataclass(frozen=True)
class Spec:
    dofs: int = 12
    n_term: int = 4
    n_rew: int = 8               # entries of the reward cfg …
    zero_every: int = 0          # … of which every third (k % 3 == 1) has weight 0 when set: it keeps its episode-sum row
    obs: tuple = (GO2_POLICY, GO2_CRITIC)   # item names per observation manager
    cmd_ranges: tuple = (3, 1)   # range counts of the stepped command managers (the first is the velocity command)
    idle_cmds: int = 0           # command buffers of the user's own (plain tensors) that reward terms read: views, not managers
    contacts: int = 2            # distinct ContactManagers the terms read: feet, torso, legs, arms, head
    history: int = 2
    logging: bool = True

    def but(self, **kw):
        return replace(self, **kw)


CONTACT_LINKS = (("feet", ["F[0-3]"]), ("torso", ["torso"]), ("legs", ["L0[0-3]"]), ("arms", ["L0[4-7]"]), ("head", ["L0[89]"]))


def make_env(spec: Spec, num_envs: int, drop: Optional[str] = None):
    """``drop``: "term" / "rew" / "item" builds the same env without the last termination term / reward entry / item of the first
    observation manager."""
    from genesis_forge_amd import ManagedEnvironment
    from genesis_forge_amd.managers import (CommandManager, ContactManager, EntityManager, ObservationManager, PositionActionManager,
                                            RewardManager, TerminationManager, VelocityCommandManager)
    from genesis_forge_amd.mdp import observations, reset, rewards, terminations
    from genesis_forge_amd.scene import RobotModel, SyntheticScene, morphs

    class CapacityEnv(ManagedEnvironment):
        def __init__(self):
            super().__init__(num_envs=num_envs, dt=1 / 50, max_episode_length_sec=0.4, max_episode_random_scaling=0.2)
            self.scene = SyntheticScene(dt=self.dt, substeps=2, max_collision_pairs=12, ang_noise=0.3, contact_prob=0.3, contact_force=40.0, seed=21)
            self.terrain = self.scene.add_entity(morphs.Plane())
            joints = [(f"J{k:02d}", -1.5, 1.5) for k in range(spec.dofs)]
            links = ["torso"] + [f"L{k:02d}" for k in range(32)] + [f"F{k}" for k in range(4)]
            self.robot = self.scene.add_entity(model=RobotModel("capacity", joints, links, init_pos=(0.0, 0.0, 0.55)))

        def config(self):
            em = self.robot_manager = EntityManager(self, entity_attr="robot", on_reset={
                "position": {"fn": reset.position, "params": {"position": [0.0, 0.0, 0.55], "quat": [1.0, 0.0, 0.0, 0.0]}}})
            am = self.action_manager = PositionActionManager(self, joint_names=".*", default_pos={".*": 0.1}, scale=0.5, pd_kp=20, pd_kv=0.5)
            self.commands = []
            for c, r in enumerate(spec.cmd_ranges):
                if c == 0:
                    rng = {"lin_vel_x": [-1.0, 1.0], "lin_vel_y": [-0.5, 0.5], "ang_vel_z": [-1.0, 1.0]}
                    rng.update({f"extra{j}": [0.1 * j, 0.5 + 0.1 * j] for j in range(r - 3)})
                    self.commands.append(VelocityCommandManager(self, range=rng, resample_time_sec=0.12))
                elif r == 1:
                    self.commands.append(CommandManager(self, range=(0.3 + 0.1 * c, 0.6 + 0.1 * c), resample_time_sec=0.1 + 0.04 * c))
                else:
                    self.commands.append(CommandManager(self, range={f"r{j}": [-1.0 - j, 0.5 * j + c] for j in range(r)}, resample_time_sec=0.1 + 0.04 * c))
            vc = self.velocity_command = self.commands[0]
            self.idle = []
            for k in range(spec.idle_cmds):   # not stepped, not reset: buffers user code fills (here: once, with a pattern per env)
                col = torch.arange(num_envs, device=vc._command.device, dtype=torch.float32).unsqueeze(1) * 0.003
                self.idle.append((0.4 + col, 0.2 - col, torch.cat([0.3 - col, col - 0.1], dim=1))[k].contiguous())
            self.contact = {}
            for name, pats in CONTACT_LINKS[:spec.contacts]:
                self.contact[name] = ContactManager(self, link_names=pats, **(dict(track_air_time=True, air_time_contact_threshold=1.0) if name == "feet" else {}))
            order = [m for _n, m in self.contact.items()]
            feet = order[0]
            cm = lambda k: order[min(k, len(order) - 1)]
            for names in spec.obs:
                for name in names:
                    key = name.rstrip("*")
                    if key.startswith("norm:wide") and key[5:] not in self.contact:
                        self.contact[key[5:]] = ContactManager(self, link_names=[f"L{k:02d}" for k in range(int(key[9:]))])

            # -- rewards: the first six read every kind of view, the sixteenth / seventeenth / twenty-fourth are dense (never zero)
            ent = {"entity_manager": em}
            cat = [
                ("lin", rewards.command_tracking_lin_vel, dict(vel_cmd_manager=vc, **ent)),
                ("ang", rewards.command_tracking_ang_vel, dict(vel_cmd_manager=vc, **ent)),
                ("air", rewards.feet_air_time, dict(contact_manager=feet, time_threshold=0.04, time_threshold_max=0.5, vel_cmd_manager=vc)),
                ("bad_contact", rewards.contact_force, dict(contact_manager=cm(2), threshold=2.0)),
                ("undesired", rewards.has_contact, dict(contact_manager=cm(1), threshold=5.0)),
                ("arm_force", rewards.contact_force, dict(contact_manager=cm(3), threshold=1.0)),
                ("rate", rewards.action_rate_l2, {}),
                ("pose", rewards.dof_similar_to_default, dict(action_manager=am)),
                ("still", rewards.stand_still_joint_deviation_l1, dict(vel_cmd_manager=vc, action_manager=am, command_threshold=0.3)),
                ("slide", rewards.feet_slide, dict(contact_manager=feet)),
                ("alive", rewards.is_alive, {}),
                ("flat", rewards.flat_orientation_l2, dict(ent)),
                ("height", rewards.base_height, dict(target_height=0.5)),
                ("accel", rewards.body_acceleration_exp, dict(ent)),
                ("lin_z", rewards.lin_vel_z_l2, dict(ent)),
                ("height16", rewards.base_height, dict(target_height=0.42)),
                ("lin17", rewards.command_tracking_lin_vel, dict(vel_cmd_manager=vc, sensitivity=0.4, **ent)),
                ("ang_xy", rewards.ang_vel_xy_l2, dict(ent)),
                ("terminated", rewards.terminated, {}),
                ("force20", rewards.contact_force, dict(contact_manager=cm(2), threshold=8.0)),
                ("height21", rewards.base_height, dict(target_height=0.3)),
                ("has22", rewards.has_contact, dict(contact_manager=cm(1), threshold=12.0)),
                ("ang23", rewards.command_tracking_ang_vel, dict(vel_cmd_manager=vc, sensitivity=0.5, **ent)),
                ("height24", rewards.base_height, dict(target_height=0.36)),
            ]
            idle_terms = [("height_to", rewards.base_height, lambda t: dict(target_height=t)),
                          ("ang_to", rewards.command_tracking_ang_vel, lambda t: dict(commanded_ang_vel=t, **ent)),
                          ("lin_to", rewards.command_tracking_lin_vel, lambda t: dict(command=t, **ent))]
            for k, t in enumerate(self.idle):   # (in the place of arm_force, rate, pose: inside the Go2-like eight)
                cat[5 + k] = (idle_terms[k][0], idle_terms[k][1], idle_terms[k][2](t))
            n_rew = spec.n_rew - (1 if drop == "rew" else 0)
            rcfg = {}
            for k, (name, fn, params) in enumerate(cat[:n_rew]):
                w = 0.0 if spec.zero_every and k % 3 == 1 else (-1) ** k * (0.05 + 0.03 * k)   # distinct, non-zero
                rcfg[name] = {"weight": w, "fn": fn, "params": params}
            self.reward_manager = RewardManager(self, logging_enabled=spec.logging, cfg=rcfg)

            # -- terminations: the eighth fires at a tilt of 5 degrees, a superset of the 9 and 12 degree terms in front of it (the base tilts up to ~12 degrees in an episode)
            tcat = [
                ("timeout", terminations.timeout, {}, True),
                ("low", terminations.base_height_below_minimum, dict(minimum_height=0.2, **ent), False),
                ("torso", terminations.contact_force, dict(contact_manager=cm(1), threshold=25.0), False),
                ("tilt12", terminations.bad_orientation, dict(limit_angle=12.0, grace_steps=3, **ent), False),
                ("legs", terminations.has_contact, dict(contact_manager=cm(2), threshold=30.0, min_contacts=2), False),
                ("feet", terminations.contact_force_with_grace_period, dict(contact_manager=feet, threshold=45.0, grace_steps=5), False),
                ("tilt9", terminations.bad_orientation, dict(limit_angle=9.0, **ent), False),
                ("tilt5", terminations.bad_orientation, dict(limit_angle=5.0, **ent), False),
                ("low9", terminations.base_height_below_minimum, dict(minimum_height=0.1, **ent), False),
            ]
            n_term = spec.n_term - (1 if drop == "term" else 0)
            self.termination_manager = TerminationManager(self, term_cfg={
                name: dict({"fn": fn, "params": params}, **({"time_out": True} if to else {})) for name, fn, params, to in tcat[:n_term]})

            # -- observations
            def item(name):
                key, alt = name.rstrip("*"), name.endswith("*")
                if key.startswith("cmd"):
                    it = {"fn": self.commands[int(key[3:])].observation}
                elif key.startswith("norm:"):
                    it = {"fn": observations.contact_force, "params": {"contact_manager": self.contact[key[5:]]}, "scale": 0.1}
                else:
                    it = {"ang": {"fn": lambda env: em.get_angular_velocity(), "scale": 0.25},
                          "grav": {"fn": lambda env: em.get_projected_gravity()},
                          "lin": {"fn": lambda env: em.get_linear_velocity()},
                          "dof_pos": {"fn": lambda env: am.get_dofs_position()},
                          "dof_vel": {"fn": lambda env: am.get_dofs_velocity(), "scale": 0.05},
                          "actions": {"fn": lambda env: am.get_actions()},
                          "dof_force": {"fn": observations.entity_dofs_force, "params": {"action_manager": am}},
                          "raw": {"fn": observations.current_actions}}[key]
                if alt:
                    it["scale"] = 2.0 * it.get("scale", 1.0)
                return it

            self.obs_managers = []
            for m, names in enumerate(spec.obs):
                names = names[:-1] if (drop == "item" and m == 0) else names
                cfg = {f"{k:02d}_{name}": item(name) for k, name in enumerate(names)}
                kw = dict(history_len=spec.history, noise=0.01) if m == 0 else {}
                om = ObservationManager(self, name=("policy", "critic", "extra")[m], cfg=cfg, **kw)
                self.obs_managers.append(om)
                if m == 0:
                    self.observation_manager = om

    return CapacityEnv()


def run(spec: Spec, dev: str, mode: str, n: int, steps: int = 40, drop: Optional[str] = None, jit: Optional[str] = None):
    """``mode``: "ordinary" (phase by phase), "unfused" (recorded, phase chains), "fused" (recorded, the one-launch kernel where pack()
    admits the step).  Returns [per step: {name: tensor | log dict}], the env."""
    env = make_env(spec, n, drop)
    env.trace_enabled = mode != "ordinary"
    env.fuse_post_physics = mode == "fused"
    if jit:
        env.jit_programs = jit
    env.build()
    env.seed(31)
    env.reset()
    g = torch.Generator().manual_seed(5)
    f = lambda t: t.detach().cpu().clone()
    seq = []
    for _ in range(steps):
        o, r, te, tr, ex = env.step(torch.randn(n, spec.dofs, generator=g).to(dev))
        st = {"obs": f(o), "reward": f(r), "terminated": f(te), "truncated": f(tr), "log": {k: float(v) for k, v in ex["episode"].items()},
              "episode_sums": f(env.reward_manager._episode_sums), "episode_length": f(env.episode_length),
              "max_episode_length": f(env.max_episode_length), "dof_pos": f(env.robot.dof_pos), "quat": f(env.robot.quat)}
        for name, t in ex["observations"].items():
            st["obs_" + name] = f(t)
        for c, m in enumerate(env.commands):
            st[f"command{c}"] = f(m._command)
        for c, t in enumerate(env.idle):
            st[f"idle{c}"] = f(t)
        seq.append(st)
    return seq, env


def same(a, b, what=""):
    """tests/test_trace.py:_same_h's rule over named outputs: tensors bit for bit, episode-log floats within 1e-6 relative."""
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys(), f"{what}: outputs differ at step {t}"
        for k in x:
            if k == "log":
                assert x[k].keys() == y[k].keys(), f"{what}: log keys differ at step {t}"
                for key in x[k]:
                    assert abs(x[k][key] - y[k][key]) <= 1e-6 + 1e-6 * abs(y[k][key]), (what, t, key, x[k][key], y[k][key])
            else:
                assert x[k].shape == y[k].shape and torch.equal(x[k], y[k]), f"{what}: {k} differs at step {t}"


def resets(seq) -> int:
    return sum(int(s["terminated"].sum() + s["truncated"].sum()) for s in seq)


# ---- the case table ---------------------------------------------------------------------------------------------------------------
GO2 = Spec()
ITEMS12 = ITEMS13[:12]
RULE = {   # the condition GF_POST_WHY prints for each limit (the text of the UNSUP() in pack())
    "term": "N <= 0 || T.num_terms > kPostMaxTerm || T.term_out",
    "rew": "RW->num_envs != N || RW->mode != GF_REWARD_MODE_STEP || RW->num_terms > kPostMaxReward || !RW->reward || !RW->episode_seconds",
    "items": "!ob || ob->num_envs != N || ob->num_items > kPostMaxItems || ob->noise_draws || !ob->obs",
    "width": "omax >= GF_MAX_OBS_WIDTH",
    "managers": "r->num_command < 0 || r->num_command > GF_POST_MAX_CMD || r->num_observe < 0 || r->num_observe > GF_POST_MAX_OBS",
    "ranges": "s->num_envs != N || s->num_ranges > kPostMaxRanges || s->draws || s->resample_steps <= 0 || s->episode_length != T.episode_length",
    "slot": "s < 0",
    "dofs": "(needs & (PN_DOFPOS | PN_DOFVEL | PN_TARGETS | PN_ACTIONS | PN_LAST)) && !dofs_ok",
}
# at the limit: the step must be ONE launch of the fused kernel
AT = {
    "term8": GO2.but(n_term=8, contacts=3),
    "rew16": GO2.but(n_rew=16, contacts=4),
    "rew16of24": GO2.but(n_rew=24, zero_every=3, contacts=4),   # rows 1, 4 … 22 uncovered, the last term's row is 23
    "items12": GO2.but(obs=(ITEMS12, GO2_CRITIC)),
    "items12x2": GO2.but(obs=(ITEMS12, ITEMS12)),
    "width255": GO2.but(dofs=32, obs=(wide_items(32, 255), GO2_CRITIC)),
    "width255_dof12": GO2.but(obs=(wide_items(12, 255), GO2_CRITIC)),
    "obs2": GO2,
    "cmd2": GO2.but(obs=(GO2_POLICY + ("cmd1",), GO2_CRITIC)),
    "ranges4": GO2.but(cmd_ranges=(4, 1)),
    "views4": GO2.but(idle_cmds=3),   # the velocity command and three buffers of the user's own, all read by reward terms
    "contacts4": GO2.but(contacts=3, obs=(GO2_POLICY, ("lin", "norm:wide5", "dof_force", "raw"))),
    # two managers of 255 contact-force-norm columns: the interpreter's LDS is that of any 255-wide frame, a program compiled for the
    # structure would park 510 norm rows on top — more than a workgroup has (select_program passes it over)
    "norms255x2": GO2.but(obs=(NORM255, NORM255)),
    "everything28": Spec(dofs=28, n_term=8, n_rew=24, zero_every=3, contacts=3, cmd_ranges=(3, 4),
                         obs=(wide_items(28, 255), ITEMS12[:11] + ("cmd1",))),
    "everything32": Spec(dofs=32, n_term=8, n_rew=24, zero_every=3, contacts=3, cmd_ranges=(3, 4),
                         obs=(wide_items(32, 255), ITEMS12[:11] + ("cmd1",))),
}
# one past it: the config, the rule that refuses it, and whether the whole step leaves the fused kernel ("chains") or only the
# surplus manager does ("late": a third observation manager observes behind a fused launch of the first two)
PAST = {
    "term9": (AT["term8"].but(n_term=9), "term", "chains"),
    "rew17": (AT["rew16"].but(n_rew=17), "rew", "chains"),
    "items13": (GO2.but(obs=(ITEMS13, GO2_CRITIC)), "items", "chains"),
    "items13x2": (GO2.but(obs=(ITEMS13, ITEMS13)), "items", "chains"),
    "obs3": (GO2.but(obs=(GO2_POLICY, GO2_CRITIC, ("grav", "dof_pos", "cmd0"))), None, "late"),
    "cmd3": (GO2.but(cmd_ranges=(3, 1, 1), obs=(GO2_POLICY + ("cmd1", "cmd2"), GO2_CRITIC)), None, "chains"),   # (refused by the recorder)
    "ranges5": (GO2.but(cmd_ranges=(5, 1)), "ranges", "chains"),
    "views5": (GO2.but(idle_cmds=3, obs=(GO2_POLICY + ("cmd1",), GO2_CRITIC)), "slot", "chains"),   # … and the second manager's, observed
    "contacts5": (GO2.but(contacts=4, obs=(GO2_POLICY, ("lin", "norm:wide5", "dof_force", "raw"))), "slot", "chains"),
    "dof33": (GO2.but(dofs=33), "dofs", "chains"),
}
# the table entry whose removal must change the outputs (the inputs of the at-limit cases are decisive)
DECISIVE = {"term8": "term", "rew16": "rew", "items12": "item", "width255": "item"}
WIDTH256 = GO2.but(dofs=32, obs=(wide_items(32, 256), GO2_CRITIC))   # the ObservationManager itself refuses it (ValueError at build)


class PackCheckedOracle:
    """Mixed into tests/oracle_backend.OracleBackend: the CPU oracle computes, the HIP library's host-only pack() decides what fuses
    (the oracle's own check admits everything) — the recorded steps then have the structure they have on the GPU."""

    def post_check(self, refs):
        return self.hip.post_check(refs)


def pack_checked_backend(oracle_lib_path):
    from genesis_forge_amd import _native as nat
    from oracle_backend import OracleBackend

    cls = type("PackCheckedOracleBackend", (PackCheckedOracle, OracleBackend), {})
    b = cls(oracle_lib_path)
    b.hip = nat.HipBackend()   # loads the library; nothing is launched
    return b


def raw_past_refs(env, which):
    """The rules no env reaches (the recorder and the ObservationManager stop the config first), on a copy of an at-limit env's
    descriptors: a third observation / command manager, a 256-wide frame.  Returns (refs, objects to keep alive)."""
    from genesis_forge_amd import _native as nat

    src = env._trace.post_refs
    refs = nat.GfPostRefs.from_buffer_copy(src)
    keep = [src]
    if which == "obs3":
        refs.num_observe = nat.GF_POST_MAX_OBS + 1
    elif which == "cmd3":
        refs.num_command = nat.GF_POST_MAX_CMD + 1
    elif which == "width256":
        ob = nat.GfObservationArgs.from_buffer_copy(C.cast(refs.observe[0], C.POINTER(nat.GfObservationArgs)).contents)
        ob.obs_width = nat.GF_MAX_OBS_WIDTH
        refs.observe[0] = C.addressof(ob)
        keep.append(ob)
    return refs, keep


RAW_RULE = {"obs3": "managers", "cmd3": "managers", "width256": "width"}


def _why_main():
    """Child of test_one_past_means_exactly_one_rule: GF_POST_WHY is set by the parent; every refusal goes to stderr behind a
    ``case <name>`` line."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (here, os.path.join(root, "genesis-forge_amd")):
        sys.path.insert(0, p)
    from genesis_forge_amd import _native as nat
    from genesis_forge_amd import gs

    gs.set_device("cpu")
    backend = pack_checked_backend(os.path.join(root, "oracle", "libgf_oracle.so"))
    nat.set_backend(backend)
    for name, (spec, _rule, _how) in PAST.items():
        print(f"case {name}", file=sys.stderr, flush=True)
        _seq, env = run(spec, "cpu", "fused", 8, steps=3)
        print(f"fused {name} {env._trace is not None and env._trace.post_refs is not None}", file=sys.stderr, flush=True)
    _seq, env = run(AT["width255"], "cpu", "fused", 8, steps=3)
    for which in RAW_RULE:
        print(f"case raw_{which}", file=sys.stderr, flush=True)
        refs, _keep = raw_past_refs(env, which)
        print(f"fused raw_{which} {backend.hip.post_check(refs)}", file=sys.stderr, flush=True)


if __name__ == "__main__" and sys.argv[1:] == ["why"]:
    _why_main()
