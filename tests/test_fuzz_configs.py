"""Randomised task configs: the HIP path against the CPU oracle on configs nobody wrote by hand.

Each seed draws a task config from the whole mdp catalogue — which reward / termination terms, with what weights and parameters,
which observation items in what order with what scales / noise / history, how many ContactManagers and ObservationManagers (a
third one takes the recorded step off the fused kernel and onto the phase chains), whether a user-level (Python)
reward term is present (the recorded step is then cut in two around the call) — and an env count around the 64-env tile size.  The same config then runs 48 steps on the GPU and on the oracle in Philox mode; masks and integer state must be
bit-exact, floats within 1e-5 (helpers.FLOAT_TOL), log keys identical.  A second leg replays the GPU run with the recorded step
disabled: recorded (fused or chained) and phase-by-phase execution must agree bit for bit.
"""
import os
import random

import numpy as np
import pytest
import torch

from helpers import FLOAT_TOL

# GF_FUZZ_SEEDS="first:last" runs another range (a soak run hunts with hundreds; the committed default is what CI affords)
# 123 / 140: found by such a run — the control wave's pre-reset quaternion was not loaded when only the stale-quaternion stash needed it
# (termination done by a launch of its own; the body-frame items in a manager that observes behind the fused launch)
# 57 / 132 (round 3): a late observation manager's launch in front of a manager that is part of the fused launch, in call order — the
# per-piece patch tables applied the fused manager's output rotation / stream id one piece too late
# 288 / 300 (round 5): a user RewardManager (288) / TerminationManager (300) class whose step() returns a NEW tensor — the recorded step
# reset from and returned the manager's buffers instead.  333: an opaque reward term's params replaced and put back (A -> B -> A) — the
# compiled table kept the closure over the old params
SEEDS = list(range(*map(int, os.environ["GF_FUZZ_SEEDS"].split(":")))) if os.environ.get("GF_FUZZ_SEEDS") else list(range(28)) + [57, 123, 132, 140, 288, 300, 333]
STEPS = 48


SCENE_CLS = [None]   # tests/test_genesis_like.py swaps in the double with Genesis' public surface only


def make_fuzz_env(seed: int):
    from genesis_forge_amd import ManagedEnvironment
    from genesis_forge_amd.managers import (ContactManager, EntityManager, ObservationManager, PositionActionManager, RewardManager,
                                            TerminationManager, VelocityCommandManager)
    from genesis_forge_amd.mdp import observations, reset, rewards, terminations
    from genesis_forge_amd.scene import SyntheticScene, morphs
    from envs import GO2_DEFAULT_POS, GO2_JOINTS

    rnd = random.Random(1000 + seed)
    rnd_out = random.Random(77000 + seed)   # output / history modes of the observation managers (a stream of its own: the configs of the
    #                                         seeds above are what they were before the modes were drawn)

    rnd_win = random.Random(58000 + seed)   # output="window" (round 4), again a stream of its own

    def out_mode(history):
        if not history or history < 2:
            return dict(output=rnd_out.choice(["fresh", "fresh", "static"]))
        mode = dict(output=rnd_out.choice(["fresh", "fresh", "static", "static", "ring"]), history=rnd_out.choice(["auto", "auto", "shift", "unroll"]))
        if rnd_win.random() < 0.25:
            mode = dict(output="window")
        return mode

    n = rnd.choice([1, 63, 64, 65, 130, 257, 1000])
    pick = lambda p: rnd.random() < p
    uni = lambda lo, hi: round(rnd.uniform(lo, hi), 3)

    class FuzzEnv(ManagedEnvironment):
        def __init__(self):
            super().__init__(num_envs=n, dt=1 / 50, max_episode_length_sec=uni(0.4, 0.7), max_episode_random_scaling=rnd.choice([0.0, 0.1, 0.2]))
            self.scene = (SCENE_CLS[0] or SyntheticScene)(dt=self.dt, substeps=2, ang_noise=uni(0.1, 0.3), seed=seed, max_collision_pairs=rnd.choice([8, 12, 30]),
                                                           contact_prob=uni(0.05, 0.3), contact_force=uni(10.0, 60.0))
            self.terrain = self.scene.add_entity(morphs.Plane())
            self.robot = self.scene.add_entity(morphs.URDF(file="urdf/go2/urdf/go2.urdf", pos=[0.0, 0.0, 0.4], quat=[1.0, 0.0, 0.0, 0.0]))
            self.seen_params = {}   # (the params an opaque term was last called with: _seen)

        def config(self):
            em = self.robot_manager = EntityManager(self, entity_attr="robot", on_reset={
                "position": {"fn": reset.position, "params": {"position": [0.0, 0.0, uni(0.3, 0.45)], "quat": [1.0, 0.0, 0.0, 0.0],
                                                              "zero_velocity": pick(0.7)}}})
            # user-defined ACTION manager classes (handle_actions() — the reference's extension point — or step() overridden), user
            # ObservationManager classes and env-level get_observations() overrides: python phases of a recorded step (round 4).  A
            # random stream of their own: the other draws of a seed are what they were before these existed.
            rnd_usr = random.Random(55000 + seed)
            self.user_action_cls = rnd_usr.choice([None] * 17 + ["handle_actions", "handle_actions", "step"])
            self.user_obs_cls = rnd_usr.random() < 0.12
            gain = rnd_usr.choice([0.5, 0.8])

            class SmoothedActions(PositionActionManager):
                def handle_actions(s, actions):
                    prev = getattr(s, "_lp", None)
                    s._lp = actions.clone() if prev is None else gain * prev + (1.0 - gain) * actions
                    return super().handle_actions(s._lp)

            class ScaledActions(PositionActionManager):
                def step(s, actions):
                    return super().step(actions * gain)

            class ClippedObs(ObservationManager):
                def get_observations(s):
                    return super().get_observations().clamp(-2.0, 2.0)

            action_cls = {None: PositionActionManager, "handle_actions": SmoothedActions, "step": ScaledActions}[self.user_action_cls]
            am = self.action_manager = action_cls(
                self, joint_names=GO2_JOINTS, default_pos=GO2_DEFAULT_POS, scale=rnd.choice([0.25, 0.5, 1.0]),
                clip=rnd.choice([None, (-100.0, 100.0), (-1.5, 1.5)]), use_default_offset=pick(0.8), pd_kp=20, pd_kv=0.5)
            vc = self.velocity_command = VelocityCommandManager(
                self, range={"lin_vel_x": [-1.0, uni(0.2, 1.5)], "lin_vel_y": rnd.choice([[0, 0], [-0.5, 0.5]]), "ang_vel_z": [-uni(0.2, 1.0), 1.0]},
                standing_probability=0.0, resample_time_sec=uni(0.15, 0.5))
            # a user-defined manager CLASS (its own step() / reset(), the base class' resample launched from user code, torch state of its
            # own) — replayed between the native phases of a recorded step (round 3).  A random stream of its own: the other draws of a
            # seed are what they were before this existed.
            rnd_mgr = random.Random(99000 + seed)
            self.user_manager = rnd_mgr.random() < 0.3
            if self.user_manager:
                from genesis_forge_amd import gs
                from genesis_forge_amd.managers import CommandManager

                class Clock(CommandManager):
                    def __init__(s, env):
                        super().__init__(env, range=(0.5, round(rnd_mgr.uniform(1.0, 2.0), 3)), resample_time_sec=round(rnd_mgr.uniform(0.1, 0.4), 3))
                        s.phase = torch.zeros(env.num_envs, device=gs.device)

                    def step(s):
                        super().step()
                        s.phase = (s.phase + s.env.dt * s._command[:, 0]) % 1.0

                    def reset(s, env_ids=None):
                        super().reset(env_ids)
                        if env_ids is None:
                            s.phase = torch.zeros_like(s.phase)
                        else:
                            s.phase[env_ids] = 0.0

                self.clock = Clock(self)
            feet = body = None
            if pick(0.7):
                feet = self.foot_contacts = ContactManager(self, link_names=[".*_foot"], track_air_time=True, air_time_contact_threshold=uni(1.0, 8.0))
            if pick(0.6):
                body = self.body_contacts = ContactManager(self, link_names=rnd.choice([["base"], [".*_thigh", "base"], [".*_calf"]]))

            catalogue = {
                "base_height": lambda: {"fn": rewards.base_height, "params": {"target_height": uni(0.25, 0.4), "entity_attr": "robot"}},
                "track_lin": lambda: {"fn": rewards.command_tracking_lin_vel, "params": {"vel_cmd_manager": vc, "entity_manager": em, "sensitivity": uni(0.1, 0.5)}},
                "track_ang": lambda: {"fn": rewards.command_tracking_ang_vel, "params": {"vel_cmd_manager": vc, "entity_manager": em}},
                "lin_vel_z": lambda: {"fn": rewards.lin_vel_z_l2, "params": {"entity_manager": em}},
                "ang_vel_xy": lambda: {"fn": rewards.ang_vel_xy_l2, "params": {"entity_manager": em}},
                "flat": lambda: {"fn": rewards.flat_orientation_l2, "params": {"entity_manager": em}},
                "action_rate": lambda: {"fn": rewards.action_rate_l2},
                "similar": lambda: {"fn": rewards.dof_similar_to_default, "params": {"action_manager": am}},
                "stand_still": lambda: {"fn": rewards.stand_still_joint_deviation_l1, "params": {"vel_cmd_manager": vc, "action_manager": am,
                                                                                                 "command_threshold": uni(0.05, 0.6)}},
                "alive": lambda: {"fn": rewards.is_alive},
                "terminated": lambda: {"fn": rewards.terminated},
                "body_accel": lambda: {"fn": rewards.body_acceleration_exp, "params": {"entity_manager": em}},
            }
            if feet is not None:
                catalogue["air_time"] = lambda: {"fn": rewards.feet_air_time, "params": {
                    "contact_manager": feet, "time_threshold": uni(0.02, 0.2), "vel_cmd_manager": vc if pick(0.5) else None,
                    "time_threshold_max": uni(0.2, 0.5) if pick(0.4) else None}}
                catalogue["feet_slide"] = lambda: {"fn": rewards.feet_slide, "params": {"contact_manager": feet}}
            if body is not None:
                catalogue["undesired"] = lambda: {"fn": rewards.has_contact, "params": {"contact_manager": body, "threshold": uni(1.0, 20.0)}}
                catalogue["body_force"] = lambda: {"fn": rewards.contact_force, "params": {"contact_manager": body, "threshold": uni(1.0, 20.0)}}
            names = rnd.sample(sorted(catalogue), rnd.randint(1, min(10, len(catalogue))))
            rcfg = {}
            for name in names:
                item = catalogue[name]()
                item["params"] = {k: v for k, v in item.get("params", {}).items() if v is not None}
                item["weight"] = 0.0 if pick(0.08) else rnd.choice([-1, 1]) * uni(0.01, 3.0)
                rcfg[name] = item
            self.has_user_term = pick(0.3)
            self.has_user_obs = False   # a Python-level OBSERVATION item (sees the post-reset state: nothing behind it can be fused)
            if self.has_user_term:  # a user-level Python term: evaluated in torch on both sides, in the middle of the recorded step
                # (`scale`: what a params replacement edits, _replacements; 1.0 leaves every bit of the term as it was)
                rcfg["user_height"] = {"weight": 0.3, "fn": lambda env, scale=1.0: _seen(env, "user_height", scale, torch.tanh(env.robot.get_pos()[:, 2]) * scale)}
            if self.user_manager:
                rcfg["in_phase"] = {"weight": 0.2, "fn": lambda env: torch.cos(6.2831853 * self.clock.phase)}
            # user-defined RewardManager / TerminationManager CLASSES (their own step() around the library's, torch on the manager's
            # buffers): python phases of a recorded step (round 4).  A random stream of their own, as for the user command manager.
            rnd_cls = random.Random(77000 + seed)
            self.user_reward_cls, self.user_term_cls = rnd_cls.random() < 0.2, rnd_cls.random() < 0.2
            floor, grace = -round(rnd_cls.uniform(0.05, 0.5), 3), rnd_cls.choice([1, 2, 4])
            # round 5: their OUT-OF-PLACE variant — step() returns new tensors, which the env resets from, stores and returns while the
            # managers' buffers keep what super().step() left.  A stream of its own, chosen so that no seed committed before it draws it
            # (0-27, 57, 123, 132, 140 build what they built; of the seeds below 141, 29 52 66 76 77 80 81 87 88 102 130 would).
            oop = (self.user_reward_cls or self.user_term_cls) and random.Random(690000 + seed).random() < 0.25
            self.out_of_place = oop

            class CappedRewards(RewardManager):
                def step(s):
                    r = super().step()
                    if oop:
                        return torch.clamp(r, min=floor) * 2
                    r.clamp_(min=floor)
                    return r

            class GracefulTerminations(TerminationManager):
                def step(s):
                    te, tr = super().step()
                    if oop:   # (… and a few terminations of its own, so that the returned mask surely differs from the manager's)
                        return (te & (s.env.episode_length > grace)) | (s.env.episode_length % 29 == 11), tr
                    te &= s.env.episode_length > grace
                    return te, tr

            # reset(ids) overrides of the action / reward / termination manager (round 4: such a manager is reset by index list behind the
            # masked reset, also in a recorded step).  Again a stream of its own.
            rnd_rst = random.Random(59000 + seed)
            self.user_reset_cls = [k for k in ("action", "reward", "termination") if rnd_rst.random() < 0.07]

            def with_reset(base, on):
                if not on:
                    return base

                class WithReset(base):
                    def reset(s, envs_idx=None):
                        return super().reset(envs_idx)

                return WithReset

            if "action" in self.user_reset_cls:
                am.__class__ = with_reset(type(am), True)   # (the manager is built already: the draws above stay what they were)
            self.reward_manager = with_reset(CappedRewards if self.user_reward_cls else RewardManager, "reward" in self.user_reset_cls)(
                self, logging_enabled=pick(0.85), cfg=rcfg)

            tcfg = {"timeout": {"fn": terminations.timeout, "time_out": True}}
            if pick(0.8):
                tcfg["fall_over"] = {"fn": terminations.bad_orientation, "params": {"limit_angle": rnd.choice([10.0, 20.0, 30.0, 40.0]), "entity_manager": em,
                                                                                    "grace_steps": rnd.choice([0, 0, 5])}}
            if pick(0.3):
                tcfg["too_low"] = {"fn": terminations.base_height_below_minimum, "params": {"minimum_height": uni(0.05, 0.3), "entity_manager": em}}
            if body is not None and pick(0.6):
                kind = rnd.choice(["force", "has", "grace"])
                if kind == "force":
                    tcfg["body_contact"] = {"fn": terminations.contact_force, "params": {"contact_manager": body, "threshold": uni(20.0, 50.0)}}
                elif kind == "has":
                    tcfg["body_contact"] = {"fn": terminations.has_contact, "params": {"contact_manager": body, "threshold": uni(20.0, 50.0),
                                                                                       "min_contacts": rnd.choice([1, 2])}}
                else:
                    tcfg["body_contact"] = {"fn": terminations.contact_force_with_grace_period,
                                            "params": {"contact_manager": body, "threshold": uni(20.0, 50.0), "grace_steps": rnd.choice([3, 10])}}
            if pick(0.15):  # a user-level termination term (evaluated in front of the termination op)
                self.has_user_term = True
                tcfg["user_far"] = {"fn": lambda env, reach=0.35: _seen(env, "user_far", reach, env.robot.get_pos()[:, :2].abs().sum(dim=1) > reach)}
            self.termination_manager = with_reset(GracefulTerminations if self.user_term_cls else TerminationManager, "termination" in self.user_reset_cls)(
                self, logging_enabled=True, term_cfg=tcfg)

            items = {
                "velocity_cmd": lambda: {"fn": vc.observation},
                "angle_velocity": lambda: {"fn": lambda env: em.get_angular_velocity()},
                "linear_velocity": lambda: {"fn": lambda env: em.get_linear_velocity()},
                "projected_gravity": lambda: {"fn": lambda env: em.get_projected_gravity()},
                "dof_position": lambda: {"fn": lambda env: am.get_dofs_position()},
                "dof_velocity": lambda: {"fn": lambda env: am.get_dofs_velocity()},
                "actions": lambda: {"fn": lambda env: am.get_actions()},
                "dof_force": lambda: {"fn": observations.entity_dofs_force, "params": {"action_manager": am}},
            }
            if feet is not None:
                items["foot_force"] = lambda: {"fn": observations.contact_force, "params": {"contact_manager": feet}}

            def obs_cfg(k_min):
                chosen = rnd.sample(sorted(items), rnd.randint(k_min, len(items)))
                cfg = {}
                if pick(0.15):  # a user-level observation item (evaluated in front of this manager's op)
                    self.has_user_term = True
                    self.has_user_obs = True
                    cfg["user_xy"] = {"fn": lambda env: env.robot.get_pos()[:, :2] * 2.0}
                for name in chosen:
                    it = items[name]()
                    if pick(0.4):
                        it["scale"] = rnd.choice([0.05, 0.1, 0.25, 2.0])
                    if pick(0.25):
                        it["noise"] = rnd.choice([0.01, 0.05])
                    cfg[name] = it
                return cfg

            h = rnd.choice([None, None, 2, 3, 5])
            self.observation_manager = (ClippedObs if self.user_obs_cls else ObservationManager)(
                self, name="policy", cfg=obs_cfg(2), history_len=h, noise=0.02 if pick(0.15) else None, **out_mode(h))
            self.third_obs = False
            if pick(0.35):
                h = rnd.choice([None, 4])
                ObservationManager(self, name="critic", cfg=obs_cfg(1), history_len=h, **out_mode(h))
                self.third_obs = pick(0.4)
                if self.third_obs:  # more observation managers than the fused kernel takes: the third observes behind the fused launch
                    h = rnd.choice([None, 2])
                    ObservationManager(self, name="extra", cfg=obs_cfg(1), history_len=h, **out_mode(h))

    if random.Random(56000 + seed).random() < 0.1:   # an env-level get_observations() override (normalisation, clipping)
        def get_observations(self):
            o = ManagedEnvironment.get_observations(self)
            return None if o is None else o * 0.5
        FuzzEnv.get_observations = get_observations
    FuzzEnv.overrides_reset = pick(0.2)
    if FuzzEnv.overrides_reset:  # a user reset(): honoured by index list; the step is recorded up to the reset only
        FuzzEnv.reset = lambda self, envs_idx=None: ManagedEnvironment.reset(self, envs_idx)
    return FuzzEnv()


def _mutations(env, seed):
    """Live edits of a running env's config (a curriculum: config_item.py:31-44, command ranges edited in place), drawn per seed from a
    stream of their own: [(step, callable)].  Every edit must reach the very next step — recorded or not — and drop / refresh what a
    recorded step froze; about half of the seeds get one to three."""
    r = random.Random(57000 + seed)
    if r.random() < 0.5:
        return []
    out = []
    for _ in range(r.randint(1, 3)):
        at = r.randint(3, 24)
        kind = r.choice(["reward_weight", "reward_weight", "reward_param", "term_param", "range", "resample", "obs_scale", "obs_noise", "mgr_noise", "zero_weight"])
        rm, tm, vc = env.reward_manager, env.termination_manager, env.velocity_command
        if kind in ("reward_weight", "zero_weight"):
            name = r.choice(sorted(rm.cfg))
            w = 0.0 if kind == "zero_weight" else round(r.uniform(-2.0, 2.0), 3)
            out.append((at, lambda name=name, w=w: setattr(rm.cfg[name], "weight", w)))
        elif kind == "reward_param":
            cands = [(n, k) for n in sorted(rm.cfg) for k, v in rm.cfg[n].params.items() if isinstance(v, float)]
            if cands:
                n, k = r.choice(cands)
                f = round(r.uniform(0.7, 1.3), 3)
                out.append((at, lambda n=n, k=k, f=f: rm.cfg[n].params.__setitem__(k, rm.cfg[n].params[k] * f)))
        elif kind == "term_param":
            cands = [(n, k) for n in sorted(tm.term_cfg) for k, v in tm.term_cfg[n].params.items() if isinstance(v, float)]
            if cands:
                n, k = r.choice(cands)
                f = round(r.uniform(0.7, 1.3), 3)
                out.append((at, lambda n=n, k=k, f=f: tm.term_cfg[n].params.__setitem__(k, tm.term_cfg[n].params[k] * f)))
        elif kind == "range":
            hi = round(r.uniform(0.3, 2.5), 3)
            out.append((at, lambda hi=hi: vc.range["lin_vel_x"].__setitem__(1, hi)))   # in place: no setter involved
        elif kind == "resample":
            sec = round(r.uniform(0.1, 0.6), 3)
            out.append((at, lambda sec=sec: setattr(vc, "resample_time_sec", sec)))
        elif kind == "mgr_noise":
            nz = r.choice([None, 0.02, 0.04])
            out.append((at, lambda nz=nz: setattr(env.observation_manager, "noise", nz)))
        elif kind == "obs_noise":
            om = env.observation_manager
            name = r.choice(sorted(k for k in om.cfg if k != "user_xy"))
            nz = r.choice([None, 0.01, 0.05])
            out.append((at, lambda name=name, nz=nz: setattr(om.cfg[name], "noise", nz)))
        else:
            om = env.observation_manager
            cands = sorted(k for k in om.cfg if k != "user_xy")
            name = r.choice(cands)
            sc = r.choice([0.1, 0.5, 2.0])
            out.append((at, lambda name=name, sc=sc: setattr(om.cfg[name], "scale", sc)))
    return out


def _seen(env, name, value, out):
    """An opaque term's record of the param it was last called with (checked against its cfg after every step, _run)."""
    env.seen_params[name] = value
    return out


def _replacements(env, seed):
    """Round 5: a term's params REPLACED (``cfg[name].params = {...}``, a curriculum's other idiom), from a stream of its own chosen so
    that no seed committed before it draws it (of the seeds below 141, 31 34 53 55 72 82 87 92 94 130 would): [(step, callable)].  An
    opaque term is the target where there is one — its closure holds the params — and half of the draws put the old params back later
    (A -> B -> A)."""
    r = random.Random(660000 + seed)
    if r.random() >= 0.08:
        return []
    rm, tm = env.reward_manager.cfg, env.termination_manager.term_cfg
    opaque = [(c, n, k) for c, n, k in ((rm, "user_height", "scale"), (tm, "user_far", "reach")) if n in c]
    cands = opaque or [(c, n, k) for c in (rm, tm) for n in sorted(c) for k, v in c[n].params.items() if isinstance(v, float)]
    if not cands:
        return []
    cfg, name, key = r.choice(cands)
    old = dict(cfg[name].params)
    f = round(r.uniform(0.5, 1.5), 3)
    new = dict(old, **{key: f * old.get(key, 1.0 if key == "scale" else 0.35)})
    at = r.randint(3, 24)
    out = [(at, lambda: setattr(cfg[name], "params", dict(new)))]
    if r.random() < 0.5:
        out.append((at + r.randint(2, 10), lambda: setattr(cfg[name], "params", dict(old))))
    return out


def _run(seed, dev, steps=STEPS):
    env = make_fuzz_env(seed)
    env.build()
    env.seed(seed)
    obs, _ = env.reset()
    n = env.num_envs
    g = torch.Generator().manual_seed(seed)
    f = lambda t: t.detach().cpu().clone()
    out = [({"obs": f(obs)}, {})]
    edits = _mutations(env, seed) + _replacements(env, seed)
    for t in range(steps):
        for at, edit in edits:
            if at == t:
                edit()
        act = torch.randn(n, 12, generator=g)
        obs, rew, term, trunc, extras = env.step(act.to(dev))
        for name, cfg, key, dflt in (("user_height", env.reward_manager.cfg, "scale", 1.0), ("user_far", env.termination_manager.term_cfg, "reach", 0.35)):
            if name in cfg and getattr(cfg[name], "weight", 1.0) != 0:
                assert env.seen_params[name] == cfg[name].params.get(key, dflt), f"step {t}: '{name}' called with stale params"
        state = {"obs": obs, "reward": rew, "terminated": term, "truncated": trunc, "command": env.velocity_command.command,
                 "episode_length": env.episode_length, "max_episode_length": env.max_episode_length,
                 "episode_sums": env.reward_manager._episode_sums, "episode_seconds": env.reward_manager._episode_seconds,
                 "pos": env.robot.get_pos(), "quat": env.robot.get_quat(),
                 # a manager getter BETWEEN steps: just-reset envs are still rotated by their pre-reset orientation (quirk q-stale)
                 "gravity_between_steps": env.robot_manager.get_projected_gravity()}
        for name, o in extras["observations"].items():
            if name != "policy":
                state["obs_" + name] = o
        if env.user_manager:
            state["clock_phase"], state["clock_command"] = env.clock.phase, env.clock.command
        for cm in env.managers["contact"]:
            state[f"contacts_{len([k for k in state if k.startswith('contacts_')])}"] = cm.contacts
        out.append(({k: f(v) for k, v in state.items()}, {k: float(v) for k, v in extras["episode"].items()}))
    info = {"n": n, "recorded": env._trace is not None, "fused": bool(env._trace is not None and env._trace.post_refs is not None),
            "program": env._program_info, "post_refs": env._trace.post_refs if env._trace is not None else None, "env": env,
            "user_term": env.has_user_term, "user_obs": env.has_user_obs, "third_obs": env.third_obs, "overrides_reset": env.overrides_reset,
            "user_manager": env.user_manager or env.user_reward_cls or env.user_term_cls,
            # (a manager with its own reset(ids): user code behind the masked reset — between two phases of the fused launch unless every
            #  observation behind it is user code too, so either shape is right)
            "user_reset": bool(env.user_reset_cls)}
    return out, info


EXACT = ("terminated", "truncated", "episode_length", "max_episode_length")


def _compare(a, b, tol, what):
    resets = 0
    for t, ((sa, la), (sb, lb)) in enumerate(zip(a, b)):
        assert set(sa) == set(sb)
        for k in sa:
            if k in EXACT or tol == 0:
                assert torch.equal(sa[k], sb[k]) or (tol == 0 and torch.allclose(sa[k].float(), sb[k].float(), atol=0, rtol=0, equal_nan=True)), \
                    f"{what}: {k} differs at step {t}"
            else:
                assert torch.allclose(sa[k], sb[k], atol=tol, rtol=0, equal_nan=True), f"{what}: {k} differs at step {t}: {(sa[k] - sb[k]).abs().max()}"
        assert set(la) == set(lb), f"{what}: log keys differ at step {t}: {sorted(set(la) ^ set(lb))}"
        for key in la:
            assert (np.isnan(la[key]) and np.isnan(lb[key])) or abs(la[key] - lb[key]) <= tol + 1e-5 * abs(lb[key]), (what, t, key, la[key], lb[key])
        if "terminated" in sa:
            resets += int(sa["terminated"].sum() + sa["truncated"].sum())
    return resets


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_random_config_hip_equals_oracle(hip_backend, oracle_lib_path, seed):
    from genesis_forge_amd import _native as nat
    from genesis_forge_amd import gs
    from oracle_backend import OracleBackend

    hip, info = _run(seed, "cuda")
    torch.cuda.synchronize()
    gs.set_device("cpu")
    nat.set_backend(OracleBackend(oracle_lib_path))
    try:
        ref, _ = _run(seed, "cpu")
    finally:
        nat.set_backend(None)
        gs.set_device("cuda:0")
    resets = _compare(hip, ref, FLOAT_TOL, f"seed {seed} {info}")
    if info["n"] >= 63:
        assert resets > 0, "the config never reset an env: the reset path went untested"
    # every config is recorded; a user-level Python term or a third ObservationManager keeps it off the fused kernel
    assert info["recorded"], info
    if os.environ.get("GF_NO_FUSE", "0") != "1":  # (the whole suite is also run with every config forced onto the phase chains)
        # Python-level reward / termination terms leave everything behind the termination phase fused (termination runs as a launch of
        # its own, GF_POST_TERMINATION_DONE); a manager with a Python-level observation item, or a third ObservationManager, observes
        # behind the fused launch; only a reset() override keeps the post-physics phases off it (the user's code runs in the middle)
        # … and a user-defined manager class, whose step() sits between reward and reset (the phases on either side run as chains)
        brief = {k: v for k, v in info.items() if k not in ("env", "post_refs")}
        if info["overrides_reset"]:
            # … with a reset() override the recording ends in front of the reset: what is fused there is termination … command step as a
            # launch that resets nothing (GF_POST_NO_RESET; Python-level terms or a user manager class keep the chains)
            assert not info["fused"] or (info["post_refs"].flags & nat.GF_POST_NO_RESET and info["post_refs"].num_observe == 0), brief
        elif not info["user_reset"]:
            assert info["fused"] == (not info["user_manager"]), brief


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS[::2])
def test_random_config_recorded_equals_phase_by_phase(hip_backend, seed):
    fast, info = _run(seed, "cuda")
    os.environ["GF_NO_TRACE"] = "1"
    try:
        slow, info2 = _run(seed, "cuda")
    finally:
        del os.environ["GF_NO_TRACE"]
    assert info["recorded"] and not info2["recorded"]
    _compare(fast, slow, 0, f"seed {seed} {info}")


@pytest.mark.parametrize("seed", [s for s in SEEDS if s % 3 == 0])
def test_random_config_recorded_equals_phase_by_phase_cpu(oracle_backend, seed):
    """The same on the CPU oracle's gfo_run_ops: the recorded step (cut around Python-level terms where there are any)
    against the phase-by-phase step."""
    fast, info = _run(seed, "cpu", steps=30)
    os.environ["GF_NO_TRACE"] = "1"
    try:
        slow, info2 = _run(seed, "cpu", steps=30)
    finally:
        del os.environ["GF_NO_TRACE"]
    assert info["recorded"] and not info2["recorded"]
    _compare(fast, slow, 0, f"seed {seed} {info}")
    if not info["overrides_reset"] and not info["user_reset"] and os.environ.get("GF_NO_FUSE", "0") != "1":
        # (the structure check of the GPU test, here without a GPU: only user code BETWEEN post-physics phases keeps them off one launch)
        assert info["fused"] == (not info["user_manager"]), {k: v for k, v in info.items() if k not in ("env", "post_refs")}


def test_fuzz_configs_build_on_cpu(oracle_backend):
    """CPU leg: every fuzz config builds and steps on the oracle backend (host logic of rarely combined options)."""
    for seed in SEEDS:
        out, info = _run(seed, "cpu", steps=6)
        assert len(out) == 7 and out[-1][0]["obs"].shape[0] == info["n"]
        assert torch.isfinite(out[-1][0]["reward"]).all()
