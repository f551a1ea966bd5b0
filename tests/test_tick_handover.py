"""The tile a folded step's tick leaves is handed to the post-physics phase of the same workgroup through LDS
(csrc/gf_post_ws.h, ``ws_hands_over``: static programs 1 and 2 and the 12-DOF table interpreter) instead of being read back from memory.  The tick's stores stay, and every role sees the bits
it saw after a read-back — so the folded step is compared with the two launches of ``GF_FOLD_STEP=0`` bit for bit, as
``tests/test_step_fold.py`` does, with the weight on what the hand-over could break:

* after EVERY step the ten arrays the tick writes as they stand in memory (pos, quat, lin_vel, ang_vel, dof_pos, dof_vel, targets,
  actions, last_actions, episode_length), and everything the step returned;
* n = 1, 63, 65, 130 (a lane-starved tile, lanes past the tile, a partial last tile) and one size of more than 24 tiles;
* both static programs, whose reward wave derives the body-frame vectors itself (the tracking terms: ``ws_rew_body_frame``) and takes
  quaternion and velocities from the handed rows;
* two 12-DOF configs whose packed ``needs`` word lacks handed rows (no dof_vel / targets rows; no reward-wave rows), asserted on the
  word ``gf_post_physics_needs`` reports for the recorded step.  A static program is matched to one exact structure, so its word
  always carries every handed bit; these configs run the 12-DOF interpreter's tick variant, which hands over too, and there a row
  whose bit is off is read from the zero row and a base field (a third config: no position, no linear velocity) is selected against zero;
* a 12-DOF config with two observation managers, on the same kernel (the tile the handed rows share is reused between managers
  behind a barrier).

Episodes are 0.24 s (12 steps ± 10 %), so inside the 14 compared steps every env is reset once and most steps of an env reset
nothing; ``gf_step_fold_count`` says that the fold took place."""
import os
import re

import pytest

from genesis_forge_amd import _native as nat

import test_step_fold as tsf

pytestmark = pytest.mark.gpu

STEPS = 14
EPISODE_S = 0.24
N_MANY_TILES = 64 * 25 + 37   # more tiles than the 24 upkeep workgroups in front of them

TICKED = ("pos", "quat", "lin_vel", "ang_vel", "dof_pos", "dof_vel", "targets", "actions", "last_actions", "episode_length")



def _needs_bits():
    """GF_POST_NEEDS_* as include/gf_step.h declares them (the library asserts that they are the kernel's bits)."""
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gf_step.h")
    with open(header) as f:
        bits = {name: int(value) for name, value in re.findall(r"GF_POST_NEEDS_([A-Z]+) = (\d+)", f.read())}
    assert len(bits) == 14, bits
    return bits


NEEDS = _needs_bits()


def _trimmed_env(n, drop_rewards=(), drop_obs=(), critic=False):
    """bench.py's Go2 config without some reward terms / observation items, or with a second observation manager."""
    from genesis_forge_amd import tasks
    from genesis_forge_amd.managers import (EntityManager, ObservationManager, PositionActionManager, RewardManager, TerminationManager,
                                            VelocityCommandManager)
    from genesis_forge_amd.mdp import reset, rewards, terminations

    class Trimmed(tasks.Go2CommandDirectionEnv):
        def config(self):
            self.robot_manager = EntityManager(self, entity_attr="robot", on_reset={
                "position": {"fn": reset.position, "params": {"position": tasks.INITIAL_BODY_POSITION, "quat": tasks.INITIAL_QUAT, "zero_velocity": True}}})
            self.action_manager = PositionActionManager(self, joint_names=tasks.GO2_JOINTS, default_pos=tasks.GO2_DEFAULT_POS, scale=0.25,
                                                        use_default_offset=True, pd_kp=20, pd_kv=0.5)
            self.velocity_command = VelocityCommandManager(
                self, range={"lin_vel_x": [-1.0, 1.0], "lin_vel_y": [-1.0, 1.0], "ang_vel_z": [-1.0, 1.0]}, standing_probability=0.02,
                resample_time_sec=0.1)
            rcfg = {
                "base_height_target": {"weight": -50.0, "fn": rewards.base_height, "params": {"target_height": 0.3, "entity_attr": "robot"}},
                "tracking_lin_vel": {"weight": 1.0, "fn": rewards.command_tracking_lin_vel,
                                     "params": {"vel_cmd_manager": self.velocity_command, "entity_manager": self.robot_manager}},
                "lin_vel_z": {"weight": -1.0, "fn": rewards.lin_vel_z_l2, "params": {"entity_manager": self.robot_manager}},
                "action_rate": {"weight": -0.005, "fn": rewards.action_rate_l2},
                "similar_to_default": {"weight": -0.1, "fn": rewards.dof_similar_to_default, "params": {"action_manager": self.action_manager}},
            }
            self.reward_manager = RewardManager(self, logging_enabled=True, cfg={k: v for k, v in rcfg.items() if k not in drop_rewards})
            self.termination_manager = TerminationManager(self, logging_enabled=True, term_cfg={
                "timeout": {"fn": terminations.timeout, "time_out": True},
                "fall_over": {"fn": terminations.bad_orientation, "params": {"limit_angle": 10.0, "entity_manager": self.robot_manager}}})
            ocfg = {
                "velocity_cmd": {"fn": self.velocity_command.observation},
                "angle_velocity": {"fn": lambda env: self.robot_manager.get_angular_velocity()},
                "projected_gravity": {"fn": lambda env: self.robot_manager.get_projected_gravity()},
                "dof_position": {"fn": lambda env: self.action_manager.get_dofs_position()},
                "dof_velocity": {"fn": lambda env: self.action_manager.get_dofs_velocity(), "scale": 0.05},
                "actions": {"fn": lambda env: self.action_manager.get_actions()},
            }
            self.observation_manager = ObservationManager(self, name="policy", cfg={k: v for k, v in ocfg.items() if k not in drop_obs})
            if critic:
                self.critic_manager = ObservationManager(self, name="critic", cfg={
                    "linear_velocity": {"fn": lambda env: self.robot_manager.get_linear_velocity()},
                    "dof_velocity": {"fn": lambda env: self.action_manager.get_dofs_velocity()},
                    "dof_position": {"fn": lambda env: self.action_manager.get_dofs_position(), "scale": 2.0},
                    "actions": {"fn": lambda env: self.action_manager.get_actions()}})

    return Trimmed(num_envs=n, max_episode_length_s=EPISODE_S, scene_kwargs=dict(tasks._SC))


def _make(kind, n):
    from genesis_forge_amd import tasks

    if kind == "bench":
        env = tasks.bench_env(n, max_episode_length_s=EPISODE_S)
    elif kind == "simple":   # (without the BASELINE config's contact slots, which keep the tile kernel's launch)
        env = tasks.Go2SimpleEnv(num_envs=n, max_episode_length_s=EPISODE_S, scene_kwargs=dict(tasks._SC, max_collision_pairs=0))
    elif kind == "no_vel_no_targets":
        env = _trimmed_env(n, drop_obs=("dof_velocity", "actions"))
    elif kind == "no_reward_rows":
        env = _trimmed_env(n, drop_rewards=("action_rate", "similar_to_default"))
    elif kind == "no_pos_no_lin_vel":
        env = _trimmed_env(n, drop_rewards=("base_height_target", "tracking_lin_vel", "lin_vel_z"))
    else:
        env = _trimmed_env(n, critic=True)
    env.build()
    return env


def _needs_of(env):
    return nat.get_backend().post_needs(env._trace.post_refs)


def _handover_case(kind, n, program=None, needs_on=(), needs_off=()):
    """Two envs of one seed and the same actions, one folded, one with GF_FOLD_STEP=0: the same bits after every step."""
    torch = tsf._torch()
    envs = {"on": _make(kind, n), "off": _make(kind, n)}
    try:
        for env in envs.values():
            env.seed(11)
            env.reset()
        g = torch.Generator().manual_seed(31 * n + len(kind))
        width = envs["on"].action_space.shape[0]
        done_steps, compared = [], 0
        for k in range(STEPS + 6):
            act = torch.randn(n, width, generator=g).to("cuda")
            recorded = all(e._trace is not None for e in envs.values())
            out = {}
            for name, env in envs.items():
                tsf._switch(name == "on")
                c0 = tsf._count()
                out[name] = env.step(act.clone())
                folded = tsf._count() - c0
                if recorded:
                    assert folded == (1 if name == "on" else 0), f"step {k}, switch {name}: {folded} folded launches"
            s1, s2 = tsf._state_of(envs["on"]), tsf._state_of(envs["off"])
            assert set(TICKED) <= set(s1)
            for key in s1:   # the tick's ten arrays and the reward / command state behind them, as they stand in memory
                tsf._same_bits(torch, s1[key], s2[key], f"{key} differs in memory after step {k}")
            (o1, r1, t1, u1, e1), (o2, r2, t2, u2, e2) = out["on"], out["off"]
            for what, x, y in (("observations", o1, o2), ("reward", r1, r2), ("terminated", t1, t2), ("truncated", u1, u2)):
                tsf._same_bits(torch, x, y, f"{what} differ at step {k}")
            for name in e1.get("observations", {}):   # further observation managers
                tsf._same_bits(torch, e1["observations"][name], e2["observations"][name], f"observations {name} differ at step {k}")
            assert set(e1["episode"]) == set(e2["episode"])
            for key in e1["episode"]:
                tsf._same_bits(torch, torch.as_tensor(e1["episode"][key]).double().cpu(), torch.as_tensor(e2["episode"][key]).double().cpu(),
                               f"episode log {key} differs at step {k}")
            if recorded:
                done_steps.append((t1 | u1).cpu().view(1, n))
                compared += 1
                if compared == STEPS:
                    break
        assert compared == STEPS, "the step was not recorded in time"
        dones = torch.cat(done_steps)
        assert int(dones.any(dim=0).sum()) >= min(n, 2), "fewer than two envs were reset inside the compared window"
        assert bool((~dones).any()), "no env went on without a reset inside the compared window"
        if program is not None:
            what = nat.get_backend().post_describe(envs["on"]._trace.post_refs)
            assert what.startswith(f"program {program} "), what
        needs = _needs_of(envs["on"])
        for bit in needs_on:
            assert needs & NEEDS[bit], f"needs {needs:#x} lacks {bit}: the case no longer means what it says"
        for bit in needs_off:
            assert not needs & NEEDS[bit], f"needs {needs:#x} has {bit}: the case no longer means what it says"
    finally:
        tsf._switch(True)


ALL_HANDED = ("POS", "QUAT", "LIN", "ANG", "DOFPOS", "DOFVEL", "TARGETS", "ACTIONS", "LAST", "EPLEN", "DOFDEV", "ACTRATE")


@pytest.mark.parametrize("n", [1, 63, 65, 130, N_MANY_TILES])
def test_memory_holds_what_the_tick_stored(hip_backend, n):
    _handover_case("bench", n, program=1, needs_on=ALL_HANDED)


@pytest.mark.parametrize("kind,program", [("bench", 1), ("simple", 2)])
def test_reward_wave_body_frame_from_handed_rows(hip_backend, kind, program):
    """Both static programs have the tracking terms, so their reward wave rotates the handed velocities by the handed quaternion."""
    _handover_case(kind, 65, program=program, needs_on=("QUAT", "LIN", "ANG", "POS"))


@pytest.mark.parametrize("n", [1, 63, 65, 130, N_MANY_TILES])
def test_rows_nobody_needs_dof_vel_and_targets(hip_backend, n):
    # (the table interpreter's tick variant — it hands over too — whatever programs the process has registered at run time)
    tsf._with_variant(hip_backend, "interp", lambda: _handover_case("no_vel_no_targets", n, program=0, needs_on=("DOFPOS", "ACTRATE", "DOFDEV"),
                                                                    needs_off=("DOFVEL", "TARGETS")))


@pytest.mark.parametrize("n", [1, 63, 65, 130, N_MANY_TILES])
def test_rows_nobody_needs_reward_wave_rows(hip_backend, n):
    tsf._with_variant(hip_backend, "interp", lambda: _handover_case("no_reward_rows", n, program=0, needs_on=("DOFPOS", "DOFVEL", "TARGETS"),
                                                                    needs_off=("ACTRATE", "DOFDEV")))


@pytest.mark.parametrize("n", [63, 130])
def test_base_fields_nobody_needs(hip_backend, n):
    """No reward term reads the position or the linear velocity, no observation item the latter: both waves that take base fields from
    the handed rows see zeros for them."""
    tsf._with_variant(hip_backend, "interp", lambda: _handover_case("no_pos_no_lin_vel", n, program=0, needs_on=("QUAT", "ANG", "EPLEN"),
                                                                    needs_off=("POS", "LIN")))


@pytest.mark.parametrize("n", [65, 130])
def test_two_observation_managers(hip_backend, n):
    tsf._with_variant(hip_backend, "interp", lambda: _handover_case("critic", n, program=0, needs_on=("DOFPOS", "DOFVEL", "TARGETS", "LIN")))
