"""Task configs in the reference's style — this package's restatements of the reference's six shipped examples
(examples/*/environment.py: same managers, cfg dicts, weights; pinned to the reference by tests/test_examples.py) plus two
stress configs — and ``BASELINE_CONFIGS``, the table of workloads bench.py, tools/bench_configs.py and the parity tests at
the timed sizes (tests/test_bench_parity.py) share."""
import os
import torch

from genesis_forge_amd import ManagedEnvironment
from genesis_forge_amd.managers import (ContactManager, EntityManager, ObservationManager, PositionActionManager, RewardManager,
                                        TerminationManager, VelocityCommandManager)
from genesis_forge_amd.mdp import reset, rewards, terminations, observations
from genesis_forge_amd.scene import SyntheticScene, morphs

#: the scene class the task configs below build on.  Default: the synthetic stand-in with persistent, shared state buffers;
#: ``use_scene(cls)`` swaps in another one with the same constructor (tests/genesis_like.py: Genesis' public surface only)
_SCENE_CLS = [SyntheticScene]


def new_scene(**kw):
    return _SCENE_CLS[-1](**kw)


class use_scene:
    """``with use_scene(GenesisLikeScene): env = Go2CommandDirectionEnv(...)`` — envs constructed inside build on ``cls``."""

    def __init__(self, cls):
        self.cls = cls

    def __enter__(self):
        _SCENE_CLS.append(self.cls)
        return self

    def __exit__(self, *exc):
        _SCENE_CLS.pop()


INITIAL_BODY_POSITION = [0.0, 0.0, 0.4]
INITIAL_QUAT = [1.0, 0.0, 0.0, 0.0]


GO2_JOINTS = ["FL_.*_joint", "FR_.*_joint", "RL_.*_joint", "RR_.*_joint"]
GO2_DEFAULT_POS = {".*_hip_joint": 0.0, "FL_thigh_joint": 0.8, "FR_thigh_joint": 0.8, "RL_thigh_joint": 1.0, "RR_thigh_joint": 1.0,
                   ".*_calf_joint": -1.5}


def _std_obs(self, velocity_cmd=True, scales=None):
    """The observation layout every shipped Go2 / humanoid example uses (e.g. examples/command_direction/environment.py:223-247)."""
    sc = scales or {}
    cfg = {}
    if velocity_cmd:
        cfg["velocity_cmd"] = {"fn": self.velocity_command.observation}
    cfg.update({
        "angle_velocity": {"fn": lambda env: self.robot_manager.get_angular_velocity(), "scale": sc.get("ang", 1.0)},
        "linear_velocity": {"fn": lambda env: self.robot_manager.get_linear_velocity(), "scale": sc.get("lin", 1.0)},
        "projected_gravity": {"fn": lambda env: self.robot_manager.get_projected_gravity()},
        "dof_position": {"fn": lambda env: self.action_manager.get_dofs_position()},
        "dof_velocity": {"fn": lambda env: self.action_manager.get_dofs_velocity(), "scale": 0.05},
        "actions": {"fn": lambda env: self.action_manager.get_actions()},
    })
    return cfg


class Go2SimpleEnv(ManagedEnvironment):
    """BASELINE config 1 (cf. examples/simple/environment.py:95-243): static target command, action clip ±100, no command
    manager, observation scales 0.25 / 2.0 / 0.05 (O = 45)."""

    def __init__(self, num_envs=1, dt=1 / 50, max_episode_length_s=20, scene_kwargs=None):
        super().__init__(num_envs=num_envs, dt=dt, max_episode_length_sec=max_episode_length_s, max_episode_random_scaling=0.1)
        from genesis_forge_amd import gs
        self.target_command = torch.zeros((self.num_envs, 3), device=gs.device, dtype=gs.tc_float)
        self.target_command[:, 0] = 0.5
        self.scene = new_scene(dt=self.dt, substeps=2, **dict(dict(max_collision_pairs=30), **(scene_kwargs or {})))
        self.terrain = self.scene.add_entity(morphs.Plane())
        self.robot = self.scene.add_entity(morphs.URDF(file="urdf/go2/urdf/go2.urdf", pos=INITIAL_BODY_POSITION, quat=INITIAL_QUAT))

    def config(self):
        self.robot_manager = EntityManager(self, entity_attr="robot", on_reset={
            "position": {"fn": reset.position, "params": {"position": INITIAL_BODY_POSITION, "quat": INITIAL_QUAT, "zero_velocity": True}}})
        self.action_manager = PositionActionManager(self, joint_names=GO2_JOINTS, default_pos=GO2_DEFAULT_POS, scale=0.25,
                                                    clip=(-100.0, 100.0), use_default_offset=True, pd_kp=20, pd_kv=0.5)
        RewardManager(self, logging_enabled=True, cfg={
            "base_height_target": {"weight": -50.0, "fn": rewards.base_height, "params": {"target_height": 0.3, "entity_attr": "robot"}},
            "tracking_lin_vel": {"weight": 1.0, "fn": rewards.command_tracking_lin_vel,
                                 "params": {"command": self.target_command[:, :2], "entity_manager": self.robot_manager}},
            "tracking_ang_vel": {"weight": 0.2, "fn": rewards.command_tracking_ang_vel,
                                 "params": {"commanded_ang_vel": self.target_command[:, 2], "entity_manager": self.robot_manager}},
            "lin_vel_z": {"weight": -1.0, "fn": rewards.lin_vel_z_l2, "params": {"entity_manager": self.robot_manager}},
            "action_rate": {"weight": -0.005, "fn": rewards.action_rate_l2},
            "similar_to_default": {"weight": -0.1, "fn": rewards.dof_similar_to_default, "params": {"action_manager": self.action_manager}},
        })
        self.termination_manager = TerminationManager(self, logging_enabled=True, term_cfg={
            "timeout": {"fn": terminations.timeout, "time_out": True},
            "fall_over": {"fn": terminations.bad_orientation, "params": {"limit_angle": 10.0, "entity_manager": self.robot_manager}},
        })
        ObservationManager(self, cfg=_std_obs(self, velocity_cmd=False, scales={"ang": 0.25, "lin": 2.0}))


class Go2ContactsEnv(ManagedEnvironment):
    """cf. examples/contacts/environment.py:95-290: feet_air_time on the calves (threshold 0.5 s), flat_orientation, 20° limit."""

    def __init__(self, num_envs=1, dt=1 / 50, max_episode_length_s=20, scene_kwargs=None):
        super().__init__(num_envs=num_envs, dt=dt, max_episode_length_sec=max_episode_length_s, max_episode_random_scaling=0.1)
        self.scene = new_scene(dt=self.dt, substeps=2, **dict(dict(max_collision_pairs=30), **(scene_kwargs or {})))
        self.terrain = self.scene.add_entity(morphs.Plane())
        self.robot = self.scene.add_entity(morphs.URDF(file="urdf/go2/urdf/go2.urdf", pos=[0.0, 0.0, 0.35], quat=INITIAL_QUAT))

    def config(self):
        self.robot_manager = EntityManager(self, entity_attr="robot", on_reset={
            "position": {"fn": reset.position, "params": {"position": [0.0, 0.0, 0.35], "quat": INITIAL_QUAT}}})
        self.action_manager = PositionActionManager(self, joint_names=GO2_JOINTS, default_pos=GO2_DEFAULT_POS, scale=0.5,
                                                    use_default_offset=True, pd_kp=20, pd_kv=0.5)
        self.velocity_command = VelocityCommandManager(
            self, range={"lin_vel_x": [-1.0, 1.0], "lin_vel_y": [0, 0], "ang_vel_z": [-0.5, 0.5]}, standing_probability=0.0,
            resample_time_sec=5.0, debug_visualizer=True, debug_visualizer_cfg={"envs_idx": [0]})
        self.foot_contact_manager = ContactManager(self, link_names=[".*_calf"], track_air_time=True, air_time_contact_threshold=5.0)
        em, vc = self.robot_manager, self.velocity_command
        RewardManager(self, logging_enabled=True, cfg={
            "foot_air_time": {"weight": 2.5, "fn": rewards.feet_air_time,
                              "params": {"contact_manager": self.foot_contact_manager, "vel_cmd_manager": vc, "time_threshold": 0.5}},
            "tracking_lin_vel": {"weight": 1.0, "fn": rewards.command_tracking_lin_vel, "params": {"vel_cmd_manager": vc, "entity_manager": em}},
            "tracking_ang_vel": {"weight": 0.5, "fn": rewards.command_tracking_ang_vel, "params": {"vel_cmd_manager": vc, "entity_manager": em}},
            "lin_vel_z": {"weight": -1.0, "fn": rewards.lin_vel_z_l2, "params": {"entity_manager": em}},
            "ang_vel_xy": {"weight": -0.05, "fn": rewards.ang_vel_xy_l2, "params": {"entity_manager": em}},
            "action_rate": {"weight": -0.005, "fn": rewards.action_rate_l2},
            "similar_to_default": {"weight": -0.1, "fn": rewards.dof_similar_to_default, "params": {"action_manager": self.action_manager}},
            "flat_orientation": {"weight": -2.5, "fn": rewards.flat_orientation_l2},
        })
        self.termination_manager = TerminationManager(self, logging_enabled=True, term_cfg={
            "timeout": {"fn": terminations.timeout, "time_out": True},
            "fall_over": {"fn": terminations.bad_orientation, "params": {"limit_angle": 20.0, "entity_manager": em}},
        })
        ObservationManager(self, cfg=_std_obs(self))


class BerkeleyHumanoidEnv(ManagedEnvironment):
    """BASELINE config 4 (cf. examples/berkeley_humanoid/environment.py:82-274): the reference's MJCF has 12 actuated joints;
    torso contact termination (default threshold 1.0), feet_air_time clamped to 0.2 … 0.5 s."""

    POS = [0.0, 0.0, 0.515]

    def __init__(self, num_envs=1, dt=1 / 50, max_episode_length_s=20, scene_kwargs=None):
        super().__init__(num_envs=num_envs, dt=dt, max_episode_length_sec=max_episode_length_s, max_episode_random_scaling=0.1)
        self.scene = new_scene(dt=self.dt, substeps=2, **(scene_kwargs or {}))
        self.terrain = self.scene.add_entity(morphs.Plane())
        self.robot = self.scene.add_entity(morphs.MJCF(file="./model/berkeley_humanoid.xml", pos=self.POS, quat=INITIAL_QUAT))

    def config(self):
        self.robot_manager = EntityManager(self, entity_attr="robot", on_reset={
            "position": {"fn": reset.position, "params": {"position": self.POS, "quat": INITIAL_QUAT, "zero_velocity": True}}})
        self.action_manager = PositionActionManager(
            self, joint_names=[".*"],
            default_pos={"LL_HR": -0.071, "LR_HR": 0.071, "LL_HAA": 0.103, "LR_HAA": -0.103, "LL_HFE": -0.463, "LR_HFE": -0.463,
                         "LL_KFE": 0.983, "LR_KFE": 0.983, "LL_FFE": -0.350, "LR_FFE": -0.350, "LL_FAA": 0.126, "LR_FAA": -0.126},
            scale=0.5, use_default_offset=True, pd_kp=15.0, pd_kv=1.0,
            max_force={".*_HR": 20.0, ".*_HAA": 20.0, ".*_HFE": 30.0, ".*_KFE": 30.0, ".*_FFE": 20.0, ".*_FAA": 5.0})
        self.velocity_command = VelocityCommandManager(
            self, range={"lin_vel_x": [0.0, 1.0], "lin_vel_y": [0.0, 0.0], "ang_vel_z": [-0.5, 0.5]}, standing_probability=0.02,
            resample_time_sec=5.0, debug_visualizer=True, debug_visualizer_cfg={"envs_idx": [0], "arrow_offset": 0.12})
        self.torso_contact_manager = ContactManager(self, link_names=["torso"])
        self.feet_contact_manager = ContactManager(self, link_names=[".*_faa"], track_air_time=True)
        em, vc = self.robot_manager, self.velocity_command
        RewardManager(self, logging_enabled=True, cfg={
            "tracking_lin_vel": {"weight": 1.0, "fn": rewards.command_tracking_lin_vel, "params": {"vel_cmd_manager": vc, "entity_manager": em}},
            "tracking_ang_vel": {"weight": 0.5, "fn": rewards.command_tracking_ang_vel, "params": {"vel_cmd_manager": vc, "entity_manager": em}},
            "lin_vel_z": {"weight": -2.0, "fn": rewards.lin_vel_z_l2, "params": {"entity_manager": em}},
            "ang_vel_xy_l2": {"weight": -0.05, "fn": rewards.ang_vel_xy_l2, "params": {"entity_manager": em}},
            "action_rate": {"weight": -0.005, "fn": rewards.action_rate_l2},
            "similar_to_default": {"weight": -0.05, "fn": rewards.dof_similar_to_default, "params": {"action_manager": self.action_manager}},
            "feet_air_time": {"weight": 2.0, "fn": rewards.feet_air_time,
                              "params": {"time_threshold": 0.2, "time_threshold_max": 0.5, "contact_manager": self.feet_contact_manager,
                                         "vel_cmd_manager": vc}},
        })
        self.termination_manager = TerminationManager(self, logging_enabled=True, term_cfg={
            "timeout": {"fn": terminations.timeout, "time_out": True},
            "torso_contact": {"fn": terminations.contact_force, "params": {"contact_manager": self.torso_contact_manager}},
        })
        ObservationManager(self, cfg=_std_obs(self))


class Go2GaitTrainingEnv(ManagedEnvironment):
    """BASELINE config 5 (cf. examples/gait_trainer/environment.py:26-380): velocity + gait command managers, three contact
    managers, the gait manager's two reward methods, policy (62 x 5) and critic (16 x 5) observations, and — with
    ``curriculum=True`` — the example's ``reset`` override that widens the gait set from ``last_episode_mean_reward``."""

    CHECK_EVERY = 100

    def __init__(self, num_envs=1, dt=1 / 50, max_episode_length_s=20, scene_kwargs=None, curriculum=True):
        super().__init__(num_envs=num_envs, dt=dt, max_episode_length_sec=max_episode_length_s, max_episode_random_scaling=0.4)
        self._curriculum = curriculum
        self._next_curriculum_check_step = self.CHECK_EVERY
        self.scene = new_scene(dt=self.dt, substeps=2, **dict(dict(max_collision_pairs=60), **(scene_kwargs or {})))
        self.terrain = self.scene.add_entity(morphs.Plane())
        self.robot = self.scene.add_entity(morphs.URDF(file="urdf/go2/urdf/go2.urdf", pos=INITIAL_BODY_POSITION, quat=INITIAL_QUAT,
                                                       links_to_keep=["FL_foot", "FR_foot", "RL_foot", "RR_foot"]))

    def config(self):
        from genesis_forge_amd.managers import GaitCommandManager

        self.robot_manager = EntityManager(self, entity_attr="robot", on_reset={
            "position": {"fn": reset.position, "params": {"position": INITIAL_BODY_POSITION, "quat": INITIAL_QUAT, "zero_velocity": True}}})
        self.action_manager = PositionActionManager(self, joint_names=GO2_JOINTS, default_pos=GO2_DEFAULT_POS, scale=0.25,
                                                    use_default_offset=True, pd_kp=20, pd_kv=0.5)
        self.foot_contact_manager = ContactManager(self, link_names=[".*_foot"], air_time_contact_threshold=1.0)
        self.body_contact_manager = ContactManager(self, link_names=["base"], air_time_contact_threshold=1.0)
        self.bad_contact_manager = ContactManager(self, link_names=[".*_thigh", ".*_calf"])
        self.velocity_command = VelocityCommandManager(
            self, range={"lin_vel_x": [-1.0, 1.0], "lin_vel_y": [0.0, 0.0], "ang_vel_z": [-1.0, 1.0]}, standing_probability=0.00,
            resample_time_sec=3.0)
        self.gait_command_manager = GaitCommandManager(
            self, foot_names={"FL": "FL_foot", "FR": "FR_foot", "RL": "RL_foot", "RR": "RR_foot"}, resample_time_sec=4.0)
        em, vc, gait = self.robot_manager, self.velocity_command, self.gait_command_manager
        self.reward_manager = RewardManager(self, logging_enabled=True, cfg={
            "gait_phase_reward": {"weight": 1.5, "fn": gait.gait_phase_reward, "params": {"contact_manager": self.foot_contact_manager}},
            "foot_height_reward": {"weight": 0.9, "fn": gait.foot_height_reward},
            "base_height_target": {"weight": -25.0, "fn": rewards.base_height, "params": {"target_height": 0.35, "entity_attr": "robot"}},
            "tracking_lin_vel": {"weight": 1.0, "fn": rewards.command_tracking_lin_vel, "params": {"vel_cmd_manager": vc, "entity_manager": em}},
            "tracking_ang_vel": {"weight": 0.5, "fn": rewards.command_tracking_ang_vel, "params": {"vel_cmd_manager": vc, "entity_manager": em}},
            "body_acceleration": {"weight": -0.1, "fn": rewards.body_acceleration_exp, "params": {"entity_manager": em}},
            "lin_vel_z": {"weight": -0.1, "fn": rewards.lin_vel_z_l2, "params": {"entity_manager": em}},
            "action_rate": {"weight": -0.01, "fn": rewards.action_rate_l2},
            "bad_contact": {"weight": -1.0, "fn": rewards.contact_force, "params": {"contact_manager": self.bad_contact_manager}},
        })
        self.termination_manager = TerminationManager(self, logging_enabled=True, term_cfg={
            "timeout": {"fn": terminations.timeout, "time_out": True},
            "fall_over": {"fn": terminations.bad_orientation, "params": {"limit_angle": 20.0, "entity_manager": em}},
            "body_contact": {"fn": terminations.contact_force, "params": {"contact_manager": self.body_contact_manager, "threshold": 1.0}},
        })
        ocfg = {"gait_command": {"fn": gait.observation}}
        ocfg.update(_std_obs(self))
        ObservationManager(self, name="policy", history_len=5, cfg=ocfg)
        ObservationManager(self, name="critic", history_len=5, cfg={
            "foot_contact_force": {"fn": observations.contact_force, "params": {"contact_manager": self.foot_contact_manager}},
            "dof_force": {"fn": observations.entity_dofs_force, "params": {"action_manager": self.action_manager}, "scale": 0.1},
        })

    def update_curriculum(self):
        """cf. examples/gait_trainer/environment.py:354-380"""
        if self.step_count < self._next_curriculum_check_step:
            return
        self._next_curriculum_check_step = self.step_count + self.CHECK_EVERY
        if self.reward_manager.last_episode_mean_reward("gait_phase_reward", before_weight=True) > 0.75:
            self.gait_command_manager.increment_num_gaits()
            self.gait_command_manager.increment_gait_period_range()
        if self.reward_manager.last_episode_mean_reward("foot_height_reward", before_weight=True) > 0.8:
            self.gait_command_manager.increment_foot_clearance_range()


def _gait_reset_with_curriculum(self, envs_idx=None):
    out = ManagedEnvironment.reset(self, envs_idx)
    if envs_idx is not None and self._curriculum:
        self.update_curriculum()
    return out


class Go2GaitTrainingCurriculumEnv(Go2GaitTrainingEnv):
    """The example's ``reset`` override (examples/gait_trainer/environment.py:347-352).  Kept in a subclass: an env that
    overrides ``reset`` gets the reference's index-list reset path: its step is recorded up to the reset, the reset and the
    observations run phase by phase (_trace.StepTrace.tail_python)."""

    reset = _gait_reset_with_curriculum


def make_example(name: str, case: dict):
    """This package's restatement of the reference example ``name`` with the case's scene options (tests/example_cases.py)."""
    kw = dict(num_envs=case["n"], max_episode_length_s=case["episode_s"], scene_kwargs=dict(case["scene"]))
    if name == "simple":
        return Go2SimpleEnv(**kw)
    if name == "command_direction":
        kw["scene_kwargs"].setdefault("max_collision_pairs", 30)
        return Go2CommandDirectionEnv(**kw)
    if name == "contacts":
        return Go2ContactsEnv(**kw)
    if name == "rough_terrain":
        return Go2RoughTerrainEnv(height_reward=False, **kw)
    if name == "berkeley_humanoid":
        return BerkeleyHumanoidEnv(**kw)
    if name == "gait_trainer":
        return Go2GaitTrainingCurriculumEnv(**kw)
    raise KeyError(name)


class Go2CommandDirectionEnv(ManagedEnvironment):
    """BASELINE config 2: Go2 12-DOF, 6 rewards, 2 terminations, velocity command, 7 observation items (O=48)."""

    def __init__(self, num_envs=1, dt=1 / 50, max_episode_length_s=20, scene_kwargs=None, obs_noise=False, fused_obs=True,
                 contacts=False, history=None, cmd_resample_s=5.0, dofs=12):
        super().__init__(num_envs=num_envs, dt=dt, max_episode_length_sec=max_episode_length_s, max_episode_random_scaling=0.1)
        kw = dict(scene_kwargs or {})
        if contacts:
            kw.setdefault("max_collision_pairs", 12)
        self._contacts, self._history, self._cmd_resample_s, self._dofs = contacts, history, cmd_resample_s, dofs
        self.scene = new_scene(dt=self.dt, substeps=2, **kw)
        self.terrain = self.scene.add_entity(morphs.Plane())
        if dofs == 12:
            self.robot = self.scene.add_entity(morphs.URDF(file="urdf/go2/urdf/go2.urdf", pos=INITIAL_BODY_POSITION, quat=INITIAL_QUAT))
        else:  # the same manager stack over a synthetic `dofs`-joint robot (BASELINE.md plan B2: D in {12, 28})
            from genesis_forge_amd.scene import humanoid_model
            self.robot = self.scene.add_entity(model=humanoid_model(dofs))
        self._obs_noise = obs_noise
        self._fused_obs = fused_obs

    def config(self):
        self.robot_manager = EntityManager(self, entity_attr="robot", on_reset={
            "position": {"fn": reset.position, "params": {"position": INITIAL_BODY_POSITION, "quat": INITIAL_QUAT, "zero_velocity": True}}})
        if self._dofs == 12:
            joint_names, default_pos = GO2_JOINTS, GO2_DEFAULT_POS
        else:
            joint_names, default_pos = [".*"], {".*": 0.1}
        self.action_manager = getattr(self, "action_cls", PositionActionManager)(   # (tests plug a user-defined action manager class in)
            self, joint_names=joint_names, default_pos=default_pos, scale=0.25, use_default_offset=True, pd_kp=20, pd_kv=0.5)
        self.velocity_command = VelocityCommandManager(
            self, range={"lin_vel_x": [-1.0, 1.0], "lin_vel_y": [-1.0, 1.0], "ang_vel_z": [-1.0, 1.0]}, standing_probability=0.02,
            resample_time_sec=self._cmd_resample_s)
        rcfg = {
            "base_height_target": {"weight": -50.0, "fn": rewards.base_height, "params": {"target_height": 0.3, "entity_attr": "robot"}},
            "tracking_lin_vel": {"weight": 1.0, "fn": rewards.command_tracking_lin_vel,
                                 "params": {"vel_cmd_manager": self.velocity_command, "entity_manager": self.robot_manager}},
            "tracking_ang_vel": {"weight": 0.5, "fn": rewards.command_tracking_ang_vel,
                                 "params": {"vel_cmd_manager": self.velocity_command, "entity_manager": self.robot_manager}},
            "lin_vel_z": {"weight": -1.0, "fn": rewards.lin_vel_z_l2, "params": {"entity_manager": self.robot_manager}},
            "action_rate": {"weight": -0.005, "fn": rewards.action_rate_l2},
            "similar_to_default": {"weight": -0.1, "fn": rewards.dof_similar_to_default, "params": {"action_manager": self.action_manager}},
        }
        tcfg = {
            "timeout": {"fn": terminations.timeout, "time_out": True},
            "fall_over": {"fn": terminations.bad_orientation, "params": {"limit_angle": 10.0, "entity_manager": self.robot_manager}},
        }
        if self._contacts:
            self.foot_contacts = ContactManager(self, link_names=[".*_foot"], track_air_time=True, air_time_contact_threshold=5.0)
            self.body_contacts = ContactManager(self, link_names=[".*_thigh", "base"])
            rcfg["foot_air_time"] = {"weight": 2.5, "fn": rewards.feet_air_time,
                                     "params": {"contact_manager": self.foot_contacts, "time_threshold": 0.05,
                                                "vel_cmd_manager": self.velocity_command}}
            rcfg["undesired_contacts"] = {"weight": -1.0, "fn": rewards.has_contact,
                                          "params": {"contact_manager": self.body_contacts, "threshold": 5.0}}
            rcfg["ang_vel_xy"] = {"weight": -0.05, "fn": rewards.ang_vel_xy_l2, "params": {"entity_manager": self.robot_manager}}
            rcfg["flat_orientation"] = {"weight": -2.5, "fn": rewards.flat_orientation_l2, "params": {"entity_manager": self.robot_manager}}
            rcfg["terminated"] = {"weight": -100.0, "fn": rewards.terminated}
            rcfg["zero_weight"] = {"weight": 0.0, "fn": rewards.is_alive}
            tcfg["body_contact"] = {"fn": terminations.contact_force, "params": {"contact_manager": self.body_contacts, "threshold": 30.0}}
        self.reward_manager = RewardManager(self, logging_enabled=True, cfg=rcfg)
        self.termination_manager = TerminationManager(self, logging_enabled=True, term_cfg=tcfg)
        noise = 0.01 if self._obs_noise else None
        ocfg = {
            "velocity_cmd": {"fn": self.velocity_command.observation},
            "angle_velocity": {"fn": lambda env: self.robot_manager.get_angular_velocity(), "noise": noise},
            "linear_velocity": {"fn": lambda env: self.robot_manager.get_linear_velocity()},
            "projected_gravity": {"fn": lambda env: self.robot_manager.get_projected_gravity()},
            "dof_position": {"fn": lambda env: self.action_manager.get_dofs_position()},
            "dof_velocity": {"fn": lambda env: self.action_manager.get_dofs_velocity(), "scale": 0.05},
            "actions": {"fn": lambda env: self.action_manager.get_actions()},
        }
        if self._contacts:
            ocfg["foot_force"] = {"fn": observations.contact_force, "params": {"contact_manager": self.foot_contacts}, "scale": 0.1}
        self.observation_manager = ObservationManager(self, fused=self._fused_obs, cfg=ocfg, history_len=self._history)


class HumanoidGaitLikeEnv(ManagedEnvironment):
    """Stress config for the fused post-physics kernel: synthetic 28-DOF humanoid (BASELINE config 4's size), two
    command managers, two observation managers (policy with history, critic), three contact managers, the stateful
    body_acceleration_exp term, PositionWithinLimitsActionManager, zero-weight and contact terms."""

    def __init__(self, num_envs=1, dofs=28, dt=1 / 50, max_episode_length_s=1, scene_kwargs=None):
        super().__init__(num_envs=num_envs, dt=dt, max_episode_length_sec=max_episode_length_s, max_episode_random_scaling=0.4)
        from genesis_forge_amd.scene import humanoid_model
        kw = dict(max_collision_pairs=10, ang_noise=0.3, contact_prob=0.3, seed=21)
        kw.update(scene_kwargs or {})
        self.scene = new_scene(dt=self.dt, substeps=2, **kw)
        self.terrain = self.scene.add_entity(morphs.Plane())
        self.robot = self.scene.add_entity(model=humanoid_model(dofs))

    def config(self):
        from genesis_forge_amd.managers import CommandManager, PositionWithinLimitsActionManager
        self.robot_manager = EntityManager(self, entity_attr="robot", on_reset={
            "position": {"fn": reset.position, "params": {"position": [0.0, 0.0, 0.55], "quat": [1.0, 0.0, 0.0, 0.0]}}})
        self.action_manager = PositionWithinLimitsActionManager(self, joint_names=".*", default_pos={".*": 0.1}, noise_scale=0.02)
        self.velocity_command = VelocityCommandManager(self, range={"lin_vel_x": [-1.0, 1.0], "lin_vel_y": [0.0, 0.0], "ang_vel_z": [-1.0, 1.0]},
                                                       resample_time_sec=0.3)
        self.height_command = CommandManager(self, range=(0.3, 0.6), resample_time_sec=0.4)
        self.feet = ContactManager(self, link_names=[".*_faa"], track_air_time=True, air_time_contact_threshold=1.0)
        self.torso = ContactManager(self, link_names=["torso"])
        self.legs = ContactManager(self, link_names=[".*_kfe", ".*_hfe"], track_air_time=True)
        self.reward_manager = RewardManager(self, cfg={
            "lin": {"weight": 1.0, "fn": rewards.command_tracking_lin_vel, "params": {"vel_cmd_manager": self.velocity_command, "entity_manager": self.robot_manager}},
            "ang": {"weight": 0.5, "fn": rewards.command_tracking_ang_vel, "params": {"vel_cmd_manager": self.velocity_command, "entity_manager": self.robot_manager}},
            "accel": {"weight": -0.1, "fn": rewards.body_acceleration_exp, "params": {"entity_manager": self.robot_manager}},
            "rate": {"weight": -0.005, "fn": rewards.action_rate_l2},
            "pose": {"weight": -0.05, "fn": rewards.dof_similar_to_default, "params": {"action_manager": self.action_manager}},
            "still": {"weight": -0.2, "fn": rewards.stand_still_joint_deviation_l1, "params": {"vel_cmd_manager": self.velocity_command, "action_manager": self.action_manager, "command_threshold": 0.3}},
            "air": {"weight": 2.0, "fn": rewards.feet_air_time, "params": {"contact_manager": self.feet, "time_threshold": 0.04, "time_threshold_max": 0.5, "vel_cmd_manager": self.velocity_command}},
            "bad_contact": {"weight": -1.0, "fn": rewards.contact_force, "params": {"contact_manager": self.legs, "threshold": 2.0}},
            "slide": {"weight": -0.1, "fn": rewards.feet_slide, "params": {"contact_manager": self.feet}},
            "alive": {"weight": 0.3, "fn": rewards.is_alive},
            "off": {"weight": 0.0, "fn": rewards.flat_orientation_l2, "params": {"entity_manager": self.robot_manager}},
            "flat": {"weight": -1.0, "fn": rewards.flat_orientation_l2, "params": {"entity_manager": self.robot_manager}},
            "height": {"weight": -5.0, "fn": rewards.base_height, "params": {"target_height": 0.5}},
        })
        self.termination_manager = TerminationManager(self, term_cfg={
            "timeout": {"fn": terminations.timeout, "time_out": True},
            "fall": {"fn": terminations.bad_orientation, "params": {"limit_angle": 20.0, "entity_manager": self.robot_manager, "grace_steps": 3}},
            "torso": {"fn": terminations.contact_force, "params": {"contact_manager": self.torso, "threshold": 25.0}},
            "low": {"fn": terminations.base_height_below_minimum, "params": {"minimum_height": 0.2, "entity_manager": self.robot_manager}},
        })
        self.observation_manager = ObservationManager(self, name="policy", history_len=3, noise=0.01, cfg={
            "height_cmd": {"fn": self.height_command.observation},
            "velocity_cmd": {"fn": self.velocity_command.observation},
            "ang": {"fn": lambda env: self.robot_manager.get_angular_velocity(), "scale": 0.25},
            "grav": {"fn": lambda env: self.robot_manager.get_projected_gravity()},
            "pos": {"fn": lambda env: self.action_manager.get_dofs_position()},
            "vel": {"fn": lambda env: self.action_manager.get_dofs_velocity(), "scale": 0.05},
            "act": {"fn": lambda env: self.action_manager.get_actions()},
        })
        self.critic_manager = ObservationManager(self, name="critic", cfg={
            "feet": {"fn": observations.contact_force, "params": {"contact_manager": self.feet}, "scale": 0.1},
            "lin": {"fn": lambda env: self.robot_manager.get_linear_velocity()},
            "force": {"fn": observations.entity_dofs_force, "params": {"action_manager": self.action_manager}},
            "raw": {"fn": observations.current_actions},
        })


def graded_height_field(n_subterrains, cell_size, horizontal_scale: float, vertical_scale: float, max_height: float, level_axis: int = 0,
                        seed: int = 2024):
    """A deterministic integer height field (Genesis' layout: ``[nx * rows, ny * cols]`` height steps, metres = value *
    ``vertical_scale``) for a grid of ``n_subterrains`` cells: blocky random roughness (1 m blocks) whose amplitude in a cell of level
    ``l`` is ``max_height * (l + 1) / num_levels`` — level 0 the gentlest, the top level ``max_height``."""
    import numpy as np

    nx, ny = int(n_subterrains[0]), int(n_subterrains[1])
    rows, cols = int(cell_size[0] / horizontal_scale + 1e-9), int(cell_size[1] / horizontal_scale + 1e-9)
    levels = nx if level_axis == 0 else ny
    blk = max(1, int(round(1.0 / horizontal_scale)))
    rng = np.random.RandomState(seed)
    hf = np.zeros((nx * rows, ny * cols), dtype=np.int16)
    for i in range(nx):
        for j in range(ny):
            level = i if level_axis == 0 else j
            top = int(round(max_height * (level + 1) / levels / vertical_scale))
            coarse = rng.randint(0, top + 1, size=((rows + blk - 1) // blk, (cols + blk - 1) // blk))
            hf[i * rows:(i + 1) * rows, j * cols:(j + 1) * cols] = np.kron(coarse, np.ones((blk, blk), dtype=np.int64))[:rows, :cols]
    return hf


class Go2RoughTerrainEnv(ManagedEnvironment):
    """BASELINE config 3 (cf. examples/rough_terrain/environment.py:87-287): Go2 on a height-field terrain, TerrainManager,
    random terrain spawn with random yaw on reset, out_of_bounds termination, two contact managers, 9 reward terms — plus
    (``height_reward=True``) ``base_height(terrain_manager=…)`` so the in-kernel height lookup is on the path.
    ``height_scan`` (a dict of ``HeightScanner`` keyword arguments; ``{}`` is the default 17 x 11 grid) adds ``self.height_scanner``
    and a second ObservationManager, ``"critic"``: the policy's items plus the terrain heights around the base — the privileged input of
    an asymmetric critic (``RolloutStorage(env, T, obs_groups={"policy": ["policy"], "critic": ["critic"]})``) or of a teacher.
    ``None`` (the default) builds what the reference's example builds: a blind policy.
    ``depth_camera`` (a dict of ``RayCaster`` keyword arguments; ``{}`` is a 16 x 12 pinhole at 87 degrees horizontal, mounted at the
    front of the trunk and pitched 30 degrees down, 4 m range, depth output) adds ``self.depth_camera`` and an ObservationManager
    ``"depth"`` that holds that one item: what a deployable student sees
    (``obs_groups={"policy": ["policy", "depth"], "teacher": ["critic"]}``).  ``None`` builds the managers above and nothing else.
    ``curriculum`` (a dict: ``num_levels`` (5), ``num_types`` (2), ``cell_size`` ((8, 8) metres), ``max_height`` (0.1 m, the roughness of the
    top level) and ``TerrainCurriculum`` keyword arguments) makes the terrain a ``num_levels x num_types`` grid of cells whose roughness
    grows with the level index — an explicit deterministic height field (``graded_height_field``) — adds ``self.terrain_curriculum`` and
    replaces the one-rectangle spawn by ``mdp.reset.terrain_curriculum_position``: every env respawns in its own cell and moves a level up
    or down with the distance it walked.  ``None`` (the default) builds exactly what it built before.  It composes with ``height_scan``
    and ``depth_camera``.
    ``push`` (a dict of ``PushDisturbance`` keyword arguments; ``{}`` kicks x and y with up to 0.5 m/s every 10 to 15 s) adds ``self.push``
    and a ``step()`` that runs it behind the step with the step's done masks: one more launch, the step inside stays the recorded one.
    ``None`` (the default): the step is the parent class's.
    ``action_delay`` (a dict of ``lag_steps`` / ``max_lag``; ``{}`` is ``lag_steps=(0, 2)``) builds a ``DelayedPositionActionManager`` in
    place of the ``PositionActionManager``: the targets reach the actuators a per-env, per-episode number of control steps late, and
    ``self.action_delay`` is its ``ActuatorDelay``.  The action phase of the step then is the bookkeeping launch, the manager's code, the
    process launch and the delay launch; the rest of the step stays recorded.  ``None`` (the default) builds exactly what it built before."""

    #: the default sensor of ``depth_camera={}``
    DEPTH_CAMERA = dict(offset_pos=(0.3, 0.0, 0.05), offset_euler=(0.0, 30.0, 0.0), align="base", max_range=4.0, output="depth")

    def __init__(self, num_envs=1, dt=1 / 50, max_episode_length_s=20, scene_kwargs=None, height_reward=True, rotation="default",
                 terrain_kwargs=None, cmd_resample_s=5.0, height_scan=None, depth_camera=None, curriculum=None, push=None, action_delay=None):
        super().__init__(num_envs=num_envs, dt=dt, max_episode_length_sec=max_episode_length_s, max_episode_random_scaling=0.1)
        self._curriculum = None if curriculum is None else dict(curriculum)
        self._push = None if push is None else dict(push)
        self.push = None
        self._action_delay = None if action_delay is None else dict(action_delay)
        self.action_delay = None
        kw = dict(scene_kwargs or {})
        kw.setdefault("max_collision_pairs", 12)
        self._height_reward, self._rotation, self._cmd_resample_s = height_reward, rotation, cmd_resample_s
        self._height_scan = None if height_scan is None else dict(height_scan)
        self._depth_camera = None if depth_camera is None else dict(depth_camera)
        self.scene = new_scene(dt=self.dt, substeps=2, **kw)
        tk = dict(pos=(-12, -12, 0), n_subterrains=(1, 1), subterrain_size=(24, 24), vertical_scale=0.001,
                  subterrain_types=[["random_uniform_terrain"]],
                  subterrain_parameters={"random_uniform_terrain": {"min_height": 0.0, "max_height": 0.1, "step": 0.05, "downsampled_scale": 0.25}})
        if self._curriculum is not None:
            cur = self._curriculum
            levels, types = int(cur.pop("num_levels", 5)), int(cur.pop("num_types", 2))
            cell = tuple(float(v) for v in cur.pop("cell_size", (8.0, 8.0)))
            max_height = float(cur.pop("max_height", 0.1))
            if levels < 1 or types < 1 or len(cell) != 2 or min(cell) <= 0.0 or max_height < 0.0:
                raise ValueError("curriculum needs num_levels >= 1, num_types >= 1, a positive cell_size (x, y) and max_height >= 0")
            if cur.get("level_axis", "x") not in ("x", "y"):
                raise ValueError("level_axis must be 'x' or 'y'")
            n_sub = (levels, types) if cur.get("level_axis", "x") == "x" else (types, levels)
            tk.update(pos=(-n_sub[0] * cell[0] / 2, -n_sub[1] * cell[1] / 2, 0), n_subterrains=n_sub, subterrain_size=cell,
                      subterrain_types=[["random_uniform_terrain"] * n_sub[1] for _ in range(n_sub[0])])
            tk.update(terrain_kwargs or {})
            if tk.get("height_field") is None:
                # explicit: the stand-in scene's generator keys its parameters by type name, and every cell here has the same type
                tk["height_field"] = graded_height_field(n_sub, cell, tk.get("horizontal_scale", 0.25), tk["vertical_scale"], max_height,
                                                         level_axis=0 if cur.get("level_axis", "x") == "x" else 1)
        else:
            tk.update(terrain_kwargs or {})
        self.terrain = self.scene.add_entity(morph=morphs.Terrain(**tk))
        self.robot = self.scene.add_entity(morphs.URDF(file="urdf/go2/urdf/go2.urdf", pos=INITIAL_BODY_POSITION, quat=INITIAL_QUAT))

    def config(self):
        from genesis_forge_amd.managers import TerrainManager

        self.terrain_manager = TerrainManager(self)
        make_command = lambda: VelocityCommandManager(
            self, range={"lin_vel_x": [-1.0, 1.0], "lin_vel_y": [-1.0, 1.0], "ang_vel_z": [-0.5, 0.5]}, standing_probability=0.05,
            resample_time_sec=self._cmd_resample_s)
        if self._curriculum is not None:
            from genesis_forge_amd.managers import TerrainCurriculum

            self.velocity_command = make_command()   # (the curriculum reads the command an episode starts with)
            self.terrain_curriculum = TerrainCurriculum(self, self.terrain_manager, command_manager=self.velocity_command, **self._curriculum)
            spawn, params = reset.terrain_curriculum_position, {"height_offset": 0.4, "curriculum": self.terrain_curriculum}
        else:
            spawn, params = reset.randomize_terrain_position, {"height_offset": 0.4, "terrain_manager": self.terrain_manager}
        if self._rotation != "default":
            params["rotation"] = self._rotation
        self.robot_manager = EntityManager(self, entity_attr="robot", on_reset={"position": {"fn": spawn, "params": params}})
        make_actions, delay_kw = PositionActionManager, {}
        if self._action_delay is not None:
            from genesis_forge_amd.managers import DelayedPositionActionManager

            make_actions, delay_kw = DelayedPositionActionManager, dict({"lag_steps": (0, 2)}, **self._action_delay)
        self.action_manager = make_actions(
            self, joint_names=["FL_.*_joint", "FR_.*_joint", "RL_.*_joint", "RR_.*_joint"],
            default_pos={".*_hip_joint": 0.0, "FL_thigh_joint": 0.8, "FR_thigh_joint": 0.8, "RL_thigh_joint": 1.0, "RR_thigh_joint": 1.0,
                         ".*_calf_joint": -1.5},
            scale=0.25, use_default_offset=True, pd_kp=20, pd_kv=0.5, max_force=23.5, **delay_kw)
        if self._curriculum is None:
            self.velocity_command = make_command()
        self.foot_contact_manager = ContactManager(self, link_names=[".*_calf"], track_air_time=True, air_time_contact_threshold=5.0)
        self.undesired_contacts = ContactManager(self, link_names=[".*_thigh", "base"])
        rcfg = {
            "tracking_lin_vel": {"weight": 1.5, "fn": rewards.command_tracking_lin_vel,
                                 "params": {"vel_cmd_manager": self.velocity_command, "entity_manager": self.robot_manager}},
            "tracking_ang_vel": {"weight": 0.75, "fn": rewards.command_tracking_ang_vel,
                                 "params": {"vel_cmd_manager": self.velocity_command, "entity_manager": self.robot_manager}},
            "lin_vel_z": {"weight": -2.0, "fn": rewards.lin_vel_z_l2, "params": {"entity_manager": self.robot_manager}},
            "ang_vel_xy": {"weight": -0.05, "fn": rewards.ang_vel_xy_l2, "params": {"entity_manager": self.robot_manager}},
            "undesired_contacts": {"weight": -1.0, "fn": rewards.has_contact, "params": {"contact_manager": self.undesired_contacts, "threshold": 5.0}},
            "action_rate": {"weight": -0.01, "fn": rewards.action_rate_l2},
            "similar_to_default": {"weight": -0.1, "fn": rewards.dof_similar_to_default, "params": {"action_manager": self.action_manager}},
            "flat_orientation": {"weight": -1.5, "fn": rewards.flat_orientation_l2},
            "terminated": {"weight": -100.0, "fn": rewards.terminated},
        }
        if self._height_reward:
            rcfg["base_height"] = {"weight": -30.0, "fn": rewards.base_height,
                                   "params": {"target_height": 0.35, "terrain_manager": self.terrain_manager, "entity_manager": self.robot_manager}}
        self.reward_manager = RewardManager(self, logging_enabled=True, cfg=rcfg)
        self.termination_manager = TerminationManager(self, logging_enabled=True, term_cfg={
            "timeout": {"fn": terminations.timeout, "time_out": True},
            "out_of_bounds": {"fn": terminations.out_of_bounds, "params": {"terrain_manager": self.terrain_manager}},
            "bad_orientation": {"fn": terminations.bad_orientation,
                                "params": {"limit_angle": 30.0, "entity_manager": self.robot_manager, "grace_steps": 20}},
        })
        policy_items = lambda: {
            "velocity_cmd": {"fn": self.velocity_command.observation},
            "angle_velocity": {"fn": lambda env: self.robot_manager.get_angular_velocity()},
            "linear_velocity": {"fn": lambda env: self.robot_manager.get_linear_velocity()},
            "projected_gravity": {"fn": lambda env: self.robot_manager.get_projected_gravity()},
            "dof_position": {"fn": lambda env: self.action_manager.get_dofs_position()},
            "dof_velocity": {"fn": lambda env: self.action_manager.get_dofs_velocity(), "scale": 0.05},
            "actions": {"fn": lambda env: self.action_manager.get_actions()},
        }
        self.observation_manager = ObservationManager(self, cfg=policy_items())
        if self._height_scan is not None:
            from genesis_forge_amd.managers import HeightScanner

            self.height_scanner = HeightScanner(self, self.terrain_manager, entity_manager=self.robot_manager, **self._height_scan)
            self.critic_manager = ObservationManager(self, name="critic", cfg=dict(
                policy_items(), height_scan={"fn": observations.height_scan, "params": {"scanner": self.height_scanner}}))
        if self._depth_camera is not None:
            from genesis_forge_amd.managers import RayCaster
            from genesis_forge_amd.managers.ray_caster import pinhole_pattern

            kw = dict(self.DEPTH_CAMERA, **self._depth_camera)
            if kw.get("pattern") is None:
                kw["pattern"] = pinhole_pattern(16, 12, 87.0)
            self.depth_camera = RayCaster(self, self.terrain_manager, entity_manager=self.robot_manager, **kw)
            self.depth_manager = ObservationManager(self, name="depth", cfg={
                "depth": {"fn": observations.ray_cast, "params": {"caster": self.depth_camera}}})
        if self._push is not None:
            from genesis_forge_amd.managers import PushDisturbance

            self.push = PushDisturbance(self, entity_manager=self.robot_manager, **self._push)

    def build(self):
        super().build()
        if self._action_delay is not None:
            self.action_delay = self.action_manager.delay
        if self.push is not None:
            self.push.build()

    def step(self, actions):
        """The step, then the pushes with the step's done masks (code around ``super().step()``: the step inside is recorded as ever)."""
        out = super().step(actions)
        if self.push is not None:
            self.push.step(out[2], out[3])
        return out


# ----------------------------------------------------------------------------------------------------------------------------
# The workloads that get TIMED (bench.py: "go2_cmd"; tools/bench_configs.py: all of them).  tests/test_bench_parity.py walks the
# same table and compares every one of them with the oracle at the size it is timed at.
# Stand-in physics settings: small attitude noise (about 0.2 % of the envs fall over per step; SURVEY.md §8d's input spec would
# reset 2-8 % per step, which times the reset path rather than the step) and, for the configs with ContactManagers, the WALKING
# contact model of the synthetic scene (GfSynthSceneArgs.foot_link_mask): the links the config's foot ContactManager tracks touch
# the ground in a trot pattern — two to four feet of a quadruped (one or two of a biped) per tick, the ground on either side of the
# contact pair, so the Taichi kernel's matching branches (managers/contact/kernel.py:47-78), the air-time bookkeeping and
# feet_air_time (mdp/rewards.py:431-469) do real work every step — while body contacts (base / torso / thigh / calf) stay rare
# enough that the configs that terminate on them reset 0.3-0.5 % of the envs per step (episodes of a few hundred steps).
# ----------------------------------------------------------------------------------------------------------------------------
_SC = dict(ang_noise=0.05, seed=1234)
_CON = dict(_SC, contact_prob=0.15, contact_force=40.0)


def _walk(foot_links, body_prob, **kw):
    if os.environ.get("GF_SPARSE_CONTACTS") == "1":   # round 3's near-empty contact tables (0.03-0.06 contacts per env and step), for comparison only
        return dict(_SC, contact_force=40.0, contact_prob=body_prob, **kw)
    return dict(_SC, contact_force=40.0, foot_links=foot_links, foot_contact_prob=0.5, contact_prob=body_prob, **kw)


def bench_env(num_envs: int, **kw):
    """bench.py's workload: BASELINE.json's Go2 12-DOF config with the full Reward / Termination / Command manager stack."""
    return Go2CommandDirectionEnv(num_envs=num_envs, max_episode_length_s=kw.pop("max_episode_length_s", 20), scene_kwargs=dict(_SC), **kw)


#: name -> (BASELINE.json size, factory(num_envs, **env_kwargs))
BASELINE_CONFIGS = {
    "simple": (4096, lambda n, **kw: Go2SimpleEnv(num_envs=n, scene_kwargs=dict(_SC), **kw)),
    "go2_cmd": (4096, lambda n, **kw: bench_env(n, **kw)),
    "go2_cmd_65536": (65536, lambda n, **kw: bench_env(n, **kw)),
    "contacts": (4096, lambda n, **kw: Go2ContactsEnv(num_envs=n, scene_kwargs=_walk(".*_calf", 0.01), **kw)),
    "rough_terrain": (16384, lambda n, **kw: Go2RoughTerrainEnv(num_envs=n, height_reward=False,
                                                               scene_kwargs=_walk(".*_calf", 0.01, max_collision_pairs=30), **kw)),
    "humanoid": (8192, lambda n, **kw: BerkeleyHumanoidEnv(num_envs=n, scene_kwargs=_walk(".*_faa", 0.002, max_collision_pairs=30), **kw)),
    # BASELINE config 4 as stated ("~28-DOF"): the same kind of manager stack over a synthetic 28-joint humanoid (the reference's
    # berkeley_humanoid example, "humanoid" above, has 12 actuated joints)
    "humanoid28": (8192, lambda n, **kw: HumanoidGaitLikeEnv(num_envs=n, dofs=28, **kw)),
    "gait": (65536, lambda n, **kw: Go2GaitTrainingEnv(num_envs=n, scene_kwargs=_walk(".*_foot", 0.001), **kw)),
    # a USER's config: the Go2 task with observation noise — a structure none of the library's built-in programs has, so its fused
    # launch runs the program compiled for it at run time (genesis_forge_amd/_programs.py; GF_JIT) instead of the interpreter
    "go2_user": (65536, lambda n, **kw: bench_env(n, obs_noise=True, **kw)),
    "gait_8192": (8192, lambda n, **kw: Go2GaitTrainingEnv(num_envs=n, scene_kwargs=_walk(".*_foot", 0.001), **kw)),
    # the gait example AS SHIPPED: with its reset() override (curriculum hook, examples/gait_trainer/environment.py:347-352) — the reset
    # runs through user code by index list; what is recorded around it: GF_POST_NO_RESET in front, GF_POST_OBSERVE_ONLY behind
    "gait_override_8192": (8192, lambda n, **kw: Go2GaitTrainingCurriculumEnv(num_envs=n, scene_kwargs=_walk(".*_foot", 0.001), **kw)),
}
