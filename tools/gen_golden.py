#!/usr/bin/env python3
"""
Generate tests/golden/*.npz by running the REFERENCE (/root/reference/genesis_forge, imported with the
stubs of tools/ref_stubs.py) and recording its inputs and outputs.  Runs only in the build container
(the reference never travels); the fixtures are data and are committed.

The reference drives the same synthetic scene the package uses (through its Genesis-style public API,
stepped by the CPU oracle), its uniform_ calls are served from Philox draws (tests/philox.py) that the
tests feed to the kernels in parity mode, so a fixture pins the reference's manager logic — phase
order, which envs resample/reset, weights, op order — not torch's RNG stream.

Usage: python tools/gen_golden.py                     rewrites the unit fixtures and the traj_go2_* trajectories
       python tools/gen_golden.py examples [key ...]  rewrites traj_ex_<key>.npz — the reference's own example files
                                                      (tests/example_cases.py: six examples at n = 8 + the multi-tile cases)
       python tools/gen_golden.py entity_obs | contact_kernel | contact_edges | mask_edges   one unit fixture
"""
import math
import os
import sys

sys.dont_write_bytecode = True  # importing from /root/reference must not leave __pycache__ behind there

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ref_stubs  # noqa: E402

my_scene = ref_stubs.install()

import philox  # noqa: E402  (tests/)
from oracle_backend import OracleBackend  # noqa: E402  (tests/)
from genesis_forge_amd import _native as nat  # noqa: E402

nat.set_backend(OracleBackend(os.path.join(ROOT, "oracle", "libgf_oracle.so")))

import genesis_forge as ref  # noqa: E402  — the reference
from genesis_forge.managers import (ContactManager, EntityManager, ObservationManager, PositionActionManager,  # noqa: E402
                                    PositionWithinLimitsActionManager, RewardManager, TerminationManager, VelocityCommandManager,
                                    CommandManager)
from genesis_forge.mdp import reset, rewards, terminations, observations  # noqa: E402

assert ref.__file__.startswith("/root/reference"), ref.__file__
GOLD = os.path.join(ROOT, "tests", "golden")
SEED = 20251017

# ------------------------------------------------------------------------------------------------
# uniform_ interception: the reference's draws come from dense Philox arrays chosen by context
# ------------------------------------------------------------------------------------------------
CTX = {"mode": None}
_orig_uniform = torch.Tensor.uniform_


def _patched_uniform(self, lo=0.0, hi=1.0):
    mode = CTX["mode"]
    if mode is None:
        raise RuntimeError("uniform_ outside a known context")
    lo32, hi32 = np.float32(lo), np.float32(hi)
    if mode == "len":       # genesis_env.py:249
        u = CTX["u"][CTX["ids"], 0]
    elif mode == "cmd":     # command_manager.py:302 — i-th call fills range i
        u = CTX["u"][CTX["ids"], CTX["i"]]
        CTX["i"] += 1
    elif mode == "obs":     # observation_manager.py:249 — next noisy item's columns
        c0, w = CTX["cols"].pop(0)
        u = CTX["u"][:, c0:c0 + w]
    elif mode == "spawn":   # mdp/reset.py:182-193 — one call per axis given as a (lo, hi) tuple, in x, y, z order
        u = CTX["u"][CTX["ids"], 2 + CTX["axes"].pop(0)]
    else:
        raise RuntimeError(mode)
    val = (u.astype(np.float32) * np.float32(hi32 - lo32) + lo32).astype(np.float32)
    self.copy_(torch.from_numpy(np.ascontiguousarray(val)).reshape(self.shape))
    return self


torch.Tensor.uniform_ = _patched_uniform


def _patched_rand_like(t, *a, **k):
    """terrain_manager.py:236-241: the x then the y coordinates of the spawn points."""
    if CTX["mode"] != "spawn":
        raise RuntimeError("rand_like outside a known context")
    u = CTX["u"][CTX["ids"], CTX["i"]]
    CTX["i"] += 1
    return torch.from_numpy(np.ascontiguousarray(u.astype(np.float32))).reshape(t.shape)


torch.rand_like = _patched_rand_like


class Draws:
    """Per-step dense draws, shared convention with tests (philox.draws)."""

    def __init__(self, n, n_ranges, obs_width):
        self.n, self.r, self.o = n, n_ranges, obs_width
        self.step = 0

    def get(self, kind, cols):
        return philox.draws(SEED, self.step, kind, self.n, cols)


def _ids_np(ids, n):
    if ids is None:
        return np.arange(n)
    return np.asarray(torch.as_tensor(ids).cpu().numpy(), dtype=np.int64)


_HOLD = {"draws": None, "installed": False}


class _DrawsProxy:
    def get(self, kind, cols):
        return _HOLD["draws"].get(kind, cols)


def install_contexts(env, draws_obj: Draws):
    """Wrap the reference methods that consume RNG so the patched uniform_ knows what is being drawn."""
    _HOLD["draws"] = draws_obj
    if _HOLD["installed"]:
        return
    _HOLD["installed"] = True
    draws = _DrawsProxy()
    from genesis_forge import genesis_env as ge
    from genesis_forge.managers.command import command_manager as cm
    from genesis_forge.managers import observation_manager as om

    orig_reset = ge.GenesisEnv.reset

    def reset_wrap(self, envs_idx=None):
        CTX.update(mode="len", ids=_ids_np(envs_idx, self.num_envs), u=draws.get(2, 1))
        try:
            return orig_reset(self, envs_idx)
        finally:
            CTX["mode"] = None

    ge.GenesisEnv.reset = reset_wrap

    orig_resample = cm.CommandManager.resample_command

    def resample_wrap(self, env_ids):
        kind = 0 if CTX.get("cmd_phase") == "step" else 1
        CTX.update(mode="cmd", ids=_ids_np(env_ids, self.env.num_envs), i=0, u=draws.get(kind, self._command.shape[1]))
        try:
            return orig_resample(self, env_ids)
        finally:
            CTX["mode"] = None

    cm.CommandManager.resample_command = resample_wrap

    orig_step = cm.CommandManager.step

    def step_wrap(self):
        CTX["cmd_phase"] = "step"
        try:
            return orig_step(self)
        finally:
            CTX["cmd_phase"] = None

    cm.CommandManager.step = step_wrap

    orig_perform = om.ObservationManager._perform_observation

    def perform_wrap(self):
        cols, c = [], 0
        noisy = any((cfg.noise or self.noise) not in (None, 0.0) for cfg in self.cfg.values())
        for name, cfg in (self.cfg.items() if noisy else ()):
            w = OBS_WIDTHS[(self.name, name)]
            noise = cfg.noise or self.noise
            if noise is not None and noise != 0.0:
                cols.append((c, w))
            c += w
        CTX.update(mode="obs", cols=cols, u=draws.get(3, c) if noisy else None)
        try:
            return orig_perform(self)
        finally:
            CTX["mode"] = None

    om.ObservationManager._perform_observation = perform_wrap

    from genesis_forge.mdp import reset as rmod

    orig_spawn = rmod.randomize_terrain_position.__call__

    def spawn_wrap(self, env, entity, envs_idx, terrain_manager, height_offset=0.1e-3, subterrain=None,
                   rotation={"z": (0, 2 * math.pi)}, zero_velocity=True):
        axes = [k for k, ax in enumerate("xyz") if rotation is not None and isinstance(rotation.get(ax, 0), tuple)]
        CTX.update(mode="spawn", ids=_ids_np(envs_idx, env.num_envs), i=0, axes=axes, u=draws.get(4, 5))
        try:
            return orig_spawn(self, env, entity, envs_idx, terrain_manager, height_offset=height_offset, subterrain=subterrain,
                              rotation=rotation, zero_velocity=zero_velocity)
        finally:
            CTX["mode"] = None

    rmod.randomize_terrain_position.__call__ = spawn_wrap


OBS_WIDTHS = {}

INITIAL_BODY_POSITION = [0.0, 0.0, 0.4]
INITIAL_QUAT = [1.0, 0.0, 0.0, 0.0]
GO2_DEFAULT = {".*_hip_joint": 0.0, "FL_thigh_joint": 0.8, "FR_thigh_joint": 0.8, "RL_thigh_joint": 1.0, "RR_thigh_joint": 1.0,
               ".*_calf_joint": -1.5}
GO2_JOINTS = ["FL_.*_joint", "FR_.*_joint", "RL_.*_joint", "RR_.*_joint"]


class RefGo2Env(ref.ManagedEnvironment):
    """Reference ManagedEnvironment on the synthetic scene; manager cfg mirrors the command_direction example's values."""

    def __init__(self, num_envs, episode_s=20, scene_kwargs=None, contacts=False, obs_noise=True, history=None, variant="cmd"):
        super().__init__(num_envs=num_envs, dt=1 / 50, max_episode_length_sec=episode_s, max_episode_random_scaling=0.1)
        kw = dict(scene_kwargs or {})
        if contacts:
            kw.setdefault("max_collision_pairs", 12)
        self.scene = my_scene.SyntheticScene(dt=self.dt, substeps=2, **kw)
        self.terrain = self.scene.add_entity(my_scene.morphs.Plane())
        self.robot = self.scene.add_entity(my_scene.morphs.URDF(file="urdf/go2/urdf/go2.urdf", pos=INITIAL_BODY_POSITION, quat=INITIAL_QUAT))
        self._contacts, self._obs_noise, self._history, self._variant = contacts, obs_noise, history, variant

    def config(self):
        self.robot_manager = EntityManager(self, entity_attr="robot", on_reset={
            "position": {"fn": reset.position, "params": {"position": INITIAL_BODY_POSITION, "quat": INITIAL_QUAT, "zero_velocity": True}}})
        self.action_manager = PositionActionManager(self, joint_names=GO2_JOINTS, default_pos=GO2_DEFAULT, scale=0.25,
                                                    use_default_offset=True, pd_kp=20, pd_kv=0.5)
        self.velocity_command = VelocityCommandManager(
            self, range={"lin_vel_x": [-1.0, 1.0], "lin_vel_y": [-1.0, 1.0], "ang_vel_z": [-1.0, 1.0]}, standing_probability=0.02,
            resample_time_sec=CMD_RESAMPLE_S)
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
        RewardManager(self, logging_enabled=True, cfg=rcfg)
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
        widths = [3, 3, 3, 3, 12, 12, 12]
        if self._contacts:
            ocfg["foot_force"] = {"fn": observations.contact_force, "params": {"contact_manager": self.foot_contacts}, "scale": 0.1}
            widths.append(4)
        for (k, w) in zip(ocfg.keys(), widths):
            OBS_WIDTHS[("policy", k)] = w
        ObservationManager(self, cfg=ocfg, history_len=self._history)


CMD_RESAMPLE_S = 1.0

ROUGH_TERRAIN = dict(pos=(-12, -12, 0), n_subterrains=(1, 1), subterrain_size=(24, 24), vertical_scale=0.001,
                     subterrain_types=[["random_uniform_terrain"]],
                     subterrain_parameters={"random_uniform_terrain": {"min_height": 0.0, "max_height": 0.1, "step": 0.05,
                                                                      "downsampled_scale": 0.25}})


class RefGo2RoughEnv(ref.ManagedEnvironment):
    """Reference managers in the arrangement of examples/rough_terrain/environment.py:87-287 (plus base_height over the terrain),
    on the synthetic scene with a height-field terrain entity.  Mirrors tests/envs.py Go2RoughTerrainEnv."""

    def __init__(self, num_envs, episode_s=20, scene_kwargs=None, terrain_kwargs=None, rotation="default"):
        super().__init__(num_envs=num_envs, dt=1 / 50, max_episode_length_sec=episode_s, max_episode_random_scaling=0.1)
        kw = dict(scene_kwargs or {})
        kw.setdefault("max_collision_pairs", 12)
        self.scene = my_scene.SyntheticScene(dt=self.dt, substeps=2, **kw)
        tk = dict(ROUGH_TERRAIN)
        tk.update(terrain_kwargs or {})
        self.terrain = self.scene.add_entity(morph=my_scene.morphs.Terrain(**tk))
        self.robot = self.scene.add_entity(my_scene.morphs.URDF(file="urdf/go2/urdf/go2.urdf", pos=INITIAL_BODY_POSITION, quat=INITIAL_QUAT))
        self._rotation = rotation

    def config(self):
        from genesis_forge.managers import TerrainManager

        self.terrain_manager = TerrainManager(self)
        params = {"height_offset": 0.4, "terrain_manager": self.terrain_manager}
        if self._rotation != "default":
            params["rotation"] = self._rotation
        self.robot_manager = EntityManager(self, entity_attr="robot", on_reset={"position": {"fn": reset.randomize_terrain_position, "params": params}})
        self.action_manager = PositionActionManager(self, joint_names=GO2_JOINTS, default_pos=GO2_DEFAULT, scale=0.25, use_default_offset=True,
                                                    pd_kp=20, pd_kv=0.5, max_force=23.5)
        self.velocity_command = VelocityCommandManager(
            self, range={"lin_vel_x": [-1.0, 1.0], "lin_vel_y": [-1.0, 1.0], "ang_vel_z": [-0.5, 0.5]}, standing_probability=0.05,
            resample_time_sec=CMD_RESAMPLE_S)
        self.foot_contact_manager = ContactManager(self, link_names=[".*_calf"], track_air_time=True, air_time_contact_threshold=5.0)
        self.undesired_contacts = ContactManager(self, link_names=[".*_thigh", "base"])
        RewardManager(self, logging_enabled=True, cfg={
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
            "base_height": {"weight": -30.0, "fn": rewards.base_height,
                            "params": {"target_height": 0.35, "terrain_manager": self.terrain_manager, "entity_manager": self.robot_manager}},
        })
        self.termination_manager = TerminationManager(self, logging_enabled=True, term_cfg={
            "timeout": {"fn": terminations.timeout, "time_out": True},
            "out_of_bounds": {"fn": terminations.out_of_bounds, "params": {"terrain_manager": self.terrain_manager}},
            "bad_orientation": {"fn": terminations.bad_orientation,
                                "params": {"limit_angle": 30.0, "entity_manager": self.robot_manager, "grace_steps": 20}},
        })
        ocfg = {
            "velocity_cmd": {"fn": self.velocity_command.observation},
            "angle_velocity": {"fn": lambda env: self.robot_manager.get_angular_velocity()},
            "linear_velocity": {"fn": lambda env: self.robot_manager.get_linear_velocity()},
            "projected_gravity": {"fn": lambda env: self.robot_manager.get_projected_gravity()},
            "dof_position": {"fn": lambda env: self.action_manager.get_dofs_position()},
            "dof_velocity": {"fn": lambda env: self.action_manager.get_dofs_velocity(), "scale": 0.05},
            "actions": {"fn": lambda env: self.action_manager.get_actions()},
        }
        for (k, w) in zip(ocfg.keys(), [3, 3, 3, 3, 12, 12, 12]):
            OBS_WIDTHS[("policy", k)] = w
        ObservationManager(self, cfg=ocfg)


def episode_scalars(extras):
    return {k: float(v) for k, v in extras["episode"].items()}


def run_trajectory(name, n, steps, contacts, history, scene_kwargs, episode_s=2, variant="cmd", rotation="default", save=True):
    torch.manual_seed(0)
    if variant == "rough":
        env = RefGo2RoughEnv(n, episode_s=episode_s, scene_kwargs=scene_kwargs, rotation=rotation)
    else:
        env = RefGo2Env(n, episode_s=episode_s, scene_kwargs=scene_kwargs, contacts=contacts, history=history)
    obs_w = 48 + (4 if contacts else 0)
    draws = Draws(n, 3, obs_w)
    install_contexts(env, draws)
    draws.step = 0
    env.build()
    obs0, _ = env.reset()
    rng = np.random.RandomState(7)
    rec = {k: [] for k in ("actions", "obs", "reward", "terminated", "truncated", "command", "episode_length", "max_episode_length", "pos", "quat")}
    logs = []
    for t in range(steps):
        draws.step = t + 1
        act = rng.standard_normal((n, 12)).astype(np.float32)
        if t == 5:
            act[0, 0] = 1e9  # clip path
        obs, rew, term, trunc, extras = env.step(torch.from_numpy(act))
        rec["actions"].append(act)
        rec["obs"].append(obs.numpy().copy())
        rec["reward"].append(rew.numpy().copy())
        rec["terminated"].append(term.numpy().copy())
        rec["truncated"].append(trunc.numpy().copy())
        rec["command"].append(env.velocity_command._command.numpy().copy())
        rec["episode_length"].append(env.episode_length.numpy().copy())
        rec["max_episode_length"].append(env.max_episode_length.numpy().copy())
        rec["pos"].append(env.robot.get_pos().numpy().copy())
        rec["quat"].append(env.robot.get_quat().numpy().copy())
        logs.append(episode_scalars(extras))
    keys = sorted({k for d in logs for k in d})
    log_arr = np.full((steps, len(keys)), np.nan, dtype=np.float64)
    for t, d in enumerate(logs):
        for j, k in enumerate(keys):
            if k in d:
                log_arr[t, j] = d[k]
    out = {k: np.stack(v) for k, v in rec.items()}
    out.update(obs0=obs0.numpy().copy(), log_keys=np.array(keys), log_values=log_arr, seed=np.int64(SEED), n=np.int64(n),
               steps=np.int64(steps), contacts=np.int64(contacts), history=np.int64(history or 1), episode_s=np.float64(episode_s),
               cmd_resample_s=np.float64(CMD_RESAMPLE_S), scene_kwargs=np.array(repr(scene_kwargs)), variant=np.array(variant),
               rotation=np.array(repr(rotation)))
    if save:
        np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    print(name, "steps", steps, "terminated", int(out["terminated"].sum()), "truncated", int(out["truncated"].sum()),
          "log keys", len(keys))
    return out


# ------------------------------------------------------------------------------------------------
# The reference at the sizes that get timed: every other fixture is <= 130 envs
# ------------------------------------------------------------------------------------------------
AT_SIZE = {"steps": 20, "episode_s": 0.3, "cmd_resample_s": 0.2, "contacts": False, "history": 2,
           "scene_kwargs": dict(ang_noise=0.35, lin_noise=0.05, seed=17, contact_prob=0.3, contact_force=30.0)}
def at_size_name(n, contacts, variant="cmd"):
    return f"atsize_rough_{n}" if variant == "rough" else f"atsize_go2{'c' if contacts else ''}_{n}"


def run_reference_at_size(n, contacts=None, variant="cmd"):
    """The reference's own ManagedEnvironment.step (managed_env.py:274-334) at n envs — in memory, no file.  ``contacts``: with the
    two ContactManagers of the contacts example (the reference's Taichi kernel source runs under the serial `ti` emulation of
    tools/ref_stubs.py: ≈ 8 s per step at 4 096 envs, two minutes per step at 65 536 — so that variant exists at 4 096 envs only)."""
    global CMD_RESAMPLE_S
    contacts = AT_SIZE["contacts"] if contacts is None else contacts
    keep, CMD_RESAMPLE_S = CMD_RESAMPLE_S, AT_SIZE["cmd_resample_s"]
    try:
        if variant == "rough":   # BASELINE config 3's structure (terrain lookups, spawn on the terrain, out of bounds, two ContactManagers)
            return run_trajectory(at_size_name(n, False, "rough"), n=n, steps=AT_SIZE["steps"], contacts=False, history=None, variant="rough",
                                  scene_kwargs=AT_SIZE["scene_kwargs"], episode_s=AT_SIZE["episode_s"], save=False)
        return run_trajectory(at_size_name(n, contacts), n=n, steps=AT_SIZE["steps"], contacts=contacts, history=AT_SIZE["history"],
                              scene_kwargs=AT_SIZE["scene_kwargs"], episode_s=AT_SIZE["episode_s"], save=False)
    finally:
        CMD_RESAMPLE_S = keep


def gen_at_size():
    """Compact, reference-derived fixtures for the GPU box (tests/helpers.py: compact_at_size says what they hold)."""
    import helpers
    # `at_size` regenerates the three fixtures that take minutes; `at_size go2c_65536` the contact-manager run at 65 536 envs (the
    # serial Taichi emulation: ≈ 2 minutes per step, ≈ 45 minutes); `at_size <name>` any single one
    only = sys.argv[2] if len(sys.argv) > 2 else os.environ.get("GF_AT_SIZE_ONLY")
    # … `at_size rough_16384` BASELINE config 3's structure at its size (two ContactManagers under the emulation: ≈ 12 minutes)
    for n, contacts, variant in ((4096, False, "cmd"), (65536, False, "cmd"), (4096, True, "cmd"), (65536, True, "cmd"), (16384, False, "rough")):
        name = at_size_name(n, contacts, variant)
        if (only and name != "atsize_" + only) or (not only and ((n, contacts) == (65536, True) or variant == "rough")):
            continue
        out = run_reference_at_size(n, contacts, variant)
        assert np.array_equal(out["actions"], helpers.at_size_actions(n, int(out["steps"]))), "the tests regenerate the actions from the same stream"
        np.savez_compressed(os.path.join(GOLD, name + ".npz"), **helpers.compact_at_size(out, n))


def check_at_size(n, contacts=False):
    """Container only: the reference itself at n envs against this package on the CPU oracle — the same actions, the same draws,
    every env of every step, compared in lockstep (nothing is stored: a 65 536-env trajectory is 0.5 GB)."""
    import helpers
    global CMD_RESAMPLE_S
    keep, CMD_RESAMPLE_S = CMD_RESAMPLE_S, AT_SIZE["cmd_resample_s"]
    try:
        torch.manual_seed(0)
        ref_env = RefGo2Env(n, episode_s=AT_SIZE["episode_s"], scene_kwargs=AT_SIZE["scene_kwargs"], contacts=contacts,
                            history=AT_SIZE["history"])
        width = (48 + (4 if contacts else 0)) * (AT_SIZE["history"] or 1)
        draws = Draws(n, 3, width)
        install_contexts(ref_env, draws)
        draws.step = 0
        ref_env.build()
        meta = dict(n=n, seed=SEED, contacts=int(contacts), history=AT_SIZE["history"] or 1, scene_kwargs=repr(AT_SIZE["scene_kwargs"]),
                    variant="cmd", episode_s=AT_SIZE["episode_s"], cmd_resample_s=AT_SIZE["cmd_resample_s"], obs=np.empty((0, width), dtype=np.float32))
        env, _n, seed, frame, _h = helpers._trajectory_env(meta)
    finally:
        CMD_RESAMPLE_S = keep
    tol = helpers.FLOAT_TOL
    helpers.set_step_draws(env, seed, 0, n, 3, frame, "cpu")
    a0, _ = ref_env.reset()
    b0, _ = env.reset()
    np.testing.assert_allclose(b0.numpy(), a0.numpy(), atol=tol, rtol=0)
    rng = np.random.RandomState(7)
    dones = 0
    for t in range(AT_SIZE["steps"]):
        draws.step = t + 1
        act = rng.standard_normal((n, 12)).astype(np.float32)
        if t == 5:
            act[0, 0] = 1e9
        helpers.set_step_draws(env, seed, t + 1, n, 3, frame, "cpu")
        ra = ref_env.step(torch.from_numpy(act))
        rb = env.step(torch.from_numpy(act.copy()))
        for name, x, y in (("terminated", ra[2], rb[2]), ("truncated", ra[3], rb[3]), ("episode_length", ref_env.episode_length, env.episode_length),
                           ("max_episode_length", ref_env.max_episode_length, env.max_episode_length)):
            assert np.array_equal(x.numpy(), y.numpy()), f"{name} differs at step {t}"
        for name, x, y in (("obs", ra[0], rb[0]), ("reward", ra[1], rb[1]), ("command", ref_env.velocity_command._command, env.velocity_command._command),
                           ("pos", ref_env.robot.get_pos(), env.robot.get_pos()), ("quat", ref_env.robot.get_quat(), env.robot.get_quat())):
            np.testing.assert_allclose(y.numpy(), x.numpy(), atol=tol, rtol=0, err_msg=f"{name} step {t}")
        la, lb = episode_scalars(ra[4]), {k: float(v) for k, v in rb[4]["episode"].items()}
        assert set(la) == set(lb), f"log keys differ at step {t}: {sorted(la)} vs {sorted(lb)}"
        for k in la:
            assert abs(la[k] - lb[k]) <= 1e-5 + 1e-5 * abs(la[k]), f"log {k} at step {t}: {lb[k]} vs {la[k]}"
        dones += int(ra[2].sum() + ra[3].sum())
    assert dones > n // 10, f"only {dones} resets at {n} envs"
    print(f"reference == package (oracle backend) at {n} envs{' with contact managers' if contacts else ''} x {AT_SIZE['steps']} steps, {dones} resets, every env compared")


# ------------------------------------------------------------------------------------------------
# Unit fixtures: every mdp.rewards / mdp.terminations term on random states
# ------------------------------------------------------------------------------------------------
def random_state(env, rng, n):
    r = env.robot
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    r.pos[:] = torch.tensor([0.0, 0.0, 0.35]) + 0.05 * f(n, 3)
    q = torch.tensor([1.0, 0.0, 0.0, 0.0]) + 0.1 * f(n, 4)
    r.quat[:] = q / q.norm(dim=-1, keepdim=True)
    r.lin_vel[:] = f(n, 3)
    r.ang_vel[:] = f(n, 3)
    r.dof_pos[:] = env.action_manager.default_dofs_pos + 0.3 * f(n, 12)
    r.dof_vel[:] = 2.0 * f(n, 12)
    r.links_vel = f(n, r.n_links, 3)
    env.velocity_command._command[:] = torch.from_numpy(rng.uniform(-1, 1, (n, 3)).astype(np.float32))
    env.velocity_command._command[: n // 8, :2] *= 0.05  # some near-zero commands
    env._actions = f(n, 12)
    env._last_actions = f(n, 12)
    env.episode_length[:] = torch.from_numpy(rng.randint(0, 1100, n).astype(np.int32))
    env.max_episode_length[:] = torch.from_numpy(rng.randint(900, 1100, n).astype(np.int32))
    for cm_ in env.managers["contact"]:
        L = cm_.contacts.shape[1]
        cm_.contacts[:] = 6.0 * f(n, L, 3) * torch.from_numpy((rng.uniform(size=(n, L, 1)) < 0.6).astype(np.float32))
        if cm_.last_air_time is not None:
            cm_.last_air_time[:] = torch.from_numpy(rng.uniform(0, 0.6, (n, L)).astype(np.float32))
            cct = rng.uniform(0, 0.1, (n, L)).astype(np.float32)
            cct[rng.uniform(size=(n, L)) < 0.3] = np.float32(0.02)  # exactly dt: "just made contact"
            cct[rng.uniform(size=(n, L)) < 0.3] = 0.0
            cm_.current_contact_time[:] = torch.from_numpy(cct)
    for em in env.managers["entity"]:
        em.step()
    env.extras["terminations"] = torch.from_numpy(rng.uniform(size=n) < 0.2)


def state_dict(env):
    r = env.robot
    d = dict(pos=r.pos, quat=r.quat, lin_vel=r.lin_vel, ang_vel=r.ang_vel, dof_pos=r.dof_pos, dof_vel=r.dof_vel, links_vel=r.links_vel,
             command=env.velocity_command._command, actions=env._actions, last_actions=env._last_actions,
             episode_length=env.episode_length, max_episode_length=env.max_episode_length, terminations=env.extras["terminations"])
    for k, cm_ in enumerate(env.managers["contact"]):
        d[f"contacts{k}"] = cm_.contacts
        if cm_.last_air_time is not None:
            d[f"last_air{k}"] = cm_.last_air_time
            d[f"cur_contact{k}"] = cm_.current_contact_time
    return {k: v.numpy().copy() for k, v in d.items()}


def gen_terms():
    n = 257
    env = RefGo2Env(n, contacts=True, obs_noise=False)
    env.build()
    rng = np.random.RandomState(11)
    random_state(env, rng, n)
    out = {"in_" + k: v for k, v in state_dict(env).items()}
    em, am, vc = env.robot_manager, env.action_manager, env.velocity_command
    foot, body = env.foot_contacts, env.body_contacts
    explicit_cmd = torch.from_numpy(rng.uniform(-1, 1, (n, 2)).astype(np.float32))
    explicit_ang = torch.from_numpy(rng.uniform(-1, 1, (n,)).astype(np.float32))
    out["in_explicit_cmd"], out["in_explicit_ang"] = explicit_cmd.numpy(), explicit_ang.numpy()
    bacc = rewards.body_acceleration_exp(env, entity_manager=em)
    R = {
        "is_alive": rewards.is_alive(env),
        "terminated": rewards.terminated(env),
        "base_height": rewards.base_height(env, target_height=0.3),
        "dof_similar_to_default": rewards.dof_similar_to_default(env, action_manager=am),
        "lin_vel_z_l2": rewards.lin_vel_z_l2(env, entity_manager=em),
        "lin_vel_z_l2_attr": rewards.lin_vel_z_l2(env, entity_attr="robot"),
        "ang_vel_xy_l2": rewards.ang_vel_xy_l2(env, entity_manager=em),
        "flat_orientation_l2": rewards.flat_orientation_l2(env, entity_manager=em),
        "body_acceleration_exp_first": bacc(env, entity_manager=em),
        "action_rate_l2": rewards.action_rate_l2(env),
        "command_tracking_lin_vel": rewards.command_tracking_lin_vel(env, vel_cmd_manager=vc, entity_manager=em),
        "command_tracking_lin_vel_explicit": rewards.command_tracking_lin_vel(env, command=explicit_cmd, entity_manager=em, sensitivity=0.5),
        "command_tracking_ang_vel": rewards.command_tracking_ang_vel(env, vel_cmd_manager=vc, entity_manager=em),
        "command_tracking_ang_vel_explicit": rewards.command_tracking_ang_vel(env, commanded_ang_vel=explicit_ang, entity_manager=em),
        "stand_still": rewards.stand_still_joint_deviation_l1(env, vel_cmd_manager=vc, action_manager=am),
        "has_contact": rewards.has_contact(env, contact_manager=body, threshold=5.0, min_contacts=2),
        "contact_force": rewards.contact_force(env, contact_manager=body, threshold=2.0),
        "feet_air_time": rewards.feet_air_time(env, contact_manager=foot, time_threshold=0.2, vel_cmd_manager=vc),
        "feet_air_time_max": rewards.feet_air_time(env, contact_manager=foot, time_threshold=0.2, time_threshold_max=0.5),
        "feet_slide": rewards.feet_slide(env, contact_manager=foot),
    }
    # second call of the stateful term with a new state
    prev = state_dict(env)
    random_state(env, rng, n)
    out.update({"in2_" + k: v for k, v in state_dict(env).items()})
    R["body_acceleration_exp_second"] = bacc(env, entity_manager=em, sensitivity=0.1)
    # restore first state for terminations
    T = {}
    for ang in (10.0, 20.0, 30.0, 40.0):
        T[f"bad_orientation_{int(ang)}"] = terminations.bad_orientation(env, limit_angle=ang, entity_manager=em)
    T["bad_orientation_grace"] = terminations.bad_orientation(env, limit_angle=10.0, entity_manager=em, grace_steps=500)
    T["timeout"] = terminations.timeout(env)
    T["base_height_below"] = terminations.base_height_below_minimum(env, minimum_height=0.33, entity_manager=em)
    T["has_contact"] = terminations.has_contact(env, contact_manager=body, threshold=5.0, min_contacts=2)
    T["contact_force"] = terminations.contact_force(env, contact_manager=body, threshold=8.0)
    T["contact_force_grace"] = terminations.contact_force_with_grace_period(env, contact_manager=body, threshold=8.0, grace_steps=400)

    class _TM:
        def get_bounds(self, sub=None):
            return (-0.1, 0.1, -0.08, 0.12)

    T["out_of_bounds"] = terminations.out_of_bounds(env, terrain_manager=_TM(), border_margin=0.03)
    for k, v in R.items():
        out["rew_" + k] = v.detach().numpy().astype(np.float32)
    for k, v in T.items():
        out["term_" + k] = v.numpy()
    np.savez_compressed(os.path.join(GOLD, "terms_go2.npz"), **out)
    print("terms_go2:", len(R), "reward outputs,", len(T), "termination outputs")


def gen_orientation_sweep():
    """Dense sweep of quaternions whose tilt sits within a few ulps of each threshold."""
    env = RefGo2Env(8, obs_noise=False)
    env.build()
    quats, masks, angs = [], [], []
    for ang in (10.0, 20.0, 30.0, 40.0, 85.0):
        thr = math.radians(ang) if ang < 82 else math.asin(0.99)
        base = np.float32(min(thr, math.asin(0.99)))
        tilt = base + np.arange(-600, 601, dtype=np.float64) * 2e-8
        # rotation about x by tilt: q = (cos(t/2), sin(t/2), 0, 0) → |g_xy| = sin(tilt)
        for axis in (1, 2):
            q = np.zeros((tilt.size, 4), dtype=np.float64)
            q[:, 0] = np.cos(tilt / 2)
            q[:, axis] = np.sin(tilt / 2)
            q32 = q.astype(np.float32)
            n = q32.shape[0]
            env2 = env
            res = []
            for s in range(0, n, 8):
                chunk = q32[s:s + 8]
                m = chunk.shape[0]
                env2.robot.quat[:m] = torch.from_numpy(chunk)
                env2.robot_manager.step()
                env2.episode_length[:] = 5
                r = terminations.bad_orientation(env2, limit_angle=ang, entity_manager=env2.robot_manager)
                res.append(r.numpy()[:m].copy())
            quats.append(q32)
            masks.append(np.concatenate(res))
            angs.append(np.full(n, ang, dtype=np.float32))
    np.savez_compressed(os.path.join(GOLD, "orientation_sweep.npz"), quat=np.concatenate(quats), mask=np.concatenate(masks),
                        limit=np.concatenate(angs))
    print("orientation_sweep:", sum(m.size for m in masks), "cases,", int(sum(m.sum() for m in masks)), "fired")


# ------------------------------------------------------------------------------------------------
# mask_edges: every mask-valued decision at its boundary (tests/mask_edges_cases.py holds the env, the config and the block layout)
# ------------------------------------------------------------------------------------------------
def _ulps(x, k):
    """float32 ``x`` moved by k representable values (k > 0: towards +inf)."""
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return x


def _oblique(rng, thr, n, dim):
    """n random ``dim``-vectors whose exact length lies within ±4 ulp of float32(thr)."""
    t32 = np.float32(thr)
    sp = float(np.spacing(t32))
    sp_below = float(t32) - float(np.nextafter(t32, np.float32(0.0), dtype=np.float32))
    out = np.zeros((0, dim), dtype=np.float32)
    while len(out) < n:
        d = rng.standard_normal((2 * n, dim))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        # (aimed within one representable value of the threshold on either side — below a power of two they lie twice as dense —
        # where the rounding of the sum of squares decides the comparison; the components' own rounding spreads them further)
        k = rng.uniform(-1.0, 1.0, (2 * n, 1))
        v = (d * (float(t32) + k * np.where(k > 0, sp, sp_below))).astype(np.float32)
        exact = np.sqrt((v.astype(np.float64) ** 2).sum(axis=1))
        out = np.concatenate([out, v[np.abs(exact - float(t32)) <= 4.0 * sp]])
    return out[:n]


def _codes(n):
    """Placement codes (mask_edges_cases.link_index): the group of four rotates fastest, then the place in the group."""
    i = np.arange(n)
    return (4 * (i % 3) + (i // 3) % 4).astype(np.int8)


def mask_edge_blocks(benign):
    """name -> dict(thr, limit, variants, arrays): the inputs of every block, made from fixed seeds."""
    import mask_edges_cases as mc

    rng = np.random.RandomState(20260131)
    blocks = {}
    all_variants = list(range(len(mc.VARIANTS)))

    def add(name, arrays, thr=5.0, limit=10.0, variants=None):
        assert name not in blocks
        n = {a.shape[0] for a in arrays.values()}
        assert len(n) == 1 and n.pop() <= mc.N_ENVS, name
        if "force" in arrays:   # up to MAX_FORCES forces per row, zero where a block places fewer
            f = np.zeros((arrays["force"].shape[0], mc.MAX_FORCES, 3), dtype=np.float32)
            f[:, : arrays["force"].shape[1]] = arrays["force"]
            arrays = dict(arrays, force=f)
        blocks[name] = dict(thr=thr, limit=limit, variants=all_variants if variants is None else variants, arrays=arrays)

    def rep(key, n):
        return np.repeat(benign[key][None], n, axis=0).copy()

    # -- norm against a threshold, 3-vectors ---------------------------------------------------------------------------------------
    for thr in mc.THRESHOLDS:
        vs = [k for k, v in enumerate(mc.VARIANTS) if v["thr"] == thr]
        t32 = np.float32(thr)
        rows = []
        for k in (-1, 0, 1):
            for axis in range(3):
                for sign in (1.0, -1.0):
                    for _place in range(3):
                        f = np.zeros(3, dtype=np.float32)
                        f[axis] = np.float32(sign) * _ulps(t32, k)
                        rows.append(f)
        f = np.stack(rows)[:, None, :]
        add(f"c3_{thr}_axis", {"force": f, "code": _codes(len(f))}, thr=thr, variants=vs)
        f = _oblique(rng, thr, mc.N_ENVS, 3)[:, None, :]
        add(f"c3_{thr}_oblique", {"force": f, "code": _codes(len(f))}, thr=thr, variants=vs)
        # has_contact's count: 0, 1 or 2 links far over the threshold next to the probed one -> min_contacts - 1, min_contacts, min_contacts + 1
        n = 3 * 64
        f = np.zeros((n, 3, 3), dtype=np.float32)
        f[:, 0] = _oblique(rng, thr, n, 3)
        far = np.arange(n) // 64
        f[far >= 1, 1, 0] = np.float32(3.0 * thr)
        f[far >= 2, 2, 1] = np.float32(-3.0 * thr)
        add(f"c3_{thr}_count", {"force": f, "code": _codes(n)}, thr=thr, variants=vs)
        # the grace variant: episode_length = grace - 1, grace, grace + 1
        f = _oblique(rng, thr, n, 3)[:, None, :]
        ep = (mc.GRACE - 1 + np.arange(n) // 64).astype(np.int32)
        add(f"c3_{thr}_grace", {"force": f, "code": _codes(n), "episode_length": ep}, thr=thr, variants=vs)

    # -- norm against a threshold, 2-vectors (the xy command); a foot has just landed, so feet_air_time is non-zero where its mask is --
    def landed(n):
        cct, last = rep("cur_contact", n), rep("last_air", n)
        cct[np.arange(n), np.arange(n) % 4] = np.float32(mc.DT)
        last[np.arange(n), np.arange(n) % 4] = np.float32(0.45)
        return {"cur_contact": cct, "last_air": last}

    for cthr in mc.CMD_THRESHOLDS:
        t32 = np.float32(cthr)
        rows = []
        for k in (-1, 0, 1):
            for axis in range(2):
                for sign in (1.0, -1.0):
                    c = np.zeros(3, dtype=np.float32)
                    c[axis] = np.float32(sign) * _ulps(t32, k)
                    rows.append(c)
        c = np.stack(rows)
        add(f"cmd_{cthr}_axis", dict(landed(len(c)), command=c))
        c = np.zeros((mc.N_ENVS, 3), dtype=np.float32)
        c[:, :2] = _oblique(rng, cthr, mc.N_ENVS, 2)
        add(f"cmd_{cthr}_oblique", dict(landed(len(c)), command=c))

    # -- bad_orientation about oblique axes: the ±600-step sweep of orientation_sweep.npz, axis (cos φ, sin φ, 0) -------------------------
    for ang in mc.LIMITS:
        vs = [k for k, v in enumerate(mc.VARIANTS) if v["limit"] == ang]
        thr = math.radians(ang) if ang < 82 else math.asin(0.99)
        base = np.float32(min(thr, math.asin(0.99)))
        tilt = base + np.arange(-600, 601, dtype=np.float64) * 2e-8
        for phi in mc.AXES_DEG:
            q = np.zeros((tilt.size, 4), dtype=np.float64)
            q[:, 0] = np.cos(tilt / 2)
            q[:, 1] = np.sin(tilt / 2) * math.cos(math.radians(phi))
            q[:, 2] = np.sin(tilt / 2) * math.sin(math.radians(phi))
            q32 = q.astype(np.float32)
            add(f"tilt_{ang}_{phi}", {"quat": q32, "episode_length": np.full(len(q32), mc.GRACE + 1, dtype=np.int32)}, limit=ang, variants=vs)
            if phi == 45.0:
                add(f"tilt_{ang}_grace", {"quat": q32[::5].copy(), "episode_length": np.full(len(q32[::5]), mc.GRACE, dtype=np.int32)},
                    limit=ang, variants=vs)

    # -- scalar decisions ----------------------------------------------------------------------------------------------------------------
    pos = rep("pos", 3)
    pos[:, 2] = [_ulps(mc.MIN_HEIGHT, k) for k in (-1, 0, 1)]
    add("height", {"pos": pos})
    x_min, x_max, y_min, y_max = mc.BOUNDS   # the bounds the reference's way (terminations.py:126-128): Python doubles
    edges = [(0, x_min + mc.BORDER_MARGIN), (0, x_max - mc.BORDER_MARGIN), (1, y_min + mc.BORDER_MARGIN), (1, y_max - mc.BORDER_MARGIN)]
    pos = rep("pos", 12)
    for e, (axis, bound) in enumerate(edges):
        for k in (-1, 0, 1):
            pos[3 * e + k + 1, axis] = _ulps(bound, k)
    add("bounds", {"pos": pos})
    mx = int(benign["max_episode_length"])
    add("timeout", {"episode_length": np.array([mx - 1, mx, mx + 1], dtype=np.int32)})
    # feet_air_time: current_contact_time around has_made_contact's two comparisons (> 0, < dt + 1e-8)
    edge = np.float32(mc.DT + 1.0e-8)
    vals = [np.float32(0.0), np.float32(1e-45), _ulps(mc.DT, -1), np.float32(mc.DT), _ulps(mc.DT, 1), _ulps(edge, -1), edge, _ulps(edge, 1)]
    n = 4 * len(vals)
    cct, last = rep("cur_contact", n), rep("last_air", n)
    cct[np.arange(n), np.arange(n) % 4] = np.repeat(np.array(vals, dtype=np.float32), 4)
    last[np.arange(n), np.arange(n) % 4] = np.float32(0.45)
    add("air_contact_time", {"cur_contact": cct, "last_air": last})
    # … last_air_time around the clamp (time_threshold_max - time_threshold), and below time_threshold (a negative term)
    vals = [_ulps(mc.AIR_THRESHOLD_MAX, k) for k in range(-8, 9)] + [np.float32(0.0), np.float32(0.1), _ulps(mc.AIR_THRESHOLD, -1),
                                                                    np.float32(mc.AIR_THRESHOLD), _ulps(mc.AIR_THRESHOLD, 1)]
    n = 4 * len(vals)
    cct, last = rep("cur_contact", n), rep("last_air", n)
    cct[np.arange(n), np.arange(n) % 4] = np.float32(mc.DT)
    last[np.arange(n), np.arange(n) % 4] = np.repeat(np.array(vals, dtype=np.float32), 4)
    add("air_last_air_time", {"cur_contact": cct, "last_air": last})
    return blocks


def gen_mask_edges():
    """tests/golden/mask_edges.npz: inputs and the reference's outputs of every block — per-term calls, one TerminationManager.step() +
    RewardManager.step() of the mask-term config, the air-time arrays after the feet manager's air-time update."""
    import types

    import mask_edges_cases as mc
    from genesis_forge import managers as ref_managers

    api = types.SimpleNamespace(ManagedEnvironment=ref.ManagedEnvironment, managers=ref_managers, scene=my_scene, reset=reset, rewards=rewards,
                                terminations=terminations, observations=observations)
    envs = []
    for k in range(len(mc.VARIANTS)):
        env = mc.make_env(api, k)
        env.build()
        envs.append(env)
    env0 = envs[0]
    default = env0.action_manager.default_dofs_pos.numpy().astype(np.float32).reshape(-1)[:12].copy()
    assert default[0] == 0.0
    dof_pos = default.copy()
    dof_pos[0] = 1.0   # sum |dof_pos - default| is exactly 1: stand_still's value is its mask
    links_vel = np.zeros((env0.robot.n_links, 3), dtype=np.float32)
    links_vel[:, 0] = 1.0   # every link moves at exactly 1: feet_slide's value is its count of feet in contact
    f4 = lambda x: np.full(4, x, dtype=np.float32)
    benign = dict(pos=np.array([0.0, 0.0, 0.4], np.float32), quat=np.array([1.0, 0.0, 0.0, 0.0], np.float32), lin_vel=np.zeros(3, np.float32),
                  ang_vel=np.zeros(3, np.float32), dof_pos=dof_pos, dof_vel=np.zeros(12, np.float32), links_vel=links_vel,
                  command=np.array([1.0, 0.0, 0.0], np.float32), episode_length=np.int32(500), max_episode_length=np.int32(1000),
                  last_air=f4(mc.AIR_START["last_air"]), cur_air=f4(mc.AIR_START["cur_air"]), last_contact=f4(mc.AIR_START["last_contact"]),
                  cur_contact=f4(mc.AIR_START["cur_contact"]))
    blocks = mask_edge_blocks(benign)
    names = list(blocks)
    counts = [next(iter(blocks[b]["arrays"].values())).shape[0] for b in names]
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    R = int(sum(counts))
    n_c3 = int(sum(c for b, c in zip(names, counts) if b.startswith("c3_")))
    assert all(b.startswith("c3_") for b in names[: sum(b.startswith("c3_") for b in names)]), "the contact blocks come first (mgr_air covers them)"
    V = len(mc.VARIANTS)
    out = {"blocks": np.array(names), "n_envs": np.int64(mc.N_ENVS), "block_start": starts, "block_n": np.array(counts, dtype=np.int64),
           "block_thr": np.array([blocks[b]["thr"] for b in names]), "block_limit": np.array([blocks[b]["limit"] for b in names]),
           "block_variants": np.array([[k in blocks[b]["variants"] for k in range(V)] for b in names])}
    out.update({f"benign_{k}": np.asarray(v) for k, v in benign.items()})
    for k in mc.ROW_KEYS:
        out[f"in_{k}"] = np.repeat(np.asarray(benign[k])[None], R, axis=0).copy()
    out["in_force"], out["in_code"] = np.zeros((R, mc.MAX_FORCES, 3), dtype=np.float32), np.zeros(R, dtype=np.int8)
    for b, s0, c in zip(names, starts, counts):
        for k, v in blocks[b]["arrays"].items():
            out[f"in_{k}"][s0:s0 + c] = v
    out["mgr_terminated"], out["mgr_truncated"] = np.zeros((V, R), dtype=np.bool_), np.zeros((V, R), dtype=np.bool_)
    out["mgr_reward"] = np.zeros((V, R), dtype=np.float32)
    out["mgr_air"] = np.zeros((V, 4, n_c3, 4), dtype=np.float32)
    to_t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    mask_rows, float_rows = {}, {}
    out["call_force_norm"] = np.zeros((R, mc.MAX_FORCES), dtype=np.float32)
    for b, s0, c in zip(names, starts, counts):
        rows = slice(int(s0), int(s0) + c)
        st = mc.block_state(out, rows)
        mc.load_state(env0, st, to_t)
        norms = {}
        for term, (kind, val) in mc.call_terms(api, env0, blocks[b]["thr"], blocks[b]["limit"]).items():
            v = val.detach().numpy()[:c]
            if kind == "mask":
                assert v.dtype == np.bool_ or np.all((v == 0) | (v == 1)), term
                mask_rows.setdefault(term, np.zeros(R, dtype=np.bool_))[rows] = v != 0
            elif kind == "float":
                float_rows.setdefault(term, np.zeros(R, dtype=np.float32))[rows] = v
            else:
                norms[term] = v
        # observations.contact_force is one norm per force vector: stored once, read where the largest link set had the forces placed —
        # and every link set's own output must be that, laid out like its contacts (what the tests rebuild)
        code, Lmax = out["in_code"][rows].astype(np.int64), max(mc.LINK_SETS)
        at = mc.link_index(code, Lmax)
        for j in range(mc.MAX_FORCES):
            out["call_force_norm"][rows, j] = norms[f"obs_contact_force_L{Lmax}"][np.arange(c), (at + j) % Lmax]
        for L in mc.LINK_SETS:
            rebuilt = mc.expand_contacts(out["call_force_norm"][rows][:, :, None], code, L)[:, :, 0]
            assert np.array_equal(rebuilt, norms[f"obs_contact_force_L{L}"]), (b, L)
        for k in blocks[b]["variants"]:
            env = envs[k]
            mc.load_state(env, st, to_t)
            env._extras = {env.extras_logging_key: {}}
            term, trunc = env.termination_manager.step()
            rew = env.reward_manager.step()
            out["mgr_terminated"][k, rows], out["mgr_truncated"][k, rows] = term.numpy()[:c], trunc.numpy()[:c]
            out["mgr_reward"][k, rows] = rew.detach().numpy()[:c]
            if b.startswith("c3_"):   # ContactManager.step's is_contact (contact_manager.py:444-477) on the feet, threshold = the variant's
                feet = env.cms[mc.FEET]
                feet._calculate_air_time()
                out["mgr_air"][k][:, rows] = np.stack([feet.last_air_time.numpy(), feet.current_air_time.numpy(), feet.last_contact_time.numpy(),
                                                       feet.current_contact_time.numpy()])[:, :c]
    out["call_mask_names"], out["call_mask"] = np.array(list(mask_rows)), np.stack(list(mask_rows.values()))
    out["call_float_names"], out["call_float"] = np.array(list(float_rows)), np.stack(list(float_rows.values()))
    # the sensitivity condition: rows where plain products summed left to right land on the other side of the recorded mask
    fx = mc.Fixture(_DictNpz(out))
    flips = {b: mc.sensitive_rows(fx, b) for b in names if b.endswith("_oblique")}
    for b, f in flips.items():
        assert f >= mc.MIN_SENSITIVE_ROWS, f"{b}: only {f} rows tell the two norm formulas apart"
    path = os.path.join(GOLD, "mask_edges.npz")
    out["in_quat_delta"] = mc.delta_rows(out.pop("in_quat"))   # (a sweep moves a few float32 steps per row: the differences compress 4x better)
    np.savez_compressed(path, **out)
    print("mask_edges:", len(blocks), "blocks,", R, "rows,", os.path.getsize(path), "bytes; rows the plain-product norm puts on the other side:", flips)


class _DictNpz:
    """A dict with the two things mask_edges_cases.Fixture asks of an NpzFile."""

    def __init__(self, d):
        self.d, self.files = d, list(d)

    def __getitem__(self, k):
        return self.d[k]


def gen_action():
    n = 65
    out = {}
    for cls, key in ((PositionActionManager, "position"), (PositionWithinLimitsActionManager, "within")):
        class E(ref.ManagedEnvironment):
            def __init__(self):
                super().__init__(num_envs=n, dt=1 / 50, max_episode_length_sec=20)
                self.scene = my_scene.SyntheticScene(dt=self.dt)
                self.terrain = self.scene.add_entity(my_scene.morphs.Plane())
                self.robot = self.scene.add_entity(my_scene.morphs.URDF(file="go2"))

            def config(self):
                if cls is PositionActionManager:
                    self.am = cls(self, joint_names=GO2_JOINTS, default_pos=GO2_DEFAULT, scale={".*_hip_joint": 0.5, ".*": 0.25},
                                  clip={".*_calf_joint": (-2.0, -1.0)}, quiet_action_errors=True)
                else:
                    self.am = cls(self, joint_names=GO2_JOINTS, default_pos=GO2_DEFAULT, quiet_action_errors=True)

        env = E()
        env.build()
        env.reset()
        rng = np.random.RandomState(3)
        acts, targets, env_actions, env_last, eplen = [], [], [], [], []
        for t in range(3):
            a = (3.0 * rng.standard_normal((n, 12))).astype(np.float32)
            if t == 1:
                a[0, 0], a[1, 1], a[2, 2], a[3, 3] = np.nan, np.inf, -np.inf, 1e30
            env.step(torch.from_numpy(a.copy()))
            acts.append(a)
            targets.append(env.am.get_actions().numpy().copy())
            env_actions.append(env.actions.numpy().copy())
            env_last.append(env.last_actions.numpy().copy())
            eplen.append(env.episode_length.numpy().copy())
        out.update({f"{key}_actions": np.stack(acts), f"{key}_targets": np.stack(targets), f"{key}_env_actions": np.stack(env_actions),
                    f"{key}_env_last": np.stack(env_last), f"{key}_episode_length": np.stack(eplen)})
    np.savez_compressed(os.path.join(GOLD, "action.npz"), **out)
    print("action: ok")


def gen_air_time():
    """ContactManager._calculate_air_time over a scripted contact sequence (contact_manager.py:434-477)."""
    n = 33
    env = RefGo2Env(n, contacts=True, obs_noise=False)
    env.build()
    cm_ = env.foot_contacts
    rng = np.random.RandomState(5)
    seq, states = [], []
    for t in range(14):
        c = (8.0 * rng.standard_normal((n, 4, 3)) * (rng.uniform(size=(n, 4, 1)) < 0.5)).astype(np.float32)
        cm_.contacts[:] = torch.from_numpy(c)
        cm_._calculate_air_time()
        seq.append(c)
        states.append(np.stack([cm_.last_air_time.numpy(), cm_.current_air_time.numpy(), cm_.last_contact_time.numpy(),
                                cm_.current_contact_time.numpy()]).copy())
        if t == 9:
            cm_.reset(torch.tensor([0, 5, 7]))
            states[-1] = np.stack([cm_.last_air_time.numpy(), cm_.current_air_time.numpy(), cm_.last_contact_time.numpy(),
                                   cm_.current_contact_time.numpy()]).copy()
    made = cm_.has_made_contact(env.dt).numpy()
    np.savez_compressed(os.path.join(GOLD, "air_time.npz"), contacts=np.stack(seq), states=np.stack(states), made_contact=made,
                        threshold=np.float32(5.0), dt=np.float64(env.scene.dt), reset_step=np.int64(9), reset_ids=np.array([0, 5, 7]))
    print("air_time: ok")


def gen_entity_obs():
    """utils.entity_* (utils.py:13-55), EntityManager getters (entity_manager.py:130-146,189-195) and every mdp.observations
    getter (observations.py:16-193) on a random state whose quaternions are deliberately NOT all unit length."""
    from genesis_forge import utils as rutils

    n = 97
    env = RefGo2Env(n, contacts=True, obs_noise=False)
    env.build()
    rng = np.random.RandomState(31)
    random_state(env, rng, n)
    q = env.robot.quat.clone()
    q[::3] *= torch.from_numpy(rng.uniform(0.9, 1.1, (len(q[::3]), 1)).astype(np.float32))   # non-unit rows
    env.robot.quat[:] = q
    env.robot.dof_force[:] = torch.from_numpy((30.0 * rng.standard_normal((n, 12))).astype(np.float32))
    for em in env.managers["entity"]:
        em.step()
    env.action_manager.step(torch.from_numpy(rng.standard_normal((n, 12)).astype(np.float32)))
    em, am, foot = env.robot_manager, env.action_manager, env.foot_contacts
    out = {"in_" + k: v for k, v in state_dict(env).items()}
    out["in_dof_force"] = env.robot.dof_force.numpy().copy()
    out["in_targets"] = am.get_actions().numpy().copy()
    O = {
        "utils_lin_vel": rutils.entity_lin_vel(env.robot), "utils_ang_vel": rutils.entity_ang_vel(env.robot),
        "utils_projected_gravity": rutils.entity_projected_gravity(env.robot),
        "em_lin_vel": em.get_linear_velocity(), "em_ang_vel": em.get_angular_velocity(), "em_projected_gravity": em.get_projected_gravity(),
        "obs_lin_vel_mgr": observations.entity_linear_velocity(env, entity_manager=em),
        "obs_lin_vel_attr": observations.entity_linear_velocity(env, entity_attr="robot"),
        "obs_ang_vel_mgr": observations.entity_angular_velocity(env, entity_manager=em),
        "obs_ang_vel_attr": observations.entity_angular_velocity(env, entity_attr="robot"),
        "obs_projected_gravity_mgr": observations.entity_projected_gravity(env, entity_manager=em),
        "obs_dofs_position_mgr": observations.entity_dofs_position(env, action_manager=am),
        "obs_dofs_position_idx": observations.entity_dofs_position(env, dofs_idx=[7, 9, 12]),
        "obs_dofs_velocity_mgr": observations.entity_dofs_velocity(env, action_manager=am),
        "obs_dofs_velocity_idx": observations.entity_dofs_velocity(env, dofs_idx=[6, 17]),
        "obs_dofs_force_mgr": observations.entity_dofs_force(env, action_manager=am),
        "obs_dofs_force_idx": observations.entity_dofs_force(env, dofs_idx=[8, 10]),
        "obs_current_actions_mgr": observations.current_actions(env, action_manager=am),
        "obs_contact_force": observations.contact_force(env, contact_manager=foot),
    }
    for k, v in O.items():
        out["out_" + k] = v.detach().numpy().astype(np.float32)
    np.savez_compressed(os.path.join(GOLD, "entity_obs.npz"), **out)
    print("entity_obs:", len(O), "outputs")


CONTACT_CASES = [  # ContactManager ctor kwargs of the contact-kernel fixture (tests/test_contact_kernel.py builds the same three)
    dict(link_names=[".*_foot"], track_air_time=True, air_time_contact_threshold=3.0),
    dict(link_names=[".*_thigh", "base"], with_entity_attr="terrain"),
    dict(link_names=[".*_calf"], with_links_names=[".*_foot", "base"], track_air_time=True, air_time_contact_threshold=1.0),
]


def check_ti_parallel(n=4096, C=9, T=5, NL=14):
    """The chunked execution of the Taichi kernel's emulation (tools/ref_stubs.py: ti_kernel, env chunks in forked workers) against the
    serial one on the same arbitrary contact arrays (both sides of a pair, NaN / Inf forces, a with-filter): bit for bit."""
    from genesis_forge.managers.contact.kernel import kernel_get_contact_forces

    rng = np.random.RandomState(5)
    la = rng.randint(-1, NL, (n, C)).astype(np.int32)
    lb = rng.randint(0, NL, (n, C)).astype(np.int32)
    f = (10.0 * rng.standard_normal((n, C, 3))).astype(np.float32)
    f[3, 1, 0], f[77, 2, 1], f[n - 1, 0, 2] = np.nan, np.inf, -np.inf
    pos = rng.standard_normal((n, C, 3)).astype(np.float32)
    q = rng.standard_normal((n, NL, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    targets, withs = torch.tensor([2, 5, 6, 9, 13], dtype=torch.int32)[:T], torch.tensor([0, 3], dtype=torch.int32)
    res = {}
    for jobs in ("1", "8"):
        os.environ["GF_TI_JOBS"] = jobs
        for filt in (0, 1):
            out_f, out_p, cnt = torch.zeros(n, T, 3), torch.zeros(n, T, 3), torch.zeros(n, T)
            kernel_get_contact_forces(torch.from_numpy(f), torch.from_numpy(pos), torch.from_numpy(la), torch.from_numpy(lb), torch.from_numpy(q),
                                      targets, withs, out_f, out_p, cnt, filt)
            res[(jobs, filt)] = (out_f.numpy().copy(), out_p.numpy().copy(), cnt.numpy().copy())
    os.environ.pop("GF_TI_JOBS")
    for filt in (0, 1):
        for a, b in zip(res[("1", filt)], res[("8", filt)]):
            assert np.array_equal(a, b, equal_nan=True), "chunked emulation differs from the serial one"
        assert np.abs(np.nan_to_num(res[("1", filt)][0])).sum() > 0
    print("check_ti_parallel: serial == chunked (8 workers) on", n, "envs, with and without the filter")


def gen_contact_kernel():
    """ContactManager.step (contact_manager.py:331-336,384-477 + the Taichi kernel contact/kernel.py:5-90, executed from the
    reference's own source under tools/ref_stubs.py's serial ndrange) on ARBITRARY contact arrays: both link_a and link_b range
    over every link of the scene (so the reaction-force branch `target == link_a` is exercised, which the synthetic scene never
    produces), forces contain NaN / ±Inf, and two of the three managers carry a with-filter (other entity / own links)."""
    n, C, steps = 37, 9, 6

    class E(ref.ManagedEnvironment):
        def __init__(self):
            super().__init__(num_envs=n, dt=1 / 50, max_episode_length_sec=20)
            self.scene = my_scene.SyntheticScene(dt=self.dt, max_collision_pairs=C)
            self.terrain = self.scene.add_entity(my_scene.morphs.Plane())
            self.robot = self.scene.add_entity(my_scene.morphs.URDF(file="go2"))

        def config(self):
            self.cms = [ContactManager(self, **kw) for kw in CONTACT_CASES]

    env = E()
    env.build()
    sc = env.scene
    NL = sc.links_quat.shape[1]
    rng = np.random.RandomState(23)
    out = {k: [] for k in ("force", "position", "link_a", "link_b", "links_quat")}
    res = {f"m{m}_{k}": [] for m in range(3) for k in ("contacts", "contact_positions")}
    air = {f"m{m}_air": [] for m in (0, 2)}
    for t in range(steps):
        la = rng.randint(-1, NL, (n, C)).astype(np.int32)
        lb = rng.randint(0, NL, (n, C)).astype(np.int32)
        empty = rng.uniform(size=(n, C)) < 0.35
        la[empty], lb[empty] = -1, -1
        f = (10.0 * rng.standard_normal((n, C, 3))).astype(np.float32)
        f[empty] = 0.0
        if t == 2:
            f[1, 0, 0], f[2, 1, 1], f[3, 2, 2] = np.nan, np.inf, -np.inf
            la[1, 0], lb[1, 0] = 0, 5
            la[2, 1], lb[2, 1] = 0, 3
            la[3, 2], lb[3, 2] = 8, 4
        pos = rng.standard_normal((n, C, 3)).astype(np.float32)
        q = rng.standard_normal((n, NL, 4)).astype(np.float32)
        q /= np.linalg.norm(q, axis=-1, keepdims=True)
        sc.contact_force[:], sc.contact_pos[:] = torch.from_numpy(f), torch.from_numpy(pos)
        sc.link_a[:], sc.link_b[:] = torch.from_numpy(la), torch.from_numpy(lb)
        sc.links_quat[:] = torch.from_numpy(q.astype(np.float32))
        for k, v in (("force", f), ("position", pos), ("link_a", la), ("link_b", lb), ("links_quat", q.astype(np.float32))):
            out[k].append(v)
        for m, cm_ in enumerate(env.cms):
            cm_.step()
            res[f"m{m}_contacts"].append(cm_.contacts.numpy().copy())
            res[f"m{m}_contact_positions"].append(cm_.contact_positions.numpy().copy())
            if cm_.last_air_time is not None:
                air[f"m{m}_air"].append(np.stack([cm_.last_air_time.numpy(), cm_.current_air_time.numpy(), cm_.last_contact_time.numpy(),
                                                  cm_.current_contact_time.numpy()]).copy())
    data = {k: np.stack(v) for k, v in {**out, **res, **air}.items()}
    data.update(n=np.int64(n), C=np.int64(C), steps=np.int64(steps), cases=np.array(repr(CONTACT_CASES)))
    np.savez_compressed(os.path.join(GOLD, "contact_kernel.npz"), **data)
    print("contact_kernel: ok, nonzero force rows per manager", [int((np.abs(data[f"m{m}_contacts"]).sum(-1) > 0).sum()) for m in range(3)])


def gen_contact_edges():
    """The reference's Taichi kernel (contact/kernel.py:5-90, executed from its own source on arrays, as check_ti_parallel does) on ONE
    case with more than 64 contact slots per env — three occupancy-mask words in gf_contact_tile.h — that holds what the
    contact_kernel fixture lacks: self-contacts (link_a == link_b == a tracked link), slots with exactly one side -1, slots with both
    sides -1, and NaN / +-Inf force components, with and without a with-filter.  The kernel gets the forces as ContactManager hands
    them over (contact_manager.py:399-403: non-finite components replaced by 0); the fixture keeps the raw ones."""
    from genesis_forge.managers.contact.kernel import kernel_get_contact_forces

    n, C, NL = 24, 130, 20
    rng = np.random.RandomState(131)
    targets, withs = [2, 5, 6, 9, 13, 19], [0, 5, 13, 7]
    la = rng.randint(-1, NL, (n, C)).astype(np.int32)
    lb = rng.randint(-1, NL, (n, C)).astype(np.int32)
    empty = rng.uniform(size=(n, C)) < 0.4
    la[empty], lb[empty] = -1, -1
    self_c = rng.uniform(size=(n, C)) < 0.06   # self-contacts, of tracked and of untracked links
    lb[self_c] = la[self_c]
    for e, c, t in ((0, 0, 2), (1, 31, 5), (2, 32, 6), (3, 63, 9), (4, 64, 13), (5, 95, 19), (6, 96, 5), (7, 129, 13)):   # at the word boundaries too
        la[e, c], lb[e, c] = t, t
    f = (10.0 * rng.standard_normal((n, C, 3))).astype(np.float32)
    for e, c, j, v, a, b in ((8, 5, 0, np.nan, 5, 13), (9, 70, 1, np.inf, 0, 2), (10, 129, 2, -np.inf, 13, 13), (11, 64, 0, np.nan, -1, 6)):
        f[e, c, j], la[e, c], lb[e, c] = v, a, b
    f[12, 3, 1], la[12, 3], lb[12, 3] = np.nan, -1, -1   # (a non-finite force in a slot nobody includes)
    pos = rng.standard_normal((n, C, 3)).astype(np.float32)
    q = rng.standard_normal((n, NL, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    assert ((la == lb) & np.isin(la, targets)).sum() >= 8 and ((la < 0) ^ (lb < 0)).sum() > 100 and ((la < 0) & (lb < 0)).sum() > 100
    clean = torch.nan_to_num(torch.from_numpy(f), nan=0.0, posinf=0.0, neginf=0.0)
    data = dict(force=f, position=pos, link_a=la, link_b=lb, links_quat=q, targets=np.array(targets, np.int32), withs=np.array(withs, np.int32))
    T = len(targets)
    for filt in (0, 1):
        out_f, out_p, cnt = torch.zeros(n, T, 3), torch.zeros(n, T, 3), torch.zeros(n, T)
        kernel_get_contact_forces(clean, torch.from_numpy(pos), torch.from_numpy(la), torch.from_numpy(lb), torch.from_numpy(q),
                                  torch.tensor(targets, dtype=torch.int32), torch.tensor(withs, dtype=torch.int32), out_f, out_p, cnt, filt)
        data[f"f{filt}_contacts"], data[f"f{filt}_contact_positions"], data[f"f{filt}_counts"] = out_f.numpy().copy(), out_p.numpy().copy(), cnt.numpy().copy()
    np.savez_compressed(os.path.join(GOLD, "contact_edges.npz"), **data)
    print("contact_edges: ok, matched slots per link at most", [int(data[f"f{k}_counts"].max()) for k in (0, 1)])


def gen_terrain():
    """TerrainManager on a 2x2 height-field terrain: get_terrain_height at in-range, edge and out-of-range points
    (terrain_manager.py:100-166), bounds / subterrain bounds (:281-343) and generate_random_positions with given draws (:168-248)."""
    n = 64
    tk = dict(pos=(-3.0, 1.5, 0.25), n_subterrains=(2, 2), subterrain_size=(6.0, 5.0), horizontal_scale=0.25, vertical_scale=0.005,
              subterrain_types=[["flat_terrain", "random_uniform_terrain"], ["pyramid_stairs_terrain", "discrete_obstacles_terrain"]],
              subterrain_parameters={"random_uniform_terrain": {"min_height": -0.05, "max_height": 0.2},
                                     "pyramid_stairs_terrain": {"min_height": 0.0, "max_height": 0.4},
                                     "discrete_obstacles_terrain": {"min_height": -0.1, "max_height": 0.1}})
    env = RefGo2RoughEnv(n, scene_kwargs=dict(seed=77), terrain_kwargs=tk)
    install_contexts(env, Draws(n, 3, 48))
    env.build()
    tm = env.terrain_manager
    rng = np.random.RandomState(11)
    xs = np.concatenate([rng.uniform(-3.0, 9.0, 40), [-3.0, 9.0, -3.0, 9.0, -4.0, 10.5, 2.999, 3.0, 3.001, 0.0, 8.99999, -2.99999],
                         rng.uniform(-6.0, 12.0, 12)]).astype(np.float32)
    ys = np.concatenate([rng.uniform(1.5, 11.5, 40), [1.5, 11.5, 11.5, 1.5, 0.0, 13.0, 6.499, 6.5, 6.501, 5.0, 11.49999, 1.50001],
                         rng.uniform(-1.0, 14.0, 12)]).astype(np.float32)
    assert len(xs) == n
    heights = tm.get_terrain_height(torch.from_numpy(xs), torch.from_numpy(ys)).numpy().copy()
    out = dict(height_field=env.terrain.geoms[0].metadata["height_field"], terrain_kwargs=np.array(repr(tk)), x=xs, y=ys, heights=heights,
               bounds=np.array(tm.get_bounds(), dtype=np.float64), n=np.int64(n), seed=np.int64(SEED))
    names = [name for row in tk["subterrain_types"] for name in row]
    out["sub_names"] = np.array(names)
    out["sub_bounds"] = np.array([tm.get_bounds(s) for s in names], dtype=np.float64)
    cases = [(0.5, None, 0.1e-3), (0.25, "random_uniform_terrain", 0.3), (0.9, "discrete_obstacles_terrain", 0.0), (1.0, "pyramid_stairs_terrain", 0.05)]
    for k, (ratio, sub, off) in enumerate(cases):
        u = philox.draws(SEED, 100 + k, 4, n, 5)
        CTX.update(mode="spawn", ids=np.arange(n), i=0, axes=[], u=u)
        pos = tm.generate_random_positions(num=n, usable_ratio=ratio, subterrain=sub, height_offset=off).numpy().copy()
        CTX["mode"] = None
        out[f"spawn{k}_pos"] = pos
        out[f"spawn{k}_cfg"] = np.array(repr((ratio, sub, off)))
    # the flat case: no height field -> the origin's z
    np.savez_compressed(os.path.join(GOLD, "terrain.npz"), **out)
    print("terrain: ok, heights", float(heights.min()), float(heights.max()))


# ------------------------------------------------------------------------------------------------
# The reference's own example task configs (examples/*/environment.py), run UNCHANGED on the reference package
# ------------------------------------------------------------------------------------------------
def load_example_class(name, base_cls):
    """Execute /root/reference/examples/<name>/environment.py (against whatever ``genesis_forge`` / ``genesis`` are in
    sys.modules) and return its ManagedEnvironment subclass."""
    import importlib.util

    d = os.path.join("/root/reference/examples", name)
    sys.path.insert(0, d)
    for stale in ("environment", "gait_command_manager"):
        sys.modules.pop(stale, None)
    try:
        spec = importlib.util.spec_from_file_location("environment", os.path.join(d, "environment.py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules["environment"] = m
        spec.loader.exec_module(m)
    finally:
        sys.path.remove(d)
    cls = [v for v in vars(m).values() if isinstance(v, type) and issubclass(v, base_cls) and v is not base_cls]
    assert len(cls) == 1, cls
    return cls[0], m


def command_managers(env):
    """(attribute name, manager) of every command manager, in registration order."""
    out = []
    for m in env.managers["command"]:
        names = [k for k, v in vars(env).items() if v is m]
        out.append((names[0] if names else f"command{len(out)}", m))
    return out


GAIT_FIELDS = ("foot_offset", "foot_height", "gait_period", "gait_time", "gait_phase", "clock_input", "_gait_selected")


def record_step(env, rec, obs, rew, term, trunc, extras):
    f = lambda t: t.detach().cpu().numpy().copy()
    rec["obs"].append(f(obs))
    rec["reward"].append(f(rew))
    rec["terminated"].append(f(term))
    rec["truncated"].append(f(trunc))
    rec["episode_length"].append(f(env.episode_length))
    rec["max_episode_length"].append(f(env.max_episode_length))
    rec["pos"].append(f(env.robot.get_pos()))
    rec["quat"].append(f(env.robot.get_quat()))
    for k, (_, m) in enumerate(command_managers(env)):
        rec.setdefault(f"command{k}", []).append(f(m.command))
    for name, o in extras["observations"].items():
        if name != "policy":
            rec.setdefault("obs_" + name, []).append(f(o))
    g = getattr(env, "gait_command_manager", None)
    if g is not None:
        for fld in GAIT_FIELDS:
            rec.setdefault("gait_" + fld.lstrip("_"), []).append(f(getattr(g, fld)))


def run_example(name):
    import example_cases
    import gait_rng
    from genesis_forge_amd import compat

    case = example_cases.CASES[name]
    n, steps = case["n"], case["steps"]
    torch.manual_seed(0)
    compat.SCENE_OVERRIDES.clear()
    compat.SCENE_OVERRIDES.update(case["scene"])
    try:
        cls, mod = load_example_class(example_cases.example_of(name), ref.ManagedEnvironment)
        env = cls(num_envs=n, max_episode_length_s=case["episode_s"])
    finally:
        compat.SCENE_OVERRIDES.clear()
    draws = Draws(n, 3, 0)
    install_contexts(env, draws)
    if hasattr(mod, "GaitCommandManager"):
        gait_rng.install(mod.GaitCommandManager, lambda mgr, phase: draws.get(5 if phase == "step" else 6, 3))
    draws.step = 0
    env.build()
    for attr, sec in case["resample"].items():
        getattr(env, attr).resample_time_sec = sec
    obs0, _ = env.reset()
    rng = np.random.RandomState(7)
    rec = {k: [] for k in ("actions", "obs", "reward", "terminated", "truncated", "episode_length", "max_episode_length", "pos", "quat")}
    logs = []
    for t in range(steps):
        if t in case["events"]:
            example_cases.apply_event(env, case["events"][t])
        draws.step = t + 1
        act = rng.standard_normal((n, case["dofs"])).astype(np.float32)
        if t == 5:
            act[0, 0] = 1e9  # clip path
        obs, rew, term, trunc, extras = env.step(torch.from_numpy(act))
        rec["actions"].append(act)
        record_step(env, rec, obs, rew, term, trunc, extras)
        logs.append(episode_scalars(extras))
    keys = sorted({k for d in logs for k in d})
    log_arr = np.full((steps, len(keys)), np.nan, dtype=np.float64)
    for t, d in enumerate(logs):
        for j, k in enumerate(keys):
            if k in d:
                log_arr[t, j] = d[k]
    out = {k: np.stack(v) for k, v in rec.items()}
    out.update(obs0=obs0.numpy().copy(), log_keys=np.array(keys), log_values=log_arr, seed=np.int64(SEED), example=np.array(name))
    if case.get("compact"):   # (a size whose full trajectory would be hundreds of MB: sums + a strided sample, tests/helpers.py)
        import helpers
        assert np.array_equal(out["actions"], helpers.example_actions(case)), "the tests regenerate the actions from the same stream"
        np.savez_compressed(os.path.join(GOLD, f"traj_ex_{name}.npz"), **helpers.compact_example(out, n))
    else:
        np.savez_compressed(os.path.join(GOLD, f"traj_ex_{name}.npz"), **out)
    print(f"traj_ex_{name}: steps", steps, "obs", out["obs"].shape[1:], "terminated", int(out["terminated"].sum()), "truncated",
          int(out["truncated"].sum()), "log keys", len(keys))


if __name__ == "__main__":
    os.makedirs(GOLD, exist_ok=True)
    if len(sys.argv) > 1 and sys.argv[1] == "entity_obs":
        gen_entity_obs()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "contact_kernel":
        gen_contact_kernel()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "contact_edges":
        gen_contact_edges()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "mask_edges":
        gen_mask_edges()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "at_size":
        gen_at_size()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "check_ti_parallel":
        check_ti_parallel()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "check_at_size":
        check_at_size(int(sys.argv[2]), contacts=len(sys.argv) > 3 and sys.argv[3] == "contacts")
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "examples":
        import example_cases
        for ex in (sys.argv[2:] or [k for k, c in example_cases.CASES.items() if not c.get("compact")]):   # (compact cases — minutes of reference time — by name)
            run_example(ex)
        sys.exit(0)
    gen_terrain()
    gen_contact_kernel()
    gen_contact_edges()
    gen_entity_obs()
    run_trajectory("traj_go2_rough", n=16, steps=170, contacts=False, history=None, episode_s=1.5, variant="rough",
                   scene_kwargs=dict(ang_noise=0.4, lin_noise=0.05, seed=41, contact_prob=0.3, contact_force=30.0))
    gen_terms()
    gen_orientation_sweep()
    gen_action()
    gen_air_time()
    run_trajectory("traj_go2_cmd", n=12, steps=260, contacts=False, history=None,
                   scene_kwargs=dict(ang_noise=0.35, lin_noise=0.05, seed=99))
    run_trajectory("traj_go2_contacts_hist", n=10, steps=160, contacts=True, history=3,
                   scene_kwargs=dict(ang_noise=0.3, lin_noise=0.05, seed=5, contact_prob=0.3, contact_force=30.0))
