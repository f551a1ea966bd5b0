"""Host-side logic of the operator interface (no kernels beyond the oracle backend)."""
import os
import math

import numpy as np
import pytest
import torch

from envs import Go2CommandDirectionEnv


def test_manager_registration_rules(oracle_backend):
    from genesis_forge_amd.managers import RewardManager

    env = Go2CommandDirectionEnv(num_envs=4)
    env.build()
    with pytest.raises(ValueError, match="already has a manager"):
        RewardManager(env, cfg={})
    with pytest.raises(ValueError, match="not a valid manager type"):
        env.add_manager("bogus", object())
    assert env.action_space.shape == (12,) and env.observation_space.shape == (48,)
    assert env.managers["action"].dofs_idx == list(range(6, 18))


def test_dof_value_patterns(oracle_backend):
    env = Go2CommandDirectionEnv(num_envs=4)
    env.build()
    am = env.action_manager
    d = am.default_dofs_pos[0].tolist()
    assert d == pytest.approx([0.0, 0.8, -1.5, 0.0, 0.8, -1.5, 0.0, 1.0, -1.5, 0.0, 1.0, -1.5])
    with pytest.raises(RuntimeError, match="not found"):
        am._get_dof_value_array({"no_such_joint": 1.0})
    # first matching pattern wins (position_action_manager.py:487-499)
    assert am._get_dof_value_array({"FL_.*": 2.0, ".*": 1.0})[:4] == [2.0, 2.0, 2.0, 1.0]


def test_command_range_setter_validation(oracle_backend):
    env = Go2CommandDirectionEnv(num_envs=4)
    env.build()
    vc = env.velocity_command
    with pytest.raises(ValueError):
        vc.range = {"lin_vel_x": [0, 1]}
    with pytest.raises(ValueError):
        vc.range = (0, 1)
    vc.range = {"lin_vel_x": [0, 2], "lin_vel_y": [0, 0], "ang_vel_z": [-1, 1]}
    assert vc._resample_steps == int(5.0 / env.dt) == 250


def test_lazy_episode_log_semantics():
    from genesis_forge_amd._stats import LazyEpisodeLog

    calls = []

    class Snap:
        def wait(self):
            calls.append("wait")
            return "stats"

    log = LazyEpisodeLog()
    log.add_filler(lambda st, out: out.update(a=1.0, b=2.0))
    log["b"] = 5.0            # user-written key wins and does not materialise
    assert calls == []
    log.attach(Snap())
    assert "a" in log and log["b"] == 5.0 and calls == ["wait"]
    assert dict(log) == {"a": 1.0, "b": 5.0} and len(log) == 2
    assert list(log.keys()) == ["b", "a"] and calls == ["wait"]


def test_tilt_threshold_matches_torch_asin():
    from genesis_forge_amd.mdp.terminations import tilt_threshold_sin

    rng = np.random.RandomState(0)
    for limit in (0.0, 5.0, 10.0, 20.0, 30.0, 40.0, 60.0, 81.0, 82.0, 90.0, -3.0):
        x_thr, thr = tilt_threshold_sin(limit)
        x = torch.from_numpy(np.concatenate([rng.uniform(0, 1.2, 20000), [0.0, 0.99, 1.0, x_thr]]).astype(np.float32))
        near = torch.tensor(x_thr, dtype=torch.float32).view(torch.int32) + torch.arange(-50, 51, dtype=torch.int32)
        x = torch.cat([x, near.view(torch.float32)])
        x = x[(x >= 0) & torch.isfinite(x)]
        want = torch.asin(torch.clamp(x, max=0.99)) > math.radians(limit)
        got = torch.clamp(x, max=0.99) > x_thr
        assert torch.equal(want, got), f"limit {limit}: {int((want != got).sum())} mismatches"


def test_opaque_terms_run_as_external_columns(oracle_backend):
    """Lambdas / user callables keep working: evaluated by Python, folded in by the kernel."""
    from genesis_forge_amd import _native as nat
    from genesis_forge_amd.managers import RewardManager, TerminationManager
    from genesis_forge_amd.mdp import rewards

    class Env(Go2CommandDirectionEnv):
        def config(self):
            super().config()
            self.managers["reward"] = None
            self.managers["termination"] = None
            self.rm = RewardManager(self, cfg={
                "lib": {"weight": 2.0, "fn": rewards.lin_vel_z_l2, "params": {"entity_manager": self.robot_manager}},
                "opaque": {"weight": -1.5, "fn": lambda env, k: env.robot.get_pos()[:, 2] * k, "params": {"k": 3.0}},
                "bound": {"weight": 0.5, "fn": self.custom_term},
            })
            self.tm = TerminationManager(self, term_cfg={
                "opaque": {"fn": lambda env: env.robot.get_pos()[:, 2] > 0.41},
            })

        def custom_term(self, env):
            return rewards.action_rate_l2(env) + 1.0

    env = Env(num_envs=33, scene_kwargs=dict(lin_noise=0.3))
    env.build()
    env.reset()
    for _ in range(5):
        _, rew, term, _, _ = env.step(torch.randn(33, 12))
    # the terminal step's reward is computed before the reset (quirk q6), from the pre-reset state: recompute it
    # … and the step is still recorded: cut in front of the termination op and in front of the reward op, where the callables run
    # (custom_term even launches a native phase of its own, which belongs to the callable, not to the recording)
    assert env._trace is not None and [i for i, _ in env._trace.splits] == sorted(i for i, _ in env._trace.splits) and len(env._trace.splits) == 2
    ops = [env.rm._program.args.terms[k].op for k in range(3)]
    assert ops == [nat.GF_R_LIN_VEL_Z_L2, nat.GF_R_EXTERNAL, nat.GF_R_EXTERNAL]
    assert env.tm._program.args.terms[0].op == nat.GF_T_EXTERNAL
    assert term.dtype == torch.bool and rew.shape == (33,)
    w = env.rm.cfg["opaque"].weight * env.dt
    assert np.float32(w) == np.float32(-1.5 * 0.02)


def test_fused_and_unfused_observations_agree(oracle_backend):
    outs = []
    for fused in (True, False):
        env = Go2CommandDirectionEnv(num_envs=40, fused_obs=fused, obs_noise=True, max_episode_length_s=1, scene_kwargs=dict(ang_noise=0.3))
        env.build()
        env.seed(9)
        env.reset()
        g = torch.Generator().manual_seed(1)
        seq = []
        for _ in range(30):
            obs, *_ = env.step(torch.randn(40, 12, generator=g))
            seq.append(obs.clone())
        outs.append(torch.stack(seq))
        ops = {env.observation_manager._args.items[k].op for k in range(7)}
        assert (11 in ops) == (not fused)  # GF_O_EXTERNAL only on the unfused path
    assert torch.equal(outs[0], outs[1])


def test_runs_reference_style_config_through_alias(oracle_backend):
    import sys

    import genesis_forge_amd

    genesis_forge_amd.install_as_genesis_forge()
    try:
        import genesis as gs_mod
        from genesis_forge import ManagedEnvironment
        from genesis_forge.managers import EntityManager, PositionActionManager, RewardManager, TerminationManager
        from genesis_forge.mdp import reset, rewards, terminations

        class Env(ManagedEnvironment):
            def __init__(self):
                super().__init__(num_envs=8, dt=1 / 50, max_episode_length_sec=20)
                self.scene = gs_mod.Scene(show_viewer=False, sim_options=gs_mod.options.SimOptions(dt=self.dt, substeps=2),
                                          rigid_options=gs_mod.options.RigidOptions(dt=self.dt, max_collision_pairs=30))
                self.terrain = self.scene.add_entity(gs_mod.morphs.Plane())
                self.robot = self.scene.add_entity(gs_mod.morphs.URDF(file="urdf/go2/urdf/go2.urdf", pos=[0, 0, 0.4], quat=[1, 0, 0, 0]))

            def config(self):
                self.rmgr = EntityManager(self, entity_attr="robot", on_reset={"position": {"fn": reset.position, "params": {
                    "position": [0, 0, 0.4], "quat": [1, 0, 0, 0], "zero_velocity": True}}})
                self.am = PositionActionManager(self, joint_names=[".*_joint"], default_pos={".*": 0.0}, scale=0.25)
                RewardManager(self, cfg={"h": {"weight": -50.0, "fn": rewards.base_height, "params": {"target_height": 0.3}}})
                TerminationManager(self, term_cfg={"timeout": {"fn": terminations.timeout, "time_out": True}})

        env = Env()
        env.build()
        env.reset()
        _, rew, *_ = env.step(torch.zeros(8, 12))
        assert rew.shape == (8,) and float(rew[0]) == pytest.approx(-50.0 * 0.02 * (0.4 - 0.3) ** 2, abs=1e-3)
    finally:
        for k in [k for k in sys.modules if k == "genesis" or k.startswith("genesis_forge.") or k == "genesis_forge"]:
            del sys.modules[k]


def test_on_reset_helpers_follow_the_reference_code(oracle_backend):
    """mdp.reset.set_rotation / randomize_link_mass_shift / zero_all_dofs_velocity as EntityManager on_reset entries
    (reset.py:22-64,229-284), including what the reference's code actually does with scalar angles and the mass buffer."""
    from genesis_forge_amd import ManagedEnvironment
    from genesis_forge_amd.managers import EntityManager, PositionActionManager, TerminationManager
    from genesis_forge_amd.mdp import reset, terminations
    from genesis_forge_amd.scene import SyntheticScene, morphs

    class Env(ManagedEnvironment):
        def __init__(self):
            super().__init__(num_envs=6, dt=1 / 50, max_episode_length_sec=20)
            self.scene = SyntheticScene(dt=self.dt)
            self.terrain = self.scene.add_entity(morphs.Plane())
            self.robot = self.scene.add_entity(morphs.URDF(file="go2"))

        def config(self):
            self.em = EntityManager(self, entity_attr="robot", on_reset={
                "still": {"fn": reset.zero_all_dofs_velocity},
                "turn": {"fn": reset.set_rotation, "params": {"x": 0.5, "z": (0.25, 0.25)}},
                "mass": {"fn": reset.randomize_link_mass_shift, "params": {"link_name": ".*_foot", "add_mass_range": (-0.1, 0.1)}},
            })
            PositionActionManager(self, joint_names=[".*_joint"], default_pos={".*": 0.0})
            TerminationManager(self, term_cfg={"timeout": {"fn": terminations.timeout, "time_out": True}})

    env = Env()
    env.build()
    env.robot.lin_vel[:] = 1.0
    env.reset(torch.tensor([1, 4]))
    q = env.robot.get_quat()
    # only the tuple axis is applied (z = 0.25 rad); the scalar x = 0.5 is ignored exactly as in reset.py:52-58
    want = torch.tensor([math.cos(0.125), 0.0, 0.0, math.sin(0.125)])
    assert torch.allclose(q[1], want, atol=1e-6) and torch.allclose(q[4], want, atol=1e-6)
    assert torch.equal(q[0], torch.tensor([1.0, 0.0, 0.0, 0.0]))
    assert torch.all(env.robot.lin_vel[[1, 4]] == 0) and torch.all(env.robot.lin_vel[[0, 2, 3, 5]] == 1.0)
    shift = env.robot.gains["mass_shift"]
    assert shift.shape == (6, 4) and torch.all(shift == 0), "the reference hands its whole, still-zero buffer to set_mass_shift"


def test_rl_library_wrappers_over_the_recorded_step(oracle_backend):
    """An rsl_rl / skrl rollout loop through the wrappers (genesis_forge/wrappers/rsl_rl.py:11-119, skrl.py:36-54): dones =
    terminated | truncated, time-outs and the critic observation in extras, [N,1] shapes for skrl — identical whether the wrapped
    env replays a recorded step or runs phase by phase."""
    from genesis_forge_amd.wrappers import RslRlWrapper, SkrlEnvWapper

    def rollout(wrapper_cls, trace):
        env = Go2CommandDirectionEnv(num_envs=33, max_episode_length_s=0.5, cmd_resample_s=0.2, scene_kwargs=dict(ang_noise=0.3, seed=4))
        env.trace_enabled = trace
        w = wrapper_cls(env)
        w.build()
        env.seed(3)
        out = [w.reset()[0].clone()]
        if wrapper_cls is RslRlWrapper:
            obs, extras = w.get_observations()
            assert torch.equal(obs, out[0]) and "observations" in extras
        g = torch.Generator().manual_seed(1)
        for _ in range(40):
            res = w.step(torch.randn(33, 12, generator=g))
            out.append([x.clone() if isinstance(x, torch.Tensor) else x for x in res[:-1]] + [res[-1]["time_outs"].clone()])
        return out, env, res

    for cls in (RslRlWrapper, SkrlEnvWapper):
        a, _, _ = rollout(cls, False)
        b, env, last = rollout(cls, True)
        assert env._trace is not None
        assert torch.equal(a[0], b[0])
        for t, (x, y) in enumerate(zip(a[1:], b[1:])):
            for k, (u, v) in enumerate(zip(x, y)):
                assert torch.equal(u, v), f"{cls.__name__}: output {k} differs at step {t}"
        if cls is RslRlWrapper:
            obs, rew, dones, extras = last
            assert dones.dtype == torch.bool and torch.equal(dones, env.termination_manager._terminated_buf | env.termination_manager._truncated_buf)
            assert torch.equal(extras["observations"]["critic"], obs) and torch.equal(extras["time_outs"], env.termination_manager._truncated_buf)
            assert any(step[2].any() for step in b[1:]), "no env was ever done: nothing about dones was checked"
        else:
            obs, rew, term, trunc, extras = last
            assert rew.shape == (33, 1) and term.shape == (33, 1) and trunc.shape == (33, 1)


def test_rsl_rl_3_wrapper_returns_observation_groups_as_a_tensordict(oracle_backend, monkeypatch):
    """With rsl-rl-lib >= 3 the wrapper hands out the env's observation groups as a TensorDict and get_observations() returns the
    observations only (rsl_rl.py:24-34, 66-119).  Neither package is in this image: the version probe and a minimal ``tensordict``
    module are stood in."""
    import sys
    import types
    from importlib import metadata

    from genesis_forge_amd.wrappers import RslRlWrapper

    class TensorDict(dict):
        def __init__(self, data, batch_size=None, device=None):
            super().__init__(data)
            self.batch_size, self.device = batch_size, device

    monkeypatch.setitem(sys.modules, "tensordict", types.SimpleNamespace(TensorDict=TensorDict))
    real = metadata.version
    monkeypatch.setattr(metadata, "version", lambda name: "3.1.0" if name == "rsl-rl-lib" else real(name))
    env = Go2CommandDirectionEnv(num_envs=9, scene_kwargs=dict(seed=4))
    w = RslRlWrapper(env)
    assert w.rsl3 and str(w.device) == "cpu"
    w.build()
    obs, extras = w.reset()
    assert isinstance(obs, TensorDict) and set(obs) >= {"policy"} and obs["policy"].shape[0] == 9
    got = w.get_observations()
    assert isinstance(got, TensorDict) and torch.equal(got["policy"], obs["policy"])
    obs2, rew, dones, extras = w.step(torch.zeros(9, 12))
    assert isinstance(obs2, TensorDict) and "critic" in obs2 and torch.equal(obs2["critic"], obs2["policy"])
    assert dones.dtype == torch.bool and torch.equal(extras["time_outs"], env.termination_manager._truncated_buf)
    monkeypatch.setattr(metadata, "version", lambda name: "2.3.1" if name == "rsl-rl-lib" else real(name))
    w2 = RslRlWrapper(env)
    assert not w2.rsl3 and isinstance(w2.get_observations(), tuple) and isinstance(w2.step(torch.zeros(9, 12))[0], torch.Tensor)


def test_video_wrapper_drives_the_camera_and_passes_through_without_one(oracle_backend, tmp_path):
    """wrappers/video.py:90-260: a triggered recording of video_length_sec saved as <start step>.mp4, frames every steps_per_frame steps,
    a background recording between triggers, the final one saved on close; an env without a camera is passed through with a warning."""
    import warnings

    from genesis_forge_amd.wrappers import RslRlWrapper, VideoWrapper, capped_cubic_episode_trigger

    assert [e for e in range(30) if capped_cubic_episode_trigger(e)] == [0, 1, 8, 27] and capped_cubic_episode_trigger(2000) and not capped_cubic_episode_trigger(1001)

    class Cam:
        def __init__(self):
            self.calls, self._recorded_imgs = [], []

        def start_recording(self): self.calls.append("start")
        def pause_recording(self): self.calls.append("pause")
        def render(self): self.calls.append("render")
        def stop_recording(self, path, fps=None): self.calls.append(("stop", os.path.basename(path), fps))

    env = Go2CommandDirectionEnv(num_envs=5, max_episode_length_s=0.2, scene_kwargs=dict(seed=4))   # 10-step episodes at dt = 0.02
    env.camera = Cam()
    w = VideoWrapper(env, video_length_sec=0.1, out_dir=str(tmp_path / "videos"), step_trigger=lambda step: step % 12 == 0, fps=25)
    assert w.video_length_steps == 5 and w.num_envs == 5
    r = RslRlWrapper(w)
    r.build()
    r.reset()
    for _ in range(30):
        obs, rew, dones, extras = r.step(torch.zeros(5, 12))
    r.close()
    calls = env.camera.calls
    stops = [c for c in calls if isinstance(c, tuple)]
    assert [c[1] for c in stops[:3]] == ["0.mp4", "12.mp4", "24.mp4"] and all(c[2] == 25 for c in stops)
    assert calls.count("render") == 15 and calls.count("start") >= 3 and os.path.isdir(tmp_path / "videos")

    plain = Go2CommandDirectionEnv(num_envs=5, scene_kwargs=dict(seed=4))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        v = VideoWrapper(plain, out_dir=str(tmp_path / "none"))
        v.build()
    assert any("not a camera" in str(x.message) for x in caught)
    v.reset()
    out = v.step(torch.zeros(5, 12))
    assert len(out) == 5
    v.close()


def test_external_command_controller(oracle_backend):
    """use_external_controller (command_manager.py:176-207): the controller's tensor IS the command — in the observation, in the
    tracking rewards — nothing is resampled, and such a step is never recorded (the tensor is the controller's to replace)."""
    from genesis_forge_amd.mdp import rewards

    env = Go2CommandDirectionEnv(num_envs=16, max_episode_length_s=0.4, cmd_resample_s=0.1, scene_kwargs=dict(ang_noise=0.2, seed=2))
    env.build()
    env.reset()
    buf = torch.zeros(16, 3)
    env.velocity_command.use_external_controller(lambda step: buf)
    g = torch.Generator().manual_seed(0)
    for t in range(30):
        buf[:, 0], buf[:, 2] = 0.1 * t, -0.05 * t
        obs, rew, term, trunc, extras = env.step(torch.randn(16, 12, generator=g))
        assert env._trace is None
        assert torch.equal(obs[:, :3], buf), "the observation's command columns are the controller's values, also for just-reset envs"
        assert torch.equal(env.velocity_command.command, buf)
    # the tracking term reads the controller's values too (the step's reward was computed from them)
    direct = rewards.command_tracking_lin_vel(env, vel_cmd_manager=env.velocity_command, entity_manager=env.robot_manager)
    lin = env.robot_manager.get_linear_velocity()
    want = torch.exp(-torch.sum(torch.square(buf[:, :2] - lin[:, :2]), dim=1) / 0.25)
    assert torch.allclose(direct, want, atol=1e-6)


@pytest.mark.parametrize("history", [None, 3])
@pytest.mark.parametrize("trace", [False, True])
def test_returned_observations_are_the_callers_own(oracle_backend, history, trace):
    """The reference returns a fresh torch.cat every call and keeps its history private (observation_manager.py:218-226):
    an observation held across steps keeps its values, and editing it in place does not leak into later history frames.
    ADVICE r1: the old 3-slot ring overwrote held tensors two calls later and read history from the returned buffer."""
    def run(hold, edit):
        env = Go2CommandDirectionEnv(num_envs=70, max_episode_length_s=1, cmd_resample_s=0.3, history=history, scene_kwargs=dict(ang_noise=0.3, seed=3))
        env.trace_enabled = trace
        env.build()
        env.seed(9)
        env.reset()
        g = torch.Generator().manual_seed(1)
        held, outs = [], []
        for t in range(12):
            obs = env.step(torch.randn(70, 12, generator=g))[0]
            outs.append(obs.clone())
            if hold:
                held.append((obs, obs.clone()))
            if edit:
                obs.clamp_(-0.01, 0.01)   # e.g. an in-place normalisation in the training loop
        assert (env._trace is not None) == trace
        return held, outs

    held, outs = run(hold=True, edit=False)
    for t, (kept, snapshot) in enumerate(held):
        assert torch.equal(kept, snapshot), f"the observation returned at step {t} changed after later steps"
    _, edited = run(hold=False, edit=True)
    for a, b in zip(outs, edited):
        assert torch.equal(a, b), "an in-place edit of a returned observation leaked into a later observation"


@pytest.mark.parametrize("trace", [False, True])
def test_a_dropped_env_is_released(oracle_backend, trace):
    """An env nobody holds any more goes away with its managers and buffers at the next garbage collection.  The observation
    getters tag the managers' persistent tensors with their owner (managers/action.py:_tag); a strong reference there is a cycle
    through a tensor's attribute dict, which the collector does not follow while the tensor is shared: every env that had ever
    observed stayed alive, with its device buffers and its 64 pinned statistics slots, until the process ran out of mappings."""
    import gc
    import weakref

    def run():
        env = Go2CommandDirectionEnv(num_envs=70, max_episode_length_s=1, cmd_resample_s=0.3, contacts=True, history=2,
                                     scene_kwargs=dict(ang_noise=0.3, seed=3))
        env.trace_enabled = trace
        env.build()
        env.seed(9)
        env.reset()
        g = torch.Generator().manual_seed(1)
        for _ in range(6):
            out = env.step(torch.randn(70, 12, generator=g))
            dict(out[4]["episode"])
        assert (env._trace is not None) == trace
        return [weakref.ref(x) for x in (env, env.stats, env.action_manager, env.observation_manager, env.episode_length)]

    refs = run()
    gc.collect()
    assert [r() for r in refs] == [None] * len(refs)


def test_static_observation_output_is_opt_in(oracle_backend):
    """output="static": the returned tensor is one of `static_slots` persistent buffers (no copy); the default is "fresh"."""
    from genesis_forge_amd.managers import ObservationManager

    assert ObservationManager.default_output == "fresh"
    env = Go2CommandDirectionEnv(num_envs=16, scene_kwargs=dict(seed=3))
    env.build()
    env.observation_manager.output = "static"
    env.reset()
    ptrs = [env.step(torch.zeros(16, 12))[0].data_ptr() for _ in range(7)]
    assert len(set(ptrs)) == ObservationManager.static_slots and ptrs[0] == ptrs[3] == ptrs[6]
    env.observation_manager.output = "fresh"
    ptrs = {env.step(torch.zeros(16, 12))[0].data_ptr() for _ in range(3)} & set(ptrs)
    assert not ptrs, "fresh outputs never alias the persistent slots"


@pytest.mark.parametrize("trace", [False, True])
def test_in_place_history_ring_holds_the_reference_frames(oracle_backend, trace):
    """output="ring": one persistent [N, H, O] buffer, a call writes only the new frame into slot `history_head`; gathered
    newest first (`ordered`) it is exactly the default output (observation_manager.py:218-226) at every step."""
    def run(output):
        env = Go2CommandDirectionEnv(num_envs=70, max_episode_length_s=0.4, cmd_resample_s=0.2, history=3, contacts=True,
                                     scene_kwargs=dict(ang_noise=0.3, seed=3))
        env.trace_enabled = trace
        env.build()
        om = env.observation_manager
        om.output = output
        env.seed(9)
        obs0, _ = env.reset()
        g = torch.Generator().manual_seed(1)
        outs = [om.ordered(obs0).clone()]
        ptrs = set()
        for _ in range(11):
            obs = env.step(torch.randn(70, 12, generator=g))[0]
            ptrs.add(obs.data_ptr())
            outs.append(om.ordered(obs).clone())
        assert (env._trace is not None) == trace
        return outs, ptrs

    want, _ = run("fresh")
    got, ptrs = run("ring")
    assert len(ptrs) == 1, "the ring IS the returned tensor"
    for t, (a, b) in enumerate(zip(want, got)):
        assert torch.equal(a, b), f"frames differ at observation {t}"


@pytest.mark.parametrize("trace,output", [(False, "fresh"), (True, "fresh"), (True, "static")])
def test_history_unroll_equals_history_shift(oracle_backend, trace, output):
    """history="unroll" (ring + gf_history_unroll, the default for output="fresh") returns exactly the tensors history="shift"
    returns (observation_manager.py:218-226), ordinary and recorded steps alike, and the "fresh" tensors are the caller's own."""
    from genesis_forge_amd.managers import ObservationManager

    def run(history):
        old = (ObservationManager.default_output, ObservationManager.default_history)
        ObservationManager.default_output, ObservationManager.default_history = output, history
        try:
            env = Go2CommandDirectionEnv(num_envs=70, max_episode_length_s=0.4, cmd_resample_s=0.2, history=3, contacts=True,
                                         scene_kwargs=dict(ang_noise=0.3, seed=3))
            env.trace_enabled = trace
            env.build()
        finally:
            ObservationManager.default_output, ObservationManager.default_history = old
        om = env.observation_manager
        assert om._unrolled == (history == "unroll")
        env.seed(9)
        obs0, _ = env.reset()
        g = torch.Generator().manual_seed(1)
        held = [obs0]
        outs = [obs0.clone()]
        for _ in range(11):
            held.append(env.step(torch.randn(70, 12, generator=g))[0])
            outs.append(held[-1].clone())
        assert (env._trace is not None) == trace
        if output == "fresh":   # nobody overwrote a tensor the caller kept
            assert all(torch.equal(h, o) for h, o in zip(held, outs)) and len({h.data_ptr() for h in held}) == len(held)
        return outs, (env._trace.n_ops if trace else 0)

    (want, ops_shift), (got, ops_unroll) = run("shift"), run("unroll")
    assert ops_unroll == ops_shift + (1 if trace else 0), "a recorded step carries the gather as one more op behind the fused launch"
    for t, (a, b) in enumerate(zip(want, got)):
        assert torch.equal(a, b), f"observation {t} differs"


#: every module path of the reference package (gamepads and the Taichi kernel aside) with the public classes / functions it defines
#: (names only, listed from the reference's source tree): user code imports from these paths, e.g.
#: ``from genesis_forge.managers.contact.contact_manager import ContactManager``
REFERENCE_MODULES = {
    'genesis_forge': [],
    'genesis_forge.genesis_env': ['GenesisEnv'],
    'genesis_forge.managed_env': ['ManagedEnvironment', 'ManagersDict'],
    'genesis_forge.managers': [],
    'genesis_forge.managers.action': [],
    'genesis_forge.managers.action.base': ['BaseActionManager'],
    'genesis_forge.managers.action.position_action_manager': ['PositionActionManager'],
    'genesis_forge.managers.action.position_within_limits': ['PositionWithinLimitsActionManager'],
    'genesis_forge.managers.base': ['BaseManager'],
    'genesis_forge.managers.command': [],
    'genesis_forge.managers.command.command_manager': ['CommandManager'],
    'genesis_forge.managers.command.velocity_command': ['VelocityCommandManager', 'VelocityCommandRange', 'VelocityDebugVisualizerConfig'],
    'genesis_forge.managers.config': [],
    'genesis_forge.managers.config.config_item': ['ConfigItem', 'ObservationConfigItem', 'RewardConfigItem', 'TerminationConfigItem'],
    'genesis_forge.managers.config.mdp_fn_class': ['MdpFnClass', 'ResetMdpFnClass'],
    'genesis_forge.managers.config.params_dict': ['ParamsDict'],
    'genesis_forge.managers.contact': [],
    'genesis_forge.managers.contact.config': ['ContactDebugVisualizerConfig'],
    'genesis_forge.managers.contact.contact_manager': ['ContactManager'],
    'genesis_forge.managers.entity_manager': ['EntityManager', 'EntityResetConfig'],
    'genesis_forge.managers.observation_manager': ['ObservationConfig', 'ObservationManager'],
    'genesis_forge.managers.reward_manager': ['RewardConfig', 'RewardManager'],
    'genesis_forge.managers.termination_manager': ['TerminationConfig', 'TerminationManager'],
    'genesis_forge.managers.terrain_manager': ['TerrainManager'],
    'genesis_forge.mdp': [],
    'genesis_forge.mdp.observations': ['contact_force', 'current_actions', 'entity_angular_velocity', 'entity_dofs_force', 'entity_dofs_position', 'entity_dofs_velocity', 'entity_linear_velocity', 'entity_projected_gravity'],
    'genesis_forge.mdp.reset': ['position', 'randomize_link_mass_shift', 'randomize_terrain_position', 'set_rotation', 'zero_all_dofs_velocity'],
    'genesis_forge.mdp.rewards': ['action_rate_l2', 'ang_vel_xy_l2', 'base_height', 'body_acceleration_exp', 'command_tracking_ang_vel', 'command_tracking_lin_vel', 'contact_force', 'dof_similar_to_default', 'feet_air_time', 'feet_slide', 'flat_orientation_l2', 'has_contact', 'is_alive', 'lin_vel_z_l2', 'stand_still_joint_deviation_l1', 'terminated'],
    'genesis_forge.mdp.terminations': ['bad_orientation', 'base_height_below_minimum', 'contact_force', 'contact_force_with_grace_period', 'has_contact', 'out_of_bounds', 'timeout'],
    'genesis_forge.utils': ['entity_ang_vel', 'entity_lin_vel', 'entity_projected_gravity', 'links_by_name_pattern'],
    'genesis_forge.wrappers': [],
    'genesis_forge.wrappers.rsl_rl': ['RslRlWrapper'],
    'genesis_forge.wrappers.skrl': ['SkrlEnvWapper'],
    'genesis_forge.wrappers.video': ['VideoWrapper', 'capped_cubic_episode_trigger'],
    'genesis_forge.wrappers.wrapper': ['Wrapper'],
}


def test_every_module_path_of_the_reference_resolves_through_the_alias():
    import importlib

    import genesis_forge_amd
    from genesis_forge_amd import compat

    compat.install(genesis_forge_amd)
    for path, names in REFERENCE_MODULES.items():
        mod = importlib.import_module(path)
        missing = [n for n in names if not hasattr(mod, n)]
        assert not missing, f"{path}: {missing}"
