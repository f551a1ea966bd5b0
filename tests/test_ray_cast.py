"""The terrain ray caster: gf_ray_cast (csrc/gf_ray_cast.hip), managers.RayCaster and its pattern builders,
mdp.observations.ray_cast and Go2RoughTerrainEnv(depth_camera=…).

CPU half: the binding against the header, the entry's refusals (they come before any HIP call, so libgf_step.so answers them without
a GPU), the caster's ValueErrors, the pattern builders, the accuracy of the contract's float32 sequence — the torch composition a
backend without the entry gets and the numpy restatement (tests/ray_cast_cases.py), both against a float64 reference of another
structure — and the env with a "depth" observation manager on the oracle backend.  GPU half: the kernel bit for bit the numpy
restatement, distances and hit points, over the tile, pass and store-width boundaries and over every class of ray the walk
distinguishes, every output a slice of a guarded buffer."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import height_scan_cases as hc
import ray_cast_cases as rc
from guarded import Guarded, sync

INF = float("inf")
GF_OK, GF_E_NULL, GF_E_RANGE = 0, -1, -2   # include/gf_step.h
RANGE = 4.0


# ---------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------
def _terrain_manager(dev):
    from test_terrain import _terrain_manager as make

    return make(hc.terrain_fixture(), dev)


def _unit_grid_manager():
    """A 9 x 9 field over [0, 8] x [0, 8]: grid coordinates ARE world coordinates (sx = sy = 1 exactly), heights multiples of 1/8 m.
    Flat at 0 with one raised node at (2, 2) (four twisted cells around it), a ramp from x = 5 to a 1 m plateau at x >= 6."""
    from test_terrain import _terrain_manager as make

    hf = np.zeros((9, 9), dtype=np.int16)   # [x, y]
    hf[6:, :] = 8
    hf[2, 2] = 1
    fix = {"height_field": hf, "n": 8, "terrain_kwargs": repr(dict(pos=(0.0, 0.0, 0.0), n_subterrains=(1, 1), subterrain_size=(8.0, 8.0),
                                                                    horizontal_scale=1.0, vertical_scale=0.125))}
    tm = make(fix, "cuda")
    assert tuple(tm.get_bounds()) == (0.0, 8.0, 0.0, 8.0) and tuple(tm._height_field.shape) == (9, 9)
    return tm


def _field_view(tm):
    """The manager's own field and bounds, as numpy float32, for the restatement."""
    v = tm.gf_view()
    field = None if tm._height_field is None else tm._height_field.cpu().numpy()
    return field, (np.float32(v.x_min), np.float32(v.x_span), np.float32(v.y_min), np.float32(v.y_span)), float(v.origin_z)


def _caster(tm, **kw):
    from genesis_forge_amd.managers import RayCaster

    kw.setdefault("max_range", RANGE)
    return RayCaster(tm.env, tm, **kw)


def _camera(tm, **kw):
    from genesis_forge_amd.managers.ray_caster import pinhole_pattern

    return _caster(tm, pattern=pinhole_pattern(16, 12, 87.0), offset_pos=(0.3, 0.0, 0.05), offset_euler=(0.0, 30.0, 0.0), **kw)


def _lidar(tm, **kw):
    from genesis_forge_amd.managers.ray_caster import lidar_pattern

    return _caster(tm, pattern=lidar_pattern(8, (-25.0, 5.0), 360.0, 11.25), offset_pos=(0.0, 0.0, 0.1), **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _restate(tm, caster, state):
    field, view, origin_z = _field_view(tm)
    return rc.cast_f32(field, view, state[:, 0:3].numpy(), state[:, 3:7].numpy(), caster.pattern.cpu().numpy(), rc.ALIGN[caster.align],
                       caster.max_range, origin_z=origin_z)


def _want(res, caster):
    return rc.outputs_f32(res, caster.pattern.cpu().numpy(), caster.max_range, caster.miss_value,
                          caster.axis if caster.output == "depth" else None)


def _valid_args(nat, n=4, r=5):
    """A descriptor gf_ray_cast accepts.  Its pointers are never followed: every case below is refused, or has no envs."""
    a = nat.GfRayCastArgs()
    a.num_envs, a.num_rays = n, r
    a.pos = a.quat = a.pattern = a.out = 0x1000
    a.pos_stride, a.quat_stride, a.out_stride = 3, 4, r
    a.align, a.mode, a.max_range, a.miss_value = 2, 0, 4.0, 4.0
    a.axis[0] = 1.0
    return a


def _lib(nat):
    lib = C.CDLL(nat.lib_path())
    lib.gf_ray_cast.restype = C.c_int
    lib.gf_ray_cast.argtypes = [C.c_void_p, C.c_void_p]
    return lib


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the binding and the refusals
# ---------------------------------------------------------------------------------------------------------------------------
def _field(a, rows, cols):
    a.terrain.height_field, a.terrain.rows, a.terrain.cols = 0x1000, rows, cols


NULL_CASES = {
    "out": lambda a: setattr(a, "out", None),
    "pos": lambda a: setattr(a, "pos", None),
    "pattern": lambda a: setattr(a, "pattern", None),
    "quat_with_base": lambda a: setattr(a, "quat", None),
    "quat_with_yaw": lambda a: (setattr(a, "quat", None), setattr(a, "align", 1)),
}
RANGE_CASES = {
    "num_envs<0": lambda a: setattr(a, "num_envs", -1),
    "num_envs>2^31 tiles": lambda a: setattr(a, "num_envs", (2 ** 31) * rc.E),
    "num_rays=0": lambda a: (setattr(a, "num_rays", 0), setattr(a, "out_stride", 8)),
    "num_rays=2049": lambda a: (setattr(a, "num_rays", 2049), setattr(a, "out_stride", 4096)),
    "pos_stride<3": lambda a: setattr(a, "pos_stride", 2),
    "quat_stride<4": lambda a: setattr(a, "quat_stride", 3),
    "out_stride<R": lambda a: setattr(a, "out_stride", 4),
    "align=3": lambda a: setattr(a, "align", 3),
    "align=-1": lambda a: setattr(a, "align", -1),
    "mode=2": lambda a: setattr(a, "mode", 2),
    "mode=-1": lambda a: setattr(a, "mode", -1),
    "max_range<0": lambda a: setattr(a, "max_range", -0.5),
    "max_range=inf": lambda a: setattr(a, "max_range", INF),
    "max_range=nan": lambda a: setattr(a, "max_range", float("nan")),
    "rows<2": lambda a: _field(a, 1, 4),
    "cols<2": lambda a: _field(a, 4, 1),
    "rows=0": lambda a: _field(a, 0, 4),
}


def test_binding_matches_the_header():
    from genesis_forge_amd import _native as nat

    lib = _lib(nat)
    assert lib.gf_ray_cast_sizeof() == C.sizeof(nat.GfRayCastArgs) == 144
    assert lib.gf_sizeof(41) == -1   # (gf_sizeof's table stays at 40 entries: this entry reports its own size)
    assert nat.GF_RAY_CAST_MAX_RAYS == rc.MAX_RAYS == 2048 and nat.GF_RAY_CAST_TILE_ENVS == rc.E
    assert (nat.GF_RAY_ALIGN_WORLD, nat.GF_RAY_ALIGN_YAW, nat.GF_RAY_ALIGN_BASE) == (0, 1, 2) == tuple(rc.ALIGN[k] for k in ("world", "yaw", "base"))
    assert (nat.GF_RAY_MODE_DISTANCE, nat.GF_RAY_MODE_DEPTH) == (0, 1)
    assert lib.gf_abi_version() == nat.GF_ABI_VERSION == 11
    assert "ray_cast" not in nat.PHASE_FUNCS and nat.GfRayCastArgs not in nat.ABI_STRUCTS


@pytest.mark.parametrize("case", sorted(NULL_CASES))
def test_entry_refuses_missing_pointers(case):
    from genesis_forge_amd import _native as nat

    a = _valid_args(nat)
    NULL_CASES[case](a)
    assert _lib(nat).gf_ray_cast(C.byref(a), None) == GF_E_NULL


def test_entry_refuses_null_args():
    from genesis_forge_amd import _native as nat

    assert _lib(nat).gf_ray_cast(None, None) == GF_E_NULL


@pytest.mark.parametrize("case", sorted(RANGE_CASES))
def test_entry_refuses_out_of_range_fields(case):
    from genesis_forge_amd import _native as nat

    a = _valid_args(nat)
    RANGE_CASES[case](a)
    assert _lib(nat).gf_ray_cast(C.byref(a), None) == GF_E_RANGE


def test_entry_accepts_an_empty_cast_without_a_launch():
    """num_envs == 0 is GF_OK before any HIP call (this runs on a machine without a GPU): the largest and the smallest ray count, a
    zero range, infinite and zero miss values, depth mode, a 2 x 2 field, and no quaternion when the rays keep the world axes."""
    from genesis_forge_amd import _native as nat

    lib = _lib(nat)
    for edit in (lambda a: None,
                 lambda a: (setattr(a, "num_rays", 2048), setattr(a, "out_stride", 2048)),
                 lambda a: (setattr(a, "num_rays", 1), setattr(a, "out_stride", 1)),
                 lambda a: setattr(a, "max_range", 0.0),
                 lambda a: setattr(a, "miss_value", INF),
                 lambda a: (setattr(a, "miss_value", 0.0), setattr(a, "mode", 1)),
                 lambda a: _field(a, 2, 2),
                 lambda a: (setattr(a, "align", 0), setattr(a, "quat", None), setattr(a, "quat_stride", 0))):
        a = _valid_args(nat, n=0)
        edit(a)
        assert lib.gf_ray_cast(C.byref(a), None) == GF_OK


def test_caster_value_errors(oracle_backend):
    from genesis_forge_amd.managers.ray_caster import down_pattern, lidar_pattern, pinhole_pattern

    tm = _terrain_manager("cpu")
    with pytest.raises(ValueError, match="align"):
        _caster(tm, align="pitch")
    with pytest.raises(ValueError, match="output"):
        _caster(tm, output="image")
    for bad in (-1.0, INF, float("nan")):
        with pytest.raises(ValueError, match="max_range"):
            _caster(tm, max_range=bad)
    with pytest.raises(ValueError, match="rays"):
        _caster(tm, pattern=torch.zeros(0, 6))
    with pytest.raises(ValueError, match="rays"):
        _caster(tm, pattern=pinhole_pattern(64, 33, 90.0))   # 2 112
    for bad in (torch.zeros(5, 3), torch.zeros(12), torch.zeros(2, 5, 6)):
        with pytest.raises(ValueError, match=r"\[R, 6\]"):
            _caster(tm, pattern=bad)
    with pytest.raises(ValueError, match="direction"):
        _caster(tm, pattern=torch.zeros(4, 6))
    with pytest.raises(ValueError):
        pinhole_pattern(0, 4, 90.0)
    with pytest.raises(ValueError):
        pinhole_pattern(4, 4, 180.0)
    with pytest.raises(ValueError):
        lidar_pattern(0, (-10.0, 10.0))
    with pytest.raises(ValueError):
        down_pattern((1.0, 1.0), 0.0, 0.5)
    ca = _caster(tm, pattern=down_pattern((0.2, 0.1), 0.1, 0.5))   # 3 x 2 rays
    pos, quat = torch.zeros(4, 3), torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(4, 1)
    for kw in (dict(pos=pos.double()), dict(pos=torch.zeros(4, 2)), dict(pos=torch.zeros(4)), dict(quat=quat.half()),
               dict(quat=torch.zeros(4, 3)), dict(quat=torch.zeros(5, 4)), dict(out=torch.zeros(4, 5)), dict(out=torch.zeros(3, 6)),
               dict(out=torch.zeros(4, 6, dtype=torch.float64)), dict(out=torch.zeros(6, 4).T), dict(pos=torch.zeros(3, 4).T),
               dict(hits_out=torch.zeros(4, 6)), dict(hits_out=torch.zeros(4, 6, 3, dtype=torch.float64)),
               dict(hits_out=torch.zeros(4, 6, 4)[..., :3]), dict(pos=pos.to("meta"))):
        args = dict(pos=pos, quat=quat)
        args.update(kw)
        with pytest.raises(ValueError):
            ca.cast(**args)
    assert ca.cast(pos, quat).shape == (4, 6)   # (the valid call the bad ones were made from)
    with pytest.raises(ValueError, match="default output"):
        ca.cast(torch.zeros(5, 3), quat.repeat(2, 1)[:5])


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the pattern builders
# ---------------------------------------------------------------------------------------------------------------------------
def test_pinhole_pattern_order_norms_and_centre():
    from genesis_forge_amd.managers.ray_caster import pinhole_pattern

    p = pinhole_pattern(5, 3, 90.0)
    assert p.shape == (15, 6) and p.dtype == np.float64 and not p[:, 0:3].any()
    assert np.allclose(np.linalg.norm(p[:, 3:6], axis=1), 1.0, atol=1e-15, rtol=0)
    assert np.array_equal(p[7, 3:6], [1.0, 0.0, 0.0])                      # the centre pixel lies on the optical axis
    assert p[0, 4] > 0 and p[0, 5] > 0 and p[4, 4] < 0 and p[4, 5] > 0       # row 0 is the top row, left (+y) to right
    assert p[10, 4] > 0 and p[10, 5] < 0 and p[14, 4] < 0 and p[14, 5] < 0   # the last row looks down
    assert np.allclose(p[0:5, 5] / p[0:5, 3], p[0, 5] / p[0, 3])           # one image row: one height on the image plane
    assert math.isclose(-p[4, 4] / p[4, 3], math.tan(math.radians(45.0)) * 0.8, rel_tol=1e-12)   # pixel centres: (4 + 0.5) / 5 * 2 - 1 = 0.8
    assert math.isclose(p[0, 5] / p[0, 3], math.tan(math.radians(45.0)) * 3 / 5 * (2 / 3), rel_tol=1e-12)   # square pixels by default
    q = pinhole_pattern(16, 12, 87.0, 58.0)
    assert q.shape == (192, 6)
    assert math.isclose(q[0, 5] / q[0, 3], math.tan(math.radians(29.0)) * (11 / 12), rel_tol=1e-12)


def test_lidar_and_down_patterns():
    from genesis_forge_amd.managers.height_scanner import grid_pattern
    from genesis_forge_amd.managers.ray_caster import down_pattern, lidar_pattern

    p = lidar_pattern(8, (-25.0, 5.0), 360.0, 11.25)
    assert p.shape == (256, 6) and np.allclose(np.linalg.norm(p[:, 3:6], axis=1), 1.0, atol=1e-15, rtol=0)
    el = np.degrees(np.arcsin(p[:, 5])).reshape(8, 32)
    assert np.allclose(el[:, 0], np.linspace(-25.0, 5.0, 8)) and np.allclose(el, el[:, :1])   # channel-major, lowest first
    az = np.degrees(np.arctan2(p[:32, 4], p[:32, 3]))
    assert np.allclose(az, -180.0 + 11.25 * np.arange(32)) or np.allclose(np.mod(az + 360.0, 360.0), np.mod(-180.0 + 11.25 * np.arange(32) + 360.0, 360.0))
    arc = lidar_pattern(1, (-10.0, 10.0), 90.0, 45.0)
    assert arc.shape == (3, 6) and np.allclose(arc[1, 3:6], [1.0, 0.0, 0.0])   # one channel sits in the middle; an arc has both ends
    d = down_pattern((1.6, 1.0), 0.1, 0.5)
    assert d.shape == (187, 6) and np.array_equal(d[:, 0:2].astype(np.float32), grid_pattern((1.6, 1.0), 0.1))
    assert np.all(d[:, 2] == 0.5) and np.all(d[:, 3:6] == [0.0, 0.0, -1.0])


def test_mounting_pose_is_folded_into_the_pattern(oracle_backend):
    from genesis_forge_amd.managers.ray_caster import pinhole_pattern

    tm = _terrain_manager("cpu")
    ca = _caster(tm, pattern=pinhole_pattern(5, 3, 90.0), offset_pos=(0.3, -0.1, 0.05), offset_euler=(0.0, 30.0, 0.0), output="depth")
    pat = ca.pattern.double().numpy()
    assert ca.pattern.dtype == torch.float32 and ca.num_rays == 15
    assert np.array_equal(ca.pattern[:, 0:3].numpy(), np.tile(np.float32([0.3, -0.1, 0.05]), (15, 1)))
    want_axis = [math.cos(math.radians(30.0)), 0.0, -math.sin(math.radians(30.0))]   # pitched DOWN: +x turns towards -z
    assert np.allclose(pat[7, 3:6], want_axis, atol=1e-7, rtol=0) and np.allclose(ca.axis, want_axis, atol=1e-7, rtol=0)
    assert np.allclose(np.linalg.norm(pat[:, 3:6], axis=1), 1.0, atol=1e-7, rtol=0)
    yawed = _caster(tm, pattern=pinhole_pattern(5, 3, 90.0), offset_euler=(0.0, 0.0, 90.0))
    assert np.allclose(yawed.pattern[7, 3:6].numpy(), [0.0, 1.0, 0.0], atol=1e-7, rtol=0)    # yaw turns +x to +y (left)
    rolled = _caster(tm, pattern=pinhole_pattern(5, 3, 90.0), offset_euler=(90.0, 0.0, 0.0))
    assert np.allclose(rolled.pattern[7, 3:6].numpy(), [1.0, 0.0, 0.0], atol=1e-7, rtol=0)   # roll keeps the axis …
    assert rolled.pattern[2, 4] < -0.1 and abs(float(rolled.pattern[2, 5])) < 1e-6            # … and turns the top-centre pixel from +z to -y
    default = _caster(tm)
    assert default.num_rays == 192 and default.align == "base" and default.miss_value == default.max_range == RANGE


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: accuracy of the float32 sequence
# ---------------------------------------------------------------------------------------------------------------------------
def test_float32_sequence_against_the_float64_reference(oracle_backend):
    """The torch composition (what the oracle backend gets) and the numpy restatement against the float64 reference on the committed
    terrain: 64 poses within +-12 m and 64 inside the field, the 16 x 12 camera pitched 30 degrees down and the 8 x 32 lidar at
    -25 … +5 degrees, align = base, 4 m: 57 344 rays.  A ray is set aside only by the reference's own grazing flag, at most 0.5 % of them.
    Measured here: 1 ray flagged; worst |f32 - f64| over the rest 1.14e-5 m (numpy), 1.14e-5 m (torch); rc.TOL is four times that."""
    assert not hasattr(oracle_backend, "ray_cast")
    tm = _terrain_manager("cpu")
    field, view = rc.terrain_view()
    mfield, mview, _ = _field_view(tm)
    assert np.array_equal(field, mfield) and view == mview and field.shape == (40, 48)
    total = flagged = 0
    worst = {"numpy": 0.0, "torch": 0.0}
    cells = []
    for poses in rc.accuracy_poses():
        pos, quat = poses[:, 0:3], poses[:, 3:7]
        for caster in (_camera(tm), _lidar(tm)):
            assert caster.align == "base" and caster.max_range == RANGE
            pat = caster.pattern.numpy()
            ref, flag = rc.grazing_f64(field, view, pos.numpy(), quat.numpy(), pat, 2, RANGE)
            want = np.where(np.isinf(ref), RANGE, ref)
            res = rc.cast_f32(field, view, pos.numpy(), quat.numpy(), pat, 2, RANGE)
            got_np = rc.outputs_f32(res, pat, RANGE)[0].double().numpy()
            hits = torch.full((64, caster.num_rays, 3), float("nan"))
            got_t = caster.cast(pos, quat, hits_out=hits).double().numpy()
            assert bool(torch.isfinite(hits).all())
            for name, got in (("numpy", got_np), ("torch", got_t)):
                err = np.abs(got - want)[~flag]
                worst[name] = max(worst[name], float(err.max()))
            total += flag.size
            flagged += int(flag.sum())
            cells.append((float(res["cells"][res["entered"]].mean()), int(res["cells"].max())))
            assert 0.1 < res["hit"].mean() < 0.9   # (both outcomes are well represented)
    print(f"rays {total}, flagged {flagged} ({flagged / total:.5%}); worst |f32 - f64| unflagged: {worst}; cells (mean, max): {cells}")
    assert total == 57344
    assert flagged / total <= rc.GRAZING_CAP
    assert worst["numpy"] <= rc.TOL and worst["torch"] <= rc.TOL
    assert worst["numpy"] <= rc.MEASURED_F32_ERROR * 1.0001   # (the constant is the measured figure, not a looser one)


# ---------------------------------------------------------------------------------------------------------------------------
# the env: a "depth" observation manager with the cast as its one item
# ---------------------------------------------------------------------------------------------------------------------------
def _run_env(dev, trace, scene_cls=None, steps=5, n=8):
    from genesis_forge_amd import tasks

    make = lambda: tasks.Go2RoughTerrainEnv(num_envs=n, max_episode_length_s=1, cmd_resample_s=0.3, scene_kwargs=dict(ang_noise=0.4, seed=9),
                                            height_scan={"size": (0.2, 0.2), "resolution": 0.1}, depth_camera={})
    if scene_cls is None:
        env = make()
    else:
        with tasks.use_scene(scene_cls):
            env = make()
    env.trace_enabled = trace
    env.build()
    env.seed(5)
    env.reset()
    assert env.depth_camera.num_rays == 192 and env.depth_camera.output == "depth" and env.height_scanner.num_points == 9
    g = torch.Generator().manual_seed(0)
    outs = []
    for _ in range(steps):
        obs, _r, _te, _tr, extras = env.step(torch.randn(n, 12, generator=g).to(dev))
        depth, critic = extras["observations"]["depth"], extras["observations"]["critic"]
        cast = env.depth_camera.cast()
        assert depth.shape == (n, 192) and critic.shape == (n, obs.shape[1] + 9)
        assert torch.equal(depth, cast)                      # … equal to a cast made right after the step
        assert cast is env.depth_camera.cast()
        assert torch.equal(critic[:, obs.shape[1]:], env.height_scanner.scan())
        outs.append((obs.cpu().clone(), depth.cpu().clone()))
    return env, outs


def _check_env(dev):
    env, plain = _run_env(dev, trace=False)
    _, traced = _run_env(dev, trace=True)
    for t, (a, b) in enumerate(zip(plain, traced)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), f"step {t}"
    last = plain[-1][1]
    assert not torch.equal(plain[0][1], last)                            # (the robots moved: the image is not a constant)
    assert bool((last < RANGE).any()) and bool((last > 0.05).all())      # the camera sees the ground in front of the robot
    return env


def test_env_depth_observations_on_the_oracle_backend(oracle_backend):
    from genesis_forge_amd.learner import RolloutStorage

    env = _check_env("cpu")
    st = RolloutStorage(env, 4, obs_groups={"policy": ["policy", "depth"], "critic": ["critic"]})
    assert st.obs_groups["policy"] == ["policy", "depth"]


def test_depth_camera_none_builds_todays_managers(oracle_backend):
    from genesis_forge_amd import tasks

    def managers(**kw):
        env = tasks.Go2RoughTerrainEnv(num_envs=4, **kw)
        env.build()
        return env, {k: [type(m).__name__ for m in (v if isinstance(v, list) else [v])] for k, v in env.managers.items()}

    env, kinds = managers()
    assert kinds["observation"] == ["ObservationManager"] and not hasattr(env, "depth_camera") and not hasattr(env, "depth_manager")
    env1, kinds1 = managers(height_scan={})
    assert kinds1 == dict(kinds, observation=["ObservationManager"] * 2) and not hasattr(env1, "depth_camera")
    env2, kinds2 = managers(depth_camera={})
    assert kinds2 == dict(kinds, observation=["ObservationManager"] * 2)     # the caster itself registers nothing
    assert env2.depth_manager.name == "depth" and env2.depth_manager.observation_space.shape == (192,)
    assert env2.observation_manager.observation_space.shape == env.observation_manager.observation_space.shape
    cam = env2.depth_camera
    assert (cam.num_rays, cam.align, cam.output, cam.max_range, cam.miss_value) == (192, "base", "depth", 4.0, 4.0)
    assert np.allclose(cam.axis, [math.cos(math.radians(30.0)), 0.0, -0.5], atol=1e-7, rtol=0)
    env3, kinds3 = managers(height_scan={}, depth_camera={"max_range": 2.0, "output": "distance"})
    assert kinds3 == dict(kinds, observation=["ObservationManager"] * 3)
    assert [m.name for m in env3.managers["observation"]][1:] == ["critic", "depth"] and env3.depth_camera.max_range == 2.0


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _guarded_rows(n, r, gap, off=0):
    """An [n, r] view with row stride r + gap of a guarded, NaN-filled buffer that starts `off` floats past a 16-byte boundary."""
    g = Guarded(n * (r + gap), torch.float32, "cuda", off=off)
    g.t.fill_(float("nan"))
    rows = g.t.view(n, r + gap)
    return g, rows, rows[:, :r]


def _cast_and_check(tm, caster, state, gap=0, off=0, hits=True, quat=None):
    """Casts into guarded buffers; `out` and `hits_out` must equal the numpy restatement bit for bit, gaps and guards untouched.
    Returns the restatement's result and the kernel's output (on the CPU)."""
    n, r = state.shape[0], caster.num_rays
    dstate = state.cuda()
    pos = dstate[:, 0:3]                                               # column views of one [N, 7] state tensor
    if quat is None:
        quat = dstate[:, 3:7] if caster.align != "world" else None
    g, rows, out = _guarded_rows(n, r, gap, off)
    gh = Guarded(n * r * 3, torch.float32, "cuda")
    gh.t.fill_(float("nan"))
    hout = gh.t.view(n, r, 3) if hits else None
    ret = caster.cast(pos, quat, out=out, hits_out=hout)
    sync("cuda")
    assert ret is out
    assert g.guards_ok() and bool(torch.isnan(rows[:, r:]).all()) and gh.guards_ok()
    res = _restate(tm, caster, state)
    want_out, want_hits = _want(res, caster)
    got = out.cpu()
    assert torch.equal(_bits(got), _bits(want_out)), f"{int((_bits(got) != _bits(want_out)).sum())} of {got.numel()} distances differ"
    if hits:
        got_h = hout.cpu()
        assert torch.equal(_bits(got_h), _bits(want_hits)), f"{int((_bits(got_h) != _bits(want_hits)).sum())} hit coordinates differ"
    else:
        assert gh.untouched() or bool(torch.isnan(gh.t).all())
    return res, got


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(rc.SHAPES)))
def test_kernel_equals_the_restatement_over_its_boundaries(hip_backend, idx):
    """N in {1, E-1, E, E+1, 3E+5} x R in {1, 3, 63, 64, 65, 255, 256, 257, 768, 2048} (sparsely) x out_stride in {R, R+1, R+5} (and
    R+4 / R+12: whole quads behind a gap), random rays biased downwards from poses on and off the field, align = base."""
    from genesis_forge_amd import _native as nat

    assert nat.GF_RAY_CAST_TILE_ENVS == rc.E
    n, r, gap = rc.SHAPES[idx]
    tm = _terrain_manager("cuda")
    caster = _caster(tm, pattern=rc.random_rays(r, seed=300 + idx), output=("depth", "distance")[idx % 2])
    res, _ = _cast_and_check(tm, caster, rc.mixed_poses(n, seed=100 + idx), gap=gap, hits=idx % 3 != 2)
    if n * r >= 1000:   # (enough rays for every outcome)
        assert res["hit"].any() and (~res["hit"] & res["entered"]).any() and (~res["entered"]).any() and res["cells"].max() >= 8


def test_shapes_cover_the_listed_sizes():
    assert {s[0] for s in rc.SHAPES} == {1, rc.E - 1, rc.E, rc.E + 1, 3 * rc.E + 5}
    assert {s[1] for s in rc.SHAPES} == {1, 3, 63, 64, 65, 255, 256, 257, 768, 2048}
    assert {s[2] for s in rc.SHAPES} >= {0, 1, 5} and any(s[2] and s[1] % 4 == 0 and s[2] % 4 == 0 for s in rc.SHAPES)


@pytest.mark.gpu
@pytest.mark.parametrize("sensor", ["camera", "lidar"])
def test_camera_and_lidar_on_the_fixture(hip_backend, sensor):
    """The two sensors of the accuracy test on its poses: bit for bit the restatement the CPU half holds against float64."""
    tm = _terrain_manager("cuda")
    caster = (_camera if sensor == "camera" else _lidar)(tm)
    for poses in rc.accuracy_poses():
        res, _ = _cast_and_check(tm, caster, poses)
        assert 0.1 < res["hit"].mean() < 0.9 and res["cells"].max() >= 20


def _class_rays():
    """name -> (origin, direction) in world = grid coordinates of _unit_grid_manager(), and what the restatement must report."""
    return {
        "first_cell_vertical": ((0.5, 0.5, 0.5), (0.0, 0.0, -1.0)),            # dx == 0 and dy == 0
        "many_cells": ((0.3, 0.4, 0.5), (1.0, 0.1, -0.02)),                    # reaches the ramp at x > 5
        "leaves": ((0.5, 0.5, 0.5), (-1.0, -0.3, 0.2)),                        # walks off the rectangle
        "enters": ((-2.0, 3.3, 0.5), (1.0, 0.0, -0.2)),                        # dy == 0; origin outside, enters through x = 0
        "never_enters": ((-2.0, -2.0, 0.5), (-1.0, 0.0, 0.0)),
        "below": ((7.0, 7.0, 0.5), (0.3, 0.2, 0.9)),                           # under the 1 m plateau
        "dx_zero": ((3.5, 0.5, 0.5), (0.0, 1.0, -0.1)),
        "on_line_negative": ((3.0, 2.5, 0.5), (-1.0, 0.0, -0.3)),              # starts on the grid line x = 3 heading to -x
        "corner": ((0.5, 0.5, 0.5), (1.0, 1.0, -0.05)),                        # through the corners (1, 1), (2, 2), …
        "along_line": ((0.5, 3.0, 0.5), (1.0, 0.0, -0.05)),                    # runs along the grid line y = 3
        "upwards": ((4.5, 4.5, 0.5), (0.1, 0.2, 1.0)),
    }


@pytest.mark.gpu
def test_every_class_of_ray(hip_backend):
    """One env at the origin with the world's axes, so a pattern row is a world ray; the field's grid coordinates are world
    coordinates.  Every class is asserted to have been reached from the restatement's per-ray cell count, tie count and flags."""
    tm = _unit_grid_manager()
    rays = _class_rays()
    names = list(rays)
    pat = np.array([list(o) + list(np.asarray(d) / np.linalg.norm(d)) for o, d in rays.values()], dtype=np.float64)
    state = torch.tensor([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]])
    caster = _caster(tm, pattern=pat, align="world", max_range=20.0)
    res, got = _cast_and_check(tm, caster, state, gap=1)
    row = lambda key: {n: res[key][0, i] for i, n in enumerate(names)}
    hit, cells, ties, entered, left = row("hit"), row("cells"), row("ties"), row("entered"), row("left")
    dist = {n: float(got[0, i]) for i, n in enumerate(names)}
    gx, gy = res["start"][0][0], res["start"][1][0]
    du, dv = res["grid_dir"][0][0], res["grid_dir"][1][0]
    i = names.index
    assert hit["first_cell_vertical"] and cells["first_cell_vertical"] == 1 and dist["first_cell_vertical"] == 0.5
    assert du[i("first_cell_vertical")] == 0.0 and dv[i("first_cell_vertical")] == 0.0
    assert hit["many_cells"] and cells["many_cells"] >= 6 and 4.7 < dist["many_cells"] < 5.7
    assert not hit["leaves"] and entered["leaves"] and left["leaves"] and dist["leaves"] == 20.0
    assert hit["enters"] and gx[i("enters")] < 0.0 and dv[i("enters")] == 0.0 and abs(dist["enters"] - 2.5 * math.sqrt(1.04)) < 1e-5
    assert not entered["never_enters"] and cells["never_enters"] == 0 and dist["never_enters"] == 20.0
    assert hit["below"] and cells["below"] == 1 and dist["below"] == 0.0
    assert hit["dx_zero"] and du[i("dx_zero")] == 0.0 and cells["dx_zero"] >= 5
    assert gx[i("on_line_negative")] == 3.0 and du[i("on_line_negative")] < 0.0 and hit["on_line_negative"]
    assert cells["on_line_negative"] == 2                                          # cells [2, 3] and [1, 2]: the walk did not start in [3, 4]
    assert abs(dist["on_line_negative"] - (0.5 / 0.3) * math.sqrt(1.09)) > 1e-3   # NOT the flat ground's distance: it met the raised node's cell
    assert hit["corner"] and ties["corner"] >= 3 and cells["corner"] == ties["corner"] + 1
    assert gy[i("along_line")] == 3.0 and dv[i("along_line")] == 0.0 and hit["along_line"] and cells["along_line"] >= 5
    assert not hit["upwards"] and left["upwards"]
    # the hit on the raised node's cell, against the float64 reference of the same surface
    field, view, _ = _field_view(tm)
    ref = rc.cast_f64(field, view, state[:, 0:3].numpy(), state[:, 3:7].numpy(), caster.pattern.cpu().numpy(), 0, 20.0)
    want = np.where(np.isinf(ref), 20.0, ref)
    assert float(np.abs(got.double().numpy() - want).max()) <= rc.TOL
    # a miss that ends inside a cell: the same rays cut short
    short = _caster(tm, pattern=pat, align="world", max_range=1.0)
    res1, got1 = _cast_and_check(tm, short, state)
    k = i("many_cells")
    assert not res1["hit"][0, k] and res1["entered"][0, k] and not res1["left"][0, k] and 1 <= res1["cells"][0, k] <= 2
    assert float(got1[0, k]) == 1.0 and float(got1[0, i("first_cell_vertical")]) == 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("n,r,off", [(rc.E + 1, 192, 1), (3 * rc.E + 5, 64, 2), (rc.E, 256, 3)])
def test_a_misaligned_output_takes_the_one_float_path(hip_backend, n, r, off):
    """`out` starts 4, 8 or 12 bytes past a 16-byte boundary: dense rows, but no 16-byte store is possible."""
    tm = _terrain_manager("cuda")
    _cast_and_check(tm, _caster(tm, pattern=rc.random_rays(r, seed=8)), rc.mixed_poses(n, seed=7), off=off)


@pytest.mark.gpu
def test_out_as_a_column_block_of_a_wider_tensor_and_hits_absent(hip_backend):
    tm = _terrain_manager("cuda")
    n, w = 3 * rc.E + 5, 45 + 192 + 3
    state = rc.mixed_poses(n, seed=41).cuda()
    ca = _camera(tm, output="depth")
    g = Guarded(n * w, torch.float32, "cuda")
    g.t.fill_(float("nan"))
    wide = g.t.view(n, w)
    ret = ca.cast(state[:, 0:3], state[:, 3:7], out=wide[:, 45:45 + 192])
    sync("cuda")
    assert ret.data_ptr() == wide[:, 45:].data_ptr()
    assert bool(torch.isnan(wide[:, :45]).all()) and bool(torch.isnan(wide[:, 45 + 192:]).all()) and g.guards_ok()
    assert torch.equal(_bits(wide[:, 45:45 + 192]), _bits(ca.cast(state[:, 0:3], state[:, 3:7])))   # the persistent default output
    _cast_and_check(tm, ca, state.cpu(), hits=False)


@pytest.mark.gpu
def test_alignments(hip_backend):
    """world never reads the quaternion (a NaN one changes nothing); yaw uses the height scan's (cy, sy), the degenerate attitudes
    included; base follows roll and pitch."""
    tm = _terrain_manager("cuda")
    state = rc.mixed_poses(rc.E + 1, seed=21)
    r = np.float32(math.sqrt(0.5))
    state[0, 3:7] = torch.tensor([r, 0.0, r, 0.0])     # pitch exactly 90 degrees: c = s = 0 up to rounding
    state[1, 3:7] = 0.0                                # an all-zero quaternion
    pat = rc.random_rays(65, seed=22)
    world = _caster(tm, pattern=pat, align="world")
    _, got_w = _cast_and_check(tm, world, state, gap=1)
    poisoned = torch.full((rc.E + 1, 4), float("nan"), device="cuda")
    _, got_p = _cast_and_check(tm, world, state, gap=1, quat=poisoned)
    assert torch.equal(_bits(got_w), _bits(got_p)) and bool(torch.isfinite(got_p).all())
    res_y, got_y = _cast_and_check(tm, _caster(tm, pattern=pat, align="yaw"), state)
    assert torch.equal(_bits(got_y[0:2]), _bits(got_w[0:2]))              # the unit branch: (cy, sy) = (1, 0)
    pts = hc.points_f32(state[:, 0:3], state[:, 3:7], pat[:, 0:2])       # the height scan's rotation of the start offsets' (x, y)
    assert torch.equal(torch.from_numpy(res_y["o"][0]), pts[..., 0]) and torch.equal(torch.from_numpy(res_y["o"][1]), pts[..., 1])
    _, got_b = _cast_and_check(tm, _caster(tm, pattern=pat, align="base"), state)
    assert not torch.equal(got_b[2:], got_y[2:]) and not torch.equal(got_y[2:], got_w[2:])


@pytest.mark.gpu
def test_depth_mode_and_miss_values(hip_backend):
    tm = _terrain_manager("cuda")
    state = rc.mixed_poses(rc.E + 3, seed=51)
    _, dist = _cast_and_check(tm, _camera(tm), state)
    miss = dist == RANGE
    assert bool(miss.any()) and bool((~miss).any())
    cam = _camera(tm, output="depth")
    res, depth = _cast_and_check(tm, cam, state)
    assert bool(torch.equal(torch.from_numpy(~res["hit"]), miss))
    factor = torch.from_numpy(rc.depth_factor_f32(cam.pattern.cpu().numpy(), cam.axis)).unsqueeze(0)
    assert bool((factor > 0.5).all() and (factor < 1.0).any())
    assert torch.equal(_bits(depth[~miss]), _bits((dist * factor)[~miss])) and bool((depth[miss] == RANGE).all())
    for value in (INF, 0.0, -1.0):
        for output in ("distance", "depth"):
            _, got = _cast_and_check(tm, _camera(tm, output=output, miss_value=value), state, hits=False)
            assert bool((got[miss] == value).all()) and torch.equal(_bits(got[~miss]), _bits((dist if output == "distance" else depth)[~miss]))


@pytest.mark.gpu
def test_plane_without_a_height_field(hip_backend):
    from test_terrain import _flat_manager

    tm = _flat_manager()   # no height field, origin_z = 0.125
    state = hc.random_poses(rc.E + 3, seed=31)
    state[0, 2] = -0.2     # a base (and the sensor 0.1 m from it) under the plane
    ca = _lidar(tm, max_range=3.0)
    res, got = _cast_and_check(tm, ca, state, gap=3)
    assert res["cells"].max() == 0 and res["hit"].any() and not res["hit"].all()
    o, d = rc.rays_f64(state[:, 0:3].numpy(), state[:, 3:7].numpy(), ca.pattern.cpu().numpy(), 2)
    gap_z = o[..., 2] - 0.125
    with np.errstate(all="ignore"):
        t = np.where(gap_z <= 0.0, 0.0, np.where(d[..., 2] < 0.0, gap_z / -d[..., 2], np.inf))
    want = np.where(t <= 3.0, t, 3.0)
    sure = np.abs(t - 3.0) > 1e-4
    assert float(np.abs(got.double().numpy() - want)[sure].max()) <= 1e-5 and bool((got[0] == 0.0).all())


@pytest.mark.gpu
def test_down_pattern_against_the_height_scan(hip_backend):
    """The height scan's grid cast straight down from `height` above the base, yaw-aligned, equals the height scan's relative heights
    with offset = -height wherever the point lies in the rectangle and the ground is in range."""
    from genesis_forge_amd.managers import HeightScanner
    from genesis_forge_amd.managers.ray_caster import down_pattern

    tm = _terrain_manager("cuda")
    height = 0.5
    n = 3 * rc.E + 5
    state = rc.mixed_poses(n, seed=61).cuda()
    pos, quat = state[:, 0:3], state[:, 3:7]
    sc = HeightScanner(tm.env, tm, offset=-height, clip=(-INF, INF), relative=True)
    pts = torch.zeros(n, sc.num_points, 2, device="cuda")
    scan = sc.scan(pos, quat, points_out=pts).cpu().double()
    ca = _caster(tm, pattern=down_pattern((1.6, 1.0), 0.1, height), align="yaw", max_range=2.0)
    cast = ca.cast(pos, quat).cpu().double()
    x, y = pts[..., 0].cpu(), pts[..., 1].cpu()
    m = 1e-4
    inside = (x > -3.0 + m) & (x < 9.0 - m) & (y > 1.5 + m) & (y < 11.5 - m) & (scan >= 0.0) & (scan < 2.0 - m)
    assert int(inside.sum()) > 1000 and bool((~inside).any())
    assert float((cast - scan).abs()[inside].max()) <= rc.TOL
    outside = (x < -3.0 - m) | (x > 9.0 + m) | (y < 1.5 - m) | (y > 11.5 + m)
    assert bool((cast[outside] == 2.0).all())          # no surface outside the rectangle: the border clamp is not extended


@pytest.mark.gpu
def test_env_depth_observations_on_the_hip_backend(hip_backend):
    _check_env("cuda")


@pytest.mark.gpu
def test_persistent_output_and_fresh_getter_scene(hip_backend):
    """A second cast() returns the same tensor object with new values; an env on a scene with Genesis' public surface only (fresh
    getter tensors every call) sees what the env on persistent buffers sees."""
    from genesis_like import GenesisLikeScene

    env, plain = _run_env("cuda", trace=False)
    first = env.depth_camera.cast()
    before, ptr = first.clone(), first.data_ptr()
    env.step(torch.zeros(8, 12, device="cuda"))
    second = env.depth_camera.cast()
    assert second is first and second.data_ptr() == ptr and not torch.equal(second, before)
    _, fresh = _run_env("cuda", trace=False, scene_cls=GenesisLikeScene)
    _, fresh_traced = _run_env("cuda", trace=True, scene_cls=GenesisLikeScene)
    for t, (a, b, c) in enumerate(zip(plain, fresh, fresh_traced)):
        assert torch.equal(a[1], b[1]) and torch.equal(a[1], c[1]), f"step {t}"
