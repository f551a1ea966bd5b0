"""The terrain height scan: gf_height_scan (csrc/gf_height_scan.hip), managers.HeightScanner, mdp.observations.height_scan and
Go2RoughTerrainEnv(height_scan=…).

CPU half: the entry's refusals (they come before any HIP call, so libgf_step.so answers them without a GPU), the scanner's
ValueErrors, the grid pattern, the torch composition a backend without the entry gets against a float64 evaluation of the same
formulas, and the env with a "critic" observation manager on the oracle backend.  GPU half: the kernel's sample points bit for bit the
float32 restatement (tests/height_scan_cases.py) and its heights bit for bit what gf_terrain_height gives at those very points —
which is what shows that the scan and every other terrain query share one sampler — over the tile, pass and store-width boundaries,
every output a slice of a guarded buffer."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import height_scan_cases as hc
from guarded import Guarded, sync

INF = float("inf")
GF_OK, GF_E_NULL, GF_E_RANGE = 0, -1, -2   # include/gf_step.h
CLIPS = [(-0.2, 0.1), (-INF, INF), (-1.0, 1.0)]   # active on both sides (bz - offset - h spans about -0.95 … 0.5) / none / default


# ---------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------
def _terrain_manager(dev):
    from test_terrain import _terrain_manager as make

    return make(hc.terrain_fixture(), dev)


def _scanner(tm, **kw):
    from genesis_forge_amd.managers import HeightScanner

    return HeightScanner(tm.env, tm, **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _valid_args(nat, n=4, p=5):
    """A descriptor gf_height_scan accepts.  Its pointers are never followed: every case below is refused, or has no envs."""
    a = nat.GfHeightScanArgs()
    a.num_envs, a.num_points = n, p
    a.pos = a.quat = a.pattern = a.out = 0x1000
    a.pos_stride, a.quat_stride, a.out_stride = 3, 4, p
    a.align, a.relative, a.offset, a.clip_lo, a.clip_hi = 1, 1, 0.5, -1.0, 1.0
    return a


def _lib(nat):
    lib = C.CDLL(nat.lib_path())
    lib.gf_height_scan.restype = C.c_int
    lib.gf_height_scan.argtypes = [C.c_void_p, C.c_void_p]
    return lib


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: validation
# ---------------------------------------------------------------------------------------------------------------------------
NULL_CASES = {
    "out": lambda a: setattr(a, "out", None),
    "pos": lambda a: setattr(a, "pos", None),
    "pattern": lambda a: setattr(a, "pattern", None),
    "quat_with_yaw": lambda a: setattr(a, "quat", None),
}
RANGE_CASES = {
    "num_envs<0": lambda a: setattr(a, "num_envs", -1),
    "num_points=0": lambda a: (setattr(a, "num_points", 0), setattr(a, "out_stride", 8)),
    "num_points=1025": lambda a: (setattr(a, "num_points", 1025), setattr(a, "out_stride", 2048)),
    "pos_stride<3": lambda a: setattr(a, "pos_stride", 2),
    "quat_stride<4": lambda a: setattr(a, "quat_stride", 3),
    "out_stride<P": lambda a: setattr(a, "out_stride", 4),
    "align=2": lambda a: setattr(a, "align", 2),
    "align=-1": lambda a: setattr(a, "align", -1),
    "relative=2": lambda a: setattr(a, "relative", 2),
    "relative=-1": lambda a: setattr(a, "relative", -1),
    "clip_lo>clip_hi": lambda a: (setattr(a, "clip_lo", 0.5), setattr(a, "clip_hi", 0.25)),
    "rows<1": lambda a: (setattr(a.terrain, "height_field", 0x1000), setattr(a.terrain, "rows", 0), setattr(a.terrain, "cols", 4)),
    "cols<1": lambda a: (setattr(a.terrain, "height_field", 0x1000), setattr(a.terrain, "rows", 4), setattr(a.terrain, "cols", 0)),
}


def test_binding_matches_the_header():
    from genesis_forge_amd import _native as nat

    lib = _lib(nat)
    assert lib.gf_height_scan_sizeof() == C.sizeof(nat.GfHeightScanArgs)
    assert lib.gf_sizeof(41) == -1   # (gf_sizeof's table is the older entries': this one reports its own size)
    assert nat.GF_HEIGHT_SCAN_MAX_POINTS == 1024 and nat.GF_HEIGHT_SCAN_TILE_ENVS == hc.E
    assert lib.gf_abi_version() == nat.GF_ABI_VERSION == 11
    assert "height_scan" not in nat.PHASE_FUNCS and nat.GfHeightScanArgs not in nat.ABI_STRUCTS


@pytest.mark.parametrize("case", sorted(NULL_CASES))
def test_entry_refuses_missing_pointers(case):
    from genesis_forge_amd import _native as nat

    a = _valid_args(nat)
    NULL_CASES[case](a)
    assert _lib(nat).gf_height_scan(C.byref(a), None) == GF_E_NULL


def test_entry_refuses_null_args():
    from genesis_forge_amd import _native as nat

    assert _lib(nat).gf_height_scan(None, None) == GF_E_NULL


@pytest.mark.parametrize("case", sorted(RANGE_CASES))
def test_entry_refuses_out_of_range_fields(case):
    from genesis_forge_amd import _native as nat

    a = _valid_args(nat)
    RANGE_CASES[case](a)
    assert _lib(nat).gf_height_scan(C.byref(a), None) == GF_E_RANGE


def test_entry_accepts_an_empty_scan_without_a_launch():
    """num_envs == 0 is GF_OK before any HIP call (this runs on a machine without a GPU) — with infinite clips, with the largest and
    the smallest point count, and without a quaternion when the pattern keeps the world axes."""
    from genesis_forge_amd import _native as nat

    lib = _lib(nat)
    for edit in (lambda a: None,
                 lambda a: (setattr(a, "clip_lo", -INF), setattr(a, "clip_hi", INF)),
                 lambda a: (setattr(a, "clip_lo", 0.25), setattr(a, "clip_hi", 0.25)),
                 lambda a: (setattr(a, "num_points", 1024), setattr(a, "out_stride", 1024)),
                 lambda a: (setattr(a, "num_points", 1), setattr(a, "out_stride", 1)),
                 lambda a: (setattr(a, "align", 0), setattr(a, "quat", None), setattr(a, "quat_stride", 0))):
        a = _valid_args(nat, n=0)
        edit(a)
        assert lib.gf_height_scan(C.byref(a), None) == GF_OK


def test_scanner_value_errors(oracle_backend):
    tm = _terrain_manager("cpu")
    with pytest.raises(ValueError, match="align"):
        _scanner(tm, align="pitch")
    with pytest.raises(ValueError, match="clip"):
        _scanner(tm, clip=(0.5, -0.5))
    with pytest.raises(ValueError, match="points"):
        _scanner(tm, pattern=torch.zeros(0, 2))
    with pytest.raises(ValueError, match="points"):
        _scanner(tm, pattern=torch.zeros(1025, 2))
    with pytest.raises(ValueError, match="points"):
        _scanner(tm, size=(3.3, 3.3), resolution=0.1)   # 34 x 34 = 1 156
    for bad in (torch.zeros(5, 3), torch.zeros(10), torch.zeros(2, 5, 2)):
        with pytest.raises(ValueError, match=r"\[P, 2\]"):
            _scanner(tm, pattern=bad)
    sc = _scanner(tm, size=(0.2, 0.1), resolution=0.1)   # 3 x 2 points
    pos, quat = torch.zeros(4, 3), torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(4, 1)
    for kw in (dict(pos=pos.double()), dict(pos=torch.zeros(4, 2)), dict(pos=torch.zeros(4)), dict(quat=quat.half()),
               dict(quat=torch.zeros(4, 3)), dict(quat=torch.zeros(5, 4)), dict(out=torch.zeros(4, 5)), dict(out=torch.zeros(3, 6)),
               dict(out=torch.zeros(4, 6, dtype=torch.float64)), dict(out=torch.zeros(6, 4).T), dict(pos=torch.zeros(3, 4).T),
               dict(points_out=torch.zeros(4, 6)), dict(points_out=torch.zeros(4, 6, 2, dtype=torch.float64)),
               dict(points_out=torch.zeros(4, 6, 4)[..., :2]), dict(pos=pos.to("meta"))):
        args = dict(pos=pos, quat=quat)
        args.update(kw)
        with pytest.raises(ValueError):
            sc.scan(**args)
    assert sc.scan(pos, quat).shape == (4, 6)   # (the valid call the bad ones were made from)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the grid
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,resolution,nx,ny", [((1.6, 1.0), 0.1, 17, 11), ((0.0, 0.0), 0.1, 1, 1), ((1.0, 0.6), 0.2, 6, 4)])
def test_grid_pattern_order_and_values(oracle_backend, size, resolution, nx, ny):
    sc = _scanner(_terrain_manager("cpu"), size=size, resolution=resolution)
    assert sc.num_points == nx * ny and tuple(sc.pattern.shape) == (nx * ny, 2) and sc.pattern.dtype == torch.float32
    for j in range(ny):
        for i in range(nx):
            want = (np.float32(-size[0] / 2 + i * resolution), np.float32(-size[1] / 2 + j * resolution))   # float64, rounded once
            got = sc.pattern[j * nx + i]
            assert (float(got[0]), float(got[1])) == (float(want[0]), float(want[1])), (i, j)


def test_default_grid_is_17_by_11(oracle_backend):
    sc = _scanner(_terrain_manager("cpu"))
    assert sc.num_points == 187
    assert sc.pattern[0].tolist() == [np.float32(-0.8), np.float32(-0.5)] and sc.pattern[186].tolist() == [np.float32(0.8), np.float32(0.5)]
    assert sc.pattern[1].tolist() == [np.float32(-0.8 + 0.1), np.float32(-0.5)]   # x is the fast axis


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the torch composition against float64
# ---------------------------------------------------------------------------------------------------------------------------
def test_torch_fallback_against_float64(oracle_backend):
    """4 096 random poses (yaw anywhere, |pitch|, |roll| <= 45 deg: nrm = cos(pitch) >= 0.707; bases within +-12 m), 24 offsets within
    +-1.6 m.  Points: |dp_k| <= 2^-23 (20 (|ox| + |oy|) + |b_k|) (derived in height_scan_cases.point_bound).  Heights:
    |dout| <= Gx tol_x + Gy tol_y + 2^-23 (8 max|h| + |bz| + |offset|) with Gx, Gy the fixture's steepest cell-to-cell slopes — a
    bilinear sample moves at most that much per metre — and the clamp only shrinking differences."""
    assert not hasattr(oracle_backend, "height_scan")
    fix = hc.terrain_fixture()
    tm = _terrain_manager("cpu")
    n, p, offset = 4096, 24, 0.5
    state, pattern = hc.random_poses(n, seed=1), hc.random_pattern(p, seed=2)
    pos, quat = state[:, 0:3], state[:, 3:7]
    sc = _scanner(tm, pattern=pattern, offset=offset, clip=(-0.2, 0.1))
    pts = torch.full((n, p, 2), float("nan"))
    out = sc.scan(pos, quat, points_out=pts)
    assert out.shape == (n, p) and out is sc.scan(pos, quat)
    want_pts = hc.points_f64(pos, quat, pattern)
    tol = hc.point_bound(pos, pattern)
    err = (pts.double() - want_pts).abs()
    print("points: worst error / bound =", float((err / tol).max()))
    assert bool((err <= tol).all())
    # (the float32 restatement the GPU half compares bit for bit with meets the same bound)
    assert bool(((hc.points_f32(pos, quat, pattern).double() - want_pts).abs() <= tol).all())
    gx, gy, hmax = hc.field_slopes(fix)
    want = ((pos[:, 2:3].double() - offset) - hc.heights_f64(fix, want_pts)).clamp(-0.2, 0.1)
    htol = gx * tol[..., 0] + gy * tol[..., 1] + hc.EPS * (8.0 * hmax + pos[:, 2:3].double().abs() + abs(offset))
    herr = (out.double() - want).abs()
    print("heights: worst error / bound =", float((herr / htol).max()), "clamped share =", float(((want == -0.2) | (want == 0.1)).double().mean()))
    assert bool((herr <= htol).all())


# ---------------------------------------------------------------------------------------------------------------------------
# the env: a "critic" observation manager with the scan as an item
# ---------------------------------------------------------------------------------------------------------------------------
def _run_env(dev, trace, scene_cls=None, steps=6, n=8):
    from genesis_forge_amd import tasks

    make = lambda: tasks.Go2RoughTerrainEnv(num_envs=n, max_episode_length_s=1, cmd_resample_s=0.3, scene_kwargs=dict(ang_noise=0.4, seed=9),
                                            height_scan={"size": (0.2, 0.2), "resolution": 0.1})
    if scene_cls is None:
        env = make()
    else:
        with tasks.use_scene(scene_cls):
            env = make()
    env.trace_enabled = trace
    env.build()
    env.seed(5)
    env.reset()
    assert env.height_scanner.num_points == 9
    g = torch.Generator().manual_seed(0)
    outs = []
    for _ in range(steps):
        obs, _r, _te, _tr, extras = env.step(torch.randn(n, 12, generator=g).to(dev))
        critic = extras["observations"]["critic"]
        scan = env.height_scanner.scan()
        assert critic.shape == (n, obs.shape[1] + 9)
        assert torch.equal(critic[:, :obs.shape[1]], obs)          # the policy's items, then the scan
        assert torch.equal(critic[:, obs.shape[1]:], scan)         # … equal to a scan made right after the step
        assert scan is env.height_scanner.scan()
        outs.append((obs.cpu().clone(), critic.cpu().clone()))
    return env, outs


def _check_env(dev):
    env, plain = _run_env(dev, trace=False)
    _, traced = _run_env(dev, trace=True)
    for t, (a, b) in enumerate(zip(plain, traced)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), f"step {t}"
    assert not torch.equal(plain[0][1][:, -9:], plain[-1][1][:, -9:])   # (the robots moved: the scan is not a constant)
    return env


def test_env_critic_observations_on_the_oracle_backend(oracle_backend):
    from genesis_forge_amd.learner import RolloutStorage

    env = _check_env("cpu")
    st = RolloutStorage(env, 4, obs_groups={"policy": ["policy"], "critic": ["critic"]})
    assert st.obs_groups["critic"] == ["critic"]


def test_height_scan_none_builds_todays_managers(oracle_backend):
    from genesis_forge_amd import tasks

    def managers(**kw):
        env = tasks.Go2RoughTerrainEnv(num_envs=4, **kw)
        env.build()
        kinds = {k: [type(m).__name__ for m in (v if isinstance(v, list) else [v])] for k, v in env.managers.items()}
        return env, kinds

    env, kinds = managers()
    assert kinds == {"contact": ["ContactManager"] * 2, "entity": ["EntityManager"], "command": ["VelocityCommandManager"],
                     "terrain": ["TerrainManager"], "action": ["PositionActionManager"], "observation": ["ObservationManager"],
                     "reward": ["RewardManager"], "termination": ["TerminationManager"]}
    assert not hasattr(env, "height_scanner") and not hasattr(env, "critic_manager")
    env2, kinds2 = managers(height_scan={})
    assert kinds2 == dict(kinds, observation=["ObservationManager"] * 2)    # the scanner itself registers nothing
    assert env2.height_scanner.num_points == 187 and env2.critic_manager.name == "critic"
    assert env2.observation_manager.observation_space.shape == env.observation_manager.observation_space.shape
    assert env2.critic_manager.observation_space.shape == (env.observation_manager.observation_space.shape[0] + 187,)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _guarded_rows(n, p, gap, off=0):
    """An [n, p] view with row stride p + gap of a guarded, NaN-filled buffer that starts `off` floats past a 16-byte boundary."""
    g = Guarded(n * (p + gap), torch.float32, "cuda", off=off)
    g.t.fill_(float("nan"))
    rows = g.t.view(n, p + gap)
    return g, rows, rows[:, :p]


def _gaps_intact(g, rows, p):
    return g.guards_ok() and bool(torch.isnan(rows[:, p:]).all())


def _scan_and_check(tm, state, pattern, gap, off, clip, offset=0.5, align="yaw"):
    """Scans into guarded buffers and checks A (points) and B (heights, relative and absolute) of the module docstring."""
    n, p = state.shape[0], pattern.shape[0]
    dstate = state.cuda()
    pos, quat = dstate[:, 0:3], dstate[:, 3:7]                       # column views of one [N, 7] state tensor
    gp = Guarded(n * p * 2, torch.float32, "cuda")
    gp.t.fill_(float("nan"))
    pts = gp.t.view(n, p, 2)
    yaw = align == "yaw"
    lo, hi = clip
    for relative in (True, False):
        sc = _scanner(tm, pattern=pattern, offset=offset, clip=clip, relative=relative, align=align)
        g, rows, out = _guarded_rows(n, p, gap, off)
        ret = sc.scan(pos, quat if yaw else None, out=out, points_out=pts)
        sync("cuda")
        assert ret is out
        assert _gaps_intact(g, rows, p) and gp.guards_ok()
        # A: the sample points, bit for bit the float32 restatement, and within the float64 bound
        want = hc.points_f32(state[:, 0:3], state[:, 3:7], pattern, yaw=yaw)
        got = pts.cpu()
        assert torch.equal(_bits(got), _bits(want)), f"{int((_bits(got) != _bits(want)).sum())} sample coordinates differ"
        if yaw:
            assert bool(((got.double() - hc.points_f64(state[:, 0:3], state[:, 3:7], pattern)).abs() <= hc.point_bound(state[:, 0:3], pattern)).all())
        # B: the heights, bit for bit gf_terrain_height at the kernel's own points
        h = tm.get_terrain_height(pts[..., 0].reshape(-1), pts[..., 1].reshape(-1)).view(n, p).cpu()
        v = (state[:, 2:3] - torch.tensor(offset, dtype=torch.float32)) - h if relative else h
        want_out = torch.clamp(v, min=lo, max=hi)
        got_out = out.cpu()
        assert bool(torch.isfinite(got_out).all())
        assert torch.equal(_bits(got_out), _bits(want_out)), f"{int((_bits(got_out) != _bits(want_out)).sum())} heights differ (relative={relative})"
    return got, got_out


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(hc.SHAPES)))
def test_points_and_heights_over_the_kernel_boundaries(hip_backend, idx):
    """N in {1, E-1, E, E+1, 3E+5} x P in {1, 3, 4, 63, 64, 65, 187, 255, 256, 257, 1024} (sparsely) x out_stride in {P, P+1, P+5}
    (and P+4 / P+12: whole quads behind a gap).  Bases within +-12 m of a terrain that spans x -3 … 9, y 1.5 … 11.5: sample points lie
    beyond all four edges (asserted at the largest N).  The clip rotates through active-on-both-sides / infinite / default."""
    from genesis_forge_amd import _native as nat

    assert nat.GF_HEIGHT_SCAN_TILE_ENVS == hc.E
    n, p, gap = hc.SHAPES[idx]
    tm = _terrain_manager("cuda")
    state, pattern = hc.random_poses(n, seed=100 + idx), hc.random_pattern(p, seed=200 + idx)
    pts, out = _scan_and_check(tm, state, pattern, gap, off=0, clip=CLIPS[idx % 3])
    if n == 3 * hc.E + 5 and p >= 64:   # (enough bases and offsets for every edge)
        x, y = pts[..., 0], pts[..., 1]
        assert bool((x < -3).any() and (x > 9).any() and (y < 1.5).any() and (y > 11.5).any())


@pytest.mark.gpu
@pytest.mark.parametrize("n,p,off", [(hc.E + 1, 187, 1), (3 * hc.E + 5, 64, 2), (hc.E, 256, 3)])
def test_a_misaligned_output_takes_the_one_float_path(hip_backend, n, p, off):
    """`out` starts 4, 8 or 12 bytes past a 16-byte boundary: dense rows, but no 16-byte store is possible."""
    tm = _terrain_manager("cuda")
    _scan_and_check(tm, hc.random_poses(n, seed=7), hc.random_pattern(p, seed=8), gap=0, off=off, clip=(-0.2, 0.1))


@pytest.mark.gpu
def test_clip_is_active_on_both_sides(hip_backend):
    tm = _terrain_manager("cuda")
    _, out = _scan_and_check(tm, hc.random_poses(3 * hc.E + 5, seed=3), hc.random_pattern(187, seed=4), gap=0, off=0, clip=(-0.2, 0.1))
    # (_scan_and_check returns the relative=False run: terrain heights of -0.1 … 0.65 m clamped to -0.2 … 0.1)
    assert bool((out == 0.1).any()) and bool((out < 0.1).any())
    sc = _scanner(tm, pattern=hc.random_pattern(187, seed=4), clip=(-0.2, 0.1))
    state = hc.random_poses(3 * hc.E + 5, seed=3).cuda()
    rel = sc.scan(state[:, 0:3], state[:, 3:7]).cpu()
    assert bool((rel == 0.1).any()) and bool((rel == -0.2).any()) and bool(((rel > -0.2) & (rel < 0.1)).any())


@pytest.mark.gpu
def test_world_aligned_scan_never_reads_the_quaternion(hip_backend):
    tm = _terrain_manager("cuda")
    state, pattern = hc.random_poses(hc.E + 1, seed=11), hc.random_pattern(65, seed=12)
    pts, _ = _scan_and_check(tm, state, pattern, gap=1, off=0, clip=(-INF, INF), align="world")
    assert torch.equal(pts[..., 0], state[:, 0:1] + pattern[:, 0].unsqueeze(0))   # b + o, whatever the attitude
    assert torch.equal(pts[..., 1], state[:, 1:2] + pattern[:, 1].unsqueeze(0))


@pytest.mark.gpu
def test_degenerate_attitudes_take_the_unit_branch(hip_backend):
    """Pitch exactly 90 degrees (c = s = 0 up to rounding) and an all-zero quaternion: (cy, sy) = (1, 0), finite output."""
    tm = _terrain_manager("cuda")
    state = hc.random_poses(hc.E + 1, seed=21, xy=4.0)
    r = np.float32(math.sqrt(0.5))
    state[0::2, 3:7] = torch.tensor([r, 0.0, r, 0.0])
    state[1::2, 3:7] = 0.0
    pattern = hc.random_pattern(63, seed=22)
    pts, out = _scan_and_check(tm, state, pattern, gap=0, off=0, clip=(-1.0, 1.0))
    assert bool(torch.isfinite(pts).all()) and bool(torch.isfinite(out).all())
    assert torch.equal(pts[..., 0], state[:, 0:1] + pattern[:, 0].unsqueeze(0))
    assert torch.equal(pts[..., 1], state[:, 1:2] + pattern[:, 1].unsqueeze(0))


@pytest.mark.gpu
def test_flat_terrain_without_a_height_field(hip_backend):
    from test_terrain import _flat_manager

    tm = _flat_manager()   # no height field, origin_z = 0.125
    state = hc.random_poses(hc.E + 3, seed=31).cuda()
    sc = _scanner(tm, size=(0.4, 0.2), resolution=0.1, offset=0.25, clip=(-0.05, 0.3))
    g, rows, out = _guarded_rows(hc.E + 3, sc.num_points, 3)
    sc.scan(state[:, 0:3], state[:, 3:7], out=out)
    sync("cuda")
    want = torch.clamp((state[:, 2:3] - 0.25) - 0.125, min=-0.05, max=0.3).expand(-1, sc.num_points)
    assert torch.equal(_bits(out), _bits(want)) and _gaps_intact(g, rows, sc.num_points)
    assert bool((out == 0.3).any()) and bool((out == -0.05).any())


@pytest.mark.gpu
def test_out_as_a_column_block_of_a_wider_tensor(hip_backend):
    tm = _terrain_manager("cuda")
    n, w = 3 * hc.E + 5, 45 + 187 + 3
    state = hc.random_poses(n, seed=41).cuda()
    sc = _scanner(tm)
    g = Guarded(n * w, torch.float32, "cuda")
    g.t.fill_(float("nan"))
    wide = g.t.view(n, w)
    ret = sc.scan(state[:, 0:3], state[:, 3:7], out=wide[:, 45:45 + 187])
    sync("cuda")
    assert ret.data_ptr() == wide[:, 45:].data_ptr()
    assert bool(torch.isnan(wide[:, :45]).all()) and bool(torch.isnan(wide[:, 45 + 187:]).all()) and g.guards_ok()
    assert torch.equal(_bits(wide[:, 45:45 + 187]), _bits(sc.scan(state[:, 0:3], state[:, 3:7])))   # the persistent default output


@pytest.mark.gpu
def test_env_critic_observations_on_the_hip_backend(hip_backend):
    _check_env("cuda")


@pytest.mark.gpu
def test_persistent_output_and_fresh_getter_scene(hip_backend):
    """A second scan() returns the same tensor object with new values; an env on a scene with Genesis' public surface only (fresh
    getter tensors every call) scans what the env on persistent buffers scans."""
    from genesis_like import GenesisLikeScene

    env, plain = _run_env("cuda", trace=False)
    first = env.height_scanner.scan()
    before, ptr = first.clone(), first.data_ptr()
    env.step(torch.zeros(8, 12, device="cuda"))
    second = env.height_scanner.scan()
    assert second is first and second.data_ptr() == ptr and not torch.equal(second, before)
    _, fresh = _run_env("cuda", trace=False, scene_cls=GenesisLikeScene)
    _, fresh_traced = _run_env("cuda", trace=True, scene_cls=GenesisLikeScene)
    for t, (a, b, c) in enumerate(zip(plain, fresh, fresh_traced)):
        assert torch.equal(a[1], b[1]) and torch.equal(a[1], c[1]), f"step {t}"
