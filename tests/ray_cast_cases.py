"""Restatements and inputs for tests/test_ray_cast.py: the ray caster's float32 operation sequence (include/gf_step.h) in numpy array
operations, vectorised over all rays with the cell walk in lockstep under masks; a float64 reference of the same surface with another
structure (all grid-line crossings of a ray gathered and sorted, one quadratic in the ray's own parameter per segment); the terrain
as both see it; and the shapes the kernel is walked through.  Nothing here imports the HIP library.

numpy, not torch, for the reason height_scan_cases.py gives: torch's CPU sqrt is not correctly rounded on every machine."""
import ast

import numpy as np
import torch

import height_scan_cases as hc

E = 8       # GF_RAY_CAST_TILE_ENVS: envs per workgroup (asserted against the binding in the tests)
MAX_RAYS = 2048
ALIGN = {"world": 0, "yaw": 1, "base": 2}

#: |float32 sequence - float64 reference| over the unflagged rays of accuracy_poses() x {camera, lidar}: measured 1.141e-5 m (the numpy restatement; the
#: torch composition gives the same figure), times 4 for the other poses the GPU cases use on the same field and ranges.
MEASURED_F32_ERROR = 1.141e-5
TOL = 4.0 * MEASURED_F32_ERROR
GRAZING_SHIFT, GRAZING_MOVE, GRAZING_CAP = 1e-5, 1e-3, 0.005

f32 = np.float32
_ZERO, _ONE, _TWO, _HALF, _FOUR, _INF = f32(0.0), f32(1.0), f32(2.0), f32(0.5), f32(4.0), f32(np.inf)


# ---------------------------------------------------------------------------------------------------------------------------
# the terrain
# ---------------------------------------------------------------------------------------------------------------------------
def terrain_view(fix=None):
    """(field [rows = y, cols = x] float32 metres, (x_min, x_span, y_min, y_span) float32) as the TerrainManager keeps the fixture."""
    fix = hc.terrain_fixture() if fix is None else fix
    tk = ast.literal_eval(str(fix["terrain_kwargs"]))
    hf = (torch.from_numpy(np.asarray(fix["height_field"])).to(torch.float32) * float(tk["vertical_scale"])).T.contiguous().numpy()
    x_min, x_max, y_min, y_max = (float(v) for v in fix["bounds"])
    return hf, (f32(x_min), f32(x_max - x_min), f32(y_min), f32(y_max - y_min))


def _sel(c, a, b):
    return np.where(c, a, b).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the float32 sequence
# ---------------------------------------------------------------------------------------------------------------------------
def frames_f32(pos, quat, align):
    """(b [N, 3], rot: nine [N, 1] float32 columns r00 … r22)."""
    pos = np.asarray(pos, dtype=np.float32)
    n = pos.shape[0]
    one, zero = np.ones((n, 1), np.float32), np.zeros((n, 1), np.float32)
    if align == 0:
        return pos, (one, zero, zero, zero, one, zero, zero, zero, one)
    quat = np.asarray(quat, dtype=np.float32)
    qw, qx, qy, qz = quat[:, 0:1], quat[:, 1:2], quat[:, 2:3], quat[:, 3:4]
    c = _ONE - _TWO * (qy * qy + qz * qz)
    s = _TWO * (qw * qz + qx * qy)
    if align == 1:
        nrm = np.sqrt(c * c + s * s)
        flat = nrm < f32(1e-6)
        safe = np.where(flat, _ONE, nrm)
        cy = _sel(flat, _ONE, c / safe)
        sy = _sel(flat, _ZERO, s / safe)
        return pos, (cy, -sy, zero, sy, cy, zero, zero, zero, one)
    r01 = _TWO * (qx * qy - qw * qz)
    r02 = _TWO * (qx * qz + qw * qy)
    r11 = _ONE - _TWO * (qx * qx + qz * qz)
    r12 = _TWO * (qy * qz - qw * qx)
    r20 = _TWO * (qx * qz - qw * qy)
    r21 = _TWO * (qy * qz + qw * qx)
    r22 = _ONE - _TWO * (qx * qx + qy * qy)
    return pos, (c, r01, r02, s, r11, r12, r20, r21, r22)


def rays_f32(pos, quat, pattern, align):
    """World origins and directions, six [N, R] float32 arrays."""
    b, (r00, r01, r02, r10, r11, r12, r20, r21, r22) = frames_f32(pos, quat, align)
    pat = np.asarray(pattern, dtype=np.float32)
    px, py, pz, ex, ey, ez = (pat[None, :, i] for i in range(6))
    ox = b[:, 0:1] + ((r00 * px + r01 * py) + r02 * pz)
    oy = b[:, 1:2] + ((r10 * px + r11 * py) + r12 * pz)
    oz = b[:, 2:3] + ((r20 * px + r21 * py) + r22 * pz)
    dx = (r00 * ex + r01 * ey) + r02 * ez
    dy = (r10 * ex + r11 * ey) + r12 * ez
    dz = (r20 * ex + r21 * ey) + r22 * ez
    return ox, oy, oz, dx, dy, dz


def depth_factor_f32(pattern, axis):
    pat, ax = np.asarray(pattern, dtype=np.float32), np.asarray(axis, dtype=np.float32)
    return (pat[:, 3] * ax[0] + pat[:, 4] * ax[1]) + pat[:, 5] * ax[2]


def cast_f32(field, view, pos, quat, pattern, align, max_range, origin_z=0.0):
    """The contract's walk.  Returns a dict: t [N, R] float32 (valid where hit), hit, cells (cells visited per ray, 0 without a field
    or without an entry into the rectangle), ties (steps that crossed an x and a y line at once), entered (the clipped interval is not
    empty), left (a miss that walked off the rectangle or ended at its edge), start and grid_dir (grid coordinates), o and d (the rays)."""
    with np.errstate(all="ignore"):
        return _cast_f32(field, view, pos, quat, pattern, align, f32(max_range), f32(origin_z))


def _cast_f32(field, view, pos, quat, pattern, align, tmax, origin_z):
    ox, oy, oz, dx, dy, dz = rays_f32(pos, quat, pattern, align)
    shape = ox.shape
    res = dict(o=(ox, oy, oz), d=(dx, dy, dz))
    if field is None:
        c = oz - origin_z
        below = c <= _ZERO
        tt = c / (-dz)
        hit = below | ((dz < _ZERO) & (tt <= tmax))
        res.update(t=_sel(below, _ZERO, tt), hit=hit, cells=np.zeros(shape, np.int32), entered=np.zeros(shape, bool))
        return res
    H, W = field.shape
    x_min, x_span, y_min, y_span = view
    fw, fh = f32(W - 1), f32(H - 1)
    sx, sy = fw / x_span, fh / y_span
    gx0, gy0 = (ox - x_min) * sx, (oy - y_min) * sy
    du, dv = dx * sx, dy * sy
    idu, idv = _ONE / du, _ONE / dv
    # the slab test, in grid coordinates
    t0, t1 = np.zeros(shape, np.float32), np.full(shape, tmax, np.float32)
    ok = np.ones(shape, bool)
    for g0, dd, idd, far in ((gx0, du, idu, fw), (gy0, dv, idv, fh)):
        moving = dd != _ZERO
        ta, tb = (-g0) * idd, (far - g0) * idd
        lo, hi = _sel(ta < tb, ta, tb), _sel(ta < tb, tb, ta)
        t0 = _sel(moving & (lo > t0), lo, t0)
        t1 = _sel(moving & (hi < t1), hi, t1)
        ok &= moving | ((g0 >= _ZERO) & (g0 <= far))
    ok &= t0 <= t1
    # the entry cell
    tin = t0
    cell = []
    for g0, dd, last in ((gx0, du, W - 2), (gy0, dv, H - 2)):
        gin = g0 + tin * dd
        fl = np.floor(gin)
        i = np.where(ok, fl, _ZERO).astype(np.int64)
        i = i - ((dd < _ZERO) & (gin == fl))
        cell.append(np.clip(i, 0, last).astype(np.int32))
    ix, iy = cell
    sgx, sgy = np.where(du > _ZERO, 1, -1).astype(np.int32), np.where(dv > _ZERO, 1, -1).astype(np.int32)
    active = ok.copy()
    hit = np.zeros(shape, bool)
    left = np.zeros(shape, bool)
    t = np.zeros(shape, np.float32)
    cells = np.zeros(shape, np.int32)
    ties = np.zeros(shape, np.int32)
    for _ in range((W - 1) + (H - 1) + 1):
        if not active.any():
            break
        cells += active
        tnx = _sel(du != _ZERO, ((ix + (du > _ZERO)).astype(np.float32) - gx0) * idu, _INF)
        tny = _sel(dv != _ZERO, ((iy + (dv > _ZERO)).astype(np.float32) - gy0) * idv, _INF)
        tn = _sel(tnx < tny, tnx, tny)
        tout = _sel(tn < t1, tn, t1)
        tout = _sel(tout > tin, tout, tin)
        smax = tout - tin
        u0 = (gx0 + tin * du) - ix.astype(np.float32)
        v0 = (gy0 + tin * dv) - iy.astype(np.float32)
        u0 = _sel(u0 < _ZERO, _ZERO, u0)
        u0 = _sel(u0 > _ONE, _ONE, u0)
        v0 = _sel(v0 < _ZERO, _ZERO, v0)
        v0 = _sel(v0 > _ONE, _ONE, v0)
        zin = oz + tin * dz
        h00, h10, h01, h11 = field[iy, ix], field[iy, ix + 1], field[iy + 1, ix], field[iy + 1, ix + 1]
        a, b = h10 - h00, h01 - h00
        k = (h00 - h10) - (h01 - h11)
        C = zin - (((h00 + a * u0) + b * v0) + (k * u0) * v0)
        B = dz - ((a * du + b * dv) + k * (u0 * dv + v0 * du))
        A = -((k * du) * dv)
        s = np.full(shape, _INF, np.float32)
        lin = (A == _ZERO) & (B < _ZERO)
        s = _sel(lin, C / (-B), s)
        disc = B * B - (_FOUR * A) * C
        quad = (A != _ZERO) & (disc >= _ZERO)
        sq = np.sqrt(np.where(quad, disc, _ZERO).astype(np.float32))
        q = -_HALF * (B + _sel(B < _ZERO, -sq, sq))
        r1, r2 = q / A, C / q
        s = _sel(quad & (r1 >= _ZERO) & (r1 < s), r1, s)
        s = _sel(quad & (r2 >= _ZERO) & (r2 < s), r2, s)
        under = C <= _ZERO
        found = active & (under | (s <= smax))
        t = _sel(found, _sel(under, tin, tin + s), t)
        hit |= found
        active &= ~found
        ended = active & ~(tn < t1)
        left |= ended & (t1 < tmax)
        active &= ~ended
        ties += active & (tnx <= tn) & (tny <= tn)
        ix = np.where(active & (tnx <= tn), ix + sgx, ix)
        iy = np.where(active & (tny <= tn), iy + sgy, iy)
        off = active & ((ix < 0) | (ix > W - 2) | (iy < 0) | (iy > H - 2))
        left |= off
        active &= ~off
        ix, iy = np.clip(ix, 0, W - 2).astype(np.int32), np.clip(iy, 0, H - 2).astype(np.int32)
        tin = _sel(active, tout, tin)
    assert t.dtype == np.float32
    res.update(t=t, hit=hit, cells=cells, ties=ties, entered=ok, left=left, start=(gx0, gy0), grid_dir=(du, dv))
    return res


def outputs_f32(res, pattern, max_range, miss_value=None, depth_axis=None):
    """(out [N, R], hits [N, R, 3]) float32 torch tensors from cast_f32's result, as the kernel writes them."""
    tmax = f32(max_range)
    miss = tmax if miss_value is None else f32(miss_value)
    t, hit = res["t"], res["hit"]
    val = t if depth_axis is None else t * depth_factor_f32(pattern, depth_axis)[None, :]
    out = _sel(hit, val, miss)
    te = _sel(hit, t, tmax)
    (ox, oy, oz), (dx, dy, dz) = res["o"], res["d"]
    hits = np.stack([ox + te * dx, oy + te * dy, oz + te * dz], axis=-1)
    assert out.dtype == np.float32 and hits.dtype == np.float32
    return torch.from_numpy(out), torch.from_numpy(hits)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the float64 reference
# ---------------------------------------------------------------------------------------------------------------------------
def rays_f64(pos, quat, pattern, align):
    pos, pat = np.asarray(pos, dtype=np.float64), np.asarray(pattern, dtype=np.float64)
    n = pos.shape[0]
    rot = np.tile(np.eye(3), (n, 1, 1))
    if align:
        q = np.asarray(quat, dtype=np.float64)
        qw, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        full = np.stack([np.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)], -1),
                         np.stack([2 * (qw * qz + qx * qy), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)], -1),
                         np.stack([2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)], -1)], 1)
        if align == 2:
            rot = full
        else:
            c, s = full[:, 0, 0], full[:, 1, 0]
            nrm = np.sqrt(c * c + s * s)
            flat = nrm < 1e-6
            cy, sy = np.where(flat, 1.0, c / np.where(flat, 1.0, nrm)), np.where(flat, 0.0, s / np.where(flat, 1.0, nrm))
            rot[:, 0, 0], rot[:, 0, 1], rot[:, 1, 0], rot[:, 1, 1] = cy, -sy, sy, cy
    o = pos[:, None, :] + np.einsum("nij,rj->nri", rot, pat[:, 0:3])
    d = np.einsum("nij,rj->nri", rot, pat[:, 3:6])
    return o, d


def cast_f64(field, view, pos, quat, pattern, align, max_range, z_shift=0.0):
    """[N, R] float64 distances along the ray to the bilinear surface, inf for a miss.  Every crossing of a grid line inside the clipped
    interval is gathered and sorted; each segment between two crossings lies in one cell (the one its midpoint is in), where the gap
    z - S is a quadratic c0 + c1 t + c2 t² in the ray's own parameter; the answer is the smallest root over all segments."""
    o, d = rays_f64(pos, quat, pattern, align)
    o = o.copy()
    o[..., 2] += z_shift
    fld = field.astype(np.float64)
    H, W = fld.shape
    x_min, x_span, y_min, y_span = (float(v) for v in view)
    shape = o.shape[:2]
    with np.errstate(all="ignore"):
        g0 = np.stack([(o[..., 0] - x_min) / x_span * (W - 1), (o[..., 1] - y_min) / y_span * (H - 1)], -1)
        dg = np.stack([d[..., 0] / x_span * (W - 1), d[..., 1] / y_span * (H - 1)], -1)
        t0, t1 = np.zeros(shape), np.full(shape, float(max_range))
        ok = np.ones(shape, bool)
        lines = []
        for ax, far in ((0, W - 1), (1, H - 1)):
            mv = dg[..., ax] != 0.0
            ta, tb = -g0[..., ax] / dg[..., ax], (far - g0[..., ax]) / dg[..., ax]
            t0 = np.where(mv, np.maximum(t0, np.minimum(ta, tb)), t0)
            t1 = np.where(mv, np.minimum(t1, np.maximum(ta, tb)), t1)
            ok &= mv | ((g0[..., ax] >= 0) & (g0[..., ax] <= far))
            tl = (np.arange(far + 1)[None, None, :] - g0[..., ax, None]) / dg[..., ax, None]
            lines.append(np.where(mv[..., None], tl, np.inf))
        ok &= t0 <= t1
        T = np.concatenate([t0[..., None], t1[..., None]] + lines, axis=-1)
        T = np.sort(np.clip(np.where(np.isnan(T), np.inf, T), t0[..., None], t1[..., None]), axis=-1)
        Ta, Tb = T[..., :-1], T[..., 1:]
        mid = 0.5 * (Ta + Tb)
        ix = np.clip(np.floor(np.nan_to_num(g0[..., 0, None] + mid * dg[..., 0, None])), 0, W - 2).astype(np.int64)
        iy = np.clip(np.floor(np.nan_to_num(g0[..., 1, None] + mid * dg[..., 1, None])), 0, H - 2).astype(np.int64)
        h00, h10, h01, h11 = fld[iy, ix], fld[iy, ix + 1], fld[iy + 1, ix], fld[iy + 1, ix + 1]
        a, b, k = h10 - h00, h01 - h00, h00 - h10 - h01 + h11
        U, V = g0[..., 0, None] - ix, g0[..., 1, None] - iy
        du, dv = dg[..., 0, None], dg[..., 1, None]
        c0 = o[..., 2, None] - (h00 + a * U + b * V + k * U * V)
        c1 = d[..., 2, None] - (a * du + b * dv + k * (U * dv + V * du))
        c2 = -k * du * dv
        best = np.where(c0 + Ta * (c1 + Ta * c2) <= 0.0, Ta, np.inf)        # already at or under the surface where the segment starts
        disc = c1 * c1 - 4.0 * c2 * c0
        sq = np.sqrt(np.maximum(disc, 0.0))
        q = -0.5 * (c1 + np.where(c1 < 0, -sq, sq))
        roots = [np.where(c2 != 0, q / c2, np.inf), np.where(q != 0, c0 / q, np.inf)]
        eps = 1e-12
        for r in roots:
            good = (disc >= 0) & (r >= Ta - eps) & (r <= Tb + eps) & np.isfinite(r)
            best = np.where(good & (r < best), np.clip(r, Ta, Tb), best)
        res = best.min(axis=-1)
    return np.where(ok, res, np.inf)


def grazing_f64(field, view, pos, quat, pattern, align, max_range):
    """(reference distances, grazing flag): a ray is grazing when its float64 distance — max_range for a miss — moves by more than
    GRAZING_MOVE when the origin is shifted by +-GRAZING_SHIFT in z.  Computed from the float64 reference alone."""
    d = lambda v: np.where(np.isinf(v), float(max_range), v)
    ref = cast_f64(field, view, pos, quat, pattern, align, max_range)
    up = cast_f64(field, view, pos, quat, pattern, align, max_range, z_shift=GRAZING_SHIFT)
    dn = cast_f64(field, view, pos, quat, pattern, align, max_range, z_shift=-GRAZING_SHIFT)
    flag = (np.abs(d(up) - d(ref)) > GRAZING_MOVE) | (np.abs(d(dn) - d(ref)) > GRAZING_MOVE)
    return ref, flag


# ---------------------------------------------------------------------------------------------------------------------------
# 3. inputs and shapes
# ---------------------------------------------------------------------------------------------------------------------------
def accuracy_poses():
    """The two pose sets of the accuracy test: 64 bases within +-12 m (most outside the field) and 64 inside it."""
    inside = hc.random_poses(64, seed=12, xy=5.0)
    inside[:, 0] += 3.0
    inside[:, 1] += 6.5
    return [hc.random_poses(64, seed=11, xy=12.0), inside]


def mixed_poses(n, seed):
    """n poses, alternately anywhere within +-12 m and inside the field, for the GPU shapes."""
    a, b = hc.random_poses(n, seed, xy=12.0), hc.random_poses(n, seed + 1000, xy=5.0)
    b[:, 0] += 3.0
    b[:, 1] += 6.5
    a[1::2] = b[1::2]
    return a


def random_rays(r, seed, down=0.6):
    """[r, 6] float32: start offsets within +-0.3 m, unit directions over the sphere biased downwards (float64, rounded once)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(r, 3))
    d[:, 2] -= down
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return torch.from_numpy(np.concatenate([rng.uniform(-0.3, 0.3, (r, 3)), d], axis=1).astype(np.float32))


#: (N, R, extra floats between output rows): the tile size and the 256-lane pass crossed sparsely; R + gap with both multiples of 4
#: is the whole-quad path, gap 0 the dense one, 1 / 5 the one-float path
SHAPES = [
    (1, 1, 0), (1, 256, 0), (1, 2048, 1),
    (E - 1, 3, 0), (E - 1, 64, 5), (E - 1, 257, 0),
    (E, 63, 1), (E, 256, 0), (E, 768, 0),
    (E + 1, 1, 5), (E + 1, 65, 0), (E + 1, 255, 5), (E + 1, 64, 12),
    (3 * E + 5, 3, 1), (3 * E + 5, 64, 0), (3 * E + 5, 257, 1), (3 * E + 5, 768, 5), (3 * E + 5, 256, 4), (3 * E + 5, 2048, 0),
]
