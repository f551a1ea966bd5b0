"""Restatements and inputs for tests/test_height_scan.py: the height scan's sample points in float32 (the kernel's operation sequence,
one rounding per torch op on the CPU) and in float64, the error bound between the two, random poses, and the shapes the kernel is
walked through.  Nothing here imports the HIP library."""
import ast
import math

import numpy as np
import torch

import helpers

E = 16      # GF_HEIGHT_SCAN_TILE_ENVS: envs per workgroup (asserted against the binding in the tests)
EPS = 2.0 ** -23


def terrain_fixture():
    return helpers.load("terrain")


def quat_from_euler(roll, pitch, yaw):
    """(w, x, y, z) of the intrinsic z-y'-x'' rotation (yaw, then pitch, then roll), float64 in and out."""
    cr, sr = np.cos(roll / 2), np.sin(roll / 2)
    cp, sp = np.cos(pitch / 2), np.sin(pitch / 2)
    cy, sy = np.cos(yaw / 2), np.sin(yaw / 2)
    return np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], axis=-1)


def random_poses(n, seed, xy=12.0, tilt_deg=45.0):
    """n poses: yaw anywhere, |pitch| and |roll| <= tilt_deg, bases within +-xy metres, z in 0.2 … 0.9.  Returns one [n, 7] float32
    state tensor (x, y, z, qw, qx, qy, qz): pos and quat are column views of it."""
    rng = np.random.default_rng(seed)
    yaw = rng.uniform(-math.pi, math.pi, n)
    pitch = np.deg2rad(rng.uniform(-tilt_deg, tilt_deg, n))
    roll = np.deg2rad(rng.uniform(-tilt_deg, tilt_deg, n))
    q = quat_from_euler(roll, pitch, yaw)
    pos = np.stack([rng.uniform(-xy, xy, n), rng.uniform(-xy, xy, n), rng.uniform(0.2, 0.9, n)], axis=-1)
    return torch.from_numpy(np.concatenate([pos, q], axis=-1).astype(np.float32))


def random_pattern(p, seed, reach=1.6):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.uniform(-reach, reach, (p, 2)).astype(np.float32))


def points_f32(pos, quat, pattern, yaw=True):
    """[N, P, 2] world sample points: include/gf_step.h's sequence in numpy float32 array operations, one rounding each — IEEE add,
    multiply, divide and square root are correctly rounded there as on the GPU, and nothing is fused.  (numpy, not torch: torch's CPU
    sqrt goes through a vector maths library that is not correctly rounded on every CPU.)"""
    pos, pattern = pos.cpu().numpy().astype(np.float32), pattern.cpu().numpy().astype(np.float32)
    one, two = np.float32(1.0), np.float32(2.0)
    bx, by = pos[:, 0:1], pos[:, 1:2]
    ox, oy = pattern[None, :, 0], pattern[None, :, 1]
    if yaw:
        quat = quat.cpu().numpy().astype(np.float32)
        qw, qx, qy, qz = quat[:, 0:1], quat[:, 1:2], quat[:, 2:3], quat[:, 3:4]
        c = one - two * (qy * qy + qz * qz)
        s = two * (qw * qz + qx * qy)
        nrm = np.sqrt(c * c + s * s)
        flat = nrm < np.float32(1e-6)
        safe = np.where(flat, one, nrm)
        cy = np.where(flat, one, c / safe)
        sy = np.where(flat, np.float32(0.0), s / safe)
    else:
        cy, sy = np.ones_like(bx), np.zeros_like(bx)
    px = bx + (cy * ox - sy * oy)
    py = by + (sy * ox + cy * oy)
    out = np.stack([px, py], axis=-1)
    assert out.dtype == np.float32
    return torch.from_numpy(out)


def points_f64(pos, quat, pattern, yaw=True):
    """The same formulas evaluated in float64 from the float32 inputs."""
    pos, pattern = pos.cpu().double(), pattern.cpu().double()
    bx, by = pos[:, 0:1], pos[:, 1:2]
    ox, oy = pattern[:, 0].unsqueeze(0), pattern[:, 1].unsqueeze(0)
    if yaw:
        quat = quat.cpu().double()
        qw, qx, qy, qz = quat[:, 0:1], quat[:, 1:2], quat[:, 2:3], quat[:, 3:4]
        c = 1.0 - 2.0 * (qy * qy + qz * qz)
        s = 2.0 * (qw * qz + qx * qy)
        nrm = torch.sqrt(c * c + s * s)
        flat = nrm < 1e-6
        cy = torch.where(flat, torch.ones_like(c), c / nrm)
        sy = torch.where(flat, torch.zeros_like(s), s / nrm)
    else:
        cy, sy = torch.ones_like(bx), torch.zeros_like(bx)
    return torch.stack([bx + (cy * ox - sy * oy), by + (sy * ox + cy * oy)], dim=-1)


def point_bound(pos, pattern):
    """[N, P, 2]: |dp_k| <= 2^-23 (20 (|ox| + |oy|) + |b_k|).  (cy, sy) carry at most about 16 eps absolute error at nrm >= 0.7 —
    c and s a few eps each from their products and sums, the quotient by nrm ~1.4 times that plus its own rounding —, which enters
    the point multiplied by |ox| or |oy|; the two products, their difference and the final sum add (|ox| + |oy|) eps and
    (|b_k| + |ox| + |oy|) eps / 2 more."""
    pos, pattern = pos.cpu().double(), pattern.cpu().double()
    reach = 20.0 * (pattern[:, 0].abs() + pattern[:, 1].abs()).unsqueeze(0)           # [1, P]
    return EPS * torch.stack([reach + pos[:, 0:1].abs(), reach + pos[:, 1:2].abs()], dim=-1)


def field_slopes(fix):
    """(Gx, Gy): the largest height difference between adjacent cells of the fixture's field ([rows = y, cols = x] metres, as the
    TerrainManager keeps it) over the cell pitch — the most a bilinear sample can move per metre of x or y."""
    tk = ast.literal_eval(str(fix["terrain_kwargs"]))
    hf = np.asarray(fix["height_field"], dtype=np.float64) * float(tk["vertical_scale"])   # [x, y] before the manager's transpose
    x_min, x_max, y_min, y_max = (float(v) for v in fix["bounds"])
    pitch_x, pitch_y = (x_max - x_min) / (hf.shape[0] - 1), (y_max - y_min) / (hf.shape[1] - 1)
    gx = float(np.abs(np.diff(hf, axis=0)).max()) / pitch_x
    gy = float(np.abs(np.diff(hf, axis=1)).max()) / pitch_y
    return gx, gy, float(np.abs(hf).max())


def heights_f64(fix, pts):
    """TerrainManager.get_terrain_height's formulas (bilinear, border clamp, align_corners) in float64 at pts [..., 2]."""
    tk = ast.literal_eval(str(fix["terrain_kwargs"]))
    hf = torch.from_numpy(np.asarray(fix["height_field"], dtype=np.float64) * float(tk["vertical_scale"])).T.contiguous()   # [y, x]
    x_min, x_max, y_min, y_max = (float(v) for v in fix["bounds"])
    H, W = hf.shape
    ix = ((pts[..., 0] - x_min) / (x_max - x_min) * (W - 1)).clamp(0.0, W - 1.0)
    iy = ((pts[..., 1] - y_min) / (y_max - y_min) * (H - 1)).clamp(0.0, H - 1.0)
    x0, y0 = ix.floor().long(), iy.floor().long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    tx, ty = ix - x0, iy - y0
    return (hf[y0, x0] * (1 - tx) * (1 - ty) + hf[y0, x1] * tx * (1 - ty) + hf[y1, x0] * (1 - tx) * ty + hf[y1, x1] * tx * ty)


#: (N, P, extra floats between output rows): the tile size E and the 256-lane pass crossed sparsely.  out_stride = P is the dense
#: 16-byte path whatever P is, P + 1 / P + 5 the one-float path (P + 4 with P % 4 == 0 would be the whole-quad path: last row)
SHAPES = [
    (1, 1, 0), (1, 187, 0), (1, 1024, 1),
    (E - 1, 3, 0), (E - 1, 64, 5), (E - 1, 257, 0),
    (E, 4, 0), (E, 63, 1), (E, 256, 0), (E, 1024, 0),
    (E + 1, 1, 5), (E + 1, 65, 0), (E + 1, 187, 1), (E + 1, 255, 5),
    (3 * E + 5, 3, 1), (3 * E + 5, 4, 5), (3 * E + 5, 64, 0), (3 * E + 5, 187, 0), (3 * E + 5, 257, 1), (3 * E + 5, 1024, 5),
    (3 * E + 5, 256, 4), (E + 1, 64, 12),
]
