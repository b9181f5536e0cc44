"""FLOAT64 restatement (NumPy) of the training augmentation that csrc/augment.hip computes, written from the definitions in
include/mi355seg.h / ``mi355seg.data.AugmentParams`` (dataloader.py:69-86 with config.aug=True; UNPINNED: torchio is absent and
the reference holds no fixture of its data pipeline).  Shared by tests/test_augment.py and tests/test_gpu_augment.py; it takes the
SAME drawn parameters as the kernels (the float32 3x4 matrix, bias coefficients, control points, sigma) and, for the noise, the
field recovered from the device (the generator is graded on its own)."""
import numpy as np


def unit(n):
    """normalised voxel coordinate (2 q + 1 - n) / (n - 1), q = 0 .. n-1"""
    return (2.0 * np.arange(n, dtype=np.float64) + 1.0 - n) / (n - 1.0)


def bias_field(coef, shape):
    """exp(sum c_ijk a0^i a1^j a2^k), i + j + k <= 3, coefficients in torchio's loop order (i outermost, k innermost)"""
    coef = np.asarray(coef, dtype=np.float64)
    a0, a1, a2 = unit(shape[0])[:, None, None], unit(shape[1])[None, :, None], unit(shape[2])[None, None, :]
    arg = np.zeros(shape, dtype=np.float64)
    n = 0
    for i in range(4):
        for j in range(4 - i):
            for k in range(4 - i - j):
                arg = arg + coef[n] * a0 ** i * a1 ** j * a2 ** k
                n += 1
    assert n == 20
    return np.exp(arg)


def stats(x, coef):
    """(mu, rho) of x * b over every voxel of every channel: mean and 1 / unbiased std; x [C,D,H,W]"""
    xb = np.asarray(x, dtype=np.float64) * bias_field(coef, x.shape[1:])[None]
    return float(xb.mean()), float(1.0 / xb.std(ddof=1)), xb


def volume(xb, mu, rho, sigma, g):
    """V = (x b - mu) rho + sigma g"""
    return (xb - mu) * rho + sigma * np.asarray(g, dtype=np.float64)


def bspline(f):
    return np.stack([(1 - f) ** 3 / 6.0, (3 * f ** 3 - 6 * f ** 2 + 4) / 6.0, (-3 * f ** 3 + 3 * f ** 2 + 3 * f + 1) / 6.0, f ** 3 / 6.0])


def displacement(cp, shape, axes):
    """uniform cubic B-spline displacement [3, len(z), len(y), len(x)] of the 7x7x7 control grid at the voxels axes = (z, y, x)"""
    cp = np.asarray(cp, dtype=np.float64)
    idx, wts = [], []
    for a, n in zip(axes, shape):
        u = 4.0 * np.asarray(a, dtype=np.float64) / (n - 1.0)
        i = np.minimum(np.floor(u), 3).astype(np.int64)
        idx.append(i)
        wts.append(bspline(u - i))                          # [4, len]
    out = np.zeros((3, len(axes[0]), len(axes[1]), len(axes[2])), dtype=np.float64)
    for a in range(4):
        for b in range(4):
            for c in range(4):
                w = wts[0][a][:, None, None] * wts[1][b][None, :, None] * wts[2][c][None, None, :]
                out += w[None] * cp[:, (idx[0] + a)[:, None, None], (idx[1] + b)[None, :, None], (idx[2] + c)[None, None, :]]
    return out


def coordinates(prm, origin, ps):
    """t = M [p; 1] (+ displacement(p)) for the patch voxels p = origin + offset: float64 [3, pd, ph, pw]"""
    m = np.asarray(prm.matrix, dtype=np.float64)
    axes = [np.arange(o, o + p, dtype=np.float64) for o, p in zip(origin, ps)]
    p = np.stack(np.meshgrid(*axes, indexing="ij"))
    t = np.einsum("ab,bzyx->azyx", m[:, :3], p) + m[:, 3][:, None, None, None]
    if prm.elastic:
        t = t + displacement(prm.cp, prm.shape, axes)
    return t


def inside(t, shape):
    n = np.asarray(shape, dtype=np.float64)[:, None, None, None]
    return np.all((t >= -0.5) & (t < n - 0.5), axis=0)


def sample_image(V, t, pad):
    """trilinear interpolation of V [C,D,H,W] at t (neighbour indices clamped to the volume) inside, ``pad`` outside"""
    shape = V.shape[1:]
    ins = inside(t, shape)
    lo, fr = [], []
    for a in range(3):
        ta = np.clip(t[a], -0.5, shape[a] - 0.5)
        f0 = np.floor(ta)
        lo.append(f0.astype(np.int64))
        fr.append(ta - f0)
    out = np.zeros((V.shape[0],) + t.shape[1:], dtype=np.float64)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = (fr[0] if dz else 1 - fr[0]) * (fr[1] if dy else 1 - fr[1]) * (fr[2] if dx else 1 - fr[2])
                z = np.clip(lo[0] + dz, 0, shape[0] - 1)
                y = np.clip(lo[1] + dy, 0, shape[1] - 1)
                x = np.clip(lo[2] + dx, 0, shape[2] - 1)
                out += w[None] * V[:, z, y, x]
    return np.where(ins[None], out, pad), ins


def sample_label(lbl, t):
    """the source label at floor(t + 0.5) inside, 0 outside; lbl [Cy,D,H,W]"""
    shape = lbl.shape[1:]
    ins = inside(t, shape)
    q = [np.clip(np.floor(np.clip(t[a], -0.5, shape[a] - 0.5) + 0.5).astype(np.int64), 0, shape[a] - 1) for a in range(3)]
    return np.where(ins[None], lbl[:, q[0], q[1], q[2]], 0.0), ins


def border_distance(t, shape):
    """distance of t to the nearest face of the sampling domain [-0.5, n - 0.5) on any axis"""
    n = np.asarray(shape, dtype=np.float64)[:, None, None, None]
    return np.minimum(np.abs(t + 0.5), np.abs(t - (n - 0.5))).min(axis=0)


def half_integer_distance(t):
    """distance of t to the nearest half-integer on any axis (where floor(t + 0.5) jumps)"""
    s = t + 0.5
    return np.abs(s - np.round(s)).min(axis=0)


def adjacent_step(V):
    """largest absolute difference between adjacent voxels of V [C,D,H,W] along any spatial axis"""
    return max(float(np.abs(np.diff(V, axis=a)).max()) for a in (1, 2, 3))
