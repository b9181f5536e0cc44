#!/usr/bin/env python3
"""Generator of tests/golden/hd95.npz: ``metric(gt, pred, spacing)`` of the reference's utils/metric.py:20-75 executed from the
reference file itself on a set of mask pairs, five numbers per pair (precision, recall, jaccard, dice, hs95).

usage: python tests/golden/make_hd95.py /path/to/reference        (needs scipy; the tests do not)

PINNED by the reference: the function is lifted out of the file's syntax tree (its module-level imports, torchio and monai, are
absent here) and run as it stands, so the order of the five numbers, precision, recall and the call
``compute_hausdorff_distance(pred, gdth, percentile=95, spacing=spacing)`` are the reference's own.  The arguments of that call
are recorded.
UNPINNED: ``compute_hausdorff_distance`` itself is monai's and is not here.  ``_StandIn`` restates it from monai 1.3.1 (the
reference's pin) without the source at hand: edge voxels of each mask by ``binary_erosion`` with the default structure,
``distance_transform_edt(~edges_other, sampling=spacing)`` read at the edge voxels of the first mask, ``np.percentile`` (linear
interpolation), the maximum of the two directions; one channel, so none is dropped.  A mask without foreground gives NaN (the least
certain part; the tests ask for "not finite" only).  Every recorded distance is also checked here against all pairwise distances
between the two edge sets, the large pair included.

Only inputs (bit-packed masks, or the recipe and a CRC32 for the large pair), spacings and recorded numbers are stored.
"""
import ast
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------------ inputs (no scipy below this line
# until the generator proper: the tests rebuild the large pair with large_pair())
def blob(shape, seed, cutoff, thresh, shift=(0, 0, 0)):
    """A smooth random mask: standard_normal(shape) from default_rng(seed), Fourier coefficients above ``cutoff`` cycles per voxel
    zeroed, scaled to unit deviation, rolled by ``shift`` voxels, thresholded at ``thresh`` deviations."""
    f = np.fft.fftn(np.random.default_rng(seed).standard_normal(shape))
    k = np.sqrt(sum(np.square(g) for g in np.meshgrid(*[np.fft.fftfreq(n) for n in shape], indexing="ij")))
    f[k > cutoff] = 0
    field = np.real(np.fft.ifftn(f))
    field = np.roll(field / field.std(), shift, axis=(0, 1, 2))
    return (field > thresh).astype(np.uint8)


LARGE = {"shape": (96, 128, 160), "spacing": (1.25, 0.7, 0.7), "seed": 11, "cutoff": 0.05,
         "gt_thresh": 0.8, "pred_thresh": 0.7, "pred_shift": (1, 1, 0)}


def large_pair(rec=LARGE):
    """(gt, pred) uint8 masks of the large case: one field, thresholded twice, the second shifted."""
    shape = tuple(int(v) for v in rec["shape"])
    gt = blob(shape, int(rec["seed"]), float(rec["cutoff"]), float(rec["gt_thresh"]))
    pred = blob(shape, int(rec["seed"]), float(rec["cutoff"]), float(rec["pred_thresh"]), tuple(int(v) for v in rec["pred_shift"]))
    return gt, pred


def pack_crc(gt, pred):
    return zlib.crc32(np.packbits(gt.ravel()).tobytes() + np.packbits(pred.ravel()).tobytes())


def small_cases():
    """[(name, gt, pred, spacing, as_float)] uint8 masks [D, H, W]."""
    S = (24, 40, 56)
    z = np.zeros(S, np.uint8)
    cases = []
    a, b = z.copy(), z.copy()
    a[4:14, 8:28, 10:40] = 1
    b[6:16, 11:31, 14:46] = 1
    cases.append(("boxes", a, b, (1.5, 0.8, 0.6), False))
    a, b = z.copy(), z.copy()
    a[2, 3, 4] = 1
    b[20, 30, 50] = 1
    cases.append(("voxels", a, b, (2.0, 1.0, 0.5), False))
    a = np.ones((12, 12, 12), np.uint8)
    b = a.copy()
    b[:, :, 6:] = 0
    cases.append(("border", a, b, (1.0, 1.0, 1.0), False))
    a = z.copy()
    a[3:20, 5:33, 7:50] = 1
    a[8:12, 10:20, 20:30] = 0
    cases.append(("identical", a, a.copy(), (1.0, 1.0, 3.0), False))
    a, b = z.copy(), z.copy()
    a[11:13, 2:38, 3:53] = 1
    b[2:22, 4:36, 27:29] = 1
    cases.append(("plates", a, b, (0.9, 1.1, 1.0), False))
    g = blob((40, 40, 40), 3, 0.06, 0.8)
    p = blob((40, 40, 40), 3, 0.06, 0.6, (0, 1, 0))
    for i, sp in enumerate([(1.0, 1.0, 1.0), (0.7, 1.3, 0.9), (2.0, 1.0, 1.5)]):
        cases.append((f"blob40_s{i}", g, p, sp, False))
    cases.append(("blobs48", blob((48, 48, 48), 5, 0.055, 0.9), blob((48, 48, 48), 6, 0.055, 0.9), (1.0, 1.0, 2.5), False))
    a, b = z.copy(), z.copy()
    a[5:15, 6:30, 9:41] = 1
    b[4:15, 9:27, 12:47] = 1
    cases.append(("float01", a, b, (1.2, 0.9, 0.9), True))
    e = np.zeros((12, 12, 12), np.uint8)
    f = e.copy()
    f[3:9, 2:10, 4:8] = 1
    cases.append(("empty_gt", e, f, (1.0, 1.0, 1.0), False))
    cases.append(("empty_pred", f, e, (1.0, 1.0, 1.0), False))
    cases.append(("empty_both", e, e.copy(), (1.0, 1.0, 1.0), False))
    return cases


# ------------------------------------------------------------------------------------------------ the generator
class _StandIn:
    """compute_hausdorff_distance(y_pred, y, percentile=, spacing=) restated with scipy; records how it was called."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def edges(m):
        from scipy import ndimage
        m = m != 0
        return ndimage.binary_erosion(m) ^ m

    def __call__(self, y_pred, y, include_background=False, distance_metric="euclidean", percentile=None, directed=False, spacing=None):
        import torch
        from scipy import ndimage
        self.calls.append({"shape": tuple(y_pred.shape), "percentile": percentile, "spacing": spacing})
        assert y_pred.shape == y.shape and y_pred.ndim == 5 and y_pred.shape[:2] == (1, 1)
        ep, eg = self.edges(np.asarray(y_pred)[0, 0]), self.edges(np.asarray(y)[0, 0])
        if not ep.any() or not eg.any():
            return torch.full((1, 1), float("nan"), dtype=torch.float64)
        d_pg = ndimage.distance_transform_edt(~eg, sampling=spacing)[ep]       # pred surface -> gt surface
        d_gp = ndimage.distance_transform_edt(~ep, sampling=spacing)[eg]
        v = max(np.percentile(d_pg, percentile), np.percentile(d_gp, percentile))
        return torch.full((1, 1), float(v), dtype=torch.float64)


def brute_hd(gt, pred, spacing, percentile=95.0, chunk=2048):
    """All pairwise distances between the two edge-voxel sets in millimetres, row and column minima, np.percentile."""
    import torch
    sp = torch.tensor(spacing, dtype=torch.float64)
    a = torch.from_numpy(np.argwhere(_StandIn.edges(gt))).double() * sp
    b = torch.from_numpy(np.argwhere(_StandIn.edges(pred))).double() * sp
    row = torch.empty(len(a), dtype=torch.float64)
    col = torch.full((len(b),), float("inf"), dtype=torch.float64)
    for i in range(0, len(a), chunk):
        d = torch.cdist(a[i:i + chunk], b, compute_mode="donot_use_mm_for_euclid_dist")
        row[i:i + chunk] = d.min(1).values
        col = torch.minimum(col, d.min(0).values)
    return max(np.percentile(row.numpy(), percentile), np.percentile(col.numpy(), percentile)), len(a), len(b)


def main(ref):
    import copy
    import torch
    stand = _StandIn()
    ns = {"np": np, "copy": copy, "compute_hausdorff_distance": stand}
    path = os.path.join(ref, "utils", "metric.py")
    for node in ast.parse(open(path).read()).body:       # as make_golden.py: _lift
        if isinstance(node, ast.FunctionDef) and node.name == "metric":
            exec(compile(ast.Module([node], []), path, "exec"), ns)
    rec = {"names": np.array([c[0] for c in small_cases()])}
    worst = 0.0
    for name, g, p, sp, as_float in small_cases():
        dt = torch.float32 if as_float else torch.int64
        stand.calls.clear()
        out = ns["metric"](torch.from_numpy(g)[None].to(dt), torch.from_numpy(p)[None].to(dt), sp)
        assert len(stand.calls) == 1
        rec[name + "/gt_bits"], rec[name + "/pred_bits"] = np.packbits(g.ravel()), np.packbits(p.ravel())
        rec[name + "/shape"] = np.array(g.shape, np.int64)
        rec[name + "/spacing"] = np.array(sp, np.float64)
        rec[name + "/as_float"] = np.array(as_float)
        rec[name + "/out"] = np.array([float(v) for v in out], np.float64)      # precision, recall, jaccard, dice, hs95
        rec[name + "/call_percentile"] = np.array(float(stand.calls[0]["percentile"]))
        rec[name + "/call_spacing"] = np.array(stand.calls[0]["spacing"], np.float64)
        if np.isfinite(out[4]):
            bf, na, nb = brute_hd(g, p, sp)
            gap = abs(bf - out[4]) / max(bf, 1e-300) if bf else abs(out[4])
            worst = max(worst, gap)
            print(f"{name:12s} {g.shape} hs95 {float(out[4]):.12f} brute {bf:.12f} gap {gap:.1e} edges {na} / {nb}")
        else:
            print(f"{name:12s} {g.shape} hs95 {out[4]}")
    g, p = large_pair()
    stand.calls.clear()
    out = ns["metric"](torch.from_numpy(g)[None].long(), torch.from_numpy(p)[None].long(), LARGE["spacing"])
    bf, na, nb = brute_hd(g, p, LARGE["spacing"])
    gap = abs(bf - out[4]) / bf
    worst = max(worst, gap)
    print(f"large        {g.shape} hs95 {float(out[4]):.12f} brute {bf:.12f} gap {gap:.1e} edges {na} / {nb}")
    for k, v in LARGE.items():
        rec["large/" + k] = np.array(v)
    rec["large/crc32"] = np.array(pack_crc(g, p), np.int64)
    rec["large/out"] = np.array([float(v) for v in out], np.float64)
    rec["large/edge_counts"] = np.array([na, nb], np.int64)
    assert worst < 1e-12, worst
    np.savez_compressed(os.path.join(HERE, "hd95.npz"), **rec)
    print("worst relative gap scipy restatement vs brute force:", worst, "bytes:", os.path.getsize(os.path.join(HERE, "hd95.npz")))


if __name__ == "__main__":
    main(sys.argv[1])
