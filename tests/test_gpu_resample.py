"""csrc/resample.hip on the device: the cubic B-spline prefilter, the gathers at orders 0 / 1 / 3, the label resampler, the fused
resample + argmax of the way back, and the call sites (the patch queue, predict.py).

The oracle is scipy.ndimage in fp64 on the TABLES' coordinates (base + the fp32 fraction, formed here from the fp64 formula
c(o) = clamp((o + 0.5) r - 0.5, 0, n - 1), not by the package): spline_filter(order=3, mode='mirror') for the prefilter and
map_coordinates for the gathers.

Bounds.  Order 0 and the nearest label mode: exact.  Order 1 and the probabilities of the way back: 16 * 2^-24 * max|x| (eight
products of three fp32 weights and an eight-term FMA sum).  Prefilter and order 3: no clean derivation (the coefficients reach about
1.2 max|x| and the recursion carries its rounding forward), so the bound is 4 x the largest error of a float32 CPU restatement
(scipy's spline_filter / map_coordinates(prefilter=False) with float32 input and output) against the fp64 oracle over this file's
own inputs, computed once per run (fixture ``restated``) -- never from the kernel's result.  Labels (linear) and the argmax of the
way back: equal to the fp64 one-hot / per-class oracle wherever its top-two margin is at least 1e-5 / 2e-5, and at most 1 % of a
case's voxels may fall below that margin (asserted for the oracle alone).  Every test prints its measured figure beside its bound
(pytest -rA); DESIGN.md section 4.19 holds the largest."""
import math
import os

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mi355seg
    mi355seg.lib()
    return mi355seg


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def smooth(shape, seed, channels=None):
    """z-scored smoothed noise, float32"""
    full = shape if channels is None else (channels,) + tuple(shape)
    x = np.random.default_rng(seed).standard_normal(full)
    x = ndi.gaussian_filter(x, [0.0] * (len(full) - 3) + [0.8 if n > 1 else 0.0 for n in shape])
    return ((x - x.mean()) / x.std()).astype(np.float32)


def out_len(n, r):
    return max(1, math.ceil(n / r - 1e-6))


def coords(n_in, n_out, ratio, order):
    """the coordinates the tables stand for, in fp64: order 0 the index, else floor(c) + fp32(c - floor(c))"""
    c = np.clip((np.arange(n_out, dtype=np.float64) + 0.5) * ratio - 0.5, 0.0, n_in - 1.0)
    if order == 0:
        return np.floor(c + 0.5)
    return np.floor(c) + (c - np.floor(c)).astype(np.float32).astype(np.float64)


def grid(shape, out_shape, ratios, order):
    return np.meshgrid(*[coords(n, no, r, order) for n, no, r in zip(shape, out_shape, ratios)], indexing="ij")


# (shape, ratios): the volumes and the per-axis ratios of the issue, mixed across axes; 0.4 is "2.5 mm to 1.0 mm", 2.5 its way back;
# the last case makes the order-3 box outgrow 64 KB of LDS at 4 x 8 x 32 outputs, so the host halves it
CASES = [((17, 23, 37), (0.7, 1.25, 2.5)), ((1, 1, 5), (1.0, 1.0, 0.5)), ((2, 3, 1), (0.5, 0.75, 1.0)), ((5, 4, 130), (1.5, 0.7, 0.75)),
         ((40, 9, 7), (0.4, 0.5, 1.25)), ((12, 22, 84), (2.5, 2.5, 2.5)), ((9, 11, 13), (1.0, 1.0, 1.0))]
IDS = ["x".join(map(str, c[0])) for c in CASES]
LINES = [1, 2, 3, 13, 14, 15]
PREFILTER_SHAPES = [c[0] for c in CASES[:5]] + [s for n in LINES for s in ((n, 3, 5), (3, n, 5), (3, 5, n))] + [(1, 2, 200), (2, 70, 3), (66, 1, 67)]


VOLUME_SHAPE, VOLUME_SPACING, VOLUME_TARGET = (10, 24, 26), (2.5, 0.7, 0.7), (1.0, 1.0, 1.0)
VOLUME_RATIOS = tuple(t / s for s, t in zip(VOLUME_SPACING, VOLUME_TARGET))


def volume_input():
    """the two-channel volume of test_resample_volume_channels_spacings_and_identity"""
    return smooth(VOLUME_SHAPE, 31, channels=2)


def case_out(shape, ratios):
    return tuple(out_len(n, r) for n, r in zip(shape, ratios))


@pytest.fixture(scope="module")
def restated():
    """the float32 CPU restatement against the fp64 oracle on this file's inputs -> {"prefilter": largest error, "order3": largest error}"""
    pre = 0.0
    for i, shape in enumerate(PREFILTER_SHAPES):
        x = smooth(shape, 100 + i)
        ref = ndi.spline_filter(x.astype(np.float64), order=3, mode="mirror", output=np.float64)
        pre = max(pre, float(np.abs(ndi.spline_filter(x, order=3, mode="mirror", output=np.float32).astype(np.float64) - ref).max()))
    o3 = 0.0
    inputs = [(smooth(shape, 200 + i), shape, ratios) for i, (shape, ratios) in enumerate(CASES)]
    inputs += [(x, VOLUME_SHAPE, VOLUME_RATIOS) for x in volume_input()]
    for x, shape, ratios in inputs:
        g = grid(shape, case_out(shape, ratios), ratios, 3)
        ref = ndi.map_coordinates(x.astype(np.float64), g, order=3, mode="mirror")
        c32 = ndi.spline_filter(x, order=3, mode="mirror", output=np.float32)
        got = ndi.map_coordinates(c32, g, order=3, mode="mirror", prefilter=False, output=np.float32)     # the tables' coordinates, exact
        o3 = max(o3, float(np.abs(got.astype(np.float64) - ref).max()))
    print(f"[resample] float32 CPU restatement against fp64: prefilter {pre:.3e}, order 3 {o3:.3e}; the bounds are 4 x these")
    assert 1e-8 < pre < 1e-4 and 1e-8 < o3 < 1e-4
    return {"prefilter": pre, "order3": o3}


# ---------------------------------------------------------------------------------------------- prefilter
@pytest.mark.parametrize("shape", PREFILTER_SHAPES, ids=["x".join(map(str, s)) for s in PREFILTER_SHAPES])
def test_prefilter_against_spline_filter(seg, restated, shape):
    F = seg.functional
    x = smooth(shape, 100 + PREFILTER_SHAPES.index(shape))
    ref = ndi.spline_filter(x.astype(np.float64), order=3, mode="mirror", output=np.float64)
    xd = dev(x)
    got = F.bspline3_prefilter(xd)
    again = F.bspline3_prefilter(xd)
    inplace = xd.clone()
    assert F.bspline3_prefilter(inplace, out=inplace) is inplace
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)) and torch.equal(got.view(torch.int32), inplace.view(torch.int32))
    assert torch.equal(xd, dev(x))                                              # the input is untouched out of place
    err, bound = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max()), 4.0 * restated["prefilter"]
    print(f"[resample] prefilter {shape}: error {err:.3e} (bound {bound:.3e} = 4 x the float32 restatement), max|c| {np.abs(ref).max():.2f}")
    assert got.shape == xd.shape and err <= bound
    # the passes one by one (W, H, D) are the whole, bitwise
    y = xd
    for axis in (2, 1, 0):
        if shape[axis] > 1:
            y = F.bspline3_prefilter(y, axis=axis)
    assert torch.equal(y.view(torch.int32), got.view(torch.int32))


def test_prefilter_channels_are_independent(seg):
    F = seg.functional
    x = smooth((6, 7, 70), 7, channels=3)
    whole = F.bspline3_prefilter(dev(x))
    for c in range(3):
        assert torch.equal(whole[c].view(torch.int32), F.bspline3_prefilter(dev(x[c])).view(torch.int32))


# ---------------------------------------------------------------------------------------------- gathers
@pytest.mark.parametrize("order", [0, 1, 3])
@pytest.mark.parametrize("shape,ratios", CASES, ids=IDS)
def test_gather_against_map_coordinates(seg, restated, shape, ratios, order):
    F = seg.functional
    x = smooth(shape, 200 + CASES.index((shape, ratios)))
    out_shape = case_out(shape, ratios)
    tables = F.ResampleTables(shape, out_shape, ratios, order, torch.device("cuda", 0))
    src = F.bspline3_prefilter(dev(x)) if order == 3 else dev(x)
    got = F.resample3d(src, tables)
    assert torch.equal(got.view(torch.int32), F.resample3d(src, tables).view(torch.int32))          # twice: the same bits
    g = grid(shape, out_shape, ratios, order)
    ref = ndi.map_coordinates(x.astype(np.float64), g, order=order, mode="mirror")
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
    bound = {0: 0.0, 1: 16 * EPS * float(np.abs(x).max()), 3: 4.0 * restated["order3"]}[order]
    print(f"[resample] order {order} {shape} -> {out_shape}: error {err:.3e} (bound {bound:.3e})")
    assert tuple(got.shape) == out_shape and err <= bound
    if order == 0:
        idx = [c.astype(np.int64) for c in g]
        assert np.array_equal(got.cpu().numpy(), x[idx[0], idx[1], idx[2]])


@pytest.mark.parametrize("order", [0, 1, 3])
def test_resample_volume_channels_spacings_and_identity(seg, restated, order):
    F = seg.functional
    x = volume_input()
    spacing, target = VOLUME_SPACING, VOLUME_TARGET
    xd = dev(x)
    got = F.resample_volume(xd, spacing, target, order)
    out_shape = F.resampled_shape(x.shape[1:], spacing, target)
    assert out_shape == (25, 17, 19) and tuple(got.shape) == (2,) + out_shape
    g = grid(x.shape[1:], out_shape, [t / s for s, t in zip(spacing, target)], order)
    for c in range(2):
        ref = ndi.map_coordinates(x[c].astype(np.float64), g, order=order, mode="mirror")
        err = float(np.abs(got[c].cpu().numpy().astype(np.float64) - ref).max())
        bound = {0: 0.0, 1: 16 * EPS * float(np.abs(x).max()), 3: 4.0 * restated["order3"]}[order]
        print(f"[resample] resample_volume order {order} channel {c}: error {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        assert torch.equal(got[c].view(torch.int32), F.resample_volume(xd[c], spacing, target, order).view(torch.int32))
    assert F.resample_volume(xd, spacing, spacing, order) is xd                 # identity spacing: the input itself
    same = F.ResampleTables(x.shape[1:], x.shape[1:], (1.0, 1.0, 1.0), order, xd.device)
    if order < 3:                                                               # and the kernels reproduce it bit for bit
        assert torch.equal(F.resample3d(xd, same).view(torch.int32), xd.view(torch.int32))


# ---------------------------------------------------------------------------------------------- labels
def label_volume(kind, shape, seed):
    rng = np.random.default_rng(seed)
    if kind == "smooth3":                                                       # three classes from thresholds of a smoothed field
        f = ndi.gaussian_filter(rng.standard_normal(shape), 2.0)
        lo, hi = np.percentile(f, [40, 75])
        return ((f > lo).astype(np.float32) + (f > hi).astype(np.float32))
    small = tuple(-(-n // 3) for n in shape)                                    # sixteen classes in random blocks of 3^3
    y = np.repeat(np.repeat(np.repeat(rng.integers(0, 16, small), 3, 0), 3, 1), 3, 2)
    return y[:shape[0], :shape[1], :shape[2]].astype(np.float32)


def onehot_oracle(y, out_shape, ratios):
    g = grid(y.shape, out_shape, ratios, 1)
    w = np.stack([ndi.map_coordinates((y == k).astype(np.float64), g, order=1, mode="nearest") for k in range(16)])
    top = np.sort(w, axis=0)
    return np.argmax(w, axis=0), top[-1] - top[-2]


LABEL_CASES = [((17, 23, 37), (0.5, 1.5, 0.75)), ((40, 9, 7), (1.25, 0.7, 1.0)), ((5, 4, 130), (1.0, 0.75, 1.25)), ((23, 37, 17), (0.7, 0.5, 1.5))]


@pytest.mark.parametrize("kind", ["smooth3", "blocks16"])
@pytest.mark.parametrize("shape,ratios", LABEL_CASES, ids=["x".join(map(str, c[0])) for c in LABEL_CASES])
def test_labels_linear_and_nearest(seg, shape, ratios, kind):
    F = seg.functional
    y = label_volume(kind, shape, 5)
    out_shape = case_out(shape, ratios)
    ref, margin = onehot_oracle(y, out_shape, ratios)
    keep = margin >= 1e-5
    left_out = 1.0 - float(keep.mean())
    assert left_out <= 0.01, f"the oracle leaves out {left_out:.2%} of the voxels: this case does not qualify"
    lin = F.ResampleTables(shape, out_shape, ratios, 1, torch.device("cuda", 0))
    near = F.ResampleTables(shape, out_shape, ratios, 0, torch.device("cuda", 0))
    for t, conv in ((torch.float32, np.float32), (torch.int64, np.int64)):
        yd = dev(y).to(t)
        got, bad = F.resample3d_labels(yd, lin, "linear")
        again, _ = F.resample3d_labels(yd, lin, "linear")
        assert got.dtype == t and int(bad) == 0 and torch.equal(got, again)
        assert np.array_equal(got.cpu().numpy()[keep], ref[keep].astype(conv))
        n, bad = F.resample3d_labels(yd, near, "nearest")
        idx = [c.astype(np.int64) for c in grid(shape, out_shape, ratios, 0)]
        assert int(bad) == 0 and np.array_equal(n.cpu().numpy(), y[idx[0], idx[1], idx[2]].astype(conv))
    print(f"[resample] labels {kind} {shape} -> {out_shape}: equal on {keep.mean():.4%} of the voxels, {left_out:.4%} below the 1e-5 margin")


def test_labels_exact_tie_gives_the_lowest_class_and_bad_labels_raise(seg):
    F = seg.functional
    # ratio 2 reads four voxels at 0.5 and 2.5: weights 0.5 / 0.5 exactly, the lower class on either side
    line = dev(np.array([3.0, 5.0, 5.0, 3.0], dtype=np.float32).reshape(1, 1, 4))
    t = F.ResampleTables((1, 1, 4), (1, 1, 2), (1.0, 1.0, 2.0), 1, line.device)
    assert t.frac_host.tolist() == [0.0, 0.0, 0.5, 0.5] and t.base_host.tolist() == [0, 0, 0, 2]
    for v in (line, line.to(torch.int64)):
        got, bad = F.resample3d_labels(v, t, "linear")
        assert got.cpu().reshape(-1).tolist() == [3, 3] and int(bad) == 0
    y = dev(label_volume("blocks16", (6, 7, 8), 2))
    assert torch.equal(F.resample_labels(y, (1, 1, 1), (1, 1, 1), "linear"), y) and torch.equal(F.resample_labels(y, (1, 1, 1), (1, 1, 1), "nearest"), y)
    for badv in (16.0, -1.0, 2.5, float("nan")):
        y2 = y.clone()
        y2[2, 3, 4] = badv
        for mode in ("linear", "nearest"):
            with pytest.raises(ValueError, match="not an integer in 0 .. 15"):
                F.resample_labels(y2, (1, 1, 1), (1, 1, 1), mode)
        _, bad = F.resample3d_labels(y2, F.ResampleTables((6, 7, 8), (6, 7, 8), (1.0, 1.0, 1.0), 0, y.device), "nearest")
        assert int(bad) == 1


@pytest.mark.parametrize("shape", [(3, 3, 5), (41, 41, 41), (104, 101, 100)], ids=lambda s: "x".join(map(str, s)))
def test_bad_label_count_in_every_block_regime(seg, shape):
    """the label kernel runs one block per 256 output voxels, at most 4096, and the count is reduced in two stages: one block with
    fewer than 64 live threads, 270 blocks (the finalize's ragged second trip), 4104 -> 4096 (a ragged grid-stride tail).  Bad labels
    at the first, the last and one interior voxel: exactly 3, and the volume itself comes back."""
    F = seg.functional
    y = label_volume("blocks16", shape, 4)
    y[0, 0, 0], y[-1, -1, -1], y[shape[0] // 2, shape[1] // 3, 1] = 16.0, -1.0, 17.0
    same = F.ResampleTables(shape, shape, (1.0, 1.0, 1.0), 0, torch.device("cuda", 0))
    for t in (torch.float32, torch.int64):
        yd = dev(y).to(t)
        got, bad = F.resample3d_labels(yd, same, "nearest")
        assert int(bad) == 3 and torch.equal(got, yd)


def blob(shape):
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    r = ((z - 13.3) / 9.0) ** 2 + ((y - 15.6) / 11.0) ** 2 + ((x - 14.2) / 7.5) ** 2 + 0.08 * np.sin(0.9 * x) * np.cos(0.7 * y)
    return (r < 1.0).astype(np.float32)


def test_round_trip_linear_keeps_more_dice_than_nearest(seg):
    F = seg.functional
    m = blob((28, 32, 30))
    md = dev(m)
    dice = {}
    for mode in ("linear", "nearest"):
        there = F.resample_labels(md, (0.75, 0.75, 0.75), (1.0, 1.0, 1.0), mode)
        back = F.resample_back_labels(there, m.shape, (0.75, 0.75, 0.75), (1.0, 1.0, 1.0), mode)
        assert tuple(there.shape) == (21, 24, 23) and tuple(back.shape) == m.shape
        b = back.cpu().numpy()
        dice[mode] = 2.0 * float((b * m).sum()) / float(b.sum() + m.sum())
    print(f"[resample] round trip 0.75 -> 1.0 -> 0.75 of a blob of {int(m.sum())} voxels: Dice linear {dice['linear']:.4f} nearest {dice['nearest']:.4f}")
    assert dice["linear"] > dice["nearest"]


# ---------------------------------------------------------------------------------------------- way back: resample + argmax
@pytest.mark.parametrize("K", [2, 4, 16])
@pytest.mark.parametrize("shape,ratios", [((17, 23, 37), (0.7, 1.25, 1.5)), ((5, 4, 130), (1.5, 0.5, 0.75)), ((2, 3, 1), (0.5, 0.75, 1.0))],
                         ids=["17x23x37", "5x4x130", "2x3x1"])
def test_way_back_argmax(seg, shape, ratios, K):
    """prob lives on the RESAMPLED grid `shape`; the way back reads it with ratio s / t = `ratios` into the original grid"""
    F = seg.functional
    logits = smooth(shape, 40 + K, channels=K).astype(np.float64) * 2.0
    p = np.exp(logits - logits.max(0))
    p = (p / p.sum(0)).astype(np.float32)
    out_shape = case_out(shape, ratios)
    spacing, target = ratios, (1.0, 1.0, 1.0)                                   # s / t = ratios
    g = grid(shape, out_shape, ratios, 1)
    ref = np.stack([ndi.map_coordinates(p[k].astype(np.float64), g, order=1, mode="nearest") for k in range(K)])
    top = np.sort(ref, axis=0)
    keep = (top[-1] - top[-2]) >= 2e-5
    left_out = 1.0 - float(keep.mean())
    assert left_out <= 0.01, f"the oracle leaves out {left_out:.2%} of the voxels: this case does not qualify"
    pd = dev(p)
    labels, prob = F.resample_back_argmax(pd, out_shape, spacing, target, return_probabilities=True)
    alone = F.resample_back_argmax(pd, out_shape, spacing, target)
    assert labels.dtype == torch.int64 and tuple(labels.shape) == (1,) + out_shape and tuple(prob.shape) == (K,) + out_shape
    assert torch.equal(labels, alone) and torch.equal(labels, F.resample_back_argmax(pd, out_shape, spacing, target))
    err, bound = float(np.abs(prob.cpu().numpy().astype(np.float64) - ref).max()), 16 * EPS * float(p.max())
    print(f"[resample] way back K={K} {shape} -> {out_shape}: probabilities {err:.3e} (bound {bound:.3e}), {left_out:.4%} below the 2e-5 margin")
    assert err <= bound and np.array_equal(labels.cpu().numpy()[0][keep], np.argmax(ref, axis=0)[keep])
    # every channel equals the order-1 gather of that channel, bitwise
    t = F.ResampleTables(shape, out_shape, ratios, 1, pd.device)
    assert torch.equal(prob.view(torch.int32), F.resample3d(pd, t).view(torch.int32))
    # logits-scale, all channels equal: nothing compares greater, label 0
    flat = torch.full((K,) + tuple(shape), 1.0e4, device="cuda")
    assert int(F.resample_back_argmax(flat, out_shape, spacing, target).abs().max()) == 0


# ---------------------------------------------------------------------------------------------- the queue
@pytest.fixture()
def cohort(tmp_path):
    d, g = tmp_path / "img", tmp_path / "gt"
    d.mkdir()
    g.mkdir()
    vols, spacings = {}, {"v0": (2.5, 0.7, 0.7), "v1": (1.0, 1.5, 0.75)}
    for i, (name, shape) in enumerate((("v0", (10, 30, 32)), ("v1", (22, 14, 28)))):
        x = smooth(shape, 60 + i) * (20.0 + 10 * i) + 50.0 * i
        y = label_volume("blocks16", shape, 70 + i) % 4
        np.save(str(d / f"{name}.npy"), x)
        np.save(str(g / f"{name}.npy"), y)
        vols[name] = (x, y)
    f = tmp_path / "spacings.csv"
    f.write_text("file,sz,sy,sx\n" + "".join(f"{n}.npy,{s[0]},{s[1]},{s[2]}\n" for n, s in spacings.items()))
    return str(d), str(g), str(f), vols, spacings


def count_windows(whole, xp, yp, ps):
    """how often the patch (xp, yp) occurs as a window of the (image, labels) pairs in ``whole``, compared bitwise"""
    hits = 0
    for xr, yr in whole:
        zs, ys, xs = np.nonzero(xr[:xr.shape[0] - ps[0] + 1, :xr.shape[1] - ps[1] + 1, :xr.shape[2] - ps[2] + 1].view(np.int32) == xp.view(np.int32)[0, 0, 0])
        for z, yy, xx in zip(zs, ys, xs):
            sl = (slice(z, z + ps[0]), slice(yy, yy + ps[1]), slice(xx, xx + ps[2]))
            hits += int(np.array_equal(xr[sl].view(np.int32), xp.view(np.int32)) and np.array_equal(yr[sl], yp))
    return hits


@pytest.mark.parametrize("variant", ["label_sampler", "clip_znorm", "order3_nearest"])
def test_queue_patches_come_from_the_resampled_volumes(seg, cohort, variant):
    from mi355seg import data
    from mi355seg.config import Config
    from mi355seg.intensity import IntensitySpec
    from mi355seg.resample import parse_resample
    F = seg.functional
    d, g, f, vols, spacings = cohort
    order, labels = (3, "nearest") if variant == "order3_nearest" else (1, "linear")
    spec = parse_resample(Config({"resample_spacing": "1,1,1", "resample_order": order, "resample_labels": labels, "spacing_file": f}))
    intensity = IntensitySpec("clip_znorm", (1.0, 99.0)) if variant == "clip_znorm" else None
    ps = (8, 8, 8)
    q = data.DevicePatchQueue(d, g, ps, 2, 4, torch.device("cuda", 0), seed=5, queue_length=4, samples_per_volume=2, intensity=intensity,
                              sampler="label" if variant == "label_sampler" else "uniform", resample=spec)
    whole = []
    for name, (x, y) in vols.items():
        xr = F.resample_volume(dev(x)[None], spacings[name], (1.0, 1.0, 1.0), order)
        assert tuple(xr.shape[1:]) == F.resampled_shape(x.shape, spacings[name], (1.0, 1.0, 1.0)) != x.shape
        xn = F.normalize_intensity(xr, intensity) if intensity else F.znormalize(xr)
        whole.append((xn[0].cpu().numpy(), F.resample_labels(dev(y), spacings[name], (1.0, 1.0, 1.0), labels).cpu().numpy()))
    seen = 0
    for batch in q:
        for xp, yp in zip(batch["source"]["data"].cpu().numpy(), batch["gt"]["data"].cpu().numpy()):
            assert xp.shape == (1,) + ps and count_windows(whole, xp[0], yp[0], ps) == 1
            seen += 1
    assert seen == 8


def test_queue_with_aug_samples_the_resampled_volume(seg, cohort):
    from mi355seg import data
    from mi355seg.resample import ResampleSpec, SpacingSource
    d, g, f, vols, spacings = cohort
    spec = ResampleSpec((1.0, 1.0, 1.0), 1, "linear", SpacingSource(table=spacings, path=f))
    q = data.DevicePatchQueue(d, g, (8, 8, 8), 2, 2, torch.device("cuda", 0), seed=5, queue_length=4, samples_per_volume=2, aug=True, resample=spec)
    for batch in q:
        assert tuple(batch["source"]["data"].shape) == (2, 1, 8, 8, 8) and bool(torch.isfinite(batch["source"]["data"]).all())
    shapes = sorted(tuple(x.shape[1:]) for x, _ in q.cache.values())
    assert set(shapes) <= {(25, 21, 23), (22, 21, 21)} and shapes


# ---------------------------------------------------------------------------------------------- predict.py
class Stub(torch.nn.Module):
    """two-class logits from the (normalised) image: enough structure for components and blending to matter"""

    def __init__(self):
        super().__init__()
        self.bias = torch.nn.Parameter(torch.tensor(0.2))

    def forward(self, x):
        s = x[:, :1]
        return torch.cat([self.bias - s, s - self.bias], 1)


@pytest.mark.parametrize("mode,extra", [("crop", []), ("hann", []), ("hann", ["config.save_probabilities=true"]), ("crop", ["config.keep_largest=1"]),
                                        ("crop", ["config.resample_labels=nearest", "config.resample_order=3"])],
                         ids=["crop", "hann", "hann_prob", "crop_keep_largest", "crop_nearest_order3"])
def test_predict_grades_on_the_original_grid(seg, cohort, tmp_path, mode, extra):
    import mi355seg.predict as P
    from mi355seg.config import compose, parse_patch_size
    from mi355seg.utils.metric import metric_with_spacing
    F = seg.functional
    d, g, f, vols, spacings = cohort
    conf_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(P.__file__))), "conf")
    common = ["config=unet", f"config.output_dir={tmp_path / 'logs'}", "config.patch_size=16,16,16", "config.batch_size=2", "config.ckpt=None",
              f"config.pred_data_path={d}", f"config.pred_gt_path={g}", "config.patch_overlap=4", f"config.overlap_mode={mode}"]
    keys = ["config.resample_spacing=1,1,1", f"config.spacing_file={f}"] + extra
    cfg = compose(conf_dir, common + keys + [f"config.hydra_path={tmp_path / 'on'}"], job_name="predict")
    parse_patch_size(cfg)
    model = Stub()
    rows = P.predict(cfg, model, log=lambda *_: None)
    order = 3 if "config.resample_order=3" in extra else 1
    labels = "nearest" if "config.resample_labels=nearest" in extra else "linear"
    assert [r["file"] for r in rows] == ["v0", "v1"]
    for row, (name, (x, y)) in zip(rows, vols.items()):
        sp = spacings[name]
        mask = np.load(os.path.join(cfg.hydra_path, f"{name}_pred.npy"))
        assert mask.shape == (1,) + x.shape and mask.dtype == np.uint8
        # the same walk by hand: forward, normalise, slide, back
        vol = P.znorm(F.resample_volume(dev(x)[None], sp, (1.0, 1.0, 1.0), order))
        if mode == "crop":
            m = P.sliding_window_predict(model.cuda(), vol, (16, 16, 16), (4, 4, 4), batch_size=2)
            want = F.resample_back_labels(m, x.shape, sp, (1.0, 1.0, 1.0), labels)
        else:
            m, prob = P.sliding_window_predict(model.cuda(), vol, (16, 16, 16), (4, 4, 4), batch_size=2, overlap_mode=mode, return_probabilities=True)
            want, pb = F.resample_back_argmax(prob, x.shape, sp, (1.0, 1.0, 1.0), return_probabilities=True)
            if extra:
                saved = np.load(os.path.join(cfg.hydra_path, f"{name}_prob.npy"))
                assert saved.shape == (2,) + x.shape and np.array_equal(saved, pb.cpu().numpy())
        if "config.keep_largest=1" in extra:
            want, _ = F.filter_components(want, min_voxels=0, keep_largest=1, connectivity=26, inplace=False)
            assert ndi.label(mask[0], np.ones((3, 3, 3)))[1] == 1
        assert np.array_equal(mask, want.cpu().numpy().astype(np.uint8)) and 0 < mask.sum() < mask.size
        gt = dev(y)[None].to(torch.int64)
        ref = dict(zip(P.METRIC_COLUMNS, metric_with_spacing(gt, dev(mask.astype(np.int64)), sp)))          # that volume's OWN spacing
        assert {k: row[k] for k in P.METRIC_COLUMNS} == ref
        print(f"[resample] predict {mode} {extra} {name}: dice {row['dice']:.4f} hs95 {row['hs95']:.3f} on the original grid {x.shape}")


def test_predict_without_the_key_is_unchanged_and_spacing_file_alone_grades_per_volume(seg, cohort, tmp_path):
    import mi355seg.predict as P
    from mi355seg.config import compose, parse_patch_size
    from mi355seg.utils.metric import metric_with_spacing
    d, g, f, vols, spacings = cohort
    conf_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(P.__file__))), "conf")
    # the cohort's volumes are smaller than a 16^3 patch along one axis on their own grids: patch 8
    common = ["config=unet", f"config.output_dir={tmp_path / 'logs'}", "config.patch_size=8,8,8", "config.batch_size=2", "config.ckpt=None",
              f"config.pred_data_path={d}", f"config.pred_gt_path={g}", "config.patch_overlap=2"]
    model = Stub()
    out = {}
    for tag, keys in (("plain", []), ("file", [f"config.spacing_file={f}"])):
        cfg = compose(conf_dir, common + keys + [f"config.hydra_path={tmp_path / tag}"], job_name="predict")
        parse_patch_size(cfg)
        out[tag] = (cfg, P.predict(cfg, model, log=lambda *_: None))
    for name, (x, y) in vols.items():
        want = P.sliding_window_predict(model.cuda(), P.znorm(dev(x)[None]), (8, 8, 8), (2, 2, 2), batch_size=2)          # the parent's walk
        for tag in out:
            assert np.array_equal(np.load(os.path.join(out[tag][0].hydra_path, f"{name}_pred.npy")), want.cpu().numpy().astype(np.uint8))
    assert sorted(out["plain"][1][0]) == ["dice", "file", "jaccard"]
    for row, (name, (x, y)) in zip(out["file"][1], vols.items()):
        mask = dev(np.load(os.path.join(out["file"][0].hydra_path, f"{name}_pred.npy")).astype(np.int64))
        assert {k: row[k] for k in P.METRIC_COLUMNS} == dict(zip(P.METRIC_COLUMNS, metric_with_spacing(dev(y)[None].to(torch.int64), mask, spacings[name])))


# ---------------------------------------------------------------------------------------------- refusals through the C-ABI
def test_refusals(seg):
    L = seg.lib()
    E = seg.Mi355SegError
    x = torch.zeros(2 * 4 * 4 * 4 + 1, device="cuda")
    y = torch.zeros(2 * 8 * 8 * 8, device="cuda")
    lab = torch.zeros(8 * 8 * 8, dtype=torch.int64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.zeros(L.query("mi355seg_resample3d_labels_ws_bytes"), dtype=torch.uint8, device="cuda")
    base_h = np.concatenate([np.arange(8) // 2] * 3).astype(np.int32)
    above, below = base_h + 1, base_h - 1                                       # kept alive: the calls get their addresses
    base, frac = dev(base_h), torch.zeros(24, device="cuda")
    X, Y, B, Fr, BH = x.data_ptr(), y.data_ptr(), base.data_ptr(), frac.data_ptr(), base_h.ctypes.data

    def pre(xp=X, dims=(2, 4, 4, 4), yp=Y, wsb=None):
        L.call("mi355seg_bspline3_prefilter_f32", xp, *dims, yp, ws.data_ptr(), ws.numel() if wsb is None else wsb, None)

    def gather(xp=X, dims=(2, 4, 4, 4), order=1, b=B, fr=Fr, bh=BH, yp=Y, out=(8, 8, 8)):
        L.call("mi355seg_resample3d_f32", xp, *dims, order, b, fr, bh, yp, *out, None)

    def labels(fn="f32", xp=X, mode=1, bh=BH, yp=Y, badp=None, wsp=None, wsb=None, out=(8, 8, 8)):
        L.call("mi355seg_resample3d_labels_" + fn, xp, 1, 4, 4, 4, mode, B, Fr, bh, yp, *out, bad.data_ptr() if badp is None else badp,
               ws.data_ptr() if wsp is None else wsp, ws.numel() if wsb is None else wsb, None)

    def argmax(K=2, pp=X, bh=BH, lp=None, po=None):
        L.call("mi355seg_resample3d_argmax_f32", pp, K, 4, 4, 4, B, Fr, bh, lab.data_ptr() if lp is None else lp, po, 8, 8, 8, None)

    for call in (pre, gather, labels, argmax):                                  # the arguments of the refusals below are otherwise fine
        call()
    with pytest.raises(E, match="prefilter: null"):
        pre(xp=None)
    with pytest.raises(E, match="prefilter: pointers must be 4-byte aligned"):
        pre(xp=X + 2)
    with pytest.raises(E, match="prefilter: sizes must be positive"):
        pre(dims=(2, 4, 0, 4))
    with pytest.raises(E, match="prefilter: the tensor has 2\\^31"):
        pre(dims=(2, 1024, 1024, 1024))
    with pytest.raises(E, match="workspace too small"):
        pre(wsb=L.query("mi355seg_bspline3_prefilter_ws_bytes", 2, 4, 4, 4) - 1)
    with pytest.raises(E, match="prefilter_axis: axis 3"):
        L.call("mi355seg_bspline3_prefilter_axis_f32", X, 2, 4, 4, 4, 3, Y, ws.data_ptr(), ws.numel(), None)
    with pytest.raises(E, match="prefilter_axis: axis 1 has length 1"):
        L.call("mi355seg_bspline3_prefilter_axis_f32", X, 2, 4, 1, 4, 1, Y, ws.data_ptr(), ws.numel(), None)
    with pytest.raises(E, match="resample3d: order 2"):
        gather(order=2)
    with pytest.raises(E, match="resample3d: null"):
        gather(fr=None)
    with pytest.raises(E, match="resample3d: null table"):
        gather(bh=None)
    with pytest.raises(E, match="resample3d: pointers must be 4-byte aligned"):
        gather(yp=Y + 1)
    with pytest.raises(E, match="resample3d: in place"):
        gather(yp=X)
    with pytest.raises(E, match="resample3d: sizes must be positive"):
        gather(out=(8, 0, 8))
    with pytest.raises(E, match="resample3d: a volume of 2\\^31"):
        gather(dims=(2, 1024, 1024, 1024))
    for where in (0, 9, 23):
        for v in (-1, 4):
            b2 = base_h.copy()
            b2[where] = v
            with pytest.raises(E, match="resample3d: a table base outside the source"):
                gather(bh=b2.ctypes.data)
    b2 = base_h.copy()
    b2[19] = 0                                                                  # x: 0 0 1 0 2 2 3 3
    with pytest.raises(E, match="resample3d: a descending table"):
        gather(order=3, bh=b2.ctypes.data)
    gather(order=1, bh=b2.ctypes.data)                                          # orders 0 and 1 take any table inside the source
    with pytest.raises(E, match="labels_f32: mode 2"):
        labels(mode=2)
    with pytest.raises(E, match="labels_i64: null"):
        labels(fn="i64", badp=0)
    with pytest.raises(E, match="labels_i64: misaligned"):
        labels(fn="i64", xp=X + 4)
    with pytest.raises(E, match="labels_f32: a table base outside"):
        labels(bh=above.ctypes.data)
    with pytest.raises(E, match="workspace too small"):
        labels(wsb=ws.numel() - 1)
    for K in (0, 17, -1):
        with pytest.raises(E, match=f"argmax: K = {K}"):
            argmax(K=K)
    with pytest.raises(E, match="argmax: null"):
        argmax(pp=None)
    with pytest.raises(E, match="argmax: misaligned"):
        argmax(lp=lab.data_ptr() + 4)
    with pytest.raises(E, match="argmax: in place"):
        argmax(po=X)
    with pytest.raises(E, match="argmax: a table base outside"):
        argmax(bh=below.ctypes.data)
    torch.cuda.synchronize()
