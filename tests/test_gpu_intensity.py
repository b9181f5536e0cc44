"""csrc/intensity.hip on the device: exact percentiles by radix select, moments of the mapped masked voxels, the piecewise-linear
map, functional.normalize_intensity for every config.intensity mode, and the call sites (landmark training, the patch queue,
predict.py).

References are written out here in numpy fp64 (np.sort, np.percentile(x.astype(np.float64), q), explicit segment arithmetic) and do
not call the package's host implementation.

Exact checks: the two order statistics behind every percentile equal np.sort at the ranks floor(q / 100 * (m - 1)) and that + 1
clamped to m - 1 (compared by value, so -0.0 == 0.0); the masked count m; two runs give the same bits; in place == out of place.
Interpolated percentiles: |got - np.percentile| <= 1e-12 * max(1, |ref|).
Moments: the count is exact.  With an exact map (identity, clamp) every term map(x) - pivot is formed in fp64, a thread adds at most
4 * ceil(n / (4 * 256 * blocks)) <= 36 terms in sequence at the sizes here and the trees above it add 6 + 2 + 8 + 6 + 2 levels: a sum
of at most 64 roundings, |err| <= 2^-47 * sum|d|, so |mean err| <= 2^-47 * max|d| (+ one rounding of the mean itself) and the
variance sum d^2 - (sum d)^2 / c is off by at most 2^-45 * max d^2 (three such sums).  numpy's own pairwise sums are inside that.
With a sloped map every mapped value carries the fp32 error of the map, so mean and std are graded within the map's own bound.
Map and whole modes: per voxel, with j its segment in the fp64 reference,
    2^-24 * (|kx[j] * slope[j]| + |ky[j]|) + 2^-22 * max|ref|
(the shape of _znorm_bound in tests/test_gpu_losses.py: the knot and the value move by half an ulp when they become fp32, and the
subtraction, the slope and the fused multiply-add round the result), plus 2^-24 * |kx[k]| * |slope[k-1] - slope[k]| for a voxel that
the fp32 knot k puts on the other side of that knot (the map is continuous, so no voxel is left out).  Every test prints its measured
maximum beside the bound (pytest -rA); DESIGN.md section 4.18 holds the largest."""
import os

import numpy as np
import pytest
import torch

from oracle.fill import fill_module_

pytestmark = pytest.mark.gpu

QS = (0.0, 0.5, 1.0, 10.0, 20.0, 30.0, 40.0, 50.0, 60.0, 70.0, 80.0, 90.0, 99.0, 99.5, 100.0)
NYUL = (1.0, 10.0, 20.0, 30.0, 40.0, 50.0, 60.0, 70.0, 80.0, 90.0, 99.0)
TILE = 4096                    # one workgroup's tile of the histogram kernel: 256 threads x 4 loads x 4 voxels
LM = np.array([0.0, 8.0, 21.0, 30.0, 41.0, 50.0, 58.0, 71.0, 80.0, 93.0, 100.0])


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mi355seg
    mi355seg.lib()
    return mi355seg


def gauss(n, seed, offset=0.0, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(n) * scale + offset).astype(np.float32)


def ct_like(n, seed=3):
    """70 % of the voxels at -1024 (air), the rest N(40, 300)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(40.0, 300.0, n).astype(np.float32)
    x[rng.random(n) < 0.7] = -1024.0
    return x


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---------------------------------------------------------------------------------------------- order statistics and percentiles
def check_percentiles(F, tag, x, mask_gt=None, qs=QS, chunk=16):
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    v = x if mask_gt is None else x[x > np.float32(mask_gt)]
    s = np.sort(v)
    m = s.size
    xd = dev(x)
    worst = 0.0
    for i in range(0, len(qs), chunk):
        q = np.asarray(qs[i:i + chunk], dtype=np.float64)
        r = F.percentiles(xd, q, mask_gt)
        values, order, counts = r.values.cpu().numpy(), r.order.cpu().numpy(), r.counts.cpu().numpy()
        assert values.dtype == np.float64 and order.dtype == np.float32 and order.shape == (q.size, 2)
        assert counts.tolist() == [m, 0], f"{tag}: m {counts.tolist()} != {m}"
        lo = np.floor(q / 100.0 * (m - 1)).astype(np.int64)
        hi = np.minimum(lo + 1, m - 1)
        assert np.array_equal(order[:, 0], s[lo]) and np.array_equal(order[:, 1], s[hi]), \
            f"{tag}: order statistics {order.tolist()} != {np.stack([s[lo], s[hi]], 1).tolist()}"
        ref = np.percentile(v.astype(np.float64), q)
        err = float(np.max(np.abs(values - ref) / np.maximum(1.0, np.abs(ref))))
        worst = max(worst, err)
        assert err <= 1e-12, f"{tag}: percentile error {err:.3e} > 1e-12"
    print(f"[intensity] percentiles {tag}: n {x.size} m {m} largest relative error {worst:.3e} (bound 1e-12), order statistics exact")
    return worst


GAUSS_SIZES = [1, 2, 3, 5, 6, 7, 1023, 1025, TILE - 1, TILE, TILE + 1, 37 * 41 * 43, 4428244]      # 1024: one of a tile's four load rows


@pytest.mark.parametrize("n", GAUSS_SIZES)
def test_order_statistics_gaussian(seg, n):
    check_percentiles(seg.functional, f"gaussian n={n}", gauss(n, 11 + n, offset=3.0, scale=20.0))


def special_inputs():
    rng = np.random.default_rng(7)
    two = np.where(rng.random(1025) < 0.3, np.float32(-2.5), np.float32(7.25)).astype(np.float32)
    ints = rng.integers(-3, 4, 2001).astype(np.float32)                      # duplicates straddle every rank
    low_bits = (1.0 + rng.permutation(777) * 2.0 ** -23).astype(np.float32)  # only the last pass separates them
    assert np.unique(low_bits).size == 777
    mixed = np.concatenate([gauss(300, 5, scale=10.0), np.array([0.0, -0.0] * 20 + [1e-42, -1e-42] * 10 + [3e38, -3e38] * 3, np.float32)])
    mixed = rng.permutation(mixed).astype(np.float32)
    return {"all equal": np.full(1025, -1024.0, np.float32), "two values": two, "integers -3..3": ints, "lowest mantissa bits": low_bits,
            "mixed signs, zeros, denormals, 3e38": mixed, "ct-like": ct_like(37 * 41 * 43)}


@pytest.mark.parametrize("name", list(special_inputs()))
def test_order_statistics_special_inputs(seg, name):
    check_percentiles(seg.functional, name, special_inputs()[name])


def test_order_statistics_in_chunks_and_single(seg):
    x = gauss(5003, 2)
    check_percentiles(seg.functional, "chunks of 4", x, chunk=4)
    check_percentiles(seg.functional, "one at a time", x, qs=(50.0, 99.5), chunk=1)
    check_percentiles(seg.functional, "16 in one call", x, qs=QS + (33.3,), chunk=16)


@pytest.mark.parametrize("name", ["gaussian", "ct-like"])
def test_masked_percentiles(seg, name):
    x = gauss(37 * 41 * 43, 4, offset=100.0, scale=30.0) if name == "gaussian" else ct_like(37 * 41 * 43)
    mean = float(np.float32(x.astype(np.float64).mean()))
    check_percentiles(seg.functional, f"{name} x > mean", x, mask_gt=mean)
    check_percentiles(seg.functional, f"{name} x > -1024", x, mask_gt=-1024.0)
    check_percentiles(seg.functional, f"{name} x > max of the rest: two voxels", x, mask_gt=float(np.sort(x)[-3]))


def test_percentiles_refusals(seg):
    F, Err = seg.functional, seg.Mi355SegError
    from mi355seg.intensity import IDENTITY, IntensitySpec
    x = gauss(1021, 9)
    xd = dev(x)
    top = np.sort(x)
    for t, left in ((float(top[-1]), 0), (float(top[-2]), 1)):
        r = F.percentiles(xd, (50.0,), t)
        assert r.counts.cpu().tolist() == [left, 0]                      # the entry point reports m; the callers refuse it
        with pytest.raises(ValueError, match=f"the mask leaves {left} voxels"):
            F.volume_percentiles(xd, (50.0,), t)
        with pytest.raises(ValueError, match=f"the mask leaves {left} voxels"):
            F.normalize_intensity(xd, IntensitySpec("rescale", mask=t))
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[513] = bad
        assert F.percentiles(dev(y), (50.0,)).counts.cpu().tolist() == [1020, 1]
        for mask in ("none", "mean", 0.0):
            with pytest.raises(ValueError, match="non-finite"):
                F.normalize_intensity(dev(y), IntensitySpec("clip_znorm", mask=mask))
    with pytest.raises(Err, match="17 percentiles asked for"):
        F.percentiles(xd, np.linspace(0, 100, 17))
    with pytest.raises(Err, match="outside 0 .. 100"):
        F.percentiles(xd, (101.0,))
    with pytest.raises(Err, match="16-byte aligned"):
        F.percentiles(xd[1:], (50.0,))
    with pytest.raises(Err, match="16-byte aligned"):
        F.intensity_moments(xd[1:], IDENTITY)
    for fn in (lambda t: F.percentiles(t, (50.0,)), lambda t: F.normalize_intensity(t, IntensitySpec("rescale")),
               lambda t: F.intensity_map(t, IDENTITY)):
        with pytest.raises(Err, match="no CPU fallback"):
            fn(torch.from_numpy(x))
    for const_mode, text in (("rescale", "percentile range is empty"), ("clip_znorm", "standard deviation is 0")):
        with pytest.raises(ValueError, match=text):
            F.normalize_intensity(dev(np.full(1025, -1024.0, np.float32)), IntensitySpec(const_mode))
    with pytest.raises(ValueError, match="percentiles are all equal"):
        F.normalize_intensity(dev(np.full(1025, -1024.0, np.float32)), IntensitySpec("histogram", landmarks=LM))


def test_two_runs_give_the_same_bits(seg):
    F = seg.functional
    xd = dev(ct_like(100003))
    a = F.percentiles(xd, QS, -1024.0)
    a = [t.clone() for t in a]
    b = F.percentiles(xd, QS, -1024.0)
    assert all(torch.equal(s.view(torch.uint8), t.view(torch.uint8)) for s, t in zip(a, b))


# ---------------------------------------------------------------------------------------------- the fp64 restatement of the map
def seg_index(x64, kx):
    j = np.zeros(x64.shape, dtype=np.int64)
    for k in kx[1:-1]:
        j += k <= x64
    return j


def ref_map(x, kx, ky, slope, lo=-np.inf, hi=np.inf):
    """-> (y, per-voxel bound without the 2^-22 max|ref| term)"""
    kx, ky, slope = (np.asarray(a, dtype=np.float64) for a in (kx, ky, slope))
    xc = np.clip(x.astype(np.float64), lo, hi)
    j = seg_index(xc, kx)
    y = (xc - kx[j]) * slope[j] + ky[j]
    bound = 2.0 ** -24 * (np.abs(kx[j] * slope[j]) + np.abs(ky[j]))
    # the segment the fp32 kernel sees: fp32 voxel clamped to the fp32 bounds, against the fp32 knots
    xc32 = np.clip(x.astype(np.float32), np.float32(lo), np.float32(hi)).astype(np.float64)
    j32 = seg_index(xc32, kx.astype(np.float32).astype(np.float64))
    per_knot = np.zeros(kx.size)                      # per interior knot k: 2^-24 |kx[k]| |slope[k-1] - slope[k]|
    per_knot[1:-1] = 2.0 ** -24 * np.abs(kx[1:-1]) * np.abs(slope[:-1] - slope[1:])
    cum = np.cumsum(per_knot)                          # cum[b] - cum[a]: the knots a+1 .. b that lie between segment a and segment b
    return y, bound + cum[np.maximum(j, j32)] - cum[np.minimum(j, j32)]


def ref_mask(x, mask):
    v = x.astype(np.float64).ravel()
    if mask == "none":
        return v
    t = np.float64(np.float32(v.mean())) if mask == "mean" else np.float64(np.float32(mask))
    return v[v > t]


def nyul_knots(v, landmarks):
    p = np.percentile(v, NYUL)
    dp, dl = np.diff(p), np.diff(landmarks)
    slope = np.array([dl[i] / dp[i] if dp[i] > 0 else 0.0 for i in range(10)])
    return p, np.asarray(landmarks, dtype=np.float64), slope


def ref_mode(x, mode, mask, pct=(0.5, 99.5), out=(0.0, 1.0), landmarks=LM):
    """the fp64 restatement of one mode -> (y, per-voxel bound)"""
    v = ref_mask(x, mask)
    if mode == "rescale":
        lo, hi = np.percentile(v, pct)
        y, b = ref_map(x, (lo, hi), out, ((out[1] - out[0]) / (hi - lo),), lo, hi)
    elif mode == "clip_znorm":
        lo, hi = np.percentile(v, pct)
        c = np.clip(v, lo, hi)
        mean, std = c.mean(), c.std(ddof=1)
        y, b = ref_map(x, (mean, mean + std), (0.0, 1.0), (1.0 / std,), lo, hi)
    else:
        p, l, slope = nyul_knots(v, landmarks)
        if mode == "histogram_znorm":
            yv, _ = ref_map(v, p, l, slope)
            mean, std = yv.mean(), yv.std(ddof=1)
            l, slope = (l - mean) / std, slope / std
        y, b = ref_map(x, p, l, slope)
    return y, b + 2.0 ** -22 * float(np.max(np.abs(y)))


def grade(tag, got, ref, bound):
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, dtype=np.float64).reshape(ref.shape)
    err = np.abs(got - ref)
    share = float(np.max(err / bound))
    print(f"[intensity] {tag}: kernel error {float(err.max()):.3e}  bound {float(np.max(bound)):.3e}  largest share of its bound {share:.3f}  "
          f"(max|ref| {float(np.max(np.abs(ref))):.3e})")
    assert np.all(np.isfinite(got)), f"{tag}: result is not finite"
    assert np.all(err <= bound), f"{tag}: kernel error reaches {share:.3f} of its bound"
    return share


# ---------------------------------------------------------------------------------------------- moments
@pytest.mark.parametrize("n,offset", [(7, 0.0), (1021, 0.0), (100003, 1000.0), (4428244, 1000.0), (1025 * 33, -300.0), (300003, 1000.0), (2200003, 1000.0)])
def test_moments_exact_maps(seg, n, offset):
    """identity and clamp, with and without a mask: count exact, mean and std within the summation bound of the file's docstring.
    The grid is ceil((n / 4 + 1) / 256) blocks, at most 2048: n = 7 is one block with fewer than 64 live threads, 300003 gives 293
    blocks (the finalize's ragged second trip over the partials), 2200003 passes the cap with a ragged tail and n % 4 = 3."""
    F = seg.functional
    from mi355seg import intensity as I
    x = gauss(n, 19 + n) + np.float32(offset)
    xd = dev(x)
    x64 = x.astype(np.float64)
    lo, hi = np.percentile(x64, (5.0, 90.0))
    for tag, imap, t in (("identity", I.IDENTITY, None), ("identity, x > mean", I.IDENTITY, float(np.float32(x64.mean()))),
                         ("clamp 5..90", I.clamp_map(lo, hi), None), ("clamp 5..90, x > 10 %", I.clamp_map(lo, hi), float(np.float32(np.percentile(x64, 10.0))))):
        v = x64 if t is None else x64[x64 > np.float64(np.float32(t))]
        y = np.clip(v, np.float64(np.float32(imap.clip_lo)), np.float64(np.float32(imap.clip_hi)))   # the clamp bounds as the kernel holds them
        pivot = float(x[0])
        c, mean, var, s = F.intensity_moments(xd, imap, t, pivot).cpu().tolist()
        assert c == y.size
        d = np.max(np.abs(y - pivot))
        bm = 2.0 ** -47 * d + 2.0 ** -52 * abs(y.mean())
        bs = 2.0 ** -45 * d * d / y.std(ddof=1)
        em, es = abs(mean - y.mean()), abs(np.sqrt(var) - y.std(ddof=1))
        print(f"[intensity] moments n={n} offset={offset} {tag}: count {int(c)} mean error {em:.3e} (bound {bm:.3e}) std error {es:.3e} (bound {bs:.3e})")
        assert em <= bm and es <= bs
        assert abs(s - (y - pivot).sum()) <= 2.0 ** -47 * np.abs(y - pivot).sum()


def test_moments_sloped_map(seg):
    """an 11-knot map and the run-time knot count (nk = 5): the mapped values carry the map's fp32 error, mean and std its bound"""
    F = seg.functional
    from mi355seg.intensity import IntensityMap
    x = gauss(37 * 41 * 43, 8, offset=-300.0, scale=40.0)
    xd = dev(x)
    v = ref_mask(x, "mean")
    t = float(np.float32(x.astype(np.float64).mean()))
    p, l, slope = nyul_knots(v, LM)
    for tag, (kx, ky, sl) in (("nk=11", (p, l, slope)), ("nk=5", (p[::2][:5], l[::2][:5], np.diff(l[::2][:5]) / np.diff(p[::2][:5])))):
        y, b = ref_map(v, kx, ky, sl)
        bound = float(np.max(b)) + 2.0 ** -22 * float(np.max(np.abs(y)))
        c, mean, var, _ = F.intensity_moments(xd, IntensityMap(kx, ky, sl), t, float(y[0])).cpu().tolist()
        em, es = abs(mean - y.mean()), abs(np.sqrt(var) - y.std(ddof=1))
        print(f"[intensity] moments sloped map {tag}: count {int(c)} mean error {em:.3e} std error {es:.3e} (bound {bound:.3e}, 2 x for std)")
        assert c == v.size and em <= bound and es <= 2 * bound


# ---------------------------------------------------------------------------------------------- the map and the whole modes
SHAPES = [(2,), (7,), (1021,), (37, 41, 43), (2, 33, 35, 36)]
MODE_KW = [("rescale", {}), ("rescale", {"pct": (2.0, 90.0), "out": (-1.0, 3.0)}), ("clip_znorm", {}), ("histogram", {}), ("histogram_znorm", {})]


def mode_volume(shape):
    n = int(np.prod(shape))
    return gauss(n, 40 + n, offset=120.0, scale=35.0).reshape(shape)


@pytest.mark.parametrize("mask", ["none", "mean"])
@pytest.mark.parametrize("mode,kw", MODE_KW, ids=[m + ("_custom" if k else "") for m, k in MODE_KW])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(str(s) for s in sh) for sh in SHAPES])
def test_whole_modes(seg, shape, mode, kw, mask):
    F = seg.functional
    from mi355seg.intensity import IntensitySpec
    x = mode_volume(shape)
    spec = IntensitySpec(mode, kw.get("pct", (0.5, 99.5)), kw.get("out", (0.0, 1.0)), mask, LM)
    if ref_mask(x, mask).size < 2:                                    # n = 2 under the mean mask: one voxel is left
        with pytest.raises(ValueError, match="the mask leaves 1 voxels"):
            F.normalize_intensity(dev(x), spec)
        return
    ref, bound = ref_mode(x, mode, mask, **kw)
    got = F.normalize_intensity(dev(x), spec)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(shape)
    grade(f"{mode} {kw} mask={mask} {shape}", got, ref, bound)
    if mode == "rescale":
        a, b = (np.float32(o) for o in spec.out)
        assert float(got.min()) >= a and float(got.max()) <= b, f"rescale leaves [{a}, {b}]: {float(got.min())} .. {float(got.max())}"


def test_clip_znorm_full_range_is_znormalize(seg):
    F = seg.functional
    from mi355seg.intensity import IntensitySpec
    for shape, off in (((37, 41, 43), 1000.0), ((1021,), -300.0)):
        x = gauss(int(np.prod(shape)), 77, offset=off).reshape(shape)
        x64 = x.astype(np.float64)
        ref = (x64 - x64.mean()) / x64.std(ddof=1)
        bound = 2.0 ** -24 * abs(x64.mean()) / x64.std(ddof=1) + 2.0 ** -22 * np.max(np.abs(ref))       # _znorm_bound
        got = F.normalize_intensity(dev(x), IntensitySpec("clip_znorm", (0.0, 100.0)))
        zn = F.znormalize(dev(x))
        grade(f"clip_znorm 0,100 {shape} vs fp64", got, ref, np.full(ref.shape, bound))
        grade(f"znormalize {shape} vs fp64", zn, ref, np.full(ref.shape, bound))


@pytest.mark.parametrize("nk", [2, 5, 11, 12])
def test_map_in_place_and_every_knot_count(seg, nk):
    F = seg.functional
    from mi355seg.intensity import IntensityMap
    x = gauss(37 * 41 * 43 + 3, 6, offset=10.0, scale=50.0)
    kx = np.sort(np.random.default_rng(nk).normal(10.0, 50.0, nk))
    if nk >= 5:
        kx[2] = kx[1]                                                  # a zero-width segment
    ky = np.cumsum(np.random.default_rng(nk + 1).random(nk)) * 10.0
    slope = np.array([(ky[i + 1] - ky[i]) / (kx[i + 1] - kx[i]) if kx[i + 1] > kx[i] else 0.0 for i in range(nk - 1)])
    for lo, hi in ((-np.inf, np.inf), (-40.0, 75.0)):
        imap = IntensityMap(kx, ky, slope, lo, hi)
        ref, b = ref_map(x, kx, ky, slope, lo, hi)
        xd = dev(x)
        out = F.intensity_map(xd, imap)
        grade(f"map nk={nk} clip=({lo}, {hi})", out, ref, b + 2.0 ** -22 * np.max(np.abs(ref)))
        same = F.intensity_map(xd, imap, out=xd)
        assert same is xd and torch.equal(xd.view(torch.int32), out.view(torch.int32))


def test_ct_like_volume_with_equal_nyul_percentiles(seg):
    F = seg.functional
    from mi355seg.intensity import IntensitySpec
    x = ct_like(37 * 41 * 43).reshape(37, 41, 43)
    p = np.percentile(x.astype(np.float64), NYUL)
    assert np.all(p[:7] == -1024.0) and p[8] > -1024.0
    for mode in ("histogram", "histogram_znorm"):
        ref, bound = ref_mode(x, mode, "none")
        got = F.normalize_intensity(dev(x), IntensitySpec(mode, landmarks=LM))
        assert bool(torch.isfinite(got).all())
        grade(f"{mode} on the CT-like volume (p[0..6] = -1024)", got, ref, bound)
    air = F.normalize_intensity(dev(x), IntensitySpec("histogram", landmarks=LM))[dev(x) == -1024.0]
    j = int(np.sum(p[1:10] <= -1024.0))                                # air sits ON the last of the equal knots: exactly its landmark
    assert float(air.min()) == float(air.max()) == float(np.float32(LM[j]))


def test_histogram_with_own_landmarks_maps_p_to_l(seg):
    F = seg.functional
    from mi355seg import intensity as I
    x = gauss(37 * 41 * 43, 12, offset=300.0, scale=80.0)
    xd = dev(x)
    p = np.percentile(x.astype(np.float64), NYUL)
    own = (p - p[0]) / (p[10] - p[0]) * 100.0
    pd = F.volume_percentiles(xd, NYUL)
    assert np.max(np.abs(pd - p) / np.maximum(1.0, np.abs(p))) <= 1e-12
    imap = I.histogram_map(pd, own)
    got = F.intensity_map(dev(p.astype(np.float32)), imap).cpu().numpy().astype(np.float64)
    ref, b = ref_map(p.astype(np.float32), p, own, np.diff(own) / np.diff(p))
    grade("histogram, own landmarks: the map at fp32(p[i])", got, ref, b + 2.0 ** -22 * 100.0)
    moved = 2.0 ** -24 * np.abs(p) * np.max(np.diff(own) / np.diff(p))         # fp32(p[i]) is not p[i]: half an ulp along the steepest segment
    grade("histogram, own landmarks: p[i] -> l[i]", got, own, b + 2.0 ** -22 * 100.0 + moved)


# ---------------------------------------------------------------------------------------------- end to end
@pytest.fixture()
def cohort(tmp_path):
    """three small volumes; the label volume holds each voxel's own linear index, so a label patch says where it was cut"""
    d, g = tmp_path / "img", tmp_path / "gt"
    d.mkdir()
    g.mkdir()
    vols = []
    for i in range(3):
        shape = (20 + i, 22, 24 + 2 * i)
        v = gauss(int(np.prod(shape)), 60 + i, offset=80.0 * i + 20.0, scale=10.0 + 5 * i).reshape(shape)
        np.save(str(d / f"v{i}.npy"), v)
        np.save(str(g / f"v{i}.npy"), (np.arange(v.size, dtype=np.float32) + i * 2.0 ** 20).reshape(shape))
        vols.append(v)
    return str(d), str(g), vols


def test_train_landmarks_device_equals_cpu(seg, cohort):
    from mi355seg import data
    d, g, vols = cohort
    files = sorted(os.path.join(d, f) for f in os.listdir(d))
    for mask in ("none", "mean", 30.0):
        a, b = data.train_landmarks(files, mask, "cuda"), data.train_landmarks(files, mask, "cpu")
        err = float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))
        print(f"[intensity] train_landmarks mask={mask}: device vs numpy {err:.3e} (bound 1e-12)")
        assert a[0] == 0.0 and a[10] == 100.0 and np.all(np.diff(a) > 0) and err <= 1e-12


@pytest.mark.parametrize("mode", ["rescale", "clip_znorm", "histogram", "histogram_znorm", None])
def test_queue_patches_are_slices_of_the_normalised_volume(seg, cohort, mode):
    from mi355seg import data
    from mi355seg.intensity import IntensitySpec
    F = seg.functional
    d, g, vols = cohort
    spec = IntensitySpec(mode, mask="mean", landmarks=LM) if mode else None
    q = data.DevicePatchQueue(d, g, (8, 8, 12), 2, 6, torch.device("cuda", 0), seed=5, queue_length=6, samples_per_volume=3, intensity=spec)
    whole = [F.normalize_intensity(dev(v), spec) if spec else F.znormalize(dev(v)) for v in vols]       # without the key: today's z-score
    seen = 0
    for batch in q:
        for xp, yp in zip(batch["source"]["data"], batch["gt"]["data"]):
            first = int(yp[0, 0, 0, 0])
            i, lin = first >> 20, first & ((1 << 20) - 1)
            z, y, x = np.unravel_index(lin, vols[i].shape)
            want = whole[i][z:z + 8, y:y + 8, x:x + 12]
            assert torch.equal(xp[0].view(torch.int32), want.view(torch.int32))
            seen += 1
    assert seen == 12


def test_predict_cli_with_and_without_the_key(seg, tmp_path):
    from mi355seg.config import compose, parse_patch_size
    from mi355seg.intensity import IntensitySpec
    from mi355seg.predict import main as predict_main, sliding_window_predict, znorm
    from mi355seg.registry import build_model
    import mi355seg.predict as P
    F = seg.functional
    img, gt = tmp_path / "img", tmp_path / "gt"
    img.mkdir()
    gt.mkdir()
    x = ct_like(64 ** 3, seed=21).reshape(64, 64, 64)
    np.save(str(img / "case.npy"), x)
    np.save(str(gt / "case.npy"), (x > 100.0).astype(np.float32))
    conf_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(P.__file__))), "conf")
    common = ["config=unet", f"config.output_dir={tmp_path / 'logs'}", "config.patch_size=32,32,32", "config.batch_size=2",
              f"config.pred_data_path={img}", f"config.pred_gt_path={gt}", "config.patch_overlap=0"]
    cfg = compose(conf_dir, common, job_name="predict")
    parse_patch_size(cfg)
    torch.manual_seed(3)
    model = fill_module_(build_model(cfg))
    ckpt = str(tmp_path / "model.pt")
    torch.save({"model": model.state_dict()}, ckpt)
    common.append(f"config.ckpt={ckpt}")
    model = model.cuda().eval()
    vol = dev(x)[None]
    for name, keys, normed in (("clip", ["config.intensity=clip_znorm", "config.intensity_percentiles=1,99", "config.intensity_mask=-1024"],
                                F.normalize_intensity(vol, IntensitySpec("clip_znorm", (1.0, 99.0), mask=-1024.0))),
                               ("plain", [], znorm(vol))):
        cfg, rows = predict_main(common + [f"config.hydra_path={tmp_path / name}"] + keys)
        mask = np.load(os.path.join(cfg.hydra_path, "case_pred.npy"))
        want = sliding_window_predict(model, normed, (32, 32, 32), (0, 0, 0), batch_size=2)
        assert mask.shape == (1, 64, 64, 64) and np.array_equal(mask, want.cpu().numpy().astype(np.uint8)), name
        print(f"[intensity] predict {name}: {int(mask.sum())} of {mask.size} voxels labelled 1")
    assert torch.equal(znorm(vol), (vol - vol.mean()) / vol.std())           # the default path is predict.znorm, as before
