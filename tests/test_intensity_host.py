"""config.intensity on the host (no GPU, no library call): the keys' parser and every refusal, the knot / slope / clip tables of each
mode against hand-computed cases, the composition of the Nyul map with a z-score, landmark training and the CPU branch of the patch
queue.  The references are written out here in numpy fp64 (np.percentile, explicit segment arithmetic) and do not call the package's
host implementation; that implementation is checked against them."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from mi355seg import data
from mi355seg import intensity as I
from mi355seg.config import Config

NYUL = (1, 10, 20, 30, 40, 50, 60, 70, 80, 90, 99)


def cfg(**kw):
    return Config({"data_path": "/d", "gt_path": "/g", "patch_size": 8, "batch_size": 1, **kw})


# ---------------------------------------------------------------------------------------------- references (numpy fp64, stand-alone)
def ref_mask(x, mask):
    v = x.astype(np.float64).ravel()
    if mask == "none":
        return v
    t = np.float64(np.float32(v.mean())) if mask == "mean" else np.float64(np.float32(mask))
    return v[v > t]


def ref_piecewise(x, p, l):
    """the piecewise-linear function through (p[i], l[i]): end segments extrapolate, a zero-width segment has slope 0; the segment of
    x is the last one whose left INTERIOR knot is <= x"""
    x = x.astype(np.float64)
    y = np.empty_like(x)
    for idx, xv in np.ndenumerate(x):
        j = 0
        for i in range(1, len(p) - 1):
            if p[i] <= xv:
                j = i
        s = (l[j + 1] - l[j]) / (p[j + 1] - p[j]) if p[j + 1] > p[j] else 0.0
        y[idx] = (xv - p[j]) * s + l[j]
    return y


def ref_normalize(x, mode, mask="none", pct=(0.5, 99.5), out=(0.0, 1.0), landmarks=None):
    v = ref_mask(x, mask)
    x64 = x.astype(np.float64)
    if mode == "rescale":
        lo, hi = np.percentile(v, pct)
        return out[0] + (np.clip(x64, lo, hi) - lo) * (out[1] - out[0]) / (hi - lo)
    if mode == "clip_znorm":
        lo, hi = np.percentile(v, pct)
        c = np.clip(v, lo, hi)
        return (np.clip(x64, lo, hi) - c.mean()) / c.std(ddof=1)
    p = np.percentile(v, NYUL)
    y = ref_piecewise(x64, p, landmarks)
    if mode == "histogram":
        return y
    yv = ref_piecewise(v, p, landmarks)
    return (y - yv.mean()) / yv.std(ddof=1)


LM = np.array([0.0, 8.0, 21.0, 30.0, 41.0, 50.0, 58.0, 71.0, 80.0, 93.0, 100.0])


def volume(shape=(9, 10, 11), seed=0, offset=100.0, scale=30.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale + offset).astype(np.float32)


# ---------------------------------------------------------------------------------------------- parsing
def test_absent_empty_and_znorm_mean_todays_path():
    for c in (cfg(), cfg(intensity=None), cfg(intensity=""), cfg(intensity="None"), cfg(intensity="znorm")):
        assert I.parse_intensity(c) is None


def test_defaults_and_every_key(tmp_path):
    s = I.parse_intensity(cfg(intensity="rescale"))
    assert (s.mode, s.percentiles, s.out, s.mask, s.landmarks) == ("rescale", (0.5, 99.5), (0.0, 1.0), "none", None)
    s = I.parse_intensity(cfg(intensity="rescale", intensity_percentiles="1,99", intensity_out="-1,1", intensity_mask="mean"))
    assert (s.percentiles, s.out, s.mask) == ((1.0, 99.0), (-1.0, 1.0), "mean")
    s = I.parse_intensity(cfg(intensity="clip_znorm", intensity_percentiles=[0, 100], intensity_mask=-1024))
    assert (s.mode, s.percentiles, s.mask) == ("clip_znorm", (0.0, 100.0), -1024.0)
    assert I.parse_intensity(cfg(intensity="clip_znorm", intensity_mask="none")).mask == "none"
    assert I.parse_intensity(cfg(intensity="clip_znorm", intensity_mask="-0.5")).mask == -0.5
    f = str(tmp_path / "lm.npy")
    np.save(f, LM)
    for mode in ("histogram", "histogram_znorm"):
        s = I.parse_intensity(cfg(intensity=mode, intensity_landmarks=f))
        assert s.mode == mode and np.array_equal(s.landmarks, LM) and s.landmarks.dtype == np.float64


@pytest.mark.parametrize("kw, text", [
    (dict(intensity="zscore"), "config.intensity must be one of znorm, rescale, clip_znorm, histogram, histogram_znorm, got 'zscore'"),
    (dict(intensity=3), "config.intensity must be one of"),
    (dict(intensity="rescale", intensity_percentiles="5"), "config.intensity_percentiles must be two numbers p0,p1 with 0 <= p0 < p1 <= 100"),
    (dict(intensity="rescale", intensity_percentiles="99,1"), "config.intensity_percentiles must be two numbers"),
    (dict(intensity="rescale", intensity_percentiles="-1,50"), "config.intensity_percentiles must be two numbers"),
    (dict(intensity="rescale", intensity_percentiles="0,100.5"), "config.intensity_percentiles must be two numbers"),
    (dict(intensity="rescale", intensity_percentiles="a,b"), "config.intensity_percentiles must be two numbers"),
    (dict(intensity="rescale", intensity_out="1,1"), "config.intensity_out must be two numbers a,b with a < b"),
    (dict(intensity="rescale", intensity_out="0,1,2"), "config.intensity_out must be two numbers"),
    (dict(intensity="rescale", intensity_mask="median"), "config.intensity_mask must be none, mean or a number, got 'median'"),
    (dict(intensity="rescale", intensity_mask="nan"), "config.intensity_mask must be none, mean or a number"),
    (dict(intensity_percentiles="1,99"), "config.intensity_percentiles='1,99' needs config.intensity=rescale or clip_znorm (it is znorm)"),
    (dict(intensity="znorm", intensity_mask="mean"), "config.intensity_mask='mean' needs config.intensity=rescale or clip_znorm or histogram"),
    (dict(intensity="clip_znorm", intensity_out="0,1"), "config.intensity_out='0,1' needs config.intensity=rescale (it is clip_znorm)"),
    (dict(intensity="histogram", intensity_landmarks="/x.npy", intensity_percentiles="1,99"), "config.intensity_percentiles='1,99' needs"),
    (dict(intensity="rescale", intensity_landmarks="/x.npy"), "config.intensity_landmarks='/x.npy' needs config.intensity=histogram or histogram_znorm"),
    (dict(intensity="histogram"), "config.intensity=histogram needs config.intensity_landmarks=/abs/file.npy"),
    (dict(intensity="histogram_znorm", intensity_landmarks="rel/lm.npy"), "config.intensity_landmarks must be an absolute path"),
])
def test_refusal_texts(kw, text):
    with pytest.raises(ValueError) as e:
        I.parse_intensity(cfg(**kw))
    assert text in str(e.value)


def test_landmark_files(tmp_path):
    thirteen = np.array([0, 8, 21, 25.5, 30, 41, 50, 58, 71, 75.5, 80, 93, 100.0])
    f13, fbad, fdesc = (str(tmp_path / n) for n in ("l13.npy", "bad.npy", "desc.npy"))
    np.save(f13, thirteen)
    np.save(fbad, np.arange(12.0))
    np.save(fdesc, LM[::-1].copy())
    assert np.array_equal(I.parse_intensity(cfg(intensity="histogram", intensity_landmarks=f13)).landmarks, LM)   # entries 3 and 9 dropped
    for f in (fbad, fdesc):
        with pytest.raises(ValueError, match="expected 11 finite, increasing landmark values"):
            I.parse_intensity(cfg(intensity="histogram", intensity_landmarks=f))


def test_refused_with_aug_and_with_synthetic():
    with pytest.raises(ValueError, match="cannot be combined with config.aug=true: the augmentation kernel owns the normalisation"):
        data.make_loader(cfg(intensity="rescale", aug=True), "cpu", 1)
    with pytest.raises(ValueError, match="data_path=synthetic draws"):
        data.make_loader(cfg(intensity="clip_znorm", data_path="synthetic"), "cpu", 1)
    with pytest.raises(ValueError, match="config.aug=true"):
        data.DevicePatchQueue("/d", "/g", 8, 1, 1, "cpu", aug=True, intensity=I.IntensitySpec("rescale"))
    loader = data.make_loader(cfg(data_path="synthetic", intensity="znorm"), "cpu", 1)      # znorm stays allowed everywhere
    assert isinstance(loader, data.SyntheticPatches)


# ---------------------------------------------------------------------------------------------- the tables of each mode
def test_rescale_table():
    m = I.rescale_map(10.0, 50.0, -1.0, 1.0)
    assert (m.kx.tolist(), m.ky.tolist(), m.slope.tolist(), m.clip_lo, m.clip_hi) == ([10.0, 50.0], [-1.0, 1.0], [0.05], 10.0, 50.0)
    assert m(np.array([0.0, 10.0, 30.0, 50.0, 99.0])).tolist() == [-1.0, -1.0, 0.0, 1.0, 1.0]
    with pytest.raises(ValueError, match="percentile range is empty"):
        I.rescale_map(3.0, 3.0, 0.0, 1.0)


def test_rescale_fp32_table_stays_inside_the_range():
    """the slope handed to the kernel is rounded down until the fp32 formula cannot leave [a, b]"""
    rng = np.random.default_rng(5)
    for _ in range(200):
        lo, span = rng.normal(0, 1000), abs(rng.normal(0, 500)) + 1e-3
        a, b = sorted(rng.normal(0, 3, 2).astype(np.float32).astype(np.float64))
        if a == b:
            continue
        kx, ky, slope, clo, chi = I.rescale_map(lo, lo + span, a, b).f32()
        top = np.float32(np.float32(chi) - kx[0])                                   # x' - kx[0] at x' = clip_hi, rounded as the kernel does
        y = Fraction(float(top)) * Fraction(float(slope[0])) + Fraction(float(ky[0]))   # what the fused multiply-add rounds, exactly
        assert y <= Fraction(float(np.float32(b))) and np.float32(clo) == kx[0] and ky[0] == np.float32(a)
        s32 = (b - a) / (np.float64(np.float32(chi)) - np.float64(kx[0]))            # the slope between the ROUNDED knots
        assert abs(slope[0] - s32) <= 3 * np.spacing(np.float32(s32))


def test_zscore_and_clamp_tables():
    m = I.zscore_map(5.0, 2.0, 1.0, 9.0)
    assert (m.kx.tolist(), m.ky.tolist(), m.slope.tolist(), m.clip_lo, m.clip_hi) == ([5.0, 7.0], [0.0, 1.0], [0.5], 1.0, 9.0)
    assert m(np.array([-3.0, 5.0, 8.0, 20.0])).tolist() == [-2.0, 0.0, 1.5, 2.0]
    c = I.clamp_map(-2.0, 3.0)
    assert c(np.array([-5.0, 0.25, 7.0])).tolist() == [-2.0, 0.25, 3.0]
    with pytest.raises(ValueError, match="standard deviation is 0"):
        I.zscore_map(1.0, 0.0)


def test_histogram_table_with_equal_adjacent_percentiles():
    p = np.array([-1024.0] * 4 + [0.0, 10.0, 20.0, 30.0, 40.0, 50.0, 90.0])
    m = I.histogram_map(p, LM)
    want = [0.0, 0.0, 0.0, (41.0 - 30.0) / 1024.0, 0.9, 0.8, 1.3, 0.9, 1.3, 7.0 / 40.0]
    assert np.allclose(m.slope, want, rtol=1e-15, atol=0) and m.slope[:3].tolist() == [0.0, 0.0, 0.0]
    assert np.array_equal(m.kx, p) and np.array_equal(m.ky, LM) and m.clip_lo == -np.inf and m.clip_hi == np.inf
    x = np.array([-2000.0, -1024.0, -512.0, 0.0, 5.0, 50.0, 90.0, 130.0])
    want_y = [0.0, 30.0, 35.5, 41.0, 45.5, 93.0, 100.0, 107.0]            # below p[0]: slope 0; -1024 sits on knot 3; the end extrapolates
    assert np.allclose(m(x), want_y, rtol=1e-15, atol=1e-12)
    assert np.array_equal(m(x), ref_piecewise(x, p, LM))
    with pytest.raises(ValueError, match="percentiles are all equal"):
        I.histogram_map(np.full(11, 7.0), LM)


def test_histogram_then_zscore_is_one_map():
    x = volume().astype(np.float64)
    p = np.percentile(x, NYUL)
    h = I.histogram_map(p, LM)
    y = h(x)
    mean, std = y.mean(), y.std(ddof=1)
    one = h.then_zscore(mean, std)
    assert one.kx.size == 11 and np.array_equal(one.kx, h.kx)
    seq = (y - mean) / std
    assert np.max(np.abs(one(x) - seq)) <= 8 * np.finfo(np.float64).eps * max(1.0, np.max(np.abs(seq)))


# ---------------------------------------------------------------------------------------------- the numpy implementation against the references
MODES = [("rescale", {}), ("rescale", {"pct": (2.0, 90.0), "out": (-1.0, 3.0)}), ("clip_znorm", {}), ("clip_znorm", {"pct": (0.0, 100.0)}),
         ("histogram", {"landmarks": LM}), ("histogram_znorm", {"landmarks": LM})]


@pytest.mark.parametrize("mask", ["none", "mean", 95.0])
@pytest.mark.parametrize("mode, kw", MODES)
def test_host_implementation_matches_the_reference(mode, kw, mask):
    x = volume()
    spec = I.IntensitySpec(mode, kw.get("pct", (0.5, 99.5)), kw.get("out", (0.0, 1.0)), mask, kw.get("landmarks"))
    got = I.normalize_intensity_host(x, spec)
    ref = ref_normalize(x, mode, mask, **kw)
    assert got.dtype == np.float32 and got.shape == x.shape
    tol = 2.0 ** -23 * max(1.0, np.max(np.abs(ref)))             # the float32 result of an fp64 evaluation
    assert np.max(np.abs(got - ref)) <= tol


def test_clip_znorm_full_range_is_the_plain_zscore():
    x = volume()
    got = I.normalize_intensity_host(x, I.IntensitySpec("clip_znorm", (0.0, 100.0)))
    x64 = x.astype(np.float64)
    assert np.max(np.abs(got - (x64 - x64.mean()) / x64.std(ddof=1))) <= 2.0 ** -22


def test_host_refusals():
    x = volume()
    bad = x.copy()
    bad[1, 2, 3] = np.nan
    with pytest.raises(ValueError, match="1 non-finite voxels"):
        I.normalize_intensity_host(bad, I.IntensitySpec("rescale"))
    bad[1, 2, 3] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        I.normalize_intensity_host(bad, I.IntensitySpec("clip_znorm", mask="mean"))
    with pytest.raises(ValueError, match="the mask leaves 0 voxels"):
        I.normalize_intensity_host(x, I.IntensitySpec("rescale", mask=1e9))
    one = x.copy()
    one.ravel()[7] = 1e6
    with pytest.raises(ValueError, match="the mask leaves 1 voxels"):
        I.normalize_intensity_host(one, I.IntensitySpec("rescale", mask=1e5))
    const = np.full((4, 4, 4), 3.0, np.float32)
    with pytest.raises(ValueError, match="percentile range is empty"):
        I.normalize_intensity_host(const, I.IntensitySpec("rescale"))
    with pytest.raises(ValueError, match="standard deviation is 0"):
        I.normalize_intensity_host(const, I.IntensitySpec("clip_znorm"))
    with pytest.raises(ValueError, match="percentiles are all equal"):
        I.normalize_intensity_host(const, I.IntensitySpec("histogram", landmarks=LM))


# ---------------------------------------------------------------------------------------------- landmark training and the queue, CPU path
@pytest.fixture()
def cohort(tmp_path):
    d, g = tmp_path / "img", tmp_path / "gt"
    d.mkdir()
    g.mkdir()
    vols = []
    for i in range(3):
        v = volume((10, 12, 14), seed=10 + i, offset=50.0 * i, scale=10.0 + 5 * i)
        np.save(str(d / f"v{i}.npy"), v)
        np.save(str(g / f"v{i}.npy"), (v > v.mean()).astype(np.float32))
        vols.append(v)
    return str(d), str(g), vols


def test_train_landmarks_cpu(cohort):
    d, g, vols = cohort
    files = sorted(os.path.join(d, f) for f in os.listdir(d))
    for mask in ("none", "mean"):
        l = data.train_landmarks(files, mask, "cpu")
        assert l.dtype == np.float64 and l.shape == (11,) and l[0] == 0.0 and l[10] == 100.0 and np.all(np.diff(l) > 0)
        want = np.zeros(11)
        for v in vols:
            p = np.percentile(ref_mask(v, mask), NYUL)
            want += (p - p[0]) / (p[10] - p[0]) * 100.0
        assert np.max(np.abs(l - want / 3)) <= 1e-12 * 100.0


@pytest.mark.parametrize("mode, kw", MODES)
def test_queue_cpu_branch(cohort, mode, kw):
    d, g, vols = cohort
    spec = I.IntensitySpec(mode, kw.get("pct", (0.5, 99.5)), kw.get("out", (0.0, 1.0)), "mean", kw.get("landmarks"))
    q = data.DevicePatchQueue(d, g, 8, 2, 2, "cpu", seed=3, intensity=spec)
    plain = data.DevicePatchQueue(d, g, 8, 2, 2, "cpu", seed=3)
    for idx, v in enumerate(vols):
        x, _ = q._subject(idx)
        ref = ref_normalize(v, mode, "mean", **kw)
        assert x.dtype == torch.float32 and tuple(x.shape) == (1,) + v.shape
        assert np.max(np.abs(x[0].numpy() - ref)) <= 2.0 ** -23 * max(1.0, np.max(np.abs(ref)))
        xz, _ = plain._subject(idx)                              # without the key: the z-score of today
        vt = torch.from_numpy(v)[None]
        assert torch.equal(xz, (vt - vt.mean()) / vt.std())
    for a, b in zip(q, plain):                                   # the same patch placement either way
        assert a["source"]["data"].shape == b["source"]["data"].shape == (2, 1, 8, 8, 8)
        assert torch.equal(a["gt"]["data"], b["gt"]["data"])


def test_make_loader_passes_the_spec(cohort):
    d, g, _ = cohort
    q = data.make_loader(cfg(data_path=d, gt_path=g, intensity="rescale", intensity_out="0,2"), "cpu", 1)
    assert q.intensity.mode == "rescale" and q.intensity.out == (0.0, 2.0)
    assert data.make_loader(cfg(data_path=d, gt_path=g), "cpu", 1).intensity is None
