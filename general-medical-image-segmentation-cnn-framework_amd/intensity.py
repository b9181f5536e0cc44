"""``config.intensity``: per-volume intensity normalisation beyond the plain z-score -- the host side.  Pure numpy, needs no GPU and
no library: the keys' parser, the piecewise-linear map every mode reduces to, and an fp64 numpy implementation of the same
definitions (the CPU plumbing branch of ``data.DevicePatchQueue``; the device path is ``functional.normalize_intensity``, which
takes its percentiles and moments from csrc/intensity.hip and shares ``build_map`` with this file).

UNPINNED restatements, as the rest of the data path (torchio is absent from the build image and the reference holds no fixture of
its data pipeline; dataloader.py:19 imports RescaleIntensity and HistogramStandardization and wires neither in).  All elements of a
tensor are ONE volume, as ``functional.znormalize``.  Definitions, with v = the masked voxels (``config.intensity_mask``), m of them,
and P(q) = ``np.percentile(v, q)`` (method ``linear``):

``znorm`` (or the key absent / empty)   today's path, untouched: ``functional.znormalize`` / ``predict.znorm``.
``rescale``      tio.RescaleIntensity(out_min_max=(a, b), percentiles=(p0, p1)): lo = P(p0), hi = P(p1), x' = clamp(x, lo, hi),
                 y = a + (x' - lo) * (b - a) / (hi - lo).  ``config.intensity_percentiles=p0,p1`` (default 0.5,99.5; 0 <= p0 < p1
                 <= 100), ``config.intensity_out=a,b`` (default 0,1; a < b).  hi == lo raises (torchio warns and returns the input).
``clip_znorm``   x' = clamp(x, P(p0), P(p1)); y = (x' - mean) / std, mean and unbiased std over the CLAMPED masked voxels.
``histogram``    Nyul / tio.HistogramStandardization: p[0..10] = P(1, 10, 20, ..., 90, 99), l[0..10] the trained landmarks
                 (``config.intensity_landmarks=/abs/file.npy``: 11 float64 values; a 13-entry torchio file is accepted by dropping its
                 entries 3 and 9, the quartiles torchio itself skips).  y = the piecewise-linear function through (p[i], l[i]); the end
                 segments extrapolate; where p[i+1] == p[i] the segment has slope 0; no clamp.  p[10] == p[0] raises.
``histogram_znorm``  the same map followed by (y - mean) / std over the MAPPED masked voxels, composed into ONE map on the host.
``config.intensity_mask``  ``none`` (default): every voxel; ``mean``: the voxels with x > T, T = the mean of all voxels rounded to fp32
                 (ZNormalization.mean); a number T: the voxels with x > fp32(T).  The mask selects the voxels that enter the
                 statistics; the map is applied to EVERY voxel, as torchio does.
Raised as ``ValueError``: a non-finite voxel, fewer than two masked voxels, a zero range or zero standard deviation (torchio warns or
raises there; this package raises, as ``predict.znorm`` does)."""
import fractions
import os

import numpy as np

from .config import absent

MODES = ("znorm", "rescale", "clip_znorm", "histogram", "histogram_znorm")
NYUL_PERCENTILES = (1.0, 10.0, 20.0, 30.0, 40.0, 50.0, 60.0, 70.0, 80.0, 90.0, 99.0)
DEFAULT_PERCENTILES = (0.5, 99.5)
DEFAULT_OUT = (0.0, 1.0)


class IntensitySpec:
    """One parsed ``config.intensity`` setting: ``mode`` (never ``znorm``: that is ``None``), ``percentiles`` (p0, p1), ``out`` (a, b),
    ``mask`` (``"none"``, ``"mean"`` or a float) and ``landmarks`` (float64[11] or ``None``)."""

    def __init__(self, mode, percentiles=DEFAULT_PERCENTILES, out=DEFAULT_OUT, mask="none", landmarks=None):
        if mode not in MODES[1:]:
            raise ValueError(f"intensity mode must be one of {', '.join(MODES[1:])}, got {mode!r}")
        self.mode = mode
        self.percentiles = (float(percentiles[0]), float(percentiles[1]))
        self.out = (float(out[0]), float(out[1]))
        self.mask = mask if mask in ("none", "mean") else float(mask)
        self.landmarks = None if landmarks is None else check_landmarks(landmarks, "landmarks")
        if not 0.0 <= self.percentiles[0] < self.percentiles[1] <= 100.0:
            raise ValueError(f"intensity percentiles must be p0,p1 with 0 <= p0 < p1 <= 100, got {percentiles!r}")
        if not self.out[0] < self.out[1]:
            raise ValueError(f"intensity output range must be a,b with a < b, got {out!r}")
        if not np.isfinite(self.mask if not isinstance(self.mask, str) else 0.0):
            raise ValueError(f"intensity mask must be none, mean or a finite number, got {mask!r}")

    def __repr__(self):
        return (f"IntensitySpec({self.mode}, percentiles={self.percentiles}, out={self.out}, mask={self.mask}, "
                f"landmarks={'yes' if self.landmarks is not None else 'no'})")


def check_landmarks(values, what):
    """-> float64[11], increasing (equal neighbours allowed, not all equal); 13 torchio entries lose entries 3 and 9 (the quartiles)."""
    l = np.asarray(values, dtype=np.float64).reshape(-1)
    if l.size == 13:
        l = np.delete(l, (3, 9))
    if l.size != 11 or not np.all(np.isfinite(l)) or np.any(np.diff(l) < 0) or not l[10] > l[0]:
        raise ValueError(f"{what}: expected 11 finite, increasing landmark values (or torchio's 13), got {np.asarray(values).shape} "
                         f"{np.asarray(values).reshape(-1)[:13].tolist()}")
    return l


def load_landmarks(path):
    if not os.path.isabs(str(path)):
        raise ValueError(f"config.intensity_landmarks must be an absolute path to a .npy file, got {path!r}")
    return check_landmarks(np.load(path), f"config.intensity_landmarks={path}")


def _two_numbers(v):
    parts = v.strip("()[] ").split(",") if isinstance(v, str) else (list(v) if isinstance(v, (list, tuple)) else [v])
    if len(parts) != 2:
        raise ValueError
    out = [float(p) for p in parts]
    if not all(np.isfinite(o) for o in out) or any(isinstance(p, bool) for p in parts):
        raise ValueError
    return out


def parse_intensity(config):
    """``config.intensity`` and its companions (``intensity_percentiles``, ``intensity_out``, ``intensity_mask``,
    ``intensity_landmarks``) -> ``None`` (absent, empty or ``znorm``: today's path) or an ``IntensitySpec``.  The one parser of these
    keys: ``data.make_loader`` and ``predict.predict`` both call it.  A key given without the mode it belongs to raises ``ValueError``."""
    mode = getattr(config, "intensity", None)
    pct, out = getattr(config, "intensity_percentiles", None), getattr(config, "intensity_out", None)
    mask, lm = getattr(config, "intensity_mask", None), getattr(config, "intensity_landmarks", None)
    if not absent(mode) and (not isinstance(mode, str) or mode not in MODES):
        raise ValueError(f"config.intensity must be one of {', '.join(MODES)}, got {mode!r}")
    mode = "znorm" if absent(mode) else mode
    for key, val, owners in (("intensity_percentiles", pct, ("rescale", "clip_znorm")), ("intensity_out", out, ("rescale",)),
                             ("intensity_mask", mask, MODES[1:]), ("intensity_landmarks", lm, ("histogram", "histogram_znorm"))):
        if not absent(val) and mode not in owners:
            raise ValueError(f"config.{key}={val!r} needs config.intensity={' or '.join(owners)} (it is {mode})")
    if mode == "znorm":
        return None
    p, o = DEFAULT_PERCENTILES, DEFAULT_OUT
    if not absent(pct):
        try:
            p = _two_numbers(pct)
            ok = 0.0 <= p[0] < p[1] <= 100.0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"config.intensity_percentiles must be two numbers p0,p1 with 0 <= p0 < p1 <= 100, got {pct!r}")
    if not absent(out):
        try:
            o = _two_numbers(out)
            ok = o[0] < o[1]
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"config.intensity_out must be two numbers a,b with a < b, got {out!r}")
    m = "none"
    if not absent(mask):                                    # "none" itself reads as absent
        if isinstance(mask, str) and mask == "mean":
            m = "mean"
        else:
            try:
                m = float(mask)
                ok = np.isfinite(m) and not isinstance(mask, bool)
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"config.intensity_mask must be none, mean or a number, got {mask!r}")
    landmarks = None
    if mode in ("histogram", "histogram_znorm"):
        if absent(lm):
            raise ValueError(f"config.intensity={mode} needs config.intensity_landmarks=/abs/file.npy "
                             f"(tools/train_landmarks.py writes one)")
        landmarks = load_landmarks(lm)
    return IntensitySpec(mode, p, o, m, landmarks)


def refuse_for_training(spec, aug, data_path):
    """The two settings ``config.intensity`` (other than znorm) cannot be combined with, each with its reason."""
    if spec is None:
        return
    if aug:
        raise ValueError(f"config.intensity={spec.mode} cannot be combined with config.aug=true: the augmentation kernel owns the "
                         f"normalisation there (bias field -> z-score -> noise in one resampling launch); use config.aug=false")
    if str(data_path) == "synthetic":
        raise ValueError(f"config.intensity={spec.mode} needs volumes to normalise: data_path=synthetic draws N(0,1) patches that are "
                         f"their own volumes (use config.intensity=znorm)")


class IntensityMap:
    """The continuous piecewise-linear map of include/mi355seg.h: ``x' = clamp(x, clip_lo, clip_hi)``, ``j`` = the number of interior
    knots ``kx[1 .. nk-2]`` that are <= x', ``y = (x' - kx[j]) * slope[j] + ky[j]``.  fp64 here; ``f32()`` gives what the kernel takes."""

    def __init__(self, kx, ky, slope, clip_lo=-np.inf, clip_hi=np.inf, bounded=None):
        self.kx, self.ky, self.slope = (np.asarray(a, dtype=np.float64) for a in (kx, ky, slope))
        self.clip_lo, self.clip_hi, self.bounded = float(clip_lo), float(clip_hi), bounded
        if not (2 <= self.kx.size <= 12 and self.ky.size == self.kx.size and self.slope.size == self.kx.size - 1):
            raise ValueError(f"IntensityMap: expected 2 .. 12 knots with as many values and one slope fewer, got {self.kx.size}, "
                             f"{self.ky.size}, {self.slope.size}")

    def __call__(self, x):
        xc = np.clip(np.asarray(x, dtype=np.float64), self.clip_lo, self.clip_hi)
        j = np.zeros(xc.shape, dtype=np.int64)
        for k in self.kx[1:-1]:
            j += k <= xc
        return (xc - self.kx[j]) * self.slope[j] + self.ky[j]

    def then_zscore(self, mean, std):
        """the map followed by (y - mean) / std, as one map"""
        return IntensityMap(self.kx, (self.ky - mean) / std, self.slope / std, self.clip_lo, self.clip_hi)

    def f32(self):
        """(kx, ky, slope) as float32 arrays and the clip bounds as floats.  A ``bounded`` map (rescale) takes its slope from the
        ROUNDED knots, (fp32(b) - fp32(a)) / (fp32(hi) - fp32(lo)), so that the top of the range still lands on b, and then rounds
        it DOWN as far as it takes for the fp32 kernel formula to stay inside [fp32(a), fp32(b)]: the fused multiply-add rounds once
        and is monotone, so it is enough that (fp32(hi) - fp32(lo)) * slope + fp32(a) <= fp32(b) holds exactly (checked in rationals)."""
        kx, ky, slope = (a.astype(np.float32) for a in (self.kx, self.ky, self.slope))
        lo, hi = np.float32(self.clip_lo), np.float32(self.clip_hi)
        if self.bounded is not None:
            fr = fractions.Fraction
            top = np.float32(self.bounded[1])
            span = fr(float(np.float32(hi - lo)))                     # the kernel's x' - kx[0] at the top of the range, as it rounds it
            if hi > lo:
                slope[0] = np.float32((float(top) - float(ky[0])) / (float(hi) - float(lo)))
            while span * fr(float(slope[0])) + fr(float(ky[0])) > fr(float(top)):
                slope[0] = np.nextafter(slope[0], np.float32(0.0))
        return kx, ky, slope, float(lo), float(hi)


IDENTITY = IntensityMap((0.0, 1.0), (0.0, 1.0), (1.0,))


def clamp_map(lo, hi):
    """y = clamp(x, lo, hi): the identity segment with the clip bounds (exact in fp32: (x' - 0) * 1 + 0)"""
    return IntensityMap((0.0, 1.0), (0.0, 1.0), (1.0,), lo, hi)


def rescale_map(lo, hi, a, b):
    if not hi > lo:
        raise ValueError(f"intensity rescale: the percentile range is empty (lo = hi = {lo}): a constant volume cannot be rescaled")
    return IntensityMap((lo, hi), (a, b), ((b - a) / (hi - lo),), lo, hi, bounded=(a, b))


def zscore_map(mean, std, clip_lo=-np.inf, clip_hi=np.inf):
    if not std > 0.0:
        raise ValueError("intensity z-score: standard deviation is 0 for this volume (tio.ZNormalization raises here too)")
    return IntensityMap((mean, mean + std), (0.0, 1.0), (1.0 / std,), clip_lo, clip_hi)


def histogram_map(p, l):
    p, l = np.asarray(p, dtype=np.float64), np.asarray(l, dtype=np.float64)
    if not p[-1] > p[0]:
        raise ValueError(f"intensity histogram: the volume's percentiles are all equal ({p[0]}): a constant volume has no histogram "
                         f"to standardise")
    dp, dl = np.diff(p), np.diff(l)
    slope = np.where(dp > 0, dl / np.where(dp > 0, dp, 1.0), 0.0)
    return IntensityMap(p, l, slope)


def build_map(spec, percentiles, moments):
    """The map of ``spec`` for one volume.  ``percentiles(qs)`` -> float64 values of the masked voxels; ``moments(imap)`` ->
    (count, mean, unbiased variance) of ``imap(x)`` over the masked voxels.  Shared by the device path and the numpy one."""
    if spec.mode in ("rescale", "clip_znorm"):
        lo, hi = (float(v) for v in percentiles(spec.percentiles))
        if spec.mode == "rescale":
            return rescale_map(lo, hi, *spec.out)
        _, mean, var = moments(clamp_map(lo, hi))
        return zscore_map(mean, float(np.sqrt(var)), lo, hi)
    if spec.landmarks is None:
        raise ValueError(f"intensity {spec.mode}: no landmarks given")
    h = histogram_map(percentiles(NYUL_PERCENTILES), spec.landmarks)
    if spec.mode == "histogram":
        return h
    _, mean, var = moments(h)
    if not var > 0.0:
        raise ValueError("intensity z-score: standard deviation is 0 for this volume (tio.ZNormalization raises here too)")
    return h.then_zscore(mean, float(np.sqrt(var)))


def check_counts(m, nonfinite, what="intensity"):
    if nonfinite:
        raise ValueError(f"{what}: the volume holds {int(nonfinite)} non-finite voxels (NaN or infinity); clean the data first")
    if m < 2:
        raise ValueError(f"{what}: the mask leaves {int(m)} voxels, the statistics need at least 2")


def host_masked(x, mask, what="intensity"):
    """the masked voxels of ``x`` (any shape) as a flat float64 array, checked"""
    v = np.asarray(x, dtype=np.float64).reshape(-1)
    nonfinite = int(v.size - np.count_nonzero(np.isfinite(v)))
    if nonfinite:
        check_counts(v.size, nonfinite, what)
    if mask != "none":
        t = np.float32(v.mean()) if mask == "mean" else np.float32(mask)
        v = v[v > np.float64(t)]
    check_counts(v.size, 0, what)
    return v


def normalize_intensity_host(x, spec):
    """``functional.normalize_intensity`` in numpy fp64 (percentiles by ``np.percentile``), returned as float32 of x's shape."""
    x = np.asarray(x)
    v = host_masked(x, spec.mask)

    def moments(imap):
        y = imap(v)
        return y.size, float(y.mean()), float(y.var(ddof=1))

    imap = build_map(spec, lambda qs: np.percentile(v, np.asarray(qs, dtype=np.float64)), moments)
    return imap(x.astype(np.float64)).astype(np.float32)


def landmarks_from_percentiles(per_volume):
    """Nyul training: each volume's 11 percentiles rescaled affinely so p[0] -> 0 and p[10] -> 100, averaged over the volumes in fp64."""
    acc = np.zeros(len(NYUL_PERCENTILES), dtype=np.float64)
    for p in per_volume:
        p = np.asarray(p, dtype=np.float64)
        if not p[-1] > p[0]:
            raise ValueError(f"train_landmarks: a volume's percentiles are all equal ({p[0]})")
        acc += (p - p[0]) / (p[-1] - p[0]) * 100.0
    if not len(per_volume):
        raise ValueError("train_landmarks: no volumes")
    out = acc / len(per_volume)
    out[0], out[-1] = 0.0, 100.0
    return out
