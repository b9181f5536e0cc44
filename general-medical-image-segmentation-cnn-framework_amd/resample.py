"""``config.resample_spacing``: bringing every volume to a common voxel spacing -- the host side.  Pure numpy, needs no GPU and no
library: the geometry (output shapes and the per-axis tables the kernels of csrc/resample.hip read), the keys' parser, the
per-volume spacing source, and an fp64 numpy implementation of the same definitions (the CPU plumbing branch of
``data.DevicePatchQueue``; the device path is ``functional.resample_volume`` / ``resample_labels`` / ``resample_back_*``).

UNPINNED restatements, as the rest of the data path (torchio and SimpleITK are absent from the build image and the reference holds no
fixture of its data pipeline; dataloader.py:10 imports ``tio.Resample`` and never wires it in).  Definitions (include/mi355seg.h,
"Resampling", holds them too), per axis independently, axis-aligned and corner-aligned, with input spacing s, target spacing t,
input length n and r = t / s:

  output length   n' = max(1, ceil(n * s / t - 1e-6))         (the 1e-6: 128 * 1.0 / 0.8 evaluates to 160.00000000000003)
  coordinate      c(o) = clamp((o + 0.5) * r - 0.5, 0, n - 1)
  way back        the same with r = s / t and the output length GIVEN (the original n)
  order 0         index floor(c + 0.5), half up
  order 1         linear between floor(c) and floor(c) + 1
  order 3         cubic B-spline: prefilter (pole sqrt(3) - 2, gain 6, whole-sample-symmetric boundary) along every axis longer than
                  1, then the 4-tap B-spline at c with mirrored taps: scipy.ndimage.map_coordinates(order=3, mode='mirror') on the
                  clamped coordinates
  labels nearest  order 0 (tio.Resample's rule for label maps)
  labels linear   per output voxel the trilinear weight of every class (the sum of the corner weights whose corner holds it); the
                  class of largest weight, the lowest class on a tie (nnU-Net's way, without the one-hot volume); labels must be
                  integers in 0 .. 15

Keys: ``config.resample_spacing=tz,ty,tx`` switches the feature on (absent or empty: off, nothing changes);
``config.resample_order=1|3`` (default 1); ``config.resample_labels=linear|nearest`` (default linear);
``config.spacing_file=/abs/spacings.csv`` with lines ``file,sz,sy,sx`` keyed by the ``.npy`` basename (a volume missing from it
raises); without that key every volume has ``config.spacing``; ``resample_spacing`` with neither raises."""
import csv
import math
import os

import numpy as np

from .config import absent

ORDERS = (0, 1, 3)
LABEL_MODES = ("nearest", "linear")
N_CLASSES = 16
POLE = math.sqrt(3.0) - 2.0
INIT_TERMS = 14                 # MI355SEG_BSPLINE_INIT_TERMS: |POLE|^14 < 2^-25, the device truncates the causal start there


# ---------------------------------------------------------------------------------------------- geometry
def _triple(v, what):
    t = tuple(float(a) for a in v)
    if len(t) != 3 or not all(np.isfinite(a) and a > 0 for a in t):
        raise ValueError(f"{what} must be three positive numbers, got {v!r}")
    return t


def resampled_shape(shape, spacing, target):
    """(D, H, W) of a volume of ``shape`` at ``spacing`` once it is resampled to ``target``: max(1, ceil(n * s / t - 1e-6)) per axis."""
    spacing, target = _triple(spacing, "spacing"), _triple(target, "target spacing")
    if len(shape) != 3 or any(int(n) < 1 for n in shape):
        raise ValueError(f"resampled_shape: expected three positive extents, got {tuple(shape)!r}")
    return tuple(max(1, int(math.ceil(int(n) * s / t - 1e-6))) for n, s, t in zip(shape, spacing, target))


def axis_coordinates(n_in, n_out, ratio):
    """float64 [n_out]: c(o) = clamp((o + 0.5) * ratio - 0.5, 0, n_in - 1)"""
    if int(n_in) < 1 or int(n_out) < 1 or not (np.isfinite(ratio) and ratio > 0):
        raise ValueError(f"resample: expected positive lengths and a positive ratio, got n_in {n_in} n_out {n_out} ratio {ratio}")
    o = np.arange(int(n_out), dtype=np.float64)
    return np.clip((o + 0.5) * float(ratio) - 0.5, 0.0, float(int(n_in) - 1))


def resample_axis_table(n_in, n_out, ratio, order):
    """The table of one axis: (base int32 [n_out], frac float32 [n_out]), decided in fp64.  Order 0: base = floor(c + 0.5), frac = 0.
    Orders 1 and 3: base = floor(c), frac = c - base; the kernels read base and min(base + 1, n_in - 1) at order 1 and the mirrored
    base - 1 .. base + 2 at order 3."""
    if order not in ORDERS:
        raise ValueError(f"resample: order must be one of {ORDERS}, got {order!r}")
    c = axis_coordinates(n_in, n_out, ratio)
    if order == 0:
        return np.floor(c + 0.5).astype(np.int32), np.zeros(int(n_out), dtype=np.float32)
    base = np.floor(c)
    return base.astype(np.int32), (c - base).astype(np.float32)


def mirror_index(i, n):
    """whole-sample-symmetric reflection of the integer array ``i`` into 0 .. n - 1"""
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i > n - 1, p - i, i)


def bspline3_weights(t):
    """the four cubic B-spline weights of the taps base - 1 .. base + 2 at fraction ``t`` (array) -> [4, len(t)]"""
    u = 1.0 - t
    return np.stack([u ** 3 / 6.0, t * t * (0.5 * t - 1.0) + 2.0 / 3.0, u * u * (0.5 * u - 1.0) + 2.0 / 3.0, t ** 3 / 6.0])


def axis_matrix(n_in, n_out, ratio, order, frac32=True):
    """float64 [n_out, n_in]: the linear operator of one axis (after the prefilter at order 3).  ``frac32``: the fraction rounded to
    fp32 as in the device's table, so host and device interpolate at the same coordinates."""
    base, frac = resample_axis_table(n_in, n_out, ratio, order)
    if not frac32:
        c = axis_coordinates(n_in, n_out, ratio)
        frac = c - np.floor(c) if order else frac
    base, frac = base.astype(np.int64), frac.astype(np.float64)
    m = np.zeros((int(n_out), int(n_in)), dtype=np.float64)
    rows = np.arange(int(n_out))
    if order == 0:
        m[rows, base] = 1.0
    elif order == 1:
        np.add.at(m, (rows, base), 1.0 - frac)
        np.add.at(m, (rows, np.minimum(base + 1, n_in - 1)), frac)
    else:
        w = bspline3_weights(frac)
        for k in range(4):
            np.add.at(m, (rows, mirror_index(base - 1 + k, n_in)), w[k])
    return m


def bspline3_prefilter_host(x, axes=(-1, -2, -3)):
    """cubic B-spline coefficients of ``x`` along ``axes`` in fp64 (scipy.ndimage.spline_filter(order=3, mode='mirror')): the exact
    mirrored causal start at every length; an axis of length 1 is left as it is"""
    c = np.array(x, dtype=np.float64)
    for ax in axes:
        n = c.shape[ax]
        if n < 2:
            continue
        v = np.moveaxis(c, ax, 0)                           # a view: the recursion below writes into c
        k = np.arange(2 * n - 2)
        zk = POLE ** k
        start = np.tensordot(zk, v[mirror_index(k, n)], axes=(0, 0)) / (1.0 - POLE ** (2 * n - 2))
        v *= 6.0
        v[0] = 6.0 * start
        for i in range(1, n):
            v[i] += POLE * v[i - 1]
        v[n - 1] = (POLE * v[n - 2] + v[n - 1]) * (POLE / (POLE * POLE - 1.0))
        for i in range(n - 2, -1, -1):
            v[i] = POLE * (v[i + 1] - v[i])
    return c


def _apply_axes(x, mats):
    """x [..., D, H, W] through the three per-axis operators"""
    y = np.asarray(x, dtype=np.float64)
    for ax, m in zip((-3, -2, -1), mats):
        y = np.moveaxis(np.tensordot(m, y, axes=(1, ax)), 0, ax)
    return y


def resample_to_host(x, out_shape, ratios, order):
    """``x`` [..., D, H, W] -> fp64 [..., *out_shape] with the per-axis ratios given (the forward and the backward direction)."""
    x = np.asarray(x)
    mats = [axis_matrix(n, no, r, order) for n, no, r in zip(x.shape[-3:], out_shape, ratios)]
    return _apply_axes(bspline3_prefilter_host(x) if order == 3 else x, mats)


def resample_host(x, spacing, target, order=1):
    """``functional.resample_volume`` in numpy fp64 (returned as float32): the CPU branch of the patch queue."""
    spacing, target = _triple(spacing, "spacing"), _triple(target, "target spacing")
    x = np.asarray(x)
    if spacing == target:
        return np.ascontiguousarray(x, dtype=np.float32)
    out_shape = resampled_shape(x.shape[-3:], spacing, target)
    return resample_to_host(x, out_shape, [t / s for s, t in zip(spacing, target)], order).astype(np.float32)


def check_labels_host(y, what="labels"):
    y = np.asarray(y)
    bad = ~((y >= 0) & (y <= N_CLASSES - 1) & (y == np.floor(y)))
    if bad.any():
        raise ValueError(f"{what}: {int(bad.sum())} voxels are not integers in 0 .. {N_CLASSES - 1}")


def resample_labels_to_host(y, out_shape, ratios, mode):
    if mode not in LABEL_MODES:
        raise ValueError(f"resample: label mode must be one of {LABEL_MODES}, got {mode!r}")
    y = np.asarray(y)
    check_labels_host(y, "resample_labels")
    if mode == "nearest":
        return resample_to_host(y, out_shape, ratios, 0).astype(y.dtype)
    mats = [axis_matrix(n, no, r, 1) for n, no, r in zip(y.shape[-3:], out_shape, ratios)]
    classes = np.unique(y)                                  # ascending: np.argmax's first maximum is the lowest class
    weights = np.stack([_apply_axes((y == k).astype(np.float64), mats) for k in classes])
    return classes[np.argmax(weights, axis=0)].astype(y.dtype)


def resample_labels_host(y, spacing, target, mode="linear"):
    """``functional.resample_labels`` in numpy fp64"""
    spacing, target = _triple(spacing, "spacing"), _triple(target, "target spacing")
    y = np.asarray(y)
    if spacing == target:
        check_labels_host(y, "resample_labels")
        return y.copy()
    out_shape = resampled_shape(y.shape[-3:], spacing, target)
    return resample_labels_to_host(y, out_shape, [t / s for s, t in zip(spacing, target)], mode)


# ---------------------------------------------------------------------------------------------- keys
def _parse_three(key, v):
    parts = v.strip("()[] ").split(",") if isinstance(v, str) else (list(v) if isinstance(v, (list, tuple)) else [v])
    try:
        if any(isinstance(p, bool) for p in parts):
            raise ValueError
        vals = [float(p) for p in parts]
        if len(vals) == 1:
            vals = vals * 3
        ok = len(vals) == 3 and all(np.isfinite(a) and a > 0 for a in vals)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"config.{key} must be three positive numbers z,y,x (or one for all three), got {v!r}")
    return tuple(vals)


def load_spacing_file(path):
    """``config.spacing_file`` -> {basename: (sz, sy, sx)}.  Lines ``file,sz,sy,sx``; empty lines, ``#`` comments and a header line
    whose first cell is ``file`` are skipped; the name is keyed by its basename with and without ``.npy``."""
    if not isinstance(path, str) or not os.path.isabs(path):
        raise ValueError(f"config.spacing_file must be an absolute path to a csv file, got {path!r}")
    if not os.path.isfile(path):
        raise ValueError(f"config.spacing_file={path}: no such file")
    table = {}
    with open(path, newline="") as fh:
        for ln, row in enumerate(csv.reader(fh), 1):
            row = [c.strip() for c in row]
            if not row or not any(row) or row[0].startswith("#") or (ln == 1 and row[0].lower() == "file"):
                continue
            try:
                if len(row) != 4:
                    raise ValueError
                sp = tuple(float(c) for c in row[1:])
                if not all(np.isfinite(a) and a > 0 for a in sp):
                    raise ValueError
            except ValueError:
                raise ValueError(f"config.spacing_file={path}: line {ln}: expected file,sz,sy,sx with three positive numbers, got {row!r}") from None
            name = os.path.basename(row[0])
            name = name[:-4] if name.endswith(".npy") else name
            if name in table:
                raise ValueError(f"config.spacing_file={path}: line {ln}: {name} is listed twice")
            table[name] = sp
    if not table:
        raise ValueError(f"config.spacing_file={path}: the file lists no volume")
    return table


class SpacingSource:
    """Where a volume's spacing comes from: ``table`` ({basename: triple}, from ``config.spacing_file``) or ``default`` (one triple,
    ``config.spacing``)."""

    def __init__(self, table=None, default=None, path=None):
        self.table, self.path = table, path
        self.default = None if default is None else _triple(default, "spacing")
        if table is None and self.default is None:
            raise ValueError("SpacingSource: neither a table nor a default spacing")

    def of(self, name):
        """the spacing of the volume ``name`` (a path or a basename, with or without .npy)"""
        if self.table is None:
            return self.default
        key = os.path.basename(str(name))
        key = key[:-4] if key.endswith(".npy") else key
        if key not in self.table:
            raise ValueError(f"config.spacing_file={self.path}: no line for the volume {key}")
        return self.table[key]

    def __repr__(self):
        return f"SpacingSource({len(self.table)} volumes from {self.path})" if self.table is not None else f"SpacingSource({self.default})"


def parse_spacing_source(config):
    """``config.spacing_file`` / ``config.spacing`` -> ``SpacingSource`` or None when neither key is set; the file wins."""
    f, sp = getattr(config, "spacing_file", None), getattr(config, "spacing", None)
    if not absent(f):
        return SpacingSource(table=load_spacing_file(f), path=f)
    if not absent(sp):
        return SpacingSource(default=_parse_three("spacing", sp))
    return None


class ResampleSpec:
    """One parsed ``config.resample_spacing`` setting: ``target`` (tz, ty, tx), ``order`` (1 or 3; 0 is accepted for library use),
    ``labels`` (``linear`` or ``nearest``) and ``spacings`` (a ``SpacingSource``)."""

    def __init__(self, target, order=1, labels="linear", spacings=None):
        self.target = _triple(target, "resample target spacing")
        if order not in ORDERS:
            raise ValueError(f"resample order must be one of {ORDERS}, got {order!r}")
        if labels not in LABEL_MODES:
            raise ValueError(f"resample label mode must be one of {LABEL_MODES}, got {labels!r}")
        if isinstance(spacings, (tuple, list)):
            spacings = SpacingSource(default=spacings)
        if not isinstance(spacings, SpacingSource):
            raise ValueError("resampling needs the volumes' spacing: config.spacing_file=/abs/spacings.csv or config.spacing=sz,sy,sx")
        self.order, self.labels, self.spacings = int(order), labels, spacings

    def __repr__(self):
        return f"ResampleSpec(target={self.target}, order={self.order}, labels={self.labels}, {self.spacings})"


def parse_resample(config):
    """``config.resample_spacing`` and its companions -> ``None`` (absent or empty: off) or a ``ResampleSpec``.  The one parser of
    these keys: ``data.make_loader`` and ``predict.predict`` both call it.  ``resample_order`` / ``resample_labels`` without
    ``resample_spacing`` raise, as does ``resample_spacing`` without a spacing source."""
    t, o, l = getattr(config, "resample_spacing", None), getattr(config, "resample_order", None), getattr(config, "resample_labels", None)
    if absent(t):
        for key, val in (("resample_order", o), ("resample_labels", l)):
            if not absent(val):
                raise ValueError(f"config.{key}={val!r} needs config.resample_spacing=tz,ty,tx")
        return None
    target = _parse_three("resample_spacing", t)
    order = 1
    if not absent(o):
        if isinstance(o, bool) or not (isinstance(o, int) or (isinstance(o, str) and o.strip().isdigit())) or int(o) not in (1, 3):
            raise ValueError(f"config.resample_order must be 1 or 3, got {o!r}")
        order = int(o)
    labels = "linear"
    if not absent(l):                                       # "none" reads as absent
        if not isinstance(l, str) or l not in LABEL_MODES:
            raise ValueError(f"config.resample_labels must be linear or nearest, got {l!r}")
        labels = l
    spacings = parse_spacing_source(config)
    if spacings is None:
        raise ValueError("config.resample_spacing needs the volumes' spacing: give config.spacing_file=/abs/spacings.csv "
                         "(lines file,sz,sy,sx) or config.spacing=sz,sy,sx")
    return ResampleSpec(target, order, labels, spacings)


def refuse_for_training(spec, data_path):
    if spec is not None and str(data_path) == "synthetic":
        raise ValueError("config.resample_spacing needs volumes with a spacing: with data_path=synthetic there is nothing to resample")
