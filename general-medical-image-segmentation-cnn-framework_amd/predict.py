"""``python predict.py config=unet config.ckpt=/abs/path`` -- the reference's sliding-window inference
(predict.py:62-183) on the MI355X path: registry + ``ckpt["model"]`` load (predict.py:79-81), per-volume
ZNormalization, grid patches with overlap, eval-mode forward, argmax, crop-mode aggregation, Dice/Jaccard.

The patch grid and the 'crop' aggregation restate torchio's GridSampler / GridAggregator (third-party, pinned
torchio==0.20.3 in the reference's requirements.txt, absent here): per axis the patch origins are
``range(0, size + 1 - patch, patch - overlap)`` plus a last origin flush with the border; each predicted patch
is cropped by ``overlap // 2`` on every side that does not touch the volume border before it is pasted.
NIfTI output (SimpleITK) is out of scope; volumes are ``.npy`` and metrics go to metrics.csv.

``config.spacing=sz,sy,sx`` (optional; one voxel spacing for every volume of the run) switches the metrics to the five numbers the
reference computes with ``metric(gt_t, pred_t, spacing)`` (predict.py:154): metrics.csv then holds ``file, precision, recall,
jaccard, dice, hs95`` and a last ``mean`` row (predict.py:186-200).  Without the key the file is ``file, jaccard, dice``, no mean row.

``config.keep_largest=K`` and / or ``config.min_component_voxels=N`` (optional) clean the aggregated mask by connected components on
the device (csrc/components.hip) before it is saved and graded: components below N voxels go, then only the K largest stay;
``config.connectivity`` = 6 | 18 | 26 (default 26).  components.csv (``file, components, kept, voxels_removed, largest``) is then
written beside metrics.csv.  Without the two keys nothing of this runs and no file is added.

``config.class_keep_largest`` and / or ``config.class_min_voxels`` (optional, with ``config.multiclass=true``) are the per-class form:
components are connected voxels of ONE class (functional.filter_components_by_class, every class in one labelling call), and each
key is one integer for every foreground class or ``k:v,k:v`` (``config.class_keep_largest=1:1,2:1,3:2``: one liver, one spleen, two
kidneys; a class that is not named is left alone; a single pair is written ``2:1,`` or ``{2: 1}``, as YAML reads ``2:1`` as 121).
components.csv is then ``file, class, components, kept, voxels_removed, largest``, one row per file and foreground class.

``config.overlap_mode=crop|average|hann|gaussian`` (optional, default crop) chooses how overlapping patches are aggregated.  ``crop`` is
the reference's mode: argmax labels, each voxel from one patch.  The other three blend the patches' class PROBABILITIES with a window
weight on the device (csrc/aggregate.hip) and take the argmax afterwards -- torchio's GridAggregator modes 'average' and 'hann', and an
nnU-Net-style Gaussian.  ``config.patch_overlap=oz,oy,ox`` (one number: all three axes; each even and smaller than the patch axis)
replaces the reference's (4, 4, 36).  ``config.save_probabilities=true`` (needs a blending mode) writes ``{name}_prob.npy``, float32
[K, D, H, W], beside ``{name}_pred.npy``.  Without the keys nothing changes and no file is added.

``config.tta=mirror`` (optional; absent, empty or ``none``: off) turns on mirror test-time augmentation, which the reference does
not have (its predict.py:133 calls the model once per patch): every patch is predicted under every combination of flips along
``config.tta_axes=z,y,x`` (any non-empty subset, default all three: 2, 4 or 8 forwards per patch), the class probabilities are
un-mirrored and averaged, and the argmax comes last.  The mirrors happen inside the gather and accumulate launches (csrc/api.hip,
csrc/aggregate.hip); in a blending mode the flips are the outer loop over the grid, in crop mode they are averaged per patch before
its labels are pasted.  Output files and their columns do not change.

``config.resample_spacing=tz,ty,tx`` (optional; the keys and definitions are in resample.py) resamples every image to that spacing
on the device (csrc/resample.hip) before it is normalised, runs the sliding window on the resampled grid and brings the result back
to the ORIGINAL grid before components, saving and metrics: in crop mode the mask through the label resampler
(``config.resample_labels``), in a blending mode the class probabilities by trilinear interpolation with the argmax in the same
launch.  ``config.spacing_file=/abs/spacings.csv`` (lines ``file,sz,sy,sx``) gives every volume its own spacing, for the resampling
and for the metrics; with it and without ``resample_spacing`` the volumes are still graded each with its own spacing.
"""
import csv
import glob
import os
import sys

import numpy as np
import torch

from . import functional as F
from .config import absent as _absent, compose, parse_patch_size
from .engine import mixed_precision_dtype
from .intensity import parse_intensity
from .resample import parse_resample, parse_spacing_source
from .registry import build_model
from .models.three_d.IS import set_band_split
from .utils.metric import class_metrics_from_counts, metric_from_counts, metric_with_spacing


def grid_locations(size, patch, overlap):
    """All patch origins [(z, y, x)] covering a volume of ``size`` (torchio GridSampler._get_patches_locations).
    UNPINNED restatement (this function and the crop aggregation below): torchio's GridSampler / GridAggregator are third-party code
    that is absent here and for which the reference holds no fixtures; restated from torchio 0.20.3 and property-tested
    (tests/test_predict_grid.py).  What IS pinned on this row is the arithmetic of the patches (test_gpu_unet.py::test_inference_path_*)."""
    axes = []
    for s, p, o in zip(size, patch, overlap):
        if p > s:
            raise ValueError(f"patch size {p} larger than the volume extent {s}")
        if o >= p or o % 2:
            raise ValueError(f"patch overlap {o} must be even and smaller than the patch size {p}")
        idx = list(range(0, s + 1 - p, p - o))
        if idx[-1] != s - p:
            idx.append(s - p)
        axes.append(idx)
    return [(z, y, x) for z in axes[0] for y in axes[1] for x in axes[2]]


def crop_window(loc, patch, size, overlap):
    """(src slices into the patch, dst slices into the volume) of torchio's GridAggregator overlap_mode='crop'."""
    src, dst = [], []
    for l, p, s, o in zip(loc, patch, size, overlap):
        a = o // 2 if l != 0 else 0
        b = o // 2 if l + p != s else 0
        src.append(slice(a, p - b))
        dst.append(slice(l + a, l + p - b))
    return tuple(src), tuple(dst)


def window_table(size, patch, overlap):
    """int32 [P, 9] rows (origin z, y, x, crop lo z, y, x, crop hi z, y, x -- the crop window in PATCH coordinates, hi exclusive) for
    the device-side gather / paste kernels, patches in torchio's order.  torchio's aggregator adds the cropped patches one after the
    other, so where two crop windows overlap (only the border-flush last patch of an axis overlaps its predecessor by more than
    ``overlap``) the LATER patch wins; the table clips every window at the start of its successor's window instead, which gives
    the same volume with disjoint windows -- the paste is then one launch with no ordering between patches."""
    axes = []
    for s, p, o in zip(size, patch, overlap):
        if p > s:
            raise ValueError(f"patch size {p} larger than the volume extent {s}")
        if o >= p or o % 2:
            raise ValueError(f"patch overlap {o} must be even and smaller than the patch size {p}")
        idx = list(range(0, s + 1 - p, p - o))
        if idx[-1] != s - p:
            idx.append(s - p)
        lo = [l + (o // 2 if l != 0 else 0) for l in idx]
        hi = [l + p - (o // 2 if l + p != s else 0) for l in idx]
        for i in range(len(idx) - 1):
            hi[i] = min(hi[i], lo[i + 1])
        axes.append([(l, a - l, b - l) for l, a, b in zip(idx, lo, hi)])
    rows = [(z[0], y[0], x[0], z[1], y[1], x[1], z[2], y[2], x[2]) for z in axes[0] for y in axes[1] for x in axes[2]]
    return np.asarray(rows, dtype=np.int32)


def window_weights(mode, patch):
    """The separable patch window of a blending mode: three fp64 arrays (wz, wy, wx) of the patch extents; the weight of patch voxel
    (z, y, x) is wz[z] * wy[y] * wx[x].
    ``average``: ones (torchio GridAggregator overlap_mode='average').
    ``hann``: 0.5 * (1 - cos(2 pi (k + 1) / (p + 1))), k = 0 .. p-1: torchio's ``torch.hann_window(p + 2, periodic=False)[1:-1]``
    per axis (GridAggregator._get_hann_window, torchio 0.20.3; UNPINNED like the grid above, checked against torch.hann_window).
    ``gaussian``: exp(-0.5 * ((k - (p - 1) / 2) / (p / 8))^2).  This one is THIS PROJECT'S OWN definition, not a restatement: an
    importance map in the manner of nnU-Net's (sigma = patch / 8) written as a product of per-axis Gaussians, without nnU-Net's
    rescaling and clamping of the 3-D map."""
    if mode not in F.OVERLAP_MODES or mode == "crop":
        raise ValueError(f"window_weights: mode must be one of {F.OVERLAP_MODES[1:]}, got {mode!r}")
    out = []
    for p in ((patch,) * 3 if isinstance(patch, int) else tuple(patch)):
        k = np.arange(int(p), dtype=np.float64)
        if mode == "average":
            out.append(np.ones(int(p), dtype=np.float64))
        elif mode == "hann":
            out.append(0.5 * (1.0 - np.cos(2.0 * np.pi * (k + 1.0) / (p + 1.0))))
        else:
            out.append(np.exp(-0.5 * ((k - (p - 1) / 2.0) / (p / 8.0)) ** 2))
    return tuple(out)


def axis_weight_sums(size, patch, overlap, weights):
    """The normaliser of a blending mode, per axis: three fp64 arrays (sz, sy, sx) of the volume extents, sz[z] = the sum of wz over
    the z-origins whose patch covers z.  The grid is a product of per-axis origins and the window a product of per-axis weights, so
    torchio's accumulated weight volume is sz[z] * sy[y] * sx[x] and need not be kept."""
    locs = grid_locations(size, patch, overlap)
    out = []
    for axis, (s, p, w) in enumerate(zip(size, patch, weights)):
        acc = np.zeros(int(s), dtype=np.float64)
        for l in sorted({loc[axis] for loc in locs}):
            acc[l:l + p] += np.asarray(w, dtype=np.float64)
        out.append(acc)
    return tuple(out)


def tta_axis_sums(sums, flips):
    """The normaliser of a blend that holds ``len(flips)`` predictions of every patch: (F * sz, sy, sx).  F is a power of two, so in
    any float format (F * sz[z] * sy[y]) * sx[x] is exactly F times the un-augmented normaliser."""
    sz, sy, sx = sums
    return len(flips) * sz, sy, sx


def check_tta_flips(tta_flips):
    """``tta_flips`` of sliding_window_predict -> the tuple of flip codes, or None for no augmentation (None or (0,)).  A tuple must be
    what functional.tta_flip_codes gives for some axes: ascending codes 0..7, the identity first, closed under the axes they use."""
    if tta_flips is None:
        return None
    flips = tuple(tta_flips)
    if any(isinstance(f, bool) or not isinstance(f, int) or not 0 <= f <= 7 for f in flips):
        raise ValueError(f"tta_flips must hold integers in 0..7 (bit 2 mirrors z, bit 1 y, bit 0 x), got {tta_flips!r}")
    mask = 0
    for f in flips:
        mask |= f
    if flips != tuple(c for c in range(8) if c & ~mask == 0):
        raise ValueError(f"tta_flips must be the ascending codes of every flip combination of some axes (functional.tta_flip_codes), "
                         f"got {tta_flips!r}")
    return None if flips == (0,) else flips


def _forward(model, x, dtype):
    with F.autocast(dtype or F.compute_dtype()):
        if getattr(model, "takes_frequency_bands", False):           # predict.py:128-131 (IS: first output only)
            from .models.three_d.IS import frequency_bands
            logits, _ = model(x, *frequency_bands(x, impl=getattr(model, "band_split", "fft")))
            return logits
        return model(x)


def _predict_tta(model, volume, ps, table, flips, batch_size, dtype, weights, sums, return_probabilities, out):
    """sliding_window_predict with mirror test-time augmentation; crop mode: ``weights`` is None and ``out`` the zeroed label volume."""
    from ._lib import lib
    C, D, H, W = volume.shape
    P, dev = table.shape[0], volume.device
    if weights is not None:
        # the flips are the OUTER loop: per accumulator element the additions happen in (flip, patch) order whatever the batch size
        acc = None
        for f in flips:
            for i in range(0, P, batch_size):
                nb = min(batch_size, P - i)
                logits = _forward(model, F.gather_patches(volume, table, i, nb, ps, flip=f), dtype)
                if acc is None:
                    acc = torch.zeros((logits.shape[1], D, H, W), dtype=torch.float32, device=dev)
                F.aggregate_patches(acc, logits.to(torch.float32), table, i, weights, flip=f)
        return F.aggregate_finalize(acc, tta_axis_sums(sums, flips), probabilities=return_probabilities)
    # crop mode: the F un-mirrored softmaxes of a batch are summed (ascending flip code) in a buffer that the accumulate kernel sees
    # as a volume [K, count * pd, ph, pw] -- patch b at origin (b * pd, 0, 0), windows of ones -- then argmax and paste as without TTA
    L, st = lib(), torch.cuda.current_stream().cuda_stream
    rows = np.zeros((min(batch_size, P), 9), dtype=np.int32)
    rows[:, 0] = np.arange(rows.shape[0]) * ps[0]
    stack = torch.from_numpy(rows).to(dev)
    ones = [torch.ones(p, dtype=torch.float32, device=dev) for p in ps]
    for i in range(0, P, batch_size):
        nb = min(batch_size, P - i)
        buf = None
        for f in flips:
            logits = _forward(model, F.gather_patches(volume, table, i, nb, ps, flip=f), dtype)
            if buf is None:
                buf = torch.zeros((logits.shape[1], nb * ps[0], ps[1], ps[2]), dtype=torch.float32, device=dev)
            F.aggregate_patches(buf, logits.to(torch.float32), stack, 0, ones, flip=f)
        labels = F.argmax_channels(buf[None])                            # int64 [1, 1, nb * pd, ph, pw]: the batch's label maps in order
        L.call("mi355seg_paste_labels_i64", labels.data_ptr(), table.data_ptr(), i, nb, ps[0], ps[1], ps[2], out.data_ptr(), D, H, W, st)
    return out


@torch.no_grad()
def sliding_window_predict(model, volume, patch_size, overlap=(4, 4, 36), batch_size=1, dtype=None, overlap_mode="crop",
                           return_probabilities=False, tta_flips=None):
    """volume: float tensor [C, D, H, W] on the GPU -> int64 label volume [1, D, H, W] (argmax over classes).
    ``dtype`` = torch.bfloat16 runs the forward under mi355seg.autocast (``config.mixed_precision=bf16``).
    Device-resident: the window table is uploaded once, each batch is one gather launch (mi355seg_gather_patches_f32), the
    eval-mode forward (BatchNorm folded into the convolutions), the channel argmax and one paste launch
    (mi355seg_paste_labels_i64); no host loop over patches, no host copies.
    ``overlap_mode`` = average | hann | gaussian blends instead: per batch one launch adds the window-weighted softmax of the logits
    into an fp32 accumulator [K, D, H, W] (mi355seg_aggregate_patches_f32, in place of the argmax and the paste), and one launch per
    volume takes the argmax of the blend (mi355seg_aggregate_finalize_f32).  ``return_probabilities`` (blending modes only) returns
    (labels, prob) with prob fp32 [K, D, H, W], the normalised blend.
    ``tta_flips`` (None or (0,): off, the launches above) = functional.tta_flip_codes(axes) predicts every patch under each of the F
    flip codes and averages the un-mirrored class probabilities before the argmax.  The gather reads the volume mirrored
    (mi355seg_gather_patches_flip_f32) and the accumulate reads the logits mirrored (mi355seg_aggregate_patches_flip_f32): no flipped
    copies.  Blending modes: the flips are the outer loop over the whole grid, all into the one accumulator, whose normaliser is
    F * sz -- the result stays bitwise independent of the batch size.  Crop mode: the F softmaxes of a batch are summed per patch,
    then argmax and paste as above."""
    from ._lib import lib
    if overlap_mode not in F.OVERLAP_MODES:
        raise ValueError(f"overlap_mode must be one of {F.OVERLAP_MODES}, got {overlap_mode!r}")
    if return_probabilities and overlap_mode == "crop":
        raise ValueError("return_probabilities needs a blending overlap_mode (average, hann or gaussian): 'crop' aggregates labels")
    flips = check_tta_flips(tta_flips)
    C, D, H, W = volume.shape
    ps = (patch_size,) * 3 if isinstance(patch_size, int) else tuple(patch_size)
    table_h = window_table((D, H, W), ps, overlap)
    P = table_h.shape[0]
    dev = volume.device
    table = torch.from_numpy(table_h).to(dev)
    volume = volume.contiguous().to(torch.float32)
    soft, acc = overlap_mode != "crop", None
    if soft:
        w64 = window_weights(overlap_mode, ps)
        weights = [torch.from_numpy(w.astype(np.float32)).to(dev) for w in w64]
        sums = [torch.from_numpy(s.astype(np.float32)).to(dev) for s in axis_weight_sums((D, H, W), ps, overlap, w64)]
    else:
        out = torch.zeros((1, D, H, W), dtype=torch.int64, device=dev)
    L, st = lib(), torch.cuda.current_stream().cuda_stream
    was_training = model.training
    model.eval()
    if flips:
        res = _predict_tta(model, volume, ps, table, flips, batch_size, dtype, weights if soft else None, sums if soft else None,
                           return_probabilities, None if soft else out)
        model.train(was_training)
        return res
    for i in range(0, P, batch_size):
        nb = min(batch_size, P - i)
        x = torch.empty((nb, C) + ps, dtype=torch.float32, device=dev)
        L.call("mi355seg_gather_patches_f32", volume.data_ptr(), C, D, H, W, table.data_ptr(), i, nb, ps[0], ps[1], ps[2], x.data_ptr(), st)
        logits = _forward(model, x, dtype)
        if soft:
            if acc is None:                                              # K is known once the first batch is through the model
                acc = torch.zeros((logits.shape[1], D, H, W), dtype=torch.float32, device=dev)
            F.aggregate_patches(acc, logits.to(torch.float32), table, i, weights)
            continue
        labels = F.argmax_channels(logits)                               # predict.py:133,139
        L.call("mi355seg_paste_labels_i64", labels.data_ptr(), table.data_ptr(), i, nb, ps[0], ps[1], ps[2], out.data_ptr(), D, H, W, st)
    model.train(was_training)
    if soft:
        return F.aggregate_finalize(acc, sums, probabilities=return_probabilities)
    return out


def znorm(v):
    """tio.ZNormalization (predict.py:94): zero mean / unit (unbiased) std over the whole volume, no epsilon -- torchio refuses a
    constant volume (``Standard deviation is 0``), so does this.  UNPINNED restatement: torchio is absent from the build image and
    the reference holds no fixture for it; the formula is torchio 0.20's ``ZNormalization.znorm``."""
    std = v.std()
    if float(std) == 0.0:
        raise RuntimeError("znorm: standard deviation is 0 for this volume (tio.ZNormalization raises here too)")
    return (v - v.mean()) / std


METRIC_COLUMNS = ("precision", "recall", "jaccard", "dice", "hs95")


def parse_spacing(config):
    """``config.spacing`` -> (sz, sy, sx) floats, or None when the key is absent or empty (metrics stay jaccard / dice)."""
    sp = getattr(config, "spacing", None)
    if sp is None or str(sp) in ("", "None", "none", "null"):
        return None
    vals = [float(v) for v in (str(sp).strip("()[] ").split(",") if isinstance(sp, str) else (sp if hasattr(sp, "__len__") else [sp]))]
    if len(vals) == 1:
        vals = vals * 3
    if len(vals) != 3 or not all(v > 0 for v in vals):
        raise ValueError(f"config.spacing must be three positive numbers sz,sy,sx, got {sp!r}")
    return tuple(vals)


COMPONENT_COLUMNS = ("components", "kept", "voxels_removed", "largest")


def parse_postprocess(config):
    """``config.keep_largest`` / ``config.min_component_voxels`` / ``config.connectivity`` -> (keep_largest, min_voxels, connectivity),
    or None when neither of the first two keys is set (absent, empty or 0): no clean-up, and connectivity is not looked at."""
    def count(key, top=None):
        v = getattr(config, key, None)
        if v is None or str(v) in ("", "None", "none", "null"):
            return 0
        if isinstance(v, bool) or not (isinstance(v, int) or (isinstance(v, str) and v.strip().isdigit())) or int(v) < 0 or (top is not None and int(v) > top):
            raise ValueError(f"config.{key} must be an integer in 0..{top}, got {v!r}" if top is not None else
                             f"config.{key} must be a non-negative integer, got {v!r}")
        return int(v)
    keep, small = count("keep_largest", F.MAX_KEEP_LARGEST), count("min_component_voxels")
    if not keep and not small:
        return None
    c = getattr(config, "connectivity", None)
    if c is None or str(c) in ("", "None", "none", "null"):
        c = 26
    if isinstance(c, bool) or not (isinstance(c, int) or (isinstance(c, str) and c.strip().isdigit())) or int(c) not in F.CONNECTIVITIES:
        raise ValueError(f"config.connectivity must be 6, 18 or 26, got {c!r}")
    return keep, small, int(c)


CLASS_COMPONENT_COLUMNS = ("class",) + COMPONENT_COLUMNS


def parse_class_postprocess(config, multiclass):
    """``config.class_keep_largest`` / ``config.class_min_voxels`` / ``config.connectivity`` -> (keep_largest, min_voxels,
    connectivity), or None when neither of the first two keys is set: no clean-up.  A value is one integer (every foreground class)
    or ``k:v,k:v`` (a class that is not named: 0; a single pair with a trailing comma, ``2:1,``, or as ``{2: 1}``: YAML reads ``2:1`` as
    the base-60 number 121), returned as an int or a {class: value} dict.  ``multiclass`` is parse_predict_multiclass's K: the keys
    need ``config.multiclass=true`` and classes in 1..K-1."""
    def per_class(key, top=None):
        v = getattr(config, key, None)
        if _absent(v):
            return 0
        bad = ValueError(f"config.{key} must be " + (f"an integer in 0..{top}" if top is not None else "a non-negative integer") +
                         f" or class:value pairs k:v,k:v, got {v!r} (YAML reads a single pair such as 2:1 as a base-60 number: write it "
                         f"with a trailing comma, 2:1, or as {{2: 1}})")
        if isinstance(v, dict):                          # {2: 1} on the command line arrives as a mapping
            v = ",".join(f"{k}:{x}" for k, x in v.items()) + ","
        if isinstance(v, bool) or not isinstance(v, (int, str)):
            raise bad
        if multiclass is None and str(v).strip() != "0":
            raise ValueError(f"config.{key} needs config.multiclass=true (config.keep_largest / config.min_component_voxels clean one foreground class)")
        def number(t):
            if not t.strip().isdigit() or (top is not None and int(t) > top):
                raise bad
            return int(t)
        if isinstance(v, int) or ":" not in v:
            return number(str(v))
        out = {}
        body = v.strip()
        for pair in (body[:-1] if body.endswith(",") else body).split(","):          # (one trailing comma: the single pair's form)
            k, sep, x = pair.partition(":")
            if not sep or not k.strip().isdigit() or int(k) in out:
                raise bad
            if not 1 <= int(k) <= multiclass - 1:
                raise ValueError(f"config.{key} names class {int(k)}; config.out_classes={multiclass} has the foreground classes 1..{multiclass - 1}")
            out[int(k)] = number(x)
        return out
    keep, small = per_class("class_keep_largest", F.MAX_KEEP_LARGEST), per_class("class_min_voxels")
    if not keep and not small:
        return None
    c = getattr(config, "connectivity", None)
    if _absent(c):
        c = 26
    if isinstance(c, bool) or not (isinstance(c, int) or (isinstance(c, str) and c.strip().isdigit())) or int(c) not in F.CONNECTIVITIES:
        raise ValueError(f"config.connectivity must be 6, 18 or 26, got {c!r}")
    return keep, small, int(c)


def class_component_rows(name, stats, K):
    """the rows of one file for write_class_components_csv: one per foreground class 1..K-1, zeros for a class that is absent"""
    none = dict.fromkeys(COMPONENT_COLUMNS, 0)
    return [{"file": name, "class": k, **stats.get(k, none)} for k in range(1, K)]


def parse_overlap_mode(config):
    """``config.overlap_mode`` -> one of functional.OVERLAP_MODES; "crop" (the reference's mode) when the key is absent or empty."""
    m = getattr(config, "overlap_mode", None)
    if _absent(m):
        return "crop"
    if not isinstance(m, str) or m not in F.OVERLAP_MODES:
        raise ValueError(f"config.overlap_mode must be one of {', '.join(F.OVERLAP_MODES)}, got {m!r}")
    return m


def parse_patch_overlap(config, patch):
    """``config.patch_overlap`` = oz,oy,ox (one number: all three axes) -> (oz, oy, ox), each even, >= 0 and smaller than the patch
    axis (grid_locations' rule); None when the key is absent or empty (the reference's (4, 4, 36) then stays)."""
    ov = getattr(config, "patch_overlap", None)
    if _absent(ov):
        return None
    parts = str(ov).strip("()[] ").split(",") if isinstance(ov, str) else (list(ov) if hasattr(ov, "__len__") else [ov])
    bad = ValueError(f"config.patch_overlap must be one or three even integers oz,oy,ox, each >= 0 and smaller than the patch axis "
                     f"{tuple(patch)}, got {ov!r}")
    vals = []
    for v in parts:
        if isinstance(v, bool) or not (isinstance(v, int) or (isinstance(v, str) and v.strip().isdigit())):
            raise bad
        vals.append(int(v))
    if len(vals) == 1:
        vals = vals * 3
    if len(vals) != 3 or any(o < 0 or o % 2 or o >= p for o, p in zip(vals, patch)):
        raise bad
    return tuple(vals)


def parse_save_probabilities(config, overlap_mode):
    """``config.save_probabilities`` -> bool (absent: False).  True needs a blending overlap mode: 'crop' has no probabilities."""
    v = getattr(config, "save_probabilities", None)
    if _absent(v):
        return False
    if isinstance(v, str) and v.strip().lower() in ("true", "false"):
        v = v.strip().lower() == "true"
    if not isinstance(v, bool):
        raise ValueError(f"config.save_probabilities must be true or false, got {v!r}")
    if v and overlap_mode == "crop":
        raise ValueError("config.save_probabilities=true needs config.overlap_mode=average, hann or gaussian "
                         "(the crop mode aggregates labels, not probabilities)")
    return v


def parse_tta(config):
    """``config.tta`` / ``config.tta_axes`` -> the flip codes of mirror test-time augmentation (functional.tta_flip_codes), or None
    when ``config.tta`` is absent, empty or ``none``.  ``config.tta_axes`` = any non-empty subset of z,y,x without duplicates (default:
    all three); giving it without ``config.tta=mirror`` is an error."""
    t, ax = getattr(config, "tta", None), getattr(config, "tta_axes", None)
    on = not _absent(t)
    if on and (not isinstance(t, str) or t != "mirror"):
        raise ValueError(f"config.tta must be mirror or none, got {t!r}")
    if _absent(ax):
        return F.tta_flip_codes(F.TTA_AXES) if on else None
    if not on:
        raise ValueError(f"config.tta_axes={ax!r} needs config.tta=mirror")
    parts = [a.strip() for a in ax.strip("()[] ").split(",")] if isinstance(ax, str) else (list(ax) if isinstance(ax, (list, tuple)) else [ax])
    if not parts or any(a not in F.TTA_AXES for a in parts) or len(set(parts)) != len(parts):
        raise ValueError(f"config.tta_axes must be a non-empty subset of {','.join(F.TTA_AXES)} without duplicates, got {ax!r}")
    return F.tta_flip_codes(parts)


def write_components_csv(path, rows):
    with open(path, "w", newline="") as fh:
        wr = csv.DictWriter(fh, fieldnames=["file"] + list(COMPONENT_COLUMNS))
        wr.writeheader()
        wr.writerows(rows)


def write_class_components_csv(path, rows):
    """config.class_keep_largest / config.class_min_voxels: rows of {file, class, components, kept, voxels_removed, largest}"""
    with open(path, "w", newline="") as fh:
        wr = csv.DictWriter(fh, fieldnames=["file"] + list(CLASS_COMPONENT_COLUMNS))
        wr.writeheader()
        wr.writerows(rows)


def write_metrics_csv(path, rows):
    """rows of {file, jaccard, dice}: those three columns, as they are.  Rows that also hold precision / recall / hs95 (a run with
    config.spacing): the reference's five columns in its order and a last row of their means (predict.py:186-200)."""
    full = bool(rows) and all(k in rows[0] for k in METRIC_COLUMNS)
    fields = ["file"] + (list(METRIC_COLUMNS) if full else ["jaccard", "dice"])
    with open(path, "w", newline="") as fh:
        wr = csv.DictWriter(fh, fieldnames=fields)
        wr.writeheader()
        wr.writerows(rows)
        if full:
            wr.writerow({"file": "mean", **{k: float(np.mean([r[k] for r in rows])) for k in METRIC_COLUMNS}})


def write_class_metrics_csv(path, rows):
    """config.multiclass: rows of {file, class, jaccard, dice}, one per file and foreground class, in the order given; rows that also
    hold precision / recall / hs95 (a run with config.spacing) get the reference's five columns in its order.  Last, one ``mean``
    row per class, ascending: the means of that class's rows."""
    full = bool(rows) and all(k in rows[0] for k in METRIC_COLUMNS)
    cols = list(METRIC_COLUMNS) if full else ["jaccard", "dice"]
    with open(path, "w", newline="") as fh:
        wr = csv.DictWriter(fh, fieldnames=["file", "class"] + cols)
        wr.writeheader()
        wr.writerows(rows)
        for k in sorted({r["class"] for r in rows}):
            wr.writerow({"file": "mean", "class": k, **{c: float(np.mean([r[c] for r in rows if r["class"] == k])) for c in cols}})


def class_metric_rows(name, gt_lab, mask, K, spacing=None):
    """The rows of one file for write_class_metrics_csv: the counts of all classes from ONE functional.class_counts launch; with a
    spacing, hs95 per class from metric_with_spacing on the class masks gt == k and mask == k."""
    m = class_metrics_from_counts(F.class_counts(gt_lab, mask, K))
    rows = []
    for k in range(1, K):
        row = {"file": name, "class": k, "jaccard": m["jaccard"][k], "dice": m["dice"][k]}
        if spacing:
            row["precision"], row["recall"] = m["precision"][k], m["recall"][k]
            row["hs95"] = metric_with_spacing((gt_lab == k).to(torch.int64), (mask == k).to(torch.int64), spacing)[4]
        rows.append(row)
    return rows


def parse_predict_multiclass(config):
    """``config.multiclass`` at predict time -> K = config.out_classes or None (train.parse_multiclass without the loss check).
    Refused with the component clean-up keys: per-class components are not built."""
    from .train import parse_multiclass
    K = parse_multiclass(config, False, data_key="pred_data_path")
    if K is not None and parse_postprocess(config) is not None:
        raise ValueError("config.multiclass does not go with config.keep_largest / config.min_component_voxels: the component "
                         "clean-up works on one foreground class")
    return K


def predict(config, model, log=print):
    device = torch.device("cuda", 0)
    if config.ckpt and str(config.ckpt) != "None":
        ckpt = torch.load(config.ckpt, map_location="cpu")
        state = {k[len("module."):] if k.startswith("module.") else k: v for k, v in ckpt["model"].items()}
        model.load_state_dict(state)
    model = model.to(device).eval()
    ps = config.patch_size
    ps = (ps,) * 3 if isinstance(ps, int) else tuple(ps)
    overlap = tuple(min(o, p - 2) // 2 * 2 for o, p in zip((4, 4, 36), ps))   # predict.py:100 overlap, kept valid for small patches
    overlap = parse_patch_overlap(config, ps) or overlap
    mode = parse_overlap_mode(config)
    save_prob = parse_save_probabilities(config, mode)
    flips = parse_tta(config)
    multiclass = parse_predict_multiclass(config)        # config.multiclass: K, or None (everything below as it was)
    if flips:
        log(f"tta: mirror, {len(flips)} flips per patch (codes {','.join(str(f) for f in flips)})")
    os.makedirs(config.hydra_path, exist_ok=True)
    if str(config.pred_data_path) == "synthetic":
        g = torch.Generator().manual_seed(7)
        cases = [("synthetic_%d" % i, torch.randn((config.in_classes,) + tuple(2 * p for p in ps), generator=g),
                  (torch.rand((1,) + tuple(2 * p for p in ps), generator=g) > 0.9).float()) for i in range(2)]
    else:
        cases = []
        for f in sorted(glob.glob(os.path.join(config.pred_data_path, "*.npy"))):
            x = torch.from_numpy(np.load(f).astype(np.float32))
            y = torch.from_numpy(np.load(os.path.join(config.pred_gt_path, os.path.basename(f))).astype(np.float32))
            cases.append((os.path.splitext(os.path.basename(f))[0], x[None] if x.dim() == 3 else x, y[None] if y.dim() == 3 else y))
    rows, comp_rows = [], []
    spacing = parse_spacing(config)
    post = parse_postprocess(config)
    class_post = parse_class_postprocess(config, multiclass)      # config.class_keep_largest / config.class_min_voxels; None: off
    intensity = parse_intensity(config)                  # config.intensity and its companions; None: the z-score of today
    if intensity is not None:
        log(f"intensity: {intensity}")
    resample = parse_resample(config)                    # config.resample_spacing and its companions; None: off
    source = resample.spacings if resample is not None else parse_spacing_source(config)
    if resample is not None:
        log(f"resample: {resample}")
    for name, x, gt in cases:
        xd = x.to(device)
        if source is not None and source.table is not None:                  # config.spacing_file: every volume is graded with its own spacing
            spacing = source.of(name)
        if resample is not None:                         # forward: the image to the common grid, before the normalisation
            grid, own = tuple(xd.shape[1:]), source.of(name)
            xd = F.resample_volume(xd, own, resample.target, resample.order)
        vol = F.normalize_intensity(xd, intensity) if intensity is not None else znorm(xd)
        want_prob = save_prob or (resample is not None and mode != "crop")
        mask = sliding_window_predict(model, vol, ps, overlap, batch_size=max(1, int(config.batch_size)), dtype=mixed_precision_dtype(config),
                                      overlap_mode=mode, return_probabilities=want_prob, tta_flips=flips)
        if want_prob:
            mask, prob = mask
        if resample is not None:                         # the way back: everything below sees the original grid
            if mode == "crop":
                mask = F.resample_back_labels(mask, grid, own, resample.target, resample.labels)
            elif save_prob:
                mask, prob = F.resample_back_argmax(prob, grid, own, resample.target, return_probabilities=True)
            else:
                mask = F.resample_back_argmax(prob, grid, own, resample.target)
        if save_prob:
            np.save(os.path.join(config.hydra_path, f"{name}_prob.npy"), prob.cpu().numpy())
        if post:
            mask, stats = F.filter_components(mask, min_voxels=post[1], keep_largest=post[0], connectivity=post[2], inplace=True)
            comp_rows.append({"file": name, **stats})
            log(f"{name}: " + " ".join(f"{k} {stats[k]}" for k in COMPONENT_COLUMNS))
        if class_post:
            mask, stats = F.filter_components_by_class(mask, min_voxels=class_post[1], keep_largest=class_post[0], connectivity=class_post[2],
                                                       inplace=True)
            new = class_component_rows(name, stats, multiclass)
            comp_rows.extend(new)
            log(f"{name}: " + " ".join(f"kept_{r['class']} {r['kept']}/{r['components']}" for r in new))
        gt_lab = gt.to(device).to(torch.int64).reshape(mask.shape)
        np.save(os.path.join(config.hydra_path, f"{name}_pred.npy"), mask.cpu().numpy().astype(np.uint8))
        if multiclass is not None:
            new = class_metric_rows(name, gt_lab, mask, multiclass, spacing)
            rows.extend(new)
            log(f"{name}: " + " ".join(f"dice_{r['class']} {r['dice']:.4f}" for r in new))
            continue
        if spacing:
            row = dict(zip(METRIC_COLUMNS, metric_with_spacing(gt_lab, mask, spacing)))
            rows.append({"file": name, **row})
            log(f"{name}: " + " ".join(f"{k} {row[k]:.4f}" for k in METRIC_COLUMNS))
            continue
        counts = F.dice_counts(gt_lab, mask)
        jac, dice = metric_from_counts(counts.cpu().tolist())
        rows.append({"file": name, "jaccard": jac, "dice": dice})
        log(f"{name}: dice {dice:.4f} jaccard {jac:.4f}")
    (write_class_metrics_csv if multiclass is not None else write_metrics_csv)(os.path.join(config.hydra_path, "metrics.csv"), rows)
    if post:
        write_components_csv(os.path.join(config.hydra_path, "components.csv"), comp_rows)
    if class_post:
        write_class_components_csv(os.path.join(config.hydra_path, "components.csv"), comp_rows)
    return rows


def main(argv=None, conf_dir=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    conf_dir = conf_dir or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "conf")
    config = compose(conf_dir, argv, job_name="predict")
    parse_patch_size(config)
    model = build_model(config)
    set_band_split(model, config)                        # config.band_split (IS only): fft | device
    return config, predict(config, model)


if __name__ == "__main__":
    main()
