"""Dice / Jaccard metric on the MI355X -- drop-in for ``metric(gt, pred, spacing=None)``
of the reference's utils/metric.py:20-75.  The integer counters are reduced on the device
(exact), only four int64 values cross PCIe; the final ratios use the reference's formula.

With ``spacing`` the reference returns five numbers, ``precision, recall, jaccard, dice, hs95`` (utils/metric.py:29-32,58-59,
72-73, called as ``metric(gt_t, pred_t, spacing)`` by predict.py:154); so does this, from ``functional.confusion_counts`` and
``functional.hd95``.  PINNED by the reference's own text: the order of the five, precision and recall, and the call
``compute_hausdorff_distance(pred, gdth, percentile=95, spacing=spacing)``.  UNPINNED restatement: what monai's function does
inside.  monai is absent here and the reference holds no fixture for it; restated from monai 1.3.1 (the reference's pin) without
the source at hand as: the edge voxels of each mask by erosion with the default six-neighbour structure (outside the array is
background), ``scipy.ndimage.distance_transform_edt(~edges_other, sampling=spacing)`` read at the edge voxels of the first, the
percentile with linear interpolation between order statistics, the maximum of the two directions, and no channel dropped because
there is one channel.  The result for a mask without foreground is the least certain part: it is NaN here, and the tests ask only
that it is not finite."""
import torch

from .. import functional as F


def metric_from_counts(counts):
    """counts = (sum gt, sum pred, nnz(gt&pred), nnz(gt|pred)) -> (jaccard, dice), metric.py:65-66."""
    gsum, psum, inter, union = [int(v) for v in counts]
    smooth = 0.001
    return inter / (union + smooth), 2 * inter / (gsum + psum + smooth)


def class_metrics_from_counts(class_counts):
    """class_counts = K rows (tp_k, pred_k, gt_k) (functional.loss_tail_labels / functional.class_counts; a tensor, or nested
    lists) -> {"dice", "jaccard", "precision", "recall": lists of K floats, "mean_dice": float}, each with the reference's
    smoothing per class (utils/metric.py:57-66).  ``mean_dice`` is the run's scalar Dice: the mean of dice_k over the foreground
    classes 1..K-1 that occur (gt_k + pred_k > 0), 0.0 when none does; at K = 2 it is metric_from_counts' Dice, number for number."""
    rows = class_counts.cpu().tolist() if hasattr(class_counts, "cpu") else list(class_counts)
    rows = [[int(v) for v in row] for row in rows]
    if not rows or any(len(row) != 3 for row in rows):
        raise ValueError(f"class_counts must be K rows of (tp, pred, gt), got {rows!r}")
    smooth = 0.001
    out = {"dice": [], "jaccard": [], "precision": [], "recall": []}
    for tp, psum, gsum in rows:
        out["dice"].append(2 * tp / (gsum + psum + smooth))
        out["jaccard"].append(tp / (gsum + psum - tp + smooth))
        out["precision"].append(tp / (psum + smooth))
        out["recall"].append(tp / (gsum + smooth))
    present = [k for k in range(1, len(rows)) if rows[k][1] + rows[k][2] > 0]
    for name in ("dice", "jaccard"):                 # (mean_jaccard: the same mean, what a step reports beside its Dice)
        out["mean_" + name] = sum(out[name][k] for k in present) / len(present) if present else 0.0
    return out


def rates_from_counts(counts):
    """counts = the eight integers of functional.confusion_counts -> (precision, recall), utils/metric.py:57-59."""
    gsum, psum, tp = int(counts[0]), int(counts[1]), int(counts[4])
    smooth = 0.001
    return tp / (psum + smooth), tp / (gsum + smooth)


def metric_with_spacing(gt, pred, spacing):
    """(precision, recall, jaccard, dice, hs95) of two int64 device label volumes, [D, H, W] with leading singleton dimensions."""
    counts = F.confusion_counts(gt, pred)
    hs95 = F.hd95(gt, pred, spacing, 95)
    counts = counts.cpu().tolist()
    precision, recall = rates_from_counts(counts)
    jaccard, dice = metric_from_counts(counts[:4])
    return precision, recall, jaccard, dice, float(hs95)


def metric(gt, pred, spacing=None):
    if spacing:
        return metric_with_spacing(gt.to(torch.int64), pred.to(torch.int64), spacing)
    gt = gt.to(torch.int64) if gt.dtype != torch.int64 else gt
    pred = pred.to(torch.int64) if pred.dtype != torch.int64 else pred
    return metric_from_counts(F.dice_counts(gt, pred).cpu().tolist())
