"""Losses on the MI355X kernels -- drop-in for the reference's utils/loss_function.py
(same names, arguments and error behaviour).  The heavy reductions (BCE, Dice sums) are
HIP kernels; the scalar glue on the resulting 0-dim tensors is torch."""
import numpy as np
import torch
import torch.nn.functional as TF
from torch import nn

from .. import functional as F


class Binary_Loss(nn.Module):
    """loss_function.py:19-41 -- BCEWithLogitsLoss with mean reduction."""

    def forward(self, model_output, targets):
        return F.bce_with_logits(model_output, targets)


class BCEWithLogitsLoss(nn.Module):
    """The live criterion of the train loop (train.py:115)."""

    def forward(self, input, target):
        return F.bce_with_logits(input, target)


def cross_entropy_3D(input, target, weight=None, size_average=True):
    """loss_function.py:8-16 -- log_softmax over dim 1 + summed NLL, divided by the voxel count."""
    return F.cross_entropy_3d(input, target, weight, size_average)


def make_one_hot(input, num_classes):
    """loss_function.py:44-58 -- [N,1,*] int64 -> [N,K,*] float one-hot; like the reference the result
    lives on the CPU (it calls ``input.cpu()``)."""
    shape = np.array(input.shape)
    shape[1] = num_classes
    result = torch.zeros(tuple(shape))
    return result.scatter_(1, input.cpu(), 1)


class BinaryDiceLoss(nn.Module):
    """loss_function.py:61-99 -- per-sample 1 - (sum x*t + s) / (sum x^p + sum t^p + s), any exponent p; every sample's
    sums come from one row-segmented reduction launch."""

    def __init__(self, smooth=1, p=2, reduction="mean"):
        super().__init__()
        self.smooth, self.p, self.reduction = smooth, p, reduction

    def forward(self, predict, target):
        assert predict.shape[0] == target.shape[0], "predict & target batch size don't match"
        n = predict.shape[0]
        s = F.dice_rows_autograd(predict.contiguous().view(n, -1), target.contiguous().view(n, -1), False, self.p)
        loss = (1 - (s[:, 0] + self.smooth) / (s[:, 3] + s[:, 4] + self.smooth)).to(torch.float32)
        if self.reduction == "mean":
            return loss.mean()
        elif self.reduction == "sum":
            return loss.sum()
        elif self.reduction == "none":
            return loss
        else:
            raise Exception("Unexpected reduction {}".format(self.reduction))


class DiceLoss(nn.Module):
    """loss_function.py:102-130 -- global soft Dice on sigmoid(predict) against a one-hot target."""

    def __init__(self, weight=None, ignore_index=None, **kwargs):
        super().__init__()
        self.kwargs, self.weight, self.ignore_index = kwargs, weight, ignore_index
        self.eplison = 1e-5

    def forward(self, predict, target):
        assert predict.shape == target.shape, "predict & target shape do not match"
        s = F.dice_sums_autograd(predict, target, True)
        intersection, union = s[0], s[1] + s[2]
        return (1 - 2 * (intersection + self.eplison) / (union + self.eplison)).to(torch.float32)


class DiceLossss(nn.Module):
    """loss_function.py:148-185 -- per-class 1 - (2 sum s*t + eps) / (sum s^2 + sum t^2 + eps), weighted mean.
    ``softmax=True`` goes through functional.softmax_channels, which holds a voxel's classes in registers and raises
    Mi355SegError for more than 16 classes; without it any class count is taken."""

    def __init__(self, n_classes):
        super().__init__()
        self.n_classes = n_classes

    def _one_hot_encoder(self, input_tensor):
        return torch.stack([(input_tensor == i) for i in range(self.n_classes)], dim=1).float()

    def forward(self, inputs, target, weight=None, softmax=False):
        if softmax:
            inputs = F.softmax_channels(inputs)
        target = self._one_hot_encoder(target)
        if weight is None:
            weight = [1] * self.n_classes
        assert inputs.size() == target.size(), "predict & target shape do not match"
        smooth = 1e-5
        n = inputs.shape[0]
        # rows = (sample, class): one reduction launch for all of them, then the per-class sums over the batch
        s = F.dice_rows_autograd(inputs.contiguous().view(n * self.n_classes, -1), target.contiguous().view(n * self.n_classes, -1), False, 2.0)
        s = s.view(n, self.n_classes, 5).sum(dim=0)
        dice = 1 - (2 * s[:, 0] + smooth) / (s[:, 3] + s[:, 4] + smooth)
        w = torch.as_tensor(weight, dtype=torch.float64, device=dice.device)
        return ((dice * w).sum() / self.n_classes).to(torch.float32)


class CompoundLoss(nn.Module):
    """``config.loss``: a voxel term plus a region term on the fused tail (functional.loss_tail: one pass over logits and target
    forward, one backward).  Modes (functional.LOSS_MODES): dice | dice_bce | ce | dice_ce | focal | dice_focal | tversky, where
    bce = nn.BCEWithLogitsLoss (train.py:115), ce = cross_entropy_3D against target.argmax(1) (loss_function.py:8-16), dice =
    DiceLoss (loss_function.py:121-130); focal (Lin et al., exponent ``focal_gamma``, no alpha balancing) and tversky (Salehi et
    al., ``tversky_alpha`` on false positives, ``tversky_beta`` on false negatives, per class over the batch) are the project's
    own.  ``weights`` = (voxel, region).  ``forward`` returns the scalar loss (an ordinary criterion); ``tail`` returns (loss,
    mask, counts, terms), which engine.train_step uses in place of criterion + two argmaxes + dice_counts.
    ``cldice_weight`` > 0 adds the soft-clDice term (functional.soft_cldice with ``cldice_iters`` and ``cldice_smooth``; DESIGN.md
    4.20): loss = tail loss + cldice_weight * cldice and ``terms`` gains a third entry, the unweighted cldice.  With the weight 0
    the object is what it is without the three arguments: the same launches and the same bits.
    ``boundary_weight`` > 0 adds the boundary term (functional.boundary_loss with the voxel spacing ``boundary_spacing``; DESIGN.md
    4.21): loss += boundary_scale * boundary, where ``boundary_scale`` is a float32[1] device buffer that starts at the weight and
    that ``set_boundary_scale`` refills in place (a captured HIP graph sees the change: the ramp of config.boundary_ramp_epochs);
    ``terms`` gains the unweighted boundary value, after the clDice entry when both are on.  ``term_names`` names the entries of
    ``terms``.  With the weight 0: the same launches and the same bits as without the two arguments."""

    def __init__(self, mode, weights=(1, 1), focal_gamma=2.0, tversky_alpha=0.3, tversky_beta=0.7,
                 cldice_weight=0.0, cldice_iters=F.CLDICE_ITERS, cldice_smooth=F.CLDICE_SMOOTH,
                 boundary_weight=0.0, boundary_spacing=(1, 1, 1)):
        super().__init__()
        self.mode = mode
        self.spec = F.LossSpec.from_mode(mode, weights, focal_gamma, tversky_alpha, tversky_beta)
        number = lambda v: not isinstance(v, bool) and isinstance(v, (int, float))
        if not number(cldice_weight) or not cldice_weight >= 0:
            raise ValueError(f"cldice_weight must be a number >= 0, got {cldice_weight!r}")
        if not number(cldice_smooth) or not cldice_smooth > 0:
            raise ValueError(f"cldice_smooth must be a number > 0, got {cldice_smooth!r}")
        self.cldice_weight, self.cldice_smooth = float(cldice_weight), float(cldice_smooth)
        self.cldice_iters = F.checked_skel_iters(cldice_iters, "cldice_iters")
        if not number(boundary_weight) or not 0 <= boundary_weight < float("inf"):
            raise ValueError(f"boundary_weight must be a number >= 0, got {boundary_weight!r}")
        self.boundary_weight = float(boundary_weight)
        self.boundary_spacing = F.checked_spacing(boundary_spacing, "boundary_spacing")
        if self.boundary_weight > 0:                # (a plain attribute would not follow .to(); a buffer must not enter a state_dict)
            self.register_buffer("boundary_scale", torch.full((1,), self.boundary_weight, dtype=torch.float32), persistent=False)

    @property
    def term_names(self):
        """The names of the entries of ``terms``, in order."""
        return ("voxel", "region") + (("cldice",) if self.cldice_weight > 0 else ()) + (("boundary",) if self.boundary_weight > 0 else ())

    def set_boundary_scale(self, value):
        """Fill ``boundary_scale`` in place: the factor of the boundary term from the next step on, captured graphs included."""
        if not self.boundary_weight > 0:
            raise ValueError("set_boundary_scale: this loss has no boundary term (boundary_weight = 0)")
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not 0 <= value < float("inf"):
            raise ValueError(f"set_boundary_scale: expected a number >= 0, got {value!r}")
        self.boundary_scale.fill_(float(value))

    def tail(self, pred, target):
        out = F.loss_tail(pred, target, self.spec)
        if not self.cldice_weight > 0 and not self.boundary_weight > 0:
            return out
        return self._extra_terms(pred, target, *out)

    def tail_labels(self, pred, labels_u8):
        """``tail`` on a uint8 label map [N,...] (functional.labels_u8; config.multiclass): (loss, mask, counts, terms,
        class_counts) with class_counts int64 [K,3] = per class (tp, pred, gt).  The one-hot target is built (once, by
        functional.one_hot_labels) only for the clDice and boundary terms; without them no one-hot tensor exists in the step."""
        loss, mask, counts, terms, class_counts = F.loss_tail_labels(pred, labels_u8, self.spec)
        if self.cldice_weight > 0 or self.boundary_weight > 0:
            loss, mask, counts, terms = self._extra_terms(pred, F.one_hot_labels(labels_u8, pred.shape[1]), loss, mask, counts, terms)
        return loss, mask, counts, terms, class_counts

    def _extra_terms(self, pred, target, loss, mask, counts, terms):
        extra = [terms]
        if self.cldice_weight > 0:
            cl, parts = F.soft_cldice_full(pred, target, self.cldice_iters, self.cldice_smooth)
            loss = loss + self.cldice_weight * cl
            extra.append(parts[:1])
        if self.boundary_weight > 0:
            if self.boundary_scale.device != pred.device:
                self.boundary_scale = self.boundary_scale.to(pred.device)        # (once: a criterion is built on the host)
            bd, parts = F.boundary_loss_full(pred, target, self.boundary_spacing)
            loss = loss + (self.boundary_scale * bd).reshape(())
            extra.append(parts)
        return loss, mask, counts, torch.cat(extra)

    def forward(self, pred, target):
        return self.tail(pred, target)[0]

    def extra_repr(self):
        s = f"mode={self.mode!r}, spec={tuple(self.spec)!r}"
        if self.cldice_weight > 0:
            s += f", cldice=(weight={self.cldice_weight!r}, iters={self.cldice_iters!r}, smooth={self.cldice_smooth!r})"
        if self.boundary_weight > 0:
            s += f", boundary=(weight={self.boundary_weight!r}, spacing={self.boundary_spacing!r})"
        return s
