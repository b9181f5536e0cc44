"""``torch.ops.mi355seg.*`` -- the hot-path kernels registered as PyTorch custom operators.

north_star asks for the HIP kernels to be "exposed as torch custom ops".  The boundary stays the C-ABI
(include/mi355seg.h, bound with ctypes in ``_lib.py``); this module registers the same entry points with the
dispatcher through ``torch.library.custom_op`` (schemas inferred from the annotations, ``register_fake`` for shape
propagation, ``register_autograd`` wiring forward to the dgrad / wgrad entry points), so the kernels are reachable as
``torch.ops.mi355seg.conv3d(x, w, b, stride, pad)`` etc. from code that speaks the dispatcher (``torch.compile`` graphs,
``opcheck``, export).  Tensors are channel-last [N, D, H, W, C] (fp32 or bf16) exactly as in ``functional``; the model
mirrors keep using the ``torch.autograd.Function`` wrappers of ``functional.py``, which additionally handle strided
channel slices of concat buffers (a custom op's outputs may not alias its inputs).

Reference calls replaced: nn.Conv3d (unet3d.py:80-98), nn.ConvTranspose3d k2 s2 (unet3d.py:29-43), nn.MaxPool3d(2,2)
(unet3d.py:19-25), nn.Upsample(2, nearest) (residual_unet3d.py:19), nn.BCEWithLogitsLoss + argmax + metric
(train.py:204-221)."""
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import functional as F
from ._lib import lib

_p, _stream = F._p, F._stream


def _or_empty(t, like, dtype):
    """A gradient that does not exist, as an operator output: an operator returns tensors, so an empty one stands for None."""
    return t if t is not None else torch.empty(0, dtype=dtype, device=like.device)


# ------------------------------------------------------------------------------------------------ Conv3d
@torch.library.custom_op("mi355seg::conv3d", mutates_args=())
def conv3d(x: Tensor, weight: Tensor, bias: Optional[Tensor], stride: int, padding: int) -> Tensor:
    xv, ldx = F.cl_view(x, "conv3d input")
    g, w = F._conv_geom(xv, weight, stride, padding, "conv3d")
    y = torch.empty(g.out_shape, dtype=xv.dtype, device=xv.device)
    L = lib()
    F._conv_fwd(L, g, xv, ldx, w, bias, y, g.Cout, F.workspace(g.ws_bytes(L, xv.dtype), xv.device))
    return y


@conv3d.register_fake
def _(x, weight, bias, stride, padding):
    return x.new_empty(F._conv_geom(x, weight, stride, padding, "conv3d")[0].out_shape)


@torch.library.custom_op("mi355seg::conv3d_dgrad", mutates_args=())
def conv3d_dgrad(dy: Tensor, weight: Tensor, D: int, H: int, W: int, stride: int, padding: int) -> Tensor:
    dyv, lddy = F.cl_view(dy, "conv3d grad")
    g, w = F._conv_geom((dyv.shape[0], D, H, W, weight.shape[1]), weight, stride, padding, "conv3d")
    dx = torch.empty(g.args[:5], dtype=dyv.dtype, device=dyv.device)
    L = lib()
    F._conv_dgrad(L, g, dyv, lddy, w, dx, g.Cin, F.workspace(g.ws_bytes(L, dyv.dtype), dyv.device))
    return dx


@conv3d_dgrad.register_fake
def _(dy, weight, D, H, W, stride, padding):
    return dy.new_empty((dy.shape[0], D, H, W, weight.shape[1]))


@torch.library.custom_op("mi355seg::conv3d_wgrad", mutates_args=())
def conv3d_wgrad(dy: Tensor, x: Tensor, kernel_size: int, stride: int, padding: int, with_bias: bool) -> Tuple[Tensor, Tensor]:
    """(dw fp32 (Cout, Cin, k, k, k), db fp32 (Cout) -- zeros(0) when with_bias is False)."""
    dyv, lddy = F.cl_view(dy, "conv3d grad")
    xv, ldx = F.cl_view(F._like(x, dyv), "conv3d input")
    g = F._ConvGeom(*xv.shape, dyv.shape[-1], kernel_size, stride, padding)
    dw = torch.empty((g.Cout, g.Cin) + (g.k,) * 3, dtype=torch.float32, device=xv.device)
    db = torch.empty(g.Cout if with_bias else 0, dtype=torch.float32, device=xv.device)
    L = lib()
    F._conv_wgrad(L, g, dyv, lddy, xv, ldx, dw, db if with_bias else None, F.workspace(g.ws_bytes(L, xv.dtype), xv.device))
    return dw, db


@conv3d_wgrad.register_fake
def _(dy, x, kernel_size, stride, padding, with_bias):
    Cout, Cin, k = dy.shape[-1], x.shape[-1], kernel_size
    return (torch.empty((Cout, Cin, k, k, k), dtype=torch.float32, device=x.device),
            torch.empty(Cout if with_bias else 0, dtype=torch.float32, device=x.device))


def _conv3d_setup(ctx, inputs, output):
    x, w, b, stride, pad = inputs
    ctx.save_for_backward(x, w)
    ctx.cfg = (stride, pad, b is not None)


def _conv3d_backward(ctx, dy):
    x, w = ctx.saved_tensors
    stride, pad, has_b = ctx.cfg
    dx = dw = db = None
    if ctx.needs_input_grad[0]:
        dx = torch.ops.mi355seg.conv3d_dgrad(dy, w, x.shape[1], x.shape[2], x.shape[3], stride, pad)
    if ctx.needs_input_grad[1] or (has_b and ctx.needs_input_grad[2]):
        dw, dbv = torch.ops.mi355seg.conv3d_wgrad(dy, x, w.shape[2], stride, pad, has_b)
        db = dbv if has_b else None
    return dx, dw, db, None, None


torch.library.register_autograd("mi355seg::conv3d", _conv3d_backward, setup_context=_conv3d_setup)


# ------------------------------------------------------------------------------------------------ ConvTranspose3d k2 s2
@torch.library.custom_op("mi355seg::conv_transpose3d_k2s2", mutates_args=())
def conv_transpose3d_k2s2(x: Tensor, weight: Tensor, bias: Optional[Tensor]) -> Tensor:
    return F._ConvT3dK2S2.apply(x.detach(), weight.detach(), None if bias is None else bias.detach())


@conv_transpose3d_k2s2.register_fake
def _(x, weight, bias):
    N, D, H, W, _ = x.shape
    return x.new_empty((N, 2 * D, 2 * H, 2 * W, weight.shape[1]))


@torch.library.custom_op("mi355seg::conv_transpose3d_k2s2_backward", mutates_args=())
def conv_transpose3d_k2s2_backward(dy: Tensor, x: Tensor, weight: Tensor, with_bias: bool) -> Tuple[Tensor, Tensor, Tensor]:
    xv, ldx = F.cl_view(x, "conv_transpose3d input")
    dyv, lddy = F.cl_view(F._like(dy, xv), "conv_transpose3d grad")
    w = F._w32(weight, "conv_transpose3d weight")
    dx, dw, db = F._convt_k2s2_bwd(lib(), xv, ldx, dyv, lddy, w, with_bias, True, True)
    return dx, dw, (db if with_bias else torch.empty(0, dtype=torch.float32, device=xv.device))


@conv_transpose3d_k2s2_backward.register_fake
def _(dy, x, weight, with_bias):
    return (torch.empty_like(x), torch.empty_like(weight), torch.empty(weight.shape[1] if with_bias else 0, dtype=torch.float32, device=x.device))


def _convt_setup(ctx, inputs, output):
    x, w, b = inputs
    ctx.save_for_backward(x, w)
    ctx.has_b = b is not None


def _convt_backward(ctx, dy):
    x, w = ctx.saved_tensors
    dx, dw, db = torch.ops.mi355seg.conv_transpose3d_k2s2_backward(dy, x, w, ctx.has_b)
    return dx, dw, (db if ctx.has_b else None)


torch.library.register_autograd("mi355seg::conv_transpose3d_k2s2", _convt_backward, setup_context=_convt_setup)


# ------------------------------------------------------------------------------------------------ pool / upsample
@torch.library.custom_op("mi355seg::max_pool3d_2x", mutates_args=())
def max_pool3d_2x(x: Tensor) -> Tuple[Tensor, Tensor]:
    """(pooled, uint8 arg-max codes 0..7 of each 2x2x2 window)."""
    return F._maxpool2_fwd(*F.cl_view(x, "max_pool3d input"))


@max_pool3d_2x.register_fake
def _(x):
    N, D, H, W, C = x.shape
    return x.new_empty((N, D // 2, H // 2, W // 2, C)), torch.empty((N, D // 2, H // 2, W // 2, C), dtype=torch.uint8, device=x.device)


@torch.library.custom_op("mi355seg::max_pool3d_2x_backward", mutates_args=())
def max_pool3d_2x_backward(dy: Tensor, idx: Tensor, D: int, H: int, W: int) -> Tensor:
    dyv, lddy = F.cl_view(dy, "max_pool3d grad")
    return F._maxpool2_bwd(dyv, lddy, idx, (dyv.shape[0], D, H, W, dyv.shape[-1]))


@max_pool3d_2x_backward.register_fake
def _(dy, idx, D, H, W):
    return dy.new_empty((dy.shape[0], D, H, W, dy.shape[-1]))


def _pool_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])
    ctx.ext = tuple(inputs[0].shape[1:4])


def _pool_backward(ctx, dy, _didx):
    (idx,) = ctx.saved_tensors
    return torch.ops.mi355seg.max_pool3d_2x_backward(dy, idx, *ctx.ext)


torch.library.register_autograd("mi355seg::max_pool3d_2x", _pool_backward, setup_context=_pool_setup)


@torch.library.custom_op("mi355seg::upsample_nearest_2x", mutates_args=())
def upsample_nearest_2x(x: Tensor) -> Tensor:
    return F._Upsample2.apply(x.detach())


@upsample_nearest_2x.register_fake
def _(x):
    N, D, H, W, C = x.shape
    return x.new_empty((N, 2 * D, 2 * H, 2 * W, C))


@torch.library.custom_op("mi355seg::upsample_nearest_2x_backward", mutates_args=())
def upsample_nearest_2x_backward(dy: Tensor) -> Tensor:
    return F._upsample2_bwd(*F.cl_view(dy, "upsample grad"))


@upsample_nearest_2x_backward.register_fake
def _(dy):
    N, D2, H2, W2, C = dy.shape
    return dy.new_empty((N, D2 // 2, H2 // 2, W2 // 2, C))


torch.library.register_autograd("mi355seg::upsample_nearest_2x", lambda ctx, dy: torch.ops.mi355seg.upsample_nearest_2x_backward(dy))


# ------------------------------------------------------------------------------------------------ loss / metric tail
@torch.library.custom_op("mi355seg::bce_argmax_dice", mutates_args=())
def bce_argmax_dice(logits: Tensor, target: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """train.py:204,209,221 in one pass: (BCE-with-logits mean loss, argmax mask int64 [N,1,...], Dice counters int64[4])."""
    loss, mask, counts = F._BCEArgmaxDice.apply(logits.detach(), target.detach())
    return loss, mask, counts


@bce_argmax_dice.register_fake
def _(logits, target):
    return (logits.new_empty(()), torch.empty((logits.shape[0], 1) + tuple(logits.shape[2:]), dtype=torch.int64, device=logits.device),
            torch.empty(4, dtype=torch.int64, device=logits.device))


@torch.library.custom_op("mi355seg::bce_with_logits_backward", mutates_args=())
def bce_with_logits_backward(logits: Tensor, target: Tensor, grad: Tensor) -> Tensor:
    lg, tg = logits.contiguous(), target.contiguous().to(torch.float32)
    d = torch.empty_like(lg)
    lib().call("mi355seg_bce_logits_bwd_f32", _p(lg), _p(tg), _p(grad.contiguous().to(torch.float32)), lg.numel(), _p(d), _stream())
    return d


@bce_with_logits_backward.register_fake
def _(logits, target, grad):
    return torch.empty_like(logits)


def _tail_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _tail_backward(ctx, g, _gm, _gc):
    logits, target = ctx.saved_tensors
    return torch.ops.mi355seg.bce_with_logits_backward(logits, target, g), None


torch.library.register_autograd("mi355seg::bce_argmax_dice", _tail_backward, setup_context=_tail_setup)


@torch.library.custom_op("mi355seg::dice_counts", mutates_args=())
def dice_counts(gt: Tensor, pred: Tensor) -> Tensor:
    """utils/metric.py:26-66 on the device: int64[4] = (sum gt, sum pred, nnz(gt & pred), nnz(gt | pred))."""
    return F.dice_counts(gt, pred)


@dice_counts.register_fake
def _(gt, pred):
    return torch.empty(4, dtype=torch.int64, device=gt.device)


@torch.library.custom_op("mi355seg::connected_components", mutates_args=())
def connected_components(mask: Tensor, connectivity: int = 26) -> Tuple[Tensor, Tensor, Tensor]:
    """Connected components of an int64 label volume (scipy.ndimage.label semantics): labels int32 [D, H, W] (1 + the raster index
    of the component's first voxel), sizes int32 [D*H*W], info int64[4]."""
    return F.connected_components(mask, connectivity)


@connected_components.register_fake
def _(mask, connectivity=26):
    shape = tuple(mask.shape[-3:])
    return (torch.empty(shape, dtype=torch.int32, device=mask.device), torch.empty(shape[0] * shape[1] * shape[2], dtype=torch.int32, device=mask.device),
            torch.empty(4, dtype=torch.int64, device=mask.device))


@torch.library.custom_op("mi355seg::connected_components_by_class", mutates_args=())
def connected_components_by_class(mask: Tensor, connectivity: int = 26) -> Tuple[Tensor, Tensor, Tensor]:
    """Class-aware connected components of an int64 label volume (voxels join only within one value 1..255; every class in one
    labelling call): labels int32 [D, H, W], sizes int32 [D*H*W], info int64[8] (slot 4: voxels outside 0..255, which raise)."""
    return F.connected_components_by_class(mask, connectivity)


@connected_components_by_class.register_fake
def _(mask, connectivity=26):
    shape = tuple(mask.shape[-3:])
    return (torch.empty(shape, dtype=torch.int32, device=mask.device), torch.empty(shape[0] * shape[1] * shape[2], dtype=torch.int32, device=mask.device),
            torch.empty(8, dtype=torch.int64, device=mask.device))


@torch.library.custom_op("mi355seg::confusion_counts", mutates_args=())
def confusion_counts(gt: Tensor, pred: Tensor) -> Tensor:
    """utils/metric.py:34-55 on the device: int64[8] = the four counters of dice_counts, then tp, fp, fn, tn."""
    return F.confusion_counts(gt, pred)


@confusion_counts.register_fake
def _(gt, pred):
    return torch.empty(8, dtype=torch.int64, device=gt.device)


@torch.library.custom_op("mi355seg::hd95", mutates_args=())
def hd95(gt: Tensor, pred: Tensor, spacing: List[float], percentile: float = 95.0) -> Tensor:
    """utils/metric.py:32 on the device: the percentile Hausdorff distance of two int64 label volumes, 0-dim fp64."""
    return F.hd95(gt, pred, spacing, percentile)


@hd95.register_fake
def _(gt, pred, spacing, percentile=95.0):
    return torch.empty((), dtype=torch.float64, device=gt.device)


# ------------------------------------------------------------------------------------------------ layout (module boundary)
@torch.library.custom_op("mi355seg::to_channels_last", mutates_args=())
def to_channels_last(x: Tensor) -> Tensor:
    """fp32 NCDHW -> channel-last [N, D, H, W, C] in the current activation storage type (fp32, or bf16 under autocast)."""
    return F.to_channels_last(x.detach()).clone()


@to_channels_last.register_fake
def _(x):
    N, C = x.shape[0], x.shape[1]
    return torch.empty((N,) + tuple(x.shape[2:]) + (C,), dtype=F.compute_dtype(), device=x.device)


@torch.library.custom_op("mi355seg::to_channels_first", mutates_args=())
def to_channels_first(x: Tensor) -> Tensor:
    """channel-last (fp32 | bf16) -> fp32 NCDHW."""
    return F.to_channels_first(x.detach()).clone()


@to_channels_first.register_fake
def _(x):
    return torch.empty((x.shape[0], x.shape[-1]) + tuple(x.shape[1:-1]), dtype=torch.float32, device=x.device)


def _cl_setup(ctx, inputs, output):
    ctx.in_dtype = inputs[0].dtype


torch.library.register_autograd("mi355seg::to_channels_last", lambda ctx, g: torch.ops.mi355seg.to_channels_first(g).to(ctx.in_dtype), setup_context=_cl_setup)
torch.library.register_autograd("mi355seg::to_channels_first", lambda ctx, g: F.cast(torch.ops.mi355seg.to_channels_last(g.contiguous()), ctx.in_dtype),
                                setup_context=_cl_setup)


# ------------------------------------------------------------------------------------------------ BatchNorm3d / InstanceNorm3d + activation
@torch.library.custom_op("mi355seg::norm_stats", mutates_args=("running_mean", "running_var"))
def norm_stats(x: Tensor, running_mean: Optional[Tensor], running_var: Optional[Tensor], momentum: float, eps: float,
               instance: bool) -> Tuple[Tensor, Tensor]:
    """(mean, 1 / sqrt(var + eps)) per channel (per sample and channel for instance norm); BatchNorm running statistics are
    updated in place exactly as nn.BatchNorm3d does in training mode (unet3d.py:84-96)."""
    xv, ldx = F.cl_view(x, "norm input")
    C = xv.shape[-1]
    rows, groups = F._norm_rows(xv.shape, instance)
    L = lib()
    ws = F._norm_ws(L, rows, groups, C, xv.device)
    return F._batch_stats(L, xv, ldx, rows, groups, C, eps, running_mean, running_var, momentum, ws)


@norm_stats.register_fake
def _(x, running_mean, running_var, momentum, eps, instance):
    n = (x.shape[0] if instance else 1) * x.shape[-1]
    return torch.empty(n, dtype=torch.float32, device=x.device), torch.empty(n, dtype=torch.float32, device=x.device)


@torch.library.custom_op("mi355seg::norm_apply_act", mutates_args=())
def norm_apply_act(x: Tensor, mean: Tensor, rstd: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], residual: Optional[Tensor],
                   act: int, slope: float, instance: bool) -> Tensor:
    """act((x - mean) * rstd * gamma + beta [+ residual]) in one pass."""
    xv, ldx = F.cl_view(x, "norm input")
    C = xv.shape[-1]
    rows, groups = F._norm_rows(xv.shape, instance)
    y = torch.empty(xv.shape, dtype=xv.dtype, device=xv.device)
    F._norm_act_fwd(lib(), xv, ldx, mean, rstd, gamma, beta, F._opt_view(residual, "norm residual"), _p(y), C, rows, groups, C, act, slope)
    return y


@norm_apply_act.register_fake
def _(x, mean, rstd, gamma, beta, residual, act, slope, instance):
    return torch.empty_like(x)


@torch.library.custom_op("mi355seg::norm_act_backward", mutates_args=())
def norm_act_backward(dy: Tensor, x: Tensor, mean: Tensor, rstd: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], residual: Optional[Tensor],
                      act: int, slope: float, instance: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Backward of norm_stats + norm_apply_act with batch / instance statistics: (dx, dgamma, dbeta, dresidual); empty tensors
    where the forward had no gamma / residual."""
    xv, ldx = F.cl_view(x, "norm input")
    dyv, lddy = F.cl_view(F._like(dy, xv), "norm grad")
    C = xv.shape[-1]
    rows, groups = F._norm_rows(xv.shape, instance)
    L = lib()
    ws = F._norm_ws(L, rows, groups, C, xv.device)
    dx, dgamma, dbeta, dres, _ = F._norm_act_bwd(L, dyv, lddy, xv, ldx, mean, rstd, gamma, beta, F._opt_view(residual, "norm residual"),
                                                 rows, groups, C, act, slope, ws)
    return dx, _or_empty(dgamma, xv, torch.float32), _or_empty(dbeta, xv, torch.float32), _or_empty(dres, xv, xv.dtype)


@norm_act_backward.register_fake
def _(dy, x, mean, rstd, gamma, beta, residual, act, slope, instance):
    C = x.shape[-1]
    return (torch.empty_like(x), torch.empty(C if gamma is not None else 0, dtype=torch.float32, device=x.device),
            torch.empty(C if gamma is not None else 0, dtype=torch.float32, device=x.device),
            torch.empty_like(x) if residual is not None else torch.empty(0, dtype=x.dtype, device=x.device))


def _norm_apply_setup(ctx, inputs, output):
    x, mean, rstd, gamma, beta, residual, act, slope, instance = inputs
    ctx.save_for_backward(x, mean, rstd, gamma, beta, residual)
    ctx.cfg = (act, slope, instance)


def _norm_apply_backward(ctx, dy):
    """The statistics are functions of x: the backward kernel differentiates through them (batch / instance statistics), so the
    gradient reaches x here and norm_stats itself is registered as non-differentiable."""
    x, mean, rstd, gamma, beta, residual = ctx.saved_tensors
    act, slope, instance = ctx.cfg
    dx, dgamma, dbeta, dres = torch.ops.mi355seg.norm_act_backward(dy, x, mean, rstd, gamma, beta, residual, act, slope, instance)
    return dx, None, None, (dgamma if gamma is not None else None), (dbeta if beta is not None else None), (dres if residual is not None else None), None, None, None


torch.library.register_autograd("mi355seg::norm_apply_act", _norm_apply_backward, setup_context=_norm_apply_setup)


def batch_norm_act(x, gamma, beta, running_mean, running_var, momentum, eps, act, slope, residual=None):
    """Training-mode act(BatchNorm3d(x) [+ residual]) through the dispatcher: two ops, one fused backward."""
    mean, rstd = torch.ops.mi355seg.norm_stats(x.detach(), running_mean, running_var, momentum, eps, False)
    return torch.ops.mi355seg.norm_apply_act(x, mean, rstd, gamma, beta, residual, act, slope, False)


# ------------------------------------------------------------------------------------------------ conv + BatchNorm + activation (one node)
@torch.library.custom_op("mi355seg::conv_bn_act", mutates_args=())
def conv_bn_act(x: Tensor, weight: Tensor, bias: Optional[Tensor], gamma: Tensor, beta: Tensor, running_mean: Tensor, running_var: Tensor,
                stride: int, padding: int, momentum: float, eps: float, act: int, slope: float) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Training-mode act(BatchNorm3d(conv3d(x))) (unet3d.py:80-98): the batch statistics come out of the convolution's epilogue.
    Functional (an operator with an autograd formula may not mutate its inputs): returns (activation, raw convolution output,
    mean, rstd, updated running_mean, updated running_var); ``conv_bn_act_train`` below writes the last two back into the
    module's buffers, as aten's native_batch_norm callers do."""
    xv, ldx = F.cl_view(x, "conv3d input")
    g, w = F._conv_geom(xv, weight, stride, padding, "conv3d")
    Cout, rows = g.Cout, g.rows_out
    dev = xv.device
    L = lib()
    ws = F.workspace(F._conv_norm_ws(L, g, xv.dtype, rows, Cout), dev)
    y = torch.empty(g.out_shape, dtype=xv.dtype, device=dev)
    sums = torch.empty(2 * Cout, dtype=torch.float64, device=dev)
    F._conv_fwd(L, g, xv, ldx, w, bias, y, Cout, ws, sums)
    new_rm, new_rv = running_mean.detach().clone(), running_var.detach().clone()
    mean, rstd = F._stats_from_sums(L, sums, rows, Cout, eps, new_rm, new_rv, momentum)
    a = torch.empty_like(y)
    F._norm_act_fwd(L, y, Cout, mean, rstd, gamma, beta, F._NO_RES, _p(a), Cout, rows, 1, Cout, act, slope)
    return a, y, mean, rstd, new_rm, new_rv


@conv_bn_act.register_fake
def _(x, weight, bias, gamma, beta, running_mean, running_var, stride, padding, momentum, eps, act, slope):
    shape = F._conv_geom(x, weight, stride, padding, "conv3d")[0].out_shape
    f = lambda: torch.empty(shape[-1], dtype=torch.float32, device=x.device)
    return x.new_empty(shape), x.new_empty(shape), f(), f(), f(), f()


@torch.library.custom_op("mi355seg::conv_bn_act_backward", mutates_args=())
def conv_bn_act_backward(da: Tensor, x: Tensor, weight: Tensor, y: Tensor, mean: Tensor, rstd: Tensor, gamma: Tensor, beta: Tensor,
                         stride: int, padding: int, act: int, slope: float, with_bias: bool, need_dx: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(dx, dw, dbias, dgamma, dbeta): BatchNorm + activation backward with the conv-bias column sums in the same pass, then the
    input and weight gradients of the convolution."""
    xv, ldx = F.cl_view(x, "conv3d input")
    dav, ldda = F.cl_view(F._like(da, xv), "conv+norm grad")
    g, w = F._conv_geom(xv, weight, stride, padding, "conv3d")
    Cout, rows = g.Cout, g.rows_out
    dev = xv.device
    L = lib()
    ws = F.workspace(F._conv_norm_ws(L, g, xv.dtype, rows, Cout), dev)
    dy, dgamma, dbeta, _, db = F._norm_act_bwd(L, dav, ldda, y, Cout, mean, rstd, gamma, beta, F._NO_RES, rows, 1, Cout, act, slope, ws, with_bias)
    dx = torch.empty(xv.shape if need_dx else (0,), dtype=xv.dtype, device=dev)
    if need_dx:
        F._conv_dgrad(L, g, dy, Cout, w, dx, g.Cin, ws)
    dw = torch.empty_like(w)
    F._conv_wgrad(L, g, dy, Cout, xv, ldx, dw, None, ws)
    return dx, dw, _or_empty(db, xv, torch.float32), dgamma, dbeta


@conv_bn_act_backward.register_fake
def _(da, x, weight, y, mean, rstd, gamma, beta, stride, padding, act, slope, with_bias, need_dx):
    C = weight.shape[0]
    f = lambda n: torch.empty(n, dtype=torch.float32, device=x.device)
    return (torch.empty_like(x) if need_dx else torch.empty(0, dtype=x.dtype, device=x.device), torch.empty_like(weight), f(C if with_bias else 0), f(C), f(C))


def _cba_setup(ctx, inputs, output):
    x, w, b, gamma, beta, rm, rv, stride, pad, momentum, eps, act, slope = inputs
    _a, y, mean, rstd, _rm, _rv = output
    ctx.save_for_backward(x, w, y, mean, rstd, gamma, beta)
    ctx.cfg = (stride, pad, act, slope, b is not None)


def _cba_backward(ctx, da, _dy, _dm, _dr, _drm, _drv):
    x, w, y, mean, rstd, gamma, beta = ctx.saved_tensors
    stride, pad, act, slope, has_b = ctx.cfg
    dx, dw, db, dgamma, dbeta = torch.ops.mi355seg.conv_bn_act_backward(da, x, w, y, mean, rstd, gamma, beta, stride, pad, act, slope, has_b, ctx.needs_input_grad[0])
    return (dx if ctx.needs_input_grad[0] else None), dw, (db if has_b else None), dgamma, dbeta, None, None, None, None, None, None, None, None


torch.library.register_autograd("mi355seg::conv_bn_act", _cba_backward, setup_context=_cba_setup)


def conv_bn_act_train(x, conv, bn, act, slope=0.0):
    """One conv -> BatchNorm3d -> activation unit of the reference's blocks (unet3d.py:80-98) through the dispatcher, training mode."""
    stride, pad = F._module_stride_pad(conv, "conv_bn_act_train")
    a, _y, _m, _r, rm, rv = torch.ops.mi355seg.conv_bn_act(x, conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                                            stride, pad, float(bn.momentum), float(bn.eps), int(act), float(slope))
    with torch.no_grad():
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
        bn.num_batches_tracked.add_(1)
    return a


# ------------------------------------------------------------------------------------------------ activation, channel concat
@torch.library.custom_op("mi355seg::activation", mutates_args=())
def activation(x: Tensor, act: int, slope: float) -> Tensor:
    return F._Act.apply(x.detach(), None, act, slope)


@activation.register_fake
def _(x, act, slope):
    return torch.empty_like(x)


@torch.library.custom_op("mi355seg::activation_backward", mutates_args=())
def activation_backward(dy: Tensor, x: Tensor, act: int, slope: float) -> Tensor:
    xv, ldx = F.cl_view(x, "activation input")
    dyv, lddy = F.cl_view(F._like(dy, xv), "activation grad")
    C = xv.shape[-1]
    return F._act_bwd(dyv, lddy, xv, ldx, F._NO_RES, xv.numel() // C, C, act, slope)


@activation_backward.register_fake
def _(dy, x, act, slope):
    return torch.empty_like(x)


def _act_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0])
    ctx.cfg = (inputs[1], inputs[2])


torch.library.register_autograd("mi355seg::activation", lambda ctx, dy: (torch.ops.mi355seg.activation_backward(dy, ctx.saved_tensors[0], *ctx.cfg), None, None),
                                setup_context=_act_setup)


@torch.library.custom_op("mi355seg::cat_channels", mutates_args=())
def cat_channels(a: Tensor, b: Tensor) -> Tensor:
    """torch.cat((a, b), dim=channel) for channel-last tensors (unet3d.py:60-70): two strided row copies."""
    return F._CatChannels.apply(a.detach(), b.detach())


@cat_channels.register_fake
def _(a, b):
    return a.new_empty(tuple(a.shape[:-1]) + (a.shape[-1] + b.shape[-1],))


def _cat_setup(ctx, inputs, output):
    ctx.ca = inputs[0].shape[-1]


torch.library.register_autograd("mi355seg::cat_channels", lambda ctx, g: (g[..., :ctx.ca].contiguous(), g[..., ctx.ca:].contiguous()), setup_context=_cat_setup)


OPS = ["conv3d", "conv3d_dgrad", "conv3d_wgrad", "conv_transpose3d_k2s2", "conv_transpose3d_k2s2_backward", "max_pool3d_2x",
       "max_pool3d_2x_backward", "upsample_nearest_2x", "upsample_nearest_2x_backward", "bce_argmax_dice", "bce_with_logits_backward",
       "dice_counts", "confusion_counts", "hd95", "connected_components", "connected_components_by_class", "to_channels_last", "to_channels_first", "norm_stats", "norm_apply_act", "norm_act_backward", "conv_bn_act",
       "conv_bn_act_backward", "activation", "activation_backward", "cat_channels"]
