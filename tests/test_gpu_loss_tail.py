"""The fused tail of the compound losses (csrc/loss_tail.hip through functional.loss_tail, utils.loss_function.CompoundLoss,
engine.train_step and train.py's config.loss) against the fp64 CPU restatement of DESIGN.md 4.16's table
(tests/test_loss_tail_host.py::ref_tail) on the same seeded fp32 inputs, with ATen-CPU fp32's own error printed beside every
graded figure (``pytest -rA``), as tests/test_gpu_losses.py does.

Bounds (the project's, tests/test_gpu_losses.py):
  * loss and the two terms: 1e-6 * max(1, |ref|);
  * the per-class sums: 1e-6 relative with the denominator clamped at 1;
  * the gradient: 1e-9 + 2e-5 * max|ref| -- for EVERY mode.  focal, dice_focal and tversky were allowed up to 4x the ATen-fp32 error
    if this did not fit; it fits, so no factor was chosen.  Measured on an MI355X, worst case per mode as kernel error (ATen-fp32
    error) and share of this bound: focal 2.0e-9 (2.0e-9) 5.1 % and dice_focal 2.1e-9 (1.9e-9) 5.1 %, both at gamma = 8 (the powf
    path); tversky 1.4e-8 (1.4e-8) 2.9 %; dice 4.2 %, dice_bce 1.3 %, ce 1.1 %, dice_ce 1.0 % (DESIGN.md 4.16 has the table).
  * mask and the four counters: equality, and bitwise equality with functional.bce_argmax_dice;
  * against the library composition: twice the loss bound, twice the gradient bound -- and, for the one-hot targets used there, the
    same bits in the gradient."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from test_loss_tail_host import MODES, TERMS, ref_tail

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-6
LIB_GRAD = 2e-5
SUMS_TOL = 1e-6
F64, F32 = torch.float64, torch.float32
UP = 1.7                                     # every backward runs under (1.7 * loss).backward()
SIGMOID_MODES = tuple(m for m in MODES if TERMS[m][0] != "ce")

# tests/test_gpu_losses.py's SMALL, by value: S = 1, prime S, numel % 4 in {0, 1, 2, 3}, K in {1, 2, 3, 4, 5, 16}
SMALL = [
    (1, 2, 1, 1, 1), (3, 2, 1, 1, 1), (3, 1, 1, 1, 7), (1, 3, 1, 3, 3), (1, 5, 2, 3, 5), (3, 4, 3, 5, 7), (1, 16, 1, 1, 13),
    (3, 5, 1, 1, 211), (2, 3, 5, 7, 11),
]
VEC = [(2, 2, 4, 6, 8), (1, 4, 3, 4, 4), (2, 8, 2, 2, 4)]      # S % 4 == 0: the 16-byte paths (K <= 4), and K = 8 beside them
BIG = (2, 2, 97, 101, 113)                   # N * S = 2,214,122 > 2 * 2,048 * 256: past the grid cap, every thread makes several trips
SHAPES = SMALL + VEC + [BIG]


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mi355seg
    mi355seg.lib()          # raises if the HIP library is missing -- no fallback
    return mi355seg


def _lf():
    from mi355seg.utils import loss_function
    return loss_function


def _sid(s):
    return "x".join(str(v) for v in s)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _maxabs(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _admits(mode, shape):
    return shape[1] >= 2 or TERMS[mode][0] != "ce"


_CASES = {}


def _case(shape):
    """logits (a few units), labels, one-hot and soft target of one shape -- made once, shared, never modified"""
    if shape not in _CASES:
        N, K = shape[:2]
        base = 1000 * (sum(shape) % 97)
        x = torch.randn(shape, generator=_gen(base + 1)) * 3.0
        lab = torch.randint(0, K, (N,) + tuple(shape[2:]), generator=_gen(base + 2))
        onehot = torch.stack([(lab == i) for i in range(K)], dim=1).float()
        soft = torch.rand(shape, generator=_gen(base + 3))
        _CASES[shape] = (x, lab, onehot, soft)
    return _CASES[shape]


def _counts_ref(gt, pr):
    """utils/metric.py:26-43 (tests/test_gpu_losses.py's formula): value sums and the non-zero counts of the BITWISE and / or"""
    return [int(gt.sum()), int(pr.sum()), int(((gt & pr) != 0).sum()), int(((gt | pr) != 0).sum())]


def _ref(x, t, mode, dt, up=UP, **kw):
    """restatement in dtype dt: loss, terms[2], sums[K, 5], d(up * loss)/dx"""
    xr = x.detach().to(dt).requires_grad_(True)
    loss, v, r, sums = ref_tail(xr, t, mode, **kw)
    (loss * up).backward()
    return loss.detach(), torch.stack([v.detach(), r.detach()]), sums.detach(), xr.grad


def _spec(seg, mode, weights=(1.0, 1.0), gamma=2.0, alpha=0.3, beta=0.7):
    return seg.functional.LossSpec.from_mode(mode, weights, gamma, alpha, beta)


def _dev(seg, x, t, mode, up=UP, **kw):
    xg = x.detach().cuda().requires_grad_(True)
    loss, mask, counts, terms, sums = seg.functional.loss_tail_full(xg, t.cuda(), _spec(seg, mode, **kw))
    assert loss.dtype == F32 and loss.dim() == 0 and mask.dtype == torch.int64 and counts.dtype == torch.int64
    assert terms.dtype == F64 and tuple(terms.shape) == (2,) and sums.dtype == F64 and tuple(sums.shape) == (x.shape[1], 5)
    assert loss.requires_grad and not (mask.requires_grad or counts.requires_grad or terms.requires_grad or sums.requires_grad)
    (loss * up).backward()
    assert xg.grad.dtype == F32 and xg.grad.shape == x.shape
    return loss.detach().cpu(), mask.cpu(), counts.cpu().tolist(), terms.cpu(), sums.cpu(), xg.grad.cpu()


def _grade(tag, got, ref, aten, bound, den=None):
    got, ref, aten = [torch.as_tensor(v).detach().cpu().to(F64) for v in (got, ref, aten)]
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(aten).all()), f"{tag}: the CPU references must be finite"
    den = 1.0 if den is None else den
    ek, ea = _maxabs((got - ref) / den), _maxabs((aten - ref) / den)
    print(f"[loss_tail] {tag}: kernel error {ek:.3e}  ATen-fp32 error {ea:.3e}  bound {bound:.3e}  (max|ref| {_maxabs(ref):.3e})")
    assert bool(torch.isfinite(got).all()), f"{tag}: kernel result is not finite"
    assert ek <= bound, f"{tag}: kernel error {ek:.3e} > bound {bound:.3e} (ATen fp32: {ea:.3e})"
    return ek, ea


def _loss_bound(ref):
    return LOSS_TOL * max(1.0, _maxabs(torch.as_tensor(ref)))


def _grad_bound(ref):
    return 1e-9 + LIB_GRAD * _maxabs(ref)


def _check(seg, tag, x, t, mode, up=UP, **kw):
    """loss, terms, sums and gradient of one call against fp64 (ATen fp32 beside them); returns the device results"""
    l64, t64, s64, g64 = _ref(x, t, mode, F64, up, **kw)
    l32, t32, s32, g32 = _ref(x, t, mode, F32, up, **kw)
    out = _dev(seg, x, t, mode, up, **kw)
    loss, mask, counts, terms, sums, grad = out
    _grade(f"{tag} loss", loss, l64, l32, _loss_bound(l64))
    for i, name in enumerate(("voxel", "region")):
        _grade(f"{tag} terms[{name}]", terms[i], t64[i], t32[i], _loss_bound(t64[i]))
    _grade(f"{tag} sums", sums, s64, s32, SUMS_TOL, den=s64.abs().clamp_min(1))
    _grade(f"{tag} grad", grad, g64, g32, _grad_bound(g64))
    return out


# ----------------------------------------------------------------------------- shapes x modes x targets
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_every_mode_on_every_shape(seg, shape, mode):
    """Every mode on every shape it admits (ce needs K >= 2), one-hot targets and -- for the sigmoid modes -- soft targets: loss,
    both terms, the per-class sums and the gradient against fp64; mask and counters exact and bitwise those of bce_argmax_dice;
    dice_bce and dice_ce also against the composition of the library losses they replace."""
    if not _admits(mode, shape):
        with pytest.raises(seg.Mi355SegError, match="ce term needs K >= 2"):
            seg.functional.loss_tail(torch.zeros(shape).cuda(), torch.zeros(shape).cuda(), _spec(seg, mode))
        return
    F, LF = seg.functional, _lf()
    x, lab, onehot, soft = _case(shape)
    mask_r = x.argmax(1, keepdim=True)
    for name, t in (("onehot", onehot), ("soft", soft)):
        if name == "soft" and mode not in SIGMOID_MODES:
            continue
        tag = f"{mode} {_sid(shape)} {name}"
        loss, mask, counts, terms, sums, grad = _check(seg, tag, x, t, mode)
        assert torch.equal(mask, mask_r) and counts == _counts_ref(t.argmax(1, keepdim=True), mask_r), tag
        _, mask_b, counts_b = F.bce_argmax_dice(x.cuda(), t.cuda())
        assert torch.equal(mask.cuda(), mask_b) and counts == counts_b.cpu().tolist(), tag
    if mode in ("dice_bce", "dice_ce"):
        xg = x.cuda().requires_grad_(True)
        if mode == "dice_bce":
            comp = LF.DiceLoss()(xg, onehot.cuda()) + LF.BCEWithLogitsLoss()(xg, onehot.cuda())
        else:
            comp = LF.cross_entropy_3D(xg, lab.cuda()) + LF.DiceLoss()(xg, onehot.cuda())
        (comp * UP).backward()
        loss, _, _, _, _, grad = _dev(seg, x, onehot, mode)
        dl, dg = abs(float(loss) - float(comp.detach())), _maxabs(grad - xg.grad.cpu())
        lb, gb = 2 * _loss_bound(comp.detach().cpu()), 2 * _grad_bound(xg.grad.cpu())
        print(f"[loss_tail] {mode} {_sid(shape)} vs library composition: loss {dl:.3e} (bound {lb:.3e})  grad {dg:.3e} (bound {gb:.3e})")
        assert dl <= lb and dg <= gb
        # more than the bound: with 0 / 1 targets the backward returns the composition's bits (each term's gradient rounded as the
        # unfused kernels round it, then added) -- what keeps the zero-gradient parameters of a network where the composition has them
        assert torch.equal(grad, xg.grad.cpu()), f"{mode} {_sid(shape)}: the gradient differs from the composition's in {int((grad != xg.grad.cpu()).sum())} elements"


# ----------------------------------------------------------------------------- weights, upstream factor, parameters
@pytest.mark.parametrize("mode", MODES)
def test_weights_parameters_and_upstream_factor(seg, mode):
    """weights = (0.3, 2.0), other exponents and Tversky weights, upstream factors 0 and -3 (1.7 everywhere else)."""
    shape = (3, 4, 3, 5, 7)
    x, _, onehot, soft = _case(shape)
    t = soft if mode in SIGMOID_MODES else onehot
    _check(seg, f"{mode} weights (0.3, 2.0)", x, t, mode, weights=(0.3, 2.0))
    _check(seg, f"{mode} upstream -3", x, t, mode, up=-3.0)
    grad = _dev(seg, x, t, mode, up=0.0)[5]
    assert not bool(grad.any()), "an upstream factor of 0 gives an all-zero gradient"
    if TERMS[mode][0] == "focal":
        for gamma in (0.0, 1.0, 1.5, 3.0, 8.0):
            _check(seg, f"{mode} gamma {gamma}", x, t, mode, gamma=gamma)
    if mode == "tversky":
        for alpha, beta in ((0.5, 0.5), (0.0, 1.0), (1.0, 0.0), (0.0, 0.25), (2.0, 3.0)):
            _check(seg, f"tversky alpha {alpha} beta {beta}", x, t, mode, alpha=alpha, beta=beta)


def test_dice_bce_with_a_zero_region_weight_is_bce(seg):
    """weights = (1, 0) on dice_bce: the loss is BCE within the loss bound (fp64 BCE, and the live tail's own loss), the gradient too."""
    import torch.nn.functional as TF
    shape = (2, 3, 5, 7, 11)
    x, _, onehot, _ = _case(shape)
    loss, _, _, terms, _, grad = _dev(seg, x, onehot, "dice_bce", weights=(1.0, 0.0))
    xr = x.double().requires_grad_(True)
    bce = TF.binary_cross_entropy_with_logits(xr, onehot.double())
    (bce * UP).backward()
    live = seg.functional.bce_argmax_dice(x.cuda(), onehot.cuda())[0]
    print(f"[loss_tail] dice_bce (1, 0) vs bce: {abs(float(loss) - float(bce)):.3e}, vs the live tail {abs(float(loss) - float(live)):.3e}")
    assert abs(float(loss) - float(bce)) <= _loss_bound(bce.detach()) and abs(float(loss) - float(live)) <= _loss_bound(bce.detach())
    assert abs(float(terms[0]) - float(bce)) <= _loss_bound(bce.detach()) and float(terms[1]) > 0        # the region term is still reported
    assert _maxabs(grad.double() - xr.grad) <= _grad_bound(xr.grad)


# ----------------------------------------------------------------------------- value edges
MAGS = [0.0, 1e-3, 1.0, 20.0, 88.0, 1e4]
EDGE_VALUES = torch.tensor([s * m for m in MAGS for s in (1.0, -1.0)], dtype=F32)        # 12 values, -0.0 among them
EDGE_TARGETS = torch.tensor([0.0, 1.0, 0.25, 0.7], dtype=F32)


def _edge_grid():
    """[1, 2, 3, 4, 4] logits and targets: every edge value against every target in channel 0, the same table rolled in channel 1"""
    v = EDGE_VALUES.repeat_interleave(4)                        # 48
    t = EDGE_TARGETS.repeat(12)
    x = torch.stack([v, v.roll(5)]).reshape(1, 2, 3, 4, 4).clone()
    tt = torch.stack([t, t.roll(7)]).reshape(1, 2, 3, 4, 4).clone()
    return x, tt


@pytest.mark.parametrize("mode", MODES)
def test_value_edges(seg, mode):
    """Logits 0, +-1e-3, +-1, +-20, +-88, +-1e4 against targets 0, 1 and soft ones: finite loss and gradient, graded like any other
    input (the loss is of the order 1e3 here, so its bound is relative)."""
    x, t = _edge_grid()
    loss, mask, counts, _, _, grad = _check(seg, f"edges {mode}", x, t, mode)
    assert math.isfinite(float(loss)) and bool(torch.isfinite(grad).all())
    mask_r = x.argmax(1, keepdim=True)
    assert torch.equal(mask, mask_r) and counts == _counts_ref(t.argmax(1, keepdim=True), mask_r)


@pytest.mark.parametrize("mode", MODES)
def test_all_background_and_all_ones_targets(seg, mode):
    """T_k = 0 for every class but the background (the eps branch of the region terms), a saturated prediction against it, and a
    target of all ones."""
    shape = (2, 3, 4, 5, 6)
    x = _case(shape)[0]
    bg = torch.zeros(shape)
    bg[:, 0] = 1.0
    for name, xx, t in (("background", x, bg), ("background saturated", torch.full(shape, -30.0) + x / 3, bg), ("zeros", x, torch.zeros(shape)),
                        ("ones", x, torch.ones(shape))):
        _check(seg, f"{mode} target {name}", xx, t, mode)
    if mode == "tversky":
        for alpha, beta in ((0.0, 0.7), (0.3, 0.0)):
            _check(seg, f"tversky alpha {alpha} beta {beta} target background", x, bg, mode, alpha=alpha, beta=beta)


@pytest.mark.parametrize("gamma", [1.0, 2.0])
def test_focal_at_q_zero_and_q_one(seg, gamma):
    """q = p + t - 2 p t is exactly 0 (p == t) and exactly 1 (p == 1 - t) at saturated logits: the term is q^gamma * bce = 0 or 1e4,
    its gradient gamma q^(gamma-1) (1 - 2t) p (1 - p) bce + q^gamma (p - t) = 0 or +-1 (p (1 - p) == 0), for gamma = 1 (q^0 at q = 0)
    and 2."""
    x = torch.tensor([1e4, -1e4, 1e4, -1e4]).reshape(1, 1, 1, 1, 4)
    t = torch.tensor([1.0, 0.0, 0.0, 1.0]).reshape(1, 1, 1, 1, 4)
    loss, _, _, terms, _, grad = _check(seg, f"focal gamma {gamma} at q = 0, 1", x, t, "focal", gamma=gamma)
    assert float(loss) == 5000.0 and float(terms[0]) == 5000.0
    want = torch.tensor([0.0, 0.0, 0.25, -0.25]) * UP
    assert torch.equal(grad.reshape(-1), want.to(F32)), grad


@pytest.mark.parametrize("mode", MODES)
def test_one_nan_logit(seg, mode):
    """One NaN logit: the loss is NaN, the mask follows torch.argmax (the NaN wins its voxel), no other voxel's mask changes."""
    shape = (2, 3, 3, 5, 7)
    x, _, onehot, _ = _case(shape)
    clean = seg.functional.loss_tail(x.cuda(), onehot.cuda(), _spec(seg, mode))
    xn = x.clone()
    xn[1, 2, 1, 3, 4] = float("nan")
    loss, mask, counts, terms = seg.functional.loss_tail(xn.cuda(), onehot.cuda(), _spec(seg, mode))
    assert math.isnan(float(loss)) and math.isfinite(float(clean[0]))
    assert torch.equal(mask.cpu(), xn.argmax(1, keepdim=True)) and int(mask[1, 0, 1, 3, 4]) == 2
    diff = (mask != clean[1]).cpu()
    diff[1, 0, 1, 3, 4] = False
    assert not bool(diff.any())
    assert counts.cpu().tolist() == _counts_ref(onehot.argmax(1, keepdim=True), xn.argmax(1, keepdim=True))


# ----------------------------------------------------------------------------- views, determinism, the K cap
def _one_in(t):
    """The same values as a contiguous view that starts ONE element into a flat buffer: contiguous, but not 16-byte aligned"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def _permuted(t):
    """The same values, logical shape and dtype in a non-contiguous layout (the last two dimensions swapped in memory)"""
    d = t.dim()
    order = list(range(d - 2)) + [d - 1, d - 2]
    v = t.permute(order).contiguous().permute(order)
    assert v.shape == t.shape and not v.is_contiguous()
    return v


@pytest.mark.parametrize("mode", ["dice_bce", "dice_ce", "dice_focal", "tversky"])
def test_misaligned_and_permuted_views(seg, mode):
    """Logits and target one element into a flat buffer, and permuted: every output and the gradient bit-identical to the aligned
    contiguous copies' (aligned_contiguous); at a shape with S % 4 == 0, where the copies take the 16-byte paths."""
    F = seg.functional
    shape = (2, 3, 4, 6, 8)
    x, _, onehot, soft = _case(shape)
    t = soft if mode in SIGMOID_MODES else onehot

    def run(view):
        xs = view(x.cuda()).detach().requires_grad_(True)
        outs = F.loss_tail_full(xs, view(t.cuda()), _spec(seg, mode))
        (outs[0] * UP).backward()
        return [o.detach().clone() for o in outs] + [xs.grad.clone()]
    base = run(lambda v: v.clone(memory_format=torch.contiguous_format))
    for name, view in (("one element in", _one_in), ("permuted", _permuted)):
        for a, b in zip(run(view), base):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), f"{mode} {name}"


@pytest.mark.parametrize("shape", [(3, 4, 3, 5, 7), BIG], ids=_sid)
def test_two_calls_are_bitwise_equal_whatever_the_workspace_held(seg, shape):
    """Fixed-order partials, no atomics: loss, terms, sums, mask, counters and gradient of two calls are bitwise equal with the shared
    workspace overwritten with NaN (all bits set) in between -- every partial is written before it is read."""
    F = seg.functional
    x, _, onehot, _ = _case(shape)
    xg, tg = x.cuda(), onehot.cuda()
    for mode in ("dice_ce", "dice_focal", "tversky"):
        def run():
            xs = xg.detach().requires_grad_(True)
            outs = F.loss_tail_full(xs, tg, _spec(seg, mode))
            F.workspace(1, xs.device).fill_(255)
            (outs[0] * UP).backward()
            return [o.detach().clone() for o in outs] + [xs.grad.clone()]
        a = run()
        ws = F.workspace(1, xg.device)
        assert bool(torch.isnan(ws[:ws.numel() // 8 * 8].view(F64)).all())
        b = run()
        for u, v in zip(a, b):
            assert torch.equal(u, v), mode


def test_more_than_16_classes_raises(seg):
    """K = 17: refused by the C entry point before any launch (tests/test_loss_tail_host.py checks the same call without a GPU)."""
    x = torch.zeros((1, 17, 2, 3, 4)).cuda()
    for mode in ("dice", "dice_ce"):
        with pytest.raises(seg.Mi355SegError, match="K must be in 1..16, got 17"):
            seg.functional.loss_tail(x, x, _spec(seg, mode))
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- engine
def _unet_step(seg, criterion):
    from mi355seg.engine import train_step
    from mi355seg.models.three_d.unet3d import UNet3D
    from oracle.fill import fill_module_, make_input, make_labels
    x, gt = make_input((1, 1, 16, 16, 16)).cuda(), make_labels((1, 1, 16, 16, 16)).cuda()
    m = fill_module_(UNet3D(1, 2, 4)).cuda().train()
    out = train_step(m, torch.optim.Adam(m.parameters(), lr=1e-3), x, gt, criterion=criterion, sync_metric=False)
    return out, {k: p.grad.detach().cpu() for k, p in m.named_parameters()}, gt


@pytest.fixture(scope="module")
def unet_steps(seg):
    """the same first step of UNet3D(1, 2, 4) at [1, 1, 16^3] three times: CompoundLoss("dice_bce"), the unfused criterion, the default"""
    LF = _lf()
    fused, g_fused, gt = _unet_step(seg, LF.CompoundLoss("dice_bce"))
    plain, g_plain, _ = _unet_step(seg, lambda p, t: LF.DiceLoss()(p, t) + LF.BCEWithLogitsLoss()(p, t))
    default, _, _ = _unet_step(seg, None)
    return fused, g_fused, plain, g_plain, default, gt


def test_train_step_uses_the_tail_of_a_compound_loss(seg, unet_steps):
    """train_step(UNet3D(1, 2, 4), criterion=CompoundLoss("dice_bce")) at [1, 1, 16^3]: the loss equals the fp64 composition on the
    returned pred, mask and counters equal the default step's (and the unfused criterion's), and the two terms come back as
    'loss_terms' -- which no other criterion adds."""
    from oracle import losses as OL
    fused, _, plain, _, default, gt = unet_steps
    assert "loss_terms" in fused and "loss_terms" not in plain and "loss_terms" not in default
    pred = fused["pred"].detach().cpu().double()
    gt2 = seg.functional.two_channel_gt(gt).cpu().double()          # train.py:190-193, what the step hands its criterion
    dice, bce = OL.dice_loss(pred, gt2), OL.bce_with_logits(pred, gt2)
    print(f"[loss_tail] engine: loss {float(fused['loss']):.9f} fp64 composition {float(dice + bce):.9f}")
    assert abs(float(fused["loss"]) - float(dice + bce)) <= _loss_bound(dice + bce)
    terms = fused["loss_terms"].cpu()
    assert abs(float(terms[0]) - float(bce)) <= _loss_bound(bce) and abs(float(terms[1]) - float(dice)) <= _loss_bound(dice)
    assert torch.equal(fused["pred"], plain["pred"]) and torch.equal(fused["pred"], default["pred"])
    assert torch.equal(fused["mask"], default["mask"]) and torch.equal(fused["counts"], default["counts"])
    assert torch.equal(fused["mask"], plain["mask"]) and torch.equal(fused["counts"], plain["counts"])


def test_train_step_parameter_gradients_equal_the_unfused_criterions(seg, unet_steps):
    """Every parameter's gradient of the fused step against the same step with the unfused criterion
    ``lambda p, t: DiceLoss()(p, t) + BCEWithLogitsLoss()(p, t)``, within 2 * (1e-9 + 2e-5 * max|ref|) with ref that parameter's
    gradient in the unfused step.

    The biases of the convolutions that feed a BatchNorm decide this test: their exact gradient is ZERO (the norm removes a
    per-channel constant), what a step returns for them is the cancellation residue of a sum of terms of the size of the weight
    gradients (1e-2 here, residue 1e-9 .. 1e-8), and a change of the logit gradient in its last bit redraws it.  A backward that
    rounds the sum of the two terms once moves encoder1.enc1conv1.bias by 1.68e-8 and decoder2.dec2conv1.bias by 2.65e-9 (bound
    2.0e-9) while the other 68 parameters stay below 2 per cent of their bounds.  loss_tail_bwd_kernel therefore forms each
    term's gradient as the unfused kernels do, rounds it and adds the two as autograd does: the logit gradient has the composition's
    bits for 0 / 1 targets (test_every_mode_on_every_shape asserts it), and measured on an MI355X every difference here is 0."""
    _, g_fused, _, g_plain, _, _ = unet_steps
    bad = []
    for k, ref in g_plain.items():
        err, bound = _maxabs(g_fused[k] - ref), 2 * _grad_bound(ref)
        print(f"[loss_tail] engine grad {k}: difference {err:.3e}  bound {bound:.3e}  (max|ref| {_maxabs(ref):.3e})")
        if not err <= bound:
            bad.append(f"{k}: {err:.3e} > {bound:.3e} (max|ref| {_maxabs(ref):.3e})")
    assert not bad, "; ".join(bad)


_GRAPHED = r"""
import sys, torch
sys.path.insert(0, %r)
import mi355seg
from mi355seg.engine import GraphedTrainStep, train_step
from mi355seg.models.three_d.unet3d import UNet3D
from mi355seg.utils.loss_function import CompoundLoss
from oracle.fill import fill_module_, make_input, make_labels
x, gt = make_input((1, 1, 16, 16, 16)).cuda(), make_labels((1, 1, 16, 16, 16)).cuda()

def build():
    m = fill_module_(UNet3D(1, 2, 4)).cuda().train()
    return m, torch.optim.Adam(m.parameters(), lr=1e-3, capturable=True), CompoundLoss("dice_bce")

m0, o0, c0 = build()
for _ in range(4):
    e = train_step(m0, o0, x, gt, criterion=c0, sync_metric=False)
l0, t0 = e["loss"].item(), e["loss_terms"].tolist()
m1, o1, c1 = build()
g = GraphedTrainStep(m1, o1, x, gt, criterion=c1, warmup=1)
assert "loss_terms" in g.first
for _ in range(3):
    r = g(x, gt, sync_metric=False)
l1, t1 = r["loss"].item(), r["loss_terms"].tolist()
torch.cuda.synchronize()
assert l0 == l1 and t0 == t1, (l0, l1, t0, t1)
for (k, a), (_, b) in zip(m0.state_dict().items(), m1.state_dict().items()):
    assert torch.equal(a, b), k
print("GRAPHED_COMPOUND_LOSS_OK", l1)
"""


def test_graphed_step_with_a_compound_loss_equals_the_eager_steps(seg):
    """Four eager steps with CompoundLoss("dice_bce") and a capturable Adam against GraphedTrainStep(criterion=..., warmup=1) plus
    three replays: the last loss, its terms and every state-dict entry bitwise equal -- nothing of the tail goes through the host.
    Run once, in a process of its own, with a timeout."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _GRAPHED % root], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "GRAPHED_COMPOUND_LOSS_OK" in p.stdout, (p.returncode, p.stdout[-1000:], p.stderr[-3000:])


# ----------------------------------------------------------------------------- train.py
def _train_rows(tmp_path, name, extra, seed=11):
    from mi355seg.train import main
    torch.manual_seed(seed)
    cfg, res = main(["config=unet", f"config.output_dir={tmp_path / name}", "config.data_path=synthetic", "config.patch_size=16,16,16",
                     "config.epochs=1"] + extra)
    rows = [json.loads(l) for l in open(os.path.join(cfg.hydra_path, "scalars.jsonl")).read().strip().splitlines()]
    return cfg, res, rows


def test_train_cli_config_loss(seg, tmp_path):
    """``train.py ... config.loss=dice_bce``: a checkpoint and a scalars.jsonl whose rows hold both term keys, with Training/Loss =
    voxel + region; ``config.loss=bce`` and no key at all write bitwise equal Training/Loss sequences without the term keys."""
    cfg, res, rows = _train_rows(tmp_path, "dice_bce", ["config.loss=dice_bce"])
    assert os.path.exists(os.path.join(cfg.hydra_path, "latest_checkpoint.pt")) and len(rows) == 4 and res["epoch"] == 1
    for r in rows:
        assert {"Training/Loss", "Training/dice", "Training/loss_voxel", "Training/loss_region"} <= set(r)
        assert 0.0 < r["Training/loss_voxel"] and 0.0 < r["Training/loss_region"] < 1.0
        assert abs(r["Training/Loss"] - (r["Training/loss_voxel"] + r["Training/loss_region"])) <= 1e-6 * max(1.0, r["Training/Loss"])
    _, _, bce = _train_rows(tmp_path, "bce", ["config.loss=bce"])
    _, _, absent = _train_rows(tmp_path, "absent", [])
    assert [r["Training/Loss"] for r in bce] == [r["Training/Loss"] for r in absent] and len(bce) == 4
    assert all("Training/loss_voxel" not in r and "Training/loss_region" not in r for r in bce + absent)
    assert [r["Training/Loss"] for r in bce] != [r["Training/Loss"] for r in rows]
    with pytest.raises(ValueError, match="config.loss"):
        _train_rows(tmp_path, "bad", ["config.loss=dice+bce"])
