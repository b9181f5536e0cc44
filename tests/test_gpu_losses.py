"""The kernels of csrc/loss.hip (BCE-with-logits, channel argmax, Dice counters, the fused bce_argmax_dice tail, two_channel_gt,
dice_sums, dice_rows, channel softmax, ce3d, znorm) against the same operation in plain torch on the CPU in FLOAT64, on the same
seeded fp32 inputs, through the public Python surface (functional.*, utils.loss_function.*, utils.metric.metric): at sizes with
every ``numel % 4`` tail, past the 2,048-block grid cap (every thread makes two trips, the last one ragged), at the value edges of
expf / log1pf / the max-subtracted softmax, with labels outside [0, K), through misaligned and permuted views, and at the sizes
the benchmark times them at.

Bounds (the project's own, tests/test_gpu_ops.py::test_bce_argmax_dice and
tests/test_gpu_models.py::test_library_losses_vs_reference_fixture):
  * a scalar loss: 1e-6 absolute, relative to the fp64 value where that exceeds 1 (``LOSS_TOL * max(1, |ref|)``);
  * gradients: 1e-9 + 1e-5 * max|ref| (BCE), 1e-9 + 2e-5 * max|ref| (the library losses);
  * dice_sums / dice_rows sums: 1e-6 relative with the denominator clamped at 1;
  * integer results (masks, counters, two_channel_gt): equality.
Two bounds the project had not set come from the number formats and are derived where they are defined (SOFTMAX, ZNORM below).
Every graded quantity is also computed by ATen-CPU in fp32 and printed (``pytest -rA``): kernel error, ATen-fp32 error, bound."""
import math

import pytest
import torch
import torch.nn.functional as TF

from oracle import losses as OL

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-6
BCE_GRAD = 1e-5
LIB_GRAD = 2e-5
SUMS_TOL = 1e-6
F64 = torch.float64
F32 = torch.float32


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mi355seg
    mi355seg.lib()          # raises if the HIP library is missing -- no fallback
    return mi355seg


# ----------------------------------------------------------------------------- helpers
def _lf():
    from mi355seg.utils import loss_function
    return loss_function


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=_gen(seed)) * scale


def _labels(shape, K, seed):
    return torch.randint(0, K, shape, generator=_gen(seed))


def _onehot(lab, K):
    """[N, *] int64 -> [N, K, *] float"""
    return torch.stack([(lab == i) for i in range(K)], dim=1).float()


def _maxabs(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _grade(tag, got, ref, aten, bound):
    """|got - ref| <= bound (max norm), with ATen-CPU fp32's own distance from the fp64 reference printed beside it."""
    got, ref, aten = [torch.as_tensor(v).detach().cpu().to(F64) for v in (got, ref, aten)]
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(aten).all()), f"{tag}: the CPU references must be finite"
    ek, ea = _maxabs(got - ref), _maxabs(aten - ref)
    print(f"[losses] {tag}: kernel error {ek:.3e}  ATen-fp32 error {ea:.3e}  bound {bound:.3e}  (max|ref| {_maxabs(ref):.3e})")
    assert bool(torch.isfinite(got).all()), f"{tag}: kernel result is not finite"
    assert ek <= bound, f"{tag}: kernel error {ek:.3e} > bound {bound:.3e} (ATen fp32: {ea:.3e})"
    return ek, ea


def _loss_bound(ref):
    return LOSS_TOL * max(1.0, abs(float(ref)))


def _grad_bound(ref, c):
    return 1e-9 + c * _maxabs(ref)


def _grade_full_size_grad(tag, got, ref, aten, c):
    """The project's gradient bound, and beside it the same coefficient WITHOUT the 1e-9 floor: at 78.6 M elements a mean-reduced
    loss has gradient entries of 1e-7, and the floor alone would let an error of one per cent pass."""
    ek, ea = _grade(tag, got, ref, aten, _grad_bound(ref, c))
    m = _maxabs(ref)
    print(f"[losses] {tag}, relative to max|ref|: kernel {ek / m:.3e}  ATen-fp32 {ea / m:.3e}  bound {c:.1e}")
    assert ek <= c * m, f"{tag}: kernel error {ek / m:.3e} of max|ref| > {c:.1e}"


def _grade_sums(tag, got, ref, aten):
    """dice_sums / dice_rows: |got - ref| / max(|ref|, 1) <= 1e-6"""
    got, ref, aten = [v.detach().cpu().to(F64) for v in (got, ref, aten)]
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(aten).all()), f"{tag}: the CPU references must be finite"
    den = ref.abs().clamp_min(1)
    ek, ea = _maxabs((got - ref) / den), _maxabs((aten - ref) / den)
    print(f"[losses] {tag}: kernel error {ek:.3e}  ATen-fp32 error {ea:.3e}  bound {SUMS_TOL:.3e}  (relative, denominator >= 1)")
    assert bool(torch.isfinite(got).all()) and ek <= SUMS_TOL, f"{tag}: kernel error {ek:.3e} > {SUMS_TOL:.1e} (ATen fp32: {ea:.3e})"


def _cpu(fn, x, dt, up=1.7):
    """value and d(up * value)/dx of fn on the CPU in dtype dt; fn(x, dt) casts its other operands itself"""
    xr = x.detach().to(dt).requires_grad_(True)
    val = fn(xr, dt)
    (val * up).backward()
    return val.detach(), xr.grad


def _dev(fn, x, up=1.7):
    xg = x.detach().cuda().requires_grad_(True)
    val = fn(xg)
    (val * up).backward()
    return val.detach().cpu(), xg.grad.cpu()


def _check_loss(tag, x, cpu_fn, dev_fn, grad_c, up=1.7):
    """A scalar loss and its input gradient on the device against fp64 (and ATen fp32 beside it)."""
    v64, g64 = _cpu(cpu_fn, x, F64, up)
    v32, g32 = _cpu(cpu_fn, x, F32, up)
    vd, gd = _dev(dev_fn, x, up)
    assert vd.dtype == F32 and gd.dtype == F32 and gd.shape == x.shape
    _grade(tag + " loss", vd, v64, v32, _loss_bound(v64))
    _grade(tag + " grad", gd, g64, g32, _grad_bound(g64, grad_c))
    return vd, gd


def _sums_ref(x, t, dt, sig, p=2.0):
    a = torch.sigmoid(x.to(dt)) if sig else x.to(dt)
    b = t.to(dt)
    return torch.stack([(a * b).sum(-1), a.sum(-1), b.sum(-1), a.pow(p).sum(-1), b.pow(p).sum(-1)], dim=-1)


def _counts_ref(gt, pr):
    """utils/metric.py:26-43: value sums and the non-zero counts of the BITWISE and / or"""
    return [int(gt.sum()), int(pr.sum()), int(((gt & pr) != 0).sum()), int(((gt | pr) != 0).sum())]


# N, K, D, H, W: S = 1, prime S, numel % 4 in {0, 1, 2, 3}, N in {1, 3} (and 2), K in {1, 2, 3, 4, 5, 16}
SMALL = [
    (1, 2, 1, 1, 1),         # S = 1, numel 2
    (3, 2, 1, 1, 1),         # S = 1, N = 3, numel 6 (% 4 = 2)
    (3, 1, 1, 1, 7),         # K = 1, prime S, numel 21 (% 4 = 1)
    (1, 3, 1, 3, 3),         # numel 27 (% 4 = 3)
    (1, 5, 2, 3, 5),         # numel 150 (% 4 = 2)
    (3, 4, 3, 5, 7),         # numel 1260 (% 4 = 0), S = 105 odd
    (1, 16, 1, 1, 13),       # K = 16 (the softmax kernel's cap), prime S
    (3, 5, 1, 1, 211),       # prime S, numel 3165 (% 4 = 1)
    (2, 3, 5, 7, 11),        # numel 2310 (% 4 = 2)
]
# past the grid cap of 2,048 blocks x 256 threads: N * S > 2 * 524,288 (per-voxel kernels: two full trips and a ragged third) and
# numel > 4 * 2 * 524,288 (float4 kernels); the second one has an odd numel (% 4 = 1) so that the tail sits behind a wrapped grid
BIG = [
    (2, 2, 97, 101, 113),    # N * S = 2,214,122; numel = 4,428,244
    (1, 5, 101, 103, 107),   # N * S = 1,113,121; numel = 5,565,605
]
SHAPES = SMALL + BIG


def _sid(s):
    return "x".join(str(v) for v in s)


def _case(shape, seed=0):
    """logits (a few units), labels, one-hot target and a soft target for one sweep shape"""
    N, K, D, H, W = shape
    base = 1000 * (sum(shape) % 97) + seed
    x = _randn(shape, base + 1, 3.0)
    lab = _labels((N, D, H, W), K, base + 2)
    soft = torch.rand(shape, generator=_gen(base + 3))
    return x, lab, _onehot(lab, K), soft


# ----------------------------------------------------------------------------- A1: shape sweep
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_bce_with_logits_shapes(seg, shape):
    """bce_fwd_kernel / bce_bwd_kernel (float4 body, ``numel & 3`` tail, grid-stride wrap) through functional.bce_with_logits and
    the two criterion modules, one-hot and soft targets."""
    F, LF = seg.functional, _lf()
    x, _, onehot, soft = _case(shape)
    for name, t, fn in (("onehot", onehot, F.bce_with_logits), ("soft", soft, LF.Binary_Loss()), ("soft-module", soft, LF.BCEWithLogitsLoss())):
        _check_loss(f"bce {_sid(shape)} {name}", x, lambda z, dt, t=t: TF.binary_cross_entropy_with_logits(z, t.to(dt)),
                    lambda z, t=t, fn=fn: fn(z, t.cuda()), BCE_GRAD)


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_argmax_counts_and_fused_tail_shapes(seg, shape):
    """argmax_kernel, dice_counts_kernel and bce_argmax_dice_kernel: masks and counters exact, the fused loss and its gradient
    against fp64; the fused kernel's target argmax on a one-hot AND on a soft target."""
    F = seg.functional
    from mi355seg.utils.metric import metric, metric_from_counts
    N, K = shape[:2]
    x, _, onehot, soft = _case(shape)
    x[0, :, 0, 0, 0] = 0.25                                      # an exact tie across all classes: class 0 wins
    mask_r = x.argmax(1, keepdim=True)
    mask_g = F.argmax_channels(x.cuda())
    assert mask_g.dtype == torch.int64 and torch.equal(mask_g.cpu(), mask_r)
    for name, t in (("onehot", onehot), ("soft", soft)):
        gt_r = t.argmax(1, keepdim=True)
        want = _counts_ref(gt_r, mask_r)
        assert F.dice_counts(gt_r.cuda(), mask_g).cpu().tolist() == want
        assert metric(gt_r.cuda(), mask_g) == metric_from_counts(want)
        out = {}

        def fused(z, t=t, out=out):
            loss, out["mask"], out["counts"] = F.bce_argmax_dice(z, t.cuda())
            return loss
        _check_loss(f"bce_argmax_dice {_sid(shape)} {name}", x, lambda z, dt, t=t: TF.binary_cross_entropy_with_logits(z, t.to(dt)),
                    fused, BCE_GRAD)
        assert torch.equal(out["mask"].cpu(), mask_r) and out["counts"].cpu().tolist() == want


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_two_channel_gt_shapes(seg, shape):
    """two_channel_gt_kernel against cat([(gt == 0), gt], 1) (train.py:190-193), float and int64 label volumes."""
    F = seg.functional
    N, K, D, H, W = shape
    gt = _labels((N, 1, D, H, W), 2, 5 + sum(shape)).float()
    want = torch.cat([(gt == 0).float(), gt], dim=1)
    got = F.two_channel_gt(gt.cuda())
    assert got.dtype == F32 and torch.equal(got.cpu(), want)
    assert torch.equal(F.two_channel_gt(gt.long().cuda()).cpu(), want)


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_dice_sums_and_dice_loss_shapes(seg, shape):
    """dice_sums_kernel / dice_sums_bwd_kernel: the five sums with and without the sigmoid, the gradient under a full random fp64
    upstream vector (columns 2 and 4 do not depend on x: the gradient must ignore them), and DiceLoss on top."""
    F, LF = seg.functional, _lf()
    x, _, onehot, soft = _case(shape)
    g5 = torch.randn(5, generator=_gen(11), dtype=F64)
    x_signed = x
    for sig in (True, False):
        # without the sigmoid a long signed sum can cancel to less than the rounding of its own fp32 products (a relative bound says
        # nothing there): signed inputs at the tiny sizes, non-negative ones -- what the library feeds it, probabilities -- elsewhere
        x = x_signed if (sig or x_signed.numel() <= 32) else x_signed.abs()
        for name, t in (("onehot", onehot), ("soft", soft)):
            tag = f"dice_sums {_sid(shape)} sigmoid={sig} {name}"
            ref64, ref32 = _sums_ref(x.reshape(-1), t.reshape(-1), F64, sig), _sums_ref(x.reshape(-1), t.reshape(-1), F32, sig)
            got = F.dice_sums(x.cuda(), t.cuda(), apply_sigmoid=sig)
            assert got.dtype == F64 and tuple(got.shape) == (5,)
            _grade_sums(tag, got, ref64, ref32)

            def cpu_fn(z, dt, t=t, sig=sig):
                return (_sums_ref(z.reshape(-1), t.reshape(-1), dt, sig) * g5.to(dt)).sum()
            _, g64 = _cpu(cpu_fn, x, F64, 1.0)
            _, g32 = _cpu(cpu_fn, x, F32, 1.0)
            xg = x.cuda().requires_grad_(True)
            s = F.dice_sums_autograd(xg, t.cuda(), sig)
            _grade_sums(tag + " (autograd)", s, ref64, ref32)
            s.backward(g5.cuda(), retain_graph=True)
            _grade(tag + " grad", xg.grad, g64, g32, _grad_bound(g64, LIB_GRAD))
            first = xg.grad.clone()
            xg.grad = None
            g5b = g5.clone()
            g5b[2], g5b[4] = 123.0, -7.0
            s.backward(g5b.cuda())
            assert torch.equal(xg.grad, first), "columns 2 and 4 carry no dependence on x"
    _check_loss(f"DiceLoss {_sid(shape)}", x_signed, lambda z, dt: OL.dice_loss(z, onehot.to(dt)), lambda z: LF.DiceLoss()(z, onehot.cuda()), LIB_GRAD)


def _softmax_bound(K):
    """SOFTMAX (derived, the project had no bound for this tensor): outputs lie in [0, 1]; on the same fp32 inputs the kernel
    differs from exact arithmetic by the rounding of v - m (1/2 ulp of an argument whose exp is not negligible, i.e. below
    1e-7 of the output), expf (<= 2 ulp), K - 1 additions (<= K - 1 ulp of the sum), one reciprocal and one product (<= 2.5 ulp):
    (K + 8) ulp of 1 = (K + 8) * 2^-24 bounds it with a margin of about two.
    The backward, dx = y * (dy - sum_k dy y), is graded on the same scale times max|dy|: its dot product of K terms and the
    subtraction round at the size of dy, not of dx (a saturated voxel has dx of 1e-5 |dy| and still the rounding of |dy|), so
    the losses' bound relative to max|dx| does not fit this op."""
    return (K + 8) * 2.0 ** -24


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_softmax_channels_shapes(seg, shape):
    """softmax_ch_kernel / softmax_ch_bwd_kernel against torch.softmax(dim=1) in fp64, forward and backward (random upstream)."""
    F = seg.functional
    K = shape[1]
    x = _case(shape)[0]
    gy = _randn(shape, 13)
    y64, y32 = torch.softmax(x.double(), 1), torch.softmax(x, 1)
    xg = x.cuda().requires_grad_(True)
    y = F.softmax_channels(xg)
    _grade(f"softmax {_sid(shape)}", y, y64, y32, _softmax_bound(K))
    y.backward(gy.cuda())
    _, g64 = _cpu(lambda z, dt: (torch.softmax(z, 1) * gy.to(dt)).sum(), x, F64, 1.0)
    _, g32 = _cpu(lambda z, dt: (torch.softmax(z, 1) * gy.to(dt)).sum(), x, F32, 1.0)
    _grade(f"softmax {_sid(shape)} grad", xg.grad, g64, g32, _softmax_bound(K) * _maxabs(gy))


def test_softmax_channels_more_than_16_classes_raises(seg):
    """The C side holds a voxel's classes in registers and caps K at 16: softmax_channels with K = 17 raises, and so does
    DiceLossss(17)(..., softmax=True), which goes through it (without softmax=True it takes any class count)."""
    F, LF = seg.functional, _lf()
    x = _randn((1, 17, 2, 3, 4), 1).cuda()
    lab = _labels((1, 2, 3, 4), 17, 2).cuda()
    with pytest.raises(seg.Mi355SegError):
        F.softmax_channels(x)
    with pytest.raises(seg.Mi355SegError):
        LF.DiceLossss(17)(x, lab, softmax=True)
    got = LF.DiceLossss(17)(torch.softmax(x, 1), lab)
    want = OL.dice_loss_multiclass(torch.softmax(x.cpu().double(), 1), lab.cpu(), 17)
    assert abs(got.item() - float(want)) <= _loss_bound(want)


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_cross_entropy_3d_shapes(seg, shape):
    """ce3d_fwd_kernel / ce3d_bwd_kernel through utils.loss_function.cross_entropy_3D: with and without class weights, both
    size_average values."""
    LF = _lf()
    N, K = shape[:2]
    x, lab, _, _ = _case(shape)
    w = torch.rand(K, generator=_gen(17)) + 0.25
    for weight in (None, w):
        for sa in (True, False):
            _check_loss(f"ce3d {_sid(shape)} weight={weight is not None} size_average={sa}", x,
                        lambda z, dt, weight=weight, sa=sa: OL.cross_entropy_3d(z, lab, None if weight is None else weight.to(dt), sa),
                        lambda z, weight=weight, sa=sa: LF.cross_entropy_3D(z, lab.cuda(), weight, sa), LIB_GRAD)


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_dice_lossss_and_binary_dice_shapes(seg, shape):
    """DiceLossss (softmax_channels + dice_rows over (sample, class) rows) and BinaryDiceLoss (dice_rows over samples)."""
    LF = _lf()
    N, K = shape[:2]
    x, lab, onehot, _ = _case(shape)
    wts = [0.5 + 0.1 * i for i in range(K)]
    _check_loss(f"DiceLossss {_sid(shape)} softmax", x, lambda z, dt: OL.dice_loss_multiclass(z, lab, K, softmax=True),
                lambda z: LF.DiceLossss(K)(z, lab.cuda(), softmax=True), LIB_GRAD)
    _check_loss(f"DiceLossss {_sid(shape)} weighted", x, lambda z, dt: OL.dice_loss_multiclass(z, lab, K, weight=wts),
                lambda z: LF.DiceLossss(K)(z, lab.cuda(), weight=wts), LIB_GRAD)
    pr = torch.sigmoid(x)
    for red in ("mean", "sum"):
        _check_loss(f"BinaryDiceLoss {_sid(shape)} {red}", pr, lambda z, dt, red=red: OL.binary_dice_loss(z, onehot.to(dt), reduction=red),
                    lambda z, red=red: LF.BinaryDiceLoss(reduction=red)(z, onehot.cuda()), LIB_GRAD)


def _znorm_bound(x64, ref):
    """ZNORM (derived, the project had no per-op bound): the kernel forms mean and 1/std in fp64 and hands them to the apply pass as
    fp32 -- the mean moves by up to 1/2 ulp (<= 2^-24 |mean|), i.e. 2^-24 |mean| / std in the result; 1/std, the subtraction and
    the product add 1.5 ulp of the result, taken as 2^-22 max|result| with a margin of about two."""
    return 2.0 ** -24 * abs(float(x64.mean())) / float(x64.std()) + 2.0 ** -22 * _maxabs(ref)


ZNORM_CASES = [(2, 0.0), (5, 0.0), (6, 0.0), (7, 0.0), (1021, 3.0), (100003, 1000.0), (4428244, 1000.0), (5565605, -300.0)]


@pytest.mark.parametrize("n,offset", ZNORM_CASES, ids=[f"n{n}_off{int(o)}" for n, o in ZNORM_CASES])
def test_znormalize(seg, n, offset):
    """znorm_sums / finalize / apply: (x - mean) / std (unbiased) against fp64; n = 2, n % 4 in {1, 2, 3}, CT-like offsets (mean
    1000, std 1: the pivoted sums keep the variance), past the grid cap."""
    F = seg.functional
    x = _randn((n,), 19 + n) + offset
    x64 = x.double()
    ref = (x64 - x64.mean()) / x64.std()
    aten = (x - x.mean()) / x.std()
    got = F.znormalize(x.cuda())
    assert got.dtype == F32 and got.shape == x.shape
    _grade(f"znormalize n={n} offset={offset}", got, ref, aten, _znorm_bound(x64, ref))
    vol = x.reshape(1, 1, 1, 1, n)
    assert torch.equal(F.znormalize(vol.cuda()).reshape(-1), got)          # any shape: one volume


ROWS = ([(R, L) for R in (1, 2, 7) for L in (1, 3, 4, 1023, 4097, 70001)] + [(2049, L) for L in (1, 3, 4, 1023)]
        + [(65536, L) for L in (1, 3, 4)])


@pytest.mark.parametrize("R,L", ROWS, ids=[f"R{r}_L{l}" for r, l in ROWS])
def test_dice_rows(seg, R, L):
    """dice_rows_kernel (float4 path; the scalar path for R > 1 with L % 4 != 0; one block per row when R > 2048; slices of
    65,535 rows), its one-block-per-row finalize and dice_rows_bwd for p in {1, 2, 3, 1.5}, with and without the sigmoid, under a full random
    fp64 upstream [R, 5] (columns 2 and 4 ignored by the gradient)."""
    F = seg.functional
    x0 = _randn((R, L), 23 + R + L)
    t = torch.rand((R, L), generator=_gen(29 + R + L))
    t[:, ::3] = (t[:, ::3] > 0.5).float()                        # hard 0 / 1 among soft targets
    g = torch.randn((R, 5), generator=_gen(31), dtype=F64)
    for p in (1, 2, 3, 1.5):
        for sig in (True, False):
            # without the sigmoid: a^1.5 needs a >= 0, and a long signed sum can cancel to less than the rounding of its own fp32 terms
            # (a relative bound says nothing there) -- signed inputs for the short rows, non-negative ones (BinaryDiceLoss gets
            # probabilities) elsewhere
            x = x0 if (sig or (p != 1.5 and L <= 4 and R <= 7)) else x0.abs()
            tag = f"dice_rows R={R} L={L} p={p} sigmoid={sig}"
            ref64, ref32 = _sums_ref(x, t, F64, sig, p), _sums_ref(x, t, F32, sig, p)
            xg = x.cuda().requires_grad_(True)
            s = F.dice_rows_autograd(xg, t.cuda(), sig, p)
            assert s.dtype == F64 and tuple(s.shape) == (R, 5)
            _grade_sums(tag, s, ref64, ref32)
            s.backward(g.cuda(), retain_graph=True)
            _, g64 = _cpu(lambda z, dt: (_sums_ref(z, t, dt, sig, p) * g.to(dt)).sum(), x, F64, 1.0)
            _, g32 = _cpu(lambda z, dt: (_sums_ref(z, t, dt, sig, p) * g.to(dt)).sum(), x, F32, 1.0)
            _grade(tag + " grad", xg.grad, g64, g32, _grad_bound(g64, LIB_GRAD))
            first = xg.grad.clone()
            xg.grad = None
            gb = g.clone()
            gb[:, 2], gb[:, 4] = 5.0, -11.0
            s.backward(gb.cuda())
            assert torch.equal(xg.grad, first), "columns 2 and 4 carry no dependence on x"


@pytest.mark.parametrize("up", [0.0, 1.7, -3.0])
def test_upstream_scalar_factor(seg, up):
    """d(up * loss): gscale reaches bce_bwd / ce3d_bwd, the fp64 upstream vector reaches dice_sums_bwd / dice_rows_bwd / softmax_bwd;
    up = 0 gives an all-zero gradient."""
    F, LF = seg.functional, _lf()
    shape = (3, 4, 3, 5, 7)
    N, K = shape[:2]
    x, lab, onehot, soft = _case(shape, seed=7)
    cases = [
        ("bce", BCE_GRAD, lambda z, dt: TF.binary_cross_entropy_with_logits(z, soft.to(dt)), lambda z: F.bce_with_logits(z, soft.cuda())),
        ("bce_argmax_dice", BCE_GRAD, lambda z, dt: TF.binary_cross_entropy_with_logits(z, onehot.to(dt)), lambda z: F.bce_argmax_dice(z, onehot.cuda())[0]),
        ("ce3d", LIB_GRAD, lambda z, dt: OL.cross_entropy_3d(z, lab), lambda z: LF.cross_entropy_3D(z, lab.cuda())),
        ("DiceLoss", LIB_GRAD, lambda z, dt: OL.dice_loss(z, onehot.to(dt)), lambda z: LF.DiceLoss()(z, onehot.cuda())),
        ("DiceLossss", LIB_GRAD, lambda z, dt: OL.dice_loss_multiclass(z, lab, K, softmax=True), lambda z: LF.DiceLossss(K)(z, lab.cuda(), softmax=True)),
        ("BinaryDiceLoss", LIB_GRAD, lambda z, dt: OL.binary_dice_loss(torch.sigmoid(z), onehot.to(dt)),
         lambda z: LF.BinaryDiceLoss()(torch.sigmoid(z), onehot.cuda())),
    ]
    for name, c, cpu_fn, dev_fn in cases:
        _, gd = _check_loss(f"upstream {up} {name}", x, cpu_fn, dev_fn, c, up)
        if up == 0.0:
            assert not bool(gd.any()), name


# ----------------------------------------------------------------------------- A2: value edges
MAGS = [0.0, 1e-6, 1e-3, 1.0, 20.0, 88.7, 104.0, 1e4]            # the expf / log1pf regimes, both signs below
EDGE_VALUES = torch.tensor([s * m for m in MAGS for s in (1.0, -1.0)], dtype=F32)        # 16 values, -0.0 among them
EDGE_TARGETS = torch.tensor([0.0, 1.0, 0.25, 0.7], dtype=F32)


def _edge_grid():
    """[1, 2, 4, 4, 4] logits and targets: every edge value against every target in channel 0, the same table rolled by five in
    channel 1 (so the two channels disagree about the argmax)."""
    v = EDGE_VALUES.repeat_interleave(4)                        # 64
    t = EDGE_TARGETS.repeat(16)
    x = torch.stack([v, v.roll(5)]).reshape(1, 2, 4, 4, 4).clone()
    tt = torch.stack([t, t.roll(7)]).reshape(1, 2, 4, 4, 4).clone()
    return x, tt


def _edge_classes(K=4):
    """[2, K, 4, 8, 8] logits drawn from the edge values by a seeded draw, plus hand-made voxels (all equal, +-1e4 against each
    other, 104 against 88.7), and labels."""
    idx = torch.randint(0, 16, (2, K, 4, 8, 8), generator=_gen(41))
    x = EDGE_VALUES[idx].clone()
    x[0, :, 0, 0, 0] = 1e4
    x[0, :, 0, 0, 1] = torch.tensor([1e4, -1e4, 0.0, -0.0])[:K]
    x[0, :, 0, 0, 2] = torch.tensor([104.0, 88.7, -88.7, 20.0])[:K]
    x[0, :, 0, 0, 3] = torch.tensor([1e-6, -1e-6, 1e-3, 0.0])[:K]
    lab = _labels((2, 4, 8, 8), K, 43)
    return x, lab


def test_value_edges_bce_and_dice_sums(seg):
    """log1p(exp(-|x|)) and 1 / (1 + exp(-x)) at |x| in {0, 1e-6, 1e-3, 1, 20, 88.7, 104, 1e4} of both signs against targets 0, 1
    and soft ones: bce_with_logits, bce_argmax_dice (mask and counters too), dice_sums with the sigmoid, DiceLoss.  The loss is
    of the order 1e3 here (a 1e4 logit against the wrong target), so its bound is relative to the fp64 value."""
    F, LF = seg.functional, _lf()
    x, t = _edge_grid()
    bce = lambda z, dt: TF.binary_cross_entropy_with_logits(z, t.to(dt))
    _check_loss("edges bce", x, bce, lambda z: F.bce_with_logits(z, t.cuda()), BCE_GRAD)
    out = {}

    def fused(z):
        loss, out["mask"], out["counts"] = F.bce_argmax_dice(z, t.cuda())
        return loss
    _check_loss("edges bce_argmax_dice", x, bce, fused, BCE_GRAD)
    mask_r, gt_r = x.argmax(1, keepdim=True), t.argmax(1, keepdim=True)
    assert torch.equal(out["mask"].cpu(), mask_r) and out["counts"].cpu().tolist() == _counts_ref(gt_r, mask_r)
    _grade_sums("edges dice_sums sigmoid", F.dice_sums(x.cuda(), t.cuda(), apply_sigmoid=True),
                _sums_ref(x.reshape(-1), t.reshape(-1), F64, True), _sums_ref(x.reshape(-1), t.reshape(-1), F32, True))
    _check_loss("edges DiceLoss", x, lambda z, dt: OL.dice_loss(z, t.to(dt)), lambda z: LF.DiceLoss()(z, t.cuda()), LIB_GRAD)


def test_value_edges_softmax_and_cross_entropy(seg):
    """The max-subtracted softmax and logsumexp at the same magnitudes across K = 4: softmax_channels, cross_entropy_3D with and
    without class weights and both size_average values, DiceLossss(softmax=True)."""
    F, LF = seg.functional, _lf()
    x, lab = _edge_classes(4)
    y = F.softmax_channels(x.cuda())
    _grade("edges softmax", y, torch.softmax(x.double(), 1), torch.softmax(x, 1), _softmax_bound(4))
    w = torch.tensor([0.5, 1.0, 2.0, 0.25])
    for weight in (None, w):
        for sa in (True, False):
            _check_loss(f"edges ce3d weight={weight is not None} size_average={sa}", x,
                        lambda z, dt, weight=weight, sa=sa: OL.cross_entropy_3d(z, lab, None if weight is None else weight.to(dt), sa),
                        lambda z, weight=weight, sa=sa: LF.cross_entropy_3D(z, lab.cuda(), weight, sa), LIB_GRAD)
    _check_loss("edges DiceLossss softmax", x, lambda z, dt: OL.dice_loss_multiclass(z, lab, 4, softmax=True),
                lambda z: LF.DiceLossss(4)(z, lab.cuda(), softmax=True), LIB_GRAD)


NAN, INF = float("nan"), float("inf")
ARGMAX_VOXELS = [
    [1.0, 1.0, 1.0, 1.0],            # exact ties across K = 4: the first wins
    [0.5, 2.0, 2.0, 2.0],            # a tie that does not start at class 0
    [-INF, -INF, -INF, -INF],        # all -inf
    [0.0, INF, 3.0, INF],            # +inf in two classes
    [-INF, INF, -INF, INF],
    [-0.0, 0.0, -0.0, 0.0],          # -0.0 == +0.0: class 0
    [0.0, -0.0, -1.0, -0.0],
    [NAN, 1.0, 3.0, 2.0],            # NaN in class 0
    [1.0, NAN, 3.0, 2.0],            # NaN in a later class: it beats the 3
    [1.0, 5.0, 3.0, NAN],            # ... in the last
    [1.0, NAN, 3.0, NAN],            # NaN in two classes: the first NaN
    [NAN, NAN, NAN, NAN],
    [INF, NAN, -INF, 0.0],           # NaN beats +inf
    [3.0, 2.0, 1.0, 0.0],
    [0.0, 1.0, 2.0, 3.0],
]


def _argmax_tensor(rows):
    """[2, 4, 1, 3, len(rows)]: the voxels of ``rows`` repeated at six positions"""
    v = torch.tensor(rows, dtype=F32).t()                        # [4, V]
    return v.reshape(1, 4, 1, 1, -1).expand(2, 4, 1, 3, len(rows)).contiguous()


def test_argmax_value_edges(seg):
    """torch.argmax's order in argmax_kernel and in BOTH argmaxes of bce_argmax_dice_kernel: the first maximum wins, a NaN beats
    every number and the first NaN wins.  With NaN in the data the loss is NaN on both sides, so there only the mask and the
    counters are compared; the NaN-free voxels are graded with the loss as well."""
    F = seg.functional
    x = _argmax_tensor(ARGMAX_VOXELS)
    assert x.argmax(1)[0, 0, 0].tolist() == [0, 1, 0, 1, 1, 0, 0, 0, 1, 3, 1, 0, 1, 0, 3]          # what ATen does, spelled out
    # a target whose argmax meets the same edges in another order (soft, not one-hot): the rows rolled by four
    t = _argmax_tensor(ARGMAX_VOXELS[4:] + ARGMAX_VOXELS[:4])
    mask_r, gt_r = x.argmax(1, keepdim=True), t.argmax(1, keepdim=True)
    mask_g = F.argmax_channels(x.cuda())
    assert torch.equal(mask_g.cpu(), mask_r)
    assert torch.equal(F.argmax_channels(t.cuda()).cpu(), gt_r)
    want = _counts_ref(gt_r, mask_r)
    assert F.dice_counts(gt_r.cuda(), mask_g).cpu().tolist() == want
    loss, mask_f, counts_f = F.bce_argmax_dice(x.cuda(), t.cuda())
    assert torch.equal(mask_f.cpu(), mask_r) and counts_f.cpu().tolist() == want
    assert math.isnan(loss.item()) and math.isnan(float(TF.binary_cross_entropy_with_logits(x.double(), t.double())))
    # the NaN- and inf-free voxels: masks, counters and the loss
    fin = [r for r in ARGMAX_VOXELS if all(math.isfinite(v) for v in r)]
    xf = _argmax_tensor(fin)
    tf_ = torch.sigmoid(_argmax_tensor(fin[2:] + fin[:2]))       # a soft target in (0, 1) with ties of its own
    out = {}

    def fused(z):
        l, out["mask"], out["counts"] = F.bce_argmax_dice(z, tf_.cuda())
        return l
    _check_loss("argmax edges (finite) bce_argmax_dice", xf, lambda z, dt: TF.binary_cross_entropy_with_logits(z, tf_.to(dt)), fused, BCE_GRAD)
    mr, gr = xf.argmax(1, keepdim=True), tf_.argmax(1, keepdim=True)
    assert torch.equal(out["mask"].cpu(), mr) and out["counts"].cpu().tolist() == _counts_ref(gr, mr)


def test_two_channel_gt_label_values(seg):
    """Label values {0, -0.0, 1, 2, 0.5, -1}: the background channel is (gt == 0) -- true for -0.0 --, the second channel is gt."""
    F = seg.functional
    vals = torch.tensor([0.0, -0.0, 1.0, 2.0, 0.5, -1.0])
    gt = vals[torch.randint(0, 6, (3, 1, 3, 5, 7), generator=_gen(47))]
    gt[0, 0, 0, 0, :6] = vals
    want = torch.cat([(gt == 0).float(), gt], dim=1)
    got = F.two_channel_gt(gt.cuda()).cpu()
    assert torch.equal(got, want)
    assert torch.equal(torch.signbit(got[:, 1]), torch.signbit(gt[:, 0]))          # -0.0 passes through as it is


@pytest.mark.parametrize("kind", ["zeros", "ones", "multiclass"])
def test_dice_counts_and_metric_past_the_cap(seg, kind):
    """dice_counts / metric on masks that are all zero, all one, and multi-class int64 (the bitwise & / | of utils/metric.py:40-41:
    1 & 2 == 0 does not intersect, 1 | 2 counts once) at 2,214,122 elements: the counters stay exact."""
    F = seg.functional
    from mi355seg.utils.metric import metric
    from oracle.metric import metric as ometric
    shape = (2, 1, 97, 101, 113)
    if kind == "multiclass":
        gt, pr = _labels(shape, 4, 53), _labels(shape, 4, 59)
    else:
        gt = torch.zeros(shape, dtype=torch.int64) if kind == "zeros" else torch.ones(shape, dtype=torch.int64)
        pr = gt.clone()
    pairs = [(gt, pr)] if kind == "multiclass" else [(gt, pr), (gt, 1 - pr), (gt, _labels(shape, 2, 61))]
    for a, b in pairs:
        want = _counts_ref(a, b)
        assert F.dice_counts(a.cuda(), b.cuda()).cpu().tolist() == want
        assert metric(a.cuda(), b.cuda()) == ometric(a, b)
        assert metric(a.cuda().to(torch.int32), b.cuda().float()) == ometric(a, b)       # any dtype goes through int64


def test_empty_foreground(seg):
    """The smooth / eplison branches: an all-zero target, and a saturated all-negative prediction against it (every sum the ratio
    is made of is ~0): DiceLoss, BinaryDiceLoss, DiceLossss."""
    LF = _lf()
    shape = (2, 3, 4, 5, 6)
    K = 3
    zeros = torch.zeros(shape)
    lab_bg = torch.zeros((2, 4, 5, 6), dtype=torch.int64)        # every voxel is class 0: classes 1 and 2 have no foreground
    for name, x in (("random", _randn(shape, 67, 3.0)), ("saturated", torch.full(shape, -30.0) + _randn(shape, 71))):
        _check_loss(f"empty DiceLoss {name}", x, lambda z, dt: OL.dice_loss(z, zeros.to(dt)), lambda z: LF.DiceLoss()(z, zeros.cuda()), LIB_GRAD)
        _check_loss(f"empty BinaryDiceLoss {name}", x, lambda z, dt: OL.binary_dice_loss(torch.sigmoid(z), zeros.to(dt)),
                    lambda z: LF.BinaryDiceLoss()(torch.sigmoid(z), zeros.cuda()), LIB_GRAD)
        _check_loss(f"empty DiceLossss {name}", x, lambda z, dt: OL.dice_loss_multiclass(z, lab_bg, K, softmax=True),
                    lambda z: LF.DiceLossss(K)(z, lab_bg.cuda(), softmax=True), LIB_GRAD)
    # nothing predicted and nothing there: probabilities of exactly zero
    p0 = torch.zeros(shape)
    got = LF.BinaryDiceLoss()(p0.cuda(), zeros.cuda())
    assert got.item() == 0.0                                     # 1 - smooth / smooth
    got = LF.DiceLossss(K)(p0.cuda(), lab_bg.cuda())
    want = OL.dice_loss_multiclass(p0.double(), lab_bg, K)
    assert abs(got.item() - float(want)) <= _loss_bound(want)


# ----------------------------------------------------------------------------- A3: labels of cross_entropy_3D
def _ce_ref_ignoring(z, lab, K, weight, sa):
    """The fp64 F.nll_loss formulation with every label outside [0, K) mapped to ignore_index = -100 (the divisor stays numel)."""
    lab = torch.where((lab >= 0) & (lab < K), lab, torch.full_like(lab, -100))
    logp = TF.log_softmax(z, 1).permute(0, 2, 3, 4, 1).reshape(-1, K)
    loss = TF.nll_loss(logp, lab.reshape(-1), weight=weight, reduction="sum", ignore_index=-100)
    return loss / float(lab.numel()) if sa else loss


@pytest.mark.parametrize("bad", [-100, 4, -1, 2 ** 40], ids=["ignore_index", "K", "minus1", "2pow40"])
def test_cross_entropy_3d_labels_outside_the_classes(seg, bad):
    """functional.cross_entropy_3d's documented rule: a label outside [0, K) is ignored -- F.nll_loss's own behaviour for -100, and
    for K, -1 and 2**40 (where ATen raises) the call does not raise but treats the voxel the same way.  Value and gradient equal
    the fp64 F.nll_loss formulation, the gradient is EXACTLY zero on the ignored voxels, with and without class weights, both
    size_average values.  (2**40 truncated to 32 bits is 0: the kernel must compare the 64-bit label.)"""
    LF = _lf()
    N, K, D, H, W = 2, 4, 5, 7, 9
    x = _randn((N, K, D, H, W), 73, 3.0)
    lab = _labels((N, D, H, W), K, 79)
    lab[0, 1:3, 2:5, 3:8] = bad                                  # a block of them
    lab[1, 4, 6, 8] = bad                                        # and the very last voxel
    ignored = (lab == bad)
    if bad == -100:                                              # ATen itself agrees with the formulation used below
        assert float(OL.cross_entropy_3d(x.double(), lab)) == float(_ce_ref_ignoring(x.double(), lab, K, None, True))
    w = torch.tensor([0.5, 1.0, 2.0, 0.25])
    for weight in (None, w):
        for sa in (True, False):
            _, gd = _check_loss(f"ce3d label {bad} weight={weight is not None} size_average={sa}", x,
                                lambda z, dt, weight=weight, sa=sa: _ce_ref_ignoring(z, lab, K, None if weight is None else weight.to(dt), sa),
                                lambda z, weight=weight, sa=sa: LF.cross_entropy_3D(z, lab.cuda(), weight, sa), LIB_GRAD)
            gi = gd.permute(0, 2, 3, 4, 1)[ignored]
            assert gi.numel() == int(ignored.sum()) * K and not bool(gi.any()), "the gradient of an ignored voxel is exactly zero"
            assert bool(gd.permute(0, 2, 3, 4, 1)[~ignored].any())


def test_cross_entropy_3d_bad_labels_touch_nothing_outside_the_tensors(seg):
    """Canary around the C entry points: logits, class weights, labels and dlogits are the MIDDLE slices of larger buffers filled
    with a sentinel; after forward and backward on labels {K, -1, -100, 2**40, 2**31 + 1} the sentinels are intact, the loss
    equals the ignoring fp64 reference and dlogits is finite everywhere (zero on the ignored voxels)."""
    F = seg.functional
    L = seg.lib()
    N, K, S = 2, 4, 5 * 7 * 9
    n = N * K * S
    SENT = -12345.5
    x = _randn((N, K, 5, 7, 9), 83, 3.0)
    lab = _labels((N, 5, 7, 9), K, 89)
    flat = lab.view(-1)
    bads = [K, -1, -100, 2 ** 40, 2 ** 31 + 1, -(2 ** 40), K + 1000000]
    for i, b in enumerate(bads):
        flat[i * 17 + 3] = b
    flat[-1] = K
    w = torch.tensor([0.5, 1.0, 2.0, 0.25])
    bx = torch.full((3 * n,), SENT, device="cuda")
    bd = torch.full((3 * n,), SENT, device="cuda")
    bw = torch.full((3 * K,), SENT, device="cuda")
    bl = torch.full((3 * N * S,), 2 ** 50, dtype=torch.int64, device="cuda")
    bx[n:2 * n] = x.reshape(-1).cuda()
    bw[K:2 * K] = w.cuda()
    bl[N * S:2 * N * S] = flat.cuda()
    xs, ds, wsl, ls = bx[n:2 * n], bd[n:2 * n], bw[K:2 * K], bl[N * S:2 * N * S]
    loss = torch.empty((), device="cuda")
    gscale = torch.ones(1, device="cuda")
    ws = F.workspace(L.query("mi355seg_loss_ws_bytes", n), xs.device)
    st = torch.cuda.current_stream().cuda_stream
    L.call("mi355seg_ce3d_fwd_f32", xs.data_ptr(), ls.data_ptr(), wsl.data_ptr(), N, K, S, 1, loss.data_ptr(), ws.data_ptr(), ws.numel(), st)
    L.call("mi355seg_ce3d_bwd_f32", xs.data_ptr(), ls.data_ptr(), wsl.data_ptr(), gscale.data_ptr(), N, K, S, 1, ds.data_ptr(), st)
    torch.cuda.synchronize()
    for buf, m in ((bx, n), (bd, n), (bw, K)):
        assert bool((buf[:m] == SENT).all()) and bool((buf[2 * m:] == SENT).all()), "a sentinel next to the tensors changed"
    assert bool((bl[:N * S] == 2 ** 50).all()) and bool((bl[2 * N * S:] == 2 ** 50).all())
    assert torch.equal(xs.cpu(), x.reshape(-1)) and torch.equal(ls.cpu(), flat)
    v64, g64 = _cpu(lambda z, dt: _ce_ref_ignoring(z, lab, K, w.to(dt), True), x, F64, 1.0)
    v32, g32 = _cpu(lambda z, dt: _ce_ref_ignoring(z, lab, K, w.to(dt), True), x, F32, 1.0)
    d = ds.cpu().view(N, K, 5, 7, 9)
    assert bool(torch.isfinite(d).all())
    _grade("ce3d canary loss", loss, v64, v32, _loss_bound(v64))
    _grade("ce3d canary grad", d, g64, g32, _grad_bound(g64, LIB_GRAD))
    bad = (lab < 0) | (lab >= K)
    assert int(bad.sum()) == len(bads) + 1 and not bool(d.permute(0, 2, 3, 4, 1)[bad].any())


# ----------------------------------------------------------------------------- A4: views
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
    assert v.shape == t.shape and (not v.is_contiguous() or t.shape[-1] == 1 or t.shape[-2] == 1)
    return v


def _run_views(fn, x, *others):
    """fn(x, *others) -> tensor or tuple of tensors; run on an aligned clone, on the one-element-in view and on the permuted view of
    EVERY operand; outputs and the gradient w.r.t. x (upstream: ones scaled by 1.7 over the first output) must be bit-identical."""
    def run(view):
        xs = view(x).detach().requires_grad_(True)
        out = fn(xs, *[view(o) for o in others])
        outs = out if isinstance(out, (tuple, list)) else (out,)
        if outs[0].requires_grad:
            (outs[0].float() * 1.7).sum().backward()
        return [o.detach().clone() for o in outs], (None if xs.grad is None else xs.grad.clone())
    base_o, base_g = run(lambda t: t.clone(memory_format=torch.contiguous_format))
    for name, view in (("one element in", _one_in), ("permuted", _permuted)):
        o, g = run(view)
        assert len(o) == len(base_o)
        for a, b in zip(o, base_o):
            assert a.dtype == b.dtype and torch.equal(a, b), f"{name}: output differs from the aligned clone's"
        assert (g is None) == (base_g is None)
        if g is not None:
            assert g.shape == x.shape and torch.equal(g, base_g), f"{name}: gradient differs from the aligned clone's"
    return base_o, base_g


def test_loss_entry_points_on_misaligned_and_permuted_views(seg):
    """bce_with_logits, bce_argmax_dice, znormalize, dice_sums(_autograd) and cross_entropy_3D on a contiguous view one element
    into a flat buffer (where ``.contiguous()`` alone leaves the pointer misaligned and the float4 entry points answer EINVAL) and
    on a permuted input: value and gradient bit-identical to the same call on an aligned clone."""
    F, LF = seg.functional, _lf()
    shape = (2, 3, 3, 5, 7)                                      # K * S = 315: x[1:] of such a batch is misaligned as well
    x = _randn(shape, 97, 3.0).cuda()
    t = torch.rand(shape, generator=_gen(101)).cuda()
    lab = _labels((2, 3, 5, 7), 3, 103).cuda()
    o, g = _run_views(lambda a, b: F.bce_with_logits(a, b), x, t)
    assert g is not None and abs(o[0].item() - float(TF.binary_cross_entropy_with_logits(x.cpu().double(), t.cpu().double()))) < 1e-6
    _run_views(lambda a, b: F.bce_argmax_dice(a, b), x, t)
    _run_views(lambda a, b: F.dice_sums(a, b, True), x, t)
    _run_views(lambda a, b: F.dice_sums_autograd(a, b, True)[0] + F.dice_sums_autograd(a, b, False)[3], x, t)
    _run_views(lambda a: LF.cross_entropy_3D(a, lab), x)
    _run_views(lambda a, b: LF.DiceLoss()(a, b), x, t)
    o, _ = _run_views(lambda a: F.znormalize(a), x)
    assert abs(float(o[0].mean())) < 1e-5
    # a batch slice: contiguous, storage offset K * S = 315 elements
    xb, tb = torch.cat([x, x]), torch.cat([t, t])
    assert xb[1:].is_contiguous() and xb[1:].data_ptr() % 16 != 0
    v = xb[1:].detach().requires_grad_(True)
    l = F.bce_with_logits(v, tb[1:])
    l.backward()
    c = xb[1:].clone().requires_grad_(True)
    lc = F.bce_with_logits(c, tb[1:].clone())
    lc.backward()
    assert torch.equal(l, lc) and torch.equal(v.grad, c.grad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_channel_last_ops_on_misaligned_and_permuted_views(seg, dtype):
    """cl_view hands the float4 / 8 x bf16 paths an aligned tensor: activation, instance_norm_act, max_pool3d_2x and
    upsample_nearest_2x on a contiguous [N, D, H, W, C] view one element into a flat buffer and on a permuted one -- result and
    input gradient bit-identical to the aligned clone's."""
    F = seg.functional
    x = _randn((2, 4, 6, 8, 8), 107).cuda().to(dtype)
    xv, ld = F.cl_view(_one_in(x))
    assert ld == 8 and xv.data_ptr() % 16 == 0 and torch.equal(xv, x)
    for fn in (lambda a: F.activation(a, F.ACT_RELU), lambda a: F.instance_norm_act(a, 1e-5, F.ACT_LRELU, 0.01),
               lambda a: F.max_pool3d_2x(a), lambda a: F.upsample_nearest_2x(a)):
        o, g = _run_views(fn, x)
        assert o[0].dtype == dtype and g is not None and g.dtype == dtype


# ----------------------------------------------------------------------------- A5: determinism, workspace reuse
def test_reductions_are_deterministic_and_the_workspace_carries_nothing_over(seg):
    """Every reduction called twice is bit-identical (fixed-order partials, no atomics), and bce_with_logits -> dice_sums ->
    cross_entropy_3d -> dice_rows -> znormalize -> bce_with_logits on one stream gives the first value again: the shared
    workspace() buffer is written before it is read by each of them, at a size (past the grid cap) where all 2,048 partials
    are in use and at a small one right after it (whose few partials lie in what the large call left behind)."""
    F = seg.functional
    big, small = (2, 2, 97, 101, 113), (3, 4, 3, 5, 7)
    data = {}
    for shape in (big, small):
        x, lab, onehot, soft = _case(shape, seed=3)
        data[shape] = (x.cuda(), lab.cuda(), onehot.cuda(), soft.cuda())

    def calls(shape):
        x, lab, onehot, soft = data[shape]
        n = x.shape[0]
        return [
            ("bce", lambda: F.bce_with_logits(x, soft)),
            ("dice_sums", lambda: F.dice_sums(x, onehot, True)),
            ("ce3d", lambda: F.cross_entropy_3d(x, lab)),
            ("dice_rows", lambda: F.dice_rows_autograd(x.view(n, -1), soft.view(n, -1), True, 2.0)),
            ("znorm", lambda: F.znormalize(x)),
            ("fused", lambda: torch.cat([v.reshape(-1).double() for v in F.bce_argmax_dice(x, onehot)])),
            ("counts", lambda: F.dice_counts(lab, F.argmax_channels(x).view(lab.shape))),
        ]
    first = {}
    for shape in (big, small):
        for name, fn in calls(shape):
            a, b = fn().clone(), fn().clone()
            assert torch.equal(a, b), f"{name} {shape}: two calls differ"
            first[(shape, name)] = a
    for shape in (big, small):                                   # interleaved: every call after every other, sizes alternating
        other = small if shape == big else big
        for name, fn in calls(shape):
            for oname, ofn in calls(other):
                ofn()
                assert torch.equal(fn(), first[(shape, name)]), f"{name} {shape} after {oname} {other}"


# ----------------------------------------------------------------------------- A6: the sizes the benchmark times
def test_full_size_cfg4_cross_entropy_plus_dice(seg):
    """cfg 4's criterion as bench.py times it: cross_entropy_3D(pred, lab) + DiceLoss()(pred, onehot) on [1, 4, 160, 192, 160]
    (78.6 M logits, 4.9 M voxels: 19 trips of the capped grid), loss and the whole pred.grad against fp64."""
    LF = _lf()
    shape = (1, 4, 160, 192, 160)
    x = _randn(shape, 211, 3.0)
    lab = _labels((1, 160, 192, 160), 4, 223)
    onehot = _onehot(lab, 4)
    res = {}
    for dt in (F64, F32):
        parts = {}

        def crit(z, dt_, parts=parts):
            parts["ce"], parts["dice"] = OL.cross_entropy_3d(z, lab), OL.dice_loss(z, onehot.to(dt_))
            return parts["ce"] + parts["dice"]
        v, g = _cpu(crit, x, dt, 1.0)
        res[dt] = (v, g, parts["ce"].detach(), parts["dice"].detach())
    xg, lg, og = x.cuda().requires_grad_(True), lab.cuda(), onehot.cuda()
    ce, dice = LF.cross_entropy_3D(xg, lg), LF.DiceLoss()(xg, og)
    loss = ce + dice
    loss.backward()
    _grade("full cfg4 cross_entropy_3D loss", ce, res[F64][2], res[F32][2], _loss_bound(res[F64][2]))
    _grade("full cfg4 DiceLoss loss", dice, res[F64][3], res[F32][3], _loss_bound(res[F64][3]))
    _grade("full cfg4 CE+Dice loss", loss, res[F64][0], res[F32][0], _loss_bound(res[F64][0]))
    _grade_full_size_grad("full cfg4 CE+Dice grad", xg.grad, res[F64][1], res[F32][1], LIB_GRAD)


def test_full_size_cfg4_dice_lossss_softmax(seg):
    """DiceLossss(4)(pred, lab, softmax=True) on [1, 4, 160, 192, 160]: softmax_channels + dice_rows over four rows of 4.9 M
    (float4 path, 2,048 / 4 blocks per row) and their backward kernels against fp64."""
    LF = _lf()
    shape = (1, 4, 160, 192, 160)
    x = _randn(shape, 227, 3.0)
    lab = _labels((1, 160, 192, 160), 4, 229)
    v64, g64 = _cpu(lambda z, dt: OL.dice_loss_multiclass(z, lab, 4, softmax=True), x, F64, 1.0)
    v32, g32 = _cpu(lambda z, dt: OL.dice_loss_multiclass(z, lab, 4, softmax=True), x, F32, 1.0)
    vd, gd = _dev(lambda z: LF.DiceLossss(4)(z, lab.cuda(), softmax=True), x, 1.0)
    _grade("full cfg4 DiceLossss loss", vd, v64, v32, _loss_bound(v64))
    _grade_full_size_grad("full cfg4 DiceLossss grad", gd, g64, g32, LIB_GRAD)


def test_full_size_cfg2_cfg3_bce_argmax_dice(seg):
    """The fused tail of the default step at cfg 2 / 3's [2, 2, 128, 128, 128]: loss and gradient against fp64, the mask equal to
    torch.argmax, the four counters exact."""
    F = seg.functional
    shape = (2, 2, 128, 128, 128)
    x = _randn(shape, 233, 3.0)
    lab = (_randn((2, 128, 128, 128), 239) > 0.8).long()
    tgt = _onehot(lab, 2)
    out = {}

    def fused(z):
        loss, out["mask"], out["counts"] = F.bce_argmax_dice(z, tgt.cuda())
        return loss
    bce = lambda z, dt: TF.binary_cross_entropy_with_logits(z, tgt.to(dt))
    v64, g64 = _cpu(bce, x, F64, 1.0)
    v32, g32 = _cpu(bce, x, F32, 1.0)
    vd, gd = _dev(fused, x, 1.0)
    _grade("full cfg2/3 bce_argmax_dice loss", vd, v64, v32, _loss_bound(v64))
    _grade_full_size_grad("full cfg2/3 bce_argmax_dice grad", gd, g64, g32, BCE_GRAD)
    mask_r = x.argmax(1, keepdim=True)
    assert torch.equal(out["mask"].cpu(), mask_r)
    assert out["counts"].cpu().tolist() == _counts_ref(lab.unsqueeze(1), mask_r)
