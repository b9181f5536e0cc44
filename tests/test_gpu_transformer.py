"""The token-encoder kernels of csrc/transformer.hip (LayerNorm forward / backward with and without the pass-through addend, the row
softmax with and without the attention-dropout factor, attention on separate and on fused [B, P, 3E] operands, the seating of the
QKV parameters, one whole TransformerBlock at E 768 / P 216 / FFN 2048) against the same operation in plain torch on the CPU in
FLOAT64, on the same seeded fp32 inputs, through the public Python surface (functional.*, layers.*, models.three_d.unetr.*); the C ABI
is called directly only where a refusal must be shown to write nothing.  ATen-CPU in fp32 on the same inputs is a second witness:
every graded quantity prints ``[transformer] tag: kernel error / ATen-fp32 error / bound`` (``pytest -rA``).

Bounds
  * fp32 outputs at unit scale: 1e-5 * max(1, max|ref|); fp32 gradients: 2e-5 * max(1, max|ref|); dgamma / dbeta: 1e-4 * max(1, max|ref|);
  * softmax probabilities, forward and backward: 1e-6 absolute; claims of bitwise equality are equality;
  * LayerNorm on offset / tiny-variance rows: the fp32 INPUT already limits the result (the error grows like eps32 * |mean| / sigma), so the
    bound there is max(the plain bound, 4 x ATen-fp32's own error against fp64 on the same input), computed in the test and printed; the 4
    covers another summation order in an otherwise identical two-pass formula.  dbeta does not depend on x and keeps the plain bound;
  * inside autocast(bfloat16) the GEMM operands are rounded to bf16 in registers and the products accumulated in fp32.  A bound of the
    fp32-accumulation kind does not hold there (an fp32-level difference in the scores flips bf16 roundings of the probabilities), so the
    result is held from two sides: (i) its distance from the fp64 chain with the operands rounded at the same points (q, k, v; pd; dO; dS;
    every Linear operand) is at most 4 x the distance of the same rounded chain run in fp32 on the CPU, and (ii) its distance from the
    UN-rounded fp64 chain is at most 2 x the rounded fp64 chain's -- the kernel may not be further from the truth than bf16 operands
    make unavoidable.  All four numbers are printed.  Both sides have the quantity's fp32 bound as a floor (see _grade_lowp).

DESIGN.md section 4.10 lists what this file changed in the code."""
import copy
import math

import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
SOFTMAX_TOL = 1e-6


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mi355seg
    mi355seg.lib()          # raises if the HIP library is missing -- no fallback
    return mi355seg


# ----------------------------------------------------------------------------- helpers
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed, scale=1.0, offset=0.0):
    return torch.randn(shape, generator=_gen(seed)) * scale + offset


def _maxabs(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _out_bound(ref):
    return 1e-5 * max(1.0, _maxabs(ref))


def _grad_bound(ref):
    return 2e-5 * max(1.0, _maxabs(ref))


def _affine_bound(ref):
    return 1e-4 * max(1.0, _maxabs(ref))


def _grade(tag, got, ref, aten, bound):
    """|got - ref| <= bound (max norm), with ATen-CPU fp32's own distance from the fp64 reference printed beside it."""
    got, ref, aten = [torch.as_tensor(v).detach().cpu().to(F64) for v in (got, ref, aten)]
    assert got.shape == ref.shape, f"{tag}: shape {tuple(got.shape)} vs reference {tuple(ref.shape)}"
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(aten).all()), f"{tag}: the CPU references must be finite"
    ek, ea = _maxabs(got - ref), _maxabs(aten - ref)
    print(f"[transformer] {tag}: kernel error {ek:.3e}  ATen-fp32 error {ea:.3e}  bound {bound:.3e}  (max|ref| {_maxabs(ref):.3e})")
    assert bool(torch.isfinite(got).all()), f"{tag}: kernel result is not finite"
    assert ek <= bound, f"{tag}: kernel error {ek:.3e} > bound {bound:.3e} (ATen fp32: {ea:.3e})"
    return ek, ea


def _grade_conditioned(tag, got, ref, aten, plain):
    """The LayerNorm bound on rows whose fp32 input limits the result: max(plain, 4 x ATen-fp32's own error)."""
    ea = _maxabs(aten.detach().cpu().to(F64) - ref.detach().cpu().to(F64))
    return _grade(tag, got, ref, aten, max(plain, 4.0 * ea))


def _grade_lowp(tag, got, r64, r32, u64, plain):
    """The two-sided bf16 scheme of the module docstring.  ``plain``: the quantity's fp32 bound, the floor of both sides -- a quantity the bf16
    rounding does not touch (a bias gradient is a sum of the incoming gradient: the two fp64 chains agree to the last bit, and 2 x 0 is no
    bound for fp32 arithmetic) is graded as it is in fp32."""
    got, r64, r32, u64 = [t.detach().cpu().to(F64) for t in (got, r64, r32, u64)]
    assert got.shape == r64.shape, f"{tag}: shape {tuple(got.shape)} vs reference {tuple(r64.shape)}"
    assert all(bool(torch.isfinite(t).all()) for t in (r64, r32, u64)), f"{tag}: the CPU references must be finite"
    e_kr, e_cr, e_ku, e_ru = _maxabs(got - r64), _maxabs(r32 - r64), _maxabs(got - u64), _maxabs(r64 - u64)
    print(f"[transformer] {tag}: kernel vs rounded-fp64 {e_kr:.3e}  rounded-fp32 vs rounded-fp64 {e_cr:.3e} (x4 = bound)  "
          f"kernel vs fp64 {e_ku:.3e}  rounded-fp64 vs fp64 {e_ru:.3e} (x2 = bound)  (max|ref| {_maxabs(u64):.3e})")
    assert bool(torch.isfinite(got).all()), f"{tag}: kernel result is not finite"
    assert e_kr <= max(4.0 * e_cr, plain), f"{tag}: (i) {e_kr:.3e} from the rounded fp64 chain > 4 x {e_cr:.3e} (fp32 floor {plain:.1e})"
    assert e_ku <= max(2.0 * e_ru, plain), f"{tag}: (ii) {e_ku:.3e} from the fp64 chain > 2 x {e_ru:.3e} (fp32 floor {plain:.1e})"


def _offset_view(t, floats=1):
    """The values of ``t`` (CPU) on the device as a CONTIGUOUS view that starts ``floats`` floats into a larger buffer: 4-byte aligned only."""
    buf = torch.empty(t.numel() + floats, dtype=F32, device="cuda")
    v = buf[floats:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * floats % 16
    return v


def _raises(seg, fn, *needles):
    with pytest.raises(seg.Mi355SegError) as e:
        fn()
        torch.cuda.synchronize()
    for n in needles:
        assert n in str(e.value), f"{n!r} not in {e.value}"


# ============================================================================= A. LayerNorm
def _ln_cpu(x, g, b, dy, eps, dt, addend=None):
    """y, dx, dgamma, dbeta of LayerNorm over the last dimension in dtype dt (ATen on the CPU)"""
    xr, gr, br = [t.detach().to(dt).clone().requires_grad_(True) for t in (x, g, b)]
    y = TF.layer_norm(xr, (x.shape[-1],), gr, br, eps)
    y.backward(dy.to(dt))
    dx = xr.grad if addend is None else xr.grad + addend.to(dt)
    return y.detach(), dx, gr.grad, br.grad


def _ln_dev(seg, x, g, b, dy, eps, addend=None, fork=False, module=False):
    F = seg.functional
    xg = x.cuda().requires_grad_(True) if not x.is_cuda else x.detach().requires_grad_(True)
    gg, bg = g.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    if module:
        from mi355seg.layers import LayerNorm
        ln = LayerNorm(x.shape[-1], eps=eps).cuda()
        with torch.no_grad():
            ln.weight.copy_(gg)
            ln.bias.copy_(bg)
        gg, bg = ln.weight, ln.bias
        y = ln(xg)
        y.backward(dy.cuda())
    elif fork:
        y, xp = F.layer_norm_fork(xg, gg, bg, eps)
        assert xp.shape == xg.shape and torch.equal(xp, xg)
        torch.autograd.backward([y, xp], [dy.cuda(), addend if addend.is_cuda else addend.cuda()])
    else:
        y = F.layer_norm(xg, gg, bg, eps)
        y.backward(dy.cuda())
    assert y.dtype == F32 and y.shape == x.shape and xg.grad.shape == x.shape
    return y.detach().cpu(), xg.grad.cpu(), gg.grad.cpu(), bg.grad.cpu()


def _ln_check(tag, dev, r64, r32, conditioned=False):
    grade = _grade_conditioned if conditioned else (lambda t, a, b, c, bound: _grade(t, a, b, c, bound))
    grade(tag + " y", dev[0], r64[0], r32[0], _out_bound(r64[0]))
    grade(tag + " dx", dev[1], r64[1], r32[1], _grad_bound(r64[1]))
    grade(tag + " dgamma", dev[2], r64[2], r32[2], _affine_bound(r64[2]))
    _grade(tag + " dbeta", dev[3], r64[3], r32[3], _affine_bound(r64[3]))


def _ln_inputs(rows, E, seed, offset=0.5, sigma=2.0):
    x = _randn((rows, E), seed, sigma, offset)
    if E == 2:
        # two values per row: sigma = |a - b| / 2, and a row with a ~ b is the ill-conditioned case graded elsewhere.  Keep |a - b| >= 1, so
        # that eps32 * |mean| / sigma stays below 1e-6 and the plain bounds are the right ones for this sweep.
        x[:, 1] = x[:, 0] + (1.0 + _randn((rows,), seed + 7).abs()) * torch.where(_randn((rows,), seed + 8) > 0, 1.0, -1.0)
    g = _randn((E,), seed + 1, 0.5, 1.0)
    b = _randn((E,), seed + 2, 0.3)
    dy = _randn((rows, E), seed + 3)
    return x, g, b, dy


# every E with at least two row counts; every row count at least once; rows % 4 in {0, 1, 2, 3}
LN_SWEEP = [(1, 1), (5, 1), (1001, 1), (3, 2), (216, 2), (4, 63), (1001, 63), (5, 64), (432, 64), (1, 65), (1001, 65), (3, 96), (216, 96),
            (1, 768), (216, 768), (432, 768), (4, 2047), (5, 2047), (1, 2048), (3, 2048), (216, 2048)]


@pytest.mark.parametrize("rows,E", LN_SWEEP)
def test_layer_norm_shape_sweep(seg, rows, E):
    """y, dx, dgamma, dbeta of layer_norm and of layer_norm_fork (dx = pass-through + LayerNorm backward) at every (rows, E) edge: a wavefront
    per row and four rows per workgroup (rows % 4), 64 lanes x up to 32 columns per lane (E around 64 and at the 2,048 limit), E = 1 (var = 0)."""
    x, g, b, dy = _ln_inputs(rows, E, 100 + rows + E)
    for eps in (1e-6, 1e-5):
        r64, r32 = _ln_cpu(x, g, b, dy, eps, F64), _ln_cpu(x, g, b, dy, eps, F32)
        _ln_check(f"layer_norm {rows}x{E} eps {eps:g}", _ln_dev(seg, x, g, b, dy, eps), r64, r32)
    add = _randn((rows, E), 5 + rows)
    r64, r32 = _ln_cpu(x, g, b, dy, 1e-6, F64, add), _ln_cpu(x, g, b, dy, 1e-6, F32, add)
    _ln_check(f"layer_norm_fork {rows}x{E}", _ln_dev(seg, x, g, b, dy, 1e-6, add, fork=True), r64, r32)


@pytest.mark.parametrize("shape", [(2, 216, 768), (2, 3, 5, 96), (3, 7, 65)])
def test_layer_norm_nd_and_non_contiguous(seg, shape):
    """3-D / 4-D inputs through layers.LayerNorm, and non-contiguous x / dy / pass-through gradient through the functional forms."""
    E = shape[-1]
    x, g, b, dy = _ln_inputs(math.prod(shape[:-1]), E, 300 + E)
    x, dy = x.view(shape), dy.view(shape)
    r64, r32 = _ln_cpu(x, g, b, dy, 1e-6, F64), _ln_cpu(x, g, b, dy, 1e-6, F32)
    _ln_check(f"layers.LayerNorm {shape}", _ln_dev(seg, x, g, b, dy, 1e-6, module=True), r64, r32)
    # the same numbers as views of wider / transposed buffers: a column slice (row pitch 2E), and dy / the addend as transposes
    wide = torch.zeros(shape[:-1] + (2 * E,), device="cuda")
    wide[..., :E] = x.cuda()
    xv = wide[..., :E]
    dyv = dy.cuda().transpose(0, 1).contiguous().transpose(0, 1)
    assert not xv.is_contiguous() and not dyv.is_contiguous()
    _ln_check(f"layer_norm {shape} strided", _ln_dev(seg, xv, g, b, dyv, 1e-6), r64, r32)
    add = _randn(shape, 17)
    addv = add.cuda().transpose(0, 1).contiguous().transpose(0, 1)
    r64, r32 = _ln_cpu(x, g, b, dy, 1e-6, F64, add), _ln_cpu(x, g, b, dy, 1e-6, F32, add)
    _ln_check(f"layer_norm_fork {shape} strided", _ln_dev(seg, xv, g, b, dyv, 1e-6, addv, fork=True), r64, r32)


LN_VALUES = [(0.5, 2.0), (1e4, 1.0), (0.0, 1e-4), (1e3, 1e-3), (-3e4, 10.0)]


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
@pytest.mark.parametrize("case", list(range(len(LN_VALUES))) + ["mixed", "gamma", "dy0"])
def test_layer_norm_value_cases(seg, case, eps):
    """432 x 768 (cfg 5 at batch 2) with rows N(offset, sigma^2) far from centred / unit variance, rows that mix these, gamma with zeros and
    negative entries, dy = 0.  Bound: max(plain, 4 x ATen-fp32's own error), see the module docstring."""
    rows, E = 432, 768
    x, g, b, dy = _ln_inputs(rows, E, 500)
    if isinstance(case, int):
        off, sig = LN_VALUES[case]
        x = _randn((rows, E), 501 + case, sig, off)
    elif case == "mixed":
        for i, (off, sig) in enumerate(LN_VALUES):
            x[i::5] = _randn((len(range(i, rows, 5)), E), 520 + i, sig, off)
    elif case == "gamma":
        g[::3] = 0.0
        g[1::3] = -g[1::3].abs()
    else:
        dy = torch.zeros_like(dy)
    r64, r32 = _ln_cpu(x, g, b, dy, eps, F64), _ln_cpu(x, g, b, dy, eps, F32)
    dev = _ln_dev(seg, x, g, b, dy, eps)
    _ln_check(f"layer_norm values {case} eps {eps:g}", dev, r64, r32, conditioned=True)
    if case == "dy0":
        assert not dev[1].any() and not dev[2].any() and not dev[3].any()
    add = _randn((rows, E), 540)
    r64, r32 = _ln_cpu(x, g, b, dy, eps, F64, add), _ln_cpu(x, g, b, dy, eps, F32, add)
    _ln_check(f"layer_norm_fork values {case} eps {eps:g}", _ln_dev(seg, x, g, b, dy, eps, add, fork=True), r64, r32, conditioned=True)


def test_layer_norm_constant_rows(seg):
    """var = 0: y is beta exactly, the saved mean is the constant, dx is finite and dgamma gets nothing from those rows.  dx is not graded there:
    rstd = eps^-1/2 makes it ill-conditioned in any precision.  The constants have short mantissas, so their 768-term sums are exact."""
    F = seg.functional
    rows, E = 433, 768
    x, g, b, dy = _ln_inputs(rows, E, 600)
    const = {0: 3.25, 7: -1024.0, 100: 0.0, rows - 1: 0.5}
    for r, c in const.items():
        x[r] = c
    idx = torch.tensor(sorted(const))
    rest = torch.tensor([r for r in range(rows) if r not in const])
    xg, gg, bg = x.cuda().requires_grad_(True), g.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = F.layer_norm(xg, gg, bg, 1e-6)
    mean = y.grad_fn.saved_tensors[2].cpu()
    y.backward(dy.cuda())
    yc = y.detach().cpu()
    assert torch.equal(yc[idx], b.expand(len(idx), E)), "constant rows: y must be beta exactly"
    assert torch.equal(mean[idx], torch.tensor([const[int(r)] for r in idx])), "constant rows: the mean is the constant"
    assert bool(torch.isfinite(xg.grad).all())
    r64, r32 = _ln_cpu(x, g, b, dy, 1e-6, F64), _ln_cpu(x, g, b, dy, 1e-6, F32)
    _grade("layer_norm constant rows: y", yc, r64[0], r32[0], _out_bound(r64[0]))
    _grade("layer_norm constant rows: dx elsewhere", xg.grad.cpu()[rest], r64[1][rest], r32[1][rest], _grad_bound(r64[1][rest]))
    # the fp64 dgamma of the remaining rows alone: nothing may come from the constant ones
    only = _ln_cpu(x[rest], g, b, dy[rest], 1e-6, F64)
    _grade("layer_norm constant rows: dgamma", gg.grad, only[2], r32[2], _affine_bound(only[2]))
    _grade("layer_norm constant rows: dbeta", bg.grad, r64[3], r32[3], _affine_bound(r64[3]))


def test_layer_norm_fork_unused_outputs(seg):
    """Either output of layer_norm_fork unused: the norm unused -> dx is the pass-through gradient itself and gamma / beta get none;
    the pass-through unused -> the plain LayerNorm backward."""
    F = seg.functional
    x, g, b, dy = _ln_inputs(216, 768, 700)
    add = _randn((216, 768), 701)
    xg, gg, bg = x.cuda().requires_grad_(True), g.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    _, xp = F.layer_norm_fork(xg, gg, bg, 1e-6)
    xp.backward(add.cuda())
    assert torch.equal(xg.grad.cpu(), add) and gg.grad is None and bg.grad is None
    xg.grad = None
    n, _ = F.layer_norm_fork(xg, gg, bg, 1e-6)
    n.backward(dy.cuda())
    r64, r32 = _ln_cpu(x, g, b, dy, 1e-6, F64), _ln_cpu(x, g, b, dy, 1e-6, F32)
    _ln_check("layer_norm_fork, pass-through unused", (n.detach().cpu(), xg.grad.cpu(), gg.grad.cpu(), bg.grad.cpu()), r64, r32)
    plain = _ln_dev(seg, x, g, b, dy, 1e-6)
    assert all(torch.equal(a, c) for a, c in zip((n.detach().cpu(), xg.grad.cpu(), gg.grad.cpu(), bg.grad.cpu()), plain))


def test_layer_norm_refusals(seg):
    """E = 2049 is refused with the limit in the message and nothing written (the C entry point, on sentinel-filled outputs); gamma / beta of
    the wrong length, dtype or device are refused before any launch -- a shorter gamma would be read out of bounds."""
    F, L = seg.functional, seg.lib()
    x = torch.randn(8, 2049, device="cuda")
    g, b = torch.ones(2049, device="cuda"), torch.zeros(2049, device="cuda")
    _raises(seg, lambda: F.layer_norm(x, g, b, 1e-6), "2048")
    _raises(seg, lambda: F.layer_norm_fork(x, g, b, 1e-6), "2048")
    y, mean, rstd = torch.full_like(x, -7.0), torch.full((8,), -7.0, device="cuda"), torch.full((8,), -7.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _raises(seg, lambda: L.call("mi355seg_layernorm_fwd_f32", x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                8, 2049, 1e-6, st), "2048")
    dx, dg, db = torch.full_like(x, -7.0), torch.full((2049,), -7.0, device="cuda"), torch.full((2049,), -7.0, device="cuda")
    for name, extra in (("mi355seg_layernorm_bwd_f32", ()), ("mi355seg_layernorm_bwd_add_f32", (x.data_ptr(),))):
        _raises(seg, lambda: L.call(name, x.data_ptr(), x.data_ptr(), g.data_ptr(), mean.data_ptr(), rstd.data_ptr(), *extra,
                                    dx.data_ptr(), dg.data_ptr(), db.data_ptr(), 8, 2049, st))
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in (y, mean, rstd, dx, dg, db)), "a refused call wrote to its outputs"
    x = torch.randn(8, 96, device="cuda")
    good = torch.ones(96, device="cuda")
    bad = {"short": torch.ones(95, device="cuda"), "long": torch.ones(97, device="cuda"), "double": torch.ones(96, device="cuda", dtype=F64),
           "bf16": torch.ones(96, device="cuda", dtype=BF16), "cpu": torch.ones(96), "strided": torch.ones(192, device="cuda")[::2]}
    for fn in (F.layer_norm, lambda *a: F.layer_norm_fork(*a)[0]):
        for what, t in bad.items():
            _raises(seg, lambda: fn(x, t, good, 1e-6))
            _raises(seg, lambda: fn(x, good, t, 1e-6))
        assert bool(torch.isfinite(fn(x, good, good, 1e-6)).all())


@pytest.mark.parametrize("rows,E", [(432, 768), (1001, 65), (5, 2047)])
def test_layer_norm_is_deterministic(seg, rows, E):
    """Two calls are bitwise equal: the dgamma / dbeta reduction adds its eight row groups in a fixed order."""
    x, g, b, dy = _ln_inputs(rows, E, 800)
    add = _randn((rows, E), 801)
    for fork in (False, True):
        a, c = [_ln_dev(seg, x, g, b, dy, 1e-6, add, fork=fork) for _ in range(2)]
        assert all(torch.equal(p, q) for p, q in zip(a, c))


# ============================================================================= B. row softmax
def _softmax_ref(x, keep, dyk, dt):
    """y = softmax(x), yk = y * keep, and d(x) for an incoming gradient of yk, written out in dtype dt"""
    y = torch.softmax(x.to(dt), dim=-1)
    k = torch.ones_like(y) if keep is None else keep.to(dt)
    dy = dyk.to(dt) * k
    return y, y * k, y * (dy - (y * dy).sum(-1, keepdim=True))


def _softmax_dev(seg, x, keep, dyk):
    """softmax_last (keep None, through autograd) or the _softmax_keep / _softmax_keep_bwd pair attention runs"""
    F = seg.functional
    rows, L = x.shape
    if keep is None:
        xg = x.cuda().requires_grad_(True)
        y = F.softmax_last(xg)
        y.backward(dyk.cuda())
        # and the keep-less branch of the pair (what attention runs without dropout): the same kernels, so the same bits
        p, pd = F._softmax_keep(x.cuda(), None, rows, L)
        assert pd is p and torch.equal(p, y) and torch.equal(F._softmax_keep_bwd(p, dyk.cuda(), None, rows, L), xg.grad)
        return y.detach().cpu(), y.detach().cpu(), xg.grad.cpu()
    kd = keep.cuda()
    p, pd = F._softmax_keep(x.cuda(), kd, rows, L)
    ds = F._softmax_keep_bwd(p, dyk.cuda(), kd, rows, L)
    return p.cpu(), pd.cpu(), ds.cpu()


def _softmax_check(seg, tag, x, keep, dyk, exact_ref=True):
    y, yk, dx = _softmax_dev(seg, x, keep, dyk)
    r64, r32 = _softmax_ref(x, keep, dyk, F64), _softmax_ref(x, keep, dyk, F32)
    _grade(tag + " y", y, r64[0], r32[0], SOFTMAX_TOL)
    _grade(tag + " y*keep", yk, r64[1], r32[1], SOFTMAX_TOL * max(1.0, _maxabs(keep) if keep is not None else 1.0))
    _grade(tag + " dx", dx, r64[2], r32[2], SOFTMAX_TOL)
    sums = y.double().sum(-1)
    assert _maxabs(sums - 1.0) <= SOFTMAX_TOL, f"{tag}: row sums off by {_maxabs(sums - 1.0):.3e}"
    if keep is not None:
        assert not yk[keep == 0].any(), f"{tag}: y * keep must be exactly 0 where keep is 0"
    return y, yk, dx


def _keep(shape, seed, p=0.9):
    return (torch.rand(shape, generator=_gen(seed)) < p).float() / p


SOFTMAX_L = [1, 2, 63, 64, 65, 216, 1000, 2048]
SOFTMAX_ROWS = [1, 5, 2 * 12 * 216]


@pytest.mark.parametrize("L", SOFTMAX_L)
@pytest.mark.parametrize("rows", SOFTMAX_ROWS)
def test_softmax_rows_sweep(seg, rows, L):
    """Forward and backward at every L edge (64 lanes x up to 32 columns) and row count (rows % 4, the cfg 5 count), logits at scales 1, 30
    and 100 -- far past where expf overflows without the max subtraction --, without a mask and with Bernoulli(0.9) / 0.9.  The incoming
    gradient is uniform in [-1, 1): the 1e-6 bound is absolute, and dx = y (dy - y.dy) carries the scale of dy."""
    for scale in (1.0, 30.0, 100.0):
        x = _randn((rows, L), 1000 + L + rows, scale)
        dyk = torch.rand((rows, L), generator=_gen(1001 + L)) * 2 - 1
        _softmax_check(seg, f"softmax {rows}x{L} scale {scale:g}", x, None, dyk)
        _softmax_check(seg, f"softmax_keep {rows}x{L} scale {scale:g}", x, _keep((rows, L), 1002 + L), dyk)


@pytest.mark.parametrize("rows,L", [(5, 65), (5184, 216), (5, 2048), (1, 2)])
def test_softmax_rows_value_edges(seg, rows, L):
    """-inf entries (probability exactly 0, the rest sums to 1), rows of equal values (uniform), a unique maximum 200 above the rest
    (exactly 1.0 and exactly 0: exp(-200) is below the smallest fp32 denormal)."""
    dyk = torch.rand((rows, L), generator=_gen(1100)) * 2 - 1
    for keep in (None, _keep((rows, L), 1101)):
        kt = "" if keep is None else "_keep"
        x = _randn((rows, L), 1102, 3.0)
        hole = torch.rand((rows, L), generator=_gen(1103)) < 0.3
        hole[:, 0] = False                                          # never a whole row
        x[hole] = -math.inf
        y, _, dx = _softmax_check(seg, f"softmax{kt} {rows}x{L} -inf entries", x, keep, dyk)
        assert not y[hole].any() and not dx[hole].any(), "-inf logits: probability and gradient exactly 0"
        x = _randn((rows, 1), 1104, 50.0).expand(rows, L).contiguous()
        y, _, _ = _softmax_check(seg, f"softmax{kt} {rows}x{L} equal values", x, keep, dyk)
        assert _maxabs(y.double() - 1.0 / L) <= SOFTMAX_TOL
        x = _randn((rows, L), 1105)
        top = torch.randint(0, L, (rows,), generator=_gen(1106))
        x[torch.arange(rows), top] = x.max() + 200.0
        y, _, _ = _softmax_check(seg, f"softmax{kt} {rows}x{L} unique maximum", x, keep, dyk)
        want = torch.zeros(rows, L)
        want[torch.arange(rows), top] = 1.0
        assert torch.equal(y, want), "a maximum 200 above the rest: exactly 1.0 there and exactly 0 elsewhere"


@pytest.mark.parametrize("rows,L", [(5, 65), (5184, 216), (3, 2048)])
def test_softmax_keep_masks(seg, rows, L):
    """keep of all ones (the pair equals the plain kernels bitwise), all zeros (yk and the score gradient exactly 0), and rows that are
    wholly or partly zero (the gradient at a dropped position is -y . dot, graded against fp64 like the rest)."""
    F = seg.functional
    x = _randn((rows, L), 1200, 2.0)
    dyk = torch.rand((rows, L), generator=_gen(1201)) * 2 - 1
    plain = _softmax_dev(seg, x, None, dyk)
    ones = _softmax_check(seg, f"softmax_keep {rows}x{L} keep = 1", x, torch.ones(rows, L), dyk)
    assert all(torch.equal(a, c) for a, c in zip(plain, ones))
    y, yk, dx = _softmax_check(seg, f"softmax_keep {rows}x{L} keep = 0", x, torch.zeros(rows, L), dyk)
    assert torch.equal(y, plain[0]) and not yk.any() and not dx.any()
    keep = _keep((rows, L), 1202)
    keep[0] = 0.0                                                   # a row of zeros
    keep[rows - 1, ::2] = 0.0                                       # a half-zero row
    y, yk, dx = _softmax_check(seg, f"softmax_keep {rows}x{L} zero rows", x, keep, dyk)
    assert not dx[0].any()
    with pytest.raises(seg.Mi355SegError):
        F._softmax_keep(x.cuda(), torch.ones(rows, L + 1, device="cuda"), rows, L)


def test_softmax_refuses_long_rows(seg):
    F = seg.functional
    x = torch.randn(4, 2049, device="cuda")
    _raises(seg, lambda: F.softmax_last(x), "2048")
    _raises(seg, lambda: F._softmax_keep(x, None, 4, 2049), "2048")
    _raises(seg, lambda: F._softmax_keep(x, torch.ones_like(x), 4, 2049), "2048")


# ============================================================================= C. attention
def _attn_chain(q, k, v, keep, do, heads, dt, rounded):
    """softmax(Q K^T / sqrt(d)) * keep @ V per (batch, head) and its backward written out as products in dtype dt.  ``rounded``: every GEMM
    operand (q, k, v; pd; dO; dS) is rounded to bf16 first, as the kernels do in registers inside autocast(bfloat16)."""
    r = (lambda t: t.to(BF16).to(dt)) if rounded else (lambda t: t)
    B, P, E = q.shape
    d = E // heads
    alpha = 1.0 / (d ** 0.5)
    split = lambda t: t.to(dt).view(B, P, heads, d).permute(0, 2, 1, 3)
    merge = lambda t: t.permute(0, 2, 1, 3).reshape(B, P, E)
    Q, K, V, DO = r(split(q)), r(split(k)), r(split(v)), r(split(do))
    p = torch.softmax((Q @ K.transpose(-1, -2)) * alpha, dim=-1)
    kp = None if keep is None else keep.to(dt)
    pd = r(p if kp is None else p * kp)
    out = pd @ V
    dpd = DO @ V.transpose(-1, -2)
    dV = pd.transpose(-1, -2) @ DO
    dp = dpd if kp is None else dpd * kp
    ds = r(p * (dp - (p * dp).sum(-1, keepdim=True)))
    dQ = (ds @ K) * alpha
    dK = (ds.transpose(-1, -2) @ Q) * alpha
    return merge(out), merge(dQ), merge(dK), merge(dV)


def _attn_dev(seg, fused, q, k, v, keep, do, heads, lowp, offset=False):
    """(out, dq, dk, dv) on the device; ``fused``: attention_qkv on the concatenation.  ``offset``: every operand and the incoming gradient
    are contiguous views that start one float into a larger buffer (4-byte aligned)."""
    F = seg.functional
    E = q.shape[-1]
    put = _offset_view if offset else (lambda t: t.cuda())
    kd = None if keep is None else keep.cuda()
    ctx = F.autocast(BF16 if lowp else F32)
    if fused:
        base = put(torch.cat([q, k, v], dim=-1))
        leaf = base.detach().requires_grad_(True)
        with ctx:
            out = F.attention_qkv(leaf, heads, kd)
        torch.autograd.backward([out], [put(do)])
        g = leaf.grad
        res = out, g[..., :E], g[..., E:2 * E], g[..., 2 * E:]
    else:
        leaves = [put(t).detach().requires_grad_(True) for t in (q, k, v)]
        with ctx:
            out = F.attention(*leaves, heads, kd)
        torch.autograd.backward([out], [put(do)])
        res = (out,) + tuple(t.grad for t in leaves)
    torch.cuda.synchronize()
    assert all(t.dtype == F32 for t in res)
    return tuple(t.detach().cpu().contiguous() for t in res)


def _attn_inputs(B, P, heads, d, masked, seed):
    E = heads * d
    q, k, v, do = (_randn((B, P, E), seed + i) for i in range(4))
    keep = _keep((B, heads, P, P), seed + 4) if masked else None
    return q, k, v, keep, do


def _attn_grade(tag, got, lowp, q, k, v, keep, do, heads, batches=None):
    if batches is not None:                                         # grade these batches only (the device ran all of them)
        got = tuple(t[batches] for t in got)
        q, k, v, do = (t[batches] for t in (q, k, v, do))
        keep = None if keep is None else keep[batches]
    names = ("out", "dq", "dk", "dv")
    u64 = _attn_chain(q, k, v, keep, do, heads, F64, False)
    if not lowp:
        u32 = _attn_chain(q, k, v, keep, do, heads, F32, False)
        for n, a, r, t in zip(names, got, u64, u32):
            _grade(f"{tag} {n}", a, r, t, _out_bound(r) if n == "out" else _grad_bound(r))
    else:
        r64, r32 = _attn_chain(q, k, v, keep, do, heads, F64, True), _attn_chain(q, k, v, keep, do, heads, F32, True)
        for n, a, r, t, u in zip(names, got, r64, r32, u64):
            _grade_lowp(f"{tag} {n}", a, r, t, u, _out_bound(u) if n == "out" else _grad_bound(u))


ATTN_SHAPES = [(1, 216, 12, 64), (2, 216, 12, 64), (2, 8, 4, 24), (2, 50, 4, 24), (1, 27, 12, 64), (3, 64, 2, 8), (8, 216, 12, 64)]


@pytest.mark.parametrize("lowp", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("B,P,heads,d", ATTN_SHAPES)
def test_attention_against_fp64(seg, B, P, heads, d, masked, lowp):
    """attention (separate q, k, v) and attention_qkv (the fused [B, P, 3E] layout UNETR runs): output, dQ, dK, dV.  cfg 5 at batch 1 and 2, the
    model fixture's shape, P % 8 != 0 (no pair launch), the 48^3 patch count, a small-head shape, and batch 8 of cfg 5 (more than 4,096 32x32
    tiles: the single and the pair launch both leave the small-GEMM kernel; graded on batches 0 and 7 to keep the CPU chains short).  The two
    entry points run the same kernels in the same order -- only pitches differ -- and must agree bitwise."""
    q, k, v, keep, do = _attn_inputs(B, P, heads, d, masked, 2000 + B + P)
    sep = _attn_dev(seg, False, q, k, v, keep, do, heads, lowp)
    fus = _attn_dev(seg, True, q, k, v, keep, do, heads, lowp)
    tag = f"({B},{P},{heads},{d}) {'bf16' if lowp else 'fp32'} {'mask' if masked else 'nomask'}"
    batches = [0, 7] if B == 8 else None
    _attn_grade("attention " + tag, sep, lowp, q, k, v, keep, do, heads, batches)
    _attn_grade("attention_qkv " + tag, fus, lowp, q, k, v, keep, do, heads, batches)
    for n, a, c in zip(("out", "dq", "dk", "dv"), sep, fus):
        assert torch.equal(a, c), f"attention and attention_qkv differ in {n} by {_maxabs(a - c):.3e}"


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
def test_attention_pair_launch_is_bitwise_the_two_launches(seg, monkeypatch, masked):
    """MI355SEG_NO_GEMM_PAIRS=1 against the default at the cfg 5 shape, through the real autograd path and with real softmax output."""
    q, k, v, keep, do = _attn_inputs(2, 216, 12, 64, masked, 2100)
    monkeypatch.delenv("MI355SEG_NO_GEMM_PAIRS", raising=False)
    pair = _attn_dev(seg, True, q, k, v, keep, do, 12, True)
    monkeypatch.setenv("MI355SEG_NO_GEMM_PAIRS", "1")
    single = _attn_dev(seg, True, q, k, v, keep, do, 12, True)
    for n, a, c in zip(("out", "dq", "dk", "dv"), pair, single):
        assert torch.equal(a, c), f"pair launch and two launches differ in {n} by {_maxabs(a - c):.3e}"


@pytest.mark.parametrize("lowp", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("fused", [False, True], ids=["attention", "attention_qkv"])
@pytest.mark.parametrize("B,P,heads,d", [(2, 216, 12, 64), (2, 8, 4, 24)])
def test_attention_on_misaligned_views(seg, B, P, heads, d, fused, lowp):
    """qkv (or q, k, v) and the incoming gradient as contiguous views one float into a larger buffer -- what ``.contiguous()`` hands back
    unchanged.  Nothing may raise and the results meet the bounds of the aligned case.  (The pair launch of attention_qkv's backward, which
    needs 16-byte aligned operands, exists only inside autocast(bfloat16); fp32 is the control.)"""
    q, k, v, keep, do = _attn_inputs(B, P, heads, d, True, 2200 + P)
    got = _attn_dev(seg, fused, q, k, v, keep, do, heads, lowp, offset=True)
    _attn_grade(f"{'attention_qkv' if fused else 'attention'} misaligned ({B},{P},{heads},{d}) {'bf16' if lowp else 'fp32'}", got, lowp, q, k, v, keep, do, heads)


def test_attention_refusals(seg):
    """A head split that does not divide E, a fused width that is not a multiple of 3, a mask of the wrong shape and q / k / v of different
    shapes raise before any launch (E // heads would leave the last columns of the output unwritten)."""
    F = seg.functional
    t = lambda *s: torch.randn(*s, device="cuda")
    q = t(2, 8, 96)
    for lowp in (False, True):
        with F.autocast(BF16 if lowp else F32):
            _raises(seg, lambda: F.attention(q, q, q, 5))
            _raises(seg, lambda: F.attention(q, q, q, 0))
            _raises(seg, lambda: F.attention(q, t(2, 8, 48), q, 4))
            _raises(seg, lambda: F.attention(q, q, t(2, 7, 96), 4))
            _raises(seg, lambda: F.attention(q, t(1, 8, 96), q, 4))
            _raises(seg, lambda: F.attention(t(16, 96), t(16, 96), t(16, 96), 4))
            _raises(seg, lambda: F.attention(q, q, q, 4, t(2, 4, 8, 7)))
            _raises(seg, lambda: F.attention(q, q, q, 4, t(2, 8, 8)))
            _raises(seg, lambda: F.attention(q, q, q, 4, torch.ones(2, 4, 8, 8)))
            _raises(seg, lambda: F.attention_qkv(t(2, 8, 289), 4))
            _raises(seg, lambda: F.attention_qkv(t(2, 8, 3 * 98), 4))
            _raises(seg, lambda: F.attention_qkv(t(16, 288), 4))
            _raises(seg, lambda: F.attention_qkv(t(2, 8, 288), 4, t(2, 4, 8, 9)))
            assert bool(torch.isfinite(F.attention_qkv(t(2, 8, 288), 4, torch.ones(2, 4, 8, 8, device="cuda"))).all())


def test_linear_refusals(seg):
    """linear: a weight whose second dimension is not K, a bias that does not have N elements, parameters of another dtype or device."""
    F = seg.functional
    x, w, b = torch.randn(16, 96, device="cuda"), torch.randn(64, 96, device="cuda"), torch.randn(64, device="cuda")
    assert F.linear(x, w, b).shape == (16, 64)
    for lowp in (False, True):
        with F.autocast(BF16 if lowp else F32):
            _raises(seg, lambda: F.linear(x, torch.randn(64, 95, device="cuda"), b))
            _raises(seg, lambda: F.linear(x, torch.randn(64, 97, device="cuda"), b))
            _raises(seg, lambda: F.linear(x, torch.randn(64 * 96, device="cuda"), b))
            _raises(seg, lambda: F.linear(x, w, torch.randn(63, device="cuda")))
            _raises(seg, lambda: F.linear(x, w, torch.randn(65, device="cuda")))
            _raises(seg, lambda: F.linear(x, w.double(), b))
            _raises(seg, lambda: F.linear(x, w, b.cpu()))
            _raises(seg, lambda: F.linear(x, w.cpu(), b))


# ============================================================================= D. QKV seating
def _attn_module(seg, heads=4, E=96):
    from mi355seg.models.three_d.unetr import SelfAttention
    m = SelfAttention(heads, E, 0.1)
    with torch.no_grad():
        for i, (n, p) in enumerate(sorted(m.named_parameters())):
            p.copy_(_randn(tuple(p.shape), 3000 + i, 0.05 if p.dim() == 1 else p.shape[1] ** -0.5))
    return m.eval()


def _qkv_params(m):
    return (m.query.weight, m.key.weight, m.value.weight, m.query.bias, m.key.bias, m.value.bias)


def _attn_module_run(m, x, dy):
    """output and the gradients of the input and of all eight parameters"""
    for p in m.parameters():
        p.grad = None
    xg = x.detach().clone().requires_grad_(True)
    out, _ = m(xg)
    out.backward(dy)
    torch.cuda.synchronize()
    return {"out": out.detach().clone(), "dx": xg.grad.clone(), **{n: p.grad.clone() for n, p in m.named_parameters()}}


def test_qkv_seating_survives_moves_and_loads(seg):
    """After construction + .cuda(), after .cpu().cuda() and after load_state_dict of a reference-layout dict (separate query / key / value
    tensors) the six parameters are slices of one buffer, state_dict() has the reference's keys and shapes, and the values round-trip exactly."""
    from oracle.nets import _SelfAttention
    F = seg.functional
    ref = _SelfAttention(4, 96, 0.1)
    want_keys = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    m = _attn_module(seg)
    values = {k: v.clone() for k, v in m.state_dict().items()}

    def check(mod, vals, where):
        assert F.qkv_params_are_fused(*_qkv_params(mod)), f"{where}: the QKV parameters are not seated in one buffer"
        sd = mod.state_dict()
        assert {k: tuple(v.shape) for k, v in sd.items()} == want_keys, where
        for k, v in vals.items():
            assert torch.equal(sd[k].cpu(), v.cpu()), f"{where}: {k} changed"
        E, K = mod.query.weight.shape
        fw = torch.as_strided(mod.query.weight.detach(), (3 * E, K), (K, 1))
        assert torch.equal(fw, torch.cat([mod.query.weight, mod.key.weight, mod.value.weight]).detach())

    m.cuda()
    check(m, values, "after .cuda()")
    m.cpu()
    assert not F.qkv_params_are_fused(*_qkv_params(m))                     # (the fused form is a device layout)
    m.cuda()
    check(m, values, "after .cpu().cuda()")
    new = {k: _randn(tuple(v.shape), 3100 + i) for i, (k, v) in enumerate(ref.state_dict().items())}
    m.load_state_dict(new)
    check(m, new, "after load_state_dict")
    m2 = _attn_module(seg).cuda()
    m2.load_state_dict({k: v.cuda() for k, v in new.items()})
    x, dy = torch.randn(2, 8, 96, device="cuda"), torch.randn(2, 8, 96, device="cuda")
    a, c = _attn_module_run(m, x, dy), _attn_module_run(m2, x, dy)
    assert all(torch.equal(a[k], c[k]) for k in a)


def test_qkv_seating_keeps_an_earlier_optimizer(seg):
    """An optimizer built BEFORE .cuda() still updates the seated parameters: after one Adam step the fused buffer's rows are the three
    parameters, and they changed."""
    F = seg.functional
    m = _attn_module(seg).train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    m.cuda()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert F.qkv_params_are_fused(*_qkv_params(m))
    m.attn_dropout.forced_masks = [torch.ones(2, 4, 8, 8)]
    m.proj_dropout.forced_masks = [torch.ones(2, 8, 96)]
    out, _ = m(torch.randn(2, 8, 96, device="cuda"))
    out.square().sum().backward()
    opt.step()
    torch.cuda.synchronize()
    assert F.qkv_params_are_fused(*_qkv_params(m))
    E, K = m.query.weight.shape
    fw = torch.as_strided(m.query.weight.detach(), (3 * E, K), (K, 1))
    fb = torch.as_strided(m.query.bias.detach(), (3 * E,), (1,))
    assert torch.equal(fw, torch.cat([m.query.weight, m.key.weight, m.value.weight]).detach())
    assert torch.equal(fb, torch.cat([m.query.bias, m.key.bias, m.value.bias]).detach())
    for k, v in m.state_dict().items():
        if k != "key.bias":                                         # (its gradient is zero in exact arithmetic: a shift of every score of a row)
            assert not torch.equal(v, before[k]), f"{k} was not updated by the optimizer made before .cuda()"


@pytest.mark.parametrize("lowp", [False, True], ids=["fp32", "bf16"])
def test_qkv_deepcopy_and_unseated_fallback(seg, lowp):
    """copy.deepcopy of the module re-seats its parameters (a plain copy would silently take the torch.cat path), and its output and all
    gradients are bitwise the original's; so are those of the torch.cat fallback (parameters un-seated by assigning fresh .data)."""
    import pickle
    F = seg.functional
    m = _attn_module(seg, 12, 768).cuda()
    x, dy = torch.randn(2, 216, 768, device="cuda"), torch.randn(2, 216, 768, device="cuda")
    with F.autocast(BF16 if lowp else F32):
        want = _attn_module_run(m, x, dy)
        for how, dup in (("deepcopy", copy.deepcopy(m)), ("pickle", pickle.loads(pickle.dumps(m)))):
            assert F.qkv_params_are_fused(*_qkv_params(dup)), f"{how}: the copy lost the fused form"
            assert dup.query.weight.data_ptr() != m.query.weight.data_ptr()
            got = _attn_module_run(dup, x, dy)
            for k in want:
                assert torch.equal(got[k], want[k]), f"{how}: {k} differs by {_maxabs(got[k] - want[k]):.3e}"
        block = copy.deepcopy(torch.nn.ModuleList([m]))              # a copy of an enclosing module re-seats too
        assert F.qkv_params_are_fused(*_qkv_params(block[0]))
        loose = copy.deepcopy(m)
        for p in _qkv_params(loose):
            p.data = p.data.clone()
        assert not F.qkv_params_are_fused(*_qkv_params(loose))
        got = _attn_module_run(loose, x, dy)
        for k in want:
            assert torch.equal(got[k], want[k]), f"torch.cat fallback: {k} differs by {_maxabs(got[k] - want[k]):.3e}"


# ============================================================================= E. a TransformerBlock at production size
class _RoundedMatmul(torch.autograd.Function):
    """a @ b with both operands -- and in the backward the incoming gradient -- rounded to bf16, computed in the operands' dtype"""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        r = lambda t: t.to(BF16).to(t.dtype)
        return r(a) @ r(b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        r = lambda t: t.to(BF16).to(t.dtype)
        return r(g) @ r(b).transpose(-1, -2), r(a).transpose(-1, -2) @ r(g)


BLOCK_E, BLOCK_HEADS, BLOCK_P, BLOCK_FFN, BLOCK_DROP, FFN_DROP = 768, 12, 216, 2048, 0.1, 0.1


def _block_params(seed):
    """seeded N(0, K^-1/2) weights, small biases, gamma around 1 (named as in the module's state_dict)"""
    E, FF = BLOCK_E, BLOCK_FFN
    shapes = {"attention_norm.weight": (E,), "attention_norm.bias": (E,), "mlp_norm.weight": (E,), "mlp_norm.bias": (E,),
              "mlp.w_1.weight": (FF, E), "mlp.w_1.bias": (FF,), "mlp.w_2.weight": (E, FF), "mlp.w_2.bias": (E,),
              "attn.query.weight": (E, E), "attn.query.bias": (E,), "attn.key.weight": (E, E), "attn.key.bias": (E,),
              "attn.value.weight": (E, E), "attn.value.bias": (E,), "attn.out.weight": (E, E), "attn.out.bias": (E,)}
    out = {}
    for i, (n, s) in enumerate(shapes.items()):
        if len(s) == 2:
            out[n] = _randn(s, seed + i, s[1] ** -0.5)
        elif n.endswith("norm.weight"):
            out[n] = _randn(s, seed + i, 0.1, 1.0)
        else:
            out[n] = _randn(s, seed + i, 0.05)
    return out


def _block_chain(x, params, masks, dy, dt, rounded, preact_only=False):
    """The pre-norm block of unetr.py:148-168 written out in dtype dt: x1 = x + out(attention(LN x)) * mp, y = x1 + w_2(relu(w_1 LN x1) * mf),
    the dropout factors as explicit products (None: eval).  ``rounded``: every Linear and attention GEMM rounds its operands to bf16."""
    mm = _RoundedMatmul.apply if rounded else torch.matmul
    W = {n: t.to(dt).clone().requires_grad_(True) for n, t in params.items()}
    xr = x.to(dt).clone().requires_grad_(True)
    ma, mp, mf = (None if m is None else m.to(dt) for m in masks)
    lin = lambda t, n: (mm(t.reshape(-1, t.shape[-1]), W[n + ".weight"].t()) + W[n + ".bias"]).view(*t.shape[:-1], -1)
    B, P, E = x.shape
    H, d = BLOCK_HEADS, E // BLOCK_HEADS
    split = lambda t: t.view(B, P, H, d).permute(0, 2, 1, 3)
    n1 = TF.layer_norm(xr, (E,), W["attention_norm.weight"], W["attention_norm.bias"], 1e-6)
    q, k, v = split(lin(n1, "attn.query")), split(lin(n1, "attn.key")), split(lin(n1, "attn.value"))
    p = torch.softmax(mm(q, k.transpose(-1, -2)) * (1.0 / d ** 0.5), dim=-1)      # (d = 64: the scale is a power of two and commutes with the rounding)
    if ma is not None:
        p = p * ma
    mixed = mm(p, v).permute(0, 2, 1, 3).reshape(B, P, E)
    o = lin(mixed, "attn.out")
    x1 = (o if mp is None else o * mp.view(B, P, E)) + xr
    n2 = TF.layer_norm(x1, (E,), W["mlp_norm.weight"], W["mlp_norm.bias"], 1e-6)
    z = lin(n2, "mlp.w_1")
    if preact_only:
        return z.detach()
    h = torch.relu(z)
    if mf is not None:
        h = h * mf.view(B, P, BLOCK_FFN)
    y = lin(h, "mlp.w_2") + x1
    y.backward(dy.to(dt))
    return {"out": y.detach(), "dx": xr.grad, **{n: t.grad for n, t in W.items()}}


RELU_MARGIN = 1e-4


def _condition_relu_(x, params, masks):
    """ReLU's gradient jumps at 0: among the 432 x 2,048 pre-activations of w_1 (unit variance) a few lie within 1e-6 of it -- one of the seeded
    cases has one at 3.6e-8 --, closer than fp32 can place them (the output bound is 1e-5), and a gate that falls the other way moves a whole
    token's gradient.  That is a property of the input, not of a kernel, so the input is conditioned: the biases of the units that have such a
    pre-activation are nudged (in the fp64 reference, which alone decides) until none lies within RELU_MARGIN = 1e-4 of zero, ten times the
    output bound.  What precedes w_1 does not depend on its bias, so a nudge moves the unit's pre-activations by exactly its size."""
    bias = params["mlp.w_1.bias"]
    for trial in range(50):
        z = _block_chain(x, params, masks, None, F64, False, preact_only=True).reshape(-1, bias.numel())
        close = (z.abs() < RELU_MARGIN).any(0)
        if not bool(close.any()):
            return trial
        bias[close] += 3.0 * RELU_MARGIN
    raise AssertionError("could not move the ReLU pre-activations away from zero")


def _block_dev(seg, x, params, masks01, dy, lowp):
    from mi355seg.models.three_d.unetr import TransformerBlock
    F = seg.functional
    m = TransformerBlock(BLOCK_E, BLOCK_HEADS, BLOCK_DROP, (96, 96, 96), 16)
    m.load_state_dict(params)
    m.cuda()
    assert F.qkv_params_are_fused(*_qkv_params(m.attn))
    if masks01 is None:
        m.eval()
    else:
        m.train()
        m.attn.attn_dropout.forced_masks, m.attn.proj_dropout.forced_masks, m.mlp.dropout.forced_masks = [masks01[0]], [masks01[1]], [masks01[2]]
    xg = x.cuda().requires_grad_(True)
    with F.autocast(BF16 if lowp else F32):
        y, _ = m(xg)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    assert not (m.attn.attn_dropout.forced_masks or m.attn.proj_dropout.forced_masks or m.mlp.dropout.forced_masks)
    return {"out": y.detach().cpu(), "dx": xg.grad.cpu(), **{n: p.grad.cpu() for n, p in m.named_parameters()}}


@pytest.mark.parametrize("lowp", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("B", [1, 2])
def test_transformer_block_at_production_size(seg, B, train, lowp):
    """One TransformerBlock at E 768 / 12 heads / P 216 / FFN 2048: the pre-norm forks, the epilogue masks and the residuals composed, in train
    mode with all three dropout masks injected and in eval mode.  Output, input gradient and the gradient of EVERY parameter against the block
    written out in fp64.  The inputs are N(0, 1) plus a per-token offset, so the LayerNorms see non-centred rows."""
    E, P, H = BLOCK_E, BLOCK_P, BLOCK_HEADS
    x = _randn((B, P, E), 4000 + B) + _randn((B, P, 1), 4001, 2.0)
    dy = _randn((B, P, E), 4002)
    params = _block_params(4100)
    masks01 = masks = (None, None, None)
    if train:
        masks01 = tuple((torch.rand(s, generator=_gen(4200 + i)) < 1.0 - p).float()
                        for i, (s, p) in enumerate((((B, H, P, P), BLOCK_DROP), ((B * P, E), BLOCK_DROP), ((B * P, BLOCK_FFN), FFN_DROP))))
        masks = tuple(m / (1.0 - p) for m, p in zip(masks01, (BLOCK_DROP, BLOCK_DROP, FFN_DROP)))      # fp32 division, as the layer's own
    print(f"[transformer] block B{B}: {_condition_relu_(x, params, masks)} rounds of bias nudges keep the ReLU pre-activations {RELU_MARGIN:g} from zero")
    got = _block_dev(seg, x, params, masks01 if train else None, dy, lowp)
    u64 = _block_chain(x, params, masks, dy, F64, False)
    assert set(got) == set(u64)
    tag = f"block B{B} {'train' if train else 'eval'} {'bf16' if lowp else 'fp32'}"
    if not train and not lowp:                                      # the oracle's own block is the same arithmetic in eval mode
        from oracle.nets import _Block
        o = _Block(E, H, BLOCK_DROP).double().eval()
        o.load_state_dict({k: t.double() for k, t in params.items()})
        assert _maxabs(o(x.double()).detach() - u64["out"]) < 1e-12
    plain = {n: _out_bound(r) if n == "out" else _affine_bound(r) if "norm" in n else _grad_bound(r) for n, r in u64.items()}
    if not lowp:
        u32 = _block_chain(x, params, masks, dy, F32, False)
        for n in sorted(got):
            _grade(f"{tag} {n}", got[n], u64[n], u32[n], plain[n])
    else:
        r64, r32 = _block_chain(x, params, masks, dy, F64, True), _block_chain(x, params, masks, dy, F32, True)
        for n in sorted(got):
            _grade_lowp(f"{tag} {n}", got[n], r64[n], r32[n], u64[n], plain[n])
