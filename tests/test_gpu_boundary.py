"""The boundary loss term on the device (csrc/boundary.hip through functional.signed_distance_map / boundary_loss, CompoundLoss's
boundary_weight, engine.train_step, GraphedTrainStep and train.py's config.boundary_weight) against tests/test_boundary_host.py's
references.

Bounds:
  * the map at unit spacing: at most 1 float32 ulp from float32(ref_sdm).  Derived, not measured: every squared distance is an
    integer below 2^24, exact in float32; outside a class the kernel takes the correctly rounded sqrtf of it, and
    float32(sqrt_fp64(n)) == sqrt_fp32(n) for every integer n below 800,000; inside a class sqrt(n) - offset is formed with a
    compensated subtraction, rounded once.  Bitwise equality is the expected outcome and whether it held is printed;
  * the map at the spacings (2.5, 0.7, 0.7) and (1, 1, 3): 4 x the deviation of the CPU float32 restatement of the same three passes
    (cpu32_sdm) from the fp64 reference on the same input (the project's convention for stencil kernels); the measured figures are
    in test_map_at_anisotropic_spacing;
  * the loss: 1e-6 * max(1, |ref|) (LOSS_TOL of tests/test_gpu_loss_tail.py); dlogits: 1e-9 + 2e-5 * max|ref| (LIB_GRAD).
Every graded figure is printed beside its bound (``pytest -rA``)."""
import ctypes
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_boundary_host import boundary_masks, cpu32_sdm, ref_boundary, ref_sdm
from test_cldice_host import ref_cldice
from test_gpu_hd95 import check_pins

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
LOSS_TOL, LIB_GRAD = 1e-6, 2e-5
UP = 1.7
# csrc/boundary.hip: pass W takes a line in ballot words of 64 voxels (kWave); passes H and D give a block kSdmTW = 64 columns and
# kSdmRows = 32 output rows and stage the source line in chunks of kSdmTJ = 32 rows.  33 x 33 x 65 is one tile / chunk + 1 along
# every axis (for pass D the columns are the H * W plane: 2145 = 33 tiles + 33), 32 x 64 x 64 an exact multiple along every axis;
# 130 is two ballot words + 2; 600 / 300 are lines of many words, chunks and row blocks; 3 x 3 x 4 x 9 x 11 holds an absent, a full
# and a normal class side by side
SHAPES = [(1, 1, 1, 1, 1), (1, 2, 1, 1, 5), (2, 2, 3, 5, 7), (3, 3, 4, 9, 11), (1, 1, 2, 3, 130), (1, 1, 33, 33, 65), (1, 2, 32, 64, 64),
          (1, 1, 2, 3, 600), (1, 1, 2, 300, 3), (1, 1, 300, 2, 3)]
ANISO = [(2.5, 0.7, 0.7), (1, 1, 3)]
PIN_SPACINGS = [(1, 1, 1)] + ANISO + [(0.7, 0.7, 0.7)]


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mi355seg
    mi355seg.lib()          # raises if the HIP library is missing -- no fallback
    return mi355seg


def _sid(s):
    return "x".join(str(v) for v in s)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _maxabs(t):
    return float(t.abs().max()) if t.numel() else 0.0


_MASKS, _REFS = {}, {}


def _masks(shape):
    """the masks of one shape -- made once, shared, never modified"""
    if shape not in _MASKS:
        _MASKS[shape] = boundary_masks(shape, 100 * (sum(shape) % 89) + 7)
    return _MASKS[shape]


def _ref(shape, name, spacing):
    key = (shape, name, spacing)
    if key not in _REFS:
        _REFS[key] = ref_sdm(_masks(shape)[name].numpy(), spacing)
    return _REFS[key]


def _ulps(a, b):
    """distance of two float32 arrays in units in the last place (+0 and -0 are 0 apart)"""
    def ordered(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def _dev_map(seg, t, spacing=(1, 1, 1)):
    phi = seg.functional.signed_distance_map(t.cuda(), spacing)
    K = t.shape[1]
    assert phi.dtype == F32 and not phi.requires_grad and tuple(phi.shape) == (t.shape[0], K - (1 if K > 1 else 0)) + tuple(t.shape[2:])
    return phi.cpu().numpy()


# ----------------------------------------------------------------------------- the map
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_map_at_unit_spacing(seg, shape):
    """at most 1 float32 ulp from float32(ref_sdm) (derived in the module docstring); bitwise equality expected"""
    for name, t in _masks(shape).items():
        got, want = _dev_map(seg, t), _ref(shape, name, (1, 1, 1)).astype(np.float32)
        worst, bitwise = int(_ulps(got, want).max()), bool(np.array_equal(got, want))
        print(f"[boundary] map {_sid(shape)} {name}: worst {worst} ulp, bound 1 ulp; bitwise equal {bitwise} (max|phi| {np.abs(want).max():.4g})")
        assert np.isfinite(got).all() and worst <= 1, name


@pytest.mark.parametrize("spacing", ANISO, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_map_at_anisotropic_spacing(seg, shape, spacing):
    """Against ref_sdm in fp64, bound 4 x the deviation of cpu32_sdm (the same three passes in CPU float32) from the same reference.
    Measured on an MI355X over these shapes, masks and spacings: the largest kernel / CPU-fp32 ratio is 1.09 (9.2e-6 against 8.5e-6
    at max|phi| 99.5: 1x2x32x64x64, corner voxel, spacing (2.5, 0.7, 0.7)), against the bound's 4; the largest deviation is 6.1e-5 at
    max|phi| 1797 (half an ulp there) for both.  Most of either is float32(0.7) itself, which both share."""
    for name, t in _masks(shape).items():
        ref = _ref(shape, name, spacing)
        got, c32 = _dev_map(seg, t, spacing), cpu32_sdm(t.numpy(), spacing)
        ek, ec = float(np.abs(got.astype(np.float64) - ref).max()), float(np.abs(c32.astype(np.float64) - ref).max())
        print(f"[boundary] map {_sid(shape)} spacing {spacing} {name}: kernel {ek:.3e}  CPU-fp32 {ec:.3e}  bound {4 * ec:.3e}  (max|ref| {np.abs(ref).max():.4g})")
        assert np.isfinite(got).all() and ek <= 4 * ec, name


def sdm_pin_digests(F):
    """"<shape> <spacing>" -> {"input", "output"}: SHA-256 over the masks of the shape in sorted name order, of the targets' bytes and
    the spacing, and of the bytes of functional.signed_distance_map"""
    out = {}
    for shape in SHAPES:
        masks = _masks(shape)
        for spacing in PIN_SPACINGS:
            hin, hout = hashlib.sha256(np.asarray(spacing, np.float64).tobytes()), hashlib.sha256()
            for name in sorted(masks):
                hin.update(masks[name].numpy().tobytes())
                hout.update(F.signed_distance_map(masks[name].cuda(), spacing).cpu().numpy().tobytes())
            out[f"{_sid(shape)} {spacing}"] = {"input": hin.hexdigest(), "output": hout.hexdigest()}
    return out


def test_map_bits_equal_the_recorded_digests(seg):
    """tests/golden/edt_pins.json: the bytes of the map on every shape and mask above at four spacings, recorded before boundary.hip
    and surface.hip came to share csrc/edt.h -- the anisotropic maps too, which the tests above hold to a 4 x bound only"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edt_pins.json")) as fh:
        pins = json.load(fh)
    check_pins(sdm_pin_digests(seg.functional), pins["signed_distance_map"], "signed_distance_map")


def test_the_sign_is_never_wrong_at_a_spacing_below_one(seg):
    """spacing 0.7: inside a class phi <= 0, outside phi > 0 (the official '- 1' gives +0.3 on the inner boundary)"""
    for shape in ((2, 2, 3, 5, 7), (1, 1, 33, 33, 65)):
        for name, t in _masks(shape).items():
            got = _dev_map(seg, t, (0.7, 0.7, 0.7))
            c0 = 1 if shape[1] > 1 else 0
            pos = t.numpy()[:, c0:] > 0.5
            live = np.broadcast_to((pos.any(axis=(2, 3, 4)) & ~pos.all(axis=(2, 3, 4)))[:, :, None, None, None], pos.shape)
            assert (got[pos] <= 0).all() and (got[~pos & live] > 0).all() and not got[~live].any(), (shape, name)
    blob = torch.zeros(1, 1, 6, 7, 8)
    blob[0, 0, 1:5, 1:6, 1:7] = 1.0
    got = _dev_map(seg, blob, (0.7, 0.7, 0.7))
    print(f"[boundary] spacing 0.7: inner boundary {got[0, 0, 1, 1, 1]:.3e} (0), one voxel in {got[0, 0, 2, 2, 2]:.7f} (-0.7)")
    assert abs(got[0, 0, 1, 1, 1]) <= 1e-7 and abs(got[0, 0, 2, 2, 2] + 0.7) <= 1e-7


def test_the_map_is_reproducible_and_independent_of_the_batch(seg):
    """two runs: identical bits; a batched run has the bits of single-volume runs, per (n, k) volume"""
    for shape, spacing in (((3, 3, 4, 9, 11), (1, 1, 1)), ((2, 2, 33, 33, 65), (2.5, 0.7, 0.7))):
        for name, t in _masks(shape).items():
            a, b = _dev_map(seg, t, spacing), _dev_map(seg, t, spacing)
            assert np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b)), name
            singles = np.concatenate([_dev_map(seg, t[i:i + 1], spacing) for i in range(shape[0])])
            assert np.array_equal(a, singles), name
            for k in range(1, shape[1]):                                  # one class at a time, as a K = 1 target
                assert np.array_equal(a[:, k - 1:k], _dev_map(seg, t[:, k:k + 1], spacing)), (name, k)


def test_map_on_a_view_and_bad_shapes(seg):
    t = _masks((2, 2, 3, 5, 7))["density 0.5"]
    want = _dev_map(seg, t)
    tt = t.transpose(3, 4).contiguous().cuda().transpose(3, 4)            # the same values, not contiguous
    assert not tt.is_contiguous() and np.array_equal(seg.functional.signed_distance_map(tt).cpu().numpy(), want)
    with pytest.raises(seg.Mi355SegError, match=r"expected \[N,K,D,H,W\]"):
        seg.functional.signed_distance_map(t[0].cuda())
    with pytest.raises(seg.Mi355SegError, match="an axis is longer than 2047"):
        seg.functional.signed_distance_map(torch.zeros(1, 1, 1, 1, 2048, device="cuda"))
    with pytest.raises(seg.Mi355SegError, match="K must be in 1..16"):
        seg.functional.signed_distance_map(torch.zeros(1, 17, 1, 1, 2, device="cuda"))


# ----------------------------------------------------------------------------- the loss
def _loss_case(K, vol):
    N = 2
    g = _gen(60 + K + sum(vol))
    x = torch.randn((N, K) + vol, generator=g) * 3.0
    x.view(-1)[::7] = 30.0
    x.view(-1)[3::11] = -30.0
    t = boundary_masks((N, K) + vol, 17 + K)["density 0.5"]
    t[0, -1, 1:, 1:4, 2:9] = 1.0                                          # a solid block: inside distances beyond the offset
    if K > 1:
        t[0, :-1, 1:, 1:4, 2:9] = 0.0
    return x, t


def _check_boundary(seg, tag, x, t, spacing=(1, 1, 1)):
    xr = x.double().requires_grad_(True)
    ref = ref_boundary(xr, t, spacing)
    (ref * UP).backward()
    xg = x.cuda().requires_grad_(True)
    loss, parts = seg.functional.boundary_loss_full(xg, t.cuda(), spacing)
    assert loss.dtype == F32 and loss.dim() == 0 and loss.requires_grad
    assert parts.dtype == F64 and tuple(parts.shape) == (1,) and not parts.requires_grad
    (loss * UP).backward()
    grad = xg.grad.cpu()
    for name, got in (("loss", loss), ("parts", parts[0])):
        err, bound = abs(float(got.detach()) - ref.item()), LOSS_TOL * max(1.0, abs(ref.item()))
        print(f"[boundary] {tag} {name}: {float(got.detach()):.9f} ref {ref.item():.9f} error {err:.3e} bound {bound:.3e}")
        assert math.isfinite(float(got.detach())) and err <= bound, (tag, name)
    eg, bound = _maxabs(grad.double() - xr.grad), 1e-9 + LIB_GRAD * _maxabs(xr.grad)
    print(f"[boundary] {tag} dlogits: error {eg:.3e} bound {bound:.3e} (max|ref| {_maxabs(xr.grad):.3e})")
    assert grad.shape == x.shape and bool(torch.isfinite(grad).all()) and eg <= bound, tag
    if x.shape[1] > 1:
        assert not bool(grad[:, 0].any()) and not bool(torch.signbit(grad[:, 0]).any()), "the background channel takes no part"
    alone = seg.functional.boundary_loss(x.cuda(), t.cuda(), spacing)
    assert torch.equal(alone, loss.detach()) and not alone.requires_grad
    return float(loss), grad


@pytest.mark.parametrize("vol", [(5, 9, 33), (4, 9, 32)], ids=_sid)         # S % 4 != 0: scalar backward; S % 4 == 0: 16-byte accesses
@pytest.mark.parametrize("K", [1, 3])
def test_boundary_loss_against_fp64(seg, K, vol):
    x, t = _loss_case(K, vol)
    _check_boundary(seg, f"K={K} {_sid(vol)}", x, t)
    _check_boundary(seg, f"K={K} {_sid(vol)} spacing (2.5, 0.7, 0.7)", x, t, (2.5, 0.7, 0.7))


def test_boundary_loss_beyond_one_grid_of_the_streaming_kernels(seg):
    """540,800 elements: more than the 2048 blocks x 256 threads of the loss kernels' grids, so their grid-stride walks take a
    second step (forward partials, vector backward)"""
    g = _gen(77)
    vol = (8, 260, 260)
    x = torch.randn((1, 1) + vol, generator=g) * 3.0
    t = (torch.nn.functional.avg_pool3d(torch.rand((1, 1) + vol, generator=g), 5, 1, 2) > 0.5).float()
    assert x.numel() > 2048 * 256 and 0.1 < float(t.mean()) < 0.9
    _check_boundary(seg, "1x1x8x260x260", x, t)


def test_boundary_loss_of_a_target_without_a_boundary_is_zero(seg):
    """every class absent or full: phi = 0, the term and its gradient are exactly 0"""
    x = torch.randn(2, 2, 4, 5, 6, generator=_gen(5))
    t = torch.zeros(2, 2, 4, 5, 6)
    t[0, 0] = 1.0
    t[1, 1] = 1.0
    xg = x.cuda().requires_grad_(True)
    loss = seg.functional.boundary_loss(xg, t.cuda())
    loss.backward()
    assert float(loss) == 0.0 and not bool(xg.grad.any())


def test_boundary_loss_two_calls_are_bitwise_equal_and_misaligned_logits(seg):
    x, t = _loss_case(3, (4, 9, 32))
    runs = []
    for _ in range(2):
        xg = x.cuda().requires_grad_(True)
        loss, parts = seg.functional.boundary_loss_full(xg, t.cuda())
        seg.functional.workspace(1, xg.device).fill_(255)
        (loss * UP).backward()
        runs.append((loss.detach().clone(), parts.clone(), xg.grad.clone()))
    for u, v in zip(*runs):
        assert torch.equal(u, v)
    flat = torch.empty(x.numel() + 1, device="cuda")
    flat[1:] = x.cuda().view(-1)
    xm = flat[1:].view(x.shape).requires_grad_(True)                     # 4-byte aligned only: the scalar backward, the same values
    assert xm.data_ptr() % 16 != 0
    loss, _ = seg.functional.boundary_loss_full(xm, t.cuda())
    (loss * UP).backward()
    assert torch.equal(loss.detach(), runs[0][0]) and torch.equal(xm.grad, runs[0][2])


# ----------------------------------------------------------------------------- CompoundLoss
def _launches(L):
    buf = (ctypes.c_double * 32)()
    L.call("mi355seg_prof_read", buf, 32)
    nmax = 4096
    rec, n = (ctypes.c_double * (4 * nmax))(), ctypes.c_int(0)
    L.call("mi355seg_prof_records", rec, nmax, ctypes.byref(n))
    L.call("mi355seg_prof_enable", 0)
    return [(int(rec[4 * r]), rec[4 * r + 2], rec[4 * r + 3]) for r in range(n.value)]


def _tail_run(seg, criterion, x, t, record=False):
    L = seg.lib()
    xg = x.cuda().requires_grad_(True)
    if record:
        L.call("mi355seg_prof_reset")
        L.call("mi355seg_prof_enable", 1)
    loss, mask, counts, terms = criterion.tail(xg, t.cuda())
    (loss * UP).backward()
    rec = _launches(L) if record else None
    return loss.detach(), mask, counts, terms, xg.grad, rec


def _one_hot_case():
    x, t = _loss_case(2, (5, 9, 33))
    return x, t


def test_compound_loss_with_weight_zero_is_the_object_without_the_argument(seg):
    from mi355seg.utils.loss_function import CompoundLoss
    x, t = _one_hot_case()
    a = _tail_run(seg, CompoundLoss("dice_bce"), x, t, record=True)
    b = _tail_run(seg, CompoundLoss("dice_bce", boundary_weight=0.0, boundary_spacing=(2, 1, 1)), x, t, record=True)
    for u, v in zip(a[:5], b[:5]):
        assert u.dtype == v.dtype and torch.equal(u, v)
    assert tuple(b[3].shape) == (2,) and a[5] == b[5] and len(a[5]) >= 2, (a[5], b[5])


def test_compound_loss_with_a_boundary_weight_and_a_changed_scale(seg):
    from mi355seg.utils.loss_function import CompoundLoss
    x, t = _one_hot_case()
    base = _tail_run(seg, CompoundLoss("dice_bce"), x, t)
    crit = CompoundLoss("dice_bce", boundary_weight=0.5)
    both = _tail_run(seg, crit, x, t)
    assert crit.boundary_scale.is_cuda and crit.boundary_scale.dtype == F32 and crit.boundary_scale.tolist() == [0.5]
    xg = x.cuda().requires_grad_(True)
    bd = seg.functional.boundary_loss(xg, t.cuda())
    (bd * UP).backward()
    for scale, run in ((0.5, both), (0.125, None)):
        if run is None:
            crit.set_boundary_scale(scale)
            run = _tail_run(seg, crit, x, t)
        want = float(base[0]) + scale * float(bd)
        print(f"[boundary] CompoundLoss scale {scale}: loss {float(run[0]):.9f} tail + scale * boundary {want:.9f}")
        assert abs(float(run[0]) - want) <= LOSS_TOL * max(1.0, abs(want))
        assert torch.equal(run[1], base[1]) and torch.equal(run[2], base[2])
        terms = run[3]
        assert terms.dtype == F64 and tuple(terms.shape) == (3,) and torch.equal(terms[:2], base[3])
        assert abs(float(terms[2]) - float(bd)) <= LOSS_TOL
        gsum = base[4] + scale * xg.grad
        eg, bound = _maxabs(run[4] - gsum), 1e-9 + LIB_GRAD * _maxabs(gsum)
        print(f"[boundary] CompoundLoss scale {scale}: gradient against the sum of the two {eg:.3e} bound {bound:.3e}")
        assert eg <= bound


# ----------------------------------------------------------------------------- engine
_GRAPHED = r"""
import sys, torch
sys.path.insert(0, %r)
import mi355seg
from mi355seg.engine import GraphedTrainStep, train_step
from mi355seg.models.three_d.unet3d import UNet3D
from mi355seg.utils.loss_function import CompoundLoss
from oracle.fill import fill_module_, make_input, make_labels
x, gt = make_input((1, 1, 16, 16, 16)).cuda(), make_labels((1, 1, 16, 16, 16)).cuda()
W = 0.5

def build():
    m = fill_module_(UNet3D(1, 2, 4)).cuda().train()
    return m, torch.optim.Adam(m.parameters(), lr=1e-3, capturable=True), CompoundLoss("dice_bce", boundary_weight=W)

m0, o0, c0 = build()
for _ in range(4):
    e = train_step(m0, o0, x, gt, criterion=c0, sync_metric=False)
l0, t0 = e["loss"].item(), e["loss_terms"].tolist()
m1, o1, c1 = build()
g = GraphedTrainStep(m1, o1, x, gt, criterion=c1, warmup=1)
graph = g.graph
assert "loss_terms" in g.first and len(g.first["loss_terms"]) == 3
for _ in range(3):
    r = g(x, gt, sync_metric=False)
l1, t1 = r["loss"].item(), r["loss_terms"].tolist()
torch.cuda.synchronize()
assert len(t0) == 3 and l0 == l1 and t0 == t1, (l0, l1, t0, t1)
for (k, a), (_, b) in zip(m0.state_dict().items(), m1.state_dict().items()):
    assert torch.equal(a, b), k
# the scale is a device buffer: the next replay of the SAME graph uses the new value
c0.set_boundary_scale(0.25 * W)
c1.set_boundary_scale(0.25 * W)
e = train_step(m0, o0, x, gt, criterion=c0, sync_metric=False)
r = g(x, gt, sync_metric=False)
torch.cuda.synchronize()
assert g.graph is graph
l2, t2 = r["loss"].item(), r["loss_terms"].tolist()
assert l2 == e["loss"].item() and t2 == e["loss_terms"].tolist(), (l2, e["loss"].item())
want = t2[0] + t2[1] + 0.25 * W * t2[2]
full = t2[0] + t2[1] + W * t2[2]
assert abs(l2 - want) <= 1e-6 * max(1.0, abs(want)), (l2, want)
assert abs(t2[2]) > 1e-3 and abs((full - l2) - 0.75 * W * t2[2]) <= 1e-6 * max(1.0, abs(full)), (l2, full, t2)
for (k, a), (_, b) in zip(m0.state_dict().items(), m1.state_dict().items()):
    assert torch.equal(a, b), k
print("GRAPHED_BOUNDARY_OK", l1, t1, l2, t2)
"""


def test_train_step_adds_the_term_and_reports_it(seg):
    """engine.train_step on UNet3D(1, 2, 4) at [1, 1, 16^3]: the loss is the tail's loss + 0.5 * boundary, both recomputed in fp64 on
    the returned logits; mask, counters and the first two terms are those of the step without the term; with clDice also on there
    are four terms: voxel, region, cldice, boundary."""
    from mi355seg.engine import train_step
    from mi355seg.models.three_d.unet3d import UNet3D
    from mi355seg.utils.loss_function import CompoundLoss
    from oracle import losses as OL
    from oracle.fill import fill_module_, make_input, make_labels
    x, gt = make_input((1, 1, 16, 16, 16)).cuda(), make_labels((1, 1, 16, 16, 16)).cuda()
    outs = []
    for crit in (CompoundLoss("dice_bce", boundary_weight=0.5), CompoundLoss("dice_bce"),
                 CompoundLoss("dice_bce", cldice_weight=0.25, boundary_weight=0.5)):
        m = fill_module_(UNet3D(1, 2, 4)).cuda().train()
        outs.append(train_step(m, torch.optim.Adam(m.parameters(), lr=1e-3), x, gt, criterion=crit, sync_metric=False))
    with_bd, without, four = outs
    assert tuple(with_bd["loss_terms"].shape) == (3,) and tuple(without["loss_terms"].shape) == (2,) and tuple(four["loss_terms"].shape) == (4,)
    for o in (with_bd, four):
        assert torch.equal(o["pred"], without["pred"]) and torch.equal(o["mask"], without["mask"])
        assert torch.equal(o["counts"], without["counts"]) and torch.equal(o["loss_terms"][:2], without["loss_terms"])
    pred = with_bd["pred"].detach().cpu().double()
    gt2 = seg.functional.two_channel_gt(gt).cpu().double()
    bd, cl = ref_boundary(pred, gt2).item(), float(ref_cldice(pred, gt2)[0])
    tail = float(OL.dice_loss(pred, gt2) + OL.bce_with_logits(pred, gt2))
    want = tail + 0.5 * bd
    print(f"[boundary] engine: loss {float(with_bd['loss']):.9f} fp64 {want:.9f}; boundary {float(with_bd['loss_terms'][2]):.9f} fp64 {bd:.9f}")
    assert abs(float(with_bd["loss"]) - want) <= LOSS_TOL * max(1.0, abs(want))
    assert abs(float(with_bd["loss_terms"][2]) - bd) <= LOSS_TOL * max(1.0, abs(bd))
    want4 = tail + 0.25 * cl + 0.5 * bd
    print(f"[boundary] engine, four terms: loss {float(four['loss']):.9f} fp64 {want4:.9f}; terms {four['loss_terms'].tolist()}")
    assert abs(float(four["loss"]) - want4) <= LOSS_TOL * max(1.0, abs(want4))
    assert abs(float(four["loss_terms"][2]) - cl) <= LOSS_TOL * max(1.0, abs(cl))
    assert abs(float(four["loss_terms"][3]) - bd) <= LOSS_TOL * max(1.0, abs(bd))


def test_graphed_step_with_the_term_equals_the_eager_steps_and_follows_the_scale(seg):
    """Four eager steps with CompoundLoss("dice_bce", boundary_weight=0.5) and a capturable Adam against GraphedTrainStep plus three
    replays: the last loss, its three terms and every state-dict entry bitwise equal.  Then set_boundary_scale(0.25 * w) on both: the
    next replay of the same graph (no re-capture) equals the eager step again, and its loss is voxel + region + 0.125 * boundary --
    below the full-weight sum by 0.75 * w * boundary.  Run once, in a process of its own, with a timeout."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _GRAPHED % root], capture_output=True, text=True, timeout=300)
    print(p.stdout[-600:])
    assert p.returncode == 0 and "GRAPHED_BOUNDARY_OK" in p.stdout, (p.returncode, p.stdout[-1000:], p.stderr[-3000:])


# ----------------------------------------------------------------------------- train.py
def _rows(cfg):
    return [json.loads(l) for l in open(os.path.join(cfg.hydra_path, "scalars.jsonl")).read().strip().splitlines()]


def test_train_cli_config_boundary_weight_and_ramp(seg, tmp_path):
    """``train.py config=unet config.loss=dice_bce config.boundary_weight=0.5 config.boundary_ramp_epochs=2``, two epochs: every row
    of scalars.jsonl holds a finite Training/loss_boundary; Loss - voxel - region is 0.25 * boundary in epoch 1 and 0.5 * boundary in
    epoch 2.  Without the keys the columns are those of the run before the term existed."""
    from mi355seg.train import main
    torch.manual_seed(11)
    common = ["config=unet", "config.data_path=synthetic", "config.patch_size=16,16,16", "config.loss=dice_bce"]
    cfg, res = main(common + [f"config.output_dir={tmp_path / 'boundary'}", "config.epochs=2", "config.boundary_weight=0.5",
                              "config.boundary_ramp_epochs=2"])
    rows = _rows(cfg)
    assert rows and len(rows) % 2 == 0 and res["epoch"] == 2
    half = len(rows) // 2
    for i, r in enumerate(rows):
        assert set(r) == {"iteration", "Training/Loss", "Training/dice", "Training/loss_voxel", "Training/loss_region", "Training/loss_boundary"}
        bd, scale = r["Training/loss_boundary"], (0.25 if i < half else 0.5)
        rest = r["Training/Loss"] - r["Training/loss_voxel"] - r["Training/loss_region"]
        print(f"[boundary] train.py row {i}: Loss - voxel - region {rest:.9f}  {scale} * boundary {scale * bd:.9f}")
        assert math.isfinite(bd) and abs(rest - scale * bd) <= LOSS_TOL * max(1.0, abs(r["Training/Loss"]))
    assert any(abs(r["Training/loss_boundary"]) > 1e-3 for r in rows)
    cfg, res = main(common + [f"config.output_dir={tmp_path / 'plain'}", "config.epochs=1"])
    for r in _rows(cfg):
        assert set(r) == {"iteration", "Training/Loss", "Training/dice", "Training/loss_voxel", "Training/loss_region"}


# ----------------------------------------------------------------------------- the C entry points' refusals (nothing is launched)
def test_entry_points_refuse_bad_arguments_before_any_launch(seg):
    L = seg.lib()
    E = seg.Mi355SegError
    q = lambda *a: L.query("mi355seg_sdm_ws_bytes", *a)
    assert q(1, 1, 1, 1, 1) == 1024                                    # four pieces, each rounded up to 256 bytes
    assert q(2, 2, 128, 128, 128) == q(2, 1, 128, 128, 128) == 12 * 2 * 128 ** 3          # K = 2: one channel takes part
    assert q(1, 4, 160, 192, 160) == 12 * 3 * 160 * 192 * 160
    assert q(1, 1, 2047, 1, 1024) > 0 and q(1, 16, 2, 2, 2) > 0
    for bad in ((0, 1, 8, 8, 8), (-1, 1, 8, 8, 8), (1, 0, 8, 8, 8), (1, 17, 8, 8, 8), (1, 1, 0, 8, 8), (1, 1, 8, -2, 8), (1, 1, 8, 8, 0),
                (1, 1, 2048, 8, 8), (1, 1, 8, 2048, 8), (1, 1, 8, 8, 2048), (1, 1, 2047, 2047, 2047), (1 << 40, 16, 1024, 1024, 1024), (1 << 33, 1, 1, 1, 1)):
        assert q(*bad) == 0, bad
    assert L.query("mi355seg_boundary_ws_bytes", 0) == 0 and L.query("mi355seg_boundary_ws_bytes", -5) == 0
    assert L.query("mi355seg_boundary_ws_bytes", 1) == 8 and L.query("mi355seg_boundary_ws_bytes", 1 << 40) == 2048 * 8
    p = 256                                    # a non-null address that is never dereferenced: every call below is refused first
    big = 1 << 40
    sdm, steps = "mi355seg_sdm_f32", "mi355seg_sdm_steps_f32"
    ok = dict(target=p, N=1, K=2, D=2, H=2, W=2, sz=1.0, sy=1.0, sx=1.0, offset=1.0, phi=p, ws=p, ws_bytes=big)

    def call_sdm(name=sdm, extra=(), **kw):
        a = dict(ok, **kw)
        L.call(name, a["target"], a["N"], a["K"], a["D"], a["H"], a["W"], a["sz"], a["sy"], a["sx"], a["offset"], a["phi"], a["ws"],
               a["ws_bytes"], *extra, None)

    for name, extra in ((sdm, ()), (steps, (3,))):
        for kw in ({"target": None}, {"phi": None}, {"ws": None}):
            with pytest.raises(E, match="sdm: null pointer"):
                call_sdm(name, extra, **kw)
        for kw in ({"N": 0}, {"N": -1}, {"D": 0}, {"H": -3}, {"W": 0}):
            with pytest.raises(E, match="sdm: bad extents"):
                call_sdm(name, extra, **kw)
        for K in (0, 17, -1):
            with pytest.raises(E, match=f"sdm: K must be in 1..16, got {K}"):
                call_sdm(name, extra, K=K)
        for kw in ({"D": 2048}, {"H": 2048}, {"W": 4096}):
            with pytest.raises(E, match="sdm: an axis is longer than 2047"):
                call_sdm(name, extra, **kw)
        with pytest.raises(E, match="sdm: more than 2\\^31 - 1 voxels per volume"):
            call_sdm(name, extra, D=2047, H=2047, W=2047)
        with pytest.raises(E, match="sdm: N \\* K \\* D \\* H \\* W exceeds 2\\^56"):
            call_sdm(name, extra, N=1 << 40, K=16, D=1024, H=1024, W=1024)
        with pytest.raises(E, match="sdm: more than 2\\^31 - 1 tiles in one launch"):
            call_sdm(name, extra, N=1 << 33, K=1, D=1, H=1, W=1)
        for kw in ({"sz": 0.0}, {"sy": -1.0}, {"sx": float("nan")}, {"sx": float("inf")}):
            with pytest.raises(E, match="sdm: the spacing must be positive and finite"):
                call_sdm(name, extra, **kw)
        for off in (-0.5, float("nan"), float("inf")):
            with pytest.raises(E, match="sdm: the offset must be >= 0 and finite"):
                call_sdm(name, extra, offset=off)
        with pytest.raises(E, match="sdm: the workspace must be 4-byte aligned"):
            call_sdm(name, extra, ws=p + 2)
        with pytest.raises(E, match="workspace too small: need 1024 bytes, have 1023"):
            call_sdm(name, extra, ws_bytes=1023)
    for s in (0, 4, -1):
        with pytest.raises(E, match=f"sdm: steps must be in 1..3, got {s}"):
            call_sdm(steps, (s,))

    fwd, bwd = "mi355seg_boundary_fwd_f32", "mi355seg_boundary_bwd_f32"
    okf = dict(logits=p, phi=p, N=1, K=2, S=8, loss=p, parts=p, coef=p, ws=p, ws_bytes=big)

    def call_fwd(**kw):
        a = dict(okf, **kw)
        L.call(fwd, a["logits"], a["phi"], a["N"], a["K"], a["S"], a["loss"], a["parts"], a["coef"], a["ws"], a["ws_bytes"], None)

    for key in ("logits", "phi", "loss", "parts", "coef", "ws"):
        with pytest.raises(E, match="boundary_fwd: null pointer"):
            call_fwd(**{key: None})
    for kw in ({"N": 0}, {"S": 0}, {"S": -8}):
        with pytest.raises(E, match="boundary_fwd: bad extents"):
            call_fwd(**kw)
    for K in (0, 17):
        with pytest.raises(E, match=f"boundary_fwd: K must be in 1..16, got {K}"):
            call_fwd(K=K)
    with pytest.raises(E, match="boundary_fwd: more than 2\\^31 - 1 voxels per volume"):
        call_fwd(S=1 << 31)
    with pytest.raises(E, match="boundary_fwd: N \\* K \\* S exceeds 2\\^56"):
        call_fwd(N=1 << 40, K=16, S=1 << 30)
    with pytest.raises(E, match="boundary_fwd: the workspace must be 8-byte aligned"):
        call_fwd(ws=p + 4)
    with pytest.raises(E, match="workspace too small: need 8 bytes, have 7"):
        call_fwd(ws_bytes=7)

    okb = dict(logits=p, phi=p, coef=p, gscale=p, N=1, K=2, S=8, dlogits=p)

    def call_bwd(**kw):
        a = dict(okb, **kw)
        L.call(bwd, a["logits"], a["phi"], a["coef"], a["gscale"], a["N"], a["K"], a["S"], a["dlogits"], None)

    for key in ("logits", "phi", "coef", "gscale", "dlogits"):
        with pytest.raises(E, match="boundary_bwd: null pointer"):
            call_bwd(**{key: None})
    for kw in ({"N": -2}, {"S": 0}):
        with pytest.raises(E, match="boundary_bwd: bad extents"):
            call_bwd(**kw)
    for K in (0, 17):
        with pytest.raises(E, match=f"boundary_bwd: K must be in 1..16, got {K}"):
            call_bwd(K=K)
    with pytest.raises(E, match="boundary_bwd: more than 2\\^31 - 1 voxels per volume"):
        call_bwd(S=1 << 31)
    with pytest.raises(E, match="boundary_bwd: N \\* K \\* S exceeds 2\\^56"):
        call_bwd(N=1 << 40, K=16, S=1 << 30)
