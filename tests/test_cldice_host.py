"""The soft-clDice term without a GPU: the fp64 reference that tests/test_gpu_cldice.py grades the kernels against
(``ref_soft_skel`` / ``ref_cldice``, DESIGN.md 4.20: one uniform step per level, ties routed to ONE voxel, the candidate with the
lowest raster index), checked against the official open / loop formulation of clDice (Shit et al., CVPR 2021) composed from ATen's
pools; train.parse_loss's three keys, CompoundLoss's three arguments, and the refusals of the C entry points that need no launch."""
import pytest
import torch
import torch.nn.functional as TF

import mi355seg
from mi355seg.config import Config

INF = float("inf")
CROSS = [(-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0)]            # raster order (z, y, x)
BOX = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def _shifted(x, offsets, pad):
    """[len(offsets), N, C, D, H, W]: entry k holds x[v + offsets[k]] at v, ``pad`` outside the volume"""
    D, H, W = x.shape[2:]
    xp = TF.pad(x, (1, 1, 1, 1, 1, 1), value=pad)
    return torch.stack([xp[:, :, 1 + dz:1 + dz + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dz, dy, dx in offsets])


def ref_erode(x):
    """minimum over the voxel and its 6 face neighbours; torch.min(0) returns, and routes the gradient to, the first minimal index"""
    return _shifted(x, CROSS, INF).min(0).values


def ref_dilate(x):
    return _shifted(x, BOX, -INF).max(0).values


def ref_soft_skel(x, iters):
    e, skel = x, torch.zeros_like(x)
    for _ in range(iters + 1):
        e1 = ref_erode(e)
        delta = TF.relu(e - ref_dilate(e1))
        skel = skel + TF.relu(delta - skel * delta)
        e = e1
    return skel


def ref_cldice(logits, target, iters=3, smooth=1.0):
    """(cldice, tprec, tsens) in the dtype of ``logits``"""
    c0 = 1 if logits.shape[1] > 1 else 0
    P, T = torch.sigmoid(logits[:, c0:]), target[:, c0:].to(logits.dtype)
    sp, st = ref_soft_skel(P, iters), ref_soft_skel(T, iters)
    tprec = ((sp * T).sum() + smooth) / (sp.sum() + smooth)
    tsens = ((st * P).sum() + smooth) / (st.sum() + smooth)
    return 1.0 - 2.0 * tprec * tsens / (tprec + tsens), tprec, tsens


# ----------------------------------------------------------------------------- the official formulation and its uniform-step restatement, from ATen's pools
def aten_erode(x):
    p1 = -TF.max_pool3d(-x, (3, 1, 1), (1, 1, 1), (1, 0, 0))
    p2 = -TF.max_pool3d(-x, (1, 3, 1), (1, 1, 1), (0, 1, 0))
    p3 = -TF.max_pool3d(-x, (1, 1, 3), (1, 1, 1), (0, 0, 1))
    return torch.min(torch.min(p1, p2), p3)


def aten_dilate(x):
    return TF.max_pool3d(x, (3, 3, 3), (1, 1, 1), (1, 1, 1))


def official_soft_skel(x, iters):
    """soft_skel of the official clDice: open, then a loop of erode / open / update"""
    skel = TF.relu(x - aten_dilate(aten_erode(x)))
    for _ in range(iters):
        x = aten_erode(x)
        delta = TF.relu(x - aten_dilate(aten_erode(x)))
        skel = skel + TF.relu(delta - skel * delta)
    return skel


def aten_soft_skel(x, iters):
    """the uniform step of DESIGN.md 4.20 from ATen's pools: the composition whose fp32 bits the device forward has"""
    e, skel = x, torch.zeros_like(x)
    for _ in range(iters + 1):
        e1 = aten_erode(e)
        delta = TF.relu(e - aten_dilate(e1))
        skel = skel + TF.relu(delta - skel * delta)
        e = e1
    return skel


def permutation_input(shape, seed):
    """pairwise distinct values in (0, 1), as float32: x = (randperm(n) + 0.5) / n"""
    n = 1
    for s in shape:
        n *= s
    return ((torch.randperm(n, generator=torch.Generator().manual_seed(seed)).double() + 0.5) / n).float().reshape(shape)


SHAPES = [(1, 1, 1, 1, 1), (1, 1, 1, 1, 5), (2, 1, 2, 2, 2), (1, 2, 3, 5, 7), (1, 1, 4, 9, 11)]
ITERS = (1, 3, 6)


def _grad(fn, x, w):
    xr = x.detach().clone().requires_grad_(True)
    (fn(xr) * w).sum().backward()
    return xr.grad


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_equals_the_official_formulation_forward(shape, iters):
    """forward, exactly, in fp32 and fp64, on random, saturated and binary inputs -- and the uniform step from ATen's pools too"""
    g = torch.Generator().manual_seed(sum(shape) + iters)
    for x in (torch.rand(shape, generator=g), torch.sigmoid(8 * torch.randn(shape, generator=g)), (torch.rand(shape, generator=g) > 0.4).float()):
        for dt in (torch.float32, torch.float64):
            xx = x.to(dt)
            want = official_soft_skel(xx, iters)
            assert torch.equal(ref_soft_skel(xx, iters), want)
            assert torch.equal(aten_soft_skel(xx, iters), want)


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_gradient_equals_the_official_formulations_on_distinct_values(shape, iters):
    """pairwise distinct values: the gradient does not depend on the tie rule (equal values in any E_j trace back to one voxel)"""
    x = permutation_input(shape, 7 + iters).double()
    w = torch.rand(shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    a, b = _grad(lambda v: ref_soft_skel(v, iters), x, w), _grad(lambda v: official_soft_skel(v, iters), x, w)
    assert float((a - b).abs().max()) <= 1e-12


@pytest.mark.parametrize("iters", ITERS)
def test_binary_inputs_conserve_the_gradient_sum(iters):
    """ties everywhere: per voxel the two rules differ, the sum of the gradient of sum(skel) does not"""
    shape = (1, 2, 5, 6, 7)
    x = (torch.rand(shape, generator=torch.Generator().manual_seed(5)) > 0.35).double()
    w = torch.ones(shape, dtype=torch.float64)
    a, b = _grad(lambda v: ref_soft_skel(v, iters), x, w), _grad(lambda v: official_soft_skel(v, iters), x, w)
    assert abs(float(a.sum()) - float(b.sum())) <= 1e-9 * max(1.0, float(b.abs().sum()))
    assert float((a - b).abs().max()) > 0.1               # (the rules do differ here)


def test_the_whole_gradient_of_an_all_equal_erosion_goes_to_the_first_voxel():
    """3 x 3 x 3 of ones: d erode(x)[1,1,1] / dx is 1 at (0,1,1), the first of the 7 candidates in raster order, and 0 elsewhere
    (ATen's three pools split it 0.25 / 0.25 / 0.5)"""
    x = torch.ones(1, 1, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    ref_erode(x)[0, 0, 1, 1, 1].backward()
    want = torch.zeros(3, 3, 3, dtype=torch.float64)
    want[0, 1, 1] = 1.0
    assert torch.equal(x.grad[0, 0], want)
    y = torch.ones(1, 1, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    ref_dilate(y)[0, 0, 1, 1, 1].backward()
    want = torch.zeros(3, 3, 3, dtype=torch.float64)
    want[0, 0, 0] = 1.0
    assert torch.equal(y.grad[0, 0], want)


def test_ref_cldice_of_a_perfect_prediction_and_of_an_empty_target():
    t = torch.zeros(1, 2, 4, 6, 8, dtype=torch.float64)
    t[0, 1, 1:3, 2, 1:7] = 1.0
    t[0, 0] = 1.0 - t[0, 1]
    cl, tp, ts = ref_cldice((t * 2 - 1) * 1e3, t)
    assert abs(float(cl)) < 1e-12 and abs(float(tp) - 1) < 1e-12 and abs(float(ts) - 1) < 1e-12
    bg = torch.zeros_like(t)
    bg[0, 0] = 1.0
    cl, tp, ts = ref_cldice(torch.zeros_like(t), bg, smooth=1.0)
    assert float(ts) == 1.0 and 0.0 < float(tp) <= 1.0 and 0.0 <= float(cl) < 1.0        # sum S_T = 0: smooth / smooth


# ----------------------------------------------------------------------------- train.parse_loss
def test_parse_loss_cldice_keys():
    from mi355seg.train import LOSS_KEYS, parse_loss
    assert {"cldice_weight", "cldice_iters", "cldice_smooth"} <= set(LOSS_KEYS)
    c = parse_loss(Config({"loss": "dice_bce", "cldice_weight": 0.5}))
    assert (c.cldice_weight, c.cldice_iters, c.cldice_smooth) == (0.5, 3, 1.0)
    c = parse_loss(Config({"loss": "dice_ce", "cldice_weight": "0.25", "cldice_iters": "10", "cldice_smooth": "0.5"}))
    assert (c.cldice_weight, c.cldice_iters, c.cldice_smooth) == (0.25, 10, 0.5)
    c = parse_loss(Config({"loss": "tversky", "cldice_weight": 0, "cldice_iters": 32}))
    assert (c.cldice_weight, c.cldice_iters) == (0.0, 32)


@pytest.mark.parametrize("loss", [None, "bce"])
@pytest.mark.parametrize("key,value", [("cldice_weight", 0.5), ("cldice_iters", 3), ("cldice_smooth", 1.0)])
def test_parse_loss_refuses_cldice_keys_without_a_compound_loss(loss, key, value):
    from mi355seg.train import parse_loss
    with pytest.raises(ValueError, match=f"config.{key} must be given only with config.loss = a compound mode") as e:
        parse_loss(Config({"loss": loss, key: value}))
    assert "config.loss=bce" in str(e.value)


@pytest.mark.parametrize("key,value", [("cldice_weight", -0.1), ("cldice_weight", "half"), ("cldice_iters", 0), ("cldice_iters", 33),
                                       ("cldice_iters", 2.5), ("cldice_iters", "2.5"), ("cldice_iters", True), ("cldice_smooth", 0),
                                       ("cldice_smooth", -1.0)])
def test_parse_loss_refuses_bad_cldice_values_naming_the_key(key, value):
    from mi355seg.train import parse_loss
    with pytest.raises(ValueError, match=f"config.{key} must be") as e:
        parse_loss(Config({"loss": "dice_bce", key: value}))
    assert repr(value) in str(e.value)


# ----------------------------------------------------------------------------- CompoundLoss
def test_compound_loss_arguments_and_repr():
    from mi355seg.utils.loss_function import CompoundLoss
    plain, zero = CompoundLoss("dice_bce"), CompoundLoss("dice_bce", cldice_weight=0.0, cldice_iters=5, cldice_smooth=2.0)
    assert zero.spec == plain.spec == mi355seg.functional.LossSpec("bce", "dice", 2.0, 0.3, 0.7, 1.0, 1.0)
    assert repr(zero) == repr(plain) and "cldice" not in repr(plain)
    c = CompoundLoss("dice_bce", cldice_weight=0.5, cldice_iters=4)
    assert c.spec == plain.spec and "cldice=(weight=0.5, iters=4, smooth=1.0)" in repr(c)
    for kw in ({"cldice_weight": -1}, {"cldice_weight": "1"}, {"cldice_iters": 0}, {"cldice_iters": 33}, {"cldice_iters": 2.5},
               {"cldice_smooth": 0}, {"cldice_smooth": None}):
        with pytest.raises(ValueError, match="cldice_"):
            CompoundLoss("dice_bce", **kw)


def test_functional_refuses_cpu_tensors_and_bad_arguments():
    F = mi355seg.functional
    x = torch.zeros(1, 2, 3, 4, 5)
    with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):
        F.soft_skeleton(x)
    with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):
        F.soft_cldice(x, x)
    for iters in (0, 33, 2.5, True):
        with pytest.raises(ValueError, match="iters must be an integer in 1..32"):
            F.soft_skeleton(x, iters)
        with pytest.raises(ValueError, match="iters must be an integer in 1..32"):
            F.soft_cldice(x, x, iters)
    with pytest.raises(ValueError, match="smooth must be a number > 0"):
        F.soft_cldice(x, x, 3, 0.0)


# ----------------------------------------------------------------------------- the C entry points' refusals (nothing is launched)
def test_entry_points_refuse_bad_arguments_before_any_launch():
    L = mi355seg.lib()
    E = mi355seg.Mi355SegError
    assert L.query("mi355seg_soft_skel_ws_bytes", 4, 8, 8, 8, 3) == 8 * 4 * 8 * 8 * 8 * 4
    assert L.query("mi355seg_soft_skel_ws_bytes", 1, 1, 1, 1, 1) == 4 * 256                   # slots are rounded up to 256 bytes
    for bad in ((0, 8, 8, 8, 3), (4, 0, 8, 8, 3), (4, 8, 8, -1, 3), (4, 8, 8, 8, 0), (4, 8, 8, 8, 33), (1 << 20, 1 << 10, 2, 1, 3)):
        assert L.query("mi355seg_soft_skel_ws_bytes", *bad) == 0
    assert L.query("mi355seg_cldice_ws_bytes", 0) == 0 and L.query("mi355seg_cldice_ws_bytes", 1) == 32
    p = 256                                    # a non-null address that is never dereferenced: every call below is refused first
    fwd, bwd = "mi355seg_soft_skel_step_fwd_f32", "mi355seg_soft_skel_step_bwd_f32"
    big = 1 << 30
    with pytest.raises(E, match="soft_skel_step_fwd: null pointer"):
        L.call(fwd, None, 1, 2, 2, 2, 3, 0, p, big, None)
    with pytest.raises(E, match="soft_skel_step_fwd: null pointer"):
        L.call(fwd, p, 1, 2, 2, 2, 3, 0, None, big, None)
    with pytest.raises(E, match="soft_skel_step_fwd: bad extents"):
        L.call(fwd, p, 1, 2, 0, 2, 3, 0, p, big, None)
    with pytest.raises(E, match="soft_skel_step_fwd: more than 2\\^31 - 1 voxels"):
        L.call(fwd, p, 1 << 20, 1 << 10, 2, 1, 3, 0, p, big, None)
    for iters in (0, 33):
        with pytest.raises(E, match=f"soft_skel_step_fwd: iters must be in 1..32, got {iters}"):
            L.call(fwd, p, 1, 2, 2, 2, iters, 0, p, big, None)
    for j in (-1, 4):
        with pytest.raises(E, match=f"soft_skel_step_fwd: level j must be in 0..iters = 3, got {j}"):
            L.call(fwd, p, 1, 2, 2, 2, 3, j, p, big, None)
    with pytest.raises(E, match="workspace too small: need 2048 bytes, have 2047"):
        L.call(fwd, p, 1, 2, 2, 2, 3, 0, p, 2047, None)
    with pytest.raises(E, match="soft_skel_step_bwd: null pointer"):
        L.call(bwd, p, None, None, p + 256, None, 1, 2, 2, 2, 3, 0, p, big, None)
    with pytest.raises(E, match="soft_skel_step_bwd: null pointer"):
        L.call(bwd, p, p, None, p + 256, None, 1, 2, 2, 2, 3, 1, p, big, None)            # j > 0 needs g_skel_in
    with pytest.raises(E, match="soft_skel_step_bwd: an output aliases an input"):
        L.call(bwd, p, p, p + 256, p + 256, p + 512, 1, 2, 2, 2, 3, 1, p, big, None)
    with pytest.raises(E, match="soft_skel_step_bwd: iters must be in 1..32, got 40"):
        L.call(bwd, p, p, None, p + 256, p + 512, 1, 2, 2, 2, 40, 1, p, big, None)
    with pytest.raises(E, match="workspace too small"):
        L.call(bwd, p, p, None, p + 256, p + 512, 1, 2, 2, 2, 3, 1, p, 8, None)
    with pytest.raises(E, match="cldice_probs: null pointer"):
        L.call("mi355seg_cldice_probs_f32", p, None, 1, 2, 8, p, p, None)
    with pytest.raises(E, match="cldice_probs: bad extents"):
        L.call("mi355seg_cldice_probs_f32", p, p, 1, 0, 8, p, p, None)
    with pytest.raises(E, match="cldice_sums: null pointer"):
        L.call("mi355seg_cldice_sums_f32", p, p, None, p, 8, p, big, None)
    with pytest.raises(E, match="cldice_sums: bad extent"):
        L.call("mi355seg_cldice_sums_f32", p, p, p, p, 0, p, big, None)
    with pytest.raises(E, match="workspace too small: need 32 bytes, have 31"):
        L.call("mi355seg_cldice_sums_f32", p, p, p, p, 8, p, 31, None)
    with pytest.raises(E, match="cldice_finalize: null pointer"):
        L.call("mi355seg_cldice_finalize", p, big, 8, 1.0, None, p, p, None)
    with pytest.raises(E, match="cldice_finalize: smooth must be > 0, got 0"):
        L.call("mi355seg_cldice_finalize", p, big, 8, 0.0, p, p, p, None)
    with pytest.raises(E, match="workspace too small"):
        L.call("mi355seg_cldice_finalize", p, 8, 8, 1.0, p, p, p, None)
    with pytest.raises(E, match="cldice_bwd_head: null pointer"):
        L.call("mi355seg_cldice_bwd_head_f32", p, None, 8, p, None)
    with pytest.raises(E, match="cldice_bwd_head: bad extent"):
        L.call("mi355seg_cldice_bwd_head_f32", p, p, -3, p, None)
    with pytest.raises(E, match="cldice_bwd_tail: null pointer"):
        L.call("mi355seg_cldice_bwd_tail_f32", p, p, p, p, None, 1, 2, 8, p, None)
    with pytest.raises(E, match="cldice_bwd_tail: bad extents"):
        L.call("mi355seg_cldice_bwd_tail_f32", p, p, p, p, p, 1, 2, 0, p, None)
