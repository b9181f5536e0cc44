"""Multi-class training and grading on the device (config.multiclass).

The label form of the fused tail (mi355seg_loss_tail_*_lab_f32: a uint8 label map in place of the float one-hot target) is graded
against the one-hot form WITHOUT a tolerance: for labels in [0, K) every shared output -- loss, terms, sums, mask, counts, coef,
dlogits -- has the one-hot form's bits on one_hot_labels(labels), through the C-ABI with garbage in the workspace.  On finite
logits that is torch.equal; with NaN and +-inf logit columns (the NaN-first argmax rule) the outputs hold NaNs, which torch.equal
calls unequal to themselves, so there the NaNs must stand in the same places and everything else must have the same BIT PATTERN
(_same_bits).  The class counters (the new output) are compared with a numpy
confusion matrix, exactly.  Then the layers above: train_step / GraphedTrainStep, the unchanged default step, train.py and
predict.py."""
import csv
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_hd95_fixture import brute_hd95, close

pytestmark = pytest.mark.gpu

MODES = ("dice", "dice_bce", "ce", "dice_ce", "focal", "dice_focal", "tversky")
CLASSES = (1, 2, 3, 4, 5, 8, 9, 16)          # the capacities 1..4 (16-byte path where S % 4 == 0), 8 and 16, full and partly filled
VEC_SHAPE, ODD_SHAPE = (2, 8, 12, 16), (2, 7, 9, 11)
BIG_SHAPE = (1, 130, 128, 128)               # K = 3: 2,129,920 voxels > 2,048 * 256 * 4, the grid-stride loop's second trip
UP = 1.7                                     # the upstream factor of every backward
F64, F32, I64, U8 = torch.float64, torch.float32, torch.int64, torch.uint8


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mi355seg
    mi355seg.lib()          # raises if the HIP library is missing -- no fallback
    return mi355seg


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _case(K, shape, seed, special=False, out_of_range=False):
    """logits [N,K,...] = 4 * randn (with ``special``: a few voxels whose class column holds NaN, +inf or -inf entries) and uint8
    labels [N,...] in [0, K) (with ``out_of_range``: a few 255s), on the device."""
    g = _gen(seed)
    N = shape[0]
    x = 4.0 * torch.randn((N, K) + tuple(shape[1:]), generator=g)
    lab = torch.randint(0, K, shape, generator=g).to(U8)
    if special:
        xf = x.view(N, K, -1)
        S = xf.shape[2]
        for i, v in enumerate((float("nan"), float("inf"), float("-inf"), float("nan"), float("inf"))):
            s = (i * 97 + 5) % S
            xf[i % N, (i * 3) % K, s] = v                       # one special entry in the column
            if K > 1:
                xf[(i + 1) % N, :, (s + 11) % S] = v            # the whole column
                xf[i % N, K - 1, (s + 23) % S] = float("nan")   # a NaN behind a number: the first NaN wins, not the first maximum
                xf[i % N, 0, (s + 23) % S] = float("inf") if i % 2 else 1.0
    if out_of_range:
        lab.view(-1)[::37] = 255
    return x.cuda(), lab.cuda()


def _bits(t):
    return t.contiguous().view({F32: torch.int32, F64: torch.int64}.get(t.dtype, t.dtype))


def _same_bits(a, b):
    """NaNs in the same places, and the same bit patterns everywhere else (+0 and -0 are told apart, as are the infinities).  A
    NaN's own sign and payload are not compared: IEEE 754 leaves them open, and they follow from which instruction forms the
    compiler chose around the NaN (measured: the loss of a NaN logit came out as 0x7fc00000 from one form and 0xffc00000 from the
    other)."""
    if not a.is_floating_point():
        return torch.equal(a, b)
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(_bits(torch.where(na, torch.zeros_like(a), a)), _bits(torch.where(nb, torch.zeros_like(b), b)))


def _spec_args(seg, mode):
    F = seg.functional
    spec = F.LossSpec.from_mode(mode)
    return spec, (F.LOSS_VOXEL_TERMS[spec.voxel], F.LOSS_REGION_TERMS[spec.region], spec.gamma)


def _raw(seg, x, target, mode, labels_form):
    """Forward and backward through the C-ABI with a workspace full of 0xff: {loss, terms, sums, mask, counts, coef, dlogits} and,
    for the label form, class_counts."""
    L, p = seg.lib(), (lambda t: t.data_ptr())
    spec, args = _spec_args(seg, mode)
    N, K = x.shape[:2]
    S = x[0, 0].numel()
    dev = x.device
    o = {"loss": torch.empty((), dtype=F32, device=dev), "terms": torch.empty(2, dtype=F64, device=dev),
         "sums": torch.empty((K, 5), dtype=F64, device=dev), "mask": torch.empty((N, 1) + tuple(x.shape[2:]), dtype=I64, device=dev),
         "counts": torch.empty(4, dtype=I64, device=dev), "coef": torch.full((1 + 2 * K,), -7.0, dtype=F64, device=dev),
         "dlogits": torch.empty_like(x)}
    g = torch.full((1,), UP, dtype=F32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    name = "mi355seg_loss_tail_lab_ws_bytes" if labels_form else "mi355seg_loss_tail_ws_bytes"
    ws = torch.full((L.query(name, N, K, S),), 255, dtype=U8, device=dev)
    head = (p(x), p(target), N, K, S, *args, spec.alpha, spec.beta, spec.w_voxel, spec.w_region,
            p(o["loss"]), p(o["terms"]), p(o["sums"]), p(o["mask"]), p(o["counts"]), p(o["coef"]))
    if labels_form:
        o["class_counts"] = torch.empty((K, 3), dtype=I64, device=dev)
        L.call("mi355seg_loss_tail_fwd_lab_f32", *head, p(o["class_counts"]), p(ws), ws.numel(), stream)
        L.call("mi355seg_loss_tail_bwd_lab_f32", p(x), p(target), p(o["coef"]), p(g), N, K, S, *args, p(o["dlogits"]), stream)
    else:
        L.call("mi355seg_loss_tail_fwd_f32", *head, p(ws), ws.numel(), stream)
        L.call("mi355seg_loss_tail_bwd_f32", p(x), p(target), p(o["coef"]), p(g), N, K, S, *args, p(o["dlogits"]), stream)
    return o


SHARED = ("loss", "terms", "sums", "mask", "counts", "coef", "dlogits")


def _confusion(lab, mask, K):
    """numpy: rows (tp_k, pred_k, gt_k); a label >= K belongs to no class."""
    lab, mask = lab.cpu().numpy().reshape(-1).astype(np.int64), mask.cpu().numpy().reshape(-1)
    return np.array([[np.sum((lab == k) & (mask == k)), np.sum(mask == k), np.sum(lab == k)] for k in range(K)], dtype=np.int64)


def _compare_forms(seg, K, shape, mode, seed, special, out_of_range=False):
    x, lab = _case(K, shape, seed, special, out_of_range)
    onehot = seg.functional.one_hot_labels(lab, K)
    a, b = _raw(seg, x, lab, mode, True), _raw(seg, x, onehot, mode, False)
    torch.cuda.synchronize()
    for name in SHARED:
        assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape, name
        if special:
            assert _same_bits(a[name], b[name]), (name, mode, K, shape)
        else:
            assert torch.equal(a[name], b[name]), (name, mode, K, shape)
    assert np.array_equal(a["class_counts"].cpu().numpy(), _confusion(lab, a["mask"], K)), (mode, K, shape)
    return a


@pytest.mark.parametrize("K", CLASSES)
@pytest.mark.parametrize("mode", MODES)
def test_label_form_has_the_bits_of_the_one_hot_form(seg, mode, K):
    """Every config.loss mode, K in {1 (not ce), 2, 3, 4, 5, 8, 9, 16}, on [2,K,8,12,16] (S % 4 == 0: the 16-byte path for K <= 4)
    and [2,K,7,9,11] (S odd: the scalar path), on finite logits (torch.equal) and on logits with NaN and +-inf columns (bits)."""
    if mode in ("ce", "dice_ce") and K == 1:
        with pytest.raises(seg.Mi355SegError, match="the ce term needs K >= 2"):      # refused, as the one-hot form refuses it
            _raw(seg, *_case(1, ODD_SHAPE, 1), mode, True)
        return
    for shape in (VEC_SHAPE, ODD_SHAPE):
        for special in (False, True):
            a = _compare_forms(seg, K, shape, mode, 100 * K + len(mode), special)
            if not special:
                assert bool(torch.isfinite(a["loss"])) and bool(torch.isfinite(a["dlogits"]).all())


@pytest.mark.parametrize("mode", MODES)
def test_label_form_past_the_grid_cap(seg, mode):
    """[1,3,130,128,128]: the smallest shape above 2,048 x 256 x 4 voxels -- every block writes a partial and the first threads
    make a second trip."""
    _compare_forms(seg, 3, BIG_SHAPE, mode, 9, special=True)


@pytest.mark.parametrize("K", [2, 3, 4, 8, 16])
def test_labels_of_255_are_the_all_zero_column(seg, K):
    """Labels >= K: members of no class (no gt_k counts them), gt.argmax = 0, and the comparison with the one-hot form still holds,
    its column being all zero there."""
    for shape in (VEC_SHAPE, ODD_SHAPE):
        for mode in ("dice_ce", "dice_focal", "tversky"):
            a = _compare_forms(seg, K, shape, mode, 7 * K, special=False, out_of_range=True)
        lab = _case(K, shape, 7 * K, out_of_range=True)[1]
        n255 = int((lab == 255).sum())
        assert n255 > 0 and int(a["class_counts"][:, 2].sum()) == lab.numel() - n255
        assert int(a["class_counts"][:, 1].sum()) == lab.numel()                  # every voxel is predicted as some class


def test_class_counts_with_a_class_that_never_occurs(seg):
    """From the tail and from mi355seg_class_counts_i64, against numpy: class 2 of 5 occurs in no label, class 4 wins no argmax."""
    F = seg.functional
    K = 5
    for shape in (VEC_SHAPE, ODD_SHAPE, (1, 40, 64, 80)):
        x, lab = _case(K, shape, 3)
        lab[lab == 2] = 3
        x[:, 4] = -50.0
        lab.view(-1)[::41] = 255
        out = F.loss_tail_labels(x, lab, F.LossSpec.from_mode("dice_ce"))
        mask, cc = out[1], out[4]
        want = _confusion(lab, mask, K)
        assert cc.dtype == I64 and tuple(cc.shape) == (K, 3) and np.array_equal(cc.cpu().numpy(), want)
        assert want[2, 2] == 0 and want[2, 0] == 0 and want[4, 1] == 0 and want[4, 2] > 0
        gt = lab.to(I64)                                         # (255 stays 255: outside [0, K) in an int64 volume too)
        got = F.class_counts(gt, mask, K)
        assert got.dtype == I64 and np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(F.class_counts(gt.reshape(-1), mask.reshape(-1), 16).cpu().numpy()[:K], want)
        assert int(F.class_counts(gt, mask, 16)[K:].sum()) == 0
        neg = gt.clone()
        neg.view(-1)[::5] = -3                                   # negative labels belong to no class either
        assert np.array_equal(F.class_counts(neg, mask, K).cpu().numpy()[:, 2],
                              np.array([np.sum(neg.cpu().numpy() == k) for k in range(K)]))
    from mi355seg.utils.metric import class_metrics_from_counts
    m = class_metrics_from_counts(cc)
    assert m["dice"][2] == 0.0 and 0.0 <= m["mean_dice"] <= 1.0


def test_functional_label_tail_equals_the_one_hot_tail_and_differentiates(seg):
    F = seg.functional
    x, lab = _case(4, VEC_SHAPE, 21)
    spec = F.LossSpec.from_mode("dice_focal", weights=(0.3, 2.0), focal_gamma=3.0)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    la, ma, ca, ta, cc = F.loss_tail_labels(xa, lab, spec)
    lb, mb, cb, tb = F.loss_tail(xb, F.one_hot_labels(lab, 4), spec)
    (la * UP).backward()
    (lb * UP).backward()
    assert torch.equal(la, lb) and torch.equal(ma, mb) and torch.equal(ca, cb) and torch.equal(ta, tb) and torch.equal(xa.grad, xb.grad)
    assert not cc.requires_grad and la.requires_grad
    with pytest.raises(ValueError, match="Label size"):
        F.loss_tail_labels(x, lab[:, :-1], spec)
    with pytest.raises(seg.Mi355SegError, match="labels must be uint8"):
        F.loss_tail_labels(x, lab.to(I64), spec)


# ----------------------------------------------------------------------------- recorded bits (tests/golden/loss_tail_pins.json)
def _pin(t):
    """SHA-256 of a tensor's bytes, every NaN written as the one quiet NaN first: NaN positions are pinned, a NaN's sign is not (the
    freedom _same_bits documents)"""
    a = t.detach().cpu().contiguous().numpy().reshape(-1)
    if a.dtype.kind == "f":
        nan = np.isnan(a)
        a = a.view({4: np.uint32, 8: np.uint64}[a.itemsize]).copy()
        a[nan] = {4: 0x7FC00000, 8: 0x7FF8000000000000}[a.itemsize]
    return hashlib.sha256(a.tobytes()).hexdigest()


def _pin_inputs(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _sid(shape):
    return "x".join(str(v) for v in shape)


def loss_tail_pin_digests(F):
    """case -> {"input", and one entry per output}: SHA-256 of the input bytes and of each output's bytes, of every kernel family of
    csrc/loss_tail.hip through the C-ABI (_raw: the workspace full of 0xff): {loss, terms, sums, mask, counts, coef, dlogits} of
    both forms (class_counts too for the label form) for every mode x K x {16-byte path, scalar path, scalar path with NaN and +-inf
    columns}, labels of 255, the grid-stride loop's second trip, and the conversion and counting kernels."""
    import mi355seg as seg
    out = {}

    def tail(K, shape, mode, seed, tag="", **kw):
        x, lab = _case(K, shape, seed, **kw)
        for form, target in (("labels", lab), ("onehot", F.one_hot_labels(lab, K))):
            o = _raw(seg, x, target, mode, form == "labels")
            out[f"tail {form} {mode} K{K} {_sid(shape)}{tag}"] = {"input": _pin_inputs(x, target), **{k: _pin(v) for k, v in o.items()}}

    for mode in MODES:
        for K in CLASSES:
            if mode in ("ce", "dice_ce") and K == 1:
                continue                                         # (refused)
            seed = 100 * K + len(mode)
            tail(K, VEC_SHAPE, mode, seed)
            tail(K, ODD_SHAPE, mode, seed)
            tail(K, ODD_SHAPE, mode, seed, " special", special=True)
    for K in (2, 4, 8, 16):
        for shape in (VEC_SHAPE, ODD_SHAPE):
            tail(K, shape, "dice_ce", 7 * K, " out_of_range", out_of_range=True)
    for mode in ("dice_ce", "dice_focal"):
        tail(3, BIG_SHAPE, mode, 9)
    for shape in ((2, 1, 8, 12, 16), (3, 1, 1, 1, 1031)):         # labels_u8 and one_hot_labels: valid labels, and values that are none
        gt = torch.randint(0, 4, shape, generator=_gen(sum(shape))).float()
        flat = gt.view(-1)
        for i, v in enumerate((0.5, -1.0, 4.0, float("nan"), float("inf"), 3.0001, -0.25, 255.0, 1e9, float("-inf"))):
            flat[(i * 13 + 40) % flat.numel()] = v
        lab, bad = F.labels_u8(gt.cuda(), 4)
        out[f"convert {_sid(shape)}"] = {"input": _pin_inputs(gt), "labels": _pin(lab), "bad": _pin(bad),
                                         "one_hot_4": _pin(F.one_hot_labels(lab, 4)), "one_hot_16": _pin(F.one_hot_labels(lab, 16))}
    g = _gen(4)
    gt, pr = torch.randint(-1, 17, (600001,), generator=g), torch.randint(0, 16, (600001,), generator=g)      # several blocks, a second trip
    for K in (4, 8, 16):
        out[f"class_counts K{K} 600001"] = {"input": _pin_inputs(gt, pr), "class_counts": _pin(F.class_counts(gt.cuda(), pr.cuda(), K))}
    torch.cuda.synchronize()
    return out


def test_loss_tail_bits_are_the_parents(seg):
    """tests/golden/loss_tail_pins.json (tests/golden/make_loss_tail_pins.py): every output of loss_tail.hip's kernels on the cases of
    loss_tail_pin_digests, recorded on the MI355X before the one-hot and the label form came to be two instantiations of one text --
    also the bits against which the modes that the unfused criterions pin only to a tolerance could move in both forms alike."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_tail_pins.json")) as fh:
        want = json.load(fh)["loss_tail"]
    got = loss_tail_pin_digests(seg.functional)
    assert sorted(got) == sorted(want), f"the cases changed: {sorted(set(got) ^ set(want))}"
    for name in sorted(got):
        assert got[name]["input"] == want[name]["input"], f"{name}: torch drew other inputs (the recorded digests are of other bytes)"
    bad = [(name, k) for name in sorted(got) for k in sorted(set(got[name]) | set(want[name])) if got[name].get(k) != want[name].get(k)]
    assert not bad, f"{len(bad)} outputs differ from the recorded bits: {bad[:12]}"


# ----------------------------------------------------------------------------- conversion kernels
@pytest.mark.parametrize("shape", [(2, 1, 8, 12, 16), (2, 1, 7, 9, 11), (1, 1, 1, 1, 1), (3, 1, 1, 1, 1031)], ids=lambda s: "x".join(map(str, s)))
def test_labels_u8_and_one_hot_against_numpy(seg, shape):
    F = seg.functional
    g = _gen(sum(shape))
    for K in (1, 2, 4, 16):
        gt = torch.randint(0, K, shape, generator=g).float()
        lab, bad = F.labels_u8(gt.cuda(), K)
        assert lab.dtype == U8 and tuple(lab.shape) == (shape[0],) + shape[2:] and bad.dtype == I64 and bad.tolist() == [0]
        assert np.array_equal(lab.cpu().numpy(), gt.numpy()[:, 0].astype(np.uint8))
        oh = F.one_hot_labels(lab, K)
        want = np.stack([(gt.numpy()[:, 0] == k) for k in range(K)], axis=1).astype(np.float32)
        assert oh.dtype == F32 and np.array_equal(oh.cpu().numpy(), want)
    # values that are no label: non-integers, negatives, >= K, NaN, inf -> 255, counted; the counter accumulates over calls
    K = 4
    gt = torch.randint(0, K, shape, generator=g).float()
    flat = gt.view(-1)
    wrong = [0.5, -1.0, 4.0, float("nan"), float("inf"), 3.0001, -0.25, 255.0, 1e9, float("-inf")]
    idx = [(i * 13) % flat.numel() for i in range(len(wrong))]
    for i, v in zip(idx, wrong):
        flat[i] = v
    n_bad = len(set(idx))
    want = gt.numpy().reshape(-1).copy()
    ok = np.isfinite(want) & (want >= 0) & (want < K) & (want == np.trunc(np.nan_to_num(want)))
    want_u8 = np.where(ok, np.nan_to_num(want, posinf=0, neginf=0), 255).astype(np.uint8)
    lab, bad = F.labels_u8(gt.cuda(), K)
    assert int((~ok).sum()) == n_bad and bad.tolist() == [n_bad]
    assert np.array_equal(lab.cpu().numpy().reshape(-1), want_u8)
    _, bad2 = F.labels_u8(gt.cuda(), K, bad)
    assert bad2 is bad and bad.tolist() == [2 * n_bad]
    oh = F.one_hot_labels(lab, K).cpu().numpy()
    assert np.array_equal(oh.reshape(shape[0], K, -1).sum(1).reshape(-1), ok.astype(np.float32))      # a 255 is an all-zero column
    assert np.array_equal(F.one_hot_labels(lab, 2).cpu().numpy().reshape(shape[0], 2, -1)[:, 1].reshape(-1), (want_u8 == 1).astype(np.float32))


def test_every_class_count_beyond_one_block(seg):
    """class_counts over 3 * 2^20 voxels (more than one block, several trips) at K = 16 and K = 3, against numpy."""
    F = seg.functional
    g = _gen(4)
    gt, pr = torch.randint(0, 16, (3, 1 << 20), generator=g), torch.randint(0, 16, (3, 1 << 20), generator=g)
    for K in (16, 3):
        want = np.array([[int(((gt == k) & (pr == k)).sum()), int((pr == k).sum()), int((gt == k).sum())] for k in range(K)])
        assert np.array_equal(F.class_counts(gt.cuda(), pr.cuda(), K).cpu().numpy(), want)


def test_refusals_on_the_device(seg):
    """The refusals that need device tensors: a misaligned view where the 16-byte path would be taken is served through a copy by
    functional (aligned_contiguous) and refused by the C entry point itself; K = 17; mismatched sizes."""
    F, L = seg.functional, seg.lib()
    x, lab = _case(3, VEC_SHAPE, 2)
    spec, args = _spec_args(seg, "dice_ce")
    flat = torch.empty(x.numel() + 1, device="cuda")
    flat[1:] = x.view(-1)
    xm = flat[1:].view(x.shape)
    assert xm.data_ptr() % 16 != 0
    a, b = F.loss_tail_labels(xm, lab, spec), F.loss_tail_labels(x, lab, spec)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    o = _raw(seg, x, lab, "dice_ce", True)
    p = lambda t: t.data_ptr()
    N, K, S = 2, 3, x[0, 0].numel()
    ws = torch.empty(L.query("mi355seg_loss_tail_lab_ws_bytes", N, K, S), dtype=U8, device="cuda")
    with pytest.raises(seg.Mi355SegError, match="with S % 4 == 0 and K <= 4"):
        L.call("mi355seg_loss_tail_fwd_lab_f32", p(xm), p(lab), N, K, S, *args, spec.alpha, spec.beta, 1.0, 1.0, p(o["loss"]), p(o["terms"]),
               p(o["sums"]), p(o["mask"]), p(o["counts"]), p(o["coef"]), p(o["class_counts"]), p(ws), ws.numel(), None)
    with pytest.raises(seg.Mi355SegError, match="with S % 4 == 0 and K <= 4"):
        L.call("mi355seg_loss_tail_bwd_lab_f32", p(x), p(lab) + 1, p(o["coef"]), p(o["coef"]), N, K, S, *args, p(o["dlogits"]), None)
    x17 = torch.zeros((1, 17, 2, 3, 4), device="cuda")
    with pytest.raises(seg.Mi355SegError, match="K must be in 1..16, got 17"):
        F.loss_tail_labels(x17, torch.zeros((1, 2, 3, 4), dtype=U8, device="cuda"), spec)
    for fn in (lambda: F.labels_u8(x17[:, :1], 17), lambda: F.one_hot_labels(lab, 0), lambda: F.class_counts(lab, lab, 17)):
        with pytest.raises(ValueError, match="K must be an integer in 1..16"):
            fn()
    with pytest.raises(ValueError, match="same number of voxels"):
        F.class_counts(lab.to(I64), lab.to(I64)[:1], 3)
    with pytest.raises(seg.Mi355SegError, match=r"expected \[N,1,...\]"):
        F.labels_u8(x, 3)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- CompoundLoss.tail_labels
def test_tail_labels_builds_the_one_hot_only_for_the_terms_that_need_it(seg, monkeypatch):
    from mi355seg.utils.loss_function import CompoundLoss
    F = seg.functional
    x, lab = _case(3, (2, 8, 8, 16), 5)
    calls = []
    real = F.one_hot_labels
    monkeypatch.setattr(F, "one_hot_labels", lambda *a: (calls.append(a[1]), real(*a))[1])
    plain = CompoundLoss("dice_ce")
    loss, mask, counts, terms, cc = plain.tail_labels(x, lab)
    assert calls == [] and tuple(terms.shape) == (2,) and tuple(cc.shape) == (3, 3)
    onehot = real(lab, 3)
    for crit in (CompoundLoss("dice_ce", cldice_weight=0.5), CompoundLoss("dice_ce", boundary_weight=0.5),
                 CompoundLoss("dice_ce", cldice_weight=0.5, boundary_weight=0.25)):
        calls.clear()
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        a = crit.tail_labels(xa, lab)
        assert calls == [3]                                      # once
        b = crit.tail(xb, onehot)
        a[0].backward()
        b[0].backward()
        assert all(torch.equal(u, v) for u, v in zip(a[:4], b)) and torch.equal(a[4], cc) and torch.equal(xa.grad, xb.grad)
        assert len(a[3]) == len(crit.term_names)


# ----------------------------------------------------------------------------- engine
class _OneHotInTheLabelPathsPlace:
    """criterion.tail(pred, one_hot) where train_step calls criterion.tail_labels(pred, labels)."""

    def __init__(self, criterion, seg):
        self.criterion, self.F = criterion, seg.functional

    def tail_labels(self, pred, labels):
        K = pred.shape[1]
        return self.criterion.tail(pred, self.F.one_hot_labels(labels, K)) + (torch.zeros((K, 3), dtype=I64, device=pred.device),)


def _unet3(classes=3):
    from mi355seg.models.three_d.unet3d import UNet3D
    from oracle.fill import fill_module_
    return fill_module_(UNet3D(1, classes, 8)).cuda().train()


def _volume_and_labels(classes=3):
    from oracle.fill import make_input
    x = make_input((2, 1, 32, 32, 32)).cuda()
    gt = torch.randint(0, classes, (2, 1, 32, 32, 32), generator=_gen(17)).float().cuda()
    return x, gt


def test_train_step_equals_the_one_hot_tail_for_three_steps(seg):
    """UNet3D(1, 3, 8) on [2,1,32^3], labels 0..2, dice_ce: after three steps every parameter (and buffer) is torch.equal to the same
    three steps taken with criterion.tail(pred, one_hot) in the label path's place; the class counters are the confusion counts of
    the returned mask, stay on the device, and the label-range counter stays 0."""
    from mi355seg.engine import train_step
    from mi355seg.utils.loss_function import CompoundLoss
    from mi355seg.utils.metric import class_metrics_from_counts
    x, gt = _volume_and_labels()
    ma, mb = _unet3(), _unet3()
    oa, ob = torch.optim.Adam(ma.parameters(), lr=1e-3), torch.optim.Adam(mb.parameters(), lr=1e-3)
    ca, cb = CompoundLoss("dice_ce"), _OneHotInTheLabelPathsPlace(CompoundLoss("dice_ce"), seg)
    bad = torch.zeros(1, dtype=I64, device="cuda")
    for step in range(3):
        a = train_step(ma, oa, x, gt, criterion=ca, sync_metric=False, multiclass=3, label_bad=bad)
        b = train_step(mb, ob, x, gt, criterion=cb, sync_metric=False, multiclass=3)
        assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["mask"], b["mask"]) and torch.equal(a["counts"], b["counts"]), step
        assert torch.equal(a["loss_terms"], b["loss_terms"]) and torch.equal(a["pred"], b["pred"])
        assert a["class_counts"].is_cuda and a["label_bad"] is bad and "dice" not in a
        assert np.array_equal(a["class_counts"].cpu().numpy(), _confusion(gt.to(U8), a["mask"], 3))
    for (k, p), (_, q) in zip(ma.state_dict().items(), mb.state_dict().items()):
        assert torch.equal(p, q), k
    assert bad.tolist() == [0]
    out = train_step(ma, oa, x, gt, criterion=ca, multiclass=3)                     # sync_metric: the floats of the class counters
    m = class_metrics_from_counts(out["class_counts"])
    assert out["dice"] == m["mean_dice"] and out["jaccard"] == m["mean_jaccard"] and out["class_dice"] == m["dice"] and len(m["dice"]) == 3
    # labels outside 0..2 are counted on the device, not read in the step
    gt_bad = gt.clone()
    gt_bad.view(-1)[:5] = torch.tensor([3.0, -1.0, 0.5, 7.0, float("nan")], device="cuda")
    out = train_step(ma, oa, x, gt_bad, criterion=ca, sync_metric=False, multiclass=3, label_bad=bad)
    assert bad.tolist() == [5] and int(out["class_counts"][:, 2].sum()) == gt.numel() - 5


_GRAPHED = r"""
import sys, torch
sys.path.insert(0, %r)
import mi355seg
from mi355seg.engine import GraphedTrainStep, train_step
from mi355seg.models.three_d.unet3d import UNet3D
from mi355seg.utils.loss_function import CompoundLoss
from oracle.fill import fill_module_, make_input
x = make_input((2, 1, 32, 32, 32)).cuda()
gt = torch.randint(0, 3, (2, 1, 32, 32, 32), generator=torch.Generator().manual_seed(17)).float().cuda()

def build():
    m = fill_module_(UNet3D(1, 3, 8)).cuda().train()
    return m, torch.optim.Adam(m.parameters(), lr=1e-3, capturable=True), CompoundLoss("dice_ce")

m0, o0, c0 = build()
for _ in range(4):
    e = train_step(m0, o0, x, gt, criterion=c0, sync_metric=False, multiclass=3)
l0, t0, k0 = e["loss"].item(), e["loss_terms"].tolist(), e["class_counts"].tolist()
m1, o1, c1 = build()
g = GraphedTrainStep(m1, o1, x, gt, criterion=c1, warmup=1, multiclass=3)
assert "class_counts" in g.first and g.label_bad.tolist() == [0]
for _ in range(3):
    r = g(x, gt, sync_metric=False)
l1, t1, k1 = r["loss"].item(), r["loss_terms"].tolist(), r["class_counts"].tolist()
torch.cuda.synchronize()
assert l0 == l1 and t0 == t1 and k0 == k1, (l0, l1, t0, t1, k0, k1)
assert r["class_counts"].is_cuda and g.label_bad.tolist() == [0]
for (k, a), (_, b) in zip(m0.state_dict().items(), m1.state_dict().items()):
    assert torch.equal(a, b), k
d = g(x, gt)
assert 0.0 <= d["dice"] <= 1.0 and len(d["class_dice"]) == 3
print("GRAPHED_MULTICLASS_OK", l1)
"""


def test_graphed_step_equals_the_eager_steps(seg):
    """Four eager steps with multiclass=3 and a capturable Adam against GraphedTrainStep(..., warmup=1, multiclass=3) plus three
    replays: the last loss, its terms, the class counters and every state-dict entry bitwise equal.  Run once, in a process of its
    own, with a timeout (as tests/test_gpu_loss_tail.py's graphed test)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _GRAPHED % root], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "GRAPHED_MULTICLASS_OK" in p.stdout, (p.returncode, p.stdout[-1000:], p.stderr[-3000:])


def _launches(L):
    buf = (ctypes.c_double * 32)()
    L.call("mi355seg_prof_read", buf, 32)
    nmax = 16384
    rec, n = (ctypes.c_double * (4 * nmax))(), ctypes.c_int(0)
    L.call("mi355seg_prof_records", rec, nmax, ctypes.byref(n))
    L.call("mi355seg_prof_enable", 0)
    return [(int(rec[4 * r]), rec[4 * r + 2], rec[4 * r + 3]) for r in range(n.value)]


def test_two_classes_equal_the_two_channel_step_and_the_default_step_is_unchanged(seg):
    """At K = 2 the label path and today's two-channel step (the same CompoundLoss, the same seed) give equal loss bits and equal
    Dice for three steps.  The default step's launch record holds the one-hot tail's launches ((8 K + 8) N S bytes forward, 12 K N S
    backward) and none of the label path's; the label path's record differs from it in exactly those: labels_u8 (5 N S bytes) in
    two_channel_gt's place and the label tail's pair ((4 K + 9) N S, (8 K + 1) N S)."""
    from mi355seg.engine import train_step
    from mi355seg.utils.loss_function import CompoundLoss
    L = seg.lib()
    x, gt = _volume_and_labels(2)
    ma, mb = _unet3(2), _unet3(2)
    oa, ob = torch.optim.Adam(ma.parameters(), lr=1e-3), torch.optim.Adam(mb.parameters(), lr=1e-3)
    ca, cb = CompoundLoss("dice_ce"), CompoundLoss("dice_ce")
    rec = {}
    for step in range(3):
        if step == 2:
            L.call("mi355seg_prof_reset")
            L.call("mi355seg_prof_enable", 1)
        a = train_step(ma, oa, x, gt, criterion=ca)
        if step == 2:
            rec["default"] = _launches(L)
            L.call("mi355seg_prof_reset")
            L.call("mi355seg_prof_enable", 1)
        b = train_step(mb, ob, x, gt, criterion=cb, multiclass=2)
        if step == 2:
            rec["labels"] = _launches(L)
        assert torch.equal(a["loss"], b["loss"]) and a["dice"] == b["dice"] and a["jaccard"] == b["jaccard"], step
        assert torch.equal(a["mask"], b["mask"]) and torch.equal(a["counts"], b["counts"]) and "class_counts" not in a
    for (k, p), (_, q) in zip(ma.state_dict().items(), mb.state_dict().items()):
        assert torch.equal(p, q), k
    NS, K, LOSS = float(gt.numel()), 2, 6                        # (family 6: the loss kernels, csrc/common.h)
    ours = {"default": [12 * NS, (8 * K + 8) * NS, 12 * K * NS],          # two_channel_gt, the one-hot tail forward, its backward
            "labels": [5 * NS, (4 * K + 9) * NS, (8 * K + 1) * NS]}       # labels_u8, the label tail forward, its backward
    picked = lambda r, vals: [e[2] for e in r if e[0] == LOSS and e[2] in vals]
    rest = lambda r, vals: [e for e in r if not (e[0] == LOSS and e[2] in vals)]
    for name, other in (("default", "labels"), ("labels", "default")):
        assert picked(rec[name], ours[name]) == ours[name], (name, picked(rec[name], ours[name]))
        assert picked(rec[name], ours[other]) == [], name
    assert rest(rec["default"], ours["default"]) == rest(rec["labels"], ours["labels"]) and len(rec["default"]) > 20


# ----------------------------------------------------------------------------- train.py and predict.py
@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    """three 48^3 volumes with labels 0..3 (nested blobs around a centre, so that every class has a surface) as .npy files"""
    root = tmp_path_factory.mktemp("multiclass")
    os.makedirs(root / "img"), os.makedirs(root / "gt")
    rng = np.random.default_rng(3)
    z, y, x = np.meshgrid(*(np.arange(48, dtype=np.float32),) * 3, indexing="ij")
    for i in range(3):
        lab = np.zeros((48, 48, 48), dtype=np.float32)
        for k, (c, r) in enumerate(((14 + 2 * i, 9), (30, 8 + i), (34 - i, 5)), start=1):
            lab[(z - c) ** 2 + (y - 24) ** 2 + (x - (12 * k)) ** 2 < r * r] = k
        img = (lab * 0.8 + rng.normal(0, 0.3, lab.shape)).astype(np.float32)
        np.save(root / "img" / f"case{i}.npy", img)
        np.save(root / "gt" / f"case{i}.npy", lab)
    return root


def _common(cohort, out):
    return ["config=unet", f"config.output_dir={out}", "config.patch_size=32,32,32", "config.batch_size=2", "config.out_classes=4",
            f"config.data_path={cohort / 'img'}", f"config.gt_path={cohort / 'gt'}", f"config.pred_data_path={cohort / 'img'}",
            f"config.pred_gt_path={cohort / 'gt'}", "config.multiclass=true"]


@pytest.fixture(scope="module")
def trained(seg, cohort, tmp_path_factory):
    from mi355seg.train import main as train_main
    out = tmp_path_factory.mktemp("multiclass_logs")
    torch.manual_seed(5)
    cfg, res = train_main(_common(cohort, out) + ["config.loss=dice_ce", "config.iters_per_epoch=3", "config.epochs=1"])
    return cfg, res


def test_train_cli_writes_the_per_class_dice(seg, trained, cohort, tmp_path):
    from mi355seg.train import main as train_main
    cfg, res = trained
    rows = [json.loads(l) for l in open(os.path.join(cfg.hydra_path, "scalars.jsonl")).read().strip().splitlines()]
    assert len(rows) == 3 and res["epoch"] == 1 and os.path.exists(os.path.join(cfg.hydra_path, "latest_checkpoint.pt"))
    for r in rows:
        per_class = [r[f"Training/dice_class_{k}"] for k in (1, 2, 3)]
        assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in per_class) and "Training/dice_class_0" not in r and "Training/dice_class_4" not in r
        assert np.isfinite(r["Training/Loss"]) and 0.0 <= r["Training/dice"] <= 1.0 and "Training/loss_voxel" in r
    with pytest.raises(ValueError, match="config.multiclass needs a compound config.loss"):
        train_main(_common(cohort, tmp_path / "bce"))
    with pytest.raises(ValueError, match="config.multiclass needs labelled volumes"):
        train_main(_common(cohort, tmp_path / "syn") + ["config.loss=dice_ce", "config.data_path=synthetic"])
    # a data set with a label the model has no class for: refused at the end of the epoch, with the count
    with pytest.raises(ValueError, match=r"config.multiclass: \d+ label voxels of epoch 1 are not integers in 0..2"):
        train_main(_common(cohort, tmp_path / "k3") + ["config.loss=dice_ce", "config.out_classes=3", "config.iters_per_epoch=2", "config.epochs=1"])


def _read_csv(path):
    with open(path, newline="") as fh:
        return list(csv.reader(fh))


def test_predict_cli_grades_every_class(seg, trained, cohort, tmp_path):
    """metrics.csv against numpy on the saved _pred.npy: the counts-based columns to 1e-12, hs95 (config.spacing=1,1,1) against the
    CPU oracle on the class masks at tests/test_gpu_hd95.py's tolerance (1e-9 relative); one run with overlap_mode=hann tta=mirror."""
    from mi355seg.predict import main as predict_main
    cfg, _ = trained
    base = _common(cohort, tmp_path / "logs") + [f"config.ckpt={os.path.join(cfg.hydra_path, 'latest_checkpoint.pt')}"]
    cfg_a, rows_a = predict_main(base + [f"config.hydra_path={tmp_path / 'plain'}"])
    cfg_b, rows_b = predict_main(base + [f"config.hydra_path={tmp_path / 'spaced'}", "config.spacing=1,1,1"])
    plain, spaced = _read_csv(os.path.join(cfg_a.hydra_path, "metrics.csv")), _read_csv(os.path.join(cfg_b.hydra_path, "metrics.csv"))
    assert plain[0] == ["file", "class", "jaccard", "dice"] and len(plain) == 1 + 9 + 3
    assert spaced[0] == ["file", "class", "precision", "recall", "jaccard", "dice", "hs95"] and len(spaced) == 1 + 9 + 3
    assert [(r[0], r[1]) for r in plain[1:]] == [(f"case{i}", str(k)) for i in range(3) for k in (1, 2, 3)] + [("mean", str(k)) for k in (1, 2, 3)]
    assert [(r[0], r[1]) for r in spaced[1:]] == [(r[0], r[1]) for r in plain[1:]]
    near = lambda got, want: abs(float(got) - want) <= 1e-12
    for i in range(3):
        gt = np.load(cohort / "gt" / f"case{i}.npy").astype(np.int64)
        pa = np.load(os.path.join(cfg_a.hydra_path, f"case{i}_pred.npy")).reshape(gt.shape)
        pb = np.load(os.path.join(cfg_b.hydra_path, f"case{i}_pred.npy")).reshape(gt.shape)
        assert np.array_equal(pa, pb) and set(np.unique(pa)) <= {0, 1, 2, 3}
        for k in (1, 2, 3):
            tp, ps, gs = float(np.sum((gt == k) & (pa == k))), float(np.sum(pa == k)), float(np.sum(gt == k))
            ra, rb = plain[1 + 3 * i + k - 1], spaced[1 + 3 * i + k - 1]
            assert near(ra[2], tp / (gs + ps - tp + 0.001)) and near(ra[3], 2 * tp / (gs + ps + 0.001))
            assert near(rb[2], tp / (ps + 0.001)) and near(rb[3], tp / (gs + 0.001)) and rb[4] == ra[2] and rb[5] == ra[3]
            want = float(brute_hd95(gt == k, pa == k, (1.0, 1.0, 1.0)))
            print(f"[multiclass] case{i} class {k}: dice {float(ra[3]):.4f} hs95 {float(rb[6])!r} oracle {want!r}")
            assert close(float(rb[6]), want, 1e-9) if np.isfinite(want) else not np.isfinite(float(rb[6]))
    for k in (1, 2, 3):
        assert near(plain[10 + k - 1][3], float(np.mean([float(plain[1 + 3 * i + k - 1][3]) for i in range(3)])))
    assert all(set(r) == {"file", "class", "jaccard", "dice"} for r in rows_a) and all("hs95" in r for r in rows_b)
    # blending and mirror TTA take K channels as they are
    cfg_c, rows_c = predict_main(base + [f"config.hydra_path={tmp_path / 'hann'}", "config.overlap_mode=hann", "config.tta=mirror"])
    assert len(rows_c) == 9
    for i in range(3):
        pc = np.load(os.path.join(cfg_c.hydra_path, f"case{i}_pred.npy"))
        assert pc.size == 48 ** 3 and set(np.unique(pc)) <= {0, 1, 2, 3}
    with pytest.raises(ValueError, match="config.multiclass does not go with config.keep_largest"):
        predict_main(base + [f"config.hydra_path={tmp_path / 'post'}", "config.keep_largest=1"])
