"""The boundary loss term without a GPU: the fp64 references that tests/test_gpu_boundary.py grades the kernels against (``ref_sdm``
from scipy's distance_transform_edt with the rules of DESIGN.md 4.21, ``ref_boundary`` in torch fp64 with autograd), ``ref_sdm``
itself checked against a brute-force all-pairs computation; ``cpu32_sdm``, the float32 restatement of the kernels' three passes
that sets the anisotropic bound; train.parse_loss's three keys, the ramp, CompoundLoss's two arguments and ``term_names``."""
import numpy as np
import pytest
import torch
from scipy.ndimage import distance_transform_edt

import mi355seg
from mi355seg.config import Config


def _c0(K):
    return 1 if K > 1 else 0


def ref_sdm(target, spacing=(1, 1, 1)):
    """phi [N, K - c0, D, H, W] in numpy fp64 of a one-hot target [N, K, D, H, W] (numpy or torch).  scipy returns meaningless values
    when its input has no zero (an all-ones mask), so the phi = 0 rule for an empty opposite set is applied here, not left to it."""
    t = np.asarray(target, dtype=np.float64)
    N, K = t.shape[:2]
    c0 = _c0(K)
    offset = float(min(spacing))
    phi = np.zeros((N, K - c0) + t.shape[2:], dtype=np.float64)
    for n in range(N):
        for k in range(c0, K):
            pos = t[n, k] > 0.5
            if not pos.any() or pos.all():
                continue                                                        # the opposite set is empty: phi = 0
            outside = distance_transform_edt(~pos, sampling=spacing)            # distance to the nearest member
            inside = distance_transform_edt(pos, sampling=spacing)              # distance to the nearest non-member
            phi[n, k - c0] = np.where(pos, -(inside - offset), outside)
    return phi


def brute_sdm(target, spacing):
    """the same map from all pairs of voxels, fp64"""
    t = np.asarray(target, dtype=np.float64)
    N, K = t.shape[:2]
    c0 = _c0(K)
    D, H, W = t.shape[2:]
    zz, yy, xx = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    pts = np.stack([zz.ravel() * spacing[0], yy.ravel() * spacing[1], xx.ravel() * spacing[2]], axis=1).astype(np.float64)
    d = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    phi = np.zeros((N, K - c0, D, H, W))
    for n in range(N):
        for k in range(c0, K):
            pos = (t[n, k] > 0.5).ravel()
            if not pos.any() or pos.all():
                continue
            to_pos, to_neg = d[:, pos].min(1), d[:, ~pos].min(1)
            phi[n, k - c0] = np.where(pos, -(to_neg - min(spacing)), to_pos).reshape(D, H, W)
    return phi


def cpu32_sdm(target, spacing):
    """The three passes of csrc/boundary.hip restated in numpy float32: integer offsets along W, then the min-plus step along H and
    along D with every product, difference and sum rounded to float32, float32 sqrt, sign and offset.  Not the kernel's bits (it
    fuses d * d + f and compensates sqrt(a) - offset): what plain float32 arithmetic costs on this input, which sets the
    anisotropic bound."""
    t = np.asarray(target)
    N, K = t.shape[:2]
    c0 = _c0(K)
    D, H, W = t.shape[2:]
    f32 = np.float32
    sz, sy, sx = (f32(v) for v in spacing)
    offset = f32(min(spacing))

    def minplus(f, axis, s):
        n = f.shape[axis]
        pos = (s * np.arange(n, dtype=f32)).astype(f32)
        f = np.moveaxis(f, axis, 0)
        out = np.full_like(f, np.inf)
        for i in range(n):
            d = (pos[i] - pos).astype(f32)
            d2 = (d * d).astype(f32).reshape((n,) + (1,) * (f.ndim - 1))
            out[i] = (f + d2).astype(f32).min(0)
        return np.moveaxis(out, 0, axis)

    phi = np.zeros((N, K - c0, D, H, W), dtype=f32)
    xs = np.arange(W)
    for n in range(N):
        for k in range(c0, K):
            pos = t[n, k] > 0.5
            sq = []
            for sites in (pos, ~pos):
                dist = np.where(sites[..., None, :], np.abs(xs[:, None] - xs[None, :]), 1 << 20).min(-1)       # [D, H, W] offsets
                d = (sx * dist.astype(f32)).astype(f32)
                f = np.where(dist >= (1 << 20), f32(np.inf), (d * d).astype(f32)).astype(f32)
                sq.append(minplus(minplus(f, 1, sy), 0, sz))
            with np.errstate(invalid="ignore"):
                outside, inside = np.sqrt(sq[0]).astype(f32), np.sqrt(sq[1]).astype(f32)
                val = np.where(pos, -(inside - offset), outside).astype(f32)
            phi[n, k - c0] = np.where(np.isinf(np.where(pos, sq[1], sq[0])), f32(0), val)
    return phi


def ref_boundary(logits, target, spacing=(1, 1, 1)):
    """mean(sigmoid(logits[:, c0:]) * phi) in the dtype of ``logits`` (fp64 for the reference), with autograd"""
    c0 = _c0(logits.shape[1])
    phi = torch.from_numpy(ref_sdm(target.detach().cpu().numpy(), spacing)).to(logits.dtype)
    return (torch.sigmoid(logits[:, c0:]) * phi).mean()


def boundary_masks(shape, seed):
    """name -> exact 0/1 one-hot float32 target [N, K, D, H, W] (K = 1: a single mask channel): three densities, one voxel in a corner,
    a full plane, and absent / full / normal classes side by side in one batch"""
    N, K, D, H, W = shape
    g = torch.Generator().manual_seed(seed)
    vol = (D, H, W)

    def one_hot(fg):
        """fg: [N, D, H, W] labels in 0..K-1 (K > 1) or a 0/1 mask (K = 1)"""
        if K == 1:
            return (fg > 0).float().unsqueeze(1)
        return torch.stack([(fg == i) for i in range(K)], dim=1).float()

    def labels(density):
        on = torch.rand((N,) + vol, generator=g) < density
        cls = torch.randint(1, max(K, 2), (N,) + vol, generator=g)
        return torch.where(on, cls, torch.zeros_like(cls))

    out = {f"density {d}": one_hot(labels(d)) for d in (0.05, 0.5, 0.95)}
    corner = torch.zeros((N,) + vol, dtype=torch.long)
    corner[:, D - 1, H - 1, W - 1] = max(K - 1, 1)
    out["corner voxel"] = one_hot(corner)
    plane = torch.zeros((N,) + vol, dtype=torch.long)
    plane[:, D // 2] = 1
    out["full plane"] = one_hot(plane)
    mixed = labels(0.5)
    mixed[0] = 0                                         # every class absent from sample 0
    if N > 1:
        mixed[1] = 1                                     # class 1 fills sample 1 (the others are absent there)
    out["absent and full"] = one_hot(mixed)
    return out


# ----------------------------------------------------------------------------- ref_sdm against all pairs
@pytest.mark.parametrize("spacing", [(1, 1, 1), (2.5, 0.7, 0.7), (1, 1, 3)], ids=str)
@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1), (1, 2, 1, 1, 5), (2, 2, 3, 5, 7), (3, 3, 5, 6, 7)], ids=lambda s: "x".join(map(str, s)))
def test_ref_sdm_equals_the_all_pairs_map(shape, spacing):
    for name, t in boundary_masks(shape, 3).items():
        a, b = ref_sdm(t.numpy(), spacing), brute_sdm(t.numpy(), spacing)
        assert a.shape == b.shape == (shape[0], shape[1] - _c0(shape[1])) + shape[2:]
        assert np.abs(a - b).max() <= 1e-12, name


def test_ref_sdm_special_cases():
    """an absent class and a full class give 0 everywhere (scipy alone does not), a single voxel gives the distance to it and
    -(d - offset) = 0 at the voxel, and the sign is never wrong at a spacing below 1"""
    t = torch.zeros(3, 1, 5, 6, 7)
    t[1] = 1.0
    t[2, 0, 2, 3, 4] = 1.0
    for spacing in ((1, 1, 1), (2.5, 0.7, 0.7)):
        phi = ref_sdm(t.numpy(), spacing)
        assert not phi[0].any() and not phi[1].any()
        assert np.abs(phi - brute_sdm(t.numpy(), spacing)).max() <= 1e-12
        assert abs(phi[2, 0, 2, 3, 4]) < 1e-12 and phi[2, 0, 0, 3, 4] == 2 * spacing[0] and abs(phi[2, 0, 2, 3, 6] - 2 * spacing[2]) < 1e-12
    # scipy on an all-ones input: the values are not a distance to anything (no zero exists), hence the guard in ref_sdm
    assert distance_transform_edt(np.ones((3, 3, 3))).max() > 0
    blob = torch.zeros(1, 1, 6, 7, 8)
    blob[0, 0, 1:5, 1:6, 1:7] = 1.0
    phi = ref_sdm(blob.numpy(), (0.7, 0.7, 0.7))
    assert (phi[blob.numpy() > 0.5] <= 0).all() and (phi[blob.numpy() < 0.5] > 0).all()
    assert abs(phi[0, 0, 1, 1, 1]) < 1e-12 and abs(phi[0, 0, 2, 2, 2] + 0.7) < 1e-12          # official "- 1" would give +0.3 and -0.4


@pytest.mark.parametrize("spacing", [(1, 1, 1), (2.5, 0.7, 0.7), (1, 1, 3)], ids=str)
def test_cpu32_restatement_follows_the_reference(spacing):
    """float32 through the same three passes: exact squares at unit spacing (outside the class the correctly rounded distance, inside
    it the rounding of sqrt before the offset is subtracted), within a few float32 roundings of the fp64 map at anisotropic spacing"""
    for name, t in boundary_masks((2, 3, 4, 9, 11), 5).items():
        ref, c32 = ref_sdm(t.numpy(), spacing), cpu32_sdm(t.numpy(), spacing)
        assert c32.dtype == np.float32 and c32.shape == ref.shape
        if spacing == (1, 1, 1):
            out = t.numpy()[:, 1:] < 0.5
            assert np.array_equal(c32[out], ref.astype(np.float32)[out]), name
            assert np.abs(c32 - ref).max() <= 0.5 * np.finfo(np.float32).eps * (np.abs(ref).max() + 1), name
        else:
            assert np.abs(c32 - ref).max() <= 8 * np.finfo(np.float32).eps * max(1.0, np.abs(ref).max()), name


def test_ref_boundary_value_and_gradient():
    t = boundary_masks((2, 3, 3, 5, 7), 9)["density 0.5"]
    x = torch.randn(t.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    loss = ref_boundary(x, t, (1, 1, 1))
    loss.backward()
    phi = torch.from_numpy(ref_sdm(t.numpy()))
    p = torch.sigmoid(x.detach()[:, 1:])
    assert abs(loss.item() - float((p * phi).sum() / phi.numel())) < 1e-15
    assert not bool(x.grad[:, 0].any())
    assert float((x.grad[:, 1:] - phi * p * (1 - p) / phi.numel()).abs().max()) < 1e-15
    # a confident, correct prediction has a negative term; the same confidence on the complement has a positive one
    blob = torch.zeros(1, 1, 6, 7, 8)
    blob[0, 0, 1:5, 1:6, 1:7] = 1.0
    sure = (blob.double() * 2 - 1) * 20
    assert float(ref_boundary(sure, blob)) < 0 < float(ref_boundary(-sure, blob))


# ----------------------------------------------------------------------------- train.parse_loss
def test_parse_loss_boundary_keys_and_defaults():
    from mi355seg.train import LOSS_KEYS, parse_loss
    assert {"boundary_weight", "boundary_spacing", "boundary_ramp_epochs"} <= set(LOSS_KEYS)
    c = parse_loss(Config({"loss": "dice_bce"}))
    assert (c.boundary_weight, c.boundary_spacing, c.boundary_ramp_epochs) == (0.0, (1.0, 1.0, 1.0), 0)
    c = parse_loss(Config({"loss": "dice_bce", "boundary_weight": 0.5}))
    assert (c.boundary_weight, c.boundary_spacing, c.boundary_ramp_epochs) == (0.5, (1.0, 1.0, 1.0), 0)
    c = parse_loss(Config({"loss": "dice_ce", "boundary_weight": "0.25", "boundary_spacing": "2.5,0.7,0.7", "boundary_ramp_epochs": "10"}))
    assert (c.boundary_weight, c.boundary_spacing, c.boundary_ramp_epochs) == (0.25, (2.5, 0.7, 0.7), 10)
    c = parse_loss(Config({"loss": "tversky", "boundary_weight": 0, "boundary_spacing": (1, 1, 3), "boundary_ramp_epochs": 0}))
    assert (c.boundary_weight, c.boundary_spacing, c.boundary_ramp_epochs) == (0.0, (1.0, 1.0, 3.0), 0)


def test_parse_loss_boundary_spacing_falls_back_to_resample_spacing():
    from mi355seg.train import parse_loss
    c = parse_loss(Config({"loss": "dice_bce", "boundary_weight": 0.5, "resample_spacing": "2,1,1"}))
    assert c.boundary_spacing == (2.0, 1.0, 1.0)
    c = parse_loss(Config({"loss": "dice_bce", "boundary_weight": 0.5, "resample_spacing": "2,1,1", "boundary_spacing": "3,3,3"}))
    assert c.boundary_spacing == (3.0, 3.0, 3.0)                       # the key of its own wins
    c = parse_loss(Config({"loss": "dice_bce", "boundary_weight": 0.5}))
    assert c.boundary_spacing == (1.0, 1.0, 1.0)


@pytest.mark.parametrize("loss", [None, "bce"])
@pytest.mark.parametrize("key,value", [("boundary_weight", 0.5), ("boundary_spacing", "1,1,1"), ("boundary_ramp_epochs", 2)])
def test_parse_loss_refuses_boundary_keys_without_a_compound_loss(loss, key, value):
    from mi355seg.train import parse_loss
    with pytest.raises(ValueError, match=f"config.{key} must be given only with config.loss = a compound mode") as e:
        parse_loss(Config({"loss": loss, key: value}))
    assert "config.loss=bce" in str(e.value)


@pytest.mark.parametrize("key,value", [("boundary_weight", -0.1), ("boundary_weight", "half"), ("boundary_weight", True),
                                       ("boundary_spacing", "1,1"), ("boundary_spacing", (1, 1)), ("boundary_spacing", "1,0,1"),
                                       ("boundary_spacing", "1,-2,1"), ("boundary_spacing", "a,b,c"), ("boundary_spacing", 2.0),
                                       ("boundary_ramp_epochs", 2.5), ("boundary_ramp_epochs", "2.5"), ("boundary_ramp_epochs", -1),
                                       ("boundary_ramp_epochs", "-3"), ("boundary_ramp_epochs", True)])
def test_parse_loss_refuses_bad_boundary_values_naming_the_key(key, value):
    from mi355seg.train import parse_loss
    with pytest.raises(ValueError, match=f"config.{key} must be") as e:
        parse_loss(Config({"loss": "dice_bce", "boundary_weight": 0.5, key: value}))
    assert repr(value) in str(e.value)


def test_ramp_values():
    from mi355seg.train import boundary_ramp
    w = 0.5
    assert [boundary_ramp(w, e, 0) for e in range(1, 7)] == [w] * 6
    assert [boundary_ramp(w, e, 1) for e in range(1, 7)] == [w] * 6
    assert [boundary_ramp(w, e, 4) for e in range(1, 7)] == [w * 0.25, w * 0.5, w * 0.75, w, w, w]


# ----------------------------------------------------------------------------- CompoundLoss
def test_compound_loss_boundary_arguments_term_names_and_repr():
    from mi355seg.utils.loss_function import CompoundLoss
    plain, zero = CompoundLoss("dice_bce"), CompoundLoss("dice_bce", boundary_weight=0.0, boundary_spacing=(2, 1, 1))
    assert zero.spec == plain.spec == mi355seg.functional.LossSpec("bce", "dice", 2.0, 0.3, 0.7, 1.0, 1.0)
    assert repr(zero) == repr(plain) and "boundary" not in repr(plain)
    assert repr(plain) == "CompoundLoss(mode='dice_bce', spec=('bce', 'dice', 2.0, 0.3, 0.7, 1.0, 1.0))"
    assert not hasattr(zero, "boundary_scale") and not list(zero.state_dict())
    c = CompoundLoss("dice_bce", boundary_weight=0.5, boundary_spacing=(2.5, 0.7, 0.7))
    assert c.spec == plain.spec and "boundary=(weight=0.5, spacing=(2.5, 0.7, 0.7))" in repr(c)
    assert c.boundary_scale.dtype == torch.float32 and c.boundary_scale.tolist() == [0.5] and not list(c.state_dict())
    c.set_boundary_scale(0.125)
    assert c.boundary_scale.tolist() == [0.125] and c.boundary_weight == 0.5
    assert plain.term_names == ("voxel", "region")
    assert CompoundLoss("dice_bce", cldice_weight=0.5).term_names == ("voxel", "region", "cldice")
    assert c.term_names == ("voxel", "region", "boundary")
    assert CompoundLoss("dice_bce", cldice_weight=0.5, boundary_weight=0.5).term_names == ("voxel", "region", "cldice", "boundary")
    for kw in ({"boundary_weight": -1}, {"boundary_weight": "1"}, {"boundary_weight": True}, {"boundary_weight": float("inf")},
               {"boundary_spacing": (1, 1)}, {"boundary_spacing": (1, 0, 1)}, {"boundary_spacing": 1.0}, {"boundary_spacing": "1,1,1"},
               {"boundary_spacing": (1, -1, 1)}, {"boundary_spacing": None}):
        with pytest.raises(ValueError, match="boundary_"):
            CompoundLoss("dice_bce", **kw)
    with pytest.raises(ValueError, match="no boundary term"):
        plain.set_boundary_scale(0.5)
    for v in (-0.5, "1", None, True):
        with pytest.raises(ValueError, match="set_boundary_scale: expected a number >= 0"):
            c.set_boundary_scale(v)


def test_functional_refuses_cpu_tensors_and_bad_spacings():
    F = mi355seg.functional
    x = torch.zeros(1, 2, 3, 4, 5)
    with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):
        F.signed_distance_map(x)
    with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):
        F.boundary_loss(x, x)
    with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):
        F.boundary_loss_full(x, x, (1, 1, 1))
    from mi355seg.utils.loss_function import CompoundLoss
    with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):
        CompoundLoss("dice_bce", boundary_weight=0.5)(x, x)
    for spacing in ((1, 1), (1, 0, 1), (1, 1, -1), 1.0, "1,1,1", (1, 1, float("inf")), (1, True, 1)):
        with pytest.raises(ValueError, match="spacing must be three positive numbers"):
            F.signed_distance_map(x, spacing)
        with pytest.raises(ValueError, match="spacing must be three positive numbers"):
            F.boundary_loss(x, x, spacing)
