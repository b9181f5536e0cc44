"""The compound losses (config.loss; csrc/loss_tail.hip), the parts that need no GPU: the C-ABI (symbols, prototypes, refusals that
never launch), train.parse_loss and LossSpec, and the fp64 restatement of DESIGN.md 4.16's table that tests/test_gpu_loss_tail.py
grades the kernels against -- checked here against the oracle's losses wherever a mode is composed of them."""
import ctypes

import pytest
import torch
import torch.nn.functional as TF

import mi355seg
from mi355seg._lib import HEADER, LIB_PATH, parse_header
from mi355seg.config import Config
from oracle import losses as OL

EPS = 1e-5
MODES = ("dice", "dice_bce", "ce", "dice_ce", "focal", "dice_focal", "tversky")
TERMS = {"dice": (None, "dice"), "dice_bce": ("bce", "dice"), "ce": ("ce", None), "dice_ce": ("ce", "dice"),
         "focal": ("focal", None), "dice_focal": ("focal", "dice"), "tversky": (None, "tversky")}
REFERENCE_MODES = ("dice", "dice_bce", "ce", "dice_ce")        # built from reference-defined terms only


# ----------------------------------------------------------------------------- the restatement (plain torch, any dtype, differentiable)
def ref_tail(x, t, mode, weights=(1.0, 1.0), gamma=2.0, alpha=0.3, beta=0.7):
    """(loss, voxel term, region term, sums [K, 5]) of the table in DESIGN.md 4.16 in x's dtype; an absent term is 0.
    M = N K S, V = N S, p = sigmoid(x), eps = 1e-5:
      bce      (1/M) sum max(x,0) - x t + log1p(exp(-|x|))
      focal    (1/M) sum q^gamma * bce_term,  q = p + t - 2 p t
      ce       (1/V) sum_v logsumexp_k x - x[argmax_k t]
      dice     1 - 2 (sum I + eps) / (sum P + sum T + eps), pooled over classes and samples
      tversky  1 - (1/K) sum_k (I_k + eps) / (I_k + alpha (P_k - I_k) + beta (T_k - I_k) + eps), per class over the batch"""
    voxel_term, region_term = TERMS[mode]
    N, K = x.shape[0], x.shape[1]
    xf, tf = x.reshape(N, K, -1), t.to(x.dtype).reshape(N, K, -1)
    p = torch.sigmoid(xf)
    zero = xf.sum() * 0
    voxel = region = zero
    if voxel_term in ("bce", "focal"):
        term = TF.binary_cross_entropy_with_logits(xf, tf, reduction="none")
        if voxel_term == "focal" and gamma != 0:
            term = (p + tf - 2 * p * tf) ** gamma * term
        voxel = term.sum() / xf.numel()
    elif voxel_term == "ce":
        label = tf.argmax(1, keepdim=True)
        voxel = (torch.logsumexp(xf, 1) - xf.gather(1, label).squeeze(1)).sum() / (xf.numel() // K)
    I, P, T = (p * tf).sum((0, 2)), p.sum((0, 2)), tf.sum((0, 2))
    if region_term == "dice":
        region = 1 - 2 * (I.sum() + EPS) / (P.sum() + T.sum() + EPS)
    elif region_term == "tversky":
        region = 1 - ((I + EPS) / (I + alpha * (P - I) + beta * (T - I) + EPS)).sum() / K
    sums = torch.stack([I, P, T, (p * p).sum((0, 2)), (tf * tf).sum((0, 2))], dim=1)
    wv, wr = weights
    return wv * voxel + wr * region, voxel, region, sums


def _case(shape, seed):
    g = torch.Generator().manual_seed(seed)
    N, K = shape[:2]
    x = torch.randn(shape, generator=g) * 3.0
    lab = torch.randint(0, K, (N,) + tuple(shape[2:]), generator=g)
    onehot = torch.stack([(lab == i) for i in range(K)], dim=1).float()
    soft = torch.rand(shape, generator=g)
    return x, lab, onehot, soft


@pytest.mark.parametrize("shape", [(2, 2, 3, 5, 7), (1, 4, 2, 3, 5), (3, 1, 1, 1, 7)], ids=lambda s: "x".join(map(str, s)))
def test_restatement_equals_the_oracle_where_a_mode_is_composed_of_it(shape):
    x, lab, onehot, soft = _case(shape, 7)
    x64 = x.double()
    K = shape[1]
    close = lambda a, b: abs(float(a) - float(b)) <= 1e-12 * max(1.0, abs(float(b)))
    for t in (onehot, soft):
        t64 = t.double()
        dice, bce = OL.dice_loss(x64, t64), OL.bce_with_logits(x64, t64)
        loss, v, r, sums = ref_tail(x64, t, "dice")
        assert close(loss, dice) and close(r, dice) and float(v) == 0.0
        loss, v, r, _ = ref_tail(x64, t, "dice_bce")
        assert close(loss, dice + bce) and close(v, bce) and close(r, dice)
        loss, v, r, _ = ref_tail(x64, t, "dice_bce", weights=(0.3, 2.0))
        assert close(loss, 0.3 * bce + 2.0 * dice)
        loss, v, _, _ = ref_tail(x64, t, "focal", gamma=0.0)
        assert close(loss, bce) and close(v, bce)
        assert float(ref_tail(x64, t, "focal", gamma=2.0)[0]) < float(bce)          # q <= 1 only ever shrinks a term
        if K >= 2:
            ce = OL.cross_entropy_3d(x64, t.argmax(1))
            loss, v, r, _ = ref_tail(x64, t, "ce")
            assert close(loss, ce) and close(v, ce) and float(r) == 0.0
            assert close(ref_tail(x64, t, "dice_ce")[0], ce + dice)
        p = torch.sigmoid(x64)
        want = torch.stack([(p * t64).sum((0, 2, 3, 4)), p.sum((0, 2, 3, 4)), t64.sum((0, 2, 3, 4)),
                            (p * p).sum((0, 2, 3, 4)), (t64 * t64).sum((0, 2, 3, 4))], 1)
        assert torch.allclose(sums, want, rtol=1e-13, atol=0)
    if K >= 2:
        assert close(ref_tail(x64, onehot, "ce")[0], OL.cross_entropy_3d(x64, lab))


def test_restatement_tversky_and_focal_closed_forms():
    """alpha = beta = 0.5 is the per-class soft Dice (I + eps) / ((P + T) / 2 + eps); the focal gradient equals the table's formula."""
    x, _, onehot, soft = _case((2, 3, 3, 4, 5), 11)
    x64 = x.double()
    p = torch.sigmoid(x64)
    I, P, T = (p * onehot).sum((0, 2, 3, 4)), p.sum((0, 2, 3, 4)), onehot.double().sum((0, 2, 3, 4))
    want = 1 - ((I + EPS) / (0.5 * (P + T) + EPS)).mean()
    assert abs(float(ref_tail(x64, onehot, "tversky", alpha=0.5, beta=0.5)[0]) - float(want)) <= 1e-13
    for gamma in (1.0, 2.0, 3.5):
        xr = x64.clone().requires_grad_(True)
        ref_tail(xr, soft, "focal", gamma=gamma)[0].backward()
        t = soft.double()
        q, bce = p + t - 2 * p * t, TF.binary_cross_entropy_with_logits(x64, t, reduction="none")
        g = (gamma * q ** (gamma - 1) * (1 - 2 * t) * p * (1 - p) * bce + q ** gamma * (p - t)) / x64.numel()
        assert float((xr.grad - g).abs().max()) <= 1e-15


# ----------------------------------------------------------------------------- C-ABI
NAMES = ("mi355seg_loss_tail_ws_bytes", "mi355seg_loss_tail_fwd_f32", "mi355seg_loss_tail_bwd_f32")


def test_abi_symbols_are_declared_and_exported():
    protos = parse_header(HEADER)
    cdll = ctypes.CDLL(LIB_PATH)
    for n in NAMES:
        assert n in protos and hasattr(cdll, n), n
    assert protos[NAMES[0]] == ("size_t", [("long long", "N"), ("int", "K"), ("long long", "S")])
    assert [name for _, name in protos[NAMES[1]][1]] == ["logits", "target", "N", "K", "S", "voxel_term", "region_term", "gamma", "alpha", "beta",
                                                         "w_voxel", "w_region", "loss", "terms", "sums", "mask", "counts", "coef",
                                                         "ws", "ws_bytes", "stream"]
    args = dict((name, t) for t, name in protos[NAMES[1]][1])
    assert args["logits"] == "const float*" and args["loss"] == "float*" and args["terms"] == "double*" and args["sums"] == "double*"
    assert args["mask"] == "int64_t*" and args["counts"] == "int64_t*" and args["coef"] == "double*" and args["gamma"] == "float"
    assert [name for _, name in protos[NAMES[2]][1]] == ["logits", "target", "coef", "gscale", "N", "K", "S", "voxel_term", "region_term", "gamma",
                                                         "dlogits", "stream"]
    args = dict((name, t) for t, name in protos[NAMES[2]][1])
    assert args["coef"] == "const double*" and args["gscale"] == "const float*" and args["dlogits"] == "float*"


def test_workspace_size():
    L = mi355seg.lib()
    q = lambda *a: L.query("mi355seg_loss_tail_ws_bytes", *a)
    for bad in ((0, 2, 8), (2, 0, 8), (2, 17, 8), (2, 2, 0), (-1, 2, 8), (2, -2, 8), (2, 2, -8)):
        assert q(*bad) == 0, bad
    assert q(1, 2, 1) == (1 + 5 * 2 + 4) * 8                                   # one block: 1 + 5 K partial sums and four counters
    assert q(2, 16, 128 ** 3) == 2048 * (1 + 5 * 16 + 4) * 8                    # the grid cap
    assert q(1, 1, 257) == 2 * (1 + 5 + 4) * 8


def test_bad_arguments_return_error_codes_and_never_launch():
    """Every refusal of include/mi355seg.h, with host addresses or null pointers in place of the tensors: a call that got past its
    argument checks would fault, not raise."""
    L = mi355seg.lib()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)

    def fwd(K=2, voxel=1, region=1, gamma=2.0, alpha=0.3, beta=0.7, wv=1.0, wr=1.0, ptr=a, ws=a, ws_bytes=1 << 20, N=1, S=8, **nulls):
        p = {n: (None if nulls.get(n) else ptr) for n in ("logits", "target", "loss", "terms", "sums", "mask", "counts", "coef")}
        L.call("mi355seg_loss_tail_fwd_f32", p["logits"], p["target"], N, K, S, voxel, region, gamma, alpha, beta, wv, wr,
               p["loss"], p["terms"], p["sums"], p["mask"], p["counts"], p["coef"], ws, ws_bytes, None)

    def bwd(K=2, voxel=1, region=1, gamma=2.0, N=1, S=8, **nulls):
        p = {n: (None if nulls.get(n) else a) for n in ("logits", "target", "coef", "gscale", "dlogits")}
        L.call("mi355seg_loss_tail_bwd_f32", p["logits"], p["target"], p["coef"], p["gscale"], N, K, S, voxel, region, gamma, p["dlogits"], None)

    E = mi355seg.Mi355SegError
    for call, name in ((fwd, "loss_tail_fwd"), (bwd, "loss_tail_bwd")):
        for K in (0, 17, -3):
            with pytest.raises(E, match=f"{name}: K must be in 1..16, got {K}"):
                call(K=K)
        for voxel in (-1, 4):
            with pytest.raises(E, match=f"{name}: unknown voxel term {voxel}"):
                call(voxel=voxel)
        for region in (-1, 3):
            with pytest.raises(E, match=f"{name}: unknown region term {region}"):
                call(region=region)
        with pytest.raises(E, match=f"{name}: both terms absent"):
            call(voxel=0, region=0)
        with pytest.raises(E, match=f"{name}: the ce term needs K >= 2"):
            call(K=1, voxel=3)
        for gamma in (0.5, -1.0, 8.5, float("nan")):
            with pytest.raises(E, match=f"{name}: gamma must be 0 or in"):
                call(voxel=2, gamma=gamma)
        for kw in ({"N": 0}, {"S": 0}, {"S": -4}):
            with pytest.raises(E, match=f"{name}: bad extents"):
                call(**kw)
    for kw in ({"alpha": -0.1}, {"beta": -1.0}, {"alpha": float("nan")}):
        with pytest.raises(E, match="alpha and beta must be >= 0"):
            fwd(region=2, **kw)
    with pytest.raises(E, match="alpha \\+ beta > 0"):
        fwd(region=2, alpha=0.0, beta=0.0)
    for kw in ({"wv": -1.0}, {"wr": -0.5}, {"wr": float("nan")}):
        with pytest.raises(E, match="weights must be >= 0"):
            fwd(**kw)
    for n in ("logits", "target", "loss", "terms", "sums", "mask", "counts", "coef"):
        with pytest.raises(E, match="loss_tail_fwd: null pointer"):
            fwd(**{n: True})
    with pytest.raises(E, match="loss_tail_fwd: null pointer"):
        fwd(ws=None)
    for n in ("logits", "target", "coef", "gscale", "dlogits"):
        with pytest.raises(E, match="loss_tail_bwd: null pointer"):
            bwd(**{n: True})
    need = L.query("mi355seg_loss_tail_ws_bytes", 1, 2, 8)
    for have in (0, need - 1):
        with pytest.raises(E, match=f"workspace too small: need {need} bytes, have {have}"):
            fwd(ws_bytes=have)


def test_functional_refuses_cpu_tensors_and_bad_specs():
    F = mi355seg.functional
    assert F.LOSS_MODES == MODES
    spec = F.LossSpec.from_mode("dice_bce")
    assert spec == F.LossSpec("bce", "dice", 2.0, 0.3, 0.7, 1.0, 1.0)
    with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):
        F.loss_tail(torch.zeros((1, 2, 4, 4, 4)), torch.zeros((1, 2, 4, 4, 4)), spec)
    with pytest.raises(TypeError, match="LossSpec"):
        F.loss_tail(torch.zeros((1, 2, 4, 4, 4)), torch.zeros((1, 2, 4, 4, 4)), "dice_bce")
    for kw in ({"weights": (1,)}, {"weights": (1, 2, 3)}, {"weights": (-1, 1)}, {"focal_gamma": 0.5}, {"focal_gamma": 9},
               {"tversky_alpha": -0.1}):
        with pytest.raises(ValueError):
            F.LossSpec.from_mode("dice_focal", **kw)
    with pytest.raises(ValueError, match="alpha"):
        F.LossSpec.from_mode("tversky", tversky_alpha=0, tversky_beta=0)
    with pytest.raises(ValueError, match="loss mode"):
        F.LossSpec.from_mode("bce")
    with pytest.raises(ValueError, match="voxel term or a region term"):
        F.LossSpec(None, None, 2.0, 0.3, 0.7, 1.0, 1.0).checked()


def test_compound_loss_is_a_criterion_with_a_tail():
    from mi355seg.utils.loss_function import CompoundLoss
    F = mi355seg.functional
    for mode in MODES:
        c = CompoundLoss(mode)
        assert isinstance(c, torch.nn.Module) and callable(c.tail) and (c.spec.voxel, c.spec.region) == TERMS[mode]
        assert c.spec == F.LossSpec.from_mode(mode)
    c = CompoundLoss("tversky", weights=(0, 2), tversky_alpha=0.0, tversky_beta=1.0)
    assert c.spec == F.LossSpec(None, "tversky", 2.0, 0.0, 1.0, 0.0, 2.0)
    with pytest.raises(ValueError):
        CompoundLoss("dice+bce")


# ----------------------------------------------------------------------------- train.parse_loss
def test_parse_loss_absent_empty_or_bce_is_todays_path():
    from mi355seg.train import parse_loss
    for cfg in ({}, {"loss": None}, {"loss": ""}, {"loss": "None"}, {"loss": "bce"}):
        assert parse_loss(Config(cfg)) is None


def test_parse_loss_modes_and_keys():
    from mi355seg.train import parse_loss
    from mi355seg.utils.loss_function import CompoundLoss
    S = mi355seg.functional.LossSpec
    for mode in MODES:
        c = parse_loss(Config({"loss": mode}))
        assert isinstance(c, CompoundLoss) and c.mode == mode and c.spec == S(*TERMS[mode], 2.0, 0.3, 0.7, 1.0, 1.0)
    assert parse_loss(Config({"loss": "dice_bce", "loss_weights": "0.3,2.0"})).spec == S("bce", "dice", 2.0, 0.3, 0.7, 0.3, 2.0)
    assert parse_loss(Config({"loss": "dice_ce", "loss_weights": (1, 0)})).spec == S("ce", "dice", 2.0, 0.3, 0.7, 1.0, 0.0)
    assert parse_loss(Config({"loss": "dice_ce", "loss_weights": "1, 0.5"})).spec.w_region == 0.5
    assert parse_loss(Config({"loss": "focal", "focal_gamma": 3})).spec == S("focal", None, 3.0, 0.3, 0.7, 1.0, 1.0)
    assert parse_loss(Config({"loss": "dice_focal", "focal_gamma": "1.5"})).spec.gamma == 1.5
    assert parse_loss(Config({"loss": "dice_focal", "focal_gamma": 0})).spec.gamma == 0.0
    assert parse_loss(Config({"loss": "tversky", "tversky_alpha": 0.5, "tversky_beta": 0.5})).spec == S(None, "tversky", 2.0, 0.5, 0.5, 1.0, 1.0)
    assert parse_loss(Config({"loss": "tversky", "tversky_alpha": 0})).spec.alpha == 0.0            # beta keeps its default 0.7
    assert parse_loss(Config({"loss": "tversky", "tversky_beta": 0})).spec.beta == 0.0


BAD_CONFIGS = [
    ("loss", {"loss": "dice+bce"}), ("loss", {"loss": "Dice"}), ("loss", {"loss": 3}), ("loss", {"loss": ["dice"]}),
    ("loss_weights", {"loss": "dice_bce", "loss_weights": "1"}), ("loss_weights", {"loss": "dice_bce", "loss_weights": 1.0}),
    ("loss_weights", {"loss": "dice_bce", "loss_weights": "1,2,3"}), ("loss_weights", {"loss": "dice_bce", "loss_weights": "-1,2"}),
    ("loss_weights", {"loss": "dice_bce", "loss_weights": "1,-0.5"}), ("loss_weights", {"loss": "dice_bce", "loss_weights": "a,b"}),
    ("loss_weights", {"loss": "dice_bce", "loss_weights": "1,,2"}), ("loss_weights", {"loss": "bce", "loss_weights": "1,1"}),
    ("loss_weights", {"loss_weights": "1,1"}),
    ("focal_gamma", {"loss": "focal", "focal_gamma": 0.5}), ("focal_gamma", {"loss": "focal", "focal_gamma": 9}),
    ("focal_gamma", {"loss": "focal", "focal_gamma": -1}), ("focal_gamma", {"loss": "focal", "focal_gamma": "two"}),
    ("focal_gamma", {"loss": "focal", "focal_gamma": True}), ("focal_gamma", {"loss": "dice_bce", "focal_gamma": 2}),
    ("focal_gamma", {"focal_gamma": 2}),
    ("tversky_alpha", {"loss": "tversky", "tversky_alpha": -0.1}), ("tversky_beta", {"loss": "tversky", "tversky_beta": "x"}),
    ("tversky_alpha", {"loss": "tversky", "tversky_alpha": 0, "tversky_beta": 0}),
    ("tversky_alpha", {"loss": "dice", "tversky_alpha": 0.3}), ("tversky_beta", {"loss": "dice_focal", "tversky_beta": 0.7}),
    ("tversky_alpha", {"tversky_alpha": 0.3}),
]


@pytest.mark.parametrize("key,cfg", BAD_CONFIGS, ids=[f"{k}-{i}" for i, (k, _) in enumerate(BAD_CONFIGS)])
def test_parse_loss_refuses_bad_values_naming_the_key(key, cfg):
    from mi355seg.train import parse_loss
    with pytest.raises(ValueError, match=f"config.{key}") as e:
        parse_loss(Config(cfg))
    assert repr(cfg[key]) in str(e.value)
    if key == "loss":
        assert all(m in str(e.value) for m in ("bce",) + MODES)              # lists what is allowed
