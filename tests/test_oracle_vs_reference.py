"""The oracle restatement (oracle/nets.py) against the reference modules on identical closed-form weights / inputs, through
the reference's outputs stored under tests/golden/ovr_<case>.npz (tests/golden/make_oracle_vs_reference.py): the state_dict
layout must be the reference's exactly (names in registration order, shapes); the forward output(s) and every parameter
gradient must match it (a seeded random sample element by element, and three whole-tensor float64 aggregates: sum g, sum |g|,
sum g * r for a fixed closed-form r).  Run side by side on one machine the two are bit-identical (the
names say so); stored values carry the thread count and vector unit of the machine that made them, so each tensor is compared
within a tolerance scaled to its OWN magnitude: elements within 1e-4 of the tensor's largest magnitude, aggregates within 1e-4
of its sum |g|, or 8x the reference's own spread of that quantity across ATen thread counts (recorded with the fixture) where
that is larger.  There is no absolute floor: the gradients of these networks span 13 orders of magnitude, and a zeroed, doubled
or negated gradient tensor fails however small it is, unless the reference's own value is rounding noise (a bias feeding a
normalisation, whose true gradient is zero, moves with the thread count as much as it is large)."""
import importlib.util
import os

import numpy as np
import torch

from conftest import GOLDEN
from oracle.fill import fill_module_, make_input
from oracle import nets

REL = 1e-4                 # of the tensor's own largest magnitude (elements) or of its sum |g| (aggregates)
SPREADS = 8.0              # times the reference's own thread-count spread of that tensor
OUT_SAMPLE = 1 << 16       # outputs larger than this are stored as a strided sample

# the fixture's own sampling and aggregates (sample_index, aggregates), from the script that writes it
_spec = importlib.util.spec_from_file_location("make_oracle_vs_reference", os.path.join(GOLDEN, "make_oracle_vs_reference.py"))
_GEN = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_GEN)


def _fixture(case):
    return np.load(os.path.join(GOLDEN, f"ovr_{case}.npz"))


def _strided(t, k):
    f = t.detach().reshape(-1)
    return f[::max(1, f.numel() // k)][:k]


def _same_keys(g, b):
    sd = b.state_dict()
    assert list(sd) == g["keys"].tolist()
    dims, off = g["shape_dims"].tolist(), 0
    for k, r in zip(g["keys"].tolist(), g["shape_rank"].tolist()):
        assert tuple(sd[k].shape) == tuple(dims[off:off + r]), k
        off += r


def _tol(ref, spread):
    return max(REL * float(np.abs(ref).max(initial=0.0)), SPREADS * float(spread))


def _close(got, ref, spread, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    err, tol = float(np.abs(got - ref).max(initial=0.0)), _tol(ref, spread)
    assert err <= tol, (what, err, tol)


def _check_grad(g, k, grad):
    """One parameter's gradient against the fixture: the sampled elements, then the three whole-tensor aggregates."""
    f = grad.detach().reshape(-1)
    tol = max(REL * float(g["gmax/" + k]), SPREADS * float(g["gspread/" + k]))
    err = float(np.abs(f.numpy()[_GEN.sample_index(f.numel())].astype(np.float64) - g["grad/" + k]).max())
    assert err <= tol, (k, "elements", err, tol)
    ref, spread = g["gagg/" + k], g["gaggspread/" + k]
    err, tol = np.abs(_GEN.aggregates(f) - ref), np.maximum(REL * ref[1], SPREADS * spread)
    assert (err <= tol).all(), (k, "sum g, sum |g|, sum g r", err.tolist(), tol.tolist())


def _check(g, outs, m):
    for i, o in enumerate(outs):
        got = o if o.numel() <= OUT_SAMPLE else _strided(o, OUT_SAMPLE)
        _close(got.numpy(), g[f"out{i}"], g["spread_out"], f"out{i}")
    no_grad = set(g["no_grad"].tolist()) - {""}
    for k, p in m.named_parameters():
        if k in no_grad:
            assert p.grad is None, k
            continue
        assert p.grad is not None, k
        _check_grad(g, k, p.grad)


def _fwd_bwd(m, x):
    y = m(x)
    y.square().mean().backward()
    return [y.detach()]


def test_unet3d_bit_identical():
    g = _fixture("unet3d")
    b = fill_module_(nets.UNet3D(1, 2, 8)).train()
    _same_keys(g, b)
    x = make_input((2, 1, 16, 16, 16))
    _check(g, _fwd_bwd(b, x), b)


def test_vnet_bit_identical():
    g = _fixture("vnet")
    b = fill_module_(nets.VNet(in_channels=1, classes=2)).train()
    _same_keys(g, b)
    x = make_input((2, 1, 16, 16, 16))
    torch.manual_seed(3)
    _check(g, _fwd_bwd(b, x), b)


def test_vnet_prelu_branch_bit_identical():
    """elu=False: nn.PReLU(nchan) in place of every ELU (vnet3d.py:14-18), incl. the state_dict keys of the slopes."""
    g = _fixture("vnet_prelu")
    b = fill_module_(nets.VNet(elu=False, in_channels=1, classes=2)).train()
    _same_keys(g, b)
    assert "down_tr64.relu2.weight" in b.state_dict() and b.state_dict()["up_tr128.relu1.weight"].shape == (64,)
    x = make_input((2, 1, 16, 16, 16))
    torch.manual_seed(3)
    _check(g, _fwd_bwd(b, x), b)


def test_resunet_bit_identical():
    """Kaiming-variance hash weights and a rough input at 64^3, where the deepest InstanceNorm still sees 4^3 voxels (at the
    sin-fill's 16 x 32 x 16 the reference's own gradients moved by up to ~90 with the thread count)."""
    from oracle.fill import RESUNET96_HEAD_SCALE, fill_module_hash_, make_input_rough
    g = _fixture("resunet")
    b = fill_module_hash_(nets.ResUNet(in_channels=4, n_classes=4, base_n_filter=4), RESUNET96_HEAD_SCALE).train()
    _same_keys(g, b)
    x = make_input_rough((1, 4, 64, 64, 64), seed=2.0)
    torch.manual_seed(5)
    _check(g, _fwd_bwd(b, x), b)


def test_unetr_bit_identical():
    g = _fixture("unetr")
    kw = dict(img_shape=(32, 32, 32), input_dim=1, output_dim=2, embed_dim=96, patch_size=16, num_heads=4, dropout=0.1)
    b = fill_module_(nets.UNETR(**kw)).train()
    _same_keys(g, b)
    x = make_input((2, 1, 32, 32, 32))
    torch.manual_seed(9)
    _check(g, _fwd_bwd(b, x), b)


def test_isnet_bit_identical_and_frequency_bands():
    """IS.py (three parameter sets, shared encoder) and the FFT band split of train.py:76-88: the reference's two filter
    functions, run as they stand on two inputs when the fixture was made, pin oracle.step.frequency_bands."""
    from oracle.step import frequency_bands
    g = _fixture("isnet")
    for tag, x in (("a", make_input((1, 1, 16, 16, 16), freq=0.37)),
                   ("b", make_input((2, 1, 8, 12, 16), freq=0.21))):       # batch 2: the all-axes forward transform quirk
        low, high = frequency_bands(x)
        _close(low.numpy(), g["band_low_" + tag], 0.0, "low_" + tag)
        _close(high.numpy(), g["band_high_" + tag], 0.0, "high_" + tag)

    b = fill_module_(nets.ISUNet3D(1, 2, 4)).train()
    _same_keys(g, b)                                                   # incl. registration order (optimizer state index)
    x = make_input((1, 1, 32, 32, 32), freq=0.37)                    # 32^3: the bottleneck still sees 2^3 voxels for BatchNorm
    low, high = frequency_bands(x)
    o1, o2 = b(x, low, high)
    (o1.square().mean() + 0.5 * o2.square().mean()).backward()
    assert set(g["no_grad"].tolist()) - {""}                           # the never-called suffixed encoders get no gradient
    _check(g, [o1.detach(), o2.detach()], b)
    for k, v in b.named_buffers():                                     # shared-encoder BN stats advanced three times
        _close(v.numpy(), g["buf/" + k], g["spread_out"], k)


def test_csrnet_bit_identical():
    g = _fixture("csrnet")
    b = fill_module_(nets.CSRNet(1, 2, 4)).train()
    _same_keys(g, b)
    x = make_input((2, 1, 32, 32, 32), freq=0.23)
    _check(g, _fwd_bwd(b, x), b)


def test_renet_bit_identical():
    from oracle.fill import make_input_rough
    g = _fixture("renet")
    b = fill_module_(nets.RE_Net()).train()
    _same_keys(g, b)
    x = make_input_rough((1, 1, 32, 32, 32), seed=5.0)
    _check(g, _fwd_bwd(b, x), b)


def test_ernet_bit_identical():
    from oracle.fill import make_input_rough
    g = _fixture("ernet")
    b = fill_module_(nets.ER_Net(classes=2, channels=1)).train()
    _same_keys(g, b)
    x = make_input_rough((1, 1, 32, 32, 32), seed=7.0)
    _check(g, _fwd_bwd(b, x), b)
