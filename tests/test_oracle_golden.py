"""The oracle (oracle/) must reproduce the fixtures captured from the reference
modules (tests/golden/make_golden.py).  Same torch build => same ATen CPU kernels, so
the tolerance is tight; it is not zero only because thread count may differ."""
import os

import numpy as np
import pytest
import torch

from oracle import losses as ol
from oracle.fill import fill_module_, make_class_labels, make_input, make_labels
from oracle.metric import metric as oracle_metric
from oracle.nets import UNet3D
from oracle.step import train_step, two_channel_gt
from conftest import load_golden

TOL = 2e-5


def _sample(t, k=4096):
    f = t.detach().reshape(-1)
    step = max(1, f.numel() // k)
    return f[::step][:k].numpy()


def test_unet3d_train_step_matches_reference_fixture(golden_dir):
    g = load_golden("unet3d_f8_32")
    m = fill_module_(UNet3D(in_channels=1, out_channels=2, init_features=8)).train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    x = make_input((2, 1, 32, 32, 32))
    gt = make_labels((2, 1, 32, 32, 32))
    grads = {}
    # capture grads before the optimizer step clears nothing (Adam keeps .grad)
    pred, mask, loss, (jac, dice) = train_step(m, opt, x, gt)
    assert abs(loss.item() - float(g["loss"])) < 1e-6
    assert np.abs(pred.detach().numpy() - g["pred"]).max() < TOL
    # masks: identical wherever the reference logit margin exceeds the tolerance
    margin = np.abs(g["pred"][:, 0] - g["pred"][:, 1])[:, None]
    same = mask.numpy().astype(np.uint8) == g["mask"]
    assert same[margin > 2 * TOL].all()
    params = dict(m.named_parameters())
    for k in g.files:
        if k.startswith("grad/"):
            ref = g[k]
            got = _sample(params[k[5:]].grad)
            assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), k
        elif k.startswith("post/"):
            assert np.abs(_sample(params[k[5:]]) - g[k]).max() < 2e-4, k   # Adam step = +-lr
        elif k.startswith("buf/"):
            assert np.abs(dict(m.named_buffers())[k[4:]].numpy() - g[k]).max() < 1e-5, k
    # Dice of the oracle metric on the fixture's own mask
    gt2 = two_channel_gt(gt)
    j2, d2 = oracle_metric(gt2.argmax(1, keepdim=True), torch.from_numpy(g["mask"].astype(np.int64)))
    assert abs(d2 - dice) < 1e-4 and abs(j2 - jac) < 1e-4
    m.eval()
    with torch.no_grad():
        pe = m(x).numpy()
    assert np.abs(pe - g["pred_eval"]).max() < 5e-4  # after one Adam step; params differ by <=2e-4 tolerance


def test_losses_match_reference_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "losses.npz"))
    shp = (2, 4, 8, 12, 10)
    logits = make_input(shp, freq=0.37, phase=0.3) * 2.0
    labels = make_class_labels((2, 8, 12, 10), 4)
    onehot = ol.make_one_hot(labels.unsqueeze(1), 4)
    assert np.array_equal(onehot.sum(dim=(0, 2, 3, 4)).numpy(), g["onehot_sum"])

    def check(fn, key):
        lg = logits.clone().requires_grad_(True)
        l = fn(lg)
        l.backward()
        assert abs(l.item() - float(g[key])) < 1e-6, key
        assert np.abs(lg.grad.numpy() - g[key + "_grad"]).max() < 1e-8 + 1e-5 * np.abs(g[key + "_grad"]).max(), key

    check(lambda z: ol.cross_entropy_3d(z, labels), "ce")
    check(lambda z: ol.bce_with_logits(z, onehot), "bce")
    check(lambda z: ol.dice_loss(z, onehot), "dice")
    check(lambda z: ol.dice_loss_multiclass(z, labels, 4, softmax=True), "dicess")
    check(lambda z: ol.dice_loss_multiclass(z, labels, 4, weight=[0.1, 0.2, 0.3, 0.4]), "dicess_w")
    pr = torch.sigmoid(logits[:, 1])
    for red in ("mean", "sum", "none"):
        got = ol.binary_dice_loss(pr, onehot[:, 1], reduction=red).numpy()
        assert np.abs(got - g["bdl_" + red]).max() < 1e-6
    with pytest.raises(Exception):
        ol.binary_dice_loss(pr, onehot[:, 1], reduction="bogus")


def test_vnet_and_resunet_oracle_match_reference_fixtures(golden_dir):
    from oracle.nets import ResUNet, VNet
    g = load_golden("vnet_32")
    torch.manual_seed(7)
    m = fill_module_(VNet(in_channels=1, classes=2)).train()
    x = make_input((2, 1, 32, 32, 32))
    gt2 = two_channel_gt(make_labels((2, 1, 32, 32, 32)))
    torch.manual_seed(11)
    pred = m(x)
    loss = ol.bce_with_logits(pred, gt2)
    assert abs(loss.item() - float(g["loss"])) < 1e-6
    assert np.abs(pred.detach().numpy() - g["pred"]).max() < TOL
    from oracle.fill import make_input_rough
    g = np.load(os.path.join(golden_dir, "resunet_f4.npz"))
    m = fill_module_(ResUNet(in_channels=4, n_classes=4, base_n_filter=4)).eval()
    x = make_input_rough((1, 4, 64, 64, 64))

    def smp(t, k=65536):
        f = t.detach().reshape(-1)
        return f[::max(1, f.numel() // k)][:k].numpy()
    # InstanceNorm over few voxels: the reference's fp32 result itself moves by ~5e-4 with the thread count
    with torch.no_grad():
        d = np.abs(smp(m(x)) - g["pred_eval"])
    assert d.mean() < 1e-5 and d.max() < 2e-3
    m.train()
    torch.manual_seed(11)
    d = np.abs(smp(m(x)) - g["pred"])
    assert d.mean() < 1e-5 and d.max() < 2e-3


def test_resunet_oracle_matches_the_well_conditioned_fixture(golden_dir):
    """resunet_f4_96.npz (kaiming-variance hash weights, 96^3: deepest InstanceNorm over 216 voxels): the oracle must sit
    within the PLAIN 1e-4 of the reference on every sampled voxel (the reference itself moves 8.6e-6 with the thread count)."""
    from oracle.fill import RESUNET96_HEAD_SCALE, fill_module_hash_, make_input_rough
    from oracle.nets import ResUNet
    g = load_golden("resunet_f4_96")
    assert float(g["thread_spread"]) < 2e-5
    m = fill_module_hash_(ResUNet(in_channels=4, n_classes=4, base_n_filter=4), RESUNET96_HEAD_SCALE).eval()
    x = make_input_rough((1, 4, 96, 96, 96), seed=2.0)
    with torch.no_grad():
        f = m(x).reshape(-1)
    K = 1 << 18
    got = f[::max(1, f.numel() // K)][:K].numpy()
    d = np.abs(got - g["pred_eval"])
    assert d.max() < TOL, d.max()
