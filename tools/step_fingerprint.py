#!/usr/bin/env python3
"""Fingerprint of a few training steps of one named configuration: one JSON object with the sha256 of the bit patterns of each
step's loss, of the last step's logits, of every parameter and buffer after it, and -- for the last step -- the library's own
launch record in order, as (family, algorithmic flops, algorithmic bytes) per launch (milliseconds dropped).  Two checkouts that
print the same line for a configuration computed the same bits with the same launches in the same order: the way to show that a
change to the Python around the kernels is "bit-identical".

usage: step_fingerprint.py --list | step_fingerprint.py <configuration>

Only the package's public surface is used (engine.train_step / GraphedTrainStep, functional.autocast, set_conv_math, the
in-library profiler), so the same file runs against an older checkout.  Inputs come from oracle.fill."""
import ctypes
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import mi355seg  # noqa: E402
from mi355seg import functional as F  # noqa: E402
from mi355seg.engine import GraphedTrainStep, train_step  # noqa: E402
from oracle.fill import fill_module_, make_input, make_labels  # noqa: E402

BF16 = torch.bfloat16


def _with(module, **attrs):
    for k, v in attrs.items():
        setattr(module, k, v)
    return module


def _model(name):
    from mi355seg.models.three_d import unet3d, vnet3d, residual_unet3d, csrnet, RE_net, ER_net, IS, unetr
    return {"unet": lambda: unet3d.UNet3D(1, 2, 16), "vnet": lambda: vnet3d.VNet(in_channels=1, classes=2),
            "resunet": lambda: residual_unet3d.UNet(4, 2, 16), "csrnet": lambda: csrnet.CSRNet(in_channels=1, out_channels=2, init_features=4),
            "renet": lambda: RE_net.RE_Net(), "ernet": lambda: ER_net.ER_Net(classes=2, channels=1),
            "isnet": lambda: IS.UNet3D(in_channels=1, out_channels=2, init_features=4),
            "isnet_device_bands": lambda: _with(IS.UNet3D(in_channels=1, out_channels=2, init_features=4), band_split="device"),
            "unetr": lambda: unetr.UNETR(img_shape=(32, 32, 32), input_dim=1, output_dim=2, embed_dim=96, patch_size=16, num_heads=4, dropout=0.0),
            "torch_ops": lambda: unet3d.UNet3D(1, 2, 8)}[name]()


# name -> (model, input shape, conv math, autocast dtype, mode)
CONFIGS = {f"unet-{m}": ("unet", (2, 1, 32, 32, 32), m, None, "train") for m in ("f16x3", "bf16x6", "fp32")}
CONFIGS.update({
    "unet-f16x3-graph": ("unet", (2, 1, 32, 32, 32), "f16x3", None, "graph"),
    "unet-bf16": ("unet", (2, 1, 32, 32, 32), None, BF16, "train"),
    "unet-eval-fp32": ("unet", (2, 1, 32, 32, 32), None, None, "eval"),
    "unet-eval-bf16": ("unet", (2, 1, 32, 32, 32), None, BF16, "eval"),
    "vnet": ("vnet", (1, 1, 32, 32, 32), None, None, "train"),
    "vnet-bf16": ("vnet", (1, 1, 32, 32, 32), None, BF16, "train"),
    "resunet": ("resunet", (1, 4, 32, 48, 32), None, None, "train"),
    "resunet-bf16": ("resunet", (1, 4, 32, 48, 32), None, BF16, "train"),
    "resunet-n2": ("resunet", (2, 4, 32, 48, 32), None, None, "train"),
    "csrnet": ("csrnet", (2, 1, 32, 32, 32), None, None, "train"),
    "renet": ("renet", (1, 1, 32, 32, 32), None, None, "train"),
    "ernet": ("ernet", (1, 1, 32, 32, 32), None, None, "train"),
    "isnet": ("isnet", (1, 1, 32, 32, 32), None, None, "train"),
    "isnet-bands-device": ("isnet_device_bands", (1, 1, 32, 32, 32), None, None, "train"),     # config.band_split=device (csrc/band.hip)
    "unetr": ("unetr", (2, 1, 32, 32, 32), None, None, "train"),
    "torch_ops": ("torch_ops", (2, 1, 32, 32, 32), None, None, "ops"),
})


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def launches(L):
    """The profiler's per-launch records since the last reset, in order, without the milliseconds."""
    buf = (ctypes.c_double * 32)()
    L.call("mi355seg_prof_read", buf, 32)                # (synchronises the recorded events)
    nmax = 65536
    rec, n = (ctypes.c_double * (4 * nmax))(), ctypes.c_int(0)
    L.call("mi355seg_prof_records", rec, nmax, ctypes.byref(n))
    L.call("mi355seg_prof_enable", 0)
    return [(int(rec[4 * r]), rec[4 * r + 2], rec[4 * r + 3]) for r in range(n.value)]


def profiled(L):
    L.call("mi355seg_prof_reset")
    L.call("mi355seg_prof_enable", 1)


def torch_ops_step(m, x, gt):
    """The forward / backward of tests/test_custom_ops.py written in torch.ops.mi355seg calls only (the module is a parameter container)."""
    from mi355seg import custom_ops as C
    from oracle.step import two_channel_gt
    ops, RELU = torch.ops.mi355seg, F.ACT_RELU

    def block(h, blk):
        conv1, norm1, _r1, conv2, norm2, _r2 = blk.children()
        return C.conv_bn_act_train(C.conv_bn_act_train(h, conv1, norm1, RELU), conv2, norm2, RELU)
    h, skips = ops.to_channels_last(x), []
    for enc in (m.encoder1, m.encoder2, m.encoder3, m.encoder4):
        skips.append(block(h, enc))
        h, _idx = ops.max_pool3d_2x(skips[-1])
    h = block(h, m.bottleneck)
    for up, dec in ((m.upconv4, m.decoder4), (m.upconv3, m.decoder3), (m.upconv2, m.decoder2), (m.upconv1, m.decoder1)):
        h = block(ops.cat_channels(ops.conv_transpose3d_k2s2(h, up.weight, up.bias), skips.pop()), dec)
    logits = ops.to_channels_first(ops.conv3d(h, m.conv.weight, m.conv.bias, 1, 0))
    loss, _mask, _counts = ops.bce_argmax_dice(logits, two_channel_gt(gt).float())
    loss.backward()
    return logits, loss


def fingerprint(name):
    model, shape, math, dtype, mode = CONFIGS[name]
    L = mi355seg.lib()
    mi355seg.set_conv_math(math or mi355seg.DEFAULT_CONV_MATH)
    torch.manual_seed(7)
    torch.cuda.manual_seed(7)                            # (Dropout3d draws from the device generator)
    m = fill_module_(_model(model)).cuda()
    x = make_input(shape).cuda()
    gt = make_labels((shape[0], 1) + shape[2:]).cuda()
    out = {"config": name, "loss": [], "launches": None}
    if mode == "eval":
        m.eval()
        profiled(L)
        with torch.no_grad(), F.autocast(dtype or torch.float32):
            pred = m(x)
        out["launches"] = launches(L)
    elif mode == "ops":
        m.train()
        profiled(L)
        pred, loss = torch_ops_step(m, x, gt)
        out["launches"] = launches(L)
        out["loss"].append(sha(loss))
        out["grad"] = {k: sha(p.grad) for k, p in m.named_parameters()}
    elif mode == "graph":
        m.train()
        g = GraphedTrainStep(m, torch.optim.Adam(m.parameters(), lr=1e-3, capturable=True), x, gt, warmup=2, dtype=dtype)
        out["loss"].append(sha(g.first["loss"]))
        for _ in range(2):
            o = g(x, gt, sync_metric=False)
            out["loss"].append(sha(o["loss"]))
        pred = o["pred"]
    else:
        m.train()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        for step in range(3):                            # step 1 records the prepack plan, steps 2-3 replay it
            if step == 2:
                profiled(L)
            o = train_step(m, opt, x, gt, sync_metric=False, dtype=dtype)
            out["loss"].append(sha(o["loss"]))
        out["launches"] = launches(L)
        pred = o["pred"]
    torch.cuda.synchronize()
    out["logits"] = sha(pred)
    out["param"] = {k: sha(p) for k, p in m.named_parameters()}
    out["buffer"] = {k: sha(b) for k, b in m.named_buffers()}
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2 or (sys.argv[1] != "--list" and sys.argv[1] not in CONFIGS):
        sys.exit(__doc__)
    print("\n".join(CONFIGS) if sys.argv[1] == "--list" else json.dumps(fingerprint(sys.argv[1]), sort_keys=True))
