"""GPU parity of the whole drop-in 3D U-Net train step (train.py:187-221) against
(a) the golden fixture captured from the reference modules and (b) the CPU oracle run
here on the same closed-form weights/inputs.  fp32: logits and Dice within 1e-4, argmax
masks identical wherever the reference logit margin exceeds the tolerance."""
import os

import numpy as np
import pytest
import torch

from oracle.fill import fill_module_, make_input, make_labels
from oracle.metric import metric as oracle_metric
from oracle.step import two_channel_gt

from conftest import load_golden

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _sample(t, k=4096):
    f = t.detach().reshape(-1)
    step = max(1, f.numel() // k)
    return f[::step][:k].cpu().numpy()


@pytest.fixture(autouse=True, params=["f16x3", "bf16x6", "fp32"])
def conv_math(request):
    """Every model-level parity test runs under all three arithmetics of the MFMA convolutions: the split-precision "f16x3",
    "bf16x6" and the exact fp32 MFMA (include/mi355seg.h, mi355seg_set_conv_math)."""
    import mi355seg
    mi355seg.set_conv_math(request.param)
    yield request.param
    mi355seg.set_conv_math(mi355seg.DEFAULT_CONV_MATH)


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mi355seg
    mi355seg.lib()
    return mi355seg


def test_unet3d_train_step_vs_reference_fixture(seg, golden_dir):
    from mi355seg.models.three_d.unet3d import UNet3D
    from mi355seg.engine import train_step
    g = load_golden("unet3d_f8_32")
    m = fill_module_(UNet3D(in_channels=1, out_channels=2, init_features=8)).cuda().train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    x = make_input((2, 1, 32, 32, 32)).cuda()
    gt = make_labels((2, 1, 32, 32, 32)).cuda()
    out = train_step(m, opt, x, gt)
    pred = out["pred"].detach().cpu().numpy()
    assert abs(out["loss"].item() - float(g["loss"])) < 1e-5
    assert np.abs(pred - g["pred"]).max() < TOL
    margin = np.abs(g["pred"][:, 0] - g["pred"][:, 1])[:, None]
    same = out["mask"].cpu().numpy().astype(np.uint8) == g["mask"]
    excluded = int((margin <= 2 * TOL).sum())
    assert same[margin > 2 * TOL].all(), "argmax mask differs where the reference margin is decisive"
    assert excluded < 0.001 * margin.size
    # Dice from the device counters vs the oracle metric on the reference mask
    gt2 = two_channel_gt(gt.cpu())
    jo, do = oracle_metric(gt2.argmax(1, keepdim=True), torch.from_numpy(g["mask"].astype(np.int64)))
    assert abs(out["dice"] - do) < TOL and abs(out["jaccard"] - jo) < TOL
    params = dict(m.named_parameters())
    for k in g.files:
        if k.startswith("grad/"):
            ref = g[k]
            got = _sample(params[k[5:]].grad)
            assert np.abs(got - ref).max() <= 2e-4 * max(1e-3, np.abs(ref).max()), k
        elif k.startswith("buf/"):
            assert np.abs(dict(m.named_buffers())[k[4:]].cpu().numpy() - g[k]).max() < 1e-5, k
    gn = np.array([float(p.grad.double().norm()) for p in m.parameters()])
    assert np.abs(gn - g["gradnorm"]).max() <= 2e-4 * g["gradnorm"].max()
    for k, b in m.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(b) == 1
    # parameters after the Adam step (train.py:109,213).  Step 1 of Adam moves every weight by -lr * g / (|g| + eps):
    # -+lr wherever the gradient is decisive, so there the post-step samples must agree to a small fraction of lr;
    # where |g| is within a few orders of eps = 1e-8 the step is rounding-sensitive and only the 2 * lr envelope holds.
    lr, checked = 1e-3, 0
    for k in g.files:
        if not k.startswith("post/"):
            continue
        ref_post, ref_grad = g[k].astype(np.float64), g["grad/" + k[5:]].astype(np.float64)
        got_post = _sample(params[k[5:]]).astype(np.float64)
        d = np.abs(got_post - ref_post)
        decisive = np.abs(ref_grad) > 1e-4
        assert d.max() <= 2 * lr + 1e-7, (k, d.max())
        if decisive.any():
            assert d[decisive].max() < 0.01 * lr, (k, d[decisive].max(), int(decisive.sum()))
            checked += int(decisive.sum())
    assert checked > 1000, checked
    m.eval()
    with torch.no_grad():
        pe = m(x).cpu().numpy()
    assert np.abs(pe - g["pred_eval"]).max() < 1e-3      # after one Adam step (sign-sensitive +-lr updates)


def test_unet3d_matches_oracle_other_shape(seg):
    """Non-cubic volume, batch 1, 3 input channels, 3 classes, width 4."""
    from mi355seg.models.three_d.unet3d import UNet3D
    from oracle.nets import UNet3D as OracleUNet
    a = fill_module_(OracleUNet(3, 3, 4)).train()
    b = fill_module_(UNet3D(3, 3, 4)).cuda().train()
    x = make_input((1, 3, 16, 32, 48), freq=0.013)
    ya = a(x)
    ya.square().mean().backward()
    yb = b(x.cuda())
    yb.square().mean().backward()
    assert (yb.detach().cpu() - ya.detach()).abs().max() < TOL
    ga = dict(a.named_parameters())
    gmax = max(float(q.grad.abs().max()) for q in ga.values())
    for k, p in b.named_parameters():
        ref = ga[k].grad      # conv biases in front of a BatchNorm have an exactly-zero true gradient
        assert (p.grad.cpu() - ref).abs().max() <= 2e-4 * float(ref.abs().max()) + 1e-6 * gmax, k


def test_train_cli_checkpoints_and_resume(seg, tmp_path):
    """`train.py config=unet config.k=v`: two epochs on synthetic patches, reference checkpoint format, resume."""
    from mi355seg.train import main
    out = str(tmp_path / "logs")
    args = ["config=unet", f"config.output_dir={out}", "config.patch_size=32,32,32", "config.batch_size=1",
            "config.iters_per_epoch=2", "config.epochs=2"]
    cfg, res = main(args)
    assert res["epoch"] == 2 and 0.0 < res["loss_avg"] < 2.0
    latest = os.path.join(cfg.hydra_path, "latest_checkpoint.pt")
    assert os.path.exists(latest) and os.path.exists(os.path.join(cfg.hydra_path, "checkpoint_0002.pt"))
    ck = torch.load(latest, map_location="cpu")
    assert set(ck) == {"model", "optim", "scheduler", "epoch"} and ck["epoch"] == 2
    assert "encoder1.enc1conv1.weight" in ck["model"] and len(ck["model"]) == 136
    # the reference saves DDP-wrapped state dicts ("module." prefix, train.py:286-306): resume must accept them
    ck["model"] = {"module." + k: v for k, v in ck["model"].items()}
    pref = str(tmp_path / "prefixed.pt")
    torch.save(ck, pref)
    args2 = [a if not a.startswith("config.output_dir=") else f"config.output_dir={tmp_path / 'logs_resume'}" for a in args[:-1]]
    cfg2, res2 = main(args2 + ["config.epochs=3", "config.load_mode=1", f"config.ckpt={pref}"])   # own run dir (same-second runs)
    assert res2["epoch"] == 3
    lines = open(os.path.join(cfg2.hydra_path, "scalars.jsonl")).read().strip().splitlines()
    assert len(lines) == 2 and "Training/dice" in lines[0]


def test_train_cli_cfg1_default_patch_vs_oracle_step(seg, tmp_path):
    """BASELINE configs[0] on the HIP path at its own shape: ``train.py config=unet`` with the reference's defaults (UNet3D(1, 2, 32),
    patch_size 64 x 64 x 64, kaiming init, Adam 1e-3; conf/config/unet.yaml:1-16, train.py:324-331), batch 1, one iteration -- against
    the CPU oracle's train step (train.py:187-221) on the same initial weights (same global seed, same init policy, same parameter
    order) and the same patch: loss and Dice within 1e-4 (north_star), every parameter after the Adam step within rounding of an
    lr-sized update."""
    from mi355seg.data import make_loader
    from mi355seg.train import main
    from oracle.nets import UNet3D as OracleUNet
    from oracle.step import train_step as oracle_step, weights_init_normal
    args = ["config=unet", f"config.output_dir={tmp_path / 'cfg1'}", "config.batch_size=1", "config.iters_per_epoch=1", "config.epochs=1"]
    torch.manual_seed(11)
    cfg, res = main(args)
    assert tuple(cfg.patch_size) == (64, 64, 64) and cfg.init_type == "kaiming"
    got = torch.load(os.path.join(cfg.hydra_path, "latest_checkpoint.pt"), map_location="cpu")["model"]
    # the oracle on the same start: same seed -> the same kaiming draws in the same parameter order; the same synthetic patch
    torch.manual_seed(11)
    m = OracleUNet(1, 2, 32)
    m.apply(weights_init_normal("kaiming"))
    m.train()
    batch = next(iter(make_loader(cfg, torch.device("cuda", 0), 1, seed=1234)))
    x, gt = batch["source"]["data"].cpu(), batch["gt"]["data"].cpu()
    assert tuple(x.shape) == (1, 1, 64, 64, 64)
    opt = torch.optim.Adam(m.parameters(), lr=float(cfg.init_lr))
    # (the GPU model of the logits comparison below is built from the oracle's INITIAL weights, before its optimizer step)
    from mi355seg.models.three_d.unet3d import UNet3D
    gm = UNet3D(1, 2, 32)
    gm.load_state_dict(m.state_dict())
    pred_ref, mask_ref, loss, (_, dice) = oracle_step(m, opt, x, gt)
    # north_star's bar on the logits themselves: the same step through engine.train_step, logits within 1e-4 of the oracle's, masks
    # identical wherever the oracle's margin is decisive
    from mi355seg.engine import make_adam, train_step
    gm = gm.cuda().train()
    o = train_step(gm, make_adam(gm.parameters(), lr=float(cfg.init_lr)), x.cuda(), gt.cuda())
    pg, pr = o["pred"].detach().cpu(), pred_ref.detach()
    assert float((pg - pr).abs().max()) < TOL, float((pg - pr).abs().max())
    decisive = (pr[:, 1] - pr[:, 0]).abs() > 2 * TOL
    assert int(((pg.argmax(1) != pr.argmax(1)) & decisive).sum()) == 0 and float(decisive.float().mean()) > 0.99
    assert abs(o["loss"].item() - float(loss)) < 1e-5 and abs(o["dice"] - float(dice)) < TOL
    del gm, o
    assert abs(res["loss_avg"] - float(loss)) < TOL, (res["loss_avg"], float(loss))
    assert abs(res["dice_avg"] - float(dice)) < TOL, (res["dice_avg"], float(dice))
    want = m.state_dict()
    assert set(want) == set(got) and len(got) == 136
    lr = float(cfg.init_lr)
    grads = {k: p.grad for k, p in m.named_parameters()}
    for k, w in want.items():
        if not w.is_floating_point():
            assert torch.equal(w, got[k]), k
            continue
        d = (w - got[k]).abs()
        if k not in grads:                                   # BatchNorm running statistics
            assert float(d.max()) <= 1e-5 * max(1.0, float(w.abs().max())), (k, float(d.max()))
            continue
        # the first Adam step is lr * g / (|g| + eps) = lr * sign(g): an element whose gradient is rounding noise (every conv bias in
        # front of a BatchNorm has gradient exactly 0 in exact arithmetic) may land 2 lr away; where the oracle's gradient is
        # well above that noise (2 % of the tensor's largest: fp32 reassociation through nine training-mode BatchNorm layers is the noise
        # floor of the small ones) the two steps must coincide
        assert float(d.max()) <= 2.05 * lr, (k, float(d.max()))
        g = grads[k].abs()
        solid = g > 2e-2 * float(g.max())
        if ("conv" in k and k.endswith(".bias") and not k.startswith("conv.")) or int(solid.sum()) == 0:
            continue
        off = int((d[solid] > 0.05 * lr).sum())
        assert off <= max(2, 0.01 * int(solid.sum())), (k, off, int(solid.sum()))


def test_train_cli_hip_graph_matches_eager(seg, tmp_path):
    """config.hip_graph=true: the iteration is captured after the first (eager) one and replayed; with StepLR stepping every epoch
    (the learning rate lives in a device tensor) the run must land EXACTLY on the checkpoint of the eager run that keeps the same
    optimizer state on the device (config.capturable_adam=true: same kernels, same order, same arithmetic -- same bits)."""
    from mi355seg.train import main
    common = ["config=unet", "config.patch_size=32,32,32", "config.batch_size=1", "config.iters_per_epoch=3", "config.epochs=2",
              "config.scheduler_step_size=1"]
    torch.manual_seed(5)                   # train.py draws the initial weights from the global RNG (weights_init_normal, no seed of its own)
    cfg_a, res_a = main(common + [f"config.output_dir={tmp_path / 'eager'}", "config.capturable_adam=true"])
    torch.manual_seed(5)
    cfg_b, res_b = main(common + [f"config.output_dir={tmp_path / 'graph'}", "config.hip_graph=true"])
    a = torch.load(os.path.join(cfg_a.hydra_path, "latest_checkpoint.pt"), map_location="cpu")
    b = torch.load(os.path.join(cfg_b.hydra_path, "latest_checkpoint.pt"), map_location="cpu")
    assert res_a["loss_avg"] == res_b["loss_avg"] and res_a["dice_avg"] == res_b["dice_avg"]
    for k in a["model"]:
        assert torch.equal(a["model"][k], b["model"][k]), k
    assert abs(float(b["optim"]["param_groups"][0]["lr"]) - 0.001 * 0.8 ** 2) < 1e-9
    # and the host-state Adam of a plain run (lr / step / bias corrections as host doubles) agrees with both to rounding
    torch.manual_seed(5)
    cfg_c, res_c = main(common + [f"config.output_dir={tmp_path / 'plain'}"])
    assert abs(res_a["loss_avg"] - res_c["loss_avg"]) < 1e-4


_CAPTURE_AFTER_EAGER = r"""
import sys, torch
sys.path.insert(0, %r)
import mi355seg
from mi355seg.engine import GraphedTrainStep, train_step
from mi355seg.models.three_d.unet3d import UNet3D
from oracle.fill import fill_module_, make_input, make_labels
x, gt = make_input((1, 1, 16, 16, 16)).cuda(), make_labels((1, 1, 16, 16, 16)).cuda()

def build():
    m = fill_module_(UNet3D(1, 2, 4)).cuda().train()
    return m, torch.optim.Adam(m.parameters(), lr=1e-3, capturable=True)

# eager reference: four steps
m0, o0 = build()
for _ in range(4):
    l0 = train_step(m0, o0, x, gt, sync_metric=False)["loss"].item()
# one eager step on the DEFAULT stream whose outputs stay alive (pred -> autograd graph -> the parameters' gradient accumulators,
# bound to the default stream; p.grad is set as well), then capture: one warm-up step + two replays
m1, o1 = build()
held = train_step(m1, o1, x, gt, sync_metric=False)
assert held["pred"].grad_fn is not None and all(p.grad is not None for p in m1.parameters())
g = GraphedTrainStep(m1, o1, x, gt, warmup=1)
for _ in range(2):
    l1 = g(x, gt, sync_metric=False)["loss"].item()
torch.cuda.synchronize()
assert held["pred"].grad_fn is not None
assert l0 == l1, (l0, l1)
for (k, a), (_, b) in zip(m0.state_dict().items(), m1.state_dict().items()):
    assert torch.equal(a, b), k
print("CAPTURED_AFTER_EAGER_OK")
"""


def test_graphed_step_captures_after_an_eager_step_with_a_live_output(seg):
    """VERDICT r4 item 8 / ADVICE: capturing after an eager backward of the same model used to abort the process inside
    hipStreamEndCapture whenever an old output was still referenced (gradient accumulators bound to the default stream; the
    constructor refused by a p.grad heuristic).  engine.GraphedTrainStep now captures on stand-in leaves whose accumulators are born
    on the capturing stream, so the scenario must simply work -- and land bitwise on the eager run's parameters.  Run once, in a
    process of its own: if the capture did abort, it would take that process, not the test session."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _CAPTURE_AFTER_EAGER % root], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "CAPTURED_AFTER_EAGER_OK" in p.stdout, (p.returncode, p.stdout[-1000:], p.stderr[-3000:])


def test_graphed_step_needs_a_capturable_optimizer(seg):
    from mi355seg.engine import GraphedTrainStep
    from mi355seg.models.three_d.unet3d import UNet3D
    from oracle.fill import fill_module_, make_input, make_labels
    x, gt = make_input((1, 1, 16, 16, 16)).cuda(), make_labels((1, 1, 16, 16, 16)).cuda()
    m = fill_module_(UNet3D(1, 2, 4)).cuda().train()
    with pytest.raises(ValueError, match="capturable"):
        GraphedTrainStep(m, torch.optim.Adam(m.parameters(), lr=1e-3), x, gt)


def test_predict_cli_sliding_window(seg, tmp_path):
    """predict.py: checkpoint load, eval-mode BN (running stats), grid patches + crop aggregation, metrics.csv."""
    from mi355seg.predict import main as predict_main, sliding_window_predict
    from mi355seg.train import main as train_main
    out = str(tmp_path / "logs")
    common = ["config=unet", f"config.output_dir={out}", "config.patch_size=32,32,32", "config.batch_size=2"]
    cfg, _ = train_main(common + ["config.iters_per_epoch=2", "config.epochs=1"])
    ckpt = os.path.join(cfg.hydra_path, "latest_checkpoint.pt")
    cfg2, rows = predict_main(common + [f"config.ckpt={ckpt}"])
    assert len(rows) == 2 and all(0.0 <= r["dice"] <= 1.0 for r in rows)
    assert os.path.exists(os.path.join(cfg2.hydra_path, "metrics.csv"))
    pred = np.load(os.path.join(cfg2.hydra_path, "synthetic_0_pred.npy"))
    assert pred.shape == (1, 64, 64, 64) and set(np.unique(pred)) <= {0, 1}
    # a volume that is exactly one patch: sliding window == plain eval forward + argmax
    from mi355seg.models.three_d.unet3d import UNet3D
    m = fill_module_(UNet3D(1, 2, 8)).cuda().eval()
    vol = make_input((1, 32, 32, 32)).cuda()
    a = sliding_window_predict(m, vol, (32, 32, 32), (4, 4, 4))
    with torch.no_grad():
        b = m(vol[None]).argmax(1)
    assert torch.equal(a, b)
    assert not m.training
    # mixed-precision inference (config.mixed_precision=bf16): eval-mode results do not depend on how patches are batched,
    # and a one-patch volume equals the plain bf16 forward + argmax
    big = make_input((1, 48, 40, 64)).cuda()
    p1 = sliding_window_predict(m, big, (32, 32, 32), (4, 4, 4), batch_size=1, dtype=torch.bfloat16)
    p3 = sliding_window_predict(m, big, (32, 32, 32), (4, 4, 4), batch_size=3, dtype=torch.bfloat16)
    assert p1.shape == (1, 48, 40, 64) and torch.equal(p1, p3)
    with torch.no_grad(), seg.autocast(torch.bfloat16):
        bb = m(vol[None]).argmax(1)
    assert torch.equal(sliding_window_predict(m, vol, (32, 32, 32), (4, 4, 4), dtype=torch.bfloat16), bb)


def test_inference_path_against_the_oracle_eval_forward(seg, golden_dir):
    """predict.py:79-81,98-147 as a kernel path.  (1) model.eval() under no_grad runs the FOLDED form (eval-mode BatchNorm inside the
    packed weights and the bias slot, activation in the conv epilogue): logits against the pinned oracle's eval forward (itself
    bit-identical to the reference, tests/test_oracle_vs_reference.py) and the reference fixture's eval logits at 1e-4, and against
    the two-pass form (conv, then norm_act with running statistics), under both conv maths (module fixture) and in bf16 within
    the bf16 rounding of the two-pass bf16 result.  (2) The device-resident sliding window (gather launch, folded forward, argmax,
    paste launch) against torchio-order aggregation done on the host FROM THE ORACLE'S logits of every patch: identical labels
    wherever the oracle's logit margin is decisive.  (The grid itself is restated from torchio, which is absent: that part stays
    unpinned, see DESIGN.)"""
    from mi355seg.models.three_d.unet3d import UNet3D
    from mi355seg.predict import crop_window, grid_locations, sliding_window_predict
    from oracle.nets import UNet3D as OracleUNet
    o = fill_module_(OracleUNet(1, 2, 8)).eval()
    m = fill_module_(UNet3D(1, 2, 8)).cuda().eval()
    x = make_input((2, 1, 32, 32, 32))
    with torch.no_grad():
        want = o(x)
        got = m(x.cuda())                                   # folded one-pass form
    with torch.enable_grad():
        two_pass = m(x.cuda()).detach()                     # grad mode on: the conv + norm_act form (eval statistics)
    assert (got.cpu() - want).abs().max() < TOL and (two_pass.cpu() - want).abs().max() < TOL
    assert (got - two_pass).abs().max() < 2e-5
    with torch.no_grad(), seg.autocast(torch.bfloat16):
        g16 = m(x.cuda())
    with torch.enable_grad(), seg.autocast(torch.bfloat16):
        t16 = m(x.cuda()).detach()
    assert (g16 - t16).abs().max() <= 0.05 * float(want.abs().max()) and (g16.cpu() - want).abs().max() <= 0.08 * float(want.abs().max())
    # sliding window over a volume of several patches per axis, ragged last patch, batches of 3
    size, ps, ov = (40, 48, 72), (32, 32, 32), (4, 4, 12)
    vol = make_input((1,) + size, freq=0.017)
    labels = sliding_window_predict(m, vol.cuda(), ps, ov, batch_size=3).cpu()
    ref = torch.full((1,) + size, -1, dtype=torch.int64)
    margin = torch.full((1,) + size, 0.0)
    with torch.no_grad():
        for loc in grid_locations(size, ps, ov):
            z, y, w = loc
            lg = o(vol[None, :, z:z + 32, y:y + 32, w:w + 32])[0]
            src, dst = crop_window(loc, ps, size, ov)
            ref[(0,) + dst] = lg.argmax(0)[src]
            margin[(0,) + dst] = (lg[0] - lg[1]).abs()[src]
    assert int((ref < 0).sum()) == 0
    decisive = margin > 2 * TOL
    assert float(decisive.float().mean()) > 0.95 and torch.equal(labels[decisive], ref[decisive])


def test_hip_graph_train_step_matches_eager(seg):
    """The captured-and-replayed step (engine.GraphedTrainStep) is the same arithmetic as the eager one: identical
    loss, Dice counters and parameters after the same number of optimiser steps."""
    from mi355seg.engine import GraphedTrainStep, train_step
    from mi355seg.models.three_d.unet3d import UNet3D
    from oracle.fill import fill_module_, make_input, make_labels
    x = make_input((1, 1, 32, 32, 32)).cuda()
    gt = make_labels((1, 1, 32, 32, 32)).cuda()
    xs = [x + 0.1 * i for i in range(3)]

    def fresh():
        m = fill_module_(UNet3D(1, 2, 8)).cuda().train()
        return m, torch.optim.Adam(m.parameters(), lr=1e-3, capturable=True)

    m0, o0 = fresh()
    eager = [train_step(m0, o0, x, gt, sync_metric=False) for _ in range(3)]          # == the graph's 3 warm-up steps
    eager += [train_step(m0, o0, xi, gt, sync_metric=False) for xi in xs]
    eager = [(float(e["loss"]), e["counts"].tolist()) for e in eager]
    m1, o1 = fresh()
    g = GraphedTrainStep(m1, o1, x, gt, warmup=2)                                      # 2 eager + 1 captured-but-not-run...
    got = []
    for xi in [x] + xs:                                                                # capture does not execute: replay the 3rd step
        out = g(xi, gt, sync_metric=False)
        got.append((float(out["loss"]), out["counts"].tolist()))
    assert got == eager[2:]
    for (k, a), (_, b) in zip(m0.state_dict().items(), m1.state_dict().items()):
        assert torch.equal(a, b), k


def test_make_adam_matches_default_adam(seg):
    """engine.make_adam (train.py:109's optimizer as torch's fused single-kernel Adam) against the default implementation:
    the same update rule, so five steps on the same gradients agree to fp32 rounding."""
    from mi355seg.engine import make_adam
    g = torch.Generator().manual_seed(7)
    shapes = [(64, 32, 3, 3, 3), (64,), (17,), (5, 3)]
    pa = [torch.randn(s, generator=g).cuda().requires_grad_(True) for s in shapes]
    pb = [p.detach().clone().requires_grad_(True) for p in pa]
    oa, ob = make_adam(pa, lr=1e-3), torch.optim.Adam(pb, lr=1e-3)
    assert oa.defaults.get("fused"), "make_adam must pick the fused implementation for CUDA parameters"
    for step in range(5):
        for a, b in zip(pa, pb):
            gr = torch.randn(a.shape, generator=g).cuda()
            a.grad, b.grad = gr.clone(), gr.clone()
        oa.step(); ob.step()
    for a, b in zip(pa, pb):
        assert (a - b).abs().max() <= 2e-6 * max(1.0, float(b.abs().max()))
    # CPU parameters: the default implementation, no error
    assert not make_adam([torch.zeros(3, requires_grad=True)], lr=1e-3).defaults.get("fused")


def test_carried_operand_maxima_bound_the_tensors(seg, monkeypatch):
    """the f16x3 operand maxima ride along as tensor attributes / device scalars and are never re-measured; a too-SMALL one
    would overflow the fp16 high part silently.  Debug mode ``functional.check_amax()`` compares every maximum a convolution is handed with
    the tensor's true maximum: a whole U-Net train step (double-conv nodes with the norm prologue's BOUND, pool- and head-fused blocks,
    concat buffers, ConvT, weights from the multi-tensor prefetch) must pass it, and a tensor modified through a raw pointer after its
    maximum was recorded -- the case the invariant in functional.check_amax's docstring forbids -- must be caught."""
    from mi355seg.engine import make_adam, train_step
    from mi355seg.models.three_d.unet3d import UNet3D
    from oracle.fill import fill_module_, make_input, make_labels
    F = seg.functional
    if seg.get_conv_math() != "f16x3":
        pytest.skip("operand maxima are an f16x3 matter")
    F.check_amax(True)
    try:
        m = fill_module_(UNet3D(1, 2, 32)).cuda().train()
        x, gt = make_input((1, 1, 32, 32, 32)).cuda(), make_labels((1, 1, 32, 32, 32)).cuda()
        out = train_step(m, make_adam(m.parameters(), lr=1e-3), x, gt)
        assert np.isfinite(out["loss"].item())
        # the forbidden case: a raw-pointer write behind the recorded maximum (copy_ would bump the version; the library's kernels do not)
        t = torch.rand(1, 8, 8, 16, 32, device="cuda")
        F._set_amax(t, F._measure_amax(t, 32, 8 * 8 * 16, 32))
        assert F._get_amax(t) is not None
        five = t * 0 + 5.0
        seg.lib().call("mi355seg_act_fwd_f32", five.data_ptr(), 32, None, 0, t.data_ptr(), 32, 8 * 8 * 16, 32, F.ACT_NONE, 0.0,
                       torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        with pytest.raises(seg.Mi355SegError, match="too small"):
            F._get_amax(t)
    finally:
        F.check_amax(False)
