#!/usr/bin/env python3
"""Sliding-window inference (predict.py:98-147: grid patches with overlap (4, 4, 36), eval-mode forward, argmax, crop-mode
aggregation) of a synthetic volume: voxels of the volume per second and patches per second, fp32 (default conv math) or bf16.

usage: bench_predict.py [unet|vnet|res_unet] [--volume 256 256 256] [--patch 128] [--batch 2] [--dtype f32|bf16] [--reps 3]
                        [--metrics [--spacing 1.25 0.7 0.7]]

--metrics also times ``metric(gt, pred, spacing)`` (precision, recall, jaccard, dice, hs95: utils/metric.py of the package) with
device events around the whole call, after a warm-up, over 10 x --reps calls, on two pairs of the volume's size: the predicted volume against
itself shifted by one voxel along every axis (a random-weight network predicts speckle, so nearly every foreground voxel is a
surface voxel: the most the sort and the gather can be handed), and a smooth blob against the same field at a lower threshold,
shifted (surfaces like an organ's).  The surface sizes are printed with the times."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import mi355seg  # noqa: E402
from mi355seg.engine import weights_init_normal  # noqa: E402
from mi355seg.predict import grid_locations, sliding_window_predict  # noqa: E402


def smooth_blob(shape, seed, cutoff, thresh, shift):
    """int64 [1, D, H, W] on the GPU: low-passed Gaussian noise (Fourier coefficients above ``cutoff`` cycles per voxel zeroed),
    rolled by ``shift`` voxels, thresholded at ``thresh`` standard deviations."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    f = torch.fft.fftn(torch.randn(shape, device="cuda", generator=g))
    k2 = sum(torch.fft.fftfreq(n, device="cuda").reshape([-1 if i == j else 1 for j in range(3)]) ** 2 for i, n in enumerate(shape))
    field = torch.fft.ifftn(torch.where(k2 > cutoff * cutoff, torch.zeros_like(f), f)).real
    field = torch.roll(field / field.std(), shift, (0, 1, 2))
    return (field > thresh).to(torch.int64)[None]


def time_metrics(pred, spacing, reps):
    from mi355seg import functional as F
    from mi355seg.utils.metric import metric
    shape = tuple(pred.shape[-3:])
    pairs = {"pred": (torch.roll(pred, (1, 1, 1), (-3, -2, -1)), pred),
             "blob": (smooth_blob(shape, 1, 0.03, 0.8, (0, 0, 0)), smooth_blob(shape, 1, 0.03, 0.7, (1, 2, 1)))}
    res = {"spacing": list(spacing)}
    for name, (gt, pr) in pairs.items():
        vals = metric(gt, pr, spacing)                                  # warm-up: code objects, workspace, sort buffers
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(10 * reps):                                      # a call is milliseconds: time a window of 0.1 s
            vals = metric(gt, pr, spacing)
        t1.record()
        torch.cuda.synchronize()
        info = F.mask_edges(gt, pr)[1].tolist()
        res[f"metric_{name}_ms"] = t0.elapsed_time(t1) / (10 * reps)
        res[f"metric_{name}_edge_voxels"] = info[:2]
        res[f"metric_{name}_box"] = [info[5] - info[2], info[6] - info[3], info[7] - info[4]]
        res[f"metric_{name}_values"] = [float(v) for v in vals]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("name", nargs="?", default="unet", choices=["unet", "vnet", "res_unet"])
    ap.add_argument("--volume", type=int, nargs=3, default=[256, 256, 256])
    ap.add_argument("--patch", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--metrics", action="store_true")
    ap.add_argument("--spacing", type=float, nargs=3, default=[1.25, 0.7, 0.7])
    a = ap.parse_args()
    mi355seg.lib()
    torch.manual_seed(0)
    if a.name == "unet":
        from mi355seg.models.three_d.unet3d import UNet3D
        m, cin = UNet3D(1, 2, 32), 1
    elif a.name == "vnet":
        from mi355seg.models.three_d.vnet3d import VNet
        m, cin = VNet(in_channels=1, classes=2), 1
    else:
        from mi355seg.models.three_d.residual_unet3d import UNet
        m, cin = UNet(4, 4, 32), 4
    m.apply(weights_init_normal("kaiming"))
    m = m.cuda().eval()
    vol = torch.randn((cin,) + tuple(a.volume), device="cuda")
    ps, ov = (a.patch,) * 3, (4, 4, 36)
    npatch = len(grid_locations(tuple(a.volume), ps, ov))
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    sliding_window_predict(m, vol, ps, ov, a.batch, dtype=dt)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        out = sliding_window_predict(m, vol, ps, ov, a.batch, dtype=dt)
    torch.cuda.synchronize()
    sec = (time.perf_counter() - t0) / a.reps
    nvox = a.volume[0] * a.volume[1] * a.volume[2]
    res = {"model": a.name, "volume": a.volume, "patch": a.patch, "overlap": list(ov), "batch": a.batch, "dtype": a.dtype,
           "conv_math": "bf16" if a.dtype == "bf16" else mi355seg.get_conv_math(), "patches": npatch, "s_per_volume": sec,
           "volume_voxels_per_s": nvox / sec, "patches_per_s": npatch / sec, "labels": int(out.max().item()) + 1}
    if a.metrics:
        res["forward_ms"] = sec * 1e3
        res.update(time_metrics(out, tuple(a.spacing), a.reps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
