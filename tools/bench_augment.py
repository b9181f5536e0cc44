#!/usr/bin/env python3
"""Device-side training augmentation (csrc/augment.hip; dataloader.py:69-86 with config.aug=True) at the sizes bench.py trains at:
cfg 2 (U-Net) = a batch of 2 x 1 x 128^3 and cfg 4 (Res-U-Net) = 1 x 4 x 160x192x160, patches cut from 256^3 volumes, affine and
elastic visits.

Per configuration and mode, with device events after a warm-up, the median (min .. max) of ``--windows`` windows of at least
``--window-s`` seconds each:
  stats_ms      the three statistics launches of one subject visit (functional.augment_stats)
  sample_ms     the one sampling launch of a batch, table already on the device (the kernel's own cost)
  batch_ms      functional.augment_sample: table build on the host + one upload + the launch (what the queue pays per batch)
  plain_ms      the same batch from the un-augmented queue: torch.stack of the patch windows of the z-normalised volumes
  bytes         compulsory traffic: the output writes plus ONE read of the touched source region (the bounding box of the mapped
                patch, clipped to the volume, image and label channels), and the rate sample_ms achieves against it

usage: bench_augment.py [--windows 5] [--window-s 0.25] [--configs cfg2 cfg4] [--once]
``--once`` runs every launch exactly once per configuration and mode (for a rocprofv3 --kernel-trace --stats run: launch counts)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mi355seg  # noqa: E402
from mi355seg import functional as F  # noqa: E402
from mi355seg.data import AugmentParams  # noqa: E402

CONFIGS = {"cfg2": dict(batch=2, C=1, patch=(128, 128, 128), step_ms=18.8),        # README: the fp32 U-Net train step
           "cfg4": dict(batch=1, C=4, patch=(160, 192, 160), step_ms=21.0)}        # README: the Res-U-Net leg
VOLUME = (256, 256, 256)


def timed(fn, windows, window_s):
    """median, min, max ms per call of ``fn`` over ``windows`` windows of >= ``window_s`` seconds (device events)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(); fn(); t1.record()
    torch.cuda.synchronize()
    n = max(3, int(window_s * 1e3 / max(t0.elapsed_time(t1), 1e-3)) + 1)
    res = []
    for _ in range(windows):
        t0.record()
        for _ in range(n):
            fn()
        t1.record()
        torch.cuda.synchronize()
        res.append(t0.elapsed_time(t1) / n)
    return {"median": float(np.median(res)), "min": min(res), "max": max(res), "calls_per_window": n}


def draw(rng, elastic):
    """a visit of the wanted kind from the queue's own distribution (redrawn until OneOf picks it)"""
    while True:
        p = AugmentParams.draw(rng, VOLUME)
        if p.elastic == elastic:
            return p


def touched_voxels(prm, origin, ps):
    """voxels of the bounding box of the mapped patch, clipped to the volume (elastic: widened by the largest displacement)"""
    m = prm.matrix.astype(np.float64)
    cs = np.array([[origin[a] + (ps[a] - 1) * ((k >> a) & 1) for a in range(3)] + [1.0] for k in range(8)])
    t = cs @ m.T
    slack = float(np.abs(prm.cp).max()) if prm.elastic else 0.0
    lo = np.clip(np.floor(t.min(0) - slack), 0, np.array(VOLUME) - 1)
    hi = np.clip(np.ceil(t.max(0) + slack) + 1, 0, np.array(VOLUME) - 1)
    return int(np.prod(hi - lo + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_augment.py measures on an MI355X; there is nothing to time without one"
    L = mi355seg.lib()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    for name in a.configs:
        cfg = CONFIGS[name]
        B, C, ps = cfg["batch"], cfg["C"], cfg["patch"]
        vols = [(torch.randn((C,) + VOLUME, device=dev, generator=gen) * 50 - 300,
                 (torch.rand((1,) + VOLUME, device=dev, generator=gen) > 0.6).float()) for _ in range(B)]
        normed = [F.znormalize(x) for x, _ in vols]
        rng = np.random.default_rng(1)
        origins = [tuple(int(rng.integers(0, n - p + 1)) for n, p in zip(VOLUME, ps)) for _ in range(B)]
        pS = int(np.prod(ps))

        def plain():
            xs = [v[(slice(None),) + tuple(slice(o, o + p) for o, p in zip(og, ps))] for v, og in zip(normed, origins)]
            ys = [y[(slice(None),) + tuple(slice(o, o + p) for o, p in zip(og, ps))] for (_, y), og in zip(vols, origins)]
            return torch.stack(xs), torch.stack(ys)

        for mode in ("affine", "elastic"):
            prms = [draw(rng, mode == "elastic") for _ in range(B)]
            stats = [F.augment_stats(x, p) for (x, _), p in zip(vols, prms)]
            cps = [torch.from_numpy(p.cp).to(dev) if p.elastic else None for p in prms]
            patches = [(x, y, st, cp, o, p) for (x, y), st, cp, o, p in zip(vols, stats, cps, origins, prms)]
            xb, yb = F.augment_sample(patches, ps)
            if a.once:
                torch.cuda.synchronize()
                print(json.dumps({"config": name, "mode": mode, "once": True, "finite": bool(torch.isfinite(xb).all())}))
                continue
            # the launch alone: the table F.augment_sample builds, kept on the device
            tab = np.zeros((B, F.AUG_DESC_WORDS), dtype=np.int32)
            t64, tf = tab.view(np.int64), tab.view(np.float32)
            for i, (x, y, st, cp, o, p) in enumerate(patches):
                t64[i, 0], t64[i, 1], t64[i, 2], t64[i, 3] = x.data_ptr(), y.data_ptr(), st.data_ptr(), (cp.data_ptr() if p.elastic else 0)
                tab[i, 8:11], tab[i, 11:14], tab[i, 14] = VOLUME, o, int(p.elastic)
                tf[i, 16:28], tf[i, 28:48], tf[i, 48] = p.matrix.reshape(-1), p.bias, p.sigma
                t64[i, 25] = p.seed
            table = torch.from_numpy(tab).to(dev)
            ox, oy = torch.empty_like(xb), torch.empty_like(yb)
            st_ = torch.cuda.current_stream().cuda_stream
            launch = lambda: L.call("mi355seg_augment_sample_f32", table.data_ptr(), B, C, 1, ps[0], ps[1], ps[2], ox.data_ptr(), oy.data_ptr(), st_)
            launch()
            assert torch.equal(ox, xb) and torch.equal(oy, yb)
            r_stats = timed(lambda: F.augment_stats(vols[0][0], prms[0]), a.windows, a.window_s)
            r_sample = timed(launch, a.windows, a.window_s)
            r_batch = timed(lambda: F.augment_sample(patches, ps), a.windows, a.window_s)
            r_plain = timed(plain, a.windows, a.window_s)
            out_bytes = 4 * B * (C + 1) * pS
            src_bytes = 4 * (C + 1) * sum(touched_voxels(p, o, ps) for p, o in zip(prms, origins))
            res = {"config": name, "mode": mode, "batch": [B, C] + list(ps), "volume": list(VOLUME), "stats_ms": r_stats, "sample_ms": r_sample,
                   "batch_ms": r_batch, "plain_ms": r_plain, "out_bytes": out_bytes, "src_bytes": src_bytes,
                   "sample_gbps_vs_compulsory": (out_bytes + src_bytes) / (r_sample["median"] * 1e-3) / 1e9,
                   "stats_gbps_two_reads": 2 * 4 * C * int(np.prod(VOLUME)) / (r_stats["median"] * 1e-3) / 1e9,
                   "out_of_domain_share": float((xb == torch.stack([s[2] for s in stats]).reshape(B, 1, 1, 1, 1)).float().mean())}
            if cfg["step_ms"]:
                res["share_of_train_step"] = r_batch["median"] / cfg["step_ms"]
            print(json.dumps(res), flush=True)
        del vols, normed


if __name__ == "__main__":
    main()
