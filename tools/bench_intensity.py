#!/usr/bin/env python3
"""Intensity normalisation on the device (csrc/intensity.hip; config.intensity) against numpy on the host, at 128^3 and 256^3, on
three inputs: Gaussian, the CT-like volume (70 % of the voxels at one value, the rest Gaussian) and an all-equal volume.

Cache-cold: every timed call works on the next of enough copies of the volume to exceed 512 MiB (L2 and the 256 MiB Infinity Cache
hold none of it when its turn comes again; what the chain's own later passes find in cache is part of the chain).  Device events
after a warm-up, the median (min .. max) of ``--windows`` windows of at least ``--window-s`` seconds each.  Per (shape, input):
  select2_ms / select11_ms   the nine launches of mi355seg_percentiles_f32 for 2 percentiles (0.5, 99.5) and the 11 of Nyul; the bytes
                 its four histogram passes read (16 B per voxel) over that time, as a fraction of ``copy_gbps``: what a device-to-device
                 copy of 256 MiB moves in this process (read + write bytes)
  moments_ms     the two launches of mi355seg_intensity_moments_f32 (clamp map), 4 B per voxel
  map2_ms / map11_ms   the one launch of mi355seg_intensity_map_f32 with 2 and with 11 knots, out of place, 8 B per voxel
  <mode>_ms      functional.normalize_intensity whole, per mode, host clock: launches, the device-to-host copies of the statistics and
                 the knot arithmetic on the host between them (the all-equal volume has no range to normalise: not timed)
  host_ms        np.percentile of the same volume plus the numpy map of intensity.normalize_intensity_host, per mode (host clock)
The percentiles of the device and of numpy are asserted equal to 1e-12 before anything is timed.

usage: bench_intensity.py [--windows 5] [--window-s 0.25] [--host-reps 3] [--shapes 128 256]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mi355seg  # noqa: E402
from mi355seg import functional as F  # noqa: E402
from mi355seg import intensity as I  # noqa: E402

LANDMARKS = np.array([0.0, 8.0, 21.0, 30.0, 41.0, 50.0, 58.0, 71.0, 80.0, 93.0, 100.0])
LAUNCHES = {"select": 9, "moments": 2, "map": 1}


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


def host_timed(fn, reps):
    """median, min, max ms of ``fn`` on the host clock; ``fn`` ends synchronised"""
    res = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        res.append((time.perf_counter() - t) * 1e3)
    return {"median": float(np.median(res)), "min": min(res), "max": max(res), "calls": reps}


def make_input(kind, n, seed=1):
    rng = np.random.default_rng(seed)
    if kind == "equal":
        return np.full(n, -1024.0, np.float32)
    x = rng.normal(40.0, 300.0, n).astype(np.float32)
    if kind == "ct70":
        x[rng.random(n) < 0.7] = -1024.0
    return x


class Rotation:
    """enough device copies of a volume to exceed 512 MiB; ``next()`` hands out the one whose last use is longest ago"""

    def __init__(self, x, dev):
        k = max(2, (512 << 20) // (x.size * 4) + 1)
        self.copies = [torch.from_numpy(x).to(dev) for _ in range(k)]
        self.i = 0

    def next(self):
        self.i = (self.i + 1) % len(self.copies)
        return self.copies[self.i]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", type=int, default=[128, 256])
    ap.add_argument("--inputs", nargs="+", default=["gaussian", "ct70", "equal"], choices=["gaussian", "ct70", "equal"])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_intensity.py measures on an MI355X; there is nothing to time without one"
    mi355seg.lib()
    dev = torch.device("cuda:0")
    src = torch.empty(64 << 20, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    r_copy = timed(lambda: dst.copy_(src), a.windows, a.window_s)
    copy_gbps = 2 * src.numel() * 4 / (r_copy["median"] * 1e-3) / 1e9
    del src, dst
    modes = {"rescale": I.IntensitySpec("rescale"), "clip_znorm": I.IntensitySpec("clip_znorm"),
             "histogram": I.IntensitySpec("histogram", landmarks=LANDMARKS), "histogram_znorm": I.IntensitySpec("histogram_znorm", landmarks=LANDMARKS)}
    for side in a.shapes:
        for kind in a.inputs:
            n = side ** 3
            x = make_input(kind, n)
            rot = Rotation(x, dev)
            out = torch.empty_like(rot.copies[0])
            got = F.percentiles(rot.next(), I.NYUL_PERCENTILES).values.cpu().numpy()
            ref = np.percentile(x.astype(np.float64), I.NYUL_PERCENTILES)
            assert np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))) <= 1e-12, "device and numpy percentiles disagree"
            rate = lambda r, nbytes: {"gbps": nbytes / (r["median"] * 1e-3) / 1e9, "fraction_of_copy_rate": nbytes / (r["median"] * 1e-3) / 1e9 / copy_gbps}
            row = {"shape": [side] * 3, "input": kind, "copies": len(rot.copies), "copy_gbps": copy_gbps, "launches": LAUNCHES}
            for name, qs in (("select2", (0.5, 99.5)), ("select11", I.NYUL_PERCENTILES)):
                r = timed(lambda: F.percentiles(rot.next(), qs), a.windows, a.window_s)
                row[name + "_ms"] = r
                row[name + "_read"] = rate(r, 16 * n)
            lo, hi = (float(v) for v in ref[[0, 10]])
            clamp = I.clamp_map(lo, hi)
            r = timed(lambda: F.intensity_moments(rot.next(), clamp, None, lo), a.windows, a.window_s)
            row["moments_ms"], row["moments_read"] = r, rate(r, 4 * n)
            if hi > lo:
                m2 = I.rescale_map(lo, hi, 0.0, 1.0)
                m11 = I.histogram_map(ref, LANDMARKS)
                for name, imap in (("map2", m2), ("map11", m11)):
                    r = timed(lambda: F.intensity_map(rot.next(), imap, out=out), a.windows, a.window_s)
                    row[name + "_ms"], row[name + "_traffic"] = r, rate(r, 8 * n)
                for mode, spec in modes.items():
                    def whole():
                        F.normalize_intensity(rot.next(), spec)
                        torch.cuda.synchronize()
                    whole()
                    row[mode + "_ms"] = host_timed(whole, 10)
                    row[mode + "_host_ms"] = host_timed(lambda: I.normalize_intensity_host(x, spec), a.host_reps)
            row["np_percentile2_ms"] = host_timed(lambda: np.percentile(x, (0.5, 99.5)), a.host_reps)
            print(json.dumps(row), flush=True)
            del rot, out


if __name__ == "__main__":
    main()
