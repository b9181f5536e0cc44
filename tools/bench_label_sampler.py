#!/usr/bin/env python3
"""Label-balanced patch sampling on the device (csrc/sampler.hip; tio.LabelSampler semantics, config.sampler=label) against the host
statement of the same sampler, on sparse vessel-like labels (foreground ~0.5 % of the voxels).

Per (volume, patch) pair, with device events after a warm-up, the median (min .. max) of ``--windows`` windows of at least
``--window-s`` seconds each:
  build_ms      the two launches of mi355seg_label_index_build_f32 (once per subject and patch size), index already allocated
  build_call_ms functional.label_index: allocation, the two launches and the device-to-host copy of the 17 counts (host clock)
  select_us     the one launch of mi355seg_label_index_select for ``--picks`` picks, pick table already on the device
  pick_call_us  functional.label_pick + the copy of the origins to the host: what a subject visit of the queue pays (host clock)
  host_ms       the same picks on the host by the numpy statement the tests use: ``np.flatnonzero(region.ravel() == l)[r]`` per pick,
                the labels already in host memory (host clock, median of ``--host-reps`` runs)
  label_bytes   4 bytes per voxel of the region of valid centres, the bytes the build has to read, and the rate build_ms achieves
                against them as a fraction of ``copy_gbps``: what a device-to-device copy of 256 MiB moves here (read + write bytes)
The origins of the device and the host are asserted equal before anything is timed.

usage: bench_label_sampler.py [--windows 5] [--window-s 0.25] [--picks 10] [--host-reps 5] [--cases 128/64 256/128 256/64]"""
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
from mi355seg.data import draw_label_picks  # noqa: E402

CASES = {"128/64": (128, 64), "256/128": (256, 128), "256/64": (256, 64)}           # volume^3 / patch^3


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


def vessels(n, seed):
    """float32 [n,n,n] labels: a few thin tubes of class 1 (and fewer of class 2) through background"""
    rng = np.random.default_rng(seed)
    y = np.zeros((n, n, n), dtype=np.float32)
    t = np.arange(n)
    for k in range(max(4, n // 8)):
        a, b = rng.uniform(0.1, 0.9, 2) * n
        fa, fb = rng.uniform(0.5, 2.0, 2)
        yy = np.clip((a + 0.2 * n * np.sin(fa * 2 * np.pi * t / n)).astype(int), 1, n - 2)
        xx = np.clip((b + 0.2 * n * np.cos(fb * 2 * np.pi * t / n)).astype(int), 1, n - 2)
        for dy in (0, 1):
            for dx in (0, 1):
                y[t, yy + dy, xx + dx] = 1.0 if k % 4 else 2.0
    return y


def host_picks(y, ps, classes, ranks):
    r = y[tuple(slice(p // 2, p // 2 + n - p + 1) for n, p in zip(y.shape, ps))]
    flat = r.ravel()
    e = np.array([np.flatnonzero(flat == l)[k] for l, k in zip(classes, ranks)], dtype=np.int64)
    return np.stack(np.unravel_index(e, r.shape), axis=1).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--picks", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=list(CASES))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_label_sampler.py measures on an MI355X; there is nothing to time without one"
    L = mi355seg.lib()
    dev = torch.device("cuda:0")
    src = torch.empty(64 << 20, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    r_copy = timed(lambda: dst.copy_(src), a.windows, a.window_s)
    copy_gbps = 2 * src.numel() * 4 / (r_copy["median"] * 1e-3) / 1e9
    del src, dst
    for name in a.cases:
        n, p = CASES[name]
        ps = (p, p, p)
        y = vessels(n, 3)
        yd = torch.from_numpy(y).to(dev)
        index = F.label_index(yd, ps)
        rng = np.random.default_rng(1)
        classes, ranks = draw_label_picks(rng, index.counts, None, a.picks)
        got = F.label_pick(index, classes, ranks).cpu().numpy()
        assert np.array_equal(got, host_picks(y, ps, classes, ranks)), "device and host disagree"
        st = torch.cuda.current_stream().cuda_stream
        nbytes = L.query("mi355seg_label_index_bytes", n, n, n, *ps)
        idx2, cnt2 = torch.empty_like(index.index), torch.empty(17, dtype=torch.int64, device=dev)
        picks = torch.from_numpy(np.ascontiguousarray(np.stack([classes, ranks], axis=1))).to(dev)
        org = torch.empty((a.picks, 3), dtype=torch.int32, device=dev)
        build = lambda: L.call("mi355seg_label_index_build_f32", yd.data_ptr(), n, n, n, *ps, idx2.data_ptr(), nbytes, cnt2.data_ptr(), st)
        select = lambda: L.call("mi355seg_label_index_select", yd.data_ptr(), n, n, n, *ps, index.index.data_ptr(), picks.data_ptr(),
                                a.picks, org.data_ptr(), st)
        build(); select()
        assert torch.equal(idx2, index.index) and np.array_equal(org.cpu().numpy(), got)
        r_build = timed(build, a.windows, a.window_s)
        r_select = timed(select, a.windows, a.window_s)
        r_build_call = host_timed(lambda: F.label_index(yd, ps), 20)
        r_pick_call = host_timed(lambda: F.label_pick(index, classes, ranks).cpu(), 50)
        r_host = host_timed(lambda: host_picks(y, ps, classes, ranks), a.host_reps)
        label_bytes = 4 * int(np.prod(index.region))
        gbps = label_bytes / (r_build["median"] * 1e-3) / 1e9
        us = lambda r: {k: (v * 1e3 if k != "calls_per_window" and k != "calls" else v) for k, v in r.items()}
        print(json.dumps({"case": name, "volume": [n] * 3, "patch": list(ps), "region": list(index.region), "chunks": int(index.index.shape[1]),
                          "index_bytes": int(nbytes), "foreground_share_of_region": float(index.counts[1:16].sum() / np.prod(index.region)),
                          "picks": a.picks, "build_ms": r_build, "build_call_ms": r_build_call, "select_us": us(r_select),
                          "pick_call_us": us(r_pick_call), "host_ms": r_host, "label_bytes": label_bytes, "build_gbps": gbps,
                          "copy_gbps": copy_gbps, "build_fraction_of_copy_rate": gbps / copy_gbps}), flush=True)


if __name__ == "__main__":
    main()
