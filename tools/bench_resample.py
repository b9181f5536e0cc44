#!/usr/bin/env python3
"""Resampling to a target spacing on the device (csrc/resample.hip; config.resample_spacing) against scipy.ndimage.zoom on the host.

Shapes: 128^3 and 256 x 256 x 64 (D = 64) from spacing (2.5, 0.7, 0.7) to 1 mm, and 256^3 to 1.5 x its size per axis.

Cache-cold: every timed call works on the next of enough copies of the volume to exceed 512 MiB.  Device events after a warm-up, the
median (min .. max) of ``--windows`` windows of at least ``--window-s`` seconds each.  The per-axis tables are uploaded once, outside
the timed region (``functional.ResampleTables``), so a timed call is the library's launches alone.  Every kernel is reported with the
bytes it must move (source read once + result written once; the prefilter passes: one read and one write of the volume each) over
its time, as a fraction of ``copy_gbps``: what a device-to-device copy of 256 MiB moves in this process (read + write bytes).
  prefilter_w / _h / _d   the three passes of mi355seg_bspline3_prefilter_axis_f32, each alone
  gather0 / gather1 / gather3   mi355seg_resample3d_f32 at orders 0 / 1 / 3 (order 3 on prefiltered coefficients)
  labels_nearest / labels_linear   mi355seg_resample3d_labels_f32 (two launches) on a block label volume of 4 classes
  back_k2 / back_k4   mi355seg_resample3d_argmax_f32, the resampled grid back to the original one, K = 2 and 4 (no probability output)
  volume1_ms / volume3_ms   functional.resample_volume whole at orders 1 and 3, host clock (tables, upload, launches, synchronised)
  zoom1_ms / zoom3_ms   scipy.ndimage.zoom of the same volume to the same shape at orders 1 and 3 on the host

usage: bench_resample.py [--windows 5] [--window-s 0.2] [--host-reps 1] [--cases 0 1 2]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import scipy.ndimage as ndi  # noqa: E402
import torch  # noqa: E402
import mi355seg  # noqa: E402
from mi355seg import functional as F  # noqa: E402

CASES = [((128, 128, 128), (2.5, 0.7, 0.7), (1.0, 1.0, 1.0)), ((64, 256, 256), (2.5, 0.7, 0.7), (1.0, 1.0, 1.0)),
         ((256, 256, 256), (1.5, 1.5, 1.5), (1.0, 1.0, 1.0))]


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
    res = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        res.append((time.perf_counter() - t) * 1e3)
    return {"median": float(np.median(res)), "min": min(res), "max": max(res), "calls": reps}


class Rotation:
    """enough device copies of a tensor to exceed 512 MiB; ``next()`` hands out the one whose last use is longest ago"""

    def __init__(self, t):
        k = max(2, (512 << 20) // (t.numel() * t.element_size()) + 1)
        self.copies = [t.clone() for _ in range(k)]
        self.i = 0

    def next(self):
        self.i = (self.i + 1) % len(self.copies)
        return self.copies[self.i]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.2)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--cases", nargs="+", type=int, default=[0, 1, 2])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resample.py measures on an MI355X; there is nothing to time without one"
    mi355seg.lib()
    dev = torch.device("cuda:0")
    src = torch.empty(64 << 20, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    r_copy = timed(lambda: dst.copy_(src), a.windows, a.window_s)
    copy_gbps = 2 * src.numel() * 4 / (r_copy["median"] * 1e-3) / 1e9
    del src, dst
    for ci in a.cases:
        shape, spacing, target = CASES[ci]
        out_shape = F.resampled_shape(shape, spacing, target)
        n_in, n_out = int(np.prod(shape)), int(np.prod(out_shape))
        rng = np.random.default_rng(ci)
        x = ndi.gaussian_filter(rng.standard_normal(shape), 1.0).astype(np.float32)
        ratios = [t / s for s, t in zip(spacing, target)]
        back = [s / t for s, t in zip(spacing, target)]
        row = {"shape": list(shape), "out_shape": list(out_shape), "spacing": spacing, "target": target, "copy_gbps": copy_gbps}

        def rate(r, nbytes):
            g = nbytes / (r["median"] * 1e-3) / 1e9
            return {"gbps": g, "fraction_of_copy_rate": g / copy_gbps}

        rot = Rotation(torch.from_numpy(x).to(dev))
        row["copies"] = len(rot.copies)
        out = torch.empty_like(rot.copies[0])
        for name, axis in (("prefilter_w", 2), ("prefilter_h", 1), ("prefilter_d", 0)):
            r = timed(lambda: F.bspline3_prefilter(rot.next(), out=out, axis=axis), a.windows, a.window_s)
            row[name + "_ms"], row[name + "_traffic"] = r, rate(r, 8 * n_in)
        coef = Rotation(F.bspline3_prefilter(rot.copies[0]))
        for order in (0, 1, 3):
            tables = F.ResampleTables(shape, out_shape, ratios, order, dev)
            pool = coef if order == 3 else rot
            r = timed(lambda: F.resample3d(pool.next(), tables), a.windows, a.window_s)
            row[f"gather{order}_ms"], row[f"gather{order}_traffic"] = r, rate(r, 4 * (n_in + n_out))
        del coef
        small = tuple(-(-n // 8) for n in shape)
        y = np.repeat(np.repeat(np.repeat(rng.integers(0, 4, small), 8, 0), 8, 1), 8, 2)[:shape[0], :shape[1], :shape[2]].astype(np.float32)
        lab = Rotation(torch.from_numpy(np.ascontiguousarray(y)).to(dev))
        for mode in F.RESAMPLE_LABEL_MODES:
            tables = F.ResampleTables(shape, out_shape, ratios, F.RESAMPLE_LABEL_MODES.index(mode), dev)
            r = timed(lambda: F.resample3d_labels(lab.next(), tables, mode), a.windows, a.window_s)
            row[f"labels_{mode}_ms"], row[f"labels_{mode}_traffic"] = r, rate(r, 4 * (n_in + n_out))
        del lab
        tables = F.ResampleTables(out_shape, shape, back, 1, dev)
        labels = torch.empty((1,) + tuple(shape), dtype=torch.int64, device=dev)
        for K in (2, 4):
            prob = Rotation(torch.rand((K,) + tuple(out_shape), device=dev))
            L = mi355seg.lib()

            def way_back():
                p = prob.next()
                L.call("mi355seg_resample3d_argmax_f32", p.data_ptr(), K, *out_shape, *tables.args(), labels.data_ptr(), None, *shape,
                       torch.cuda.current_stream().cuda_stream)
            r = timed(way_back, a.windows, a.window_s)
            row[f"back_k{K}_ms"], row[f"back_k{K}_traffic"] = r, rate(r, 4 * K * n_out + 8 * n_in)
            del prob
        for order in (1, 3):
            def whole():
                F.resample_volume(rot.next(), spacing, target, order)
                torch.cuda.synchronize()
            whole()
            row[f"volume{order}_ms"] = host_timed(whole, 10)
            zoom = [o / n for o, n in zip(out_shape, shape)]
            row[f"zoom{order}_ms"] = host_timed(lambda: ndi.zoom(x, zoom, order=order, mode="mirror"), a.host_reps)
        print(json.dumps(row), flush=True)
        del rot, out


if __name__ == "__main__":
    main()
