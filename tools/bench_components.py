#!/usr/bin/env python3
"""Connected components of a predicted mask on the device (csrc/components.hip; functional.connected_components / filter_components,
``predict.py ... config.keep_largest=1``) against the host path it replaces, per (volume, mask, connectivity).

Masks: ``blob``, the smooth organ-like mask of ``bench_predict.py --metrics``; ``speckle``, independent voxels at density 0.31 (the
6-connectivity percolation threshold, where clusters are most tortuous); ``serpentine``, a one-voxel-wide path through every tile of
the volume (the longest merge chains and the deepest finds).

With device events after a warm-up, the median (min .. max) of ``--windows`` windows of at least ``--window-s`` seconds each:
  label_ms      the whole mi355seg_components_label_i64 call (five launches), outputs and workspace already allocated
  local_ms .. info_ms   each launch on its own, as the difference of two prefixes of the call (mi355seg_components_label_steps_i64);
                info_ms is the reduction over sizes[] and its one-block finalise together
  filter_ms     the one launch of mi355seg_components_filter_i64 (min_voxels = 2, no keep list)
  call_ms       functional.filter_components(mask, keep_largest=1): labelling, the compact table (torch.nonzero, a sort), the filter
                and the copy of the four statistics to the host (host clock)
  host_ms       what a user does today: mask to the host, scipy.ndimage.label, np.bincount, a mask of the largest component and the
                copy back (host clock, median of ``--host-reps`` runs)
  flatten / filter fraction of the copy rate: their algorithmic bytes (12 and 20 per voxel) over their time, against ``copy_gbps``,
                what a device-to-device copy of 256 MiB moves here (read + write bytes)
Labels, sizes and info are asserted equal to scipy's before anything is timed.

usage: bench_components.py [--sizes 128 256] [--masks blob speckle serpentine] [--connectivity 6 26] [--windows 5] [--window-s 0.25]
                           [--host-reps 3]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy import ndimage  # noqa: E402
import mi355seg  # noqa: E402
from mi355seg import functional as F  # noqa: E402
from bench_predict import smooth_blob  # noqa: E402

STEPS = ("local", "merge", "flatten", "info_reduce", "info_finalize")


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


def serpentine(n):
    """int64 [n, n, n]: every second row of every second slice, joined at alternating ends: one 6-connected path, one voxel wide"""
    m = np.zeros((n, n, n), dtype=np.int64)
    m[0::2, 0::2, :] = 1
    zs, line = list(range(0, n, 2)), 0
    for zi, z in enumerate(zs):
        ys = list(range(0, n, 2))[::-1 if zi % 2 else 1]
        for yi, y in enumerate(ys):
            end = n - 1 if line % 2 == 0 else 0
            if yi + 1 < len(ys):
                m[z, (y + ys[yi + 1]) // 2, end] = 1
            elif zi + 1 < len(zs):
                m[z + 1, y, end] = 1
            line += 1
    return m


def make_mask(kind, n):
    if kind == "blob":
        return smooth_blob((n, n, n), 1, 0.03, 0.8, (0, 0, 0))[0].contiguous()
    if kind == "speckle":
        g = torch.Generator(device="cuda").manual_seed(5)
        return (torch.rand((n, n, n), device="cuda", generator=g) < 0.31).to(torch.int64)
    return torch.from_numpy(serpentine(n)).cuda()


def host_path(mask, structure):
    m = mask.cpu().numpy()
    lab, n = ndimage.label(m != 0, structure)
    counts = np.bincount(lab.ravel())
    keep = (lab == (1 + int(np.argmax(counts[1:])))) if n else np.zeros_like(m, dtype=bool)
    out = torch.from_numpy(np.where(keep, m, 0)).cuda()
    torch.cuda.synchronize()
    return lab, n, counts, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--masks", nargs="+", default=["blob", "speckle", "serpentine"], choices=["blob", "speckle", "serpentine"])
    ap.add_argument("--connectivity", type=int, nargs="+", default=[6, 26], choices=[6, 18, 26])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_components.py measures on an MI355X; there is nothing to time without one"
    L = mi355seg.lib()
    dev = torch.device("cuda:0")
    src = torch.empty(64 << 20, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    copy_gbps = 2 * src.numel() * 4 / (timed(lambda: dst.copy_(src), a.windows, a.window_s)["median"] * 1e-3) / 1e9
    del src, dst
    st = torch.cuda.current_stream().cuda_stream
    for n in a.sizes:
        numel = n ** 3
        need = L.query("mi355seg_components_ws_bytes", n, n, n)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        labels = torch.empty((n, n, n), dtype=torch.int32, device=dev)
        sizes = torch.empty(numel, dtype=torch.int32, device=dev)
        info = torch.empty(4, dtype=torch.int64, device=dev)
        out = torch.empty((n, n, n), dtype=torch.int64, device=dev)
        removed = torch.empty(1, dtype=torch.int64, device=dev)
        for kind in a.masks:
            mask = make_mask(kind, n)
            for conn in a.connectivity:
                structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn])
                lab, ncomp, counts, _ = host_path(mask, structure)
                got_l, got_s, got_i = F.connected_components(mask, conn)
                first = np.asarray(ndimage.minimum(np.arange(numel).reshape(lab.shape), lab, np.arange(1, ncomp + 1))).reshape(-1)
                assert np.array_equal(got_l.cpu().numpy(), np.concatenate([[0], first + 1])[lab]), "labels differ from scipy's"
                want_s = np.zeros(numel, dtype=np.int64)
                want_s[first] = counts[1:]
                assert np.array_equal(got_s.cpu().numpy(), want_s) and got_i.tolist()[:3] == [int(counts[1:].sum()), ncomp, int(counts[1:].max())]

                def prefix(k):
                    return lambda: L.call("mi355seg_components_label_steps_i64", mask.data_ptr(), n, n, n, conn, labels.data_ptr(),
                                          sizes.data_ptr(), info.data_ptr(), ws.data_ptr(), need, k, st)
                r_label = timed(lambda: L.call("mi355seg_components_label_i64", mask.data_ptr(), n, n, n, conn, labels.data_ptr(), sizes.data_ptr(),
                                               info.data_ptr(), ws.data_ptr(), need, st), a.windows, a.window_s)
                pre = [0.0] + [timed(prefix(k), a.windows, a.window_s)["median"] for k in range(1, 6)]
                step_ms = {STEPS[k]: pre[k + 1] - pre[k] for k in range(5)}
                r_filter = timed(lambda: L.call("mi355seg_components_filter_i64", mask.data_ptr(), labels.data_ptr(), sizes.data_ptr(), numel, 2,
                                                None, 0, out.data_ptr(), removed.data_ptr(), st), a.windows, a.window_s)
                r_call = host_timed(lambda: F.filter_components(mask, keep_largest=1, connectivity=conn), 10)
                r_host = host_timed(lambda: host_path(mask, structure), a.host_reps)
                flatten_gbps = 12 * numel / (step_ms["flatten"] * 1e-3) / 1e9
                filter_gbps = 20 * numel / (r_filter["median"] * 1e-3) / 1e9
                print(json.dumps({"volume": [n] * 3, "mask": kind, "connectivity": conn, "foreground": int(got_i[0]), "components": ncomp,
                                  "largest": int(got_i[2]), "label_ms": r_label, "local_ms": step_ms["local"], "merge_ms": step_ms["merge"],
                                  "flatten_ms": step_ms["flatten"], "info_ms": step_ms["info_reduce"] + step_ms["info_finalize"],
                                  "filter_ms": r_filter, "call_ms": r_call, "host_ms": r_host, "copy_gbps": copy_gbps,
                                  "flatten_gbps": flatten_gbps, "flatten_fraction_of_copy_rate": flatten_gbps / copy_gbps,
                                  "filter_gbps": filter_gbps, "filter_fraction_of_copy_rate": filter_gbps / copy_gbps}), flush=True)


if __name__ == "__main__":
    main()
