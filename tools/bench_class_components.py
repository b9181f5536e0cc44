#!/usr/bin/env python3
"""Per-class connected components on the device (csrc/components.hip; functional.connected_components_by_class /
component_table / filter_components_by_class) against the two routes a multi-class user had before, per (volume, K, mask,
connectivity).  K counts the classes with the background, as ``config.out_classes``: K - 1 foreground classes.

Masks: ``smooth``, the argmax of K smoothed random fields (a few large components per class, the shape of a multi-organ
prediction); ``speckle``, independent voxels at density 0.31 with a class drawn uniformly from 1..K-1.

Every device time is CACHE-COLD: before each timed call a 512 MiB buffer is overwritten (twice the last-level cache), then one call
between two device events; the median (min .. max) of ``--reps`` such calls.
  label_ms       the whole mi355seg_components_label_classes_i64 call (a 64-byte clear and five launches)
  local_ms .. info_ms   each launch on its own, as the difference of two prefixes of the call (..._label_classes_steps_i64)
  table_ms       mi355seg_components_table_i64: count, scan, table, relabel (four launches)
  filter_ms      the one launch of mi355seg_components_filter_table_i64 (every second component kept)
  binary_ms      what the parent commit can do: K - 1 calls of mi355seg_components_label_i64, one per class mask ``mask == k``, the
                 class masks built beforehand; binary_with_masks_ms builds each of them (``(mask == k).to(int64)``) inside the time
  call_ms        functional.filter_components_by_class(mask, keep_largest=1) with its host reads (host clock)
  host_ms        the host route: mask to the host, scipy.ndimage.label of every ``mask == k``, the labels back (host clock; ONE run per row
                 unless --host-reps says more)
  fractions of the copy rate: flatten (12 bytes per voxel), table (4 + 4 + 8) and filter (20) over their times, against copy_gbps, a
                 device-to-device copy of 256 MiB measured the same cache-cold way (read + write bytes)
The component count is asserted equal to scipy's before anything is timed.

usage: bench_class_components.py [--sizes 128 256] [--classes 2 4 16] [--masks smooth speckle] [--connectivity 6 26] [--reps 15]
                                 [--host-reps 1]"""
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

STEPS = ("local", "merge", "flatten", "info_reduce", "info_finalize")


class Cold:
    """device-event time of single calls, each behind a write of 512 MiB that pushes the call's operands out of the caches"""

    def __init__(self, reps):
        self.reps = reps
        self.scrub = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
        self.t0, self.t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def __call__(self, fn):
        fn()
        res = []
        for i in range(self.reps):
            self.scrub.fill_(i & 1)
            self.t0.record()
            fn()
            self.t1.record()
            torch.cuda.synchronize()
            res.append(self.t0.elapsed_time(self.t1))
        return {"median": float(np.median(res)), "min": min(res), "max": max(res), "calls": self.reps}


def host_timed(fn, reps):
    res = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        res.append((time.perf_counter() - t) * 1e3)
    return {"median": float(np.median(res)), "min": min(res), "max": max(res), "calls": reps}


def make_mask(kind, n, K, seed=5):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if kind == "speckle":
        fg = torch.rand((n, n, n), device="cuda", generator=g) < 0.31
        return (fg * torch.randint(1, K, (n, n, n), device="cuda", generator=g)).to(torch.int64)
    fields = torch.randn((K, 1, n, n, n), device="cuda", generator=g)
    for _ in range(3):                                   # three box filters of 9: close to a Gaussian of sigma 4.5
        fields = torch.nn.functional.avg_pool3d(fields, 9, 1, 4, count_include_pad=False)
    return fields[:, 0].argmax(0).to(torch.int64).contiguous()


def host_path(mask, K, structure):
    m = mask.cpu().numpy()
    total, labs = 0, []
    for k in range(1, K):
        lab, n = ndimage.label(m == k, structure)
        total += n
        labs.append(torch.from_numpy(lab).cuda())
    torch.cuda.synchronize()
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--classes", type=int, nargs="+", default=[2, 4, 16])
    ap.add_argument("--masks", nargs="+", default=["smooth", "speckle"], choices=["smooth", "speckle"])
    ap.add_argument("--connectivity", type=int, nargs="+", default=[6, 26], choices=[6, 18, 26])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_class_components.py measures on an MI355X; there is nothing to time without one"
    L = mi355seg.lib()
    dev = torch.device("cuda:0")
    cold = Cold(a.reps)
    src = torch.empty(64 << 20, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    copy_gbps = 2 * src.numel() * 4 / (cold(lambda: dst.copy_(src))["median"] * 1e-3) / 1e9
    del src, dst
    st = torch.cuda.current_stream().cuda_stream
    for n in a.sizes:
        numel = n ** 3
        need, need_bin = L.query("mi355seg_components_classes_ws_bytes", n, n, n), L.query("mi355seg_components_ws_bytes", n, n, n)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        tws = torch.empty(L.query("mi355seg_components_table_ws_bytes", numel), dtype=torch.uint8, device=dev)
        labels = torch.empty((n, n, n), dtype=torch.int32, device=dev)
        lc = torch.empty((n, n, n), dtype=torch.int32, device=dev)
        sizes = torch.empty(numel, dtype=torch.int32, device=dev)
        info = torch.empty(8, dtype=torch.int64, device=dev)
        out = torch.empty((n, n, n), dtype=torch.int64, device=dev)
        one = torch.empty((n, n, n), dtype=torch.int64, device=dev)
        removed = torch.empty(1, dtype=torch.int64, device=dev)
        for K in a.classes:
            for kind in a.masks:
                mask = make_mask(kind, n, K)
                per_class = [(mask == k).to(torch.int64) for k in range(1, K)]
                for conn in a.connectivity:
                    structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn])
                    counts = []
                    r_host = host_timed(lambda: counts.append(host_path(mask, K, structure)), a.host_reps)
                    got = F.connected_components_by_class(mask, conn)
                    ncomp = int(got[2][1])
                    assert ncomp == counts[-1], "the component count differs from scipy's"
                    first = torch.empty(ncomp, dtype=torch.int32, device=dev)
                    size = torch.empty(ncomp, dtype=torch.int32, device=dev)
                    cls = torch.empty(ncomp, dtype=torch.int64, device=dev)
                    keep = (torch.arange(ncomp, device=dev) % 2).to(torch.uint8)

                    def label(k=5):
                        L.call("mi355seg_components_label_classes_steps_i64", mask.data_ptr(), n, n, n, conn, labels.data_ptr(), sizes.data_ptr(),
                               info.data_ptr(), ws.data_ptr(), need, k, st)

                    def binary(build):
                        for k, m in enumerate(per_class, start=1):
                            if build:
                                m = one.copy_(mask == k)
                            L.call("mi355seg_components_label_i64", m.data_ptr(), n, n, n, conn, labels.data_ptr(), sizes.data_ptr(),
                                   info.data_ptr(), ws.data_ptr(), need_bin, st)

                    pre = [0.0] + [cold(lambda k=k: label(k))["median"] for k in range(1, 6)]
                    step_ms = {STEPS[k]: pre[k + 1] - pre[k] for k in range(5)}
                    r_binary, r_masks = cold(lambda: binary(False)), cold(lambda: binary(True))
                    r_label = cold(label)                   # last: labels, sizes and info are the class-aware ones from here on
                    r_table = cold(lambda: L.call("mi355seg_components_table_i64", mask.data_ptr(), labels.data_ptr(), sizes.data_ptr(), numel, ncomp,
                                                  lc.data_ptr(), first.data_ptr(), size.data_ptr(), cls.data_ptr(), tws.data_ptr(), tws.numel(), st))
                    r_filter = cold(lambda: L.call("mi355seg_components_filter_table_i64", mask.data_ptr(), lc.data_ptr(), keep.data_ptr(), ncomp,
                                                   numel, out.data_ptr(), removed.data_ptr(), st))
                    r_call = host_timed(lambda: F.filter_components_by_class(mask, keep_largest=1, connectivity=conn), 5)
                    gbps = lambda nbytes, ms: nbytes * numel / (ms * 1e-3) / 1e9
                    fl, tb, fi = gbps(12, step_ms["flatten"]), gbps(16, r_table["median"]), gbps(20, r_filter["median"])
                    print(json.dumps({"volume": [n] * 3, "classes": K, "mask": kind, "connectivity": conn, "foreground": int(got[2][0]),
                                      "components": ncomp, "largest": int(got[2][2]), "label_ms": r_label, "local_ms": step_ms["local"],
                                      "merge_ms": step_ms["merge"], "flatten_ms": step_ms["flatten"],
                                      "info_ms": step_ms["info_reduce"] + step_ms["info_finalize"], "table_ms": r_table, "filter_ms": r_filter,
                                      "binary_calls": K - 1, "binary_ms": r_binary, "binary_with_masks_ms": r_masks, "call_ms": r_call,
                                      "host_ms": r_host, "copy_gbps": copy_gbps, "flatten_fraction_of_copy_rate": fl / copy_gbps,
                                      "table_fraction_of_copy_rate": tb / copy_gbps, "filter_fraction_of_copy_rate": fi / copy_gbps}), flush=True)
                del per_class


if __name__ == "__main__":
    main()
