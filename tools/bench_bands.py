#!/usr/bin/env python3
"""The IS network's frequency-band split (train.py:76-88,198-201) at the sizes the networks train at, both implementations in one
process: ``impl="fft"`` (torch.fft on rocFFT) and ``impl="device"`` (csrc/band.hip, one launch).

Per shape one JSON line.  After a warm-up of both paths, ``--rounds`` rounds alternate a window of ``--calls`` fft calls and a window
of ``--calls`` device calls, each window between two device events; per path the median (min .. max) of the windows' ms per call:
  fft_ms, device_ms   ms per call from the host (allocation of the two outputs and the Python around the launch included on both
                      sides: what an eager step pays; at the small shape this is the host's cost, not the kernel's)
  ratio               fft_ms / device_ms (medians)
  device_graph_ms     the device path's ``--calls`` launches captured once in a graph and replayed: the kernel alone, back to back
  device_gbps         the device path's compulsory traffic -- one read of x, one write each of low and high, 3 x the tensor -- over
                      device_graph_ms; copy_gbps is the float4-copy rate of the MI355X (6.29 TB/s) it stands beside
  max_abs_diff        max |device - fft| over both bands on the timed input (the two paths must agree before their times compare)

usage: bench_bands.py [--calls 30] [--rounds 5] [--shapes 1,1,64,64,64 ...]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mi355seg  # noqa: E402
from mi355seg.models.three_d.IS import frequency_bands  # noqa: E402

SHAPES = [(1, 1, 64, 64, 64), (2, 1, 128, 128, 128), (1, 1, 160, 192, 160)]
COPY_GBPS = 6290.0              # measured float4 copy, MI355X


def window(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=None, help="B,C,D,H,W ...")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bands.py measures on an MI355X; there is nothing to time without one"
    L = mi355seg.lib()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shapes] if a.shapes else SHAPES
    for shape in shapes:
        x = torch.randn(shape, device=dev, generator=gen)
        paths = {"fft": lambda: frequency_bands(x, impl="fft"), "device": lambda: frequency_bands(x, impl="device")}
        for fn in paths.values():                       # warm-up: code objects, rocFFT plans, the basis cache
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        diff = max(float((d - f).abs().max()) for d, f in zip(paths["device"](), paths["fft"]()))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(a.calls):
                paths["device"]()
        graph.replay()
        torch.cuda.synchronize()
        ms = {k: [] for k in list(paths) + ["graph"]}
        for _ in range(a.rounds):
            for k, fn in paths.items():
                ms[k].append(window(fn, a.calls))
            ms["graph"].append(window(graph.replay, 1) / a.calls)
        B, C, D, H, W = shape
        (_, rh, qh), (_, rw, qw) = (mi355seg.functional._band_basis_device(n, 0.04, dev) for n in (H, W))
        nbytes = 3 * 4 * x.numel()
        res = {"shape": list(shape), "calls_per_window": a.calls, "rounds": a.rounds, "fft_ms": spread(ms["fft"]),
               "device_ms": spread(ms["device"]), "ratio": float(np.median(ms["fft"]) / np.median(ms["device"])),
               "device_graph_ms": spread(ms["graph"]),
               "device_bytes": nbytes, "device_gbps": nbytes / (float(np.median(ms["graph"])) * 1e-3) / 1e9, "copy_gbps": COPY_GBPS,
               "modes": {"rH": rh, "qH": qh, "rW": rw, "qW": qw},
               "row_chunks": int(L.query("mi355seg_band_split_supported", B, C, D, H, W, rh, qh, rw, qw)), "max_abs_diff": diff}
        print(json.dumps(res), flush=True)
        del x, graph


if __name__ == "__main__":
    main()
