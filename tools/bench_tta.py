#!/usr/bin/env python3
"""Mirror test-time augmentation of the sliding-window inference (``predict.py ... config.tta=mirror``): what the two mirrored launches
cost beside their un-mirrored counterparts, and what a whole-volume prediction with 8 flips costs beside the same walk written with
``torch.flip`` and beside 8 un-augmented predictions, per (volume, patch, overlap, K).

Launches.  The batch is the first ``--batch`` patches of the grid.  The versions ALTERNATE within the process: every round times
one window (at least ``--window-s`` seconds of back-to-back calls, device events) of each version in turn, and a ratio is formed per
round, so drift of the machine hits both sides of a ratio alike.  Reported: the median (min .. max) over ``--rounds`` rounds.
  gather_ms["plain"], ["flip1"], ["flip6"], ["flip7"]   one launch of mi355seg_gather_patches_f32 / mi355seg_gather_patches_flip_f32
  accumulate_ms[...]                                     one launch of mi355seg_aggregate_patches_f32 / ..._flip_f32 (Hann window)
  *_ms["plain_again"]    the plain launch timed a second time in every round: plain_again / plain is the SPREAD of repeated plain
                         launches in this run, the yardstick for the ratios flipN / plain (``*_ratio_to_plain``)
Every timed call works on the next of several buffer sets, together larger than ``--cold-mib`` (default 1 GiB, four times the
Infinity Cache), so that no call finds its operands cached by the call before it.  A mirrored launch moves exactly the bytes of the
plain one (``*_bytes``: patches read and written; logits read, covered accumulator read and written).

Whole volume (``--no-walk`` skips it).  UNet3D(1, K, 32) in eval mode, fp32, Hann blending, batches of ``--batch``; one warm-up,
then ``--walk-rounds`` rounds of the three versions in turn, each timed once per round from its first launch to its finalise:
  walk_ms["tta"]         sliding_window_predict(tta_flips=(0..7)): the mirrors inside the gather and accumulate launches
  walk_ms["torch_flip"]  the same walk with mi355seg_gather_patches_f32, torch.flip of the patches, torch.flip of the logits and
                         mi355seg_aggregate_patches_f32: two extra tensor copies per batch and flip
  walk_ms["plain_x8"]    8 un-augmented sliding_window_predict calls: the forwards of the walk without any mirroring
Before anything is timed the mirrored launches are checked against torch.flip (bitwise) on the timed shapes.

usage: bench_tta.py [--cases 256,128,64 128,64,32] [--classes 2 4] [--batch 2] [--rounds 5] [--window-s 0.25] [--cold-mib 1024]
                    [--walk-rounds 3] [--no-walk]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mi355seg  # noqa: E402
from mi355seg import functional as F  # noqa: E402
from mi355seg.models.three_d.unet3d import UNet3D  # noqa: E402
from mi355seg.predict import axis_weight_sums, sliding_window_predict, tta_axis_sums, window_table, window_weights  # noqa: E402
from bench_aggregate import union_voxels  # noqa: E402

FLIPS = (1, 6, 7)                                    # x alone (the reversed quad), z and y (rows in another order), all three


def flip_dims(f):
    return tuple(d for d, bit in ((-3, 4), (-2, 2), (-1, 1)) if f & bit)


def summary(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def alternate(versions, rounds, window_s):
    """versions: {name: fn} -> {name: [ms per call, one per round]}; in every round each version runs one window, in turn"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = {}
    for name, fn in versions.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0.record(); fn(); t1.record()
        torch.cuda.synchronize()
        calls[name] = max(3, int(window_s * 1e3 / max(t0.elapsed_time(t1), 1e-3)) + 1)
    res = {name: [] for name in versions}
    for _ in range(rounds):
        for name, fn in versions.items():
            t0.record()
            for _ in range(calls[name]):
                fn()
            t1.record()
            torch.cuda.synchronize()
            res[name].append(t0.elapsed_time(t1) / calls[name])
    return res


def report(res, base="plain"):
    ms = {name: summary(v) for name, v in res.items()}
    ratio = {name: summary([a / b for a, b in zip(v, res[base])]) for name, v in res.items() if name != base}
    return ms, ratio


def flip_walk(model, vol, patch, overlap, batch, flips):
    """sliding_window_predict(overlap_mode='hann', tta_flips=flips) with torch.flip and the un-mirrored entry points"""
    size = tuple(vol.shape[1:])
    table_h = window_table(size, patch, overlap)
    table, P = torch.from_numpy(table_h).to(vol.device), table_h.shape[0]
    w64 = window_weights("hann", patch)
    w = [torch.from_numpy(v.astype(np.float32)).to(vol.device) for v in w64]
    sums = [torch.from_numpy(v.astype(np.float32)).to(vol.device) for v in axis_weight_sums(size, patch, overlap, w64)]
    acc = None
    with torch.no_grad():
        for f in flips:
            for i in range(0, P, batch):
                x = F.gather_patches(vol, table, i, min(batch, P - i), patch)
                logits = model(torch.flip(x, flip_dims(f)) if f else x).to(torch.float32)
                if acc is None:
                    acc = torch.zeros((logits.shape[1],) + size, dtype=torch.float32, device=vol.device)
                F.aggregate_patches(acc, torch.flip(logits, flip_dims(f)) if f else logits, table, i, w)
    return F.aggregate_finalize(acc, tta_axis_sums(sums, flips))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["256,128,64", "128,64,32"], help="volume,patch,overlap (cubes)")
    ap.add_argument("--classes", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--cold-mib", type=float, default=1024.0, help="timed calls rotate over buffer sets of at least this many MiB together")
    ap.add_argument("--walk-rounds", type=int, default=3)
    ap.add_argument("--no-walk", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tta.py measures on an MI355X; there is nothing to time without one"
    L = mi355seg.lib()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    for case in a.cases:
        n, p, o = (int(v) for v in case.split(","))
        size, patch, overlap = (n,) * 3, (p,) * 3, (o,) * 3
        table_h = window_table(size, patch, overlap)
        P, nb = table_h.shape[0], min(a.batch, table_h.shape[0])
        table = torch.from_numpy(table_h).to(dev)
        w = [torch.from_numpy(v.astype(np.float32)).to(dev) for v in window_weights("hann", patch)]
        covered = union_voxels(table_h[:nb], size, patch)
        turn = [0]

        # ---- the gather: one volume channel, as predict.py feeds the networks here
        g = torch.Generator(device=dev).manual_seed(n)
        sets = max(1, min(128, int(a.cold_mib * 2 ** 20 / (8.0 * nb * p ** 3)) + 1))
        vols = [torch.randn((1,) + size, device=dev, generator=g) for _ in range(sets)]
        outs = [torch.empty((nb, 1) + patch, device=dev) for _ in range(sets)]
        plain = F.gather_patches(vols[0], table, 0, nb, patch)
        for f in range(8):
            assert torch.equal(F.gather_patches(vols[0], table, 0, nb, patch, flip=f), torch.flip(plain, flip_dims(f)) if f else plain), f

        def gather(f):
            def call():
                turn[0] = j = (turn[0] + 1) % sets
                if f is None:
                    L.call("mi355seg_gather_patches_f32", vols[j].data_ptr(), 1, n, n, n, table.data_ptr(), 0, nb, p, p, p, outs[j].data_ptr(), st)
                else:
                    L.call("mi355seg_gather_patches_flip_f32", vols[j].data_ptr(), 1, n, n, n, table.data_ptr(), 0, nb, p, p, p, f,
                           outs[j].data_ptr(), st)
            return call

        versions = {"plain": gather(None), **{f"flip{f}": gather(f) for f in FLIPS}, "plain_again": gather(None)}
        g_ms, g_ratio = report(alternate(versions, a.rounds, a.window_s))
        print(json.dumps({"what": "gather", "volume": list(size), "patch": list(patch), "overlap": list(overlap), "batch": nb, "buffer_sets": sets,
                          "gather_bytes": 8.0 * nb * p ** 3, "gather_ms": g_ms, "gather_ratio_to_plain": g_ratio}), flush=True)
        del vols, outs, plain

        for K in a.classes:
            g = torch.Generator(device=dev).manual_seed(K)
            one_set = 4.0 * K * (nb * p ** 3 + covered)
            sets = max(1, min(128, int(a.cold_mib * 2 ** 20 / one_set) + 1))
            logits = [4.0 * torch.randn((nb, K) + patch, device=dev, generator=g) for _ in range(sets)]
            acc = [torch.zeros((K,) + size, device=dev) for _ in range(sets)]
            got, want = torch.zeros_like(acc[0]), torch.zeros_like(acc[0])
            for f in range(1, 8):                                # on the timed shape: the mirrored launch is the plain one on flipped logits
                F.aggregate_patches(got, logits[0], table, 0, w, flip=f)
                F.aggregate_patches(want, torch.flip(logits[0], flip_dims(f)), table, 0, w)
                assert torch.equal(got, want), f
            del got, want

            def accumulate(f):
                def call():
                    turn[0] = j = (turn[0] + 1) % sets
                    if f is None:
                        L.call("mi355seg_aggregate_patches_f32", logits[j].data_ptr(), K, table.data_ptr(), 0, nb, p, p, p,
                               w[0].data_ptr(), w[1].data_ptr(), w[2].data_ptr(), acc[j].data_ptr(), n, n, n, st)
                    else:
                        L.call("mi355seg_aggregate_patches_flip_f32", logits[j].data_ptr(), K, table.data_ptr(), 0, nb, p, p, p,
                               w[0].data_ptr(), w[1].data_ptr(), w[2].data_ptr(), f, acc[j].data_ptr(), n, n, n, st)
                return call

            versions = {"plain": accumulate(None), **{f"flip{f}": accumulate(f) for f in FLIPS}, "plain_again": accumulate(None)}
            a_ms, a_ratio = report(alternate(versions, a.rounds, a.window_s))
            row = {"what": "accumulate", "volume": list(size), "patch": list(patch), "overlap": list(overlap), "classes": K, "batch": nb,
                   "buffer_sets": sets, "covered_voxels": covered, "accumulate_bytes": 4.0 * K * (nb * p ** 3 + 2 * covered),
                   "accumulate_ms": a_ms, "accumulate_ratio_to_plain": a_ratio}
            print(json.dumps(row), flush=True)
            del logits, acc
            if a.no_walk:
                continue

            # ---- whole volume, 8 flips
            model = UNet3D(1, K, 32).to(dev).eval()
            vol = torch.randn((1,) + size, device=dev, generator=g)
            flips = F.tta_flip_codes()
            walks = {
                "tta": lambda: sliding_window_predict(model, vol, patch, overlap, batch_size=nb, overlap_mode="hann", tta_flips=flips),
                "torch_flip": lambda: flip_walk(model, vol, patch, overlap, nb, flips),
                "plain_x8": lambda: [sliding_window_predict(model, vol, patch, overlap, batch_size=nb, overlap_mode="hann") for _ in flips],
            }
            labels = {name: fn() for name, fn in walks.items() if name != "plain_x8"}          # warm-up, and the two must agree
            walks["plain_x8"]()
            differ = int((labels["tta"] != labels["torch_flip"]).sum())
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            res = {name: [] for name in walks}
            for _ in range(a.walk_rounds):
                for name, fn in walks.items():
                    torch.cuda.synchronize()
                    t0.record(); fn(); t1.record()
                    torch.cuda.synchronize()
                    res[name].append(t0.elapsed_time(t1))
            w_ms, w_ratio = report(res, base="tta")
            print(json.dumps({"what": "walk", "volume": list(size), "patch": list(patch), "overlap": list(overlap), "classes": K, "batch": nb,
                              "patches": P, "flips": len(flips), "forwards": len(flips) * P, "labels_differing_from_torch_flip_walk": differ,
                              "walk_ms": w_ms, "walk_ratio_to_tta": w_ratio,
                              "per_batch_ms": {name: v["median"] / (len(flips) * ((P + nb - 1) // nb)) for name, v in w_ms.items()}}), flush=True)
            del model, vol


if __name__ == "__main__":
    main()
