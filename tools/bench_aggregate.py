#!/usr/bin/env python3
"""Soft sliding-window aggregation on the device (csrc/aggregate.hip; ``predict.py ... config.overlap_mode=hann``): what the two
launches cost, beside the crop path they stand in for and the forward whose output they aggregate, per (volume, patch, overlap, K).

The batch is the first ``--batch`` patches of the grid (neighbours along x, so with an overlap they cover common voxels and the
ordered walk runs).  With device events after a warm-up, the median (min .. max) of ``--windows`` windows of at least ``--window-s``
seconds each:
  accumulate_ms   the one launch of mi355seg_aggregate_patches_f32 for the batch (Hann window, logits 4 * randn)
  finalize_ms     the one launch of mi355seg_aggregate_finalize_f32 for the volume, labels and probabilities written;
  finalize_labels_ms  the same with prob = NULL
  crop_ms         what the crop mode does for the same batch: mi355seg_argmax_ch_f32 and mi355seg_paste_labels_i64
  forward_ms      the eval-mode forward of UNet3D(1, K, 32) on the batch (fp32), the producer of those logits
  *_gbps, *_fraction_of_copy_rate: the algorithmic bytes over the time, against ``copy_gbps``, what a device-to-device copy of 256 MiB
                  moves here (read + write bytes).  accumulate: the logits read plus one read and one write of the accumulator under
                  the union of the batch's patches; finalize: acc read, labels written, probabilities written.
  accumulate_share_of_forward: accumulate_ms / forward_ms
Every timed call of the four above works on the next of several buffer sets, together larger than ``--cold-mib`` (default 1 GiB, four
times the Infinity Cache), so that no call finds its operands cached by the call before it.
Before anything is timed the finalised probabilities of one pass over the whole grid are checked to sum to 1.

usage: bench_aggregate.py [--cases 256,128,64 128,64,32] [--classes 2 4] [--batch 2] [--windows 5] [--window-s 0.25] [--cold-mib 1024]
                          [--no-forward]"""
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
from mi355seg.predict import axis_weight_sums, window_table, window_weights  # noqa: E402
from bench_components import timed  # noqa: E402


def union_voxels(table, size, patch):
    """voxels of the volume under at least one of the table's patches"""
    seen = np.zeros(size, dtype=bool)
    for z, y, x in table[:, :3]:
        seen[z:z + patch[0], y:y + patch[1], x:x + patch[2]] = True
    return int(seen.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["256,128,64", "128,64,32"], help="volume,patch,overlap (cubes)")
    ap.add_argument("--classes", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--cold-mib", type=float, default=1024.0, help="timed calls rotate over buffer sets of at least this many MiB together")
    ap.add_argument("--no-forward", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_aggregate.py measures on an MI355X; there is nothing to time without one"
    L = mi355seg.lib()
    dev = torch.device("cuda:0")
    src = torch.empty(64 << 20, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    copy_gbps = 2 * src.numel() * 4 / (timed(lambda: dst.copy_(src), a.windows, a.window_s)["median"] * 1e-3) / 1e9
    del src, dst
    st = torch.cuda.current_stream().cuda_stream
    for case in a.cases:
        n, p, o = (int(v) for v in case.split(","))
        size, patch, overlap = (n,) * 3, (p,) * 3, (o,) * 3
        table_h = window_table(size, patch, overlap)
        P, nb = table_h.shape[0], min(a.batch, table_h.shape[0])
        table = torch.from_numpy(table_h).to(dev)
        w64 = window_weights("hann", patch)
        w = [torch.from_numpy(v.astype(np.float32)).to(dev) for v in w64]
        sums = [torch.from_numpy(v.astype(np.float32)).to(dev) for v in axis_weight_sums(size, patch, overlap, w64)]
        covered = union_voxels(table_h[:nb], size, patch)
        for K in a.classes:
            g = torch.Generator(device=dev).manual_seed(K)
            # every timed call works on the next of `sets` buffer sets, together larger than --cold-mib: a call never finds its
            # operands in the 256 MiB Infinity Cache because the call before it left them there
            one_set = 4.0 * K * (nb * p ** 3 + covered)           # the smallest footprint of the four: what accumulate touches
            sets = max(1, min(128, int(a.cold_mib * 2 ** 20 / one_set) + 1))
            logits = [4.0 * torch.randn((nb, K) + patch, device=dev, generator=g) for _ in range(sets)]
            acc = [torch.zeros((K,) + size, device=dev) for _ in range(sets)]
            for i in range(P):                                   # one pass over the whole grid with the same logits: a sanity check
                F.aggregate_patches(acc[0], logits[0][:1], table, i, w)
            labels, prob = F.aggregate_finalize(acc[0], sums, probabilities=True)
            assert float((prob.sum(0) - 1).abs().max()) <= 1e-5 and bool(torch.isfinite(prob).all())
            acc[0].zero_()
            labels, prob = [torch.empty_like(labels) for _ in range(sets)], [torch.empty_like(prob) for _ in range(sets)]
            out = torch.zeros(size, dtype=torch.int64, device=dev)
            turn = [0]

            def nxt():
                turn[0] = (turn[0] + 1) % sets
                return turn[0]

            def accumulate():
                j = nxt()
                L.call("mi355seg_aggregate_patches_f32", logits[j].data_ptr(), K, table.data_ptr(), 0, nb, p, p, p,
                       w[0].data_ptr(), w[1].data_ptr(), w[2].data_ptr(), acc[j].data_ptr(), n, n, n, st)

            def finalize(with_prob):
                j = nxt()
                L.call("mi355seg_aggregate_finalize_f32", acc[j].data_ptr(), K, n, n, n, sums[0].data_ptr(), sums[1].data_ptr(),
                       sums[2].data_ptr(), labels[j].data_ptr(), prob[j].data_ptr() if with_prob else None, st)

            def crop():
                lab = F.argmax_channels(logits[nxt()])
                L.call("mi355seg_paste_labels_i64", lab.data_ptr(), table.data_ptr(), 0, nb, p, p, p, out.data_ptr(), n, n, n, st)

            r_acc = timed(accumulate, a.windows, a.window_s)
            r_fin = timed(lambda: finalize(True), a.windows, a.window_s)
            r_lab = timed(lambda: finalize(False), a.windows, a.window_s)
            r_crop = timed(crop, a.windows, a.window_s)
            acc_bytes = 4.0 * K * (nb * p ** 3 + 2 * covered)
            fin_bytes = (8.0 * K + 8.0) * n ** 3
            lab_bytes = (4.0 * K + 8.0) * n ** 3
            row = {"volume": list(size), "patch": list(patch), "overlap": list(overlap), "classes": K, "patches": P, "batch": nb, "buffer_sets": sets,
                   "covered_voxels": covered, "copy_gbps": copy_gbps, "accumulate_ms": r_acc, "finalize_ms": r_fin,
                   "finalize_labels_ms": r_lab, "crop_ms": r_crop}
            for name, nbytes, r in (("accumulate", acc_bytes, r_acc), ("finalize", fin_bytes, r_fin), ("finalize_labels", lab_bytes, r_lab)):
                gbps = nbytes / (r["median"] * 1e-3) / 1e9
                row[name + "_gbps"], row[name + "_fraction_of_copy_rate"] = gbps, gbps / copy_gbps
            if not a.no_forward:
                model = UNet3D(1, K, 32).to(dev).eval()
                x = torch.randn((nb, 1) + patch, device=dev, generator=g)
                with torch.no_grad():
                    r_fwd = timed(lambda: model(x), a.windows, a.window_s)
                row["forward_ms"] = r_fwd
                row["accumulate_share_of_forward"] = r_acc["median"] / r_fwd["median"]
                del model, x
            print(json.dumps(row), flush=True)
            del logits, acc, labels, prob, out


if __name__ == "__main__":
    main()
