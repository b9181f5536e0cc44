#!/usr/bin/env python3
"""The label form of the fused tail (``config.multiclass``; functional.loss_tail_labels on a uint8 label map) beside what it
replaces: functional.one_hot_labels followed by the one-hot form (functional.loss_tail), in the same process, on the same logits
and labels -- forward + backward together (loss, mask, counters and d loss / d logits).

Per case (shape, mode), with device events after a warm-up; the versions alternate, ``--rounds`` windows of at least ``--window-s``
seconds each, and the median (min .. max) is reported:
  labels_us / onehot_us     one forward + backward of each form (the one-hot form includes building the one-hot target)
  onehot_tail_us            the one-hot form on a target built beforehand: the one-hot tail of the parent commit alone
  onehot_again_us           the one-hot form once more in every round: the same launches as onehot_us, timed again
  same_launch_spread        |onehot_again / onehot - 1| of the medians, and the largest (max - min) / median of the two: what
                            repeated identical launches differ by in this run -- a ratio inside it says nothing
  labels_over_onehot, labels_over_onehot_tail   the ratios of the medians (below 1: the label form is faster)
  not_slower                labels_us <= onehot_us * (1 + same_launch_spread): the condition of DESIGN.md 4.22
  min_bytes_*               what each form has to move (logits, target or labels, int64 mask forward; logits, target or labels,
                            gradient backward; the one-hot form also writes its target from the labels)
Every timed call works on the next of several buffer sets, together larger than ``--cold-mib`` (default 1 GiB, four times the
Infinity Cache), so that no call finds its operands cached by the call before it.  Before anything is timed the two forms' outputs
are compared bitwise.

usage: bench_multiclass.py [--cases 2,4,128,128,128:dice_ce 1,4,160,192,160:dice_ce 1,16,96,96,96:dice_ce] [--rounds 5]
                           [--window-s 0.25] [--cold-mib 1024]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mi355seg  # noqa: E402
from mi355seg import functional as F  # noqa: E402
from bench_components import timed  # noqa: E402


def spread(vals):
    return {"median": float(np.median(vals)), "min": float(min(vals)), "max": float(max(vals))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["2,4,128,128,128:dice_ce", "1,4,160,192,160:dice_ce", "1,16,96,96,96:dice_ce"],
                    help="N,K,D,H,W:mode")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--cold-mib", type=float, default=1024.0, help="timed calls rotate over buffer sets of at least this many MiB together")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_multiclass.py measures on an MI355X; there is nothing to time without one"
    mi355seg.lib()
    dev = torch.device("cuda:0")
    for case in a.cases:
        dims, mode = case.split(":")
        shape = tuple(int(v) for v in dims.split(","))
        N, K = shape[:2]
        M, V = int(np.prod(shape)), int(np.prod(shape)) // K
        spec = F.LossSpec.from_mode(mode)
        g = torch.Generator(device=dev).manual_seed(K)
        sets = max(2, min(64, int(a.cold_mib * 2 ** 20 / (12.0 * M)) + 1))           # logits, target and gradient of one call: 12 M bytes
        xs = [(3.0 * torch.randn(shape, device=dev, generator=g)).requires_grad_(True) for _ in range(sets)]
        labs = [torch.randint(0, K, (N,) + shape[2:], device=dev, generator=g).to(torch.uint8) for _ in range(sets)]
        ts = [F.one_hot_labels(l, K) for l in labs]
        turn = [0]

        def nxt():
            turn[0] = (turn[0] + 1) % sets
            return turn[0]

        def labels(j=None):
            j = nxt() if j is None else j
            loss, mask, counts, terms, cc = F.loss_tail_labels(xs[j], labs[j], spec)
            return loss, mask, counts, terms, torch.autograd.grad(loss, xs[j])[0]

        def onehot(j=None):
            j = nxt() if j is None else j
            loss, mask, counts, terms = F.loss_tail(xs[j], F.one_hot_labels(labs[j], K), spec)
            return loss, mask, counts, terms, torch.autograd.grad(loss, xs[j])[0]

        def onehot_tail():
            j = nxt()
            loss, mask, counts, terms = F.loss_tail(xs[j], ts[j], spec)
            return loss, mask, counts, terms, torch.autograd.grad(loss, xs[j])[0]

        for u, v in zip(labels(0), onehot(0)):
            assert torch.equal(u, v), "the label form and the one-hot form differ"
        res = {"labels": [], "onehot": [], "onehot_tail": [], "onehot_again": []}
        for r in range(a.rounds + 1):                            # alternating: what else runs on the host moves all alike
            for name, fn in (("labels", labels), ("onehot", onehot), ("onehot_tail", onehot_tail), ("onehot_again", onehot)):
                t = timed(fn, 1, a.window_s)["median"] * 1e3
                if r:                                            # (the first round brings the clocks up and is dropped)
                    res[name].append(t)
        la, oh, ot, oa = (spread(res[k]) for k in ("labels", "onehot", "onehot_tail", "onehot_again"))
        same = max(abs(oa["median"] / oh["median"] - 1.0), (oh["max"] - oh["min"]) / oh["median"], (oa["max"] - oa["min"]) / oa["median"])
        row = {"shape": list(shape), "mode": mode, "buffer_sets": sets,
               "labels_us": la, "onehot_us": oh, "onehot_tail_us": ot, "onehot_again_us": oa, "same_launch_spread": same,
               "labels_over_onehot": la["median"] / oh["median"], "labels_over_onehot_tail": la["median"] / ot["median"],
               "not_slower": bool(la["median"] <= oh["median"] * (1.0 + same)),
               "min_bytes_labels": 4.0 * M + 9.0 * V + 8.0 * M + 1.0 * V,
               "min_bytes_onehot": (4.0 * M + 1.0 * V) + 8.0 * M + 8.0 * V + 12.0 * M}
        print(json.dumps(row), flush=True)
        del xs, labs, ts


if __name__ == "__main__":
    main()
