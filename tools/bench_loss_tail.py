#!/usr/bin/env python3
"""The fused tail of the compound losses (csrc/loss_tail.hip; ``train.py ... config.loss=dice_bce``) beside the composition it
replaces: the ``criterion=`` branch of engine.train_step on the library losses -- the criterion, ``argmax_channels`` twice,
``dice_counts``, and the backward of the criterion -- in the same process, on the same logits and targets.

Per case (shape, mode), forward + backward together (loss, mask, counters and d loss / d logits), with device events after a
warm-up; the two forms alternate, ``--rounds`` windows of at least ``--window-s`` seconds each, and the median (min .. max) is
reported:
  fused_us / composition_us    one forward + backward
  fused_fwd_us / fused_bwd_us  the two halves of the fused form (the forward alone, under no_grad; the backward as the difference)
  launches_*                   device kernels of one forward + backward, counted with torch.profiler in a pass of its own (null in a
                               torch build without the profiler); the timed windows run with the profiler off
  min_bytes                    what the fused form has to move: 8 M + 8 V forward (logits, target; the int64 mask), 12 M backward
                               (logits, target; the gradient), M = N K S, V = N S
  fused_gbps, fused_share_of_copy_rate   min_bytes over fused_us, against ``copy_gbps``: what a device-to-device copy of 256 MiB
                               moves in the same run (read + write bytes)
Every timed call works on the next of several buffer sets, together larger than ``--cold-mib`` (default 1 GiB, four times the
Infinity Cache), so that no call finds its operands cached by the call before it.  Before anything is timed the two forms' loss and
gradient are compared (1e-6 relative, 2 * (1e-9 + 2e-5 max|grad|)).

usage: bench_loss_tail.py [--cases 2,2,128,128,128:dice_bce 1,4,160,192,160:dice_ce] [--rounds 5] [--window-s 0.25] [--cold-mib 1024]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mi355seg  # noqa: E402
from mi355seg import functional as F  # noqa: E402
from mi355seg.utils import loss_function as LF  # noqa: E402
from bench_components import timed  # noqa: E402


def count_launches(fn):
    """device kernels of one call of ``fn`` (after a warm-up call), or None in a torch build without the profiler; an error of the
    profiler or of ``fn`` itself is not caught"""
    try:
        from torch.profiler import ProfilerActivity, profile
    except ImportError:
        return None
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and not e.name.lower().startswith("memcpy"))
    return n or None


def spread(vals):
    return {"median": float(np.median(vals)), "min": float(min(vals)), "max": float(max(vals))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["2,2,128,128,128:dice_bce", "1,4,160,192,160:dice_ce"], help="N,K,D,H,W:mode")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--cold-mib", type=float, default=1024.0, help="timed calls rotate over buffer sets of at least this many MiB together")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_loss_tail.py measures on an MI355X; there is nothing to time without one"
    mi355seg.lib()
    dev = torch.device("cuda:0")
    src = torch.empty(64 << 20, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    copy_gbps = 2 * src.numel() * 4 / (timed(lambda: dst.copy_(src), 3, a.window_s)["median"] * 1e-3) / 1e9
    del src, dst
    for case in a.cases:
        dims, mode = case.split(":")
        shape = tuple(int(v) for v in dims.split(","))
        N, K = shape[:2]
        M, V = int(np.prod(shape)), int(np.prod(shape)) // K
        if mode not in ("dice_bce", "dice_ce"):
            raise SystemExit(f"{case}: the composition is defined for dice_bce and dice_ce (the library has no focal or Tversky loss)")
        crit = LF.CompoundLoss(mode)
        g = torch.Generator(device=dev).manual_seed(K)
        sets = max(2, min(64, int(a.cold_mib * 2 ** 20 / (12.0 * M)) + 1))           # logits, target and gradient of one call: 12 M bytes
        xs = [(3.0 * torch.randn(shape, device=dev, generator=g)).requires_grad_(True) for _ in range(sets)]
        labs = [torch.randint(0, K, (N,) + shape[2:], device=dev, generator=g) for _ in range(sets)]
        ts = [torch.stack([(l == i) for i in range(K)], dim=1).float() for l in labs]
        turn = [0]

        def nxt():
            turn[0] = (turn[0] + 1) % sets
            return turn[0]

        def fused(j=None):
            j = nxt() if j is None else j
            loss, mask, counts, _ = crit.tail(xs[j], ts[j])
            return loss, mask, counts, torch.autograd.grad(loss, xs[j])[0]

        def fused_fwd():
            j = nxt()
            with torch.no_grad():
                return crit.tail(xs[j], ts[j])

        def composition(j=None):
            j = nxt() if j is None else j
            if mode == "dice_bce":
                loss = LF.DiceLoss()(xs[j], ts[j]) + LF.BCEWithLogitsLoss()(xs[j], ts[j])
            else:
                loss = LF.cross_entropy_3D(xs[j], labs[j]) + LF.DiceLoss()(xs[j], ts[j])
            with torch.no_grad():
                mask = F.argmax_channels(xs[j])
                counts = F.dice_counts(F.argmax_channels(ts[j]), mask)
            return loss, mask, counts, torch.autograd.grad(loss, xs[j])[0]

        lf, mf, cf, gf = fused(0)
        lc, mc, cc, gc = composition(0)
        assert abs(float(lf) - float(lc)) <= 2e-6 * max(1.0, abs(float(lc))), (float(lf), float(lc))
        assert float((gf - gc).abs().max()) <= 2 * (1e-9 + 2e-5 * float(gc.abs().max()))
        assert torch.equal(mf, mc) and torch.equal(cf, cc)
        del lf, mf, cf, gf, lc, mc, cc, gc
        launches = {"fused": count_launches(lambda: fused(0)), "composition": count_launches(lambda: composition(0))}
        res = {"fused": [], "composition": [], "fused_fwd": []}
        for _ in range(a.rounds):                                # alternating: what else runs on the host moves both alike
            for name, fn in (("fused", fused), ("composition", composition), ("fused_fwd", fused_fwd)):
                res[name].append(timed(fn, 1, a.window_s)["median"] * 1e3)
        min_bytes = 8.0 * M + 8.0 * V + 12.0 * M
        fu, co, ff = spread(res["fused"]), spread(res["composition"]), spread(res["fused_fwd"])
        gbps = min_bytes / (fu["median"] * 1e-6) / 1e9
        row = {"shape": list(shape), "mode": mode, "buffer_sets": sets, "copy_gbps": copy_gbps,
               "launches_fused": launches["fused"], "launches_composition": launches["composition"],
               "fused_us": fu, "composition_us": co, "fused_fwd_us": ff, "fused_bwd_us": fu["median"] - ff["median"],
               "composition_over_fused": co["median"] / fu["median"], "min_bytes": min_bytes,
               "fused_gbps": gbps, "fused_share_of_copy_rate": gbps / copy_gbps}
        print(json.dumps(row), flush=True)
        del xs, labs, ts


if __name__ == "__main__":
    main()
