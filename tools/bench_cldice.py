#!/usr/bin/env python3
"""The soft-clDice term (csrc/cldice.hip; ``train.py ... config.cldice_weight=0.5``): its two stencil kernels beside the copy rate,
and the whole term beside the same term composed from ``torch.nn.functional.max_pool3d``, minima, subtractions and ReLUs on the
device (the official clDice formulation under autograd), in the same process, on the same logits and targets.

Per case (shape N,K,D,H,W and iters), device events after a warm-up; ``--rounds`` windows of at least ``--window-s`` seconds each,
the forms alternating, median (min .. max) reported:
  step_fwd_us / step_bwd_us        one level (j = 1: the general path) of the soft skeleton of P, forward / backward
  step_*_gbps, step_*_share_of_copy_rate   the bytes the level has to move -- forward 16 B / voxel (E_j and the skeleton in, E_{j+1}
                                   and the skeleton out), backward 28 B / voxel (E_j, E_{j+1}, the skeleton, two gradients in, two
                                   out) -- over its time, against ``copy_gbps``: what a device-to-device copy of 256 MiB moves in
                                   the same run (read + write bytes)
  device_us / composition_us       soft_cldice forward + backward (cldice and d cldice / d logits)
Every timed call works on the next of several buffer sets, together larger than ``--cold-mib`` (default 1 GiB, four times the
Infinity Cache), so that no call finds its operands cached by the call before it.  Before anything is timed the two forms' cldice
(1e-5 relative) and gradient (1e-3 of its maximum: float32 sums in the composition) are compared.

usage: bench_cldice.py [--cases 2,2,128,128,128:3 2,2,128,128,128:10 1,2,160,192,160:3 1,2,160,192,160:10] [--rounds 5]
                       [--window-s 0.25] [--cold-mib 1024]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as TF  # noqa: E402
import mi355seg  # noqa: E402
from mi355seg import functional as F  # noqa: E402
from bench_components import timed  # noqa: E402


def spread(vals):
    return {"median": float(np.median(vals)), "min": float(min(vals)), "max": float(max(vals))}


def torch_erode(x):
    p1 = -TF.max_pool3d(-x, (3, 1, 1), (1, 1, 1), (1, 0, 0))
    p2 = -TF.max_pool3d(-x, (1, 3, 1), (1, 1, 1), (0, 1, 0))
    p3 = -TF.max_pool3d(-x, (1, 1, 3), (1, 1, 1), (0, 0, 1))
    return torch.min(torch.min(p1, p2), p3)


def torch_open(x):
    return TF.max_pool3d(torch_erode(x), (3, 3, 3), (1, 1, 1), (1, 1, 1))


def torch_soft_skel(x, iters):
    skel = TF.relu(x - torch_open(x))
    for _ in range(iters):
        x = torch_erode(x)
        delta = TF.relu(x - torch_open(x))
        skel = skel + TF.relu(delta - skel * delta)
    return skel


def torch_cldice(logits, target, iters, smooth=1.0):
    P, T = torch.sigmoid(logits[:, 1:]), target[:, 1:]
    sp, st = torch_soft_skel(P, iters), torch_soft_skel(T, iters)
    tprec = ((sp * T).sum() + smooth) / (sp.sum() + smooth)
    tsens = ((st * P).sum() + smooth) / (st.sum() + smooth)
    return 1.0 - 2.0 * tprec * tsens / (tprec + tsens)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["2,2,128,128,128:3", "2,2,128,128,128:10", "1,2,160,192,160:3", "1,2,160,192,160:10"],
                    help="N,K,D,H,W:iters")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--cold-mib", type=float, default=1024.0, help="timed calls rotate over buffer sets of at least this many MiB together")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cldice.py measures on an MI355X; there is nothing to time without one"
    L = mi355seg.lib()
    dev = torch.device("cuda:0")
    src = torch.empty(64 << 20, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    copy_gbps = 2 * src.numel() * 4 / (timed(lambda: dst.copy_(src), 3, a.window_s)["median"] * 1e-3) / 1e9
    del src, dst
    stream = torch.cuda.current_stream().cuda_stream
    for case in a.cases:
        dims, iters = case.split(":")
        shape, iters = tuple(int(v) for v in dims.split(",")), int(iters)
        N, K, D, H, W = shape
        assert K >= 2, "the composition drops the background channel: K >= 2"
        vox = N * (K - 1) * D * H * W
        cold = a.cold_mib * 2 ** 20
        g = torch.Generator(device=dev).manual_seed(K + iters)

        # ---- one level of the skeleton: stacks filled by a whole forward, then level 1 again and again, each call on the next stack
        stack_bytes = L.query("mi355seg_soft_skel_ws_bytes", N * (K - 1), D, H, W, iters)
        sets = max(2, min(32, int(cold / (16.0 * vox)) + 1))
        P = [torch.sigmoid(3.0 * torch.randn((N, K - 1, D, H, W), device=dev, generator=g)) for _ in range(sets)]
        stacks = [F._skel_forward(p, iters)[0] for p in P]
        grads = [[torch.randn_like(P[0]) for _ in range(2)] + [torch.empty_like(P[0]) for _ in range(2)] for _ in range(sets)]
        turn = [0]

        def nxt(n):
            turn[0] = (turn[0] + 1) % n
            return turn[0]

        def step_fwd():
            j = nxt(sets)
            L.call("mi355seg_soft_skel_step_fwd_f32", P[j].data_ptr(), N * (K - 1), D, H, W, iters, 1, stacks[j].data_ptr(), stack_bytes, stream)

        def step_bwd():
            j = nxt(sets)
            gs, ge, oe, os_ = grads[j]
            L.call("mi355seg_soft_skel_step_bwd_f32", P[j].data_ptr(), gs.data_ptr(), ge.data_ptr(), oe.data_ptr(), os_.data_ptr(),
                   N * (K - 1), D, H, W, iters, 1, stacks[j].data_ptr(), stack_bytes, stream)

        res = {"step_fwd": [], "step_bwd": []}
        for _ in range(a.rounds):
            for name, fn in (("step_fwd", step_fwd), ("step_bwd", step_bwd)):
                res[name].append(timed(fn, 1, a.window_s)["median"] * 1e3)
        sf, sb = spread(res["step_fwd"]), spread(res["step_bwd"])
        del P, stacks, grads

        # ---- the whole term, forward + backward, beside the composition
        M = N * K * D * H * W
        tsets = max(2, min(16, int(cold / (12.0 * M)) + 1))
        xs = [(3.0 * torch.randn(shape, device=dev, generator=g)).requires_grad_(True) for _ in range(tsets)]
        ts = []
        for _ in range(tsets):                               # a few thick random tubes along x: something with a centre line
            fg = (TF.avg_pool3d(torch.rand((N, 1, D, H, W), device=dev, generator=g), (5, 5, 9), 1, (2, 2, 4)) > 0.53).float()
            ts.append(torch.cat([1.0 - fg, fg], dim=1) if K == 2 else torch.cat([1.0 - fg] + [fg] * (K - 1), dim=1))

        def device(j=None):
            j = nxt(tsets) if j is None else j
            loss, _ = F.soft_cldice(xs[j], ts[j], iters)
            return loss, torch.autograd.grad(loss, xs[j])[0]

        def composition(j=None):
            j = nxt(tsets) if j is None else j
            loss = torch_cldice(xs[j], ts[j], iters)
            return loss, torch.autograd.grad(loss, xs[j])[0]

        ld, gd = device(0)
        lc, gc = composition(0)
        assert abs(float(ld) - float(lc)) <= 1e-5 * max(1.0, abs(float(lc))), (float(ld), float(lc))
        assert float((gd - gc).abs().max()) <= 1e-3 * float(gc.abs().max()), (float((gd - gc).abs().max()), float(gc.abs().max()))
        del ld, gd, lc, gc
        res = {"device": [], "composition": []}
        for _ in range(a.rounds):                                # alternating: what else runs on the host moves both alike
            for name, fn in (("device", device), ("composition", composition)):
                res[name].append(timed(fn, 1, a.window_s)["median"] * 1e3)
        de, co = spread(res["device"]), spread(res["composition"])
        fwd_gbps, bwd_gbps = 16.0 * vox / (sf["median"] * 1e-6) / 1e9, 28.0 * vox / (sb["median"] * 1e-6) / 1e9
        row = {"shape": list(shape), "iters": iters, "skeleton_voxels": vox, "buffer_sets": [sets, tsets], "copy_gbps": copy_gbps,
               "step_fwd_us": sf, "step_fwd_gbps": fwd_gbps, "step_fwd_share_of_copy_rate": fwd_gbps / copy_gbps,
               "step_bwd_us": sb, "step_bwd_gbps": bwd_gbps, "step_bwd_share_of_copy_rate": bwd_gbps / copy_gbps,
               "device_us": de, "composition_us": co, "composition_over_device": co["median"] / de["median"],
               "saved_for_backward_bytes": stack_bytes}
        print(json.dumps(row), flush=True)
        del xs, ts


if __name__ == "__main__":
    main()
