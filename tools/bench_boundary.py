#!/usr/bin/env python3
"""The boundary loss term (csrc/boundary.hip; ``train.py ... config.boundary_weight=0.5``): the three passes of the signed distance
map beside the copy rate and the fp32 rate, the loss forward + backward, the predict-time fp64 EDT (``mi355seg_edt3d_f64``) and
scipy on the same masks for scale, and a ``dice_bce`` train step with and without the term.

Per case (shape N,K,D,H,W), device events after a warm-up; ``--rounds`` windows of at least ``--window-s`` seconds each, median
(min .. max) reported:
  pass_w_us / pass_h_us / pass_d_us   one launch each, as the difference of two prefixes of the call (mi355seg_sdm_steps_f32)
  pass_*_gbps, *_share_of_copy_rate   the bytes the pass has to move per voxel of phi -- W: 4 in (target), 4 out (two uint16 offsets);
                                      H: 4 in, 8 out (two fp32 squared distances); D: 8 + 4 in (both polarities, target), 4 out (phi)
                                      -- over its time, against ``copy_gbps``: what a device-to-device copy of 256 MiB moves in the
                                      same run (read + write bytes)
  pass_h_gpairs / pass_d_gpairs       min-plus pair operations (one d * d + f and one minimum) per second: voxels x H x 2
                                      polarities, voxels x D x 1
  map_us                              the whole map (three launches)
  loss_fwd_us / loss_bwd_us           mi355seg_boundary_fwd_f32 (pass + finalise) and mi355seg_boundary_bwd_f32 on a finished map
  term_us                             functional.boundary_loss forward + backward (map, loss, gradient) under autograd
  edt3d_f64_us                        the predict-time EDT on ONE (n, k) volume of the same masks, both polarities (squared distances
                                      into a box, fp64), and that time x the volumes of the case
  scipy_ms                            scipy.ndimage.distance_transform_edt twice (inside, outside) on one (n, k) volume, on the host
  step_ms / step_with_term_ms         engine.train_step of UNet3D(1, 2, 32) with CompoundLoss("dice_bce"), without / with
                                      boundary_weight=0.5 (first case only, K = 2)
Every timed call works on the next of several buffer sets, together larger than ``--cold-mib`` (default 1 GiB, four times the
Infinity Cache), so that no call finds its operands cached by the call before it.  Before anything is timed the map of the first
volume is compared with scipy's (2e-6 relative).

usage: bench_boundary.py [--cases 2,2,128,128,128 1,4,160,192,160] [--rounds 5] [--window-s 0.25] [--cold-mib 1024] [--no-step]"""
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
from bench_components import host_timed, timed  # noqa: E402


def spread(vals):
    return {"median": float(np.median(vals)), "min": float(min(vals)), "max": float(max(vals))}


def tubes(N, K, D, H, W, dev, g):
    """a one-hot target [N, K, D, H, W]: thick random blobs, split among the foreground classes by position along x"""
    fg = TF.avg_pool3d(torch.rand((N, 1, D, H, W), device=dev, generator=g), (5, 5, 9), 1, (2, 2, 4)) > 0.53
    if K == 1:
        return fg.float()
    band = (torch.arange(W, device=dev) * (K - 1) // W + 1).view(1, 1, 1, 1, W)
    lab = torch.where(fg, band.expand(N, 1, D, H, W), torch.zeros((), dtype=torch.long, device=dev))
    return torch.cat([(lab == k).float() for k in range(K)], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["2,2,128,128,128", "1,4,160,192,160"], help="N,K,D,H,W")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--cold-mib", type=float, default=1024.0, help="timed calls rotate over buffer sets of at least this many MiB together")
    ap.add_argument("--no-step", action="store_true", help="skip the train step")
    ap.add_argument("--no-scipy", action="store_true", help="skip the host EDT")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_boundary.py measures on an MI355X; there is nothing to time without one"
    L = mi355seg.lib()
    dev = torch.device("cuda:0")
    src = torch.empty(64 << 20, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    copy_gbps = 2 * src.numel() * 4 / (timed(lambda: dst.copy_(src), 3, a.window_s)["median"] * 1e-3) / 1e9
    del src, dst
    stream = torch.cuda.current_stream().cuda_stream
    for ci, case in enumerate(a.cases):
        shape = tuple(int(v) for v in case.split(","))
        N, K, D, H, W = shape
        c0 = 1 if K > 1 else 0
        S = D * H * W
        vox = N * (K - c0) * S
        cold = a.cold_mib * 2 ** 20
        g = torch.Generator(device=dev).manual_seed(K + D)
        ws_bytes = L.query("mi355seg_sdm_ws_bytes", N, K, D, H, W)
        sets = max(2, min(16, int(cold / (4.0 * N * K * S + 16.0 * vox)) + 1))
        ts = [tubes(N, K, D, H, W, dev, g) for _ in range(sets)]
        wss = [torch.empty(ws_bytes, dtype=torch.uint8, device=dev) for _ in range(sets)]
        phis = [torch.empty((N, K - c0, D, H, W), dtype=torch.float32, device=dev) for _ in range(sets)]
        turn = [0]

        def nxt(n):
            turn[0] = (turn[0] + 1) % n
            return turn[0]

        def prefix(steps):
            def run():
                j = nxt(sets)
                L.call("mi355seg_sdm_steps_f32", ts[j].data_ptr(), N, K, D, H, W, 1.0, 1.0, 1.0, 1.0, phis[j].data_ptr(), wss[j].data_ptr(),
                       ws_bytes, steps, stream)
            return run

        # ---- the map against scipy, once
        prefix(3)()
        torch.cuda.synchronize()
        j0 = turn[0]
        mask0 = ts[j0][0, c0].cpu().numpy() > 0.5
        from scipy.ndimage import distance_transform_edt

        def scipy_map():
            return np.where(mask0, -(distance_transform_edt(mask0) - 1.0), distance_transform_edt(~mask0))

        want = scipy_map() if mask0.any() and not mask0.all() else np.zeros(mask0.shape)
        err = float(np.abs(phis[j0][0, 0].cpu().numpy() - want).max())
        assert err <= 2e-6 * max(1.0, float(np.abs(want).max())), err

        res = {1: [], 2: [], 3: []}
        for _ in range(a.rounds):
            for steps in (1, 2, 3):
                res[steps].append(timed(prefix(steps), 1, a.window_s)["median"] * 1e3)
        p1, p2, p3 = (np.array(res[s]) for s in (1, 2, 3))
        pw, ph, pd, whole = spread(p1), spread(p2 - p1), spread(p3 - p2), spread(p3)

        # ---- the loss on a finished map
        xs = [(3.0 * torch.randn(shape, device=dev, generator=g)) for _ in range(sets)]
        for j in range(sets):
            L.call("mi355seg_sdm_f32", ts[j].data_ptr(), N, K, D, H, W, 1.0, 1.0, 1.0, 1.0, phis[j].data_ptr(), wss[j].data_ptr(), ws_bytes, stream)
        lws = torch.empty(max(L.query("mi355seg_boundary_ws_bytes", vox), 8), dtype=torch.uint8, device=dev)
        loss, parts, coef = torch.empty((), device=dev), torch.empty(1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
        one = torch.ones((), device=dev)
        dxs = [torch.empty_like(xs[0]) for _ in range(2)]

        def loss_fwd():
            j = nxt(sets)
            L.call("mi355seg_boundary_fwd_f32", xs[j].data_ptr(), phis[j].data_ptr(), N, K, S, loss.data_ptr(), parts.data_ptr(), coef.data_ptr(),
                   lws.data_ptr(), lws.numel(), stream)

        def loss_bwd():
            j = nxt(sets)
            L.call("mi355seg_boundary_bwd_f32", xs[j].data_ptr(), phis[j].data_ptr(), coef.data_ptr(), one.data_ptr(), N, K, S, dxs[j & 1].data_ptr(), stream)

        def term():
            j = nxt(sets)
            x = xs[j].requires_grad_(True)
            return torch.autograd.grad(F.boundary_loss(x, ts[j]), x)[0]

        loss_fwd()
        res = {"fwd": [], "bwd": [], "term": []}
        for _ in range(a.rounds):
            for name, fn in (("fwd", loss_fwd), ("bwd", loss_bwd), ("term", term)):
                res[name].append(timed(fn, 1, a.window_s)["median"] * 1e3)
        lf, lb, te = spread(res["fwd"]), spread(res["bwd"]), spread(res["term"])

        # ---- the predict-time fp64 EDT on one volume of the same masks (both polarities as its two site maps)
        sites = [torch.stack([t[0, c0] > 0.5, t[0, c0] <= 0.5]).to(torch.uint8).contiguous() for t in ts]
        ews_bytes = L.query("mi355seg_edt3d_ws_bytes", D, H, W)
        ews = torch.empty(max(ews_bytes, 8), dtype=torch.uint8, device=dev)
        dt2 = torch.empty((2, D, H, W), dtype=torch.float64, device=dev)

        def edt64():
            j = nxt(sets)
            L.call("mi355seg_edt3d_f64", sites[j].data_ptr(), D, H, W, 0, 0, 0, D, H, W, 1.0, 1.0, 1.0, dt2.data_ptr(), ews.data_ptr(), ews_bytes, stream)

        e64 = spread([timed(edt64, 1, a.window_s)["median"] * 1e3 for _ in range(a.rounds)])
        row = {"shape": list(shape), "phi_voxels": vox, "buffer_sets": sets, "copy_gbps": copy_gbps, "map_error_vs_scipy": err,
               "pass_w_us": pw, "pass_h_us": ph, "pass_d_us": pd, "map_us": whole}
        for name, sp, nbytes in (("pass_w", pw, 8.0), ("pass_h", ph, 12.0), ("pass_d", pd, 16.0), ("map", whole, 36.0)):
            gbps = nbytes * vox / (sp["median"] * 1e-6) / 1e9
            row[f"{name}_gbps"], row[f"{name}_share_of_copy_rate"] = gbps, gbps / copy_gbps
        row["pass_h_gpairs"] = 2.0 * vox * H / (ph["median"] * 1e-6) / 1e9
        row["pass_d_gpairs"] = 1.0 * vox * D / (pd["median"] * 1e-6) / 1e9
        row.update({"loss_fwd_us": lf, "loss_bwd_us": lb, "term_us": te, "edt3d_f64_us": e64,
                    "edt3d_f64_times_volumes_us": e64["median"] * N * (K - c0), "workspace_bytes": ws_bytes})
        if not a.no_scipy:
            row["scipy_ms"] = host_timed(scipy_map, 1)["median"]
            row["scipy_times_volumes_ms"] = row["scipy_ms"] * N * (K - c0)
        del ts, wss, phis, xs, sites, dxs
        if ci == 0 and K == 2 and not a.no_step:
            from mi355seg.engine import train_step
            from mi355seg.models.three_d.unet3d import UNet3D
            from mi355seg.utils.loss_function import CompoundLoss
            x = torch.randn((N, 1, D, H, W), device=dev, generator=g)
            gt = tubes(N, 1, D, H, W, dev, g)
            for key, crit in (("step_ms", CompoundLoss("dice_bce")), ("step_with_term_ms", CompoundLoss("dice_bce", boundary_weight=0.5))):
                torch.manual_seed(0)
                m = UNet3D(1, 2, 32).to(dev).train()
                opt = torch.optim.Adam(m.parameters(), lr=1e-3)
                row[key] = spread([timed(lambda: train_step(m, opt, x, gt, criterion=crit, sync_metric=False), 1, a.window_s)["median"]
                                   for _ in range(a.rounds)])
                del m, opt
            row["term_share_of_step"] = row["step_with_term_ms"]["median"] / row["step_ms"]["median"] - 1.0
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
