#!/usr/bin/env python3
"""Generate tests/golden/ovr_<case>.npz, the stored side of tests/test_oracle_vs_reference.py, by running the REFERENCE
modules on the closed-form weights / inputs of oracle/fill.py:

    python tests/golden/make_oracle_vs_reference.py <reference checkout> [case ...]

Each file holds data only: the reference module's state_dict layout (names in registration order, shapes), its forward
output(s), every parameter gradient (a seeded random sample of its elements, its largest magnitude and three whole-tensor
float64 aggregates: sum g, sum |g| and sum g * r for a fixed closed-form r), and how far each of these moves in the reference's
own fp32 arithmetic when only the ATen thread count changes (the tests' tolerance scale).  No reference source is stored."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.fill import RESUNET96_HEAD_SCALE, fill_module_, fill_module_hash_, make_input, make_input_rough  # noqa: E402

THREADS = (1, 2, 3, 4, 8, 16, 32, 64)   # the spread is taken over these ATen thread counts
SAMPLE = 512                  # seeded random gradient sample per tensor
OUT_SAMPLE = 1 << 16          # outputs larger than this are stored as a strided sample of this many values


def _sample(t, k=SAMPLE):
    f = t.detach().reshape(-1)
    step = max(1, f.numel() // k)
    return f[::step][:k].numpy().copy()


def sample_index(n, k=SAMPLE):
    """Sorted seeded random element indices of a gradient tensor (a fixed stride can fall on one kernel tap of every filter)."""
    return np.arange(n) if n <= k else np.sort(np.random.default_rng(0).choice(n, k, replace=False))


def aggregates(g):
    """sum g, sum |g|, sum g * r (r_i = sin(12.9898 i + 1): zeroing or doubling moves the second, negating the first and third)."""
    g64 = g.detach().double().reshape(-1)
    r = torch.sin(torch.arange(g64.numel(), dtype=torch.float64) * 12.9898 + 1.0)
    return np.array([float(g64.sum()), float(g64.abs().sum()), float((g64 * r).sum())])


def _filled(make):
    return lambda R: fill_module_(make(R))


def _ref(modname, cls):
    import importlib
    return getattr(importlib.import_module(modname), cls)


def _square_mean(seed):
    def run(m, x):
        if seed is not None:
            torch.manual_seed(seed)
        y = m(x)
        y.square().mean().backward()
        return [y.detach()]
    return run


def _isnet_run(m, x):
    from oracle.step import frequency_bands
    low, high = frequency_bands(x)
    o1, o2 = m(x, low, high)
    (o1.square().mean() + 0.5 * o2.square().mean()).backward()
    return [o1.detach(), o2.detach()]


CASES = {
    # case: (module, class, filled constructor, input, forward + loss)
    "unet3d": ("models.three_d.unet3d", "UNet3D", _filled(lambda R: R(1, 2, 8)), lambda: make_input((2, 1, 16, 16, 16)), _square_mean(None)),
    "vnet": ("models.three_d.vnet3d", "VNet", _filled(lambda R: R(in_channels=1, classes=2)), lambda: make_input((2, 1, 16, 16, 16)),
             _square_mean(3)),
    "vnet_prelu": ("models.three_d.vnet3d", "VNet", _filled(lambda R: R(elu=False, in_channels=1, classes=2)),
                   lambda: make_input((2, 1, 16, 16, 16)), _square_mean(3)),
    # kaiming-variance hash weights and a rough input at 64^3 (deepest InstanceNorm over 4^3 voxels): the sin-fill at 16 x 32 x 16
    # left the reference's own output moving by 7e-3 with the thread count and its gradients by up to ~90
    "resunet": ("models.three_d.residual_unet3d", "UNet",
                lambda R: fill_module_hash_(R(in_channels=4, n_classes=4, base_n_filter=4), RESUNET96_HEAD_SCALE),
                lambda: make_input_rough((1, 4, 64, 64, 64), seed=2.0), _square_mean(5)),
    "unetr": ("models.three_d.unetr", "UNETR", _filled(lambda R: R(img_shape=(32, 32, 32), input_dim=1, output_dim=2, embed_dim=96,
                                                                   patch_size=16, num_heads=4, dropout=0.1)),
              lambda: make_input((2, 1, 32, 32, 32)), _square_mean(9)),
    "isnet": ("models.three_d.IS", "UNet3D", _filled(lambda R: R(1, 2, 4)), lambda: make_input((1, 1, 32, 32, 32), freq=0.37), _isnet_run),
    "csrnet": ("models.three_d.csrnet", "CSRNet", _filled(lambda R: R(1, 2, 4)),
               lambda: make_input((2, 1, 32, 32, 32), freq=0.23), _square_mean(None)),
    "renet": ("models.three_d.RE_net", "RE_Net", _filled(lambda R: R()), lambda: make_input_rough((1, 1, 32, 32, 32), seed=5.0),
              _square_mean(None)),
    "ernet": ("models.three_d.ER_net", "ER_Net", _filled(lambda R: R(classes=2, channels=1)),
              lambda: make_input_rough((1, 1, 32, 32, 32), seed=7.0), _square_mean(None)),
}


def _once(case):
    modname, cls, make, mk_x, run = CASES[case]
    m = make(_ref(modname, cls)).train()
    outs = run(m, mk_x())
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}
    return m, outs, grads


def record(case):
    m, outs, grads = None, None, None
    spread_out, spread_grad, spread_agg = 0.0, {}, {}
    for th in THREADS:
        torch.set_num_threads(th)
        m_t, o_t, g_t = _once(case)
        if m is None:
            m, outs, grads = m_t, o_t, g_t
            continue
        for a, b in zip(outs, o_t):
            spread_out = max(spread_out, float((a - b).abs().max()))
        for k, g in grads.items():
            if g is not None:
                spread_grad[k] = max(spread_grad.get(k, 0.0), float((g - g_t[k]).abs().max()))
                spread_agg[k] = np.maximum(spread_agg.get(k, np.zeros(3)), np.abs(aggregates(g) - aggregates(g_t[k])))
    sd = m.state_dict()
    rec = {"keys": np.array(list(sd)), "shape_rank": np.array([v.dim() for v in sd.values()], np.int64),
           "shape_dims": np.array([d for v in sd.values() for d in v.shape], np.int64),
           "spread_out": np.float64(spread_out), "torch_version": np.array(torch.__version__)}
    for i, o in enumerate(outs):
        rec[f"out{i}"] = o.numpy().copy() if o.numel() <= OUT_SAMPLE else _sample(o, OUT_SAMPLE)
    rec["no_grad"] = np.array([k for k, g in grads.items() if g is None] or [""])
    for k, g in grads.items():
        if g is None:
            continue
        rec["grad/" + k] = g.reshape(-1).numpy()[sample_index(g.numel())].copy()
        rec["gmax/" + k] = np.float64(float(g.abs().max()))
        rec["gagg/" + k] = aggregates(g)
        rec["gspread/" + k] = np.float64(spread_grad.get(k, 0.0))
        rec["gaggspread/" + k] = spread_agg.get(k, np.zeros(3))
    if case == "isnet":
        for k, v in m.named_buffers():
            rec["buf/" + k] = v.numpy().copy()
    return rec


def isnet_bands(ref_root):
    """The reference's two FFT filters (train.py) on two inputs, lifted out of its syntax tree and run as they stand."""
    import ast
    import torch.fft as fft
    ns = {"torch": torch, "fft": fft}
    path = os.path.join(ref_root, "train.py")
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name in ("low_pass_torch", "high_pass_torch"):
            exec(compile(ast.Module([node], []), "train.py", "exec"), ns)
    rec = {}
    for tag, x in (("a", make_input((1, 1, 16, 16, 16), freq=0.37)), ("b", make_input((2, 1, 8, 12, 16), freq=0.21))):
        rec["band_low_" + tag] = ns["low_pass_torch"](x, 0.04).numpy().copy()
        rec["band_high_" + tag] = ns["high_pass_torch"](x, 0.04).numpy().copy()
    return rec


def main():
    ref_root = os.path.abspath(sys.argv[1])
    sys.path.insert(0, ref_root)
    cases = sys.argv[2:] or list(CASES)
    for case in cases:
        rec = record(case)
        if case == "isnet":
            rec.update(isnet_bands(ref_root))
        out = os.path.join(HERE, f"ovr_{case}.npz")
        np.savez_compressed(out, **rec)
        print(case, os.path.getsize(out), "bytes, output spread", float(rec["spread_out"]))


if __name__ == "__main__":
    main()
