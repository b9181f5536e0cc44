"""The predict-time metrics on the device (csrc/surface.hip): mask edges, the exact anisotropic distance transform, the surface
distances, HD95 and the confusion counters, against tests/golden/hd95.npz (the reference's ``metric(gt, pred, spacing)`` run from
its own file, see tests/golden/make_hd95.py) and against the brute-force fp64 comparator of tests/test_hd95_fixture.py."""
import csv
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
from conftest import GOLDEN, load_golden
from test_hd95_fixture import COLUMNS, brute_hd95, close, edges6, hd95_cases, nearest_site_distance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mi355seg
    mi355seg.lib()
    return mi355seg


def _dev(mask):
    return torch.from_numpy(np.ascontiguousarray(mask)).to(torch.int64).cuda()


def _brute_dt(sites, spacing, box=None):
    """fp64 distance from EVERY voxel (of the box) to the nearest non-zero voxel of ``sites`` [D, H, W], by all pairs, on the device
    the test runs on (torch.cdist without the matmul form)."""
    sp = torch.tensor(spacing, dtype=torch.float64, device="cuda")
    z0, y0, x0, bd, bh, bw = box or (0, 0, 0) + tuple(sites.shape)
    grid = torch.stack(torch.meshgrid(torch.arange(z0, z0 + bd), torch.arange(y0, y0 + bh), torch.arange(x0, x0 + bw), indexing="ij"), -1)
    pts = grid.reshape(-1, 3).double().cuda() * sp
    s = torch.nonzero(torch.as_tensor(sites).cuda()).double() * sp
    return nearest_site_distance(pts, s).reshape(bd, bh, bw)


def _check_edt(F, sites2, spacing, box=None):
    """edt3d of a uint8 pair [2, D, H, W] against the brute-force distance at every voxel, relative 1e-9 (both sides are fp64 sums
    of three squared products and differ by a few 1e-16; a wrong nearest site moves the value by the gap between two lattice
    distances, orders above the bar)."""
    dt = F.edt3d(sites2.cuda(), spacing, box).sqrt()
    worst = 0.0
    for m in range(2):
        if not bool(sites2[m].any()):
            assert bool(torch.isinf(dt[m]).all())
            continue
        ref = _brute_dt(sites2[m], spacing, box)
        assert bool((ref[dt[m] == 0] == 0).all()) and bool((dt[m][ref == 0] == 0).all())
        rel = ((dt[m] - ref).abs() / ref.clamp_min(1e-300))[ref > 0]
        worst = max(worst, float(rel.max()) if rel.numel() else 0.0)
    print(f"edt3d {tuple(sites2.shape)} spacing {spacing} box {box}: worst relative gap {worst:.2e}")
    assert worst <= 1e-9
    return dt


def test_mask_edges_equal_the_six_neighbour_definition(seg):
    F = seg.functional
    for name, gt, pred, sp, _, _ in hd95_cases():
        edges, info = F.mask_edges(_dev(gt), _dev(pred))
        eg, ep = edges6(gt), edges6(pred)
        assert edges.dtype == torch.uint8 and torch.equal(edges[0].cpu().bool(), eg) and torch.equal(edges[1].cpu().bool(), ep), name
        info = info.tolist()
        assert info[:2] == [int(eg.sum()), int(ep.sum())], name
        both = torch.nonzero(eg | ep)
        if len(both):
            assert info[2:5] == both.min(0).values.tolist() and info[5:] == (both.max(0).values + 1).tolist(), name
        else:
            assert info[2:5] == list(gt.shape) and info[5:] == [0, 0, 0], name
    # labels other than 1 are foreground too, and the reference's 4-D / 5-D shapes are accepted
    lab = _dev(hd95_cases()[0][1]) * 3
    e3, _ = F.mask_edges(lab[None], lab[None, None])
    assert torch.equal(e3[0].cpu().bool(), edges6(hd95_cases()[0][1]))


_EDT_CASES = []


def edt_cases():
    """[(name, sites uint8 [2, D, H, W], spacing, box or None)]: the inputs of the exactness test and of the recorded digests
    (tests/golden/make_edt_pins.py) -- made once, shared, never modified"""
    if _EDT_CASES:
        return _EDT_CASES
    out = [(name, torch.stack([edges6(gt), edges6(pred)]).to(torch.uint8), sp, None) for name, gt, pred, sp, _, _ in hd95_cases()]
    # odd extents, with sites drawn at random
    g = torch.Generator().manual_seed(3)
    out.append(("odd", (torch.rand((2, 13, 37, 71), generator=g) > 0.995).to(torch.uint8), (1.3, 0.7, 2.1), None))
    # a one-voxel-thick volume along each axis
    for shape in [(1, 19, 45), (17, 1, 33), (9, 21, 1)]:
        out.append(("thin" + "x".join(str(v) for v in shape), (torch.rand((2,) + shape, generator=g) > 0.97).to(torch.uint8), (0.8, 1.0, 1.7), None))
    # lines longer than one LDS tile of the axis passes (64 rows), than one block of output rows (256), and than one 64-bit word
    # of the pass along W
    long = torch.zeros((2, 300, 5, 150), dtype=torch.uint8)
    long[0, 7, 2, 3] = long[0, 290, 4, 140] = long[0, 150, 0, 70] = 1
    long[1, 299, 0, 149] = 1
    out.append(("long", long, (0.5, 3.0, 1.1), None))
    tall = torch.zeros((2, 3, 270, 66), dtype=torch.uint8)
    tall[0, 1, 269, 0] = tall[0, 0, 0, 65] = tall[1, 2, 130, 64] = 1
    out.append(("tall", tall, (1.0, 0.9, 1.0), None))
    # a box inside the volume
    sites = torch.zeros((2, 20, 30, 40), dtype=torch.uint8)
    sites[0, 5:9, 7:20, 11:30] = 1
    sites[1, 6, 8, 12] = sites[1, 10, 21, 33] = 1
    out.append(("boxed", sites, (1.1, 0.6, 0.9), (4, 6, 10, 8, 17, 25)))
    _EDT_CASES.extend(out)
    return _EDT_CASES


def test_edt3d_is_exact_at_every_voxel(seg):
    F = seg.functional
    for name, sites, sp, box in edt_cases():
        part = _check_edt(F, sites, sp, box)
        if box is None:
            continue
        # the distances the whole volume gives inside the box.  Not bit for bit: the kernel forms s*i - s*j from box-relative
        # indices, and each product is rounded at its own magnitude; with indices below 64 that is at most 64 * 2^-52 = 1.4e-14 of
        # a term, so 1e-13 on the distance
        z0, y0, x0, bd, bh, bw = box
        sub = F.edt3d(sites.cuda(), sp).sqrt()[:, z0:z0 + bd, y0:y0 + bh, x0:x0 + bw]
        assert bool(((part - sub).abs() <= 1e-13 * sub).all())


def edt_pin_digests(F):
    """name -> {"input", "output"}: SHA-256 of every case's sites, spacing and box, and of the bytes of functional.edt3d's fp64
    squared distances (a boxed case: the box run, then the whole-volume run)"""
    out = {}
    for name, sites, sp, box in edt_cases():
        hin = hashlib.sha256(sites.numpy().tobytes() + np.asarray(sp, np.float64).tobytes() + np.asarray(box or (), np.int64).tobytes())
        hout = hashlib.sha256()
        for b in ([box, None] if box else [None]):
            hout.update(F.edt3d(sites.cuda(), sp, b).cpu().numpy().tobytes())
        out[name] = {"input": hin.hexdigest(), "output": hout.hexdigest()}
    return out


def check_pins(got, want, what):
    """recomputed digests against the recorded ones, every case by name"""
    assert sorted(got) == sorted(want), f"{what}: the cases changed: {sorted(set(got) ^ set(want))}"
    for name in sorted(got):
        assert got[name]["input"] == want[name]["input"], f"{what} {name}: inputs changed (the recorded digest is of other bytes)"
    bad = [name for name in sorted(got) if got[name]["output"] != want[name]["output"]]
    assert not bad, f"{what}: the output bits differ from the recorded ones in {bad}"


def test_edt3d_bits_equal_the_recorded_digests(seg):
    """tests/golden/edt_pins.json: the bytes of edt3d's output on every case of edt_cases(), recorded before surface.hip and
    boundary.hip came to share csrc/edt.h -- all four edt_pass_axis_kernel instantiations, several LDS chunks and ballot words"""
    with open(os.path.join(GOLDEN, "edt_pins.json")) as fh:
        pins = json.load(fh)
    check_pins(edt_pin_digests(seg.functional), pins["edt3d"], "edt3d")


def _large_pair():
    spec = importlib.util.spec_from_file_location("make_hd95", os.path.join(GOLDEN, "make_hd95.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    g = load_golden("hd95")
    rec = {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith("large/")}
    gt, pred = mod.large_pair(rec)
    assert mod.pack_crc(gt, pred) == int(rec["crc32"]), "the large pair's recipe no longer gives the recorded masks"
    return gt, pred, tuple(float(v) for v in rec["spacing"]), rec["out"], rec["edge_counts"].tolist()


def test_metric_with_spacing_returns_the_references_five_numbers(seg):
    from mi355seg.utils.metric import metric
    cases = [(n, g, p, sp, fl, out) for n, g, p, sp, fl, out in hd95_cases() if not n.startswith("empty")]
    gt, pred, sp, out, counts = _large_pair()
    cases.append(("large", gt, pred, sp, False, out))
    for name, gt, pred, sp, as_float, out in cases:
        dt = torch.float32 if as_float else torch.int64
        got = metric(torch.from_numpy(gt)[None].to(dt).cuda(), torch.from_numpy(pred)[None].to(dt).cuda(), sp)
        assert len(got) == 5
        print(f"{name}: got {[float(v) for v in got]} recorded {out.tolist()}")
        assert [float(v) for v in got[:4]] == out[:4].tolist(), name           # precision, recall, jaccard, dice: identical doubles
        assert close(float(got[4]), float(out[4]), 1e-9), (name, got[4], out[4])
    assert seg.functional.mask_edges(_dev(gt), _dev(pred))[1][:2].tolist() == counts
    # the reference's predict.py hands over [C=1, D, H, W]; [1, 1, D, H, W] is what it passes on to monai
    name, gt, pred, sp, _, out = cases[0]
    got5 = metric(_dev(gt)[None, None], _dev(pred)[None, None], sp)
    assert [float(v) for v in got5[:4]] == out[:4].tolist() and close(float(got5[4]), float(out[4]), 1e-9)


def test_confusion_counts_equal_the_reference_fixture(seg):
    g = np.load(os.path.join(GOLDEN, "metric.npz"))
    for n in sorted({k.split("/")[0] for k in g.files}):
        c = seg.functional.confusion_counts(torch.from_numpy(g[n + "/gt"]).to(torch.int64).cuda(), torch.from_numpy(g[n + "/pred"]).to(torch.int64).cuda())
        c = c.cpu().tolist()
        assert c[:4] == g[n + "/counts"].tolist() and [float(v) for v in c[4:]] == g[n + "/tp_fp_fn_tn"].tolist(), n


@pytest.mark.parametrize("numel", [37, 70001, 1100003])
def test_confusion_counts_equal_torch_in_every_block_regime(seg, numel):
    """the grid is ceil(numel / 256) blocks, at most 4096: one block with fewer than 64 live threads; 274 blocks, so the finalize
    makes a ragged second trip over the partials; past the cap with a ragged grid-stride tail.  Integers: equal to torch on the CPU."""
    gen = torch.Generator().manual_seed(numel)
    g, p = (torch.randint(0, 2, (numel,), generator=gen, dtype=torch.int64) for _ in range(2))
    want = [g.sum(), p.sum(), ((g & p) != 0).sum(), ((g | p) != 0).sum(), (g & p).sum(), (p * (p - g >= 1)).sum(), (g * (g - p >= 1)).sum(), (1 - (g | p)).sum()]
    assert seg.functional.confusion_counts(g.cuda(), p.cuda()).cpu().tolist() == [int(v) for v in want]


def test_metric_without_spacing_is_untouched(seg):
    from mi355seg.utils.metric import metric
    g = np.load(os.path.join(GOLDEN, "metric.npz"))
    for n in sorted({k.split("/")[0] for k in g.files}):
        gt, pred = torch.from_numpy(g[n + "/gt"]).cuda(), torch.from_numpy(g[n + "/pred"]).cuda()
        assert list(metric(gt, pred)) == g[n + "/jaccard_dice"].tolist(), n
        assert list(metric(gt, pred, None)) == g[n + "/jaccard_dice"].tolist(), n


def test_empty_masks_give_a_non_finite_distance(seg):
    from mi355seg.utils.metric import metric
    for name, gt, pred, sp, _, out in hd95_cases():
        if not name.startswith("empty"):
            continue
        got = metric(_dev(gt)[None], _dev(pred)[None], sp)
        torch.cuda.synchronize()
        assert not np.isfinite(got[4]) and not np.isfinite(out[4]), name
        assert [float(v) for v in got[:4]] == out[:4].tolist(), name
    # the kernels themselves take an empty site set: every distance is +inf
    dt = seg.functional.edt3d(torch.zeros((2, 6, 7, 8), dtype=torch.uint8, device="cuda"), (1.0, 1.0, 1.0))
    assert bool(torch.isinf(dt).all())


def test_hd95_is_deterministic(seg):
    F = seg.functional
    name, gt, pred, sp, _, _ = [c for c in hd95_cases() if c[0] == "blobs48"][0]
    a = F.hd95(_dev(gt), _dev(pred), sp)
    b = F.hd95(_dev(gt), _dev(pred), sp)
    assert a.dtype == torch.float64 and a.dim() == 0 and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    d1 = F.edt3d(F.mask_edges(_dev(gt), _dev(pred))[0], sp)
    d2 = F.edt3d(F.mask_edges(_dev(gt), _dev(pred))[0], sp)
    assert torch.equal(d1, d2)


def test_hd95_other_percentiles_and_surface_distances(seg):
    F = seg.functional
    name, gt, pred, sp, _, _ = [c for c in hd95_cases() if c[0] == "blob40_s1"][0]
    for q in (0.0, 50.0, 95.0, 100.0):
        assert close(float(F.hd95(_dev(gt), _dev(pred), sp, q)), float(brute_hd95(gt, pred, sp, q)), 1e-9), q
    edges, info = F.mask_edges(_dev(gt), _dev(pred))
    n_gt, n_pred = info[:2].tolist()
    d_gt, d_pred = F.surface_distances(edges, F.edt3d(edges, sp), n_gt, n_pred)
    spt = torch.tensor(sp, dtype=torch.float64)
    a, b = torch.nonzero(edges6(gt)).double() * spt, torch.nonzero(edges6(pred)).double() * spt
    for got, ref in ((d_gt, nearest_site_distance(a, b)), (d_pred, nearest_site_distance(b, a))):
        got, ref = got.cpu().sort().values, ref.sort().values
        assert got.shape == ref.shape and float(((got - ref).abs() / ref.clamp_min(1e-300))[ref > 0].max()) <= 1e-9


def test_bad_arguments_raise(seg):
    F = seg.functional
    v = torch.zeros((4, 5, 6), dtype=torch.int64, device="cuda")
    with pytest.raises(seg.Mi355SegError):
        F.hd95(v.cpu(), v.cpu(), (1, 1, 1))
    with pytest.raises(seg.Mi355SegError):
        F.hd95(v.float(), v.float(), (1, 1, 1))
    with pytest.raises(seg.Mi355SegError):
        F.hd95(v, v, (1, 0, 1))
    with pytest.raises(seg.Mi355SegError):
        F.hd95(v, v[:3], (1, 1, 1))
    with pytest.raises(seg.Mi355SegError):
        F.edt3d(torch.zeros((2, 4, 5, 6), dtype=torch.uint8, device="cuda"), (1, 1, 1), box=(0, 0, 0, 5, 5, 6))


def test_custom_ops_equal_functional(seg):
    from mi355seg import custom_ops  # noqa: F401
    F = seg.functional
    name, gt, pred, sp, _, _ = hd95_cases()[0]
    g, p = _dev(gt), _dev(pred)
    a = torch.ops.mi355seg.hd95(g, p, list(sp), 95.0)
    assert a.cpu().numpy().tobytes() == F.hd95(g, p, sp).cpu().numpy().tobytes()
    assert torch.equal(torch.ops.mi355seg.hd95(g, p, list(sp)), a)
    assert torch.equal(torch.ops.mi355seg.confusion_counts(g, p), F.confusion_counts(g, p))
    meta = torch.empty(gt.shape, dtype=torch.int64, device="meta")
    assert torch.ops.mi355seg.hd95(meta, meta, [1.0, 1.0, 1.0]).shape == () and torch.ops.mi355seg.confusion_counts(meta, meta).shape == (8,)


def test_predict_cli_with_spacing_writes_the_five_columns(seg, tmp_path):
    from mi355seg.predict import main as predict_main
    from mi355seg.train import main as train_main
    out = str(tmp_path / "logs")
    common = ["config=unet", f"config.output_dir={out}", "config.patch_size=32,32,32", "config.batch_size=2"]
    cfg, _ = train_main(common + ["config.iters_per_epoch=2", "config.epochs=1"])
    ckpt = os.path.join(cfg.hydra_path, "latest_checkpoint.pt")
    cfg_a, rows_a = predict_main(common + [f"config.ckpt={ckpt}", f"config.hydra_path={tmp_path / 'plain'}"])
    cfg_b, rows_b = predict_main(common + [f"config.ckpt={ckpt}", f"config.hydra_path={tmp_path / 'spaced'}", "config.spacing=1,1,2"])
    assert cfg_a.hydra_path != cfg_b.hydra_path
    with open(os.path.join(cfg_a.hydra_path, "metrics.csv"), newline="") as fh:
        plain = list(csv.reader(fh))
    with open(os.path.join(cfg_b.hydra_path, "metrics.csv"), newline="") as fh:
        spaced = list(csv.reader(fh))
    assert plain[0] == ["file", "jaccard", "dice"] and len(plain) == 3 and all(set(r) == {"file", "jaccard", "dice"} for r in rows_a)
    assert spaced[0] == ["file"] + COLUMNS and len(spaced) == 4 and spaced[3][0] == "mean"
    for ra, rb in zip(rows_a, rows_b):
        assert ra["file"] == rb["file"] and ra["dice"] == rb["dice"] and ra["jaccard"] == rb["jaccard"]
        assert 0.0 <= rb["precision"] <= 1.0 and 0.0 <= rb["recall"] <= 1.0 and isinstance(rb["hs95"], float)
        pa = np.load(os.path.join(cfg_a.hydra_path, ra["file"] + "_pred.npy"))
        pb = np.load(os.path.join(cfg_b.hydra_path, rb["file"] + "_pred.npy"))
        assert np.array_equal(pa, pb)
    for j, k in enumerate(COLUMNS):
        mean = float(np.mean([r[k] for r in rows_b]))
        assert float(spaced[3][1 + j]) == mean or (np.isnan(mean) and np.isnan(float(spaced[3][1 + j])))
