"""config.resample_spacing on the host (no GPU, no kernel launch): output shapes, the per-axis tables against the fp64 formula, the
numpy fp64 resampler against scipy.ndimage.map_coordinates, the label rule against a brute one-hot computation, the keys' parser and
every refusal, the spacing_file reader, the CPU branch of the patch queue and the argument checks of the C-ABI entry points (which
return before any launch).  The references are written out here and do not call the package's implementation."""
import ctypes
import math
import os

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import mi355seg
from mi355seg import data
from mi355seg import functional as F
from mi355seg import resample as R
from mi355seg._lib import HEADER, LIB_PATH, parse_header
from mi355seg.config import Config


def cfg(**kw):
    return Config({"data_path": "/d", "gt_path": "/g", "patch_size": 8, "batch_size": 1, **kw})


def coords(n_in, n_out, ratio):
    return np.array([min(max((o + 0.5) * ratio - 0.5, 0.0), n_in - 1.0) for o in range(n_out)], dtype=np.float64)


# ---------------------------------------------------------------------------------------------- shapes and tables
def test_resampled_shape():
    assert R.resampled_shape((128, 128, 128), (1.0, 1.0, 1.0), (0.8, 0.8, 0.8)) == (160, 160, 160)
    assert math.ceil(3 * 0.1 / 0.1) == 4 and R.resampled_shape((3, 3, 3), (0.1, 0.1, 0.1), (0.1, 0.1, 0.1)) == (3, 3, 3)   # what the 1e-6 is for
    assert R.resampled_shape((5, 40, 7), (1.0, 1.0, 1.0), (9.0, 1.0, 1.0)) == (1, 40, 7)                  # a ratio that leaves one voxel
    assert R.resampled_shape((17, 23, 37), (2.5, 0.7, 0.7), (2.5, 0.7, 0.7)) == (17, 23, 37)              # identity
    assert R.resampled_shape((64, 256, 256), (2.5, 0.7, 0.7), (1.0, 1.0, 1.0)) == (160, 180, 180)
    assert F.resampled_shape is R.resampled_shape and F.resample_axis_table is R.resample_axis_table
    for bad in ((0, 4, 4), (4, 4)):
        with pytest.raises(ValueError, match="three positive extents"):
            R.resampled_shape(bad, (1, 1, 1), (1, 1, 1))
    for sp, tg in (((1, 1), (1, 1, 1)), ((1, 1, 0), (1, 1, 1)), ((1, 1, 1), (1, -1, 1)), ((1, 1, 1), (1, float("nan"), 1))):
        with pytest.raises(ValueError, match="three positive numbers"):
            R.resampled_shape((4, 4, 4), sp, tg)


@pytest.mark.parametrize("n_in,ratio", [(37, 0.5), (37, 0.7), (23, 0.75), (17, 1.25), (40, 1.5), (9, 1.0), (130, 2.5), (1, 0.5), (2, 0.3), (5, 7.0)])
def test_axis_tables_follow_the_fp64_formula(n_in, ratio):
    n_out = max(1, math.ceil(n_in / ratio - 1e-6))
    c = coords(n_in, n_out, ratio)
    assert c[0] >= 0.0 and c[-1] <= n_in - 1 and np.all(np.diff(c) >= 0)
    if ratio < 1.0 and n_in > 1:
        assert c[0] == 0.0 and c[-1] == n_in - 1                                 # clamped at both ends
    b0, f0 = R.resample_axis_table(n_in, n_out, ratio, 0)
    assert b0.dtype == np.int32 and f0.dtype == np.float32 and np.array_equal(b0, np.floor(c + 0.5).astype(np.int32)) and not f0.any()
    assert b0.min() >= 0 and b0.max() <= n_in - 1
    for order in (1, 3):
        b, f = R.resample_axis_table(n_in, n_out, ratio, order)
        assert b.dtype == np.int32 and f.dtype == np.float32
        assert np.array_equal(b, np.floor(c).astype(np.int32)) and np.array_equal(f, (c - np.floor(c)).astype(np.float32))
        assert b.min() >= 0 and b.max() <= n_in - 1 and f.min() >= 0.0 and f.max() < 1.0
        if order == 1:
            assert np.all((np.minimum(b + 1, n_in - 1) <= n_in - 1) & ((b + 1 <= n_in - 1) | (f == 0.0)))   # base + 1 inside, or unused
        else:
            for k in range(-1, 3):
                m = R.mirror_index(b.astype(np.int64) + k, n_in)
                assert m.min() >= 0 and m.max() <= n_in - 1
    with pytest.raises(ValueError, match="order must be one of"):
        R.resample_axis_table(n_in, n_out, ratio, 2)


def test_order0_rounds_half_up():
    # ratio 2 on 8 samples: c = 0.5, 2.5, 4.5, 6.5 -> 1, 3, 5, 7 (half up, not to even)
    b, _ = R.resample_axis_table(8, 4, 2.0, 0)
    assert b.tolist() == [1, 3, 5, 7]
    assert R.mirror_index(np.array([-1, 0, 4, 5, 6]), 5).tolist() == [1, 0, 4, 3, 2]
    assert R.mirror_index(np.array([-1, 2, 3]), 2).tolist() == [1, 0, 1] and R.mirror_index(np.array([-1, 2]), 1).tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------- the fp64 resampler against scipy
def table_grid(shape, out_shape, ratios, order):
    cs = []
    for n, no, r in zip(shape, out_shape, ratios):
        b, f = R.resample_axis_table(n, no, r, order)
        cs.append(b.astype(np.float64) + f.astype(np.float64))
    return np.meshgrid(*cs, indexing="ij")


CASES = [((17, 23, 37), (0.7, 1.25, 2.5)), ((1, 1, 5), (1.0, 1.0, 0.5)), ((2, 3, 1), (0.5, 0.75, 1.0)), ((5, 4, 30), (1.5, 0.7, 0.75)),
         ((13, 14, 15), (0.75, 1.5, 1.25))]


@pytest.mark.parametrize("order", [0, 1, 3])
@pytest.mark.parametrize("shape,ratios", CASES, ids=["x".join(map(str, c[0])) for c in CASES])
def test_resample_host_against_map_coordinates(shape, ratios, order):
    x = np.random.default_rng(3).standard_normal(shape).astype(np.float32)
    out_shape = R.resampled_shape(shape, (1.0, 1.0, 1.0), ratios)
    got = R.resample_to_host(x, out_shape, ratios, order)
    ref = ndi.map_coordinates(x.astype(np.float64), table_grid(shape, out_shape, ratios, order), order=order, mode="mirror")
    err = float(np.abs(got - ref).max())
    print(f"[resample] host order {order} {shape} -> {out_shape}: {err:.3e} (bound 1e-12)")
    assert got.shape == out_shape and err <= 1e-12
    whole = R.resample_host(x[None], (1.0, 1.0, 1.0), ratios, order)
    assert whole.dtype == np.float32 and whole.shape == (1,) + out_shape and np.array_equal(whole[0], got.astype(np.float32))


@pytest.mark.parametrize("n", [1, 2, 3, 13, 14, 15, 40])
def test_prefilter_host_against_spline_filter(n):
    x = np.random.default_rng(n).standard_normal((3, n, 4))
    got = R.bspline3_prefilter_host(x, axes=(-2,))
    ref = ndi.spline_filter1d(x, order=3, axis=1, mode="mirror") if n > 1 else x
    assert np.abs(got - ref).max() <= 1e-12
    assert abs(R.POLE) ** R.INIT_TERMS < 2.0 ** -25 < abs(R.POLE) ** (R.INIT_TERMS - 1)


def onehot_labels(y, out_shape, ratios):
    """brute force: every class's one-hot volume through map_coordinates(order=1), argmax with the lowest class on ties"""
    g = table_grid(y.shape, out_shape, ratios, 1)
    w = np.stack([ndi.map_coordinates((y == k).astype(np.float64), g, order=1, mode="nearest") for k in range(16)])
    return np.argmax(w, axis=0), np.sort(w, axis=0)[-1] - np.sort(w, axis=0)[-2]


@pytest.mark.parametrize("ratios", [(0.5, 1.5, 0.75), (1.25, 0.7, 2.5)])
def test_label_rule_against_one_hot(ratios):
    rng = np.random.default_rng(5)
    y = np.repeat(np.repeat(np.repeat(rng.integers(0, 16, (4, 5, 6)), 3, 0), 3, 1), 3, 2).astype(np.float32)
    out_shape = R.resampled_shape(y.shape, (1.0, 1.0, 1.0), ratios)
    ref, margin = onehot_labels(y, out_shape, ratios)
    got = R.resample_labels_to_host(y, out_shape, ratios, "linear")
    keep = margin >= 1e-9
    assert got.dtype == np.float32 and keep.mean() > 0.9 and np.array_equal(got[keep], ref[keep].astype(np.float32))
    near = R.resample_labels_to_host(y, out_shape, ratios, "nearest")
    assert np.array_equal(near, ndi.map_coordinates(y, table_grid(y.shape, out_shape, ratios, 0), order=0))
    # an exact tie: ratio 2 reads four voxels at 0.5 and 2.5, half-way between two classes -> the lower class, whichever side it is on
    assert R.axis_matrix(4, 2, 2.0, 1).tolist() == [[0.5, 0.5, 0.0, 0.0], [0.0, 0.0, 0.5, 0.5]]
    line = np.array([3.0, 5.0, 5.0, 3.0], dtype=np.float32).reshape(1, 1, 4)
    assert R.resample_labels_to_host(line, (1, 1, 2), (1.0, 1.0, 2.0), "linear")[0, 0].tolist() == [3.0, 3.0]
    for bad in (16.0, -1.0, 0.5, float("nan")):
        y2 = y.copy()
        y2[1, 2, 3] = bad
        with pytest.raises(ValueError, match="not integers in 0 .. 15"):
            R.resample_labels_to_host(y2, out_shape, ratios, "linear")
    with pytest.raises(ValueError, match="label mode"):
        R.resample_labels_to_host(y, out_shape, ratios, "cubic")


def test_identity_spacing_returns_the_input_bit_for_bit():
    x = np.random.default_rng(1).standard_normal((2, 5, 6, 7)).astype(np.float32)
    y = np.random.default_rng(2).integers(0, 4, (1, 5, 6, 7)).astype(np.float32)
    sp = (2.5, 0.7, 0.7)
    for order in (0, 1):
        assert np.array_equal(R.resample_host(x, sp, sp, order).view(np.int32), x.view(np.int32))
        assert np.array_equal(R.resample_to_host(x, x.shape[1:], (1.0, 1.0, 1.0), order).astype(np.float32).view(np.int32), x.view(np.int32))
    for mode in R.LABEL_MODES:
        assert np.array_equal(R.resample_labels_host(y, sp, sp, mode), y)
        assert np.array_equal(R.resample_labels_to_host(y, y.shape[1:], (1.0, 1.0, 1.0), mode), y)


# ---------------------------------------------------------------------------------------------- keys
def test_keys_absent_mean_off():
    assert R.parse_resample(cfg()) is None and R.parse_resample(cfg(resample_spacing="")) is None
    assert R.parse_resample(cfg(resample_spacing=None, spacing="1,1,1")) is None
    assert R.parse_spacing_source(cfg()) is None


def test_keys_parse(tmp_path):
    s = R.parse_resample(cfg(resample_spacing="1,1.5,2", spacing="2.5,0.7,0.7"))
    assert s.target == (1.0, 1.5, 2.0) and s.order == 1 and s.labels == "linear" and s.spacings.of("any.npy") == (2.5, 0.7, 0.7)
    s = R.parse_resample(cfg(resample_spacing=1, resample_order="3", resample_labels="nearest", spacing=(1, 2, 3)))
    assert s.target == (1.0, 1.0, 1.0) and s.order == 3 and s.labels == "nearest" and s.spacings.of("v") == (1.0, 2.0, 3.0)
    f = tmp_path / "sp.csv"
    f.write_text("file,sz,sy,sx\n# comment\n\na.npy,2.5,0.7,0.7\nsub/b,1,1,1\n")
    s = R.parse_resample(cfg(resample_spacing="(1, 1, 1)", spacing_file=str(f), spacing="9,9,9"))          # the file wins
    assert s.spacings.of("/x/y/a.npy") == (2.5, 0.7, 0.7) and s.spacings.of("b") == (1.0, 1.0, 1.0) and "2 volumes" in repr(s)
    with pytest.raises(ValueError, match="no line for the volume c"):
        s.spacings.of("c.npy")
    src = R.parse_spacing_source(cfg(spacing_file=str(f)))                      # without resampling: the source alone
    assert src.table == {"a": (2.5, 0.7, 0.7), "b": (1.0, 1.0, 1.0)} and R.parse_resample(cfg(spacing_file=str(f))) is None


@pytest.mark.parametrize("kw,key", [
    ({"resample_spacing": "1,1"}, "resample_spacing"), ({"resample_spacing": "1,0,1"}, "resample_spacing"),
    ({"resample_spacing": "a,b,c"}, "resample_spacing"), ({"resample_spacing": True}, "resample_spacing"),
    ({"resample_spacing": "1,1,inf"}, "resample_spacing"),
    ({"resample_spacing": "1,1,1", "resample_order": 2}, "resample_order"), ({"resample_spacing": "1,1,1", "resample_order": "0"}, "resample_order"),
    ({"resample_spacing": "1,1,1", "resample_order": True}, "resample_order"), ({"resample_spacing": "1,1,1", "resample_order": "cubic"}, "resample_order"),
    ({"resample_spacing": "1,1,1", "resample_labels": "cubic"}, "resample_labels"), ({"resample_spacing": "1,1,1", "resample_labels": 1}, "resample_labels"),
    ({"resample_order": 3}, "resample_order"), ({"resample_labels": "nearest"}, "resample_labels"),
    ({"resample_spacing": "1,1,1", "spacing": "1,1"}, "spacing"), ({"resample_spacing": "1,1,1", "spacing": "0,1,1"}, "spacing"),
    ({"resample_spacing": "1,1,1", "spacing_file": "relative.csv"}, "spacing_file"),
    ({"resample_spacing": "1,1,1", "spacing_file": "/nonexistent/sp.csv"}, "spacing_file"),
])
def test_malformed_keys_name_themselves(kw, key):
    kw.setdefault("spacing", "1,1,1")
    with pytest.raises(ValueError, match=f"config.{key}"):
        R.parse_resample(cfg(**kw))


def test_resample_spacing_needs_a_spacing_source():
    with pytest.raises(ValueError, match="config.resample_spacing needs the volumes' spacing"):
        R.parse_resample(cfg(resample_spacing="1,1,1"))
    with pytest.raises(ValueError, match="needs the volumes' spacing"):
        R.ResampleSpec((1, 1, 1))


@pytest.mark.parametrize("text,what", [("a.npy,1,1\n", "line 1"), ("a.npy,1,1,zero\n", "line 1"), ("a.npy,1,1,1\nb.npy,1,-1,1\n", "line 2"),
                                       ("a.npy,1,1,1\na,2,2,2\n", "listed twice"), ("file,sz,sy,sx\n", "lists no volume")])
def test_spacing_file_refusals(tmp_path, text, what):
    f = tmp_path / "sp.csv"
    f.write_text(text)
    with pytest.raises(ValueError, match=f"config.spacing_file.*{what}"):
        R.load_spacing_file(str(f))


# ---------------------------------------------------------------------------------------------- the queue's CPU branch
@pytest.fixture()
def cohort(tmp_path):
    """two volumes of different spacing; the labels are blocks of classes 0 .. 3"""
    d, g = tmp_path / "img", tmp_path / "gt"
    d.mkdir()
    g.mkdir()
    rng = np.random.default_rng(11)
    vols, spacings = {}, {"v0": (2.5, 1.0, 0.75), "v1": (1.0, 1.5, 1.0)}
    for name, shape in (("v0", (8, 20, 24)), ("v1", (18, 12, 20))):
        x = ndi.gaussian_filter(rng.standard_normal(shape), 1.0).astype(np.float32) * 50.0 + 100.0
        y = np.repeat(np.repeat(np.repeat(rng.integers(0, 4, tuple(s // 2 for s in shape)), 2, 0), 2, 1), 2, 2).astype(np.float32)
        np.save(str(d / f"{name}.npy"), x)
        np.save(str(g / f"{name}.npy"), y)
        vols[name] = (x, y)
    f = tmp_path / "spacings.csv"
    f.write_text("file,sz,sy,sx\n" + "".join(f"{n}.npy,{s[0]},{s[1]},{s[2]}\n" for n, s in spacings.items()))
    return str(d), str(g), str(f), vols, spacings


@pytest.mark.parametrize("order,labels", [(1, "linear"), (3, "nearest")])
def test_queue_cpu_branch_yields_patches_of_the_resampled_volumes(cohort, order, labels):
    d, g, f, vols, spacings = cohort
    spec = R.parse_resample(cfg(resample_spacing="1,1,1", resample_order=order, resample_labels=labels, spacing_file=f))
    q = data.DevicePatchQueue(d, g, (8, 8, 8), 2, 4, torch.device("cpu"), seed=3, queue_length=4, samples_per_volume=2, resample=spec)
    whole = {}
    for name, (x, y) in vols.items():
        shape = R.resampled_shape(x.shape, spacings[name], (1.0, 1.0, 1.0))
        ratios = [1.0 / s for s in spacings[name]]
        xr = R.resample_to_host(x, shape, ratios, order).astype(np.float32)
        ref = ndi.map_coordinates(x.astype(np.float64), table_grid(x.shape, shape, ratios, order), order=order, mode="mirror")
        assert np.abs(xr - ref).max() <= 1e-4 and shape != x.shape
        xr = (torch.from_numpy(xr) - torch.from_numpy(xr).mean()) / torch.from_numpy(xr).std()
        whole[name] = (xr.numpy(), R.resample_labels_to_host(y, shape, ratios, labels))
    seen = 0
    for batch in q:
        for xp, yp in zip(batch["source"]["data"].numpy(), batch["gt"]["data"].numpy()):
            assert xp.shape == (1, 8, 8, 8) and yp.shape == (1, 8, 8, 8)
            hits = 0
            for xr, yr in whole.values():                    # the patch is a window of one resampled volume, image and labels alike
                for z in range(xr.shape[0] - 7):
                    for yy in range(xr.shape[1] - 7):
                        for xx in np.flatnonzero(xr[z, yy, :xr.shape[2] - 7] == xp[0, 0, 0, 0]):
                            hits += int(np.array_equal(xr[z:z + 8, yy:yy + 8, xx:xx + 8], xp[0]) and
                                        np.array_equal(yr[z:z + 8, yy:yy + 8, xx:xx + 8], yp[0]))
            assert hits == 1
            seen += 1
    assert seen == 8


def test_queue_refusals(cohort):
    d, g, f, vols, spacings = cohort
    spec = R.ResampleSpec((1.0, 1.0, 1.0), spacings=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="data_path=synthetic"):
        data.make_loader(cfg(data_path="synthetic", resample_spacing="1,1,1", spacing="1,1,1", iters_per_epoch=1), torch.device("cpu"), 1)
    with pytest.raises(ValueError, match="data_path=synthetic"):
        R.refuse_for_training(spec, "synthetic")
    big = R.ResampleSpec((5.0, 5.0, 5.0), spacings=(1.0, 1.0, 1.0))              # 8 x 20 x 24 -> 2 x 4 x 5: below the patch
    q = data.DevicePatchQueue(d, g, (8, 8, 8), 1, 1, torch.device("cpu"), resample=big)
    with pytest.raises(ValueError, match=r"volume \(2, 4, 5\) \(resampled from spacing .* is smaller than the patch"):
        next(iter(q))
    missing = R.ResampleSpec((1.0, 1.0, 1.0), spacings=R.SpacingSource(table={"v0": (1.0, 1.0, 1.0)}, path="/sp.csv"))
    with pytest.raises(ValueError, match="no line for the volume v1"):          # before anything is loaded
        data.DevicePatchQueue(d, g, (8, 8, 8), 1, 4, torch.device("cpu"), resample=missing)


# ---------------------------------------------------------------------------------------------- the C-ABI: declared, exported, refusing
NAMES = ("mi355seg_bspline3_prefilter_ws_bytes", "mi355seg_bspline3_prefilter_f32", "mi355seg_bspline3_prefilter_axis_f32", "mi355seg_resample3d_f32", "mi355seg_resample3d_labels_ws_bytes",
         "mi355seg_resample3d_labels_f32", "mi355seg_resample3d_labels_i64", "mi355seg_resample3d_argmax_f32")


def test_abi_symbols_are_declared_and_exported():
    protos = parse_header(HEADER)
    cdll = ctypes.CDLL(LIB_PATH)
    for n in NAMES:
        assert n in protos and hasattr(cdll, n), n
    assert [name for _, name in protos["mi355seg_resample3d_f32"][1]] == ["x", "C", "D", "H", "W", "order", "base", "frac", "base_host", "y", "Do",
                                                                          "Ho", "Wo", "stream"]


def test_functional_refuses_cpu_tensors_and_bad_arguments():
    x = torch.zeros(4, 4, 4)
    for call in (lambda: F.resample_volume(x, (1, 1, 1), (2, 2, 2)), lambda: F.bspline3_prefilter(x),
                 lambda: F.resample_labels(x, (1, 1, 1), (2, 2, 2)), lambda: F.resample_back_labels(x.long(), (8, 8, 8), (1, 1, 1), (2, 2, 2)),
                 lambda: F.resample_back_argmax(x[None], (8, 8, 8), (1, 1, 1), (2, 2, 2))):
        with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="order must be one of"):
        F.resample_volume(x, (1, 1, 1), (2, 2, 2), order=2)
    with pytest.raises(ValueError, match="three positive numbers"):
        F.resample_volume(x, (1, 1), (2, 2, 2))
    with pytest.raises(ValueError, match="mode must be one of"):
        F.resample_labels(x, (1, 1, 1), (2, 2, 2), mode="cubic")
