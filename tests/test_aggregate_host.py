"""Soft sliding-window aggregation (overlap_mode = average | hann | gaussian), the parts that need no GPU: the patch windows and the
separable normaliser of predict.py (fp64), the three config keys, the refusals of sliding_window_predict and functional, and the
C-ABI of csrc/aggregate.hip (symbols, prototypes, refusals that never launch)."""
import ctypes

import numpy as np
import pytest
import torch

import mi355seg
from mi355seg._lib import HEADER, LIB_PATH, parse_header
from mi355seg.config import Config
from mi355seg.predict import (axis_weight_sums, grid_locations, parse_overlap_mode, parse_patch_overlap, parse_save_probabilities,
                              sliding_window_predict, window_weights)

# volume, patch, overlap, classes (tests/test_gpu_aggregate.py runs the kernels on the same grids)
GRIDS = [
    ((40, 48, 72), (32, 32, 32), (4, 4, 12), 2),      # the grid of test_gpu_unet.py
    ((40, 50, 61), (16, 32, 18), (4, 8, 6), 3),       # anisotropic patch, odd W, width not a multiple of 4
    ((32, 32, 32), (32, 32, 32), (4, 4, 4), 2),       # one patch
    ((40, 40, 71), (32, 32, 32), (16, 16, 16), 4),    # half-patch overlap, border-flush last patch: 3 per axis, 12 per voxel; odd W
    ((20, 24, 37), (16, 16, 16), (8, 8, 8), 2),
]
SOFT_MODES = ("average", "hann", "gaussian")


def brute_weight_volume(size, patch, overlap, weights):
    """torchio's accumulated 3-D weight volume: ws[dst] += w3 for every patch of the grid, fp64"""
    w3 = weights[0][:, None, None] * weights[1][None, :, None] * weights[2][None, None, :]
    ws = np.zeros(size, dtype=np.float64)
    for z, y, x in grid_locations(size, patch, overlap):
        ws[z:z + patch[0], y:y + patch[1], x:x + patch[2]] += w3
    return ws


@pytest.mark.parametrize("p", [2, 3, 16, 18, 31, 32, 128])
def test_hann_window_is_torchios(p):
    want = torch.hann_window(p + 2, periodic=False, dtype=torch.float64)[1:-1].numpy()
    for got in window_weights("hann", (p, p, p)):
        assert got.dtype == np.float64 and got.shape == (p,)
        assert np.abs(got - want).max() <= 1e-15


@pytest.mark.parametrize("mode", SOFT_MODES)
@pytest.mark.parametrize("patch", [(16, 32, 18), (1, 2, 3), 32])
def test_windows_are_symmetric_and_positive(mode, patch):
    ws = window_weights(mode, patch)
    ps = (patch,) * 3 if isinstance(patch, int) else patch
    assert len(ws) == 3 and [w.shape for w in ws] == [(p,) for p in ps]
    for w in ws:
        assert w.dtype == np.float64 and (w > 0).all() and (w <= 1).all()
        assert np.abs(w - w[::-1]).max() <= 1e-15
        if mode == "average":
            assert (w == 1).all()
        elif len(w) > 2:
            assert w.argmax() in ((len(w) - 1) // 2, len(w) // 2) and w[0] == w.min()


def test_gaussian_window_is_sigma_patch_over_eight():
    k = np.arange(32)
    for w in window_weights("gaussian", 32):
        assert np.abs(w - np.exp(-0.5 * ((k - 15.5) / 4.0) ** 2)).max() <= 1e-16
    wz, wy, wx = window_weights("gaussian", (16, 32, 18))
    assert np.abs(wy - np.exp(-0.5 * ((k - 15.5) / 4.0) ** 2)).max() <= 1e-16 and len(wz) == 16 and len(wx) == 18


def test_window_weights_refuses_crop_and_unknown_modes():
    for bad in ("crop", "hamming", None):
        with pytest.raises(ValueError, match="mode"):
            window_weights(bad, 8)


@pytest.mark.parametrize("grid", range(len(GRIDS)))
@pytest.mark.parametrize("mode", SOFT_MODES)
def test_axis_weight_sums_multiply_to_the_accumulated_weight_volume(grid, mode):
    size, patch, overlap, _ = GRIDS[grid]
    w = window_weights(mode, patch)
    sz, sy, sx = axis_weight_sums(size, patch, overlap, w)
    assert [s.shape for s in (sz, sy, sx)] == [(n,) for n in size] and all(s.dtype == np.float64 for s in (sz, sy, sx))
    want = brute_weight_volume(size, patch, overlap, w)
    got = sz[:, None, None] * sy[None, :, None] * sx[None, None, :]
    assert want.min() > 0
    rel = (np.abs(got - want) / want).max()
    print(f"grid {grid} {mode}: separable normaliser vs accumulated volume, max relative difference {rel:.2e}")
    assert rel <= 1e-14


def test_axis_weight_sums_follows_grid_locations_refusals():
    w = window_weights("average", (8, 8, 8))
    with pytest.raises(ValueError, match="overlap"):
        axis_weight_sums((16, 16, 16), (8, 8, 8), (3, 0, 0), w)
    with pytest.raises(ValueError, match="larger"):
        axis_weight_sums((4, 16, 16), (8, 8, 8), (0, 0, 0), w)


def test_config_keys_absent_mean_today():
    for cfg in (Config({}), Config({"overlap_mode": None, "patch_overlap": "None", "save_probabilities": ""})):
        assert parse_overlap_mode(cfg) == "crop"
        assert parse_patch_overlap(cfg, (32, 32, 32)) is None
        assert parse_save_probabilities(cfg, "crop") is False


def test_config_keys_values():
    for m in ("crop", "average", "hann", "gaussian"):
        assert parse_overlap_mode(Config({"overlap_mode": m})) == m
    assert parse_patch_overlap(Config({"patch_overlap": 8}), (32, 32, 32)) == (8, 8, 8)
    assert parse_patch_overlap(Config({"patch_overlap": "8"}), (32, 32, 32)) == (8, 8, 8)
    assert parse_patch_overlap(Config({"patch_overlap": "4,8, 16"}), (16, 32, 18)) == (4, 8, 16)
    assert parse_patch_overlap(Config({"patch_overlap": (0, 2, 30)}), (32, 32, 32)) == (0, 2, 30)
    assert parse_patch_overlap(Config({"patch_overlap": 0}), (32, 32, 32)) == (0, 0, 0)
    assert parse_save_probabilities(Config({"save_probabilities": True}), "hann") is True
    assert parse_save_probabilities(Config({"save_probabilities": "true"}), "average") is True
    assert parse_save_probabilities(Config({"save_probabilities": False}), "crop") is False


@pytest.mark.parametrize("bad", ["max", "Hann", 3, True, ["hann"]])
def test_overlap_mode_refuses_other_values(bad):
    with pytest.raises(ValueError, match="config.overlap_mode") as e:
        parse_overlap_mode(Config({"overlap_mode": bad}))
    assert repr(bad) in str(e.value)


@pytest.mark.parametrize("bad", [3, "4,4", "4,4,4,4", "4,5,4", 32, "4,4,32", -2, "a", 2.0, True, "4,,4"])
def test_patch_overlap_refuses_odd_large_negative_and_malformed_values(bad):
    with pytest.raises(ValueError, match="config.patch_overlap") as e:
        parse_patch_overlap(Config({"patch_overlap": bad}), (32, 32, 32))
    assert repr(bad) in str(e.value)


def test_save_probabilities_needs_a_blending_mode_and_a_boolean():
    with pytest.raises(ValueError, match="config.save_probabilities.*config.overlap_mode"):
        parse_save_probabilities(Config({"save_probabilities": True}), "crop")
    for bad in (1, "yes", 0.5):
        with pytest.raises(ValueError, match="config.save_probabilities") as e:
            parse_save_probabilities(Config({"save_probabilities": bad}), "hann")
        assert repr(bad) in str(e.value)


def test_sliding_window_predict_refuses_before_it_touches_the_model():
    vol = torch.zeros((1, 8, 8, 8))
    with pytest.raises(ValueError, match="overlap_mode.*'max'"):
        sliding_window_predict(None, vol, 8, (0, 0, 0), overlap_mode="max")
    with pytest.raises(ValueError, match="return_probabilities"):
        sliding_window_predict(None, vol, 8, (0, 0, 0), return_probabilities=True)
    with pytest.raises(ValueError, match="return_probabilities"):
        sliding_window_predict(None, vol, 8, (0, 0, 0), overlap_mode="crop", return_probabilities=True)


def test_functional_refuses_cpu_tensors():
    F = mi355seg.functional
    assert F.OVERLAP_MODES == ("crop", "average", "hann", "gaussian")
    acc, logits, table = torch.zeros((2, 8, 8, 8)), torch.zeros((1, 2, 8, 8, 8)), torch.zeros((1, 9), dtype=torch.int32)
    w = window_weights("average", 8)
    with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):
        F.aggregate_patches(acc, logits, table, 0, w)
    with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):
        F.aggregate_finalize(acc, w)
    with pytest.raises(mi355seg.Mi355SegError):
        F.aggregate_finalize(acc.double(), w)


NAMES = ("mi355seg_aggregate_patches_f32", "mi355seg_aggregate_finalize_f32")


def test_abi_symbols_are_declared_and_exported():
    protos = parse_header(HEADER)
    cdll = ctypes.CDLL(LIB_PATH)
    for n in NAMES:
        assert n in protos and hasattr(cdll, n), n
    assert [name for _, name in protos[NAMES[0]][1]] == ["logits", "K", "table", "first", "count", "pd", "ph", "pw", "wz", "wy", "wx",
                                                         "acc", "D", "H", "W", "stream"]
    args = dict((name, t) for t, name in protos[NAMES[0]][1])
    assert args["logits"] == "const float*" and args["table"] == "const int*" and args["acc"] == "float*" and args["wx"] == "const float*"
    assert [name for _, name in protos[NAMES[1]][1]] == ["acc", "K", "D", "H", "W", "sz", "sy", "sx", "labels", "prob", "stream"]
    args = dict((name, t) for t, name in protos[NAMES[1]][1])
    assert args["acc"] == "const float*" and args["labels"] == "int64_t*" and args["prob"] == "float*" and args["stream"] == "void*"


def test_bad_arguments_return_error_codes_and_never_launch():
    """Null pointers everywhere: a call that got past its argument checks would fault, not raise."""
    L = mi355seg.lib()

    def patches(K=2, first=0, count=1, patch=(8, 8, 8), vol=(16, 16, 16)):
        L.call("mi355seg_aggregate_patches_f32", None, K, None, first, count, *patch, None, None, None, None, *vol, None)

    for K in (1, 0, 17, -3):
        with pytest.raises(mi355seg.Mi355SegError, match=f"aggregate_patches: K .*{K}"):
            patches(K=K)
        with pytest.raises(mi355seg.Mi355SegError, match=f"aggregate_finalize: K .*{K}"):
            L.call("mi355seg_aggregate_finalize_f32", None, K, 4, 4, 4, None, None, None, None, None, None)
    for patch in ((17, 8, 8), (8, 17, 8), (8, 8, 17)):
        with pytest.raises(mi355seg.Mi355SegError, match="larger than the volume"):
            patches(patch=patch)
    for kw in ({"count": 0}, {"first": -1}, {"patch": (0, 8, 8)}):
        with pytest.raises(mi355seg.Mi355SegError, match="aggregate_patches: bad arguments"):
            patches(**kw)
    with pytest.raises(mi355seg.Mi355SegError, match="aggregate_patches: null"):
        patches()
    with pytest.raises(mi355seg.Mi355SegError, match="aggregate_finalize: extents"):
        L.call("mi355seg_aggregate_finalize_f32", None, 2, 4, 0, 4, None, None, None, None, None, None)
    with pytest.raises(mi355seg.Mi355SegError, match="aggregate_finalize: null"):
        L.call("mi355seg_aggregate_finalize_f32", None, 2, 4, 4, 4, None, None, None, None, None, None)
    # a probability volume without the three normalisers is a null pointer too (host addresses: never dereferenced)
    buf = (ctypes.c_float * 4)()
    a = ctypes.addressof(buf)
    with pytest.raises(mi355seg.Mi355SegError, match="aggregate_finalize: null"):
        L.call("mi355seg_aggregate_finalize_f32", a, 2, 4, 4, 4, None, None, None, a, a, None)
