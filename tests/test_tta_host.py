"""Mirror test-time augmentation of the sliding-window inference, the parts that need no GPU: the flip codes, the two config keys,
the normaliser of a blend that holds F predictions of every patch, the refusals of sliding_window_predict and of functional, and the
C-ABI of the two mirrored launches (symbols, prototypes, refusals that never launch)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import mi355seg
from mi355seg._lib import HEADER, LIB_PATH, parse_header
from mi355seg.config import Config
from mi355seg.predict import (axis_weight_sums, check_tta_flips, parse_tta, sliding_window_predict, tta_axis_sums, window_weights)

F = mi355seg.functional
SUBSETS = [s for n in (1, 2, 3) for s in itertools.permutations(("z", "y", "x"), n)]
BIT = {"z": 4, "y": 2, "x": 1}


def test_axes_and_bits():
    assert F.TTA_AXES == ("z", "y", "x")
    assert F.tta_flip_codes() == F.tta_flip_codes(F.TTA_AXES) == tuple(range(8))
    assert F.tta_flip_codes("x") == F.tta_flip_codes(("x",)) == (0, 1)
    assert F.tta_flip_codes(("y",)) == (0, 2) and F.tta_flip_codes(("z",)) == (0, 4)
    assert F.tta_flip_codes(("z", "x")) == (0, 1, 4, 5) and F.tta_flip_codes(("y", "x")) == (0, 1, 2, 3)
    assert F.tta_flip_codes(("z", "y")) == (0, 2, 4, 6)


@pytest.mark.parametrize("axes", SUBSETS)
def test_flip_codes_of_every_axis_subset_in_any_order(axes):
    codes = F.tta_flip_codes(axes)
    mask = sum(BIT[a] for a in axes)
    assert isinstance(codes, tuple) and codes[0] == 0 and list(codes) == sorted(set(codes))
    assert len(codes) == 2 ** len(axes) and len(codes) in (2, 4, 8)
    assert set(codes) == {c for c in range(8) if c | mask == mask}
    assert check_tta_flips(codes) == codes


@pytest.mark.parametrize("bad", [(), [], ("w",), ("x", "x"), ("z", "y", "x", "z"), "xy", (0,), ("X",)])
def test_flip_codes_refuse_empty_unknown_and_duplicate_axes(bad):
    with pytest.raises(ValueError, match="tta_flip_codes"):
        F.tta_flip_codes(bad)


def test_config_keys_absent_mean_off():
    for cfg in (Config({}), Config({"tta": None}), Config({"tta": ""}), Config({"tta": "none"}), Config({"tta": "None", "tta_axes": ""}),
                Config({"tta": "none", "tta_axes": None})):
        assert parse_tta(cfg) is None


def test_config_keys_values():
    assert parse_tta(Config({"tta": "mirror"})) == tuple(range(8))
    assert parse_tta(Config({"tta": "mirror", "tta_axes": "z,y,x"})) == tuple(range(8))
    assert parse_tta(Config({"tta": "mirror", "tta_axes": "x"})) == (0, 1)
    assert parse_tta(Config({"tta": "mirror", "tta_axes": "x, z"})) == (0, 1, 4, 5)
    assert parse_tta(Config({"tta": "mirror", "tta_axes": ("y", "x")})) == (0, 1, 2, 3)
    assert parse_tta(Config({"tta": "mirror", "tta_axes": ["z"]})) == (0, 4)
    assert parse_tta(Config({"tta": "mirror", "tta_axes": "(y,z)"})) == (0, 2, 4, 6)


@pytest.mark.parametrize("bad", ["flip", "Mirror", "rotate", True, 1, ["mirror"]])
def test_tta_refuses_other_values(bad):
    with pytest.raises(ValueError, match="config.tta ") as e:
        parse_tta(Config({"tta": bad}))
    assert repr(bad) in str(e.value)


@pytest.mark.parametrize("bad", ["w", "x,x", "z,y,x,z", "x,,y", "zyx", 3, True, ("x", "w"), ["x", "x"], 0.5])
def test_tta_axes_refuses_unknown_axes_and_duplicates(bad):
    with pytest.raises(ValueError, match="config.tta_axes") as e:
        parse_tta(Config({"tta": "mirror", "tta_axes": bad}))
    assert repr(bad) in str(e.value)


@pytest.mark.parametrize("tta", [None, "", "none"])
def test_tta_axes_without_tta_is_an_error(tta):
    with pytest.raises(ValueError, match="config.tta_axes.*config.tta=mirror"):
        parse_tta(Config({"tta_axes": "x"} if tta is None else {"tta": tta, "tta_axes": "x"}))


@pytest.mark.parametrize("flips", [(0, 1), (0, 2, 4, 6), tuple(range(8))])
@pytest.mark.parametrize("mode", ["average", "hann", "gaussian"])
def test_normaliser_of_f_flips_is_exactly_f_times_the_plain_one(flips, mode):
    """(F * sz[z] * sy[y]) * sx[x] in fp32, formed as aggregate_finalize forms it, is F * ((sz[z] * sy[y]) * sx[x]) bit for bit."""
    size, patch, overlap = (20, 24, 37), (16, 16, 16), (8, 8, 8)
    sums = [s.astype(np.float32) for s in axis_weight_sums(size, patch, overlap, window_weights(mode, patch))]
    got = tta_axis_sums(sums, flips)
    n = np.float32(len(flips))
    assert got[0].dtype == np.float32 and np.array_equal(got[0], n * sums[0]) and got[1] is sums[1] and got[2] is sums[2]
    plain = (sums[0][:, None, None] * sums[1][None, :, None]) * sums[2][None, None, :]
    scaled = (got[0][:, None, None] * got[1][None, :, None]) * got[2][None, None, :]
    assert scaled.dtype == np.float32 and np.array_equal(scaled, n * plain)
    # the same on torch tensors, which is what sliding_window_predict hands over
    t = tta_axis_sums([torch.from_numpy(s) for s in sums], flips)
    assert t[0].dtype == torch.float32 and np.array_equal(t[0].numpy(), got[0])
    # so the mean of F equal probabilities p is p: (F terms of w * p) / (F * w) -- here in fp64 on the fp32 normalisers
    assert np.array_equal(scaled.astype(np.float64) / len(flips), plain.astype(np.float64))


def test_check_tta_flips():
    assert check_tta_flips(None) is None and check_tta_flips((0,)) is None and check_tta_flips([0]) is None
    assert check_tta_flips([0, 1]) == (0, 1) and check_tta_flips((0, 1, 4, 5)) == (0, 1, 4, 5)
    for bad in ((), (1,), (0, 8), (-1, 0), (0, 1, 2), (1, 0), (0, 0, 1), (0, 3), (0, 1.0), (0, True), (0, 1, 2, 3, 4)):
        with pytest.raises(ValueError, match="tta_flips"):
            check_tta_flips(bad)


def test_sliding_window_predict_refuses_before_it_touches_the_model():
    vol = torch.zeros((1, 8, 8, 8))
    for bad in ((0, 8), (0, -1), (0, 3), (2, 0), ("x",)):
        with pytest.raises(ValueError, match="tta_flips"):
            sliding_window_predict(None, vol, 8, (0, 0, 0), tta_flips=bad)
        with pytest.raises(ValueError, match="tta_flips"):
            sliding_window_predict(None, vol, 8, (0, 0, 0), overlap_mode="hann", tta_flips=bad)
    with pytest.raises(ValueError, match="return_probabilities"):
        sliding_window_predict(None, vol, 8, (0, 0, 0), return_probabilities=True, tta_flips=(0, 1))


def test_wrappers_refuse_bad_flip_codes_and_cpu_tensors():
    vol, table = torch.zeros((1, 8, 8, 8)), torch.zeros((1, 9), dtype=torch.int32)
    acc, logits = torch.zeros((2, 8, 8, 8)), torch.zeros((1, 2, 8, 8, 8))
    w = window_weights("average", 8)
    for bad in (-1, 8, 1.0, True, None, "x"):
        with pytest.raises(mi355seg.Mi355SegError, match="gather_patches: flip .*0..7") as e:
            F.gather_patches(vol, table, 0, 1, 8, flip=bad)
        assert repr(bad) in str(e.value)
        with pytest.raises(mi355seg.Mi355SegError, match="aggregate_patches: flip .*0..7") as e:
            F.aggregate_patches(acc, logits, table, 0, w, flip=bad)
        assert repr(bad) in str(e.value)
    for flip in (0, 1, 7):
        with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):
            F.gather_patches(vol, table, 0, 1, 8, flip=flip)
        with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):
            F.gather_patches(vol, table, 0, 1, (9, 8, 8), flip=flip)
        with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):
            F.aggregate_patches(acc, logits, table, 0, w, flip=flip)


NAMES = ("mi355seg_gather_patches_flip_f32", "mi355seg_aggregate_patches_flip_f32")


def test_abi_symbols_are_declared_and_exported():
    protos = parse_header(HEADER)
    cdll = ctypes.CDLL(LIB_PATH)
    for n in NAMES:
        assert n in protos and hasattr(cdll, n), n
    plain = [name for _, name in protos["mi355seg_gather_patches_f32"][1]]
    assert [name for _, name in protos[NAMES[0]][1]] == plain[:-2] + ["flip"] + plain[-2:] == \
        ["vol", "C", "D", "H", "W", "table", "first", "count", "pd", "ph", "pw", "flip", "out", "stream"]
    assert [name for _, name in protos[NAMES[1]][1]] == ["logits", "K", "table", "first", "count", "pd", "ph", "pw", "wz", "wy", "wx", "flip",
                                                         "acc", "D", "H", "W", "stream"]
    for n in NAMES:
        args = dict((name, t) for t, name in protos[n][1])
        assert args["flip"] == "int" and args["table"] == "const int*" and args["stream"] == "void*"
    # the un-mirrored prototypes are the parent's
    assert [name for _, name in protos["mi355seg_aggregate_patches_f32"][1]] == ["logits", "K", "table", "first", "count", "pd", "ph", "pw",
                                                                                "wz", "wy", "wx", "acc", "D", "H", "W", "stream"]


def test_bad_arguments_return_error_codes_and_never_launch():
    """Host addresses that are never dereferenced, or null pointers: a call that got past its argument checks would fault, not raise."""
    L = mi355seg.lib()
    buf = (ctypes.c_float * 4)()
    a = ctypes.addressof(buf)

    def gather(flip=0, patch=(8, 8, 8), vol=(16, 16, 16), ptr=a, count=1):
        L.call(NAMES[0], ptr, 1, *vol, ptr, 0, count, *patch, flip, ptr, None)

    def patches(flip=0, K=2, first=0, count=1, patch=(8, 8, 8), vol=(16, 16, 16), ptr=a):
        L.call(NAMES[1], ptr, K, ptr, first, count, *patch, ptr, ptr, ptr, flip, ptr, *vol, None)

    for flip in (-1, 8, 9, -8, 1 << 20):
        with pytest.raises(mi355seg.Mi355SegError, match=f"gather_patches_flip: flip .*0..7.* {flip}$"):
            gather(flip=flip)
        with pytest.raises(mi355seg.Mi355SegError, match=f"aggregate_patches_flip: flip .*0..7.* {flip}$"):
            patches(flip=flip)
    for flip in (0, 5):
        for patch in ((17, 8, 8), (8, 17, 8), (8, 8, 17)):
            with pytest.raises(mi355seg.Mi355SegError, match="gather_patches_flip: bad arguments .*17"):
                gather(flip=flip, patch=patch)
            with pytest.raises(mi355seg.Mi355SegError, match="aggregate_patches_flip: patch .*larger than the volume"):
                patches(flip=flip, patch=patch)
        with pytest.raises(mi355seg.Mi355SegError, match="gather_patches_flip: bad arguments"):
            gather(flip=flip, ptr=None)
        with pytest.raises(mi355seg.Mi355SegError, match="gather_patches_flip: bad arguments"):
            gather(flip=flip, count=0)
        with pytest.raises(mi355seg.Mi355SegError, match="aggregate_patches_flip: null"):
            patches(flip=flip, ptr=None)
        for K in (1, 17):
            with pytest.raises(mi355seg.Mi355SegError, match=f"aggregate_patches_flip: K .*{K}"):
                patches(flip=flip, K=K)
        for kw in ({"count": 0}, {"first": -1}, {"patch": (0, 8, 8)}):
            with pytest.raises(mi355seg.Mi355SegError, match="aggregate_patches_flip: bad arguments"):
                patches(flip=flip, **kw)
