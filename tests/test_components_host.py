"""Connected-component clean-up, the parts that need no GPU: which components stay (functional.select_components, plain tensor code),
the config keys of predict.py (parse_postprocess), and the C-ABI of csrc/components.hip (symbols, prototypes, refusals that never
launch)."""
import ctypes

import pytest
import torch

import mi355seg
from mi355seg._lib import HEADER, LIB_PATH, parse_header
from mi355seg.config import Config
from mi355seg.functional import select_components
from mi355seg.predict import parse_postprocess


def _table(pairs):
    """[(label, size), ...] -> the compact table select_components takes"""
    return torch.tensor([p[0] for p in pairs], dtype=torch.int32), torch.tensor([p[1] for p in pairs], dtype=torch.int32)


def test_min_voxels_keeps_a_component_of_exactly_that_size():
    lab, sz = _table([(1, 4), (10, 5), (20, 6), (31, 1)])
    keep = select_components(lab, sz, min_voxels=5)
    assert keep.dtype == torch.int32 and keep.tolist() == [10, 20]
    assert select_components(lab, sz, min_voxels=6).tolist() == [20]
    assert select_components(lab, sz).tolist() == [1, 10, 20, 31]
    assert select_components(lab, sz, min_voxels=1).tolist() == [1, 10, 20, 31]


def test_keep_largest_breaks_ties_by_the_smaller_label():
    lab, sz = _table([(3, 9), (40, 50), (7, 50), (90, 2)])
    assert select_components(lab, sz, keep_largest=1).tolist() == [7]
    assert select_components(lab, sz, keep_largest=2).tolist() == [7, 40]
    assert select_components(lab, sz, keep_largest=3).tolist() == [7, 40, 3]
    # the table's order does not matter
    assert select_components(lab.flip(0), sz.flip(0), keep_largest=1).tolist() == [7]


def test_keep_largest_beyond_the_number_of_components_keeps_all():
    lab, sz = _table([(5, 1), (2, 8), (9, 3)])
    assert select_components(lab, sz, keep_largest=16).tolist() == [2, 9, 5]
    assert select_components(lab, sz, min_voxels=2, keep_largest=16).tolist() == [2, 9]
    empty = _table([])
    assert select_components(*empty, keep_largest=3).tolist() == []


def test_keep_largest_after_min_voxels_removed_everything_is_empty():
    lab, sz = _table([(5, 1), (2, 8)])
    keep = select_components(lab, sz, min_voxels=9, keep_largest=1)
    assert keep.dtype == torch.int32 and keep.numel() == 0


def test_keep_largest_bounds():
    lab, sz = _table([(i + 1, 100 - i) for i in range(20)])
    assert select_components(lab, sz, keep_largest=16).tolist() == list(range(1, 17))
    for bad in (17, -1):
        with pytest.raises(mi355seg.Mi355SegError, match=str(bad)):
            select_components(lab, sz, keep_largest=bad)
    with pytest.raises(mi355seg.Mi355SegError, match="-3"):
        select_components(lab, sz, min_voxels=-3)


def test_sizes_near_the_int32_limit_order_correctly():
    lab, sz = _table([(2_000_000_000, 2_147_483_000), (1, 2_147_483_001), (7, 3)])
    assert select_components(lab, sz, keep_largest=2).tolist() == [1, 2_000_000_000]


def test_parse_postprocess_absent_keys_mean_off():
    assert parse_postprocess(Config({})) is None
    assert parse_postprocess(Config({"keep_largest": 0, "min_component_voxels": 0})) is None
    assert parse_postprocess(Config({"keep_largest": None, "min_component_voxels": "None"})) is None
    # connectivity is read only when one of the two keys is set
    assert parse_postprocess(Config({"connectivity": 4})) is None


def test_parse_postprocess_values():
    assert parse_postprocess(Config({"keep_largest": 1})) == (1, 0, 26)
    assert parse_postprocess(Config({"min_component_voxels": 50})) == (0, 50, 26)
    assert parse_postprocess(Config({"keep_largest": "2", "min_component_voxels": "7", "connectivity": "18"})) == (2, 7, 18)
    for c in (6, 18, 26):
        assert parse_postprocess(Config({"keep_largest": 16, "connectivity": c})) == (16, 0, c)


@pytest.mark.parametrize("bad", [4, 27, "x"])
def test_parse_postprocess_refuses_other_connectivities(bad):
    with pytest.raises(ValueError, match=repr(bad).replace("'", ".")):
        parse_postprocess(Config({"keep_largest": 1, "connectivity": bad}))


@pytest.mark.parametrize("key,bad", [("keep_largest", -1), ("min_component_voxels", -5), ("keep_largest", 17), ("keep_largest", "two"),
                                     ("min_component_voxels", 1.5)])
def test_parse_postprocess_refuses_bad_counts(key, bad):
    with pytest.raises(ValueError, match=key) as e:
        parse_postprocess(Config({key: bad}))
    assert repr(bad) in str(e.value)


NAMES = ("mi355seg_components_ws_bytes", "mi355seg_components_label_i64", "mi355seg_components_filter_i64")


def test_abi_symbols_are_declared_and_exported():
    protos = parse_header(HEADER)
    cdll = ctypes.CDLL(LIB_PATH)
    for n in NAMES:
        assert n in protos and hasattr(cdll, n), n
    assert protos["mi355seg_components_ws_bytes"] == ("size_t", [("int", "D"), ("int", "H"), ("int", "W")])
    args = dict((name, t) for t, name in protos["mi355seg_components_label_i64"][1])
    assert args["mask"] == "const int64_t*" and args["labels"] == "int32_t*" and args["sizes"] == "int32_t*" and args["info"] == "int64_t*"
    assert args["connectivity"] == "int" and args["ws_bytes"] == "size_t" and args["stream"] == "void*"
    args = dict((name, t) for t, name in protos["mi355seg_components_filter_i64"][1])
    assert args["keep_labels"] == "const int32_t*" and args["n_keep"] == "int" and args["min_voxels"] == "long long"
    assert args["out"] == "int64_t*" and args["removed"] == "int64_t*" and args["numel"] == "long long"


def test_workspace_query_and_tile_shape():
    L = mi355seg.lib()
    assert L.query("mi355seg_components_ws_bytes", 128, 128, 128) >= 4 * 128 ** 3
    assert L.query("mi355seg_components_ws_bytes", 1, 1, 1) > 0
    assert L.query("mi355seg_components_ws_bytes", 0, 4, 4) == 0
    assert L.query("mi355seg_components_ws_bytes", 2048, 1024, 1024) == 0           # 2^31 voxels
    assert L.query("mi355seg_components_ws_bytes", 1, 1, 2 ** 31 - 2) > 0
    tile = mi355seg.functional.components_tile()
    assert len(tile) == 3 and all(t >= 1 for t in tile) and 1024 <= tile[0] * tile[1] * tile[2] <= 16384
    assert L.query("mi355seg_components_tile_extent", 3) == 0


def test_bad_arguments_return_error_codes_and_never_launch():
    """Null pointers everywhere: a call that got past its argument checks would fault, not raise."""
    L = mi355seg.lib()
    big = 1 << 40
    with pytest.raises(mi355seg.Mi355SegError, match="connectivity.*5"):
        L.call("mi355seg_components_label_i64", None, 4, 4, 4, 5, None, None, None, None, big, None)
    with pytest.raises(mi355seg.Mi355SegError, match="components_label"):
        L.call("mi355seg_components_label_i64", None, 0, 4, 4, 26, None, None, None, None, big, None)
    with pytest.raises(mi355seg.Mi355SegError, match="2\\^31 - 2"):
        L.call("mi355seg_components_label_i64", None, 2048, 1024, 1024, 26, None, None, None, None, big, None)
    with pytest.raises(mi355seg.Mi355SegError, match="null"):
        L.call("mi355seg_components_label_i64", None, 4, 4, 4, 26, None, None, None, None, big, None)
    with pytest.raises(mi355seg.Mi355SegError, match="workspace too small"):
        L.call("mi355seg_components_label_i64", None, 4, 4, 4, 26, None, None, None, None, 16, None)
    for steps in (0, 6):
        with pytest.raises(mi355seg.Mi355SegError, match=f"steps.*{steps}"):
            L.call("mi355seg_components_label_steps_i64", None, 4, 4, 4, 26, None, None, None, None, big, steps, None)
    with pytest.raises(mi355seg.Mi355SegError, match="17"):
        L.call("mi355seg_components_filter_i64", None, None, None, 64, 0, None, 17, None, None, None)
    with pytest.raises(mi355seg.Mi355SegError, match="components_filter"):
        L.call("mi355seg_components_filter_i64", None, None, None, 64, 0, None, -1, None, None, None)
    with pytest.raises(mi355seg.Mi355SegError, match="components_filter"):
        L.call("mi355seg_components_filter_i64", None, None, None, 2 ** 31 - 1, 0, None, 0, None, None, None)
    with pytest.raises(mi355seg.Mi355SegError, match="null"):
        L.call("mi355seg_components_filter_i64", None, None, None, 64, 0, None, 0, None, None, None)
