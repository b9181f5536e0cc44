"""Per-class connected components, the parts that need no GPU: the per-class selection against a brute numpy
selection, the refusals of the functional entry points, the two predict keys with theirs, the CSV writer, and the C-ABI of the new
entry points (symbols, workspace sizes, refusals that never launch)."""
import csv

import numpy as np
import pytest
import torch

import mi355seg
from mi355seg import functional as F
from mi355seg._lib import parse_header
from mi355seg.config import Config, _parse_value


# ----------------------------------------------------------------------------- select_components_by_class
def brute_select(cls, size, min_voxels, keep_largest):
    get = lambda arg, k: arg.get(int(k), 0) if isinstance(arg, dict) else arg
    keep = np.zeros(len(cls), dtype=bool)
    for k in np.unique(cls):
        mine = [i for i in range(len(cls)) if cls[i] == k and size[i] >= get(min_voxels, k)]
        top = get(keep_largest, k)
        if top > 0:
            mine = sorted(mine, key=lambda i: (-size[i], i))[:top]
        keep[mine] = True
    return keep


ARGS = [(0, 0), (3, 0), (0, 1), (0, 2), (2, 16), (5, 3), ({1: 4}, 0), (0, {2: 1}), ({1: 2, 3: 9}, {1: 1, 2: 16, 7: 2}), (1, {3: 0, 1: 2}),
        ({2: 0}, {2: 0})]


@pytest.mark.parametrize("seed", range(6))
def test_selection_equals_a_brute_numpy_selection(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 60))
    cls = rng.integers(1, 5, n)
    size = rng.integers(1, 7, n)                     # few distinct sizes: ties within every class
    for mv, top in ARGS:
        got = F.select_components_by_class(torch.from_numpy(cls), torch.from_numpy(size).to(torch.int32), mv, top)
        assert got.dtype == torch.bool and got.shape == (n,)
        assert np.array_equal(got.numpy(), brute_select(cls, size, mv, top)), (mv, top, cls.tolist(), size.tolist())


def test_ties_keep_largest_above_the_count_and_the_empty_table():
    cls = torch.tensor([2, 1, 2, 1, 2, 1])
    size = torch.tensor([5, 7, 5, 7, 5, 3])
    sel = lambda *a: F.select_components_by_class(cls, size, *a).tolist()
    assert sel(0, 1) == [True, True, False, False, False, False]                 # of equal sizes the smaller rank
    assert sel(0, 2) == [True, True, True, True, False, False]
    assert sel(0, {2: 2}) == [True, True, True, True, False, True]               # a class that is not named: everything stays
    assert sel(0, 16) == [True] * 6                                              # more than there are
    assert sel(6, 0) == [False, True, False, True, False, False]
    assert sel({1: 4}, {1: 1, 2: 1}) == [True, True, False, False, False, False]
    assert sel(8, 3) == [False] * 6
    empty = F.select_components_by_class(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), 2, {1: 1})
    assert empty.dtype == torch.bool and empty.shape == (0,)
    stats = F.class_component_stats(cls, size, torch.tensor(sel(0, {2: 2})), classes=(3,))
    assert stats == {1: {"components": 3, "kept": 3, "voxels_removed": 0, "largest": 7},
                     2: {"components": 3, "kept": 2, "voxels_removed": 5, "largest": 5},
                     3: {"components": 0, "kept": 0, "voxels_removed": 0, "largest": 0}}


# ----------------------------------------------------------------------------- refusals of the functional entry points
def test_functional_entry_points_refuse_cpu_tensors_and_bad_arguments():
    E = mi355seg.Mi355SegError
    v = torch.zeros((4, 5, 6), dtype=torch.int64)
    lab, sizes, info = torch.zeros((4, 5, 6), dtype=torch.int32), torch.zeros(120, dtype=torch.int32), torch.zeros(8, dtype=torch.int64)
    for bad in (v, v.float(), v[0]):
        with pytest.raises(E):
            F.connected_components_by_class(bad)
        with pytest.raises(E):
            F.filter_components_by_class(bad, keep_largest=1)
        with pytest.raises(E):
            F.component_table(bad, lab, sizes, info)
    with pytest.raises(E, match="7"):
        F.connected_components_by_class(v, 7)
    with pytest.raises(E, match="connectivity"):
        F.connected_components_by_class(v, True)
    cls, size = torch.tensor([1, 2]), torch.tensor([3, 4])
    for kw in ({"keep_largest": 17}, {"keep_largest": -1}, {"keep_largest": {1: 17}}, {"keep_largest": {0: 1}}, {"keep_largest": {-1: 1}},
               {"keep_largest": 1.0}, {"keep_largest": True}, {"keep_largest": {"1": 1}}, {"min_voxels": -1}, {"min_voxels": {1: -2}},
               {"min_voxels": "3"}, {"min_voxels": {1: None}}, {"min_voxels": [1]}):
        with pytest.raises(E, match=next(iter(kw))):
            F.select_components_by_class(cls, size, **kw)
        with pytest.raises(E, match=next(iter(kw))):
            F.filter_components_by_class(v, **kw)                                 # (the arguments are looked at before the tensor)
    with pytest.raises(E, match="1..255"):
        F.filter_components_by_class(v, keep_largest={256: 1})
    with pytest.raises(E, match="2 classes and 3 sizes"):
        F.select_components_by_class(cls, torch.tensor([1, 2, 3]))
    with pytest.raises(E, match="integer tensors"):
        F.select_components_by_class(cls.float(), size)
    with pytest.raises(E):
        F.filter_by_component_table(v, lab, torch.ones(2, dtype=torch.bool))
    for bad in (256, -1):
        with pytest.raises(E, match="classes lie in 0..255"):
            F.class_component_stats(torch.tensor([1, bad]), size, torch.tensor([True, False]))


# ----------------------------------------------------------------------------- the predict keys
BASE = {"multiclass": True, "out_classes": 4, "pred_data_path": "/data"}


def test_the_two_keys_parse_to_an_int_or_a_dict():
    from mi355seg.predict import parse_class_postprocess as parse
    assert parse(Config(BASE), 4) is None and parse(Config({"out_classes": 1}), None) is None
    assert parse(Config({"out_classes": 2, "class_keep_largest": 0, "class_min_voxels": "0"}), None) is None
    for empty in (None, "", "None", "null", 0, "0"):
        assert parse(Config({**BASE, "class_keep_largest": empty, "class_min_voxels": empty}), 4) is None
    assert parse(Config({**BASE, "class_keep_largest": 1}), 4) == (1, 0, 26)
    assert parse(Config({**BASE, "class_keep_largest": "2", "connectivity": 6}), 4) == (2, 0, 6)
    assert parse(Config({**BASE, "class_min_voxels": 50, "connectivity": "18"}), 4) == (0, 50, 18)
    assert parse(Config({**BASE, "class_keep_largest": "1:1,2:1,3:2", "class_min_voxels": "3:100"}), 4) == ({1: 1, 2: 1, 3: 2}, {3: 100}, 26)
    assert parse(Config({**BASE, "class_keep_largest": "2:16,"}), 4) == ({2: 16}, 0, 26)
    assert parse(Config({**BASE, "class_keep_largest": 16, "class_min_voxels": "1: 5, 2: 7"}), 4) == (16, {1: 5, 2: 7}, 26)
    # the command line: YAML reads a single 2:1 as the base-60 number 121, so a single pair has a trailing comma or is a mapping
    assert _parse_value("1:1,2:2") == "1:1,2:2" and _parse_value("2:1,") == "2:1," and _parse_value("{2: 1}") == {2: 1} and _parse_value("2:1") == 121
    assert parse(Config({**BASE, "class_keep_largest": _parse_value("2:1,"), "class_min_voxels": _parse_value("{2: 1, 3: 40}")}), 4) == ({2: 1}, {2: 1, 3: 40}, 26)
    with pytest.raises(ValueError, match="config.class_keep_largest must be an integer in 0..16 .* trailing comma"):
        parse(Config({**BASE, "class_keep_largest": _parse_value("2:1")}), 4)


def test_the_two_keys_refuse_with_their_name():
    from mi355seg.predict import parse_class_postprocess as parse
    for key, top in (("class_keep_largest", 16), ("class_min_voxels", None)):
        for bad in (-1, "-1", 1.5, "x", True, "1:x", "a:1", "1:1:1", "1:1,1:2", "1;1", [1], {1: "x"}, {"a": 1}, ":", "1:", "1:1,,", ",1:1", "(1:1}", "{1:1,2:2}", "1:1,2"):
            with pytest.raises(ValueError, match=f"config.{key} must be"):
                parse(Config({**BASE, key: bad}), 4)
        for cls in (0, 4, 17):
            with pytest.raises(ValueError, match=f"config.{key} names class {cls}; config.out_classes=4"):
                parse(Config({**BASE, key: f"{cls}:1"}), 4)
        with pytest.raises(ValueError, match=f"config.{key} needs config.multiclass=true"):
            parse(Config({"out_classes": 4, key: 1}), None)
    for bad in (17, "1:17", "1:1,2:17"):
        with pytest.raises(ValueError, match="config.class_keep_largest must be an integer in 0..16"):
            parse(Config({**BASE, "class_keep_largest": bad}), 4)
    assert parse(Config({**BASE, "class_min_voxels": 17}), 4) == (0, 17, 26)
    for c in (7, "x", True):
        with pytest.raises(ValueError, match="config.connectivity must be 6, 18 or 26"):
            parse(Config({**BASE, "class_keep_largest": 1, "connectivity": c}), 4)
    assert parse(Config({**BASE, "connectivity": 7}), 4) is None                  # (not looked at without the keys)


def test_the_old_keys_still_raise_the_old_message_under_multiclass():
    from mi355seg.predict import parse_predict_multiclass
    for kw in ({"keep_largest": 1}, {"min_component_voxels": 10}, {"keep_largest": 1, "class_keep_largest": 1}):
        with pytest.raises(ValueError, match="config.multiclass does not go with config.keep_largest / config.min_component_voxels"):
            parse_predict_multiclass(Config({**BASE, **kw}))
    assert parse_predict_multiclass(Config({**BASE, "class_keep_largest": 1, "class_min_voxels": "1:2"})) == 4


# ----------------------------------------------------------------------------- components.csv
def test_class_components_csv(tmp_path):
    from mi355seg.predict import class_component_rows, write_class_components_csv
    stats = {1: {"components": 3, "kept": 1, "voxels_removed": 17, "largest": 40}, 3: {"components": 1, "kept": 1, "voxels_removed": 0, "largest": 9}}
    rows = class_component_rows("a", stats, 4) + class_component_rows("b", {}, 4)
    path = tmp_path / "components.csv"
    write_class_components_csv(path, rows)
    with open(path, newline="") as fh:
        got = list(csv.reader(fh))
    assert got[0] == ["file", "class", "components", "kept", "voxels_removed", "largest"]
    assert got[1:] == [["a", "1", "3", "1", "17", "40"], ["a", "2", "0", "0", "0", "0"], ["a", "3", "1", "1", "0", "9"],
                       ["b", "1", "0", "0", "0", "0"], ["b", "2", "0", "0", "0", "0"], ["b", "3", "0", "0", "0", "0"]]


# ----------------------------------------------------------------------------- C-ABI
NAMES = ("mi355seg_components_classes_ws_bytes", "mi355seg_components_label_classes_i64", "mi355seg_components_label_classes_steps_i64",
         "mi355seg_components_table_ws_bytes", "mi355seg_components_table_i64", "mi355seg_components_filter_table_i64")


def test_symbols_prototypes_and_workspace_sizes():
    protos = parse_header()
    L = mi355seg.lib()
    assert all(n in protos and hasattr(L.cdll, n) for n in NAMES)
    assert protos["mi355seg_components_label_classes_i64"] == protos["mi355seg_components_label_i64"]      # the same arguments
    from mi355seg import custom_ops
    assert "connected_components_by_class" in custom_ops.OPS
    for D, H, W in ((128, 128, 128), (1, 1, 1), (3, 5, 7)):
        assert L.query("mi355seg_components_classes_ws_bytes", D, H, W) >= L.query("mi355seg_components_ws_bytes", D, H, W) + D * H * W
    assert L.query("mi355seg_components_classes_ws_bytes", 0, 4, 4) == 0
    assert L.query("mi355seg_components_classes_ws_bytes", 2048, 1024, 1024) == 0
    assert L.query("mi355seg_components_table_ws_bytes", 1) > 0 and L.query("mi355seg_components_table_ws_bytes", 128 ** 3) >= 4 * 2048
    assert L.query("mi355seg_components_table_ws_bytes", 0) == 0 and L.query("mi355seg_components_table_ws_bytes", 2 ** 31 - 1) == 0


def test_refusals_before_any_launch():
    """every call here has null pointers: a check that let one through would fault, not raise"""
    L = mi355seg.lib()
    E = mi355seg.Mi355SegError
    big = 1 << 40
    lab = "mi355seg_components_label_classes_i64"
    for args, what in (((None, 4, 4, 4, 5, None, None, None, None, big, None), "connectivity"),
                       ((None, 0, 4, 4, 26, None, None, None, None, big, None), "extents"),
                       ((None, 2048, 1024, 1024, 26, None, None, None, None, big, None), "2\\^31"),
                       ((None, 4, 4, 4, 26, None, None, None, None, 16, None), "workspace too small"),
                       ((None, 4, 4, 4, 26, None, None, None, None, big, None), "null pointer")):
        with pytest.raises(E, match=what):
            L.call(lab, *args)
    for steps in (0, 6):
        with pytest.raises(E, match="steps"):
            L.call("mi355seg_components_label_classes_steps_i64", None, 4, 4, 4, 26, None, None, None, None, big, steps, None)
    tab = "mi355seg_components_table_i64"
    for args, what in (((None, None, None, 0, 0, None, None, None, None, None, big, None), "voxels"),
                       ((None, None, None, 2 ** 31 - 1, 0, None, None, None, None, None, big, None), "voxels"),
                       ((None, None, None, 64, -1, None, None, None, None, None, big, None), "n = -1"),
                       ((None, None, None, 64, 65, None, None, None, None, None, big, None), "n = 65"),
                       ((None, None, None, 64, 2, None, None, None, None, None, 8, None), "workspace too small"),
                       ((None, None, None, 64, 2, None, None, None, None, None, big, None), "null pointer")):
        with pytest.raises(E, match=what):
            L.call(tab, *args)
    flt = "mi355seg_components_filter_table_i64"
    for args, what in (((None, None, None, 0, 0, None, None, None), "voxels"),
                       ((None, None, None, 0, 2 ** 31 - 1, None, None, None), "voxels"),
                       ((None, None, None, -1, 64, None, None, None), "n = -1"),
                       ((None, None, None, 65, 64, None, None, None), "n = 65"),
                       ((None, None, None, 2, 64, None, None, None), "null pointer")):
        with pytest.raises(E, match=what):
            L.call(flt, *args)
