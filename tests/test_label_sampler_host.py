"""Host side of label-balanced patch sampling (``config.sampler=label``; tio.LabelSampler semantics, UNPINNED: the definitions of
include/mi355seg.h are the specification): ``mi355seg.data.draw_label_picks`` (class masses, the draw order, the refusals),
``parse_label_probabilities``, the refusals of ``DevicePatchQueue`` / ``make_loader``, and ``sampler="uniform"`` leaving the queue as it
was.  No GPU needed."""
import numpy as np
import pytest
import torch

import mi355seg
from mi355seg import data
from mi355seg.config import Config
from mi355seg.data import DevicePatchQueue, draw_label_picks, parse_label_probabilities

from test_data_queue import _write

COUNTS = np.array([900, 50, 0, 7, 1] + [0] * 11 + [0], dtype=np.int64)       # classes 0, 1, 3, 4 present; 2 and 5 .. 15 absent; bad = 0


def test_same_seed_same_picks():
    a = draw_label_picks(np.random.default_rng(5), COUNTS, None, 64)
    b = draw_label_picks(np.random.default_rng(5), COUNTS, None, 64)
    c = draw_label_picks(np.random.default_rng(6), COUNTS, None, 64)
    assert a[0].dtype == np.int64 and a[1].dtype == np.int64 and a[0].shape == (64,) and a[1].shape == (64,)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not (np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]))


@pytest.mark.parametrize("probs", [None, {0: 1.0, 1: 2.0, 3: 1.0}])
def test_draw_order_is_random_then_integers(probs):
    """per sample: u = rng.random(), then r = rng.integers(0, count[class]); nothing else is drawn (the generator ends in the same state)"""
    n = 40
    rng = np.random.default_rng(11)
    classes, ranks = draw_label_picks(rng, COUNTS, probs, n)
    if probs is None:
        mass = np.concatenate([[0.0], COUNTS[1:16].astype(np.float64)])
    else:
        mass = np.array([probs.get(l, 0.0) if COUNTS[l] > 0 else 0.0 for l in range(16)])
    cdf = np.cumsum(mass) / mass.sum()
    replay = np.random.default_rng(11)
    for i in range(n):
        u = replay.random()
        l = next(k for k in range(16) if cdf[k] > u)
        assert classes[i] == l
        assert ranks[i] == int(replay.integers(0, COUNTS[l]))
    assert rng.random() == replay.random()


def test_none_never_picks_background_and_weighs_by_count():
    n = 20000
    classes, ranks = draw_label_picks(np.random.default_rng(0), COUNTS, None, n)
    assert set(classes.tolist()) <= {1, 3, 4} and 0 not in classes
    total = COUNTS[1:16].sum()
    for l in (1, 3, 4):                                    # binomial: 5 standard deviations
        p = COUNTS[l] / total
        assert abs((classes == l).mean() - p) <= 5 * np.sqrt(p * (1 - p) / n), l
    assert (ranks >= 0).all() and (ranks < COUNTS[classes]).all()


def test_dict_entry_of_an_absent_class_drops_out_and_the_rest_renormalise():
    n = 20000
    classes, ranks = draw_label_picks(np.random.default_rng(1), COUNTS, {0: 1.0, 2: 5.0, 3: 3.0}, n)     # class 2 is absent
    assert set(classes.tolist()) == {0, 3}
    assert abs((classes == 0).mean() - 0.25) <= 5 * np.sqrt(0.25 * 0.75 / n)
    assert (ranks < COUNTS[classes]).all() and (ranks >= 0).all()
    assert ranks[classes == 3].max() == 6 and ranks[classes == 0].max() > 800       # ranks cover the class, by count and not by weight


def test_zero_weight_background_picks_only_class_one():
    classes, ranks = draw_label_picks(np.random.default_rng(2), COUNTS, {0: 0, 1: 1}, 500)
    assert (classes == 1).all() and (ranks < 50).all() and len(set(ranks.tolist())) > 25


def test_single_voxel_class_has_rank_zero():
    classes, ranks = draw_label_picks(np.random.default_rng(3), COUNTS, {4: 1.0}, 50)
    assert (classes == 4).all() and (ranks == 0).all()


def test_empty_probability_map_raises():
    with pytest.raises(RuntimeError, match="empty probability map"):
        draw_label_picks(np.random.default_rng(0), COUNTS, {2: 1.0, 9: 1.0}, 4)                 # every listed class absent
    background = np.zeros(17, dtype=np.int64)
    background[0] = 1000
    with pytest.raises(RuntimeError, match="empty probability map"):
        draw_label_picks(np.random.default_rng(0), background, None, 4)                         # None on an all-background region
    assert (draw_label_picks(np.random.default_rng(0), background, {0: 1.0}, 4)[0] == 0).all()


def test_parse_label_probabilities_accepts():
    assert parse_label_probabilities(None) is None
    assert parse_label_probabilities("") is None
    assert parse_label_probabilities("None") is None
    assert parse_label_probabilities({0: 0.2, 1: 0.8}) == {0: 0.2, 1: 0.8}
    assert parse_label_probabilities({"1": 1}) == {1: 1.0}
    assert parse_label_probabilities("0:0.2,1:0.8") == {0: 0.2, 1: 0.8}
    assert parse_label_probabilities(" 0:0 , 15:3 ") == {0: 0.0, 15: 3.0}
    assert parse_label_probabilities("1:1,") == {1: 1.0}                   # the trailing comma keeps a single pair a string in YAML


@pytest.mark.parametrize("value", ["0:-0.1,1:1", {1: -1.0}, "16:1.0", {-1: 1.0}, {0: 0.0, 1: 0}, "0:0,1:0", "0.5,1", "1:", "a:1", "1:nan",
                                   "1.5:1", 61, ",", ",1:1"])
def test_parse_label_probabilities_refuses(value):
    with pytest.raises(ValueError, match="label_probabilities"):
        parse_label_probabilities(value)


def test_queue_refusals_name_the_option(tmp_path):
    _write(tmp_path)
    args = (str(tmp_path / "x"), str(tmp_path / "y"), 8, 1, 2)
    with pytest.raises(mi355seg.Mi355SegError, match="sampler='label'.*no CPU fallback"):
        DevicePatchQueue(*args, "cpu", sampler="label")
    with pytest.raises(NotImplementedError, match="sampler='label' with aug=True"):
        DevicePatchQueue(*args, "cpu", sampler="label", aug=True)
    with pytest.raises(ValueError, match="sampler='weighted'"):
        DevicePatchQueue(*args, "cpu", sampler="weighted")
    with pytest.raises(ValueError, match="label_probabilities"):
        DevicePatchQueue(*args, "cpu", label_probabilities={0: 0.0})
    with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):
        mi355seg.functional.label_index(torch.zeros(1, 8, 8, 8), 4)


def test_make_loader_reads_sampler_and_label_probabilities(tmp_path, monkeypatch):
    _write(tmp_path)
    seen = {}

    class Spy(data.DevicePatchQueue):
        def __init__(self, *a, **k):
            seen.update(k)
            super().__init__(*a, **{**k, "sampler": "uniform"})

    monkeypatch.setattr(data, "DevicePatchQueue", Spy)
    cfg = Config(data_path=str(tmp_path / "x"), gt_path=str(tmp_path / "y"), patch_size=8, batch_size=1)
    data.make_loader(cfg, "cpu", 1)
    assert seen["sampler"] == "uniform" and seen["label_probabilities"] is None          # the getattr defaults
    cfg.sampler, cfg.label_probabilities = "label", "0:0.5,1:0.5"
    data.make_loader(cfg, "cpu", 1)
    assert seen["sampler"] == "label" and seen["label_probabilities"] == {0: 0.5, 1: 0.5}
    monkeypatch.undo()
    with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):                 # forwarded to the real queue
        data.make_loader(cfg, "cpu", 1)
    syn = Config(data_path="synthetic", patch_size=8, batch_size=1, sampler="label")
    with pytest.raises(ValueError, match="config.sampler=label"):
        data.make_loader(syn, "cpu", 1)
    syn.sampler = "uniform"
    assert isinstance(data.make_loader(syn, "cpu", 1), data.SyntheticPatches)


def test_command_line_form_reaches_the_loader_as_a_string():
    """the README's override: ``config.label_probabilities=0:0.5,1:0.5`` stays a string through the config parser"""
    from mi355seg.config import _parse_value
    assert parse_label_probabilities(_parse_value("0:0.5,1:0.5")) == {0: 0.5, 1: 0.5}
    assert _parse_value("label") == "label"
    assert _parse_value("1:1") == 61                                       # YAML 1.1 base 60: refused with a hint (see the refusals)
    assert parse_label_probabilities(_parse_value("1:1,")) == {1: 1.0} and parse_label_probabilities(_parse_value("{1: 1}")) == {1: 1.0}


def test_c_entry_points_refuse_bad_arguments_before_any_launch():
    """argument checks return an error code with mi355seg_last_error and touch neither the pointers nor a device"""
    L = mi355seg.lib()
    assert L.query("mi355seg_label_index_bytes", 256, 256, 256, 1, 1, 1) == (256 ** 3 // 1024) * 17 * 8       # ~2 MB for a 256^3 region
    assert L.query("mi355seg_label_index_bytes", 9, 10, 11, 4, 5, 6) == 17 * 8
    assert L.query("mi355seg_label_index_bytes", 9, 10, 11, 10, 5, 6) == 0
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data                                    # a non-null address that no refused call may read
    with pytest.raises(mi355seg.Mi355SegError, match="label_index_build: labels is null"):
        L.call("mi355seg_label_index_build_f32", None, 9, 10, 11, 4, 5, 6, p, 136, p, None)
    with pytest.raises(mi355seg.Mi355SegError, match="label_index_build: .*larger than the volume"):
        L.call("mi355seg_label_index_build_f32", p, 9, 10, 11, 4, 11, 6, p, 136, p, None)
    with pytest.raises(mi355seg.Mi355SegError, match=r"label_index_build: .*exceeds 2\^31"):
        L.call("mi355seg_label_index_build_f32", p, 2048, 1024, 1024, 4, 5, 6, p, 1 << 40, p, None)
    with pytest.raises(mi355seg.Mi355SegError, match="label_index_build: index_bytes too small"):
        L.call("mi355seg_label_index_build_f32", p, 9, 10, 11, 4, 5, 6, p, 135, p, None)
    with pytest.raises(mi355seg.Mi355SegError, match="label_index_select: index, picks or origins is null"):
        L.call("mi355seg_label_index_select", p, 9, 10, 11, 4, 5, 6, p, None, 1, p, None)
    with pytest.raises(mi355seg.Mi355SegError, match="label_index_select: n = 0 picks"):
        L.call("mi355seg_label_index_select", p, 9, 10, 11, 4, 5, 6, p, p, 0, p, None)


def test_uniform_sampler_is_the_queue_as_it_was(tmp_path):
    """sampler="uniform": the same batches, cache contents and rng consumption as a queue built without the argument"""
    _write(tmp_path)
    args = (str(tmp_path / "x"), str(tmp_path / "y"), (8, 8, 8), 2, 9, "cpu")
    kw = dict(seed=7, queue_length=6, samples_per_volume=3)
    qa, qb = DevicePatchQueue(*args, **kw), DevicePatchQueue(*args, sampler="uniform", label_probabilities=None, **kw)
    for a, b in zip(list(qa), list(qb)):
        assert torch.equal(a["source"]["data"], b["source"]["data"]) and torch.equal(a["gt"]["data"], b["gt"]["data"])
    assert sorted(qa.cache) == sorted(qb.cache) and qb.label_indices == {}
    assert qa.rng.random() == qb.rng.random()
