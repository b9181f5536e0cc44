"""Multi-class training and grading (config.multiclass), the parts that need no GPU: the key and its refusals, the
per-class metrics from the class counters, the per-class CSV writer, and the C-ABI of the label-form entry points (symbols,
prototypes, workspace sizes, refusals that never launch)."""
import csv
import ctypes

import numpy as np
import pytest
import torch

import mi355seg
from mi355seg._lib import HEADER, LIB_PATH, parse_header
from mi355seg.config import Config


# ----------------------------------------------------------------------------- config.multiclass
def _criterion(mode="dice_ce"):
    from mi355seg.train import parse_loss
    return parse_loss(Config({"loss": mode}))


def test_key_absent_or_false_changes_nothing():
    from mi355seg.train import parse_multiclass
    for cfg in ({}, {"multiclass": None}, {"multiclass": ""}, {"multiclass": False}, {"multiclass": "false"}):
        # (nothing else is looked at: out_classes = 1 and the BCE default are today's run)
        assert parse_multiclass(Config({"out_classes": 1, "data_path": "synthetic", **cfg}), None) is None


def test_key_true_gives_the_class_count():
    from mi355seg.train import parse_multiclass
    for K in (2, 4, 16):
        for v in (True, "true"):
            assert parse_multiclass(Config({"multiclass": v, "out_classes": K, "data_path": "/data"}), _criterion()) == K


def test_refusals_name_the_key():
    from mi355seg.train import parse_multiclass
    base = {"multiclass": True, "out_classes": 4, "data_path": "/data"}
    with pytest.raises(ValueError, match="config.multiclass needs a compound config.loss"):
        parse_multiclass(Config(base), None)                                   # the BCE default
    for K in (1, 17, 0, None, "4", True):
        with pytest.raises(ValueError, match="config.multiclass needs config.out_classes in 2..16"):
            parse_multiclass(Config({**base, "out_classes": K}), _criterion())
    with pytest.raises(ValueError, match="config.multiclass needs labelled volumes: data_path=synthetic"):
        parse_multiclass(Config({**base, "data_path": "synthetic"}), _criterion())
    with pytest.raises(ValueError, match="config.multiclass must be true or false"):
        parse_multiclass(Config({**base, "multiclass": "maybe"}), _criterion())


def test_predict_refuses_the_component_keys_and_synthetic_data():
    from mi355seg.predict import parse_predict_multiclass
    base = {"multiclass": True, "out_classes": 4, "pred_data_path": "/data"}
    assert parse_predict_multiclass(Config(base)) == 4                          # (no loss runs at predict time: no loss check)
    assert parse_predict_multiclass(Config({"out_classes": 4, "pred_data_path": "/data", "keep_largest": 1})) is None
    for kw in ({"keep_largest": 1}, {"min_component_voxels": 10}):
        with pytest.raises(ValueError, match="config.multiclass does not go with config.keep_largest / config.min_component_voxels"):
            parse_predict_multiclass(Config({**base, **kw}))
    with pytest.raises(ValueError, match="pred_data_path=synthetic"):
        parse_predict_multiclass(Config({**base, "pred_data_path": "synthetic"}))
    for K in (1, 17):
        with pytest.raises(ValueError, match="config.out_classes in 2..16"):
            parse_predict_multiclass(Config({**base, "out_classes": K}))


def test_train_step_refuses_a_criterion_without_the_label_tail():
    from mi355seg.engine import train_step
    opt = type("Opt", (), {"zero_grad": lambda self, set_to_none=True: None})()
    x = torch.zeros((1, 1, 4, 4, 4))
    with pytest.raises(ValueError, match="multiclass needs a criterion with a tail_labels method"):
        train_step(None, opt, x, x, criterion=None, multiclass=3)
    for K in (1, 17, True, 2.0):
        with pytest.raises(ValueError, match="multiclass must be the number of classes"):
            train_step(None, opt, x, x, criterion=_criterion(), multiclass=K)


# ----------------------------------------------------------------------------- class_metrics_from_counts
def _numpy_metrics(rows):
    r = np.asarray(rows, dtype=np.float64)
    tp, ps, gs = r[:, 0], r[:, 1], r[:, 2]
    return {"dice": 2 * tp / (gs + ps + 0.001), "jaccard": tp / (gs + ps - tp + 0.001), "precision": tp / (ps + 0.001), "recall": tp / (gs + 0.001)}


def _rows_of(conf):
    """(tp, pred, gt) per class of a confusion matrix conf[gt][pred]."""
    return [[int(conf[k, k]), int(conf[:, k].sum()), int(conf[k, :].sum())] for k in range(conf.shape[0])]


@pytest.mark.parametrize("K", [2, 3, 4, 9, 16])
def test_class_metrics_equal_numpy_fp64_on_random_confusion_matrices(K):
    from mi355seg.utils.metric import class_metrics_from_counts
    rng = np.random.default_rng(K)
    for trial in range(8):
        conf = rng.integers(0, 1 << 20, (K, K))
        if trial % 2 and K > 2:
            conf[K - 1, :] = 0; conf[:, K - 1] = 0                               # a class that neither occurs nor is predicted
        rows = _rows_of(conf)
        for given in (rows, torch.tensor(rows)):
            m = class_metrics_from_counts(given)
            want = _numpy_metrics(rows)
            for name in want:
                assert m[name] == want[name].tolist(), name                    # the same fp64 expressions: equal, not close
            present = [k for k in range(1, K) if rows[k][1] + rows[k][2] > 0]
            assert m["mean_dice"] == sum(float(want["dice"][k]) for k in present) / len(present)
            assert m["mean_jaccard"] == sum(float(want["jaccard"][k]) for k in present) / len(present)
            assert all(0.0 <= v <= 1.0 for name in want for v in m[name])
        if trial % 2 and K > 2:
            assert m["dice"][K - 1] == 0.0 and (K - 1) not in present


def test_class_metrics_all_absent_is_zero():
    from mi355seg.utils.metric import class_metrics_from_counts
    m = class_metrics_from_counts([[1000, 1000, 1000], [0, 0, 0], [0, 0, 0]])      # background only
    assert m["mean_dice"] == 0.0 and m["mean_jaccard"] == 0.0 and m["dice"][1:] == [0.0, 0.0]
    assert m["dice"][0] == 2000 / 2000.001
    with pytest.raises(ValueError):
        class_metrics_from_counts([[1, 2], [3, 4]])
    with pytest.raises(ValueError):
        class_metrics_from_counts([])


def test_two_classes_are_todays_binary_metric_number_for_number():
    from mi355seg.utils.metric import class_metrics_from_counts, metric_from_counts, rates_from_counts
    rng = np.random.default_rng(5)
    for trial in range(32):
        conf = rng.integers(0, 1 << 24, (2, 2)) if trial else np.array([[77, 0], [0, 0]])     # trial 0: no foreground at all
        gsum, psum, tp = int(conf[1, :].sum()), int(conf[:, 1].sum()), int(conf[1, 1])
        jac, dice = metric_from_counts([gsum, psum, tp, gsum + psum - tp])       # the four counters of the binary step
        m = class_metrics_from_counts(_rows_of(conf))
        assert m["mean_dice"] == dice and m["dice"][1] == dice
        assert m["mean_jaccard"] == jac and m["jaccard"][1] == jac
        assert (m["precision"][1], m["recall"][1]) == rates_from_counts([gsum, psum, 0, 0, tp, 0, 0, 0])


# ----------------------------------------------------------------------------- the per-class CSV
def test_class_csv_columns_order_and_mean_rows(tmp_path):
    from mi355seg.predict import write_class_metrics_csv
    rows = [{"file": f, "class": k, "jaccard": 0.1 * k + i, "dice": 0.2 * k + i} for i, f in enumerate(("a", "b", "c")) for k in (1, 2, 3)]
    path = tmp_path / "metrics.csv"
    write_class_metrics_csv(path, rows)
    got = list(csv.reader(open(path)))
    assert got[0] == ["file", "class", "jaccard", "dice"]
    assert [(r[0], r[1]) for r in got[1:10]] == [(f, str(k)) for f in ("a", "b", "c") for k in (1, 2, 3)]
    assert [(r[0], r[1]) for r in got[10:]] == [("mean", "1"), ("mean", "2"), ("mean", "3")]
    for r in got[10:]:
        k = int(r[1])
        assert float(r[2]) == float(np.mean([0.1 * k + i for i in range(3)])) and float(r[3]) == float(np.mean([0.2 * k + i for i in range(3)]))
    full = [{**r, "precision": 0.5, "recall": 0.25, "hs95": 2.0 + r["class"]} for r in rows]
    write_class_metrics_csv(path, full)
    got = list(csv.reader(open(path)))
    assert got[0] == ["file", "class", "precision", "recall", "jaccard", "dice", "hs95"]
    assert len(got) == 1 + 9 + 3 and got[-1][:2] == ["mean", "3"] and float(got[-1][6]) == 5.0 and float(got[-3][2]) == 0.5


# ----------------------------------------------------------------------------- C-ABI
NAMES = ("mi355seg_labels_u8_f32", "mi355seg_onehot_u8_f32", "mi355seg_loss_tail_lab_ws_bytes", "mi355seg_loss_tail_fwd_lab_f32",
         "mi355seg_loss_tail_bwd_lab_f32", "mi355seg_class_counts_ws_bytes", "mi355seg_class_counts_i64")


def test_abi_symbols_are_declared_and_exported():
    protos = parse_header(HEADER)
    cdll = ctypes.CDLL(LIB_PATH)
    for n in NAMES:
        assert n in protos and hasattr(cdll, n), n
    names = lambda n: [a for _, a in protos[n][1]]
    types = lambda n: dict((a, t) for t, a in protos[n][1])
    assert names(NAMES[0]) == ["gt", "n", "K", "labels_u8", "bad", "stream"]
    assert types(NAMES[0])["labels_u8"] == "uint8_t*" and types(NAMES[0])["bad"] == "int64_t*"
    assert names(NAMES[1]) == ["labels_u8", "N", "K", "S", "out", "stream"]
    one_hot = protos["mi355seg_loss_tail_fwd_f32"][1]
    lab = protos[NAMES[3]][1]
    # the one-hot forward with the labels in the target's place and class_counts after coef
    assert [a for _, a in lab] == [{"target": "labels"}.get(a, a) for _, a in one_hot[:18]] + ["class_counts", "ws", "ws_bytes", "stream"]
    assert types(NAMES[3])["labels"] == "const uint8_t*" and types(NAMES[3])["class_counts"] == "int64_t*"
    assert [(t, a) for t, a in protos[NAMES[4]][1] if a != "labels"] == [(t, a) for t, a in protos["mi355seg_loss_tail_bwd_f32"][1] if a != "target"]
    assert names(NAMES[6]) == ["gt_labels", "pred_labels", "n", "K", "out", "ws", "ws_bytes", "stream"]
    for n in ("labels_u8", "one_hot_labels", "loss_tail_labels", "class_counts"):
        assert callable(getattr(mi355seg.functional, n)), n


def test_workspace_sizes():
    L = mi355seg.lib()
    q = lambda *a: L.query("mi355seg_loss_tail_lab_ws_bytes", *a)
    for bad in ((0, 2, 8), (2, 0, 8), (2, 17, 8), (2, 2, 0), (-1, 2, 8)):
        assert q(*bad) == 0, bad
    assert q(1, 2, 1) == (1 + 5 * 2 + 4 + 3 * 2) * 8                            # the one-hot form's table plus 3 K class counters
    assert q(2, 16, 128 ** 3) == 2048 * (1 + 5 * 16 + 4 + 3 * 16) * 8
    for N, K, S in ((1, 3, 257), (2, 4, 8 * 12 * 16)):
        assert q(N, K, S) == L.query("mi355seg_loss_tail_ws_bytes", N, K, S) // ((1 + 5 * K + 4) * 8) * (1 + 5 * K + 4 + 3 * K) * 8
    c = lambda *a: L.query("mi355seg_class_counts_ws_bytes", *a)
    assert c(0, 2) == 0 and c(8, 0) == 0 and c(8, 17) == 0
    assert c(1, 2) == 6 * 8 and c(257, 4) == 2 * 12 * 8 and c(1 << 30, 16) == 2048 * 48 * 8


def test_bad_arguments_return_error_codes_and_never_launch():
    """Every refusal of the new entry points, with host addresses or null pointers in place of the tensors: a call that got past its
    argument checks would fault, not raise."""
    L = mi355seg.lib()
    E = mi355seg.Mi355SegError
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    assert a % 8 == 0
    a16 = a + (-a) % 16

    def fwd(K=2, voxel=1, region=1, gamma=2.0, alpha=0.3, beta=0.7, wv=1.0, wr=1.0, ws=a, ws_bytes=1 << 20, N=1, S=8, logits=a16, labels=a16, null=None):
        nulls = {null: True}
        p = {n: (None if nulls.get(n) else a) for n in ("loss", "terms", "sums", "mask", "counts", "coef", "class_counts")}
        L.call("mi355seg_loss_tail_fwd_lab_f32", None if nulls.get("logits") else logits, None if nulls.get("labels") else labels, N, K, S,
               voxel, region, gamma, alpha, beta, wv, wr, p["loss"], p["terms"], p["sums"], p["mask"], p["counts"], p["coef"],
               p["class_counts"], ws, ws_bytes, None)

    def bwd(K=2, voxel=1, region=1, gamma=2.0, N=1, S=8, logits=a16, labels=a16, dlogits=a16, null=None):
        nulls = {null: True}
        p = {n: (None if nulls.get(n) else a) for n in ("coef", "gscale")}
        L.call("mi355seg_loss_tail_bwd_lab_f32", None if nulls.get("logits") else logits, None if nulls.get("labels") else labels,
               p["coef"], p["gscale"], N, K, S, voxel, region, gamma, None if nulls.get("dlogits") else dlogits, None)

    for call, name in ((fwd, "loss_tail_fwd_lab"), (bwd, "loss_tail_bwd_lab")):
        for K in (0, 17, -3):
            with pytest.raises(E, match=f"{name}: K must be in 1..16, got {K}"):
                call(K=K)
        for voxel in (-1, 4):
            with pytest.raises(E, match=f"{name}: unknown voxel term {voxel}"):
                call(voxel=voxel)
        for region in (-1, 3):
            with pytest.raises(E, match=f"{name}: unknown region term {region}"):
                call(region=region)
        with pytest.raises(E, match=f"{name}: both terms absent"):
            call(voxel=0, region=0)
        with pytest.raises(E, match=f"{name}: the ce term needs K >= 2"):
            call(K=1, voxel=3)
        for gamma in (0.5, -1.0, 8.5, float("nan")):
            with pytest.raises(E, match=f"{name}: gamma must be 0 or in"):
                call(voxel=2, gamma=gamma)
        for kw in ({"N": 0}, {"S": 0}, {"S": -4}):
            with pytest.raises(E, match=f"{name}: bad extents"):
                call(**kw)
        # where the 16-byte path would be taken (S % 4 == 0, K <= 4) a misaligned pointer is refused
        for kw in ({"logits": a16 + 4}, {"labels": a16 + 1}, {"labels": a16 + 2}):
            with pytest.raises(E, match=f"{name}: with S % 4 == 0 and K <= 4"):
                call(**kw)
    with pytest.raises(E, match="loss_tail_bwd_lab: with S % 4 == 0 and K <= 4"):
        bwd(dlogits=a16 + 8)
    for kw in ({"alpha": -0.1}, {"beta": -1.0}, {"alpha": float("nan")}):
        with pytest.raises(E, match="alpha and beta must be >= 0"):
            fwd(region=2, **kw)
    with pytest.raises(E, match="alpha \\+ beta > 0"):
        fwd(region=2, alpha=0.0, beta=0.0)
    for kw in ({"wv": -1.0}, {"wr": -0.5}, {"wr": float("nan")}):
        with pytest.raises(E, match="weights must be >= 0"):
            fwd(**kw)
    for n in ("logits", "labels", "loss", "terms", "sums", "mask", "counts", "coef", "class_counts"):
        with pytest.raises(E, match="loss_tail_fwd_lab: null pointer"):
            fwd(null=n)
    with pytest.raises(E, match="loss_tail_fwd_lab: null pointer"):
        fwd(ws=None)
    for n in ("logits", "labels", "coef", "gscale", "dlogits"):
        with pytest.raises(E, match="loss_tail_bwd_lab: null pointer"):
            bwd(null=n)
    need = L.query("mi355seg_loss_tail_lab_ws_bytes", 1, 2, 8)
    for have in (0, need - 1, L.query("mi355seg_loss_tail_ws_bytes", 1, 2, 8)):          # (the one-hot form's size is too small)
        with pytest.raises(E, match=f"workspace too small: need {need} bytes, have {have}"):
            fwd(ws_bytes=have)
    with pytest.raises(E, match="workspace must be 8-byte aligned"):
        fwd(ws=a + 4)

    for K in (0, 17):
        with pytest.raises(E, match=f"labels_u8: K must be in 1..16, got {K}"):
            L.call("mi355seg_labels_u8_f32", a, 8, K, a, a, None)
        with pytest.raises(E, match=f"onehot_u8: K must be in 1..16, got {K}"):
            L.call("mi355seg_onehot_u8_f32", a, 1, K, 8, a, None)
        with pytest.raises(E, match=f"class_counts: K must be in 1..16, got {K}"):
            L.call("mi355seg_class_counts_i64", a, a, 8, K, a, a, 1 << 20, None)
    for args in ((None, 8, 2, a, a), (a, 8, 2, None, a), (a, 8, 2, a, None)):
        with pytest.raises(E, match="labels_u8: null pointer"):
            L.call("mi355seg_labels_u8_f32", *args, None)
    with pytest.raises(E, match="labels_u8: bad extent"):
        L.call("mi355seg_labels_u8_f32", a, 0, 2, a, a, None)
    with pytest.raises(E, match="labels_u8: the counter must be 8-byte aligned"):
        L.call("mi355seg_labels_u8_f32", a, 8, 2, a, a + 4, None)
    for args in ((None, 1, 2, 8, a), (a, 1, 2, 8, None)):
        with pytest.raises(E, match="onehot_u8: null pointer"):
            L.call("mi355seg_onehot_u8_f32", *args, None)
    for N, S in ((0, 8), (1, 0)):
        with pytest.raises(E, match="onehot_u8: bad extents"):
            L.call("mi355seg_onehot_u8_f32", a, N, 2, S, a, None)
    for args in ((None, a, 8, 2, a, a), (a, None, 8, 2, a, a), (a, a, 8, 2, None, a), (a, a, 8, 2, a, None)):
        with pytest.raises(E, match="class_counts: null pointer"):
            L.call("mi355seg_class_counts_i64", *args, 1 << 20, None)
    with pytest.raises(E, match="class_counts: bad extent"):
        L.call("mi355seg_class_counts_i64", a, a, 0, 2, a, a, 1 << 20, None)
    need = L.query("mi355seg_class_counts_ws_bytes", 8, 2)
    with pytest.raises(E, match=f"workspace too small: need {need} bytes, have {need - 1}"):
        L.call("mi355seg_class_counts_i64", a, a, 8, 2, a, a, need - 1, None)
    with pytest.raises(E, match="class_counts: the workspace must be 8-byte aligned"):
        L.call("mi355seg_class_counts_i64", a, a, 8, 2, a, a + 4, 1 << 20, None)


def test_functional_refuses_cpu_tensors_and_bad_arguments():
    F = mi355seg.functional
    E = mi355seg.Mi355SegError
    spec = F.LossSpec.from_mode("dice_ce")
    with pytest.raises(E, match="no CPU fallback"):
        F.labels_u8(torch.zeros((1, 1, 4, 4, 4)), 3)
    with pytest.raises(E, match="no CPU fallback"):
        F.one_hot_labels(torch.zeros((1, 4, 4, 4), dtype=torch.uint8), 3)
    with pytest.raises(E, match="no CPU fallback"):
        F.loss_tail_labels(torch.zeros((1, 3, 4, 4, 4)), torch.zeros((1, 4, 4, 4), dtype=torch.uint8), spec)
    with pytest.raises(E, match="no CPU fallback"):
        F.class_counts(torch.zeros(8, dtype=torch.int64), torch.zeros(8, dtype=torch.int64), 3)
    with pytest.raises(TypeError, match="LossSpec"):
        F.loss_tail_labels(torch.zeros((1, 3, 4, 4, 4)), torch.zeros((1, 4, 4, 4), dtype=torch.uint8), "dice_ce")


def test_compound_loss_has_the_label_tail():
    from mi355seg.utils.loss_function import CompoundLoss
    assert callable(CompoundLoss("dice_ce").tail_labels)
