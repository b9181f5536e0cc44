"""tests/golden/hd95.npz (made by tests/golden/make_hd95.py from the reference's own ``metric(gt, pred, spacing)`` with a scipy
stand-in for monai's ``compute_hausdorff_distance``) against a brute-force comparator written here, and the CSV writer of
predict.py.  CPU only, no scipy.

The comparator: edge voxels by the six-neighbour definition, all pairwise distances between the two coordinate sets scaled by the
spacing (fp64, no matmul form), row and column minima, ``np.percentile``, the larger of the two."""
import csv

import numpy as np
import torch
from conftest import load_golden

from oracle.metric import rates

COLUMNS = ["precision", "recall", "jaccard", "dice", "hs95"]


def hd95_cases():
    """[(name, gt, pred, spacing, as_float, out[5])] with uint8 masks [D, H, W]."""
    g = load_golden("hd95")
    cases = []
    for name in [str(n) for n in g["names"]]:
        shape = tuple(int(v) for v in g[name + "/shape"])
        n = int(np.prod(shape))
        gt = np.unpackbits(g[name + "/gt_bits"])[:n].reshape(shape)
        pred = np.unpackbits(g[name + "/pred_bits"])[:n].reshape(shape)
        cases.append((name, gt, pred, tuple(float(v) for v in g[name + "/spacing"]), bool(g[name + "/as_float"]), g[name + "/out"]))
    return cases


def edges6(mask):
    """bool torch tensor [D, H, W]: foreground voxels with a background face neighbour; outside the array is background."""
    m = torch.as_tensor(np.asarray(mask) != 0)
    p = torch.nn.functional.pad(m, (1, 1, 1, 1, 1, 1), value=False)
    inner = (p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])
    return m & ~inner


def nearest_site_distance(points, sites):
    """fp64 [len(points)]: distance from each point to the nearest of ``sites`` (both [n, 3], already in millimetres).  At most 2^22
    pairs per cdist call: 32 MiB of distances, and on the device one workgroup per pair stays far inside the launch limits."""
    chunk = max(1, (1 << 22) // max(1, len(sites)))
    out = torch.empty(len(points), dtype=torch.float64, device=points.device)
    for i in range(0, len(points), chunk):
        out[i:i + chunk] = torch.cdist(points[i:i + chunk], sites, compute_mode="donot_use_mm_for_euclid_dist").min(1).values
    return out


def brute_hd95(gt, pred, spacing, percentile=95.0):
    sp = torch.tensor(spacing, dtype=torch.float64)
    a = torch.nonzero(edges6(gt)).double() * sp
    b = torch.nonzero(edges6(pred)).double() * sp
    if len(a) == 0 or len(b) == 0:
        return float("nan")
    return max(np.percentile(nearest_site_distance(a, b).numpy(), percentile), np.percentile(nearest_site_distance(b, a).numpy(), percentile))


def close(value, expected, rel):
    """|value - expected| <= rel * |expected|; against an expected 0 (identical masks) an absolute 1e-12."""
    return abs(value - expected) <= (rel * abs(expected) if expected != 0 else 1e-12)


def test_fixture_file_is_small_and_holds_every_case():
    names = [c[0] for c in hd95_cases()]
    assert len(names) >= 12 and {"boxes", "voxels", "border", "identical", "plates", "blobs48", "float01", "empty_gt", "empty_pred",
                                 "empty_both"} <= set(names)
    assert sum(n.startswith("blob40") for n in names) == 3


def test_recorded_hd95_equals_brute_force():
    for name, gt, pred, sp, _, out in hd95_cases():
        bf = brute_hd95(gt, pred, sp)
        if name.startswith("empty"):
            assert not np.isfinite(out[4]) and not np.isfinite(bf), name
            continue
        print(f"{name}: recorded {out[4]!r} brute force {bf!r}")
        assert close(float(out[4]), float(bf), 1e-12), (name, out[4], bf)


def test_recorded_rates_equal_the_oracle_and_the_call_is_the_references():
    g = load_golden("hd95")
    for name, gt, pred, sp, _, out in hd95_cases():
        r = rates(gt, pred)
        assert out[0] == r["precision"] and out[1] == r["recall"], name
        assert float(g[name + "/call_percentile"]) == 95.0
        assert tuple(g[name + "/call_spacing"]) == sp
    assert float(g["large/out"][4]) > 0 and int(g["large/edge_counts"].min()) > 100_000


def _read(path):
    with open(path, newline="") as fh:
        return list(csv.reader(fh))


def test_metrics_csv_without_spacing_is_file_jaccard_dice(tmp_path):
    from mi355seg.predict import write_metrics_csv
    rows = [{"file": "a", "jaccard": 0.5, "dice": 0.75}, {"file": "b", "jaccard": 0.25, "dice": 0.5}]
    write_metrics_csv(str(tmp_path / "m.csv"), rows)
    assert (tmp_path / "m.csv").read_text().splitlines()[0] == "file,jaccard,dice"
    got = _read(tmp_path / "m.csv")
    assert got == [["file", "jaccard", "dice"], ["a", "0.5", "0.75"], ["b", "0.25", "0.5"]]      # no mean row


def test_metrics_csv_with_spacing_has_six_columns_and_a_mean_row(tmp_path):
    from mi355seg.predict import write_metrics_csv
    rows = [{"file": "a", "precision": 0.5, "recall": 1.0, "jaccard": 0.5, "dice": 0.75, "hs95": 2.0},
            {"file": "b", "precision": 0.25, "recall": 0.5, "jaccard": 0.25, "dice": 0.5, "hs95": 5.0}]
    write_metrics_csv(str(tmp_path / "m.csv"), rows)
    got = _read(tmp_path / "m.csv")
    assert got[0] == ["file"] + COLUMNS and len(got) == 4
    assert got[1] == ["a", "0.5", "1.0", "0.5", "0.75", "2.0"]
    assert got[3][0] == "mean" and [float(v) for v in got[3][1:]] == [0.375, 0.75, 0.375, 0.625, 3.5]


def test_spacing_key_is_optional_and_absent_means_off():
    from mi355seg.config import Config
    from mi355seg.predict import parse_spacing
    assert parse_spacing(Config()) is None and parse_spacing(Config(spacing=None)) is None
    assert parse_spacing(Config(spacing="1,1,2")) == (1.0, 1.0, 2.0)
    assert parse_spacing(Config(spacing=[1.5, 0.8, 0.6])) == (1.5, 0.8, 0.6)
