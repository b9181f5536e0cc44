"""Soft sliding-window aggregation on the device (csrc/aggregate.hip; predict.py overlap_mode = average | hann | gaussian) against
torchio's add_batch loop written out in numpy fp64: ``acc[dst] += w3 * softmax(logits)``, ``ws[dst] += w3``, ``prob = acc / ws`` over
grid_locations, patches in torchio's order.

Tolerances (set by the arithmetic, not by what the kernels give).  A probability is a sum of n <= 27 terms w * p / ws; in fp32 each
term carries the softmax (K <= 16 additions, one exp, one divide), the weight products and the fmaf, about (K + n + 12) * 2^-24
<= 3.3e-6 in all, and a fast exp adds at most eps / e absolute per term.  PROB_TOL = 1e-5 is three times that bound; a larger
measured value is a bug.  Labels must equal the fp64 argmax wherever the fp64 top-two margin is at least MARGIN = 2e-5 (twice the
tolerance: both probabilities may move by it), and such a comparison may leave out at most 1 % of a case's voxels.
Measured on an MI355X (DESIGN.md section 4.15 has the table; every test prints its figures): max |prob - fp64| 4.6e-7 over all
grids and modes, 2.1e-7 through the model, 2.8e-7 at logits of +-1e4; at most 0.160 % of a case's voxels left out; no wrong label."""
import csv
import os

import numpy as np
import pytest
import torch

from oracle.fill import fill_module_, make_input
from test_aggregate_host import GRIDS, SOFT_MODES

pytestmark = pytest.mark.gpu

PROB_TOL = 1e-5
MARGIN = 2e-5
MAX_LEFT_OUT = 0.01

# beside the five grids: shapes that reach the kernel's other instantiations (more than 4 classes: 16 register slots per voxel) and
# the 128-bit kernel with a patch origin that is no multiple of 4 (x origins 0, 10, 20, 28: it then works voxel by voxel)
EXTRA_GRIDS = [
    ((16, 20, 44), (16, 16, 16), (8, 8, 6), 3),
    ((16, 20, 44), (16, 16, 16), (8, 8, 6), 5),
    ((12, 12, 21), (8, 8, 10), (4, 4, 4), 6),
    ((16, 16, 40), (8, 8, 16), (4, 4, 8), 16),
]
ALL_GRIDS = GRIDS + EXTRA_GRIDS


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mi355seg
    mi355seg.lib()
    return mi355seg


def softmax64(logits):
    l = np.asarray(logits, dtype=np.float64)
    e = np.exp(l - l.max(axis=-4, keepdims=True))
    return e / e.sum(axis=-4, keepdims=True)


def reference(size, patch, overlap, mode, logits):
    """torchio's GridAggregator in fp64: logits [P, K, pd, ph, pw] of the grid's patches, in order -> prob [K, D, H, W]"""
    from mi355seg.predict import grid_locations, window_weights
    wz, wy, wx = window_weights(mode, patch)
    w3 = wz[:, None, None] * wy[None, :, None] * wx[None, None, :]
    acc = np.zeros((logits.shape[1],) + tuple(size), dtype=np.float64)
    ws = np.zeros(size, dtype=np.float64)
    locs = grid_locations(size, patch, overlap)
    assert len(locs) == logits.shape[0]
    for p, (z, y, x) in enumerate(locs):
        dst = (slice(z, z + patch[0]), slice(y, y + patch[1]), slice(x, x + patch[2]))
        acc[(slice(None),) + dst] += w3 * softmax64(logits[p])
        ws[dst] += w3
    return acc / ws


def run_device(seg, size, patch, overlap, mode, logits, batch):
    """the two entry points over the grid in batches of ``batch`` -> (acc, labels [D, H, W], prob), device tensors"""
    from mi355seg.predict import axis_weight_sums, window_table, window_weights
    F = seg.functional
    table = torch.from_numpy(window_table(size, patch, overlap)).cuda()
    w = window_weights(mode, patch)
    sums = axis_weight_sums(size, patch, overlap, w)
    lg = logits if torch.is_tensor(logits) else torch.tensor(logits).cuda()
    P, K = lg.shape[:2]
    assert P == table.shape[0]
    acc = torch.zeros((K,) + tuple(size), dtype=torch.float32, device="cuda")
    for i in range(0, P, batch):
        F.aggregate_patches(acc, lg[i:i + batch], table, i, w)
    labels, prob = F.aggregate_finalize(acc, sums, probabilities=True)
    only = F.aggregate_finalize(acc, sums)
    assert labels.shape == (1,) + tuple(size) and labels.dtype == torch.int64 and torch.equal(only, labels)
    return acc, labels[0], prob


def grade(tag, labels, prob, ref, cap=MAX_LEFT_OUT):
    """the module docstring's two rules; prints the figures before it asserts.  cap=None: no limit on the voxels left out (inputs
    made of saturated probabilities, whose blends tie exactly)"""
    prob, labels = prob.cpu().numpy().astype(np.float64), labels.cpu().numpy()
    err = float(np.abs(prob - ref).max())
    top = np.sort(ref, axis=0)
    decisive = top[-1] - top[-2] >= MARGIN
    left_out = 1.0 - float(decisive.mean())
    wrong = int((labels != ref.argmax(axis=0))[decisive].sum())
    print(f"{tag}: max|prob - fp64| = {err:.3e}, voxels left out of the label comparison {100 * left_out:.3f} %, wrong labels {wrong}")
    assert np.isfinite(prob).all()
    assert err <= PROB_TOL
    assert cap is None or left_out <= cap
    assert wrong == 0
    return err


_CASES = {}


def case(grid, mode):
    """(logits float32 [P, K, pd, ph, pw], fp64 reference prob) of one grid and mode: computed once, shared, never written to.
    The logits are 4 * standard_normal drawn independently per patch, so that overlapping patches disagree."""
    from mi355seg.predict import grid_locations
    size, patch, overlap, K = ALL_GRIDS[grid]
    if ("logits", grid) not in _CASES:
        P = len(grid_locations(size, patch, overlap))
        lg = (4.0 * np.random.default_rng(1000 + grid).standard_normal((P, K) + tuple(patch))).astype(np.float32)
        lg.setflags(write=False)
        _CASES["logits", grid] = lg
    lg = _CASES["logits", grid]
    if (grid, mode) not in _CASES:
        ref = reference(size, patch, overlap, mode, lg)
        ref.setflags(write=False)
        _CASES[grid, mode] = ref
    return lg, _CASES[grid, mode]


# ------------------------------------------------------------------------------------------------ 1. kernels against the reference
@pytest.mark.parametrize("mode", SOFT_MODES)
@pytest.mark.parametrize("grid", range(len(ALL_GRIDS)))
def test_kernels_against_the_fp64_aggregator(seg, grid, mode):
    size, patch, overlap, K = ALL_GRIDS[grid]
    lg, ref = case(grid, mode)
    acc, labels, prob = run_device(seg, size, patch, overlap, mode, lg, batch=3)
    grade(f"grid {grid} {size} / {patch} / {overlap} K={K} {mode}", labels, prob, ref)
    assert float((prob.sum(0) - 1).abs().max()) <= PROB_TOL


# ------------------------------------------------------------------------------------------------ 2. batch size, reproducibility
@pytest.mark.parametrize("mode", SOFT_MODES)
@pytest.mark.parametrize("grid", [0, 3, 5])
def test_result_is_bitwise_independent_of_the_batch_size_and_reproducible(seg, grid, mode):
    size, patch, overlap, K = ALL_GRIDS[grid]
    lg, _ = case(grid, mode)
    dev = torch.tensor(lg).cuda()
    P = dev.shape[0]
    runs = [run_device(seg, size, patch, overlap, mode, dev, batch=b) for b in (1, 3, P, 3)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 3. extreme logits
@pytest.mark.parametrize("mode", SOFT_MODES)
@pytest.mark.parametrize("scale", [80.0, 1e4])
@pytest.mark.parametrize("grid", [4, 1])
def test_extreme_logits_stay_finite_and_equal_logits_give_one_over_k(seg, grid, scale, mode):
    from mi355seg.predict import grid_locations
    size, patch, overlap, K = GRIDS[grid]
    locs = grid_locations(size, patch, overlap)
    rng = np.random.default_rng(7)
    lg = (scale * rng.choice([-1.0, 1.0], size=(len(locs), K) + tuple(patch))).astype(np.float32)
    lg[0] = scale                                     # one patch's worth of all-equal logits
    lg[-1] = -scale
    ref = reference(size, patch, overlap, mode, lg)
    acc, labels, prob = run_device(seg, size, patch, overlap, mode, lg, batch=2)
    assert torch.isfinite(acc).all()
    grade(f"grid {grid} logits +-{scale:g} {mode}", labels, prob, ref, cap=None)
    # the corner that only patch 0 covers: every other patch starts at or beyond the second origin of some axis
    origins = [sorted({l[a] for l in locs}) for a in range(3)]
    corner = tuple(slice(0, o[1] if len(o) > 1 else n) for o, n in zip(origins, size))
    assert float((prob[(slice(None),) + corner] - 1.0 / K).abs().max()) <= PROB_TOL
    assert int(labels[corner].abs().max()) == 0


@pytest.mark.parametrize("K", [2, 3, 16])
def test_one_patch_of_equal_logits(seg, K):
    size = patch = (32, 32, 32)
    lg = np.full((1, K) + patch, -1e4, dtype=np.float32)
    for mode in SOFT_MODES:
        acc, labels, prob = run_device(seg, size, patch, (4, 4, 4), mode, lg, batch=1)
        assert float((prob - 1.0 / K).abs().max()) <= PROB_TOL and int(labels.abs().max()) == 0


# ------------------------------------------------------------------------------------------------ 4. no overlap: the crop labels
@pytest.mark.parametrize("size,patch,K", [((32, 32, 48), (16, 16, 16), 3), ((16, 24, 27), (8, 12, 9), 2)])
def test_without_overlap_every_mode_gives_the_crop_labels(seg, size, patch, K):
    from mi355seg.predict import grid_locations, window_table
    F = seg.functional
    overlap = (0, 0, 0)
    locs = grid_locations(size, patch, overlap)
    lg = (4.0 * np.random.default_rng(11).standard_normal((len(locs), K) + tuple(patch))).astype(np.float32)
    first = lg.argmax(axis=1)
    np.put_along_axis(lg, first[:, None], np.take_along_axis(lg, first[:, None], axis=1) + np.float32(0.1), axis=1)   # top-two gap >= 0.1
    top = np.sort(lg, axis=1)
    assert float((top[:, -1] - top[:, -2]).min()) >= 0.1 - 1e-6
    dev = torch.from_numpy(lg).cuda()
    table = torch.from_numpy(window_table(size, patch, overlap)).cuda()
    crop = torch.full(size, -1, dtype=torch.int64, device="cuda")
    patch_labels = F.argmax_channels(dev)
    seg.lib().call("mi355seg_paste_labels_i64", patch_labels.data_ptr(), table.data_ptr(), 0, len(locs), *patch, crop.data_ptr(), *size,
                   torch.cuda.current_stream().cuda_stream)
    want = np.full(size, -1, dtype=np.int64)
    for p, (z, y, x) in enumerate(locs):
        want[z:z + patch[0], y:y + patch[1], x:x + patch[2]] = first[p]
    assert np.array_equal(crop.cpu().numpy(), want)
    for mode in SOFT_MODES:
        acc, labels, prob = run_device(seg, size, patch, overlap, mode, dev, batch=4)
        assert torch.equal(labels, crop), mode
        dev1 = float((prob.sum(0) - 1).abs().max())
        print(f"{size} {mode}: max|sum_k prob - 1| = {dev1:.3e}")
        assert dev1 <= PROB_TOL


# ------------------------------------------------------------------------------------------------ 5. / 6. through a model
@pytest.fixture(scope="module")
def unet(seg):
    from mi355seg.models.three_d.unet3d import UNet3D
    return fill_module_(UNet3D(1, 2, 8)).cuda().eval()


def test_crop_mode_is_the_call_without_the_keyword(seg, unet):
    from mi355seg.predict import sliding_window_predict
    size, ps, ov = (40, 48, 72), (32, 32, 32), (4, 4, 12)
    vol = make_input((1,) + size, freq=0.017).cuda()
    a = sliding_window_predict(unet, vol, ps, ov, batch_size=3)
    b = sliding_window_predict(unet, vol, ps, ov, batch_size=3, overlap_mode="crop")
    c = sliding_window_predict(unet, vol, ps, ov, batch_size=3, overlap_mode="crop", return_probabilities=False)
    assert a.dtype == torch.int64 and a.shape == (1,) + size and torch.equal(a, b) and torch.equal(a, c)
    assert not unet.training


def test_hann_blend_through_a_model_against_the_reference_fed_with_the_device_logits(seg, unet):
    from mi355seg.predict import sliding_window_predict, window_table
    size, ps, ov, bs = (40, 48, 72), (32, 32, 32), (16, 16, 16), 3
    vol = make_input((1,) + size, freq=0.017).cuda()
    labels, prob = sliding_window_predict(unet, vol, ps, ov, batch_size=bs, overlap_mode="hann", return_probabilities=True)
    assert labels.shape == (1,) + size and labels.dtype == torch.int64 and prob.shape == (2,) + size and prob.dtype == torch.float32
    assert torch.equal(sliding_window_predict(unet, vol, ps, ov, batch_size=bs, overlap_mode="hann"), labels)
    # the device's own logits of every patch: the same gather and the same batches
    table_h = window_table(size, ps, ov)
    table = torch.from_numpy(table_h).cuda()
    P = table_h.shape[0]
    logits = []
    with torch.no_grad():
        for i in range(0, P, bs):
            nb = min(bs, P - i)
            x = torch.empty((nb, 1) + ps, dtype=torch.float32, device="cuda")
            seg.lib().call("mi355seg_gather_patches_f32", vol.data_ptr(), 1, *size, table.data_ptr(), i, nb, *ps, x.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
            logits.append(unet(x).float().cpu().numpy())
    ref = reference(size, ps, ov, "hann", np.concatenate(logits))
    grade("UNet3D(1,2,8) (40,48,72) hann overlap 16", labels[0], prob, ref)


# ------------------------------------------------------------------------------------------------ 7. command line
def test_predict_cli_blends_and_saves_probabilities_and_is_unchanged_without_the_keys(seg, tmp_path):
    from mi355seg.config import compose, parse_patch_size
    from mi355seg.predict import main as predict_main
    from mi355seg.registry import build_model
    import mi355seg.predict as P
    conf_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(P.__file__))), "conf")
    common = ["config=unet", f"config.output_dir={tmp_path / 'logs'}", "config.patch_size=32,32,32", "config.batch_size=2"]
    cfg = compose(conf_dir, common, job_name="predict")
    parse_patch_size(cfg)
    torch.manual_seed(3)
    ckpt = str(tmp_path / "model.pt")
    torch.save({"model": build_model(cfg).state_dict()}, ckpt)
    common.append(f"config.ckpt={ckpt}")

    def run(name, *keys):
        cfg, rows = predict_main(common + [f"config.hydra_path={tmp_path / name}"] + list(keys))
        return cfg.hydra_path, rows

    plain, rows_plain = run("plain")
    named, rows_named = run("named", "config.overlap_mode=crop", "config.patch_overlap=4,4,30", "config.save_probabilities=false")
    soft, rows_soft = run("soft", "config.overlap_mode=hann", "config.patch_overlap=8", "config.save_probabilities=true")
    files = ["metrics.csv"] + [r["file"] + "_pred.npy" for r in rows_plain]
    assert len(rows_plain) == 2 and sorted(os.listdir(plain)) == sorted(files) == sorted(os.listdir(named))
    for f in files:                                   # the keys at their defaults: the same bytes
        with open(os.path.join(plain, f), "rb") as a, open(os.path.join(named, f), "rb") as b:
            assert a.read() == b.read(), f
    assert sorted(os.listdir(soft)) == sorted(files + [r["file"] + "_prob.npy" for r in rows_soft])
    with open(os.path.join(soft, "metrics.csv"), newline="") as fh:
        table = list(csv.reader(fh))
    assert table[0] == ["file", "jaccard", "dice"] and [r[0] for r in table[1:]] == [r["file"] for r in rows_soft]
    for r in rows_soft:
        mask = np.load(os.path.join(soft, r["file"] + "_pred.npy"))
        prob = np.load(os.path.join(soft, r["file"] + "_prob.npy"))
        assert mask.shape == (1, 64, 64, 64) and mask.dtype == np.uint8 and set(np.unique(mask)) <= {0, 1}
        assert prob.shape == (2, 64, 64, 64) and prob.dtype == np.float32 and np.isfinite(prob).all()
        assert float(np.abs(prob.astype(np.float64).sum(0) - 1).max()) <= PROB_TOL
        clear = np.abs(prob[1].astype(np.float64) - prob[0]) >= MARGIN
        assert np.array_equal(mask[0][clear], prob.argmax(0)[clear]) and 0.0 <= r["dice"] <= 1.0
    with pytest.raises(ValueError, match="config.save_probabilities"):
        run("refused", "config.save_probabilities=true")
    with pytest.raises(ValueError, match="config.patch_overlap"):
        run("refused", "config.overlap_mode=average", "config.patch_overlap=5")


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_launch_nothing(seg):
    from mi355seg.predict import window_table, window_weights
    F = seg.functional
    size, patch = (16, 16, 16), (8, 8, 8)
    table = torch.from_numpy(window_table(size, patch, (4, 4, 4))).cuda()
    w = window_weights("hann", patch)
    acc = torch.zeros((2,) + size, device="cuda")
    lg = torch.randn((2, 2) + patch, device="cuda")
    bad_calls = [
        lambda: F.aggregate_patches(torch.zeros((1,) + size, device="cuda"), lg[:, :1], table, 0, w),          # K = 1
        lambda: F.aggregate_patches(torch.zeros((17,) + size, device="cuda"), lg[:, :1].expand(2, 17, 8, 8, 8), table, 0, w),
        lambda: F.aggregate_patches(acc.cpu(), lg, table, 0, w),                                               # CPU tensors
        lambda: F.aggregate_patches(acc, lg.cpu(), table, 0, w),
        lambda: F.aggregate_patches(acc, lg, table.cpu(), 0, w),
        lambda: F.aggregate_patches(acc, lg.double(), table, 0, w),                                            # dtypes
        lambda: F.aggregate_patches(acc.double(), lg, table, 0, w),
        lambda: F.aggregate_patches(acc, lg, table.long(), 0, w),
        lambda: F.aggregate_patches(acc, torch.randn((1, 2, 8, 8, 17), device="cuda"), table, 0, window_weights("hann", (8, 8, 17))),   # patch > volume
        lambda: F.aggregate_patches(acc, lg, table, table.shape[0] - 1, w),                                    # rows past the table
        lambda: F.aggregate_patches(acc, lg, table, -1, w),
        lambda: F.aggregate_patches(acc, lg, table, 0, window_weights("hann", (8, 8, 9))),                     # window of another patch
        lambda: F.aggregate_patches(acc, lg[:, :, :, :, :4], table, 0, w),
        lambda: F.aggregate_patches(acc[:, :, :, ::2], lg, table, 0, w),                                       # accumulator not contiguous
        lambda: F.aggregate_finalize(acc[:1], [np.ones(16)] * 3),
        lambda: F.aggregate_finalize(acc.cpu(), [np.ones(16)] * 3),
        lambda: F.aggregate_finalize(acc, [np.ones(16)] * 2),
        lambda: F.aggregate_finalize(acc, [np.ones(16), np.ones(16), np.ones(15)]),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(seg.Mi355SegError):
            call()
            pytest.fail(f"call {i} was not refused")
    torch.cuda.synchronize()
    assert float(acc.abs().max()) == 0.0
    # the library itself refuses too, whatever the Python layer lets through
    L, st = seg.lib(), torch.cuda.current_stream().cuda_stream
    wd = [torch.from_numpy(v.astype(np.float32)).cuda() for v in w]
    with pytest.raises(seg.Mi355SegError, match="K"):
        L.call("mi355seg_aggregate_patches_f32", lg.data_ptr(), 1, table.data_ptr(), 0, 2, 8, 8, 8, *[v.data_ptr() for v in wd], acc.data_ptr(), 16, 16, 16, st)
    with pytest.raises(seg.Mi355SegError, match="larger than the volume"):
        L.call("mi355seg_aggregate_patches_f32", lg.data_ptr(), 2, table.data_ptr(), 0, 2, 8, 8, 8, *[v.data_ptr() for v in wd], acc.data_ptr(), 16, 4, 16, st)
    torch.cuda.synchronize()
    assert float(acc.abs().max()) == 0.0
