"""Mirror test-time augmentation of the sliding-window inference on the device: mi355seg_gather_patches_flip_f32 (csrc/api.hip),
mi355seg_aggregate_patches_flip_f32 (csrc/aggregate.hip), sliding_window_predict(tta_flips=...) and config.tta / config.tta_axes.

Exact checks.  The mirrored gather is the plain gather's output flipped; the mirrored accumulate is the un-mirrored kernel (the
parent's, whose yardstick is tests/test_gpu_aggregate.py) fed ``torch.flip``ped logits; a whole walk equals the same walk written
with ``torch.flip`` and the un-mirrored entry points, whatever the batch size.  All bitwise.

Checks against fp64.  The reference is torchio's add_batch loop of tests/test_gpu_aggregate.py with the outer loop over the flips:
``acc[dst] += w3 * softmax64(unflip(logits[f, p]))``, ``ws[dst] += w3``.  The tolerance is derived as that file derives it, with the
n terms of a probability replaced by F * n (n: the most patches on one voxel of the grid): PROB_TOL = 3 * (K + F * n + 12) * 2^-24,
computed per case, between 2.9e-6 and 2.8e-5 here.  Labels must equal the fp64 argmax wherever the fp64 top-two margin is at least
2 * PROB_TOL, and at most 1 % of a case's voxels may be left out of that comparison.  Crop mode averages F softmaxes of one patch:
its margin is twice 3 * (K + F + 12) * 2^-24.  Every test prints its figures before it asserts (DESIGN.md section 4.17 has the
measured maxima)."""
import csv
import os

import numpy as np
import pytest
import torch

from oracle.fill import fill_module_, make_input

pytestmark = pytest.mark.gpu

# volume, patch, overlap, classes: each chosen for a kernel path
GRIDS = [
    ((12, 14, 23), (8, 8, 12), (4, 4, 4), 2),         # odd W, scalar kernel; x origins 0, 8, 11; 18 patches on one voxel
    ((16, 16, 40), (8, 8, 16), (4, 4, 8), 16),        # 128-bit kernel, 16 register slots
    ((12, 12, 21), (8, 8, 10), (4, 4, 4), 6),         # width not a multiple of 4
    ((9, 10, 11), (5, 6, 7), (2, 2, 2), 3),           # odd patch extents: the centre plane maps to itself
    ((16, 20, 44), (16, 16, 16), (8, 8, 6), 3),       # 128-bit kernel, x origins 0, 10, 20, 28: voxel by voxel
    ((8, 8, 16), (8, 8, 16), (0, 0, 0), 2),           # one patch
]
SOFT_MODES = ("average", "hann", "gaussian")
ALL_FLIPS = tuple(range(8))
MAX_LEFT_OUT = 0.01
EPS = 2.0 ** -24


def flip_dims(f):
    """the trailing dims (z = -3, y = -2, x = -1) that flip code f mirrors"""
    return tuple(d for d, bit in ((-3, 4), (-2, 2), (-1, 1)) if f & bit)


def np_flip(a, f):
    return np.flip(a, flip_dims(f)) if f else a


def t_flip(t, f):
    return torch.flip(t, flip_dims(f)) if f else t


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mi355seg
    mi355seg.lib()
    return mi355seg


def stream():
    return torch.cuda.current_stream().cuda_stream


def plain_gather(seg, vol, table, first, count, patch):
    """the un-mirrored entry point itself, not the wrapper"""
    x = torch.empty((count, vol.shape[0]) + tuple(patch), dtype=torch.float32, device="cuda")
    seg.lib().call("mi355seg_gather_patches_f32", vol.data_ptr(), vol.shape[0], *vol.shape[1:], table.data_ptr(), first, count, *patch,
                   x.data_ptr(), stream())
    return x


def most_patches_on_a_voxel(size, patch, overlap):
    from mi355seg.predict import grid_locations
    cover = np.zeros(size, dtype=np.int64)
    for z, y, x in grid_locations(size, patch, overlap):
        cover[z:z + patch[0], y:y + patch[1], x:x + patch[2]] += 1
    return int(cover.max())


def prob_tol(K, F, n):
    return 3.0 * (K + F * n + 12) * EPS


def softmax64(logits):
    l = np.asarray(logits, dtype=np.float64)
    e = np.exp(l - l.max(axis=-4, keepdims=True))
    return e / e.sum(axis=-4, keepdims=True)


def reference(size, patch, overlap, mode, flips, probs):
    """torchio's GridAggregator in fp64 with the outer loop over the flips.  probs[f][p]: the fp64 softmax of the logits of patch p
    under flip code f, NOT yet un-mirrored, [K, pd, ph, pw] -> prob [K, D, H, W]"""
    from mi355seg.predict import grid_locations, window_weights
    wz, wy, wx = window_weights(mode, patch)
    w3 = wz[:, None, None] * wy[None, :, None] * wx[None, None, :]
    locs = grid_locations(size, patch, overlap)
    K = probs[flips[0]][0].shape[0]
    acc = np.zeros((K,) + tuple(size), dtype=np.float64)
    ws = np.zeros(size, dtype=np.float64)
    for f in flips:
        assert len(probs[f]) == len(locs)
        for p, (z, y, x) in enumerate(locs):
            dst = (slice(z, z + patch[0]), slice(y, y + patch[1]), slice(x, x + patch[2]))
            acc[(slice(None),) + dst] += w3 * np_flip(probs[f][p], f)
            ws[dst] += w3
    return acc / ws


def grade(tag, labels, prob, ref, tol, margin=None):
    """the module docstring's rules; prints the figures before it asserts.  prob=None: labels only"""
    margin = 2 * tol if margin is None else margin
    labels = labels.cpu().numpy().reshape(ref.shape[1:])
    err = float(np.abs(prob.cpu().numpy().astype(np.float64) - ref).max()) if prob is not None else None
    top = np.sort(ref, axis=0)
    decisive = top[-1] - top[-2] >= margin
    left_out = 1.0 - float(decisive.mean())
    wrong = int((labels != ref.argmax(axis=0))[decisive].sum())
    figure = "labels only" if err is None else f"max|prob - fp64| = {err:.3e} (tolerance {tol:.3e})"
    print(f"{tag}: {figure}, margin {margin:.3e}, voxels left out of the label comparison {100 * left_out:.3f} %, wrong labels {wrong}")
    if prob is not None:
        assert torch.isfinite(prob).all()
        assert err <= tol
    assert left_out <= MAX_LEFT_OUT
    assert wrong == 0


_CASES = {}


def case_logits(grid):
    """float32 [8, P, K, pd, ph, pw]: 4 * standard_normal drawn independently per flip code and patch; computed once, never written to"""
    from mi355seg.predict import grid_locations
    if ("logits", grid) not in _CASES:
        size, patch, overlap, K = GRIDS[grid]
        P = len(grid_locations(size, patch, overlap))
        lg = (4.0 * np.random.default_rng(2000 + grid).standard_normal((8, P, K) + tuple(patch))).astype(np.float32)
        lg.setflags(write=False)
        _CASES["logits", grid] = lg
    return _CASES["logits", grid]


def case_reference(grid, mode, flips):
    if ("probs", grid) not in _CASES:
        sm = softmax64(case_logits(grid))
        sm.setflags(write=False)
        _CASES["probs", grid] = sm
    if (grid, mode, flips) not in _CASES:
        size, patch, overlap, _ = GRIDS[grid]
        ref = reference(size, patch, overlap, mode, flips, _CASES["probs", grid])
        ref.setflags(write=False)
        _CASES[grid, mode, flips] = ref
    return _CASES[grid, mode, flips]


# ------------------------------------------------------------------------------------------------ 1. gather
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("grid", [0, 1, 2, 3])
def test_mirrored_gather_is_the_plain_gather_flipped(seg, grid, C):
    from mi355seg.predict import window_table
    F = seg.functional
    size, patch, overlap, _ = GRIDS[grid]
    table_h = window_table(size, patch, overlap)
    table, P = torch.from_numpy(table_h).cuda(), table_h.shape[0]
    vol_h = np.random.default_rng(50 + grid).standard_normal((C,) + size).astype(np.float32)
    vol = torch.from_numpy(vol_h).cuda()
    plain = plain_gather(seg, vol, table, 0, P, patch).cpu().numpy()
    want = np.stack([vol_h[:, z:z + patch[0], y:y + patch[1], x:x + patch[2]] for z, y, x in table_h[:, :3]])
    assert np.array_equal(plain, want)
    first = P // 2
    for f in ALL_FLIPS:
        got = F.gather_patches(vol, table, 0, P, patch, flip=f)
        assert got.shape == (P, C) + patch and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy(), np_flip(plain, f)), f
        part = F.gather_patches(vol, table, first, P - first, patch, flip=f)          # rows first .. of the table
        assert np.array_equal(part.cpu().numpy(), np_flip(plain[first:], f)), f
    # flip 0 of the new entry point gives the bytes of the old one
    x = torch.full((P, C) + patch, float("nan"), dtype=torch.float32, device="cuda")
    seg.lib().call("mi355seg_gather_patches_flip_f32", vol.data_ptr(), C, *size, table.data_ptr(), 0, P, *patch, 0, x.data_ptr(), stream())
    assert np.array_equal(x.cpu().numpy(), plain)


# ------------------------------------------------------------------------------------------------ 2. accumulate, exact
@pytest.mark.parametrize("grid", range(len(GRIDS)))
def test_mirrored_accumulate_is_the_plain_kernel_on_flipped_logits(seg, grid):
    """Asymmetric windows (a ramp per axis): a kernel that mirrored the weights too would differ."""
    from mi355seg.predict import window_table
    F = seg.functional
    size, patch, overlap, K = GRIDS[grid]
    table = torch.from_numpy(window_table(size, patch, overlap)).cuda()
    P = table.shape[0]
    lg = torch.tensor(case_logits(grid)).cuda()
    w = [(1.0 + np.arange(p)) / p for p in patch]
    filled = torch.from_numpy(np.random.default_rng(70 + grid).standard_normal((K,) + size).astype(np.float32)).cuda()
    for f in ALL_FLIPS:
        flipped = t_flip(lg[f], f).contiguous()
        for start in (torch.zeros_like(filled), filled):
            got, want = start.clone(), start.clone()
            for i in range(0, P, 3):
                F.aggregate_patches(got, lg[f, i:i + 3], table, i, w, flip=f)
                F.aggregate_patches(want, flipped[i:i + 3], table, i, w)
            assert torch.equal(got, want), f
        if f == 0:                                    # flip 0 of the new entry point gives the bytes of the old one
            wd = [torch.from_numpy(v.astype(np.float32)).cuda() for v in w]
            direct = filled.clone()
            for i in range(0, P, 3):
                nb = min(3, P - i)
                seg.lib().call("mi355seg_aggregate_patches_flip_f32", lg[0, i:i + nb].data_ptr(), K, table.data_ptr(), i, nb, *patch,
                               *[v.data_ptr() for v in wd], 0, direct.data_ptr(), *size, stream())
            assert torch.equal(direct, want)
    assert not torch.equal(want, filled)


# ------------------------------------------------------------------------------------------------ 3. accumulate and finalise against fp64
@pytest.mark.parametrize("mode", SOFT_MODES)
@pytest.mark.parametrize("flips", [ALL_FLIPS, (0, 1)], ids=["F8", "F2x"])
@pytest.mark.parametrize("grid", range(len(GRIDS)))
def test_kernels_against_the_fp64_aggregator_over_flips(seg, grid, flips, mode):
    from mi355seg.predict import axis_weight_sums, tta_axis_sums, window_table, window_weights
    F = seg.functional
    size, patch, overlap, K = GRIDS[grid]
    ref = case_reference(grid, mode, flips)
    tol = prob_tol(K, len(flips), most_patches_on_a_voxel(size, patch, overlap))
    assert 2.8e-6 <= tol <= 2.9e-5
    table = torch.from_numpy(window_table(size, patch, overlap)).cuda()
    P = table.shape[0]
    w = window_weights(mode, patch)
    sums = [s.astype(np.float32) for s in axis_weight_sums(size, patch, overlap, w)]
    lg = torch.tensor(case_logits(grid)).cuda()
    acc = torch.zeros((K,) + size, dtype=torch.float32, device="cuda")
    for f in flips:
        for i in range(0, P, 3):
            F.aggregate_patches(acc, lg[f, i:i + 3], table, i, w, flip=f)
    labels, prob = F.aggregate_finalize(acc, tta_axis_sums(sums, flips), probabilities=True)
    grade(f"grid {grid} {size} / {patch} / {overlap} K={K} F={len(flips)} {mode}", labels, prob, ref, tol)
    assert float((prob.sum(0) - 1).abs().max()) <= tol


# ------------------------------------------------------------------------------------------------ 4. whole walk, exact
class PositionStub(torch.nn.Module):
    """Not mirror-equivariant: logits = patch * per-class constants + a fixed position-dependent tensor of the patch shape, so a wrong
    or missing un-mirror changes the answer.  Elementwise torch operations only: deterministic."""

    def __init__(self, K, patch, seed):
        super().__init__()
        g = np.random.default_rng(seed)
        self.register_buffer("scale", torch.from_numpy((1.0 + g.standard_normal((1, K, 1, 1, 1))).astype(np.float32)))
        self.register_buffer("where", torch.from_numpy((2.0 * g.standard_normal((1, K) + tuple(patch))).astype(np.float32)))

    def forward(self, x):
        return x[:, :1] * self.scale + self.where


class ValueStub(torch.nn.Module):
    """Mirror-equivariant: the logits depend on the voxel value only."""

    def __init__(self, K, seed):
        super().__init__()
        g = np.random.default_rng(seed)
        self.register_buffer("scale", torch.from_numpy((2.0 * g.standard_normal((1, K, 1, 1, 1))).astype(np.float32)))
        self.register_buffer("shift", torch.from_numpy(g.standard_normal((1, K, 1, 1, 1)).astype(np.float32)))

    def forward(self, x):
        return x[:, :1] * self.scale + self.shift


def case_volume(grid, C=1):
    size = GRIDS[grid][0]
    return torch.from_numpy(np.random.default_rng(90 + grid).standard_normal((C,) + size).astype(np.float32)).cuda()


def flip_walk(seg, model, vol, patch, overlap, flips, batch, mode):
    """sliding_window_predict(tta_flips=flips) written with torch.flip and the un-mirrored entry points -> (labels, prob or None,
    logits): logits[f] float32 [P, K, pd, ph, pw] on the host, as the model gave them for the mirrored patches."""
    from mi355seg.predict import axis_weight_sums, tta_axis_sums, window_table, window_weights
    F = seg.functional
    size = tuple(vol.shape[1:])
    table = torch.from_numpy(window_table(size, patch, overlap)).cuda()
    P = table.shape[0]
    recorded = {f: [] for f in flips}

    def forward(i, nb, f):
        x = t_flip(plain_gather(seg, vol, table, i, nb, patch), f).contiguous()
        with torch.no_grad():
            lg = model(x).to(torch.float32)
        recorded[f].append(lg.cpu().numpy())
        return t_flip(lg, f).contiguous()

    if mode != "crop":
        w = window_weights(mode, patch)
        sums = [torch.from_numpy(s.astype(np.float32)).cuda() for s in axis_weight_sums(size, patch, overlap, w)]
        acc = None
        for f in flips:
            for i in range(0, P, batch):
                lg = forward(i, min(batch, P - i), f)
                if acc is None:
                    acc = torch.zeros((lg.shape[1],) + size, dtype=torch.float32, device="cuda")
                F.aggregate_patches(acc, lg, table, i, w)
        labels, prob = F.aggregate_finalize(acc, tta_axis_sums(sums, flips), probabilities=True)
    else:
        prob, labels = None, torch.zeros((1,) + size, dtype=torch.int64, device="cuda")
        ones = [np.ones(p) for p in patch]
        for i in range(0, P, batch):
            nb = min(batch, P - i)
            rows = np.zeros((nb, 9), dtype=np.int32)
            rows[:, 0] = np.arange(nb) * patch[0]
            stack, buf = torch.from_numpy(rows).cuda(), None
            for f in flips:
                lg = forward(i, nb, f)
                if buf is None:
                    buf = torch.zeros((lg.shape[1], nb * patch[0]) + tuple(patch[1:]), dtype=torch.float32, device="cuda")
                F.aggregate_patches(buf, lg, stack, 0, ones)
            lab = F.argmax_channels(buf[None])
            seg.lib().call("mi355seg_paste_labels_i64", lab.data_ptr(), table.data_ptr(), i, nb, *patch, labels.data_ptr(), *size, stream())
    return labels, prob, {f: np.concatenate(v) for f, v in recorded.items()}


@pytest.mark.parametrize("mode", SOFT_MODES)
@pytest.mark.parametrize("grid,flips", [(0, ALL_FLIPS), (4, ALL_FLIPS), (3, (0, 2, 4, 6)), (1, (0, 1))])
def test_blended_walk_equals_the_torch_flip_walk_at_every_batch_size(seg, grid, flips, mode):
    from mi355seg.predict import sliding_window_predict
    size, patch, overlap, K = GRIDS[grid]
    model, vol = PositionStub(K, patch, 300 + grid).cuda(), case_volume(grid)
    want_labels, want_prob, _ = flip_walk(seg, model, vol, patch, overlap, flips, 2, mode)
    for batch in (1, 2, 5):
        labels, prob = sliding_window_predict(model, vol, patch, overlap, batch_size=batch, overlap_mode=mode, return_probabilities=True,
                                              tta_flips=flips)
        assert labels.shape == (1,) + size and labels.dtype == torch.int64 and prob.shape == (K,) + size
        assert torch.equal(labels, want_labels) and torch.equal(prob, want_prob), batch
        only = sliding_window_predict(model, vol, patch, overlap, batch_size=batch, overlap_mode=mode, tta_flips=flips)
        assert torch.equal(only, labels)
    # a missing un-mirror would not have passed: the un-augmented walk differs
    _, plain = sliding_window_predict(model, vol, patch, overlap, batch_size=2, overlap_mode=mode, return_probabilities=True)
    assert not torch.equal(plain, want_prob)
    for off in (None, (0,)):                          # None and (0,) are the call without the keyword
        _, p0 = sliding_window_predict(model, vol, patch, overlap, batch_size=2, overlap_mode=mode, return_probabilities=True, tta_flips=off)
        assert torch.equal(p0, plain)


@pytest.mark.parametrize("grid,flips", [(0, ALL_FLIPS), (4, ALL_FLIPS), (3, (0, 1, 4, 5)), (1, (0, 1)), (5, ALL_FLIPS)])
def test_crop_walk_equals_the_composition_and_the_fp64_reference(seg, grid, flips):
    from mi355seg.predict import crop_window, grid_locations, sliding_window_predict
    size, patch, overlap, K = GRIDS[grid]
    model, vol = PositionStub(K, patch, 400 + grid).cuda(), case_volume(grid)
    want, _, logits = flip_walk(seg, model, vol, patch, overlap, flips, 2, "crop")
    for batch in (1, 2, 5):
        got = sliding_window_predict(model, vol, patch, overlap, batch_size=batch, tta_flips=flips)
        assert got.shape == (1,) + size and got.dtype == torch.int64
        assert torch.equal(got, want), batch
    assert torch.equal(sliding_window_predict(model, vol, patch, overlap, batch_size=2, tta_flips=(0,)),
                       sliding_window_predict(model, vol, patch, overlap, batch_size=2))
    # numpy fp64: mean over flips of the un-mirrored softmax, pasted by crop_window (later patches win, as torchio adds them)
    ref = np.zeros((K,) + size, dtype=np.float64)
    for p, loc in enumerate(grid_locations(size, patch, overlap)):
        mean = sum(np_flip(softmax64(logits[f][p]), f) for f in flips) / len(flips)
        src, dst = crop_window(loc, patch, size, overlap)
        ref[(slice(None),) + dst] = mean[(slice(None),) + src]
    tol = 3.0 * (K + len(flips) + 12) * EPS
    grade(f"grid {grid} crop F={len(flips)}", got, None, ref, tol)


@pytest.mark.parametrize("mode", SOFT_MODES)
@pytest.mark.parametrize("grid", [0, 4])
def test_equivariant_model_gives_the_unaugmented_probabilities(seg, grid, mode):
    from mi355seg.predict import sliding_window_predict
    size, patch, overlap, K = GRIDS[grid]
    model, vol = ValueStub(K, 500 + grid).cuda(), case_volume(grid)
    tol = prob_tol(K, 8, most_patches_on_a_voxel(size, patch, overlap))
    _, plain = sliding_window_predict(model, vol, patch, overlap, batch_size=3, overlap_mode=mode, return_probabilities=True)
    _, tta = sliding_window_predict(model, vol, patch, overlap, batch_size=3, overlap_mode=mode, return_probabilities=True, tta_flips=ALL_FLIPS)
    diff = float((tta.double() - plain.double()).abs().max())
    print(f"grid {grid} {mode}: max|tta - plain| = {diff:.3e} (tolerance {tol:.3e})")
    assert diff <= tol


# ------------------------------------------------------------------------------------------------ 5. through a real model and the CLI
def record_logits(model, first_output=False):
    seen = []
    handle = model.register_forward_hook(lambda m, i, o: seen.append((o[0] if first_output else o).detach().to(torch.float32).cpu().numpy()))
    return seen, handle


def recorded_probs(seen, flips, P):
    """the hook's batches, in (flip, patch) order -> {f: fp64 softmax [P, K, pd, ph, pw]}"""
    lg = np.concatenate(seen)
    assert lg.shape[0] == len(flips) * P
    return {f: softmax64(lg[j * P:(j + 1) * P]) for j, f in enumerate(flips)}


@pytest.mark.parametrize("dtype", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_unet_with_eight_flips_against_the_reference_fed_with_the_recorded_logits(seg, dtype):
    from mi355seg.models.three_d.unet3d import UNet3D
    from mi355seg.predict import grid_locations, sliding_window_predict
    size, ps, ov = (32, 32, 48), (32, 32, 32), (4, 4, 16)
    model = fill_module_(UNet3D(1, 2, 4)).cuda().eval()
    vol = make_input((1,) + size, freq=0.017).cuda()
    P = len(grid_locations(size, ps, ov))
    seen, handle = record_logits(model)
    try:
        labels, prob = sliding_window_predict(model, vol, ps, ov, batch_size=3, dtype=dtype, overlap_mode="hann", return_probabilities=True,
                                              tta_flips=ALL_FLIPS)
    finally:
        handle.remove()
    assert labels.shape == (1,) + size and prob.shape == (2,) + size and torch.isfinite(prob).all()
    ref = reference(size, ps, ov, "hann", ALL_FLIPS, recorded_probs(seen, ALL_FLIPS, P))
    grade(f"UNet3D(1,2,4) {size} hann F=8 {dtype or 'fp32'}", labels, prob, ref, prob_tol(2, 8, most_patches_on_a_voxel(size, ps, ov)))
    assert not model.training


def test_is_network_takes_its_bands_from_the_mirrored_patch(seg, monkeypatch):
    from mi355seg.models.three_d import IS
    from mi355seg.predict import grid_locations, sliding_window_predict, window_table
    size, ps, ov = (32, 32, 40), (32, 32, 32), (4, 4, 4)
    flips = seg.functional.tta_flip_codes("x")
    fed = []
    real = IS.frequency_bands

    def spy(x, limit=0.04, impl="fft"):
        fed.append(x.clone())
        return real(x, limit, impl)
    monkeypatch.setattr(IS, "frequency_bands", spy)
    model = fill_module_(IS.UNet3D(1, 2, 4)).cuda().eval()
    vol = make_input((1,) + size, freq=0.37).cuda()
    P = len(grid_locations(size, ps, ov))
    seen, handle = record_logits(model, first_output=True)
    try:
        labels, prob = sliding_window_predict(model, vol, ps, ov, batch_size=1, overlap_mode="average", return_probabilities=True, tta_flips=flips)
    finally:
        handle.remove()
    table = torch.from_numpy(window_table(size, ps, ov)).cuda()
    plain = plain_gather(seg, vol, table, 0, P, ps)
    assert len(fed) == 2 * P
    for j, f in enumerate(flips):
        for p in range(P):
            assert torch.equal(fed[j * P + p], t_flip(plain[p:p + 1], f))
    ref = reference(size, ps, ov, "average", flips, recorded_probs(seen, flips, P))
    grade(f"IS UNet3D(1,2,4) {size} average F=2 (x)", labels, prob, ref, prob_tol(2, 2, most_patches_on_a_voxel(size, ps, ov)))


def test_predict_cli_with_tta_and_unchanged_without_the_key(seg, tmp_path):
    from mi355seg.config import compose, parse_patch_size
    from mi355seg.predict import main as predict_main, sliding_window_predict, znorm
    from mi355seg.registry import build_model
    import mi355seg.predict as P
    conf_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(P.__file__))), "conf")
    common = ["config=unet", f"config.output_dir={tmp_path / 'logs'}", "config.patch_size=32,32,32", "config.batch_size=2",
              "config.pred_data_path=synthetic"]
    cfg = compose(conf_dir, common, job_name="predict")
    parse_patch_size(cfg)
    torch.manual_seed(3)
    model = fill_module_(build_model(cfg))             # filled as the other files fill models: both classes occur in the masks
    ckpt = str(tmp_path / "model.pt")
    torch.save({"model": model.state_dict()}, ckpt)
    common.append(f"config.ckpt={ckpt}")
    model = model.cuda().eval()
    g = torch.Generator().manual_seed(7)              # predict()'s synthetic cases
    vols = []
    for _ in range(2):
        vols.append(znorm(torch.randn((cfg.in_classes, 64, 64, 64), generator=g).cuda()))
        torch.rand((1, 64, 64, 64), generator=g)

    def run(name, *keys):
        lines = []
        real = P.predict
        try:
            P.predict = lambda config, m, log=print: real(config, m, log=lambda s: (lines.append(s), print(s)))
            cfg, rows = predict_main(common + [f"config.hydra_path={tmp_path / name}"] + list(keys))
        finally:
            P.predict = real
        with open(os.path.join(cfg.hydra_path, "metrics.csv"), newline="") as fh:
            table = list(csv.reader(fh))
        assert table[0] == ["file", "jaccard", "dice"] and [r[0] for r in table[1:]] == [r["file"] for r in rows] and len(rows) == 2
        assert sorted(os.listdir(cfg.hydra_path)) == sorted(["metrics.csv"] + [r["file"] + "_pred.npy" for r in rows])
        return [np.load(os.path.join(cfg.hydra_path, r["file"] + "_pred.npy")) for r in rows], lines

    cases = [("crop", ("config.tta=mirror", "config.patch_overlap=0"), dict(overlap=(0, 0, 0), tta_flips=ALL_FLIPS)),
             ("hann", ("config.tta=mirror", "config.tta_axes=z,x", "config.overlap_mode=hann", "config.patch_overlap=8,0,0"),
              dict(overlap=(8, 0, 0), overlap_mode="hann", tta_flips=(0, 1, 4, 5))),
             ("plain", ("config.patch_overlap=0",), dict(overlap=(0, 0, 0), tta_flips=None)),
             ("off", ("config.tta=none", "config.patch_overlap=0"), dict(overlap=(0, 0, 0)))]
    for name, keys, kw in cases:
        masks, lines = run(name, *keys)
        said = [l for l in lines if l.startswith("tta:")]
        assert len(said) == (1 if kw.get("tta_flips") else 0)
        if said:
            assert f"{len(kw['tta_flips'])} flips" in said[0]
        for mask, vol in zip(masks, vols):
            want = sliding_window_predict(model, vol, (32, 32, 32), batch_size=2, **kw)
            assert mask.shape == (1, 64, 64, 64) and mask.dtype == np.uint8
            assert np.array_equal(mask, want.cpu().numpy().astype(np.uint8)), name
            print(f"{name}: {int(mask.sum())} of {mask.size} voxels labelled 1")
    with pytest.raises(ValueError, match="config.tta_axes"):
        run("refused", "config.tta_axes=x")
    with pytest.raises(ValueError, match="config.save_probabilities"):
        run("refused", "config.tta=mirror", "config.save_probabilities=true")


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_launch_nothing(seg):
    from mi355seg.predict import window_table, window_weights
    F = seg.functional
    size, patch = (16, 16, 16), (8, 8, 8)
    table = torch.from_numpy(window_table(size, patch, (4, 4, 4))).cuda()
    w = window_weights("hann", patch)
    vol = torch.zeros((1,) + size, device="cuda")
    acc = torch.zeros((2,) + size, device="cuda")
    lg = torch.randn((2, 2) + patch, device="cuda")
    bad_calls = [
        lambda: F.gather_patches(vol, table, 0, 2, patch, flip=8),
        lambda: F.gather_patches(vol, table, 0, 2, patch, flip=-1),
        lambda: F.gather_patches(vol, table, 0, 2, (8, 8, 17), flip=3),                                        # patch > volume
        lambda: F.gather_patches(vol, table, 0, 2, (8, 8), flip=3),
        lambda: F.gather_patches(vol, table, table.shape[0] - 1, 2, patch, flip=3),                            # rows past the table
        lambda: F.gather_patches(vol, table, -1, 2, patch, flip=3),
        lambda: F.gather_patches(vol, table, 0, 0, patch, flip=3),
        lambda: F.gather_patches(vol.cpu(), table, 0, 2, patch, flip=3),
        lambda: F.gather_patches(vol, table.cpu(), 0, 2, patch, flip=3),
        lambda: F.gather_patches(vol.double(), table, 0, 2, patch, flip=3),
        lambda: F.gather_patches(vol[:, :, :, ::2], table, 0, 2, patch, flip=3),
        lambda: F.gather_patches(vol[0], table, 0, 2, patch, flip=3),
        lambda: F.aggregate_patches(acc, lg, table, 0, w, flip=8),
        lambda: F.aggregate_patches(acc, lg, table, 0, w, flip=-1),
        lambda: F.aggregate_patches(acc.cpu(), lg, table, 0, w, flip=5),
        lambda: F.aggregate_patches(acc, lg.cpu(), table, 0, w, flip=5),
        lambda: F.aggregate_patches(acc, torch.randn((1, 2, 8, 8, 17), device="cuda"), table, 0, window_weights("hann", (8, 8, 17)), flip=5),
        lambda: F.aggregate_patches(acc, lg, table, table.shape[0] - 1, w, flip=5),
        lambda: F.aggregate_patches(torch.zeros((17,) + size, device="cuda"), lg[:, :1].expand(2, 17, 8, 8, 8), table, 0, w, flip=5),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(seg.Mi355SegError):
            call()
            pytest.fail(f"call {i} was not refused")
    torch.cuda.synchronize()
    assert float(acc.abs().max()) == 0.0
    # the library itself refuses too, whatever the Python layer lets through
    L = seg.lib()
    wd = [torch.from_numpy(v.astype(np.float32)).cuda() for v in w]
    out = torch.zeros((2, 1) + patch, device="cuda")
    for flip in (-1, 8):
        with pytest.raises(seg.Mi355SegError, match="flip"):
            L.call("mi355seg_gather_patches_flip_f32", vol.data_ptr(), 1, *size, table.data_ptr(), 0, 2, *patch, flip, out.data_ptr(), stream())
        with pytest.raises(seg.Mi355SegError, match="flip"):
            L.call("mi355seg_aggregate_patches_flip_f32", lg.data_ptr(), 2, table.data_ptr(), 0, 2, *patch, *[v.data_ptr() for v in wd], flip,
                   acc.data_ptr(), *size, stream())
    with pytest.raises(seg.Mi355SegError, match="larger than the volume"):
        L.call("mi355seg_aggregate_patches_flip_f32", lg.data_ptr(), 2, table.data_ptr(), 0, 2, *patch, *[v.data_ptr() for v in wd], 7,
               acc.data_ptr(), 16, 4, 16, stream())
    with pytest.raises(seg.Mi355SegError, match="bad arguments"):
        L.call("mi355seg_gather_patches_flip_f32", vol.data_ptr(), 1, 16, 4, 16, table.data_ptr(), 0, 2, *patch, 7, out.data_ptr(), stream())
    torch.cuda.synchronize()
    assert float(acc.abs().max()) == 0.0 and float(out.abs().max()) == 0.0
