"""The kernels of csrc/augment.hip (statistics of a visit, the resampling gather) through ``functional.augment_stats`` /
``functional.augment_sample``, the augmenting ``DevicePatchQueue`` and ``train.py config.aug=true``, against the FLOAT64 restatement
of tests/aug_reference.py given the SAME drawn parameters (dataloader.py:69-86 with config.aug=True; UNPINNED, see
``mi355seg.data.AugmentParams``).

Bounds -- all computed from the inputs of the case, none tuned:
  * statistics: every term x*b carries at most 2^-22 relative error (the fp32 bias field and product); propagated linearly to the mean
    and the unbiased std, plus the fp32 rounding of the two results;
  * coordinates: the device may err by eps_t = 2^-24 * (8 max(n) + 64 max|cp|) voxels;
  * image voxels: 3 eps_t L + 2^-24 (16 |V|max + (8 |x b|max + |mu|) rho), L the largest step between adjacent voxels of V; voxels
    whose fp64 coordinate lies within 4 eps_t of the domain border are left out;
  * labels: equality; voxels within 4 eps_t of a half-integer coordinate are left out;
  * the left-out share of a case may not exceed 2 %;
  * noise over N voxels: |mean| <= 5 / sqrt(N), |std - 1| <= 5 / sqrt(2 N), |lag-1 correlation| <= 5 / sqrt(N).
Every graded figure is printed (``pytest -rA``)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import aug_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mi355seg
    mi355seg.lib()          # raises if the HIP library is missing -- no fallback
    return mi355seg


# ----------------------------------------------------------------------------- helpers
def _params(seg):
    from mi355seg.data import AugmentParams
    return AugmentParams


def _volume(C, shape, seed, offset=0.0, scale=1.0):
    """float32 [C,D,H,W]: a smooth anatomy-like field plus voxel noise, shifted and scaled"""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")
    out = []
    for c in range(C):
        f = np.sin(3.1 * z + c) * np.cos(2.3 * y - 0.5 * c) + 0.5 * np.sin(4.7 * x * (1 + 0.2 * c))
        out.append(f + 0.3 * rng.normal(size=shape))
    return (np.stack(out) * scale + offset).astype(np.float32)


def _labels(Cy, shape, K=4):
    """float32 [Cy,D,H,W] of K integer classes in blocks (several classes in every patch)"""
    z, y, x = np.indices(shape)
    return np.stack([((z // (5 + c) + y // (7 + c) + x // 9) % K) for c in range(Cy)]).astype(np.float32)


def _make(seg, shape, seed, elastic, flip, sigma=None):
    P = _params(seg)
    rng = np.random.default_rng(seed)
    bias = rng.uniform(-0.5, 0.5, 20)
    sigma = rng.uniform(0.05, 0.25) if sigma is None else sigma
    sd = int(rng.integers(0, 1 << 63))
    if elastic:
        cp = np.zeros((3, 7, 7, 7))
        cp[:, 2:5, 2:5, 2:5] = rng.uniform(-7.5, 7.5, (3, 3, 3, 3))
        return P(shape, bias, sigma, sd, flip, True, cp=cp)
    return P(shape, bias, sigma, sd, flip, False, scales=rng.uniform(0.9, 1.1, 3), degrees=rng.uniform(-10, 10, 3))


def _sample(seg, x, y, prm, origins, ps, stats=None):
    F = seg.functional
    stats = F.augment_stats(x, prm) if stats is None else stats
    cp = torch.from_numpy(prm.cp).cuda() if prm.elastic else None
    xb, yb = F.augment_sample([(x, y, stats, cp, o, prm) for o in origins], ps)
    return xb, yb, stats


def _recover_noise(seg, C, shape, seed):
    """g(seed, .) over a whole [C,D,H,W] volume as (sigma=1 result - sigma=0 result) with the identity map and c = 0, on a +-1
    checkerboard (|V| ~ 1, so the difference of the two fp32 results carries g to ~2^-23)."""
    P = _params(seg)
    cb = ((np.indices((C,) + tuple(shape)).sum(0) % 2) * 2 - 1).astype(np.float32)
    x = torch.from_numpy(cb).cuda()
    y = torch.zeros((1,) + tuple(shape), device="cuda")
    p1, p0 = P(shape, np.zeros(20), 1.0, seed, False, False), P(shape, np.zeros(20), 0.0, seed, False, False)
    a, _, s1 = _sample(seg, x, y, p1, [(0, 0, 0)], shape)
    b, _, s0 = _sample(seg, x, y, p0, [(0, 0, 0)], shape)
    assert torch.equal(s1[:2], s0[:2])                         # sigma does not enter mu, rho
    return (a[0].double() - b[0].double()).cpu().numpy()


def _corners(shape, ps):
    return [tuple((n - p) * b for n, p, b in zip(shape, ps, bits)) for bits in np.ndindex(2, 2, 2)]


# ----------------------------------------------------------------------------- statistics
# the block regimes of the two-stage reduction (256 threads, at most 1024 blocks; the 16-byte path has a quarter of the work items):
# one block with fewer than 64 live threads, more than 256 blocks (the finalize's ragged second trip), past the cap with a ragged tail
STATS_REGIMES = [(1, (3, 4, 5), 0.0, 1.0), (1, (3, 4, 8), 0.0, 1.0), (1, (41, 41, 41), 0.0, 1.0), (1, (64, 64, 68), 0.0, 1.0),
                 (1, (65, 65, 65), 0.0, 1.0), (1, (104, 104, 104), 0.0, 1.0)]


@pytest.mark.parametrize("C,shape,offset,scale", [(3, (41, 67, 53), -300.0, 1.0), (1, (45, 51, 64), 0.0, 1.0), (4, (33, 40, 37), 40.0, 12.0)] + STATS_REGIMES)
def test_statistics_against_fp64(seg, C, shape, offset, scale):
    """mu, rho and min V of a visit: odd sizes (scalar path) and W % 4 == 0 (16-byte path), several channels, a CT-like offset (mean
    -300, std 1); two runs bitwise equal."""
    prm = _make(seg, shape, 11 + C, False, False)
    xh = _volume(C, shape, 3 + C, offset, scale)
    x = torch.from_numpy(xh).cuda()
    F = seg.functional
    st = F.augment_stats(x, prm)
    st2 = F.augment_stats(x, prm)
    assert torch.equal(st, st2), "the statistics must be bitwise reproducible"
    mu_d, rho_d, pad_d, sig_d = [float(v) for v in st.cpu().double()]
    mu, rho, xb = R.stats(xh, prm.bias)
    n, std = xb.size, 1.0 / rho
    delta = 4 * U                                              # 2^-22 relative per term x * b
    b_mu = delta * float(np.abs(xb).mean()) + U * abs(mu)
    d_var = 2 * delta * float((np.abs(xb - mu) * np.abs(xb)).sum()) / (n - 1)
    b_rho = rho * (d_var / (2 * std)) / std + U * rho
    print(f"[augment] stats C={C} {shape} offset={offset}: mu {mu_d:.9g} vs {mu:.9g} (err {abs(mu_d - mu):.3e}, bound {b_mu:.3e});  "
          f"rho {rho_d:.9g} vs {rho:.9g} (err {abs(rho_d - rho):.3e}, bound {b_rho:.3e})")
    assert abs(mu_d - mu) <= b_mu and abs(rho_d - rho) <= b_rho
    assert sig_d == float(np.float32(prm.sigma))
    g = _recover_noise(seg, C, shape, prm.seed)
    V = R.volume(xb, mu_d, rho_d, sig_d, g)
    b_v = U * (16 * float(np.abs(V).max()) + (8 * float(np.abs(xb).max()) + abs(mu_d)) * rho_d)
    print(f"[augment] stats min V {pad_d:.9g} vs {V.min():.9g} (err {abs(pad_d - V.min()):.3e}, bound {b_v:.3e})")
    assert abs(pad_d - float(V.min())) <= b_v


# ----------------------------------------------------------------------------- identity and flip: exact
@pytest.mark.parametrize("C,shape,ps", [(1, (30, 37, 44), (8, 12, 16)), (3, (21, 26, 31), (9, 10, 11))])
def test_identity_and_flip_are_exact(seg, C, shape, ps):
    """identity map, sigma = 0, c = 0: the batch equals the z-normalised plain windows, the labels the plain windows; flip-only equals
    torch.flip of the mirrored windows -- bit for bit, every voxel (the coordinates are integers)."""
    P = _params(seg)
    x = torch.from_numpy(_volume(C, shape, 5, offset=-120.0, scale=30.0)).cuda()
    y = torch.from_numpy(_labels(2, shape)).cuda()
    origins = _corners(shape, ps) + [tuple((n - p) // 2 for n, p in zip(shape, ps))]
    for flip in (False, True):
        prm = P.identity(shape, flip=flip)
        xb, yb, st = _sample(seg, x, y, prm, origins, ps)
        V = (x - st[0]) * st[1]
        assert float(st[2]) == float(V.min()) and float(st[3]) == 0.0
        for i, o in enumerate(origins):
            if flip:
                lo = shape[0] - o[0] - ps[0]
                sl = (slice(None), slice(lo, lo + ps[0]), slice(o[1], o[1] + ps[1]), slice(o[2], o[2] + ps[2]))
                want_x, want_y = torch.flip(V[sl], dims=(1,)), torch.flip(y[sl], dims=(1,))
            else:
                sl = (slice(None),) + tuple(slice(a, a + p) for a, p in zip(o, ps))
                want_x, want_y = V[sl], y[sl]
            assert torch.equal(xb[i], want_x), f"flip={flip} origin {o}: image differs by {float((xb[i] - want_x).abs().max()):.3e}"
            assert torch.equal(yb[i], want_y), f"flip={flip} origin {o}: labels differ"
    # the plain z-normalisation kernel agrees to rounding (its sums run in another order): mu and rho rounded to fp32 in either
    # kernel (2 U |mu| rho + 2 U |V|), then the two operations of (x - mu) * rho (2 U |V|)
    zn = seg.functional.znormalize(x)
    assert float((zn - (x - st[0]) * st[1]).abs().max()) <= 2 * U * abs(float(st[0])) * float(st[1]) + 4 * U * float(zn.abs().max())


# ----------------------------------------------------------------------------- noise
def test_noise_field(seg):
    """g recovered over a whole volume: moments, lag-1 correlation along every axis, the same value from two overlapping patches,
    another field for another seed."""
    C, shape, seed = 2, (40, 45, 52), 0x1234567890ABCDEF >> 1
    g = _recover_noise(seg, C, shape, seed)
    N = g.size
    mean, std = float(g.mean()), float(g.std())
    print(f"[augment] noise N={N}: mean {mean:.3e} (bound {5 / math.sqrt(N):.3e}), std-1 {std - 1:.3e} (bound {5 / math.sqrt(2 * N):.3e}), "
          f"max|g| {np.abs(g).max():.3f}")
    assert np.isfinite(g).all() and abs(mean) <= 5 / math.sqrt(N) and abs(std - 1) <= 5 / math.sqrt(2 * N)
    z = (g - mean) / std
    for ax in (0, 1, 2, 3):
        a, b = np.moveaxis(z, ax, 0)[:-1], np.moveaxis(z, ax, 0)[1:]
        r = float((a * b).mean())
        print(f"[augment] noise lag-1 correlation along axis {ax}: {r:.3e} (bound {5 / math.sqrt(N):.3e})")
        assert abs(r) <= 5 / math.sqrt(N)
    g2 = _recover_noise(seg, C, shape, seed + 1)
    assert float(np.abs(g2 - g).mean()) > 0.5                  # E|a - b| = 2 / sqrt(pi) = 1.13 for independent normals
    # the value at a voxel is the same from two overlapping patches (sigma = 1 on a real volume)
    P = _params(seg)
    x = torch.from_numpy(_volume(C, shape, 8)).cuda()
    y = torch.zeros((1,) + shape, device="cuda")
    prm = P(shape, np.zeros(20), 1.0, seed, False, False)
    xb, _, _ = _sample(seg, x, y, prm, [(0, 0, 0), (8, 5, 4)], (24, 28, 32))
    assert torch.equal(xb[0][:, 8:, 5:, 4:], xb[1][:, :16, :23, :28])


# ----------------------------------------------------------------------------- affine and elastic against fp64
CASES = [   # C, Cy, shape (non-cubic, odd, 40..260), patch, elastic, flip
    (1, 1, (131, 45, 257), (24, 32, 30), False, False),
    (4, 2, (41, 259, 87), (24, 40, 32), False, True),
    (1, 2, (67, 131, 45), (32, 24, 28), True, True),
    (4, 1, (45, 87, 131), (24, 32, 30), True, False),
]


@pytest.mark.parametrize("C,Cy,shape,ps,elastic,flip", CASES)
def test_resampling_against_fp64(seg, C, Cy, shape, ps, elastic, flip):
    prm = _make(seg, shape, 100 + C + 2 * elastic + flip, elastic, flip)
    xh, yh = _volume(C, shape, 21 + C, offset=5.0, scale=3.0), _labels(Cy, shape)
    x, y = torch.from_numpy(xh).cuda(), torch.from_numpy(yh).cuda()
    corners = _corners(shape, ps)
    origins = corners + [tuple((n - p) // 2 for n, p in zip(shape, ps)), tuple((n - p) // 3 for n, p in zip(shape, ps))]
    xb, yb, st = _sample(seg, x, y, prm, origins, ps)
    xb, yb = xb.cpu().double().numpy(), yb.cpu().double().numpy()
    mu, rho, pad_d, sigma = [float(v) for v in st.cpu().double()]
    g = _recover_noise(seg, C, shape, prm.seed)
    _, _, xbias = R.stats(xh, prm.bias)
    V = R.volume(xbias, mu, rho, sigma, g)
    pad = float(V.min())
    eps_t = U * (8 * max(shape) + 64 * (float(np.abs(prm.cp).max()) if elastic else 0.0))
    L = R.adjacent_step(V)
    bound = 3 * eps_t * L + U * (16 * float(np.abs(V).max()) + (8 * float(np.abs(xbias).max()) + abs(mu)) * rho)
    label_set = set(np.unique(yh).tolist()) | {0.0}
    worst, n_img, n_lab, left_img, left_lab, n_out_corner = 0.0, 0, 0, 0, 0, 0
    for i, o in enumerate(origins):
        t = R.coordinates(prm, o, ps)
        want_x, ins = R.sample_image(V, t, pad)
        want_y, _ = R.sample_label(yh.astype(np.float64), t)
        keep_x = R.border_distance(t, shape) > 4 * eps_t
        keep_y = R.half_integer_distance(t) > 4 * eps_t
        n_img += keep_x.size; left_img += int((~keep_x).sum())
        n_lab += keep_y.size; left_lab += int((~keep_y).sum())
        if i < 8:
            n_out_corner += int((~ins).sum())
        err = np.abs(xb[i] - want_x)[:, keep_x]
        worst = max(worst, float(err.max()))
        assert np.isfinite(xb[i]).all()
        assert float(err.max()) <= bound, f"origin {o}: image error {err.max():.3e} > bound {bound:.3e}"
        bad = (yb[i] != want_y)[:, keep_y]
        assert not bad.any(), f"origin {o}: {int(bad.sum())} label voxels differ"
        assert set(np.unique(yb[i]).tolist()) <= label_set
    out_share = n_out_corner / (8 * np.prod(ps))
    print(f"[augment] {'elastic' if elastic else 'affine'} C={C} {shape} flip={flip}: image error {worst:.3e}  bound {bound:.3e}  "
          f"(eps_t {eps_t:.2e}, L {L:.2f}, |V|max {np.abs(V).max():.2f});  left out: image {left_img / n_img:.4%}, labels {left_lab / n_lab:.4%};  "
          f"out-of-domain share of the corner patches {out_share:.2%};  pad {pad_d:.6g} vs {pad:.6g}")
    assert left_img / n_img <= 0.02 and left_lab / n_lab <= 0.02, "more than 2 % of a case left out"
    assert out_share > 0.0, "the corner patches never left the domain: the pad path is not graded"


def test_trilinear_gather_against_scipy(seg):
    """the gather (and the fp64 restatement) against scipy.ndimage.map_coordinates(order=1) on interior voxels of an affine case"""
    from scipy.ndimage import map_coordinates
    C, shape, ps = 2, (47, 61, 53), (24, 24, 28)
    prm = _make(seg, shape, 77, False, True)
    xh = _volume(C, shape, 9)
    x, y = torch.from_numpy(xh).cuda(), torch.zeros((1,) + shape, device="cuda")
    o = tuple((n - p) // 2 for n, p in zip(shape, ps))
    xb, _, st = _sample(seg, x, y, prm, [o], ps)
    mu, rho, _, sigma = [float(v) for v in st.cpu().double()]
    _, _, xbias = R.stats(xh, prm.bias)
    V = R.volume(xbias, mu, rho, sigma, _recover_noise(seg, C, shape, prm.seed))
    t = R.coordinates(prm, o, ps)
    n = np.asarray(shape, dtype=np.float64)[:, None, None, None]
    interior = np.all((t >= 0) & (t <= n - 1), axis=0)
    assert interior.mean() > 0.9
    eps_t = U * 8 * max(shape)
    bound = 3 * eps_t * R.adjacent_step(V) + U * (16 * float(np.abs(V).max()) + (8 * float(np.abs(xbias).max()) + abs(mu)) * rho)
    ours, _ = R.sample_image(V, t, 0.0)
    for c in range(C):
        sp = map_coordinates(V[c], t, order=1, mode="nearest")
        assert float(np.abs(sp - ours[c])[interior].max()) <= 1e-12 * max(1.0, float(np.abs(V).max()))
        err = float(np.abs(xb[0, c].cpu().double().numpy() - sp)[interior].max())
        print(f"[augment] scipy cross-check channel {c}: error {err:.3e}  bound {bound:.3e}")
        assert err <= bound


# ----------------------------------------------------------------------------- the queue on the device
def _write(tmp_path, n=3, shape=(28, 34, 40), C=2):
    (tmp_path / "x").mkdir()
    (tmp_path / "y").mkdir()
    vols = []
    for i in range(n):
        xv, yv = _volume(C, shape, 50 + i, offset=10.0 * i, scale=1.0 + i), _labels(1, shape, K=3)[0]
        np.save(tmp_path / "x" / f"v{i}.npy", xv)
        np.save(tmp_path / "y" / f"v{i}.npy", yv)
        vols.append((xv, yv))
    return vols


def test_augmenting_queue_on_the_device(seg, tmp_path):
    from mi355seg.data import DevicePatchQueue
    F = seg.functional
    vols = _write(tmp_path)
    ps, spv = (16, 16, 20), 3
    mk = lambda aug, seed=11: DevicePatchQueue(str(tmp_path / "x"), str(tmp_path / "y"), ps, batch_size=2, iters=9, device="cuda:0", seed=seed,
                                               queue_length=6, samples_per_volume=spv, aug=aug)
    q, q2, plain = mk(True), mk(True), mk(False)
    seen, batches = [], []
    for b in q:
        xb, yb = b["source"]["data"], b["gt"]["data"]
        assert xb.is_cuda and yb.is_cuda and xb.dtype == torch.float32 and yb.dtype == torch.float32
        assert xb.shape == (2, 2) + ps and yb.shape == (2, 1) + ps and bool(torch.isfinite(xb).all())
        assert len(q.last_patches) == 2
        for i, (xv, yv, stats, cp, o, prm) in enumerate(q.last_patches):
            # the patch again through the public op with its visit's parameters (statistics recomputed: bitwise reproducible)
            st = F.augment_stats(xv, prm)
            assert torch.equal(st, stats)
            rx, ry = F.augment_sample([(xv, yv, st, None if cp is None else torch.from_numpy(prm.cp).cuda(), o, prm)], ps)
            assert torch.equal(rx[0], xb[i]) and torch.equal(ry[0], yb[i])
            seen.append((prm, o))                       # (the object itself: keeps its id from being reused)
        batches.append((xb, yb))
    pb = list(plain)
    assert len(batches) == len(pb) == 9
    for (xb, yb), p in zip(batches, pb):                                    # shapes and dtypes as un-augmented
        assert xb.shape == p["source"]["data"].shape and xb.dtype == p["source"]["data"].dtype
        assert yb.shape == p["gt"]["data"].shape and yb.dtype == p["gt"]["data"].dtype
    for (xb, yb), b in zip(batches, q2):                                    # the same seed gives the same batches
        assert torch.equal(xb, b["source"]["data"]) and torch.equal(yb, b["gt"]["data"])
    other = next(iter(mk(True, seed=12)))
    assert not torch.equal(other["source"]["data"], batches[0][0])
    # the spv patches of a visit share one AugmentParams (18 patches consumed = 6 whole visits), at different origins
    groups = {}
    for prm, o in seen:
        groups.setdefault(id(prm), []).append(o)
    assert len(seen) == 18 and len(groups) == 6 and all(len(v) == spv for v in groups.values())
    assert any(len(set(v)) > 1 for v in groups.values())
    for idx, (xv, yv) in enumerate(vols):                                   # the RAW volume is what is cached
        assert torch.equal(q.cache[idx][0].cpu(), torch.from_numpy(xv)) and torch.equal(q.cache[idx][1].cpu()[0], torch.from_numpy(yv))


# ----------------------------------------------------------------------------- the CLI
_CHILD = r"""
import json, sys
sys.path.insert(0, %r)
import torch
import mi355seg
from mi355seg import train
first = {}
make = train.make_loader
def spy(*a, **k):
    loader = make(*a, **k)
    class Tap:
        def __len__(self): return len(loader)
        def __iter__(self):
            for b in loader:
                first.setdefault("x", b["source"]["data"].detach().cpu().clone())
                first.setdefault("y", b["gt"]["data"].detach().cpu().clone())
                yield b
    return Tap()
train.make_loader = spy
cfg, res = train.main(sys.argv[2:])
torch.save(first, sys.argv[1])
print("RESULT " + json.dumps({"hydra_path": cfg.hydra_path, "loss_avg": res["loss_avg"], "epoch": res["epoch"]}))
"""


def _run_cli(tmp_path, tag, aug):
    out = str(tmp_path / f"first_{tag}.pt")
    args = ["config=unet", f"config.output_dir={tmp_path / ('logs_' + tag)}", "config.patch_size=32,32,32", "config.epochs=1",
            f"config.aug={aug}"]
    p = subprocess.run([sys.executable, "-c", _CHILD % ROOT, out] + args, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    lines = [json.loads(l) for l in open(os.path.join(res["hydra_path"], "scalars.jsonl")).read().strip().splitlines()]
    return torch.load(out), res, lines


def test_train_cli_with_aug(seg, tmp_path):
    """``train.py config=unet config.patch_size=32,32,32 config.epochs=1 config.aug=true`` in a child process: finishes, writes finite
    losses, and its first batch differs from the aug=false run's first batch (same seed, same synthetic source)."""
    fa, ra, la = _run_cli(tmp_path, "aug", "true")
    fp, rp, lp = _run_cli(tmp_path, "plain", "false")
    assert ra["epoch"] == 1 and len(la) >= 1 and all(math.isfinite(l["Training/Loss"]) for l in la) and math.isfinite(ra["loss_avg"])
    assert fa["x"].shape == fp["x"].shape and fa["y"].shape == fp["y"].shape and fa["x"].dtype == fp["x"].dtype
    assert bool(torch.isfinite(fa["x"]).all()) and not torch.equal(fa["x"], fp["x"])
    assert set(fa["y"].unique().tolist()) <= {0.0, 1.0}
