"""The kernels of csrc/sampler.hip (label index build, pick select) through ``functional.label_index`` / ``functional.label_pick``, the three
C entry points and the label-sampling ``DevicePatchQueue`` (``config.sampler=label``; tio.LabelSampler semantics, UNPINNED: the
definitions of include/mi355seg.h are the specification).

The reference everywhere is numpy on the host: with ``region`` the box of valid patch centres (start ``p // 2``, extents ``n - p + 1``),
``count[l] = (region == l).sum()`` and the origin of pick (l, r) is ``np.flatnonzero(region.ravel() == l)[r]`` unravelled over the region's
extents.  The device works in integers, so every comparison is exact (``array_equal``), never within a tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 1024                    # MI355SEG_LABEL_CHUNK, the kernels' chunk of consecutive region-linear voxels (asserted below)

# volume / patch pairs of the count and build tests
CASES = {
    "6^3 region, mixed patch": ((9, 10, 11), (4, 5, 6)),            # p // 2 differs per axis; less than one chunk
    "13x26x60 region": ((20, 33, 67), (8, 8, 8)),                   # 20 chunks, ragged last one, rows no multiple of 64
    "patch = volume": ((7, 9, 12), (7, 9, 12)),                     # the region is one voxel
    "40^3 / 1^3": ((40, 40, 40), (1, 1, 1)),                        # the region is the whole volume
    "one chunk exactly": ((10, 11, 20), (3, 4, 5)),                 # region 8 x 8 x 16 = 1024 = CHUNK voxels
    "one chunk and a voxel": ((6, 7, 44), (2, 3, 4)),               # region 5 x 5 x 41 = 1025 = CHUNK + 1 voxels
    "two chunks exactly": ((9, 18, 18), (2, 3, 3)),                 # region 8 x 16 x 16 = 2048 = 2 CHUNK voxels
    # the prefix scan gives each of its 256 threads ceil(chunks / 256) consecutive chunks, walked 8 at a time:
    "70^3 region": ((73, 74, 75), (4, 5, 6)),                       # 335 chunks: 2 per thread, the threads from 168 on own none
    "129^3 region": ((130, 130, 130), (2, 2, 2)),                   # 2,097 chunks: 9 per thread (one full step of 8 and a ragged one), the last thread owns fewer
}
SINGLE, OUTSIDE, ABSENT = 5, 7, 3


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mi355seg
    mi355seg.lib()          # raises if the HIP library is missing -- no fallback
    assert mi355seg.functional.LABEL_CHUNK == CHUNK
    return mi355seg


# ----------------------------------------------------------------------------- helpers
def _region(y, ps):
    return y[tuple(slice(p // 2, p // 2 + n - p + 1) for n, p in zip(y.shape, ps))]


def _labels(shape, ps, seed):
    """float32 [D,H,W]: classes 0, 1, 2 from a seeded generator; class SINGLE on exactly one voxel of the region; class OUTSIDE only
    outside the region (where there is an outside), so its count is 0; class ABSENT nowhere"""
    rng = np.random.default_rng(seed)
    y = rng.choice(3, size=shape, p=[0.7, 0.2, 0.1]).astype(np.float32)
    inside = np.zeros(shape, dtype=bool)
    _region(inside, ps)[...] = True
    y[~inside & (rng.random(shape) < 0.3)] = OUTSIDE
    m = tuple(n - p + 1 for n, p in zip(shape, ps))
    at = tuple(int(rng.integers(0, e)) + p // 2 for e, p in zip(m, ps))
    y[at] = SINGLE
    return y


def _counts(y, ps):
    r = _region(y, ps)
    c = np.array([(r == l).sum() for l in range(16)] + [0], dtype=np.int64)
    c[16] = r.size - c[:16].sum()
    return c


def _origins(y, ps, classes, ranks):
    """the numpy statement: flatnonzero over the region, unravelled over its extents"""
    r = _region(y, ps)
    flat = r.ravel()
    where = {int(l): np.flatnonzero(flat == l) for l in np.unique(classes)}
    e = np.array([where[int(l)][int(k)] for l, k in zip(classes, ranks)], dtype=np.int64)
    return np.stack(np.unravel_index(e, r.shape), axis=1).astype(np.int32)


def _every_pick(counts):
    classes = np.concatenate([np.full(int(counts[l]), l, dtype=np.int64) for l in range(16)])
    ranks = np.concatenate([np.arange(int(counts[l]), dtype=np.int64) for l in range(16)])
    return classes, ranks


@pytest.fixture(scope="module")
def cases(seg):
    """every case's labels on the host and the device and its index, built once and left unchanged"""
    out = {}
    for i, (name, (shape, ps)) in enumerate(CASES.items()):
        y = _labels(shape, ps, 100 + i)
        yd = torch.from_numpy(y).cuda()
        out[name] = (y, ps, yd, seg.functional.label_index(yd[None], ps))
    return out


# ----------------------------------------------------------------------------- build
@pytest.mark.parametrize("name", list(CASES))
def test_counts_equal_numpy(seg, cases, name):
    y, ps, yd, index = cases[name]
    want = _counts(y, ps)
    m = tuple(n - p + 1 for n, p in zip(y.shape, ps))
    assert index.region == m and index.patch == tuple(ps) and index.shape == y.shape
    assert isinstance(index.counts, np.ndarray) and index.counts.dtype == np.int64 and index.counts.shape == (17,)
    print(f"[label] {name}: region {m}, counts {index.counts.tolist()}")
    assert np.array_equal(index.counts, want)
    assert want[SINGLE] == 1 and want[OUTSIDE] == 0 and want[ABSENT] == 0 and want[16] == 0 and want[:3].sum() == int(np.prod(m)) - 1
    if int(np.prod(m)) != y.size:
        assert (y == OUTSIDE).sum() > 0                                        # the class exists, only not in the region
    nchunks = -(-int(np.prod(m)) // CHUNK)
    assert index.index.shape == (17, nchunks) and index.index.dtype == torch.int64
    assert seg.lib().query("mi355seg_label_index_bytes", *y.shape, *ps) == nchunks * 17 * 8
    # the index itself: exclusive per-class prefixes of the per-chunk counts
    flat = np.concatenate([_region(y, ps).ravel(), np.full(nchunks * CHUNK - int(np.prod(m)), -1.0, dtype=np.float32)]).reshape(nchunks, CHUNK)
    per_chunk = np.stack([(flat == l).sum(1) for l in range(16)] + [np.zeros(nchunks, dtype=np.int64)])
    assert np.array_equal(index.index.cpu().numpy(), np.cumsum(per_chunk, axis=1) - per_chunk)


def test_labels_without_the_channel_axis_and_int_patch(seg, cases):
    y, ps, yd, index = cases["13x26x60 region"]
    again = seg.functional.label_index(yd, 8)
    assert again.patch == (8, 8, 8) and np.array_equal(again.counts, index.counts) and torch.equal(again.index, index.index)


def test_two_builds_are_bitwise_equal(seg, cases):
    for name in ("13x26x60 region", "one chunk and a voxel"):
        y, ps, yd, index = cases[name]
        again = seg.functional.label_index(yd[None], ps)
        assert torch.equal(again.index, index.index) and np.array_equal(again.counts, index.counts)


def test_bad_values_are_counted_inside_the_region_only(seg):
    shape, ps = (12, 14, 16), (4, 6, 8)
    y = _labels(shape, ps, 7)
    inside, outside = y.copy(), y.copy()
    for k, v in enumerate((16.0, -1.0, 0.5, np.nan, np.inf)):
        inside[2 + k, 3 + k, 4 + k] = v                                        # region: starts (2, 3, 4), extents (9, 9, 9)
        outside[k, 0, 15 - k] = v
    assert seg.functional.label_index(torch.from_numpy(inside).cuda(), ps).counts[16] == 5
    got = seg.functional.label_index(torch.from_numpy(outside).cuda(), ps).counts
    assert got[16] == 0 and np.array_equal(got, _counts(y, ps))                     # the region itself is untouched


# ----------------------------------------------------------------------------- select
@pytest.mark.parametrize("name", ["6^3 region, mixed patch", "13x26x60 region", "patch = volume", "one chunk exactly", "one chunk and a voxel",
                                  "two chunks exactly"])
def test_select_every_pick(seg, cases, name):
    """every (class, rank) with rank < count[class], in one call"""
    y, ps, yd, index = cases[name]
    classes, ranks = _every_pick(index.counts)
    assert classes.size == int(np.prod(index.region))
    got = seg.functional.label_pick(index, classes, ranks)
    assert got.is_cuda and got.dtype == torch.int32 and got.shape == (classes.size, 3)
    want = _origins(y, ps, classes, ranks)
    assert np.array_equal(got.cpu().numpy(), want)
    # an origin is valid and the patch cut there has the picked class at offset p // 2
    assert (want >= 0).all() and (want + np.array(ps) <= np.array(y.shape)).all()
    centre = want + np.array(ps) // 2
    assert np.array_equal(y[centre[:, 0], centre[:, 1], centre[:, 2]], classes.astype(np.float32))


def test_select_at_96_cubed(seg):
    """96^3 / 64^3 (region 33^3, 36 chunks): ranks 0 and count - 1 of every class, plus 2,000 seeded random picks"""
    shape, ps = (96, 96, 96), (64, 64, 64)
    y = _labels(shape, ps, 42)
    index = seg.functional.label_index(torch.from_numpy(y).cuda()[None], ps)
    counts = _counts(y, ps)
    assert np.array_equal(index.counts, counts) and index.region == (33, 33, 33)
    present = [l for l in range(16) if counts[l] > 0]
    rng = np.random.default_rng(9)
    rc = rng.choice(present, size=2000)
    classes = np.concatenate([np.repeat(present, 2), rc]).astype(np.int64)
    ranks = np.concatenate([np.stack([np.zeros(len(present), dtype=np.int64), counts[present] - 1], 1).ravel(),
                            rng.integers(0, counts[rc])]).astype(np.int64)
    got = seg.functional.label_pick(index, classes, ranks).cpu().numpy()
    assert np.array_equal(got, _origins(y, ps, classes, ranks))


@pytest.mark.parametrize("name", ["40^3 / 1^3", "70^3 region", "129^3 region"])
def test_select_in_large_regions(seg, cases, name):
    """63, 335 and 2,097 chunks: ranks 0, count - 1 and 3,000 seeded picks of every present class"""
    y, ps, yd, index = cases[name]
    counts = index.counts
    present = [l for l in range(16) if counts[l] > 0]
    rng = np.random.default_rng(10)
    rc = rng.choice(present, size=3000)
    classes = np.concatenate([np.repeat(present, 2), rc]).astype(np.int64)
    ranks = np.concatenate([np.stack([np.zeros(len(present), dtype=np.int64), counts[present] - 1], 1).ravel(),
                            rng.integers(0, counts[rc])]).astype(np.int64)
    got = seg.functional.label_pick(index, classes, ranks).cpu().numpy()
    assert np.array_equal(got, _origins(y, ps, classes, ranks))


def test_label_pick_validates_on_the_host(seg, cases):
    y, ps, yd, index = cases["6^3 region, mixed patch"]
    E = seg.Mi355SegError
    with pytest.raises(E, match="rank"):
        seg.functional.label_pick(index, [1], [int(index.counts[1])])                  # rank == count
    with pytest.raises(E, match="rank"):
        seg.functional.label_pick(index, [OUTSIDE], [0])                               # a class with no voxel in the region
    with pytest.raises(E, match="rank"):
        seg.functional.label_pick(index, [1], [-1])
    with pytest.raises(E, match="class 16"):
        seg.functional.label_pick(index, [16], [0])
    with pytest.raises(E, match="class -1"):
        seg.functional.label_pick(index, [-1], [0])
    with pytest.raises(E, match="integer arrays"):
        seg.functional.label_pick(index, [1.0], [0])
    with pytest.raises(E, match="integer arrays"):
        seg.functional.label_pick(index, [], [])
    with pytest.raises(E, match="no CPU fallback"):
        seg.functional.label_index(torch.from_numpy(y), ps)
    with pytest.raises(E, match="ONE label channel"):
        seg.functional.label_index(torch.from_numpy(np.stack([y, y])).cuda(), ps)
    with pytest.raises(E, match="patch"):
        seg.functional.label_index(yd, (4, 5, 12))                                     # p_w > n_w


def test_c_entry_points_refuse_bad_arguments(seg, cases):
    """non-zero return and mi355seg_last_error, never a crash; nothing here reaches a launch"""
    y, ps, yd, index = cases["6^3 region, mixed patch"]
    L = seg.lib()
    D, H, W = y.shape
    nbytes = L.query("mi355seg_label_index_bytes", D, H, W, *ps)
    assert nbytes == 17 * 8
    assert L.query("mi355seg_label_index_bytes", D, H, W, D + 1, 1, 1) == 0
    assert L.query("mi355seg_label_index_bytes", 0, H, W, 1, 1, 1) == 0
    idx, cnt = torch.empty(17, dtype=torch.int64, device="cuda"), torch.empty(17, dtype=torch.int64, device="cuda")
    picks, org = torch.zeros((1, 2), dtype=torch.int64, device="cuda"), torch.empty((1, 3), dtype=torch.int32, device="cuda")
    p = lambda t: t.data_ptr()
    bad_builds = [
        ("labels is null", (None, D, H, W, *ps, p(idx), nbytes, p(cnt), None)),
        ("index or counts17 is null", (p(yd), D, H, W, *ps, None, nbytes, p(cnt), None)),
        ("index or counts17 is null", (p(yd), D, H, W, *ps, p(idx), nbytes, None, None)),
        ("larger than the volume", (p(yd), D, H, W, D + 1, ps[1], ps[2], p(idx), nbytes, p(cnt), None)),
        (r"exceeds 2\^31", (p(yd), 2048, 1024, 1024, *ps, p(idx), nbytes, p(cnt), None)),
        ("index_bytes too small", (p(yd), D, H, W, *ps, p(idx), nbytes - 1, p(cnt), None)),
        ("bad arguments", (p(yd), D, H, W, 0, ps[1], ps[2], p(idx), nbytes, p(cnt), None)),
    ]
    for msg, args in bad_builds:
        assert L.query("mi355seg_label_index_build_f32", *args) != 0
        assert L.query("mi355seg_last_error").decode().startswith("label_index_build")
        with pytest.raises(seg.Mi355SegError, match="label_index_build: .*" + msg):
            L.call("mi355seg_label_index_build_f32", *args)
    bad_selects = [
        ("labels is null", (None, D, H, W, *ps, p(index.index), p(picks), 1, p(org), None)),
        ("index, picks or origins is null", (p(yd), D, H, W, *ps, None, p(picks), 1, p(org), None)),
        ("index, picks or origins is null", (p(yd), D, H, W, *ps, p(index.index), None, 1, p(org), None)),
        ("index, picks or origins is null", (p(yd), D, H, W, *ps, p(index.index), p(picks), 1, None, None)),
        ("larger than the volume", (p(yd), D, H, W, ps[0], H + 1, ps[2], p(index.index), p(picks), 1, p(org), None)),
        (r"exceeds 2\^31", (p(yd), 1024, 2048, 1024, *ps, p(index.index), p(picks), 1, p(org), None)),
        ("n = 0 picks", (p(yd), D, H, W, *ps, p(index.index), p(picks), 0, p(org), None)),
    ]
    for msg, args in bad_selects:
        assert L.query("mi355seg_label_index_select", *args) != 0
        with pytest.raises(seg.Mi355SegError, match="label_index_select: .*" + msg):
            L.call("mi355seg_label_index_select", *args)


# ----------------------------------------------------------------------------- the queue
def _write_sparse(tmp_path, n=3, shape=(20, 18, 24), density=0.012):
    """volumes like tests/test_data_queue.py::_write, labels sparse: foreground below 2 % of the voxels"""
    (tmp_path / "x").mkdir()
    (tmp_path / "y").mkdir()
    rng = np.random.default_rng(0)
    vols = []
    for i in range(n):
        x = (rng.normal(size=shape) * (i + 1) + 10 * i).astype(np.float32)
        y = (rng.random(shape) < density).astype(np.float32)
        assert 0 < y.mean() < 0.02
        np.save(tmp_path / "x" / f"v{i}.npy", x)
        np.save(tmp_path / "y" / f"v{i}.npy", y)
        vols.append((x, y))
    return vols


PS, KW = (8, 6, 8), dict(seed=11, queue_length=6, samples_per_volume=4)


def _queue(seg, tmp_path, probs, **kw):
    from mi355seg.data import DevicePatchQueue
    return DevicePatchQueue(str(tmp_path / "x"), str(tmp_path / "y"), PS, batch_size=2, iters=7, device="cuda:0", sampler="label",
                            label_probabilities=probs, **{**KW, **kw})


def _replay(vols, probs, iters=7, bs=2):
    """the queue's label patches from the same seed on the host: draw_label_picks + the numpy statement, refill and shuffle as the queue"""
    from mi355seg.data import draw_label_picks
    rng = np.random.default_rng(KW["seed"])
    order, queue, out = [], [], []
    for _ in range(iters * bs):
        if not queue:
            while len(queue) < KW["queue_length"]:
                if not order:
                    order = list(rng.permutation(len(vols)))
                y = vols[int(order.pop())][1]
                classes, ranks = draw_label_picks(rng, _counts(y, PS), probs, KW["samples_per_volume"])
                for o in _origins(y, PS, classes, ranks):
                    queue.append(y[tuple(slice(int(a), int(a) + p) for a, p in zip(o, PS))])
            queue = [queue[i] for i in rng.permutation(len(queue))]
        out.append(queue.pop())
    return out


@pytest.mark.parametrize("probs", [{0: 0, 1: 1}, None, "0:0.0,1:2.5"])
def test_queue_centres_every_patch_on_foreground(seg, tmp_path, probs):
    vols = _write_sparse(tmp_path)
    q = _queue(seg, tmp_path, probs)
    batches = list(q)
    assert len(batches) == 7
    for b in batches:
        x, y = b["source"]["data"], b["gt"]["data"]
        assert x.is_cuda and y.is_cuda and x.shape == (2, 1) + PS and y.shape == (2, 1) + PS and x.dtype == torch.float32
        assert (y[:, 0, PS[0] // 2, PS[1] // 2, PS[2] // 2] == 1).all()
    assert len(q.cache) == 3 and sorted(q.label_indices) == sorted(q.cache)
    for idx, (xv, yv) in enumerate(vols):
        cx, cy = q.cache[idx]                                                      # (x, y) as in the uniform queue
        assert cx.shape == (1,) + xv.shape and cy.shape == (1,) + yv.shape and np.array_equal(cy.cpu().numpy()[0], yv)


def test_queue_uses_the_picks_window_for_window(seg, tmp_path):
    """{0: 1, 1: 1}: the sequence of label patches equals the host replay of the same seed -- the draws, the select, the shuffle.
    The image patch is the same window of the z-normalised volume."""
    vols = _write_sparse(tmp_path)
    probs = {0: 1, 1: 1}
    q = _queue(seg, tmp_path, probs)
    got = [(xp, yp) for b in q for xp, yp in zip(b["source"]["data"], b["gt"]["data"])]
    want = _replay(vols, probs)
    assert len(got) == len(want) == 14
    centres = []
    for (xp, yp), w in zip(got, want):
        assert np.array_equal(yp[0].cpu().numpy(), w)
        centres.append(float(w[PS[0] // 2, PS[1] // 2, PS[2] // 2]))
    assert 0.0 in centres and 1.0 in centres                                       # both classes at weight 1 : 1 in 14 patches
    normed = {i: q.cache[i][0][0].cpu().numpy() for i in q.cache}
    for xp, yp in got[:4]:                                                         # the image window belongs to the label window
        hits = 0
        for i, (_, yv) in enumerate(vols):
            u = np.lib.stride_tricks.sliding_window_view(normed[i], PS)
            m = np.abs(u - xp[0].cpu().numpy()).max(axis=(3, 4, 5)) == 0
            for z, yy, xx in zip(*np.nonzero(m)):
                hits += 1
                assert np.array_equal(yp[0].cpu().numpy(), yv[z:z + PS[0], yy:yy + PS[1], xx:xx + PS[2]])
        assert hits == 1


def test_queue_without_a_cache_keeps_no_index(seg, tmp_path):
    """indices are kept only for subjects that are themselves cached; the patches do not depend on it"""
    vols = _write_sparse(tmp_path)
    q = _queue(seg, tmp_path, {0: 1, 1: 1}, cache_gb=0.0)
    got = [yp for b in q for yp in b["gt"]["data"]]
    assert q.cache == {} and q.label_indices == {}
    for yp, w in zip(got, _replay(vols, {0: 1, 1: 1})):
        assert np.array_equal(yp[0].cpu().numpy(), w)


def test_queue_refuses_bad_label_volumes(seg, tmp_path):
    """values 16, -1, 0.5 inside the region of valid centres: ValueError naming the file; the same values outside it: accepted.
    An all-background subject under label_probabilities=None: torchio's empty probability map.  Two label channels: refused."""
    vols = _write_sparse(tmp_path, n=1)
    y = vols[0][1]
    for k, v in enumerate((16.0, -1.0, 0.5)):
        y[k, 0, 23 - k] = v                                                        # outside: the region starts at (4, 3, 4)
    np.save(tmp_path / "y" / "v0.npy", y)
    assert len(list(_queue(seg, tmp_path, None))) == 7
    for v in (16.0, -1.0, 0.5):
        bad = y.copy()
        bad[10, 9, 12] = v
        np.save(tmp_path / "y" / "v0.npy", bad)
        with pytest.raises(ValueError, match=r"v0\.npy.*sampler='label'"):
            next(iter(_queue(seg, tmp_path, None)))
    np.save(tmp_path / "y" / "v0.npy", np.zeros_like(y))
    with pytest.raises(RuntimeError, match=r"v0\.npy.*empty probability map"):
        next(iter(_queue(seg, tmp_path, None)))
    assert len(list(_queue(seg, tmp_path, {0: 1.0}))) == 7
    np.save(tmp_path / "y" / "v0.npy", np.stack([vols[0][1], vols[0][1]]))
    with pytest.raises(seg.Mi355SegError, match=r"v0\.npy.*ONE label channel"):
        next(iter(_queue(seg, tmp_path, None)))
