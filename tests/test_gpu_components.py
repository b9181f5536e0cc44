"""Connected components on the device (csrc/components.hip) against scipy.ndimage.label with generate_binary_structure(3, 1 / 2 / 3).
Everything is exact: the answer is an integer partition, and the canonical label (1 + raster index of the component's first voxel)
leaves no freedom.  Shapes are the smallest at which the tiling can go wrong (one voxel, one row, ragged tiles on every axis,
several tiles per axis); structures that must join or stay apart across tile faces, edges and corners are placed from the tile
shape the library reports."""
import csv
import itertools
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu

CONNS = (6, 18, 26)
SHAPES = [(1, 1, 1), (1, 1, 70), (3, 5, 7), (17, 33, 65), (40, 48, 72)]


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mi355seg
    mi355seg.lib()
    return mi355seg


def _structure(conn):
    return ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn])


def _dev(mask):
    return torch.from_numpy(np.ascontiguousarray(mask)).to(torch.int64).cuda()


class Oracle:
    """scipy's labelling of one (mask, connectivity) and what follows from it: the first voxel and the size of every component"""

    def __init__(self, mask, conn):
        self.mask = np.asarray(mask)
        self.ref, self.n = ndimage.label(self.mask != 0, _structure(conn))
        flat = self.ref.ravel()
        self.counts = np.bincount(flat, minlength=self.n + 1)[1:].astype(np.int64)
        idx = np.arange(1, self.n + 1)
        lin = np.arange(flat.size, dtype=np.int64).reshape(self.ref.shape)
        self.first = np.asarray(ndimage.minimum(lin, self.ref, idx), dtype=np.int64).reshape(-1) if self.n else np.zeros(0, np.int64)

    def info(self):
        if self.n == 0:
            return [0, 0, 0, 0]
        top = int(self.counts.max())
        return [int(self.counts.sum()), self.n, top, int(self.first[self.counts == top].min()) + 1]

    def filtered(self, min_voxels, keep_largest):
        """(mask after the clean-up, stats) by numpy"""
        keep = self.counts >= min_voxels
        if keep_largest > 0:
            order = sorted(np.flatnonzero(keep), key=lambda i: (-self.counts[i], self.first[i]))[:keep_largest]
            keep = np.zeros(self.n, dtype=bool)
            keep[order] = True
        stay = np.concatenate([[False], keep])[self.ref]
        out = np.where(stay, self.mask, 0)
        stats = {"components": self.n, "kept": int(keep.sum()), "voxels_removed": int((self.mask != 0).sum() - (out != 0).sum()),
                 "largest": int(self.counts.max()) if self.n else 0}
        return out, stats


def check(F, mask, conn, what="", expect_components=None):
    mask = np.asarray(mask)
    o = Oracle(mask, conn)
    if expect_components is not None:
        assert o.n == expect_components, f"{what}: scipy itself finds {o.n} components under {conn}, the case expects {expect_components}"
    labels, sizes, info = F.connected_components(_dev(mask), conn)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == mask.shape and sizes.dtype == torch.int32 and info.dtype == torch.int64
    assert sizes.shape == (mask.size,) and info.shape == (4,)
    ours = labels.cpu().numpy()
    fg = mask != 0
    tag = f"{what} {mask.shape} connectivity {conn}"
    assert np.array_equal(ours == 0, ~fg), tag                                                           # (a)
    pairs = np.unique((ours[fg].astype(np.int64) << 32) | o.ref[fg].astype(np.int64))
    assert len(pairs) == len(np.unique(ours[fg])) == len(np.unique(o.ref[fg])) == o.n, tag               # (b)
    if o.n:
        assert np.array_equal(ours[fg].astype(np.int64), o.first[o.ref[fg] - 1] + 1), tag                # (c)
    want = np.zeros(mask.size, dtype=np.int64)
    want[o.first] = o.counts
    assert np.array_equal(sizes.cpu().numpy().astype(np.int64), want), tag                               # (d)
    assert info.tolist() == o.info(), tag                                                                # (e)
    return o


def bernoulli(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.int64)


def lattice(shape):
    """body-centred lattice (joined by corners only) in the first half along z, face-centred (joined by edges) in the second"""
    z, y, x = np.indices(shape)
    bcc = (z % 2 == y % 2) & (y % 2 == x % 2)
    fcc = (z + y + x) % 2 == 0
    return np.where(z < shape[0] // 2, bcc, fcc).astype(np.int64)


def serpentine(shape):
    """a one-voxel-wide path, as a list of voxels in walking order: every second row of every second slice, joined at alternating
    ends; each step is a face step, so the path is ONE component under 6, and it crosses every tile of the volume"""
    D, H, W = shape
    path, forward = [], True
    zs = list(range(0, D, 2))
    for zi, z in enumerate(zs):
        ys = list(range(0, H, 2))
        if zi % 2:
            ys = ys[::-1]
        for yi, y in enumerate(ys):
            xs = list(range(W)) if forward else list(range(W - 1, -1, -1))
            path += [(z, y, x) for x in xs]
            if yi + 1 < len(ys):
                path.append((z, (y + ys[yi + 1]) // 2, xs[-1]))
            forward = not forward
        if zi + 1 < len(zs):
            path.append((z + 1, ys[-1], xs[-1]))
    return path


def paint(shape, voxels, value=1):
    m = np.zeros(shape, dtype=np.int64)
    for v in voxels:
        m[v] = value
    return m


# ---------------------------------------------------------------------------------------------------------------- labelling
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_regular_patterns(seg, shape):
    F = seg.functional
    z, y, x = np.indices(shape)
    for conn in CONNS:
        check(F, np.zeros(shape, np.int64), conn, "zeros", 0)
        check(F, np.ones(shape, np.int64), conn, "ones", 1)
        board = ((z + y + x) % 2).astype(np.int64)
        check(F, board, conn, "checkerboard", int(board.sum()) if conn == 6 or board.sum() <= 1 else None)
        check(F, lattice(shape), conn, "lattice")
    if min(shape) >= 3:
        board = ((z + y + x) % 2).astype(np.int64)
        assert Oracle(board, 18).n == 1 and Oracle(board, 26).n == 1
    if shape == (40, 48, 72):
        counts = [Oracle(lattice(shape), c).n for c in CONNS]
        assert len(set(counts)) == 3, f"the lattice does not separate the three connectivities: {counts}"


@pytest.mark.parametrize("density", [0.10, 0.31, 0.50, 0.90])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bernoulli_masks(seg, shape, density):
    for conn in CONNS:
        o = check(seg.functional, bernoulli(shape, density, 11), conn, f"bernoulli {density}")
        if shape == (40, 48, 72) and density == 0.31:
            print(f"bernoulli 0.31 {shape} connectivity {conn}: {o.n} components, largest {o.info()[2]}")


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("density", [0.10, 0.31, 0.50, 0.90])
def test_bernoulli_masks_at_128_cubed(seg, density, conn):
    o = check(seg.functional, bernoulli((128, 128, 128), density, 5), conn, f"bernoulli {density}")
    print(f"bernoulli {density} 128^3 connectivity {conn}: {o.n} components, largest {o.info()[2]}")


@pytest.mark.parametrize("shape", [(17, 33, 65), (40, 48, 72)], ids=lambda s: "x".join(map(str, s)))
def test_serpentine_is_one_component_and_two_when_cut(seg, shape):
    F = seg.functional
    path = serpentine(shape)
    tiles = {tuple(c // t for c, t in zip(v, F.components_tile())) for v in path}
    assert len(tiles) == int(np.prod([-(-s // t) for s, t in zip(shape, F.components_tile())])), "the path misses a tile"
    whole = paint(shape, path)
    assert whole.sum() == len(path)
    mid = next(i for i in range(len(path) // 2, len(path)) if path[i - 1][:2] == path[i][:2] == path[i + 1][:2])   # inside a row
    cut = whole.copy()
    cut[path[mid]] = 0
    for conn in CONNS:
        check(F, whole, conn, "serpentine", 1 if conn == 6 else None)
        check(F, cut, conn, "cut serpentine", 2 if conn == 6 else None)


def test_pairs_across_tile_faces_edges_and_corners(seg):
    """Two two-voxel blocks whose nearest voxels sit on either side of the first interior tile corner, displaced by each of the 13
    backward offsets: across a tile face (joined under 6, 18, 26), a tile edge (18, 26) or the corner where eight tiles meet (26)."""
    F = seg.functional
    tile = F.components_tile()
    shape = tuple(2 * t for t in tile)
    offsets = [o for o in itertools.product((-1, 0, 1), repeat=3) if o > (0, 0, 0)]
    assert len(offsets) == 13
    for o in offsets:
        p = tuple(c - 1 if d >= 0 else c for c, d in zip(tile, o))
        q = tuple(a + d for a, d in zip(p, o))
        k = next(i for i in range(3) if o[i])
        p2 = tuple(a - o[k] if i == k else a for i, a in enumerate(p))
        q2 = tuple(a + o[k] if i == k else a for i, a in enumerate(q))
        assert all(a // t != b // t for a, b, t, d in zip(p, q, tile, o) if d) and all(0 <= a < s for v in (p2, q2) for a, s in zip(v, shape))
        mask = paint(shape, [p, q, p2, q2])
        steps = sum(1 for d in o if d)
        for conn in CONNS:
            joined = steps <= {6: 1, 18: 2, 26: 3}[conn]
            check(F, mask, conn, f"pair across offset {o}", 1 if joined else 2)


def test_parallel_planes_one_voxel_apart_never_join(seg):
    F = seg.functional
    tile = F.components_tile()
    shape = tuple(t + 5 for t in tile)
    for axis in range(3):
        for lo in (1, tile[axis] - 1):              # inside a tile, and on either side of a tile border
            m = np.zeros(shape, dtype=np.int64)
            sl = [slice(None)] * 3
            for pos in (lo, lo + 2):
                sl[axis] = pos
                m[tuple(sl)] = 1
            for conn in CONNS:
                check(F, m, conn, f"planes along axis {axis} at {lo}", 2)


def _blob(shape=(20, 24, 70)):
    z, y, x = np.indices(shape)
    ball = ((z - 9) ** 2 + (y - 11) ** 2) * 9 + (x - 33) ** 2 <= 30 ** 2
    values = np.array([1, 2, 7])[(z + 2 * y + 3 * x) % 3]
    return np.where(ball, values, 0).astype(np.int64)


def test_label_values_other_than_one_are_foreground(seg):
    F = seg.functional
    m = _blob()
    assert set(np.unique(m)) == {0, 1, 2, 7}
    for conn in CONNS:
        check(F, m, conn, "blob of 1, 2, 7", 1)
    out, stats = F.filter_components(_dev(m), keep_largest=1)
    assert np.array_equal(out.cpu().numpy(), m) and stats == {"components": 1, "kept": 1, "voxels_removed": 0, "largest": int((m != 0).sum())}
    # the reference's [C=1, D, H, W] and [1, 1, D, H, W] are accepted, and the filtered mask keeps the shape
    l3 = F.connected_components(_dev(m))[0]
    assert torch.equal(F.connected_components(_dev(m)[None, None])[0], l3)
    assert F.filter_components(_dev(m)[None], min_voxels=3)[0].shape == (1,) + m.shape


def test_labelling_is_bitwise_reproducible(seg):
    F = seg.functional
    m = _dev(bernoulli((128, 128, 128), 0.31, 5))
    for conn in CONNS:
        a, b = F.connected_components(m, conn), F.connected_components(m, conn)
        assert all(torch.equal(u, v) for u, v in zip(a, b)), conn


# ---------------------------------------------------------------------------------------------------------------- filter
def _check_filter(F, o, mask, conn, min_voxels, keep_largest, **kw):
    want, stats = o.filtered(min_voxels, keep_largest)
    got, got_stats = F.filter_components(mask, min_voxels=min_voxels, keep_largest=keep_largest, connectivity=conn, **kw)
    tag = f"connectivity {conn} min_voxels {min_voxels} keep_largest {keep_largest}"
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), tag
    assert got_stats == stats and all(isinstance(v, int) for v in got_stats.values()), (tag, got_stats, stats)
    return got


@pytest.mark.parametrize("conn,density", [(26, 0.31), (6, 0.10), (18, 0.31)])
def test_filter_components_equals_numpy_on_scipy_labels(seg, conn, density):
    F = seg.functional
    rng = np.random.default_rng(3)
    m = bernoulli((40, 48, 72), density, 11) * rng.choice([1, 2, 7], size=(40, 48, 72))
    o = Oracle(m, conn)
    ranked = np.sort(o.counts)[::-1]
    assert o.n >= 17 and ranked[2] > 1
    d = _dev(m)
    for mv in (1, 2, int(ranked[2]), int(ranked[0]) + 1):
        _check_filter(F, o, d, conn, mv, 0)
    for k in (1, 2, 16):
        _check_filter(F, o, d, conn, 0, k)
        _check_filter(F, o, d, conn, 2, k)
        _check_filter(F, o, d, conn, int(ranked[2]), k)             # fewer than 16 remain
        _check_filter(F, o, d, conn, int(ranked[0]) + 1, k)         # nothing remains: an empty keep list removes everything
    assert torch.equal(d.cpu(), torch.from_numpy(m)), "the input was written to"
    # both thresholds at zero: the input, unchanged, and the stats still filled
    same, stats = F.filter_components(d, connectivity=conn)
    assert torch.equal(same, d) and stats == o.filtered(0, 0)[1]
    # in place: out aliases mask
    alias = d.clone()
    got = _check_filter(F, o, alias, conn, 2, 2, inplace=True)
    assert got.data_ptr() == alias.data_ptr()


@pytest.mark.parametrize("shape,conn,density", [((65, 64, 65), 26, 0.31), ((130, 180, 180), 6, 0.10)], ids=["65x64x65", "130x180x180"])
def test_statistics_and_filter_past_one_trip_of_the_finalize_and_past_the_grid_cap(seg, shape, conn, density):
    """the statistics pass runs ceil(voxels / 1024) blocks, at most 4096: 265 blocks (the finalize's second trip over the partials is
    ragged) and 4114 -> 4096 (the grid-stride walk makes a ragged second trip); the filter's removed count, one block per 512
    voxels, runs 529 blocks and 8227 -> 4096.  The one-block regime is in SHAPES."""
    m = bernoulli(shape, density, 7)
    o = check(seg.functional, m, conn, f"bernoulli {density}")
    _check_filter(seg.functional, o, _dev(m), conn, 3, 0)
    _check_filter(seg.functional, o, _dev(m), conn, 0, 2)


def test_filter_entry_point_with_out_aliasing_mask_and_odd_alignment(seg):
    """the C entry point itself: out == mask, and a mask that starts 8 bytes off a 16-byte boundary (the scalar path)"""
    F = seg.functional
    L = seg.lib()
    m = bernoulli((17, 33, 65), 0.31, 2) * 7
    o = Oracle(m, 26)
    want, stats = o.filtered(3, 0)
    labels, sizes, _ = F.connected_components(_dev(m), 26)
    st = torch.cuda.current_stream().cuda_stream
    removed = torch.empty(1, dtype=torch.int64, device="cuda")
    for shift in (0, 1):
        buf = torch.zeros(m.size + 2, dtype=torch.int64, device="cuda")
        view = buf[shift:shift + m.size]
        view.copy_(_dev(m).reshape(-1))
        L.call("mi355seg_components_filter_i64", view.data_ptr(), labels.data_ptr(), sizes.data_ptr(), m.size, 3, None, 0,
               view.data_ptr(), removed.data_ptr(), st)
        assert np.array_equal(view.cpu().numpy().reshape(m.shape), want) and removed.item() == stats["voxels_removed"], shift
        assert int(buf[:shift].abs().sum()) == 0 and int(buf[shift + m.size:].abs().sum()) == 0, "wrote outside the volume"


def test_equal_largest_components_the_first_in_raster_order_survives(seg):
    F = seg.functional
    m = np.zeros((12, 20, 70), dtype=np.int64)
    m[1:4, 2:6, 60:68] = 2             # starts first in raster order (smaller z), although further along x
    m[6:9, 10:14, 1:9] = 1
    m[10, 18, 30:33] = 1
    for conn in CONNS:
        o = check(F, m, conn, "equal blocks", 3)
        assert o.info()[2] == 96 and o.info()[3] == int(np.ravel_multi_index((1, 2, 60), m.shape)) + 1
        got = _check_filter(F, o, _dev(m), conn, 0, 1).cpu().numpy()
        assert got[1:4, 2:6, 60:68].min() == 2 and got.sum() == 2 * 96
        _check_filter(F, o, _dev(m), conn, 0, 2)


# ---------------------------------------------------------------------------------------------------------------- surface
def test_refusals_launch_nothing(seg):
    F = seg.functional
    v = torch.zeros((4, 5, 6), dtype=torch.int64, device="cuda")
    for bad in (v.float(), v.cpu(), v[0]):
        with pytest.raises(seg.Mi355SegError):
            F.connected_components(bad)
        with pytest.raises(seg.Mi355SegError):
            F.filter_components(bad, keep_largest=1)
    with pytest.raises(seg.Mi355SegError, match="7"):
        F.connected_components(v, 7)
    with pytest.raises(seg.Mi355SegError, match="7"):
        F.filter_components(v, min_voxels=1, connectivity=7)
    with pytest.raises(seg.Mi355SegError, match="17"):
        F.filter_components(v, keep_largest=17)
    with pytest.raises(seg.Mi355SegError):
        F.filter_components(v, min_voxels=-1)


def test_custom_op_equals_functional(seg):
    from mi355seg import custom_ops  # noqa: F401
    F = seg.functional
    m = _dev(bernoulli((17, 33, 65), 0.31, 4))
    for conn in CONNS:
        a, b = torch.ops.mi355seg.connected_components(m, conn), F.connected_components(m, conn)
        assert len(a) == 3 and all(torch.equal(u, v) for u, v in zip(a, b))
    assert all(torch.equal(u, v) for u, v in zip(torch.ops.mi355seg.connected_components(m), F.connected_components(m, 26)))
    meta = torch.empty((1, 4, 5, 6), dtype=torch.int64, device="meta")
    lab, sizes, info = torch.ops.mi355seg.connected_components(meta)
    assert lab.shape == (4, 5, 6) and lab.dtype == torch.int32 and sizes.shape == (120,) and sizes.dtype == torch.int32
    assert info.shape == (4,) and info.dtype == torch.int64


def test_predict_cli_with_keep_largest_cleans_the_saved_mask_and_the_metrics(seg, tmp_path):
    from mi355seg.predict import main as predict_main
    from mi355seg.train import main as train_main
    from mi355seg.utils.metric import metric_with_spacing
    from test_hd95_fixture import COLUMNS
    out = str(tmp_path / "logs")
    common = ["config=unet", f"config.output_dir={out}", "config.patch_size=32,32,32", "config.batch_size=2"]
    cfg, _ = train_main(common + ["config.iters_per_epoch=2", "config.epochs=1"])
    ckpt = os.path.join(cfg.hydra_path, "latest_checkpoint.pt")
    cfg_a, rows_a = predict_main(common + [f"config.ckpt={ckpt}", f"config.hydra_path={tmp_path / 'plain'}"])
    cfg_b, rows_b = predict_main(common + [f"config.ckpt={ckpt}", f"config.hydra_path={tmp_path / 'clean'}", "config.keep_largest=1",
                                           "config.connectivity=26", "config.spacing=1,1,1"])
    assert not os.path.exists(os.path.join(cfg_a.hydra_path, "components.csv"))
    assert sorted(os.listdir(cfg_a.hydra_path)) == sorted(["metrics.csv"] + [r["file"] + "_pred.npy" for r in rows_a])
    with open(os.path.join(cfg_a.hydra_path, "metrics.csv"), newline="") as fh:
        assert list(csv.reader(fh))[0] == ["file", "jaccard", "dice"]
    with open(os.path.join(cfg_b.hydra_path, "components.csv"), newline="") as fh:
        comp = list(csv.DictReader(fh))
    with open(os.path.join(cfg_b.hydra_path, "metrics.csv"), newline="") as fh:
        spaced = list(csv.reader(fh))
    assert len(comp) == len(rows_b) == len(rows_a) == 2 and list(comp[0]) == ["file", "components", "kept", "voxels_removed", "largest"]
    assert spaced[0] == ["file"] + COLUMNS and len(spaced) == 4 and spaced[3][0] == "mean"
    # the ground truth of predict.py's synthetic cases
    g = torch.Generator().manual_seed(7)
    size = tuple(2 * p for p in (32, 32, 32))
    gts = []
    for _ in range(2):
        torch.randn((cfg_b.in_classes,) + size, generator=g)
        gts.append((torch.rand((1,) + size, generator=g) > 0.9).to(torch.int64))
    for ra, rb, rc, gt, line in zip(rows_a, rows_b, comp, gts, spaced[1:3]):
        assert ra["file"] == rb["file"] == rc["file"] == line[0]
        plain = np.load(os.path.join(cfg_a.hydra_path, ra["file"] + "_pred.npy"))
        clean = np.load(os.path.join(cfg_b.hydra_path, rb["file"] + "_pred.npy"))
        o = Oracle(plain.reshape(size), 26)
        want, stats = o.filtered(0, 1)
        print(f"{ra['file']}: {stats}")
        assert clean.dtype == plain.dtype and np.array_equal(clean.reshape(size), want)
        assert ndimage.label(clean.reshape(size) != 0, _structure(26))[1] == min(1, o.n)
        assert {k: int(rc[k]) for k in stats} == stats and int(rc["kept"]) == min(1, o.n)
        again = metric_with_spacing(gt.cuda(), torch.from_numpy(clean.astype(np.int64)).cuda(), (1.0, 1.0, 1.0))
        for k, v, cell in zip(COLUMNS, again, line[1:]):
            assert rb[k] == v or (np.isnan(rb[k]) and np.isnan(v)), (k, rb[k], v)
            assert float(cell) == v or (np.isnan(float(cell)) and np.isnan(v)), (k, cell, v)
