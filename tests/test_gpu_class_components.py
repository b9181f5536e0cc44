"""Per-class connected components on the device (csrc/components.hip) against scipy.ndimage.label of every class
mask ``m == k`` with generate_binary_structure(3, 1 / 2 / 3).  Everything is exact: the canonical label (1 + raster index of the
component's first voxel) and the consecutive label (rank of the first voxel over all classes) leave no freedom.  Structures that
must join or stay apart are placed from the tile shape the library reports.  A random case first shows on the oracle's side that
the per-class partition differs from the binary one, so it cannot pass on the binary kernel."""
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
ids = lambda s: "x".join(map(str, s))


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
    """the components of every class by scipy, ranked by first voxel over all classes: first / counts / cls [n], the canonical
    labels (first + 1) and the consecutive ones (rank + 1) as volumes, and the component count of the binary mask ``m != 0``"""

    def __init__(self, mask, conn):
        self.mask = mask = np.asarray(mask)
        lin = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
        first, counts, cls = [], [], []
        self.canonical = np.zeros(mask.shape, dtype=np.int64)
        for k in np.unique(mask):
            if not 1 <= k <= 255:
                continue
            ref, n = ndimage.label(mask == k, _structure(conn))
            f = np.asarray(ndimage.minimum(lin, ref, np.arange(1, n + 1)), dtype=np.int64).reshape(-1)
            first.append(f)
            counts.append(np.bincount(ref.ravel(), minlength=n + 1)[1:].astype(np.int64))
            cls.append(np.full(n, k, dtype=np.int64))
            self.canonical[ref > 0] = f[ref[ref > 0] - 1] + 1
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
        first, counts, cls = cat(first), cat(counts), cat(cls)
        order = np.argsort(first, kind="stable")
        self.first, self.counts, self.cls, self.n = first[order], counts[order], cls[order], len(order)
        rank = np.zeros(mask.size + 1, dtype=np.int64)
        rank[self.first + 1] = np.arange(1, self.n + 1)
        self.consecutive = rank[self.canonical]
        self.n_binary = ndimage.label(mask != 0, _structure(conn))[1]

    def info(self):
        if self.n == 0:
            return [0, 0, 0, 0]
        top = int(self.counts.max())
        return [int(self.counts.sum()), self.n, top, int(self.first[self.counts == top].min()) + 1]

    def keep(self, min_voxels, keep_largest):
        get = lambda arg, k: arg.get(int(k), 0) if isinstance(arg, dict) else arg
        keep = np.zeros(self.n, dtype=bool)
        for k in np.unique(self.cls):
            mine = np.flatnonzero((self.cls == k) & (self.counts >= get(min_voxels, k)))
            if get(keep_largest, k) > 0:
                mine = mine[np.argsort(-self.counts[mine], kind="stable")][:get(keep_largest, k)]      # equal sizes: the smaller rank
            keep[mine] = True
        return keep

    def filtered(self, min_voxels, keep_largest):
        """(mask after the clean-up, stats per class) by numpy"""
        keep = self.keep(min_voxels, keep_largest)
        out = np.where(np.concatenate([[True], keep])[self.consecutive], self.mask, 0)
        named = {k for arg in (min_voxels, keep_largest) if isinstance(arg, dict) for k in arg}
        stats = {}
        for k in sorted(set(self.cls.tolist()) | named):
            mine = self.cls == k
            stats[k] = {"components": int(mine.sum()), "kept": int((mine & keep).sum()),
                        "voxels_removed": int(self.counts[mine & ~keep].sum()), "largest": int(self.counts[mine].max()) if mine.any() else 0}
        return out, stats


def check(F, mask, conn, what="", expect=None, differs=False):
    """labels, sizes, info and the table of the class-aware labelling against the oracle; ``differs``: the case is no binary one"""
    mask = np.asarray(mask)
    o = Oracle(mask, conn)
    tag = f"{what} {mask.shape} connectivity {conn}"
    if expect is not None:
        assert o.n == expect, f"{tag}: scipy itself finds {o.n} components, the case expects {expect}"
    if differs:
        assert o.n != o.n_binary, f"{tag}: {o.n} components per class and as many of the binary mask: the case shows nothing"
    d = _dev(mask)
    labels, sizes, info = F.connected_components_by_class(d, conn)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == mask.shape and sizes.dtype == torch.int32 and sizes.shape == (mask.size,)
    assert info.dtype == torch.int64 and info.shape == (8,)
    assert np.array_equal(labels.cpu().numpy(), o.canonical), tag
    want = np.zeros(mask.size, dtype=np.int64)
    want[o.first] = o.counts
    assert np.array_equal(sizes.cpu().numpy(), want), tag
    assert info.tolist() == o.info() + [0, 0, 0, 0], tag
    lc, first, size, cls = F.component_table(d, labels, sizes, info)
    assert lc.dtype == first.dtype == size.dtype == torch.int32 and cls.dtype == torch.int64 and tuple(lc.shape) == mask.shape
    assert first.shape == size.shape == cls.shape == (o.n,)
    f = first.cpu().numpy()
    assert np.all(np.diff(f) > 0), tag
    assert np.array_equal(f, o.first) and np.array_equal(size.cpu().numpy(), o.counts) and np.array_equal(cls.cpu().numpy(), o.cls), tag
    assert np.array_equal(lc.cpu().numpy(), o.consecutive), tag
    return o


def speckle(shape, classes, density, seed):
    rng = np.random.default_rng(seed)
    return ((rng.random(shape) < density) * rng.integers(1, classes + 1, shape)).astype(np.int64)


def smooth_map(shape, classes, seed, sigma=4.0):
    """argmax of classes + 1 smoothed random fields: field 0 is the background, a few large components per class"""
    rng = np.random.default_rng(seed)
    fields = np.stack([ndimage.gaussian_filter(rng.standard_normal(shape), sigma) for _ in range(classes + 1)])
    return fields.argmax(0).astype(np.int64)


def paint(shape, voxels):
    m = np.zeros(shape, dtype=np.int64)
    for v, k in voxels:
        m[v] = k
    return m


# ---------------------------------------------------------------------------------------------------------------- labelling
@pytest.mark.parametrize("classes", (2, 3, 4, 16))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_class_speckle(seg, shape, classes):
    """(seed 9: the first for which every case, the single row of 70 included, differs from the binary partition; one voxel cannot)"""
    for density, conn in itertools.product((0.10, 0.31, 0.90), CONNS):
        check(seg.functional, speckle(shape, classes, density, 9), conn, f"speckle {classes} classes {density}", differs=np.prod(shape) > 1)


@pytest.mark.parametrize("conn", CONNS)
def test_class_speckle_at_128_cubed(seg, conn):
    o = check(seg.functional, speckle((128, 128, 128), 4, 0.31, 5), conn, "speckle 4 classes 0.31", differs=True)
    print(f"speckle 128^3 connectivity {conn}: {o.n} components per class, {o.n_binary} binary")


def test_past_the_grid_cap_and_one_trip_of_the_scan(seg):
    """(130, 180, 180): 4,212,000 voxels are 4,114 blocks of the streaming passes -> the cap of 4,096, whose counts the one-block scan
    takes in 16 trips of 256; the chunks of the rank passes are ragged"""
    o = check(seg.functional, speckle((130, 180, 180), 3, 0.10, 7), 6, "speckle 3 classes 0.10", differs=True)
    assert o.n > 4096


@pytest.mark.parametrize("shape", [(40, 48, 72), (128, 128, 128)], ids=ids)
def test_smooth_class_map(seg, shape):
    tile = seg.functional.components_tile()
    m = smooth_map(shape, 4, 3)
    assert set(np.unique(m)) == {0, 1, 2, 3, 4}
    for conn in CONNS if shape[0] < 100 else (26,):
        o = check(seg.functional, m, conn, "smooth map", differs=True)
        assert o.counts.max() > 4 * np.prod(tile) or shape[0] < 100, "no component spans many tiles"


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_regular_patterns(seg, shape):
    F = seg.functional
    z, y, x = np.indices(shape)
    for conn in CONNS:
        check(F, np.zeros(shape, np.int64), conn, "zeros", 0)                      # n = 0: empty tables
        check(F, np.full(shape, 255, np.int64), conn, "all 255", 1)
        # two classes alternating voxel by voxel along x: runs of length 1, run starts at lanes 0 and 63 and at the tile border
        check(F, (x % 2 + 1).astype(np.int64), conn, "alternating along x", shape[2], differs=shape[2] > 1)
        board = ((z + y + x) % 2 + 1).astype(np.int64)
        big = min(shape) >= 3
        o = check(F, board, conn, "checkerboard", board.size if conn == 6 else (2 if big else None), differs=board.size > 1)
        assert o.n_binary == 1


def _trap_positions(tile, offset):
    """p such that the pair (p, p + offset) lies inside the first tile, or crosses the first interior tile border on any subset of
    the axes along which the offset moves: inside, every face, every edge, the corner"""
    moving = [a for a in range(3) if offset[a]]
    for crossing in itertools.chain.from_iterable(itertools.combinations(moving, r) for r in range(len(moving) + 1)):
        yield tuple((tile[a] - 1 if offset[a] > 0 else tile[a]) if a in crossing else 3 for a in range(3)), crossing


def test_a_diagonal_neighbour_behind_a_voxel_of_another_class(seg):
    """q = p + o with o a backward edge or corner offset that moves along x, both of class 1; the voxels straight across in the other
    one's row, (p_z, p_y, q_x) and (q_z, q_y, p_x), are of class 2.  p and q join under 18 (edges) / 26, never under 6; the binary
    mask has fewer components throughout."""
    F = seg.functional
    tile = F.components_tile()
    shape = tuple(2 * t for t in tile)
    offsets = [o for o in itertools.product((-1, 0, 1), repeat=3) if o > (0, 0, 0) and o[2] != 0 and (o[0], o[1]) != (0, 0)]
    assert len(offsets) == 8
    seen = set()
    for o in offsets:
        for p, crossing in _trap_positions(tile, o):
            q = tuple(a + d for a, d in zip(p, o))
            assert all((a // t != b // t) == (i in crossing) for i, (a, b, t) in enumerate(zip(p, q, tile)))
            seen.add(crossing)
            mask = paint(shape, [(p, 1), (q, 1), ((p[0], p[1], q[2]), 2), ((q[0], q[1], p[2]), 2)])
            steps = sum(1 for d in o if d)
            for conn in CONNS:
                joined = steps <= {6: 1, 18: 2, 26: 3}[conn]
                oc = check(F, mask, conn, f"diagonal trap {o} at {p}", 2 if joined else 4)
                assert oc.n_binary < oc.n                    # (p and q hang together through the voxels of class 2)
    assert seen == {(), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)}


def test_the_left_pair_is_of_another_class(seg):
    """t and the voxel across are of class 1, their left neighbours of class 2: the union of t may not be left to the pair on its
    left.  Rows one face step apart (all connectivities) and one edge step apart (18, 26); inside a tile, across its z and y borders;
    t at lane 1, inside a row, at lane 63 and at lane 0 of the next tile."""
    F = seg.functional
    tile = F.components_tile()
    shape = (2 * tile[0], 2 * tile[1], 2 * tile[2])
    for dz, dy in ((0, 1), (1, 0), (1, 1), (1, -1)):
        for z, y in ((3, 3), (tile[0] - 1 if dz else 3, 3), (3, tile[1] - 1 if dy > 0 else tile[1]), (tile[0] - 1, tile[1] - 1 if dy >= 0 else tile[1])):
            for x in (1, 20, tile[2] - 1, tile[2]):
                a, t = (z, y, x), (z + dz, y + dy, x)
                mask = paint(shape, [(a, 1), (t, 1), ((a[0], a[1], x - 1), 2), ((t[0], t[1], x - 1), 2)])
                for conn in CONNS:
                    joined = conn != 6 or abs(dz) + abs(dy) == 1
                    check(F, mask, conn, f"skip trap rows ({dz}, {dy}) at {a}", 2 if joined else 4)


def test_a_core_inside_a_closed_shell_of_another_class(seg):
    F = seg.functional
    tile = F.components_tile()
    m = np.zeros((2 * tile[0] + 3, 2 * tile[1] + 3, tile[2] + 30), dtype=np.int64)
    m[2:-2, 2:-2, 40:-5] = 1
    m[3:-3, 3:-3, 41:-6] = 2
    for conn in CONNS:
        o = check(F, m, conn, "core in shell", 2)
        assert o.n_binary == 1


def test_a_binary_mask_gives_the_binary_labelling_and_scipys_numbering(seg):
    F = seg.functional
    for shape, density in (((3, 5, 7), 0.5), ((17, 33, 65), 0.31), ((40, 48, 72), 0.10), ((40, 48, 72), 0.90)):
        m = (np.random.default_rng(2).random(shape) < density).astype(np.int64)
        d = _dev(m)
        for conn in CONNS:
            a, b = F.connected_components_by_class(d, conn), F.connected_components(d, conn)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2][:4], b[2]), (shape, conn)
            ref, n = ndimage.label(m, _structure(conn))
            for lab, sizes, info in (a, b):                  # the table works for the binary labelling too
                lc, first, size, cls = F.component_table(d, lab, sizes, info)
                assert np.array_equal(lc.cpu().numpy(), ref) and first.numel() == n and bool((cls == 1).all()), (shape, conn)
                assert np.array_equal(size.cpu().numpy(), np.bincount(ref.ravel())[1:])
    m7 = _dev(np.full((3, 5, 7), 7))                         # binary labelling of any value: cls is whatever sits at the root
    assert F.component_table(m7, *F.connected_components(m7))[3].tolist() == [7]


def test_labelling_is_bitwise_reproducible(seg):
    F = seg.functional
    m = _dev(speckle((128, 128, 128), 4, 0.31, 5))
    for conn in CONNS:
        a, b = F.connected_components_by_class(m, conn), F.connected_components_by_class(m, conn)
        assert all(torch.equal(u, v) for u, v in zip(a, b)), conn
        ta, tb = F.component_table(m, *a), F.component_table(m, *b)
        assert all(torch.equal(u, v) for u, v in zip(ta, tb)), conn


def test_values_outside_0_to_255_raise_and_are_counted(seg):
    F, L = seg.functional, seg.lib()
    shape = (17, 33, 65)
    m = speckle(shape, 3, 0.31, 4)
    m[0, 0, 0], m[5, 7, 64], m[16, 32, 3], m[9, 9, 9] = 256, -1, 2 ** 40 + 1, -(2 ** 62)
    d = _dev(m)
    with pytest.raises(seg.Mi355SegError, match="4 voxels hold values outside 0..255"):
        F.connected_components_by_class(d)
    with pytest.raises(seg.Mi355SegError, match="outside 0..255"):
        F.filter_components_by_class(d, keep_largest=1)
    # the entry point itself: the count in info[4], such voxels background in labels and sizes
    labels = torch.empty(shape, dtype=torch.int32, device="cuda")
    sizes = torch.empty(m.size, dtype=torch.int32, device="cuda")
    info = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    ws = torch.empty(L.query("mi355seg_components_classes_ws_bytes", *shape), dtype=torch.uint8, device="cuda")
    L.call("mi355seg_components_label_classes_i64", d.data_ptr(), *shape, 26, labels.data_ptr(), sizes.data_ptr(), info.data_ptr(),
           ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    o = Oracle(np.where((m < 0) | (m > 255), 0, m), 26)
    assert info.tolist() == o.info() + [4, 0, 0, 0]
    assert np.array_equal(labels.cpu().numpy(), o.canonical)


# ---------------------------------------------------------------------------------------------------------------- filter
def _check_filter(F, o, d, conn, min_voxels, keep_largest, **kw):
    want, stats = o.filtered(min_voxels, keep_largest)
    got, got_stats = F.filter_components_by_class(d, min_voxels=min_voxels, keep_largest=keep_largest, connectivity=conn, **kw)
    tag = f"connectivity {conn} min_voxels {min_voxels} keep_largest {keep_largest}"
    g = got.cpu().numpy()
    assert got.dtype == torch.int64 and np.array_equal(g, want), tag
    assert np.array_equal(g[g != 0], o.mask[g != 0]), tag                      # kept voxels keep their class value
    assert got_stats == stats and all(isinstance(v, int) for s in got_stats.values() for v in s.values()), (tag, got_stats, stats)
    return got


FILTER_ARGS = [(2, 0), (0, 1), (0, 2), (3, 16), ({1: 2, 3: 50}, 0), (0, {1: 1, 2: 2}), ({2: 3}, {1: 1, 3: 16, 9: 1}), (10 ** 6, 0), (0, {2: 0})]


@pytest.mark.parametrize("conn,density", [(26, 0.31), (6, 0.10), (18, 0.31)])
def test_filter_equals_numpy_on_the_oracle(seg, conn, density):
    F = seg.functional
    m = speckle((40, 48, 72), 3, density, 11)
    o = Oracle(m, conn)
    assert o.n >= 17 and o.n != o.n_binary
    d = _dev(m)
    for mv, top in FILTER_ARGS:
        _check_filter(F, o, d, conn, mv, top)
    assert torch.equal(d.cpu(), torch.from_numpy(m)), "the input was written to"
    same, stats = F.filter_components_by_class(d, connectivity=conn)            # both thresholds at zero: the input itself
    assert same is d and stats == o.filtered(0, 0)[1]
    alias = d.clone()
    got = _check_filter(F, o, alias, conn, 2, {1: 2, 2: 1}, inplace=True)       # in place: out aliases mask
    assert got.data_ptr() == alias.data_ptr()
    empty, stats = F.filter_components_by_class(torch.zeros_like(d), keep_largest={2: 1})
    assert int(empty.abs().sum()) == 0 and stats == {2: {"components": 0, "kept": 0, "voxels_removed": 0, "largest": 0}}


@pytest.mark.parametrize("shape", [(17, 33, 65), (130, 180, 180)], ids=ids)
def test_filter_by_table_removed_aliasing_alignment_and_odd_numel(seg, shape):
    """the pieces by hand: `removed` of the filter equals the sum of the per-class voxels_removed; the C entry point with out == mask
    and a mask 8 bytes off a 16-byte boundary (the scalar path); 17 * 33 * 65 is odd (the pair path's last voxel); the large shape
    takes the filter past its grid cap"""
    F, L = seg.functional, seg.lib()
    conn = 26 if shape[0] < 100 else 6
    m = speckle(shape, 3, 0.31 if shape[0] < 100 else 0.10, 2)
    o = Oracle(m, conn)
    d = _dev(m)
    labels, sizes, info = F.connected_components_by_class(d, conn)
    lc, first, size, cls = F.component_table(d, labels, sizes, info)
    for mv, top in ((3, 0), (0, {1: 1, 2: 2})):
        want, stats = o.filtered(mv, top)
        keep = F.select_components_by_class(cls, size, mv, top)
        assert np.array_equal(keep.cpu().numpy(), o.keep(mv, top))
        assert F.class_component_stats(cls, size, keep, top if isinstance(top, dict) else ()) == stats
        out, removed = F.filter_by_component_table(d, lc, keep)
        assert np.array_equal(out.cpu().numpy(), want)
        assert removed.item() == sum(s["voxels_removed"] for s in stats.values()) == int((m != 0).sum() - (want != 0).sum())
        flags = keep.to(torch.uint8)
        rem = torch.empty(1, dtype=torch.int64, device="cuda")
        for shift in (0, 1):
            buf = torch.zeros(m.size + 2, dtype=torch.int64, device="cuda")
            view = buf[shift:shift + m.size]
            view.copy_(d.reshape(-1))
            L.call("mi355seg_components_filter_table_i64", view.data_ptr(), lc.data_ptr(), flags.data_ptr(), flags.numel(), m.size,
                   view.data_ptr(), rem.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert np.array_equal(view.cpu().numpy().reshape(shape), want) and rem.item() == removed.item(), shift
            assert int(buf[:shift].abs().sum()) == 0 and int(buf[shift + m.size:].abs().sum()) == 0, "wrote outside the volume"


def test_equal_largest_components_of_a_class_the_first_in_raster_order_survives(seg):
    F = seg.functional
    m = np.zeros((12, 20, 70), dtype=np.int64)
    m[1:4, 2:6, 60:68] = 2             # starts first in raster order (smaller z), although further along x
    m[6:9, 10:14, 1:9] = 2
    m[6:9, 2:6, 20:28] = 1             # class 1: the same, the other way round in x
    m[1:4, 10:14, 30:38] = 1
    m[10, 18, 30:33] = 1
    for conn in CONNS:
        o = check(F, m, conn, "equal blocks", 5)
        got = _check_filter(F, o, _dev(m), conn, 0, 1).cpu().numpy()
        assert got[1:4, 2:6, 60:68].min() == 2 and got[1:4, 10:14, 30:38].min() == 1 and (got != 0).sum() == 2 * 96
        _check_filter(F, o, _dev(m), conn, 0, {2: 1})


# ---------------------------------------------------------------------------------------------------------------- surface
def test_refusals_launch_nothing(seg):
    F = seg.functional
    E = seg.Mi355SegError
    v = torch.zeros((4, 5, 6), dtype=torch.int64, device="cuda")
    for bad in (v.float(), v.cpu(), v[0], v[:0]):
        with pytest.raises(E):
            F.connected_components_by_class(bad)
        with pytest.raises(E):
            F.filter_components_by_class(bad, keep_largest=1)
    with pytest.raises(E, match="7"):
        F.connected_components_by_class(v, 7)
    with pytest.raises(E, match="7"):
        F.filter_components_by_class(v, min_voxels=1, connectivity=7)
    with pytest.raises(E, match="17"):
        F.filter_components_by_class(v, keep_largest={1: 17})
    with pytest.raises(E):
        F.filter_components_by_class(v, min_voxels={1: -1})
    with pytest.raises(E, match="inplace"):
        F.filter_components_by_class(v.transpose(0, 2), keep_largest=1, inplace=True)
    labels, sizes, info = F.connected_components_by_class(v)
    for args in ((v, labels.long(), sizes, info), (v, labels, sizes[:5], info), (v, labels, sizes, info.cpu()), (v, labels, sizes.cpu(), info),
                 (v, labels, sizes, info[:2]), (v.int(), labels, sizes, info)):
        with pytest.raises(E):
            F.component_table(*args)
    lc = F.component_table(v, labels, sizes, info)[0]
    for args in ((v, lc.long(), torch.ones(0, dtype=torch.bool, device="cuda")), (v, lc, torch.ones(1, dtype=torch.int32, device="cuda")),
                 (v, lc[:2], torch.ones(0, dtype=torch.bool, device="cuda")), (v, lc, torch.ones(1, dtype=torch.bool))):
        with pytest.raises(E):
            F.filter_by_component_table(*args)
    L = seg.lib()
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(E, match="aligned"):
        L.call("mi355seg_components_table_i64", v.data_ptr(), labels.data_ptr() + 4, sizes.data_ptr(), 120, 0, lc.data_ptr(), None, None, None,
               ws.data_ptr(), ws.numel(), st)
    with pytest.raises(E, match="null table"):
        L.call("mi355seg_components_table_i64", v.data_ptr(), labels.data_ptr(), sizes.data_ptr(), 120, 3, lc.data_ptr(), None, None, None,
               ws.data_ptr(), ws.numel(), st)
    with pytest.raises(E, match="null keep"):
        L.call("mi355seg_components_filter_table_i64", v.data_ptr(), lc.data_ptr(), None, 2, 120, v.data_ptr(), ws.data_ptr(), st)
    torch.cuda.synchronize()
    assert int(v.abs().sum()) == 0


def test_custom_op_equals_functional(seg):
    from mi355seg import custom_ops
    F = seg.functional
    assert "connected_components_by_class" in custom_ops.OPS
    m = _dev(speckle((17, 33, 65), 3, 0.31, 4))
    for conn in CONNS:
        a, b = torch.ops.mi355seg.connected_components_by_class(m, conn), F.connected_components_by_class(m, conn)
        assert len(a) == 3 and all(torch.equal(u, v) for u, v in zip(a, b))
    assert all(torch.equal(u, v) for u, v in zip(torch.ops.mi355seg.connected_components_by_class(m), F.connected_components_by_class(m, 26)))
    meta = torch.empty((1, 4, 5, 6), dtype=torch.int64, device="meta")
    lab, sizes, info = torch.ops.mi355seg.connected_components_by_class(meta)
    assert lab.shape == (4, 5, 6) and lab.dtype == torch.int32 and sizes.shape == (120,) and sizes.dtype == torch.int32
    assert info.shape == (8,) and info.dtype == torch.int64


def _read_csv(path):
    with open(path, newline="") as fh:
        return list(csv.reader(fh))


class NearestCentre(torch.nn.Module):
    """a stand-in for the network, which is not what this test is about: class k where the normalised intensity is nearest to the
    k-th of K centres -- on a noisy image a speckled multi-class mask around the structures"""

    def __init__(self, K):
        super().__init__()
        self.register_buffer("centres", torch.linspace(-0.5, 2.5, K))

    def forward(self, x):
        return -(x - self.centres.view(1, -1, 1, 1, 1)) ** 2


def test_predict_cli_cleans_every_class(seg, tmp_path, monkeypatch):
    """predict.py's command line on three 32^3 label volumes with noisy images: the saved masks of the run with
    config.class_keep_largest=1 equal the numpy clean-up of the plain run's masks; components.csv and metrics.csv follow them"""
    import mi355seg.predict as predict_module
    from mi355seg.predict import main as predict_main
    monkeypatch.setattr(predict_module, "build_model", lambda config: NearestCentre(int(config.out_classes)))
    os.makedirs(tmp_path / "img"), os.makedirs(tmp_path / "gt")
    rng = np.random.default_rng(3)
    z, y, x = np.meshgrid(*(np.arange(32, dtype=np.float32),) * 3, indexing="ij")
    for i in range(3):
        lab = np.zeros((32, 32, 32), dtype=np.float32)
        for k, c in enumerate((8 + i, 16, 24 - i), start=1):
            lab[(z - 16) ** 2 + (y - 16) ** 2 + (x - c) ** 2 < 16] = k
        np.save(tmp_path / "img" / f"case{i}.npy", (lab + rng.normal(0, 0.4, lab.shape)).astype(np.float32))
        np.save(tmp_path / "gt" / f"case{i}.npy", lab)
    base = ["config=unet", f"config.output_dir={tmp_path / 'logs'}", "config.patch_size=32,32,32", "config.batch_size=1", "config.out_classes=4",
            f"config.pred_data_path={tmp_path / 'img'}", f"config.pred_gt_path={tmp_path / 'gt'}", "config.multiclass=true"]
    cfg_a, rows_a = predict_main(base + [f"config.hydra_path={tmp_path / 'plain'}"])
    cfg_b, rows_b = predict_main(base + [f"config.hydra_path={tmp_path / 'clean'}", "config.class_keep_largest=1"])
    # without the new keys: the files of before
    assert sorted(os.listdir(cfg_a.hydra_path)) == sorted(["metrics.csv"] + [f"case{i}_pred.npy" for i in range(3)])
    assert sorted(os.listdir(cfg_b.hydra_path)) == sorted(["metrics.csv", "components.csv"] + [f"case{i}_pred.npy" for i in range(3)])
    comp, met = _read_csv(os.path.join(cfg_b.hydra_path, "components.csv")), _read_csv(os.path.join(cfg_b.hydra_path, "metrics.csv"))
    assert comp[0] == ["file", "class", "components", "kept", "voxels_removed", "largest"] and len(comp) == 1 + 9
    assert met[0] == ["file", "class", "jaccard", "dice"] and len(met) == 1 + 9 + 3 and len(rows_a) == len(rows_b) == 9
    changed = 0
    plain_met = _read_csv(os.path.join(cfg_a.hydra_path, "metrics.csv"))
    assert plain_met[0] == ["file", "class", "jaccard", "dice"] and len(plain_met) == 1 + 9 + 3
    for i in range(3):
        gt = np.load(tmp_path / "gt" / f"case{i}.npy").astype(np.int64)
        plain = np.load(os.path.join(cfg_a.hydra_path, f"case{i}_pred.npy")).reshape(gt.shape).astype(np.int64)
        # the run without the new keys: the stand-in's argmax, untouched, and its metrics
        img = np.load(tmp_path / "img" / f"case{i}.npy").astype(np.float64)
        zn = (img - img.mean()) / img.std(ddof=1)
        near = np.abs(zn[None] - np.linspace(-0.5, 2.5, 4)[:, None, None, None])
        sure = np.sort(near, 0)[1] - np.sort(near, 0)[0] > 1e-4            # (away from the ties that float32 may break the other way)
        assert np.array_equal(plain[sure], near.argmin(0)[sure]) and sure.mean() > 0.99
        for k in (1, 2, 3):
            tp, ps, gs = float(np.sum((gt == k) & (plain == k))), float(np.sum(plain == k)), float(np.sum(gt == k))
            line, row = plain_met[1 + 3 * i + k - 1], rows_a[3 * i + k - 1]
            assert line[:2] == [f"case{i}", str(k)] and (row["file"], row["class"]) == (f"case{i}", k)
            assert abs(float(line[2]) - tp / (gs + ps - tp + 0.001)) <= 1e-12 and abs(float(line[3]) - 2 * tp / (gs + ps + 0.001)) <= 1e-12
            assert float(line[2]) == row["jaccard"] and float(line[3]) == row["dice"]
        clean = np.load(os.path.join(cfg_b.hydra_path, f"case{i}_pred.npy")).reshape(gt.shape).astype(np.int64)
        want, stats = Oracle(plain, 26).filtered(0, 1)
        print(f"case{i}: {stats}")
        assert np.array_equal(clean, want)
        changed += int((clean != plain).sum())
        for k in (1, 2, 3):
            row = comp[1 + 3 * i + k - 1]
            s = stats.get(k, dict.fromkeys(("components", "kept", "voxels_removed", "largest"), 0))
            assert row[:2] == [f"case{i}", str(k)] and [int(c) for c in row[2:]] == [s["components"], s["kept"], s["voxels_removed"], s["largest"]]
            assert ndimage.label(clean == k, _structure(26))[1] == min(1, s["components"])
            tp, ps, gs = float(np.sum((gt == k) & (clean == k))), float(np.sum(clean == k)), float(np.sum(gt == k))
            line = met[1 + 3 * i + k - 1]
            assert line[:2] == [f"case{i}", str(k)]
            assert abs(float(line[2]) - tp / (gs + ps - tp + 0.001)) <= 1e-12 and abs(float(line[3]) - 2 * tp / (gs + ps + 0.001)) <= 1e-12
    assert changed > 0, "the clean-up had nothing to do: the run shows nothing"
    with pytest.raises(ValueError, match="config.class_keep_largest names class 4"):
        predict_main(base + [f"config.hydra_path={tmp_path / 'bad'}", "config.class_keep_largest=4:1,"])
    with pytest.raises(ValueError, match="config.class_min_voxels needs config.multiclass=true"):
        predict_main(base[:-1] + [f"config.hydra_path={tmp_path / 'bad'}", "config.class_min_voxels=5"])
