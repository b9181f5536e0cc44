"""Host side of the training augmentation (dataloader.py:69-86 with config.aug=True; ``mi355seg.data.AugmentParams``,
``DevicePatchQueue(aug=...)``, ``make_loader``): the drawn parameters follow torchio's defaults for RandomBiasField, RandomNoise,
RandomFlip(axes=(0,)), OneOf({RandomAffine: 0.8, RandomElasticDeformation: 0.2}), the draw is seeded, there is no CPU fallback,
and ``aug=False`` leaves the queue as it was.  No GPU needed."""
import math

import numpy as np
import pytest
import torch

import aug_reference as R

SHAPE = (41, 67, 53)


def _write(tmp_path, n=3, shape=(12, 14, 16)):
    (tmp_path / "x").mkdir()
    (tmp_path / "y").mkdir()
    rng = np.random.default_rng(0)
    for i in range(n):
        np.save(tmp_path / "x" / f"v{i}.npy", (rng.normal(size=shape) * (i + 1) + 10 * i).astype(np.float32))
        np.save(tmp_path / "y" / f"v{i}.npy", (np.indices(shape).sum(0) % (i + 2) == 0).astype(np.float32))


def _draws(n, seed=0, shape=SHAPE):
    from mi355seg.data import AugmentParams
    rng = np.random.default_rng(seed)
    return [AugmentParams.draw(rng, shape) for _ in range(n)]


def test_drawn_parameters_lie_in_their_ranges_and_shares():
    ps = _draws(2000)
    n_aff = n_flip = 0
    for p in ps:
        assert p.bias.shape == (20,) and p.bias.dtype == np.float32 and np.all(np.abs(p.bias) <= 0.5)
        assert 0.0 <= p.sigma <= 0.25 and 0 <= p.seed < 1 << 63
        assert p.matrix.shape == (3, 4) and p.matrix.dtype == np.float32 and np.isfinite(p.matrix).all()
        n_flip += p.flip
        if p.elastic:
            assert p.cp.shape == (3, 7, 7, 7) and p.cp.dtype == np.float32 and np.all(np.abs(p.cp) <= 7.5)
            free = np.zeros((7, 7, 7), dtype=bool)
            free[2:5, 2:5, 2:5] = True
            assert np.all(p.cp[:, ~free] == 0.0)                         # locked_borders=2: two layers on every face
            assert np.any(p.cp[:, free] != 0.0)
            assert np.all(p.scales == 1.0) and np.all(p.degrees == 0.0)
        else:
            n_aff += 1
            assert p.cp is None
            assert np.all((p.scales >= 0.9) & (p.scales <= 1.1)) and np.all(np.abs(p.degrees) <= 10.0)
    assert abs(n_aff / 2000 - 0.8) <= 5 * math.sqrt(0.8 * 0.2 / 2000)
    assert abs(n_flip / 2000 - 0.5) <= 5 * math.sqrt(0.25 / 2000)
    sig = np.array([p.sigma for p in ps])
    assert sig.min() < 0.02 and sig.max() > 0.23                        # the whole range is used
    b = np.stack([p.bias for p in ps])
    assert b.min() < -0.45 and b.max() > 0.45


def test_same_seed_same_parameters():
    for a, b in zip(_draws(50, seed=5), _draws(50, seed=5)):
        assert a.seed == b.seed and a.sigma == b.sigma and a.flip == b.flip and a.elastic == b.elastic
        assert np.array_equal(a.bias, b.bias) and np.array_equal(a.matrix, b.matrix)
        assert (a.cp is None and b.cp is None) or np.array_equal(a.cp, b.cp)
    assert any(a.seed != b.seed for a, b in zip(_draws(5, seed=5), _draws(5, seed=6)))


def test_matrix_is_the_stated_map():
    """matrix = F . (c + diag(1/s) R^T (p - c)), R = Rz Ry Rx: the centre is a fixed point (no translation), the linear part has
    the singular values 1/s, and the flip mirrors axis 0 of the result."""
    from mi355seg.data import AugmentParams
    n = np.array(SHAPE, dtype=np.float64)
    c = (n - 1) / 2
    ident = AugmentParams.identity(SHAPE)
    assert np.array_equal(ident.matrix, np.eye(3, 4, dtype=np.float32)) and ident.sigma == 0.0 and not ident.bias.any()
    fl = AugmentParams.identity(SHAPE, flip=True)
    want = np.eye(3, 4)
    want[0, 0], want[0, 3] = -1, SHAPE[0] - 1
    assert np.array_equal(fl.matrix, want.astype(np.float32))
    for p in [q for q in _draws(60, seed=2) if not q.elastic]:
        m = p.matrix.astype(np.float64)
        at_c = m[:, :3] @ c + m[:, 3]
        fixed = c.copy()
        if p.flip:
            fixed[0] = n[0] - 1 - c[0]                                   # == c[0]: the centre is its own mirror image
        assert np.abs(at_c - fixed).max() < 1e-4
        sv = np.linalg.svd(m[:, :3], compute_uv=False)
        assert np.allclose(np.sort(sv), np.sort(1.0 / p.scales), atol=1e-6)
        assert np.sign(np.linalg.det(m[:, :3])) == (-1 if p.flip else 1)
    # a pure rotation about axis 0 by +90 degrees: R = Rx, T(p) = c + R^T (p - c)
    q = AugmentParams((5, 5, 5), np.zeros(20), 0.0, 0, False, False, degrees=(90.0, 0.0, 0.0))
    got = q.matrix.astype(np.float64) @ np.array([2.0, 3.0, 2.0, 1.0])    # p - c = (0, 1, 0)
    assert np.allclose(got, [2.0, 2.0, 1.0], atol=1e-6)                   # R^T (0,1,0) = (0, 0, -1)


def test_reference_restatement_basics():
    """tests/aug_reference.py: the B-spline basis is a partition of unity, locked borders leave a displacement only through the free
    3x3x3 block, the bias field of zero coefficients is one, and the identity coordinates reproduce the window."""
    f = np.linspace(0, 1, 11)
    assert np.allclose(R.bspline(f).sum(0), 1.0)
    assert np.array_equal(R.bias_field(np.zeros(20), (4, 5, 6)), np.ones((4, 5, 6)))
    from mi355seg.data import AugmentParams
    p = AugmentParams.identity((9, 10, 11))
    t = R.coordinates(p, (1, 2, 3), (4, 4, 4))
    assert np.array_equal(t[:, 0, 0, 0], [1, 2, 3]) and np.array_equal(t[:, 3, 3, 3], [4, 5, 6])
    V = np.random.default_rng(0).normal(size=(2, 9, 10, 11))
    img, ins = R.sample_image(V, t, -9.0)
    assert ins.all() and np.array_equal(img, V[:, 1:5, 2:6, 3:7])
    lab, _ = R.sample_label(V, t)
    assert np.array_equal(lab, V[:, 1:5, 2:6, 3:7])
    cp = np.zeros((3, 7, 7, 7))
    cp[0, 3, 3, 3] = 6.0
    d = R.displacement(cp, (9, 10, 11), [np.arange(9.0), np.arange(10.0), np.arange(11.0)])
    assert d[1:].max() == 0.0 and d[0].max() > 0.5 and abs(d[0, 0, 0, 0]) == 0.0


def test_make_loader_forwards_config_aug(tmp_path, monkeypatch):
    import mi355seg
    from mi355seg import data
    from mi355seg.config import Config
    _write(tmp_path)
    seen = {}

    class Spy(data.DevicePatchQueue):
        def __init__(self, *a, **k):
            seen.update(k)
            super().__init__(*a, **{**k, "aug": False})

    monkeypatch.setattr(data, "DevicePatchQueue", Spy)
    cfg = Config(data_path=str(tmp_path / "x"), gt_path=str(tmp_path / "y"), patch_size=8, batch_size=1, aug=True)
    data.make_loader(cfg, "cpu", 1)
    assert seen["aug"] is True
    cfg.aug = False
    data.make_loader(cfg, "cpu", 1)
    assert seen["aug"] is False
    del cfg["aug"]
    data.make_loader(cfg, "cpu", 1)
    assert seen["aug"] is False
    # the synthetic source takes it too -- and refuses a CPU device
    syn = Config(data_path="synthetic", patch_size=8, batch_size=1, aug=True)
    with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):
        data.make_loader(syn, "cpu", 1)
    syn.aug = False
    assert isinstance(data.make_loader(syn, "cpu", 1), data.SyntheticPatches)


def test_aug_on_cpu_raises(tmp_path):
    import mi355seg
    from mi355seg.data import DevicePatchQueue
    _write(tmp_path)
    with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):
        DevicePatchQueue(str(tmp_path / "x"), str(tmp_path / "y"), 8, 1, 2, "cpu", aug=True)


def test_aug_false_is_the_queue_as_it_was(tmp_path):
    """aug=False: the same batches, cache contents and rng consumption as a queue built without the argument."""
    import mi355seg
    from mi355seg.data import DevicePatchQueue
    _write(tmp_path)
    args = (str(tmp_path / "x"), str(tmp_path / "y"), (8, 8, 8), 2, 9, "cpu")
    kw = dict(seed=7, queue_length=6, samples_per_volume=3)
    qa, qb = DevicePatchQueue(*args, **kw), DevicePatchQueue(*args, aug=False, **kw)
    for a, b in zip(list(qa), list(qb)):
        assert torch.equal(a["source"]["data"], b["source"]["data"]) and torch.equal(a["gt"]["data"], b["gt"]["data"])
    assert sorted(qa.cache) == sorted(qb.cache)
    for k in qa.cache:
        assert torch.equal(qa.cache[k][0], qb.cache[k][0]) and torch.equal(qa.cache[k][1], qb.cache[k][1])
    assert qa.rng.integers(0, 1 << 62) == qb.rng.integers(0, 1 << 62)   # both generators stand at the same point of the stream


def test_entry_points_reject_bad_arguments():
    import mi355seg
    L = mi355seg.lib()
    assert L.query("mi355seg_augment_ws_bytes", 1 << 20) > 0
    with pytest.raises(mi355seg.Mi355SegError, match="augment_stats"):
        L.call("mi355seg_augment_stats_f32", None, 1, 8, 8, 8, None, 0.0, 0, None, None, 0, None)
    with pytest.raises(mi355seg.Mi355SegError, match="augment_sample"):
        L.call("mi355seg_augment_sample_f32", None, 0, 1, 1, 8, 8, 8, None, None, None)
    with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):
        from mi355seg.data import AugmentParams
        mi355seg.functional.augment_stats(torch.zeros(1, 8, 8, 8), AugmentParams.identity((8, 8, 8)))
