"""Patch source for the train loop.  The reference feeds torchio ``Queue`` patches
(dataloader.py:52-67) as batch dicts ``{"source": {"data": x}, "gt": {"data": y}}``; torchio/NIfTI I/O is out
of scope, so this module yields the same dict shape from (a) a device-resident synthetic generator or (b) a
device-resident patch queue over a directory of ``.npy`` volumes (Queue / UniformSampler / ZNormalization semantics of
dataloader.py:52-67,94).  With ``config.aug`` both apply the reference's training augmentation (dataloader.py:69-86) on the
device: parameters drawn on the host per subject visit (``AugmentParams``), one resampling launch per batch.  With
``config.sampler=label`` the queue places its patches as tio.LabelSampler does (imported beside UniformSampler, dataloader.py:19):
picks drawn on the host from per-class counts (``draw_label_picks``), resolved to origins by one select launch per visit."""
import glob
import os

import numpy as np
import torch

from .intensity import (NYUL_PERCENTILES, host_masked, landmarks_from_percentiles, normalize_intensity_host, parse_intensity,
                        refuse_for_training)
from .resample import parse_resample, refuse_for_training as refuse_resample_for_training, resample_host, resample_labels_host


def _require_device(device, what, option="aug=True resamples with the HIP kernels of csrc/augment.hip"):
    if torch.device(device).type != "cuda":
        from ._lib import Mi355SegError
        raise Mi355SegError(f"{what}: {option} and needs an MI355X (cuda/HIP) "
                            f"device, got {device}; there is no CPU fallback in this package")


N_LABEL_CLASSES = 16            # classes 0 .. 15 of a label index; counts[16] is the `bad` bin (include/mi355seg.h)


def parse_label_probabilities(value):
    """``config.label_probabilities`` -> ``None`` or ``{label: weight}``: ``None`` / ``""`` / ``"None"`` give ``None`` (sample in
    proportion to ``label > 0``, torchio's default), a dict passes through (keys and weights converted), the command-line form
    ``"0:0.2,1:0.8"`` is parsed (a trailing comma is allowed: YAML reads a single ``1:1`` as the base-60 number 61, so a single pair is
    written ``1:1,`` or ``{1: 1}``).  A negative or non-finite weight, a label outside 0 .. 15 or an all-zero dict raise ``ValueError``."""
    if value is None or (isinstance(value, str) and value.strip() in ("", "None")):
        return None
    if isinstance(value, dict):
        items = list(value.items())
    elif isinstance(value, str):
        items = []
        for part in value.split(","):
            if not part.strip() and items:                  # a trailing comma: "1:1," (what keeps a single pair a string in YAML)
                continue
            k, sep, w = part.partition(":")
            if not sep or not k.strip() or not w.strip():
                raise ValueError(f"label_probabilities: '{part}' in '{value}' is not label:weight (expected e.g. 0:0.2,1:0.8)")
            items.append((k.strip(), w.strip()))
    else:
        raise ValueError(f"label_probabilities: expected None, a dict or a string 'label:weight,...' such as 0:0.2,1:0.8, got {value!r} "
                         f"(YAML reads a single pair such as 1:1 as a base-60 number: write it with a trailing comma, 1:1, or as {{1: 1}})")
    out = {}
    for k, w in items:
        try:
            kf, wf = float(k), float(w)
        except (TypeError, ValueError):
            raise ValueError(f"label_probabilities: '{k}:{w}' is not label:weight with an integer label and a number") from None
        if kf != int(kf) or not 0 <= int(kf) < N_LABEL_CLASSES:
            raise ValueError(f"label_probabilities: label {k} is outside 0 .. {N_LABEL_CLASSES - 1}")
        if not (wf >= 0.0 and np.isfinite(wf)):
            raise ValueError(f"label_probabilities: the weight {w} of label {k} must be a finite number >= 0")
        if int(kf) in out:
            raise ValueError(f"label_probabilities: label {int(kf)} is given twice")
        out[int(kf)] = wf
    if not any(w > 0.0 for w in out.values()):
        raise ValueError(f"label_probabilities: every weight of {value!r} is zero")
    return out


def draw_label_picks(rng, counts, label_probabilities, n):
    """``n`` picks of tio.LabelSampler from the per-class voxel counts of a subject's region of valid patch centres (UNPINNED, the
    definitions of include/mi355seg.h): ``(classes, ranks)`` as ``np.int64[n]``.  Pure host, needs no GPU and no library.
    Class masses: without ``label_probabilities`` ``M[l] = counts[l]`` for l >= 1 and ``M[0] = 0`` (torchio: probability
    proportional to ``label > 0``); with a dict ``{l: w_l}`` ``M[l] = w_l`` where ``counts[l] > 0`` and 0 elsewhere -- a label
    absent from the region drops out and the rest renormalise, as torchio's cdf normalisation does.  ``sum M == 0`` raises
    ``RuntimeError`` (torchio: empty probability map).  One sample draws ``u = rng.random()`` -- the class is the first whose
    cumulative ``M / sum M`` exceeds u -- and then ``r = rng.integers(0, counts[class])``, in that order and nothing else."""
    counts = np.asarray(counts, dtype=np.int64)[:N_LABEL_CLASSES]
    mass = np.zeros(N_LABEL_CLASSES, dtype=np.float64)
    if label_probabilities is None:
        mass[1:counts.size] = counts[1:]
    else:
        for l, w in label_probabilities.items():
            if 0 <= int(l) < counts.size and counts[int(l)] > 0:
                mass[int(l)] = float(w)
    cum = np.cumsum(mass)
    if not cum[-1] > 0.0:
        raise RuntimeError(f"empty probability map: no voxel of the region of valid patch centres carries a label with a positive "
                           f"probability (label_probabilities={label_probabilities}, region counts {counts.tolist()})")
    cdf = cum / cum[-1]                                     # ends in exactly 1.0 > u
    classes, ranks = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    for i in range(n):
        u = rng.random()
        l = int(np.searchsorted(cdf, u, side="right"))      # the first class with cdf > u; a class of mass 0 never is
        classes[i] = l
        ranks[i] = int(rng.integers(0, counts[l]))
    return classes, ranks


class AugmentParams:
    """UNPINNED restatement of the random parameters of the reference's training transform (dataloader.py:69-86 with
    ``config.aug=True``: ``Compose([RandomBiasField(), ZNormalization(), RandomNoise(), RandomFlip(axes=(0,)), OneOf({RandomAffine(): 0.8,
    RandomElasticDeformation(): 0.2})])``), with torchio's defaults for the five transforms constructed without arguments (torchio is
    absent from the build image and the reference holds no fixture of its data pipeline; tests/test_augment.py checks the properties
    stated here).  One instance belongs to one subject VISIT and is shared by that visit's patches, as torchio transforms the subject
    and then cuts patches.  Spatial axes are (D, H, W) = axes 0, 1, 2 of the volume, n = shape, c = (n - 1) / 2.

    ``bias``   float32[20]: polynomial coefficients ~ U(-0.5, 0.5) of the order-3 bias field, torchio's loop order
    ``sigma``  noise std ~ U(0, 0.25);  ``seed``: key of the counter-based noise generator, an integer in [0, 2^63)
    ``flip``   axis 0 mirrored (probability 0.5);  ``elastic``: OneOf picked the elastic deformation (probability 0.2)
    ``scales`` / ``degrees``  per-axis scale ~ U(0.9, 1.1) and Euler angle ~ U(-10, 10) degrees of an affine visit (else ones / zeros)
    ``cp``     float32 [3,7,7,7] control-point displacements ~ U(-7.5, 7.5) voxels of an elastic visit, the two outermost layers of
               every face zero (locked_borders=2); ``None`` for an affine visit
    ``matrix`` float32 [3,4], output voxel -> source voxel: ``F . (c + diag(1/s) R^T (p - c))`` with ``R = Rz Ry Rx`` (rotations about
               axes 2, 1, 0), no translation, ``F`` the flip ``q0 -> D - 1 - q0`` or the identity; for an elastic visit just ``F``, and the
               B-spline displacement of ``cp`` at p is added to the mapped point.
    The draw order is bias, sigma, seed, flip, OneOf, then the chosen transform's own parameters."""

    def __init__(self, shape, bias, sigma, seed, flip, elastic, scales=(1.0, 1.0, 1.0), degrees=(0.0, 0.0, 0.0), cp=None):
        self.shape = tuple(int(s) for s in shape)
        self.bias = np.ascontiguousarray(bias, dtype=np.float32)
        self.sigma, self.seed, self.flip, self.elastic = float(sigma), int(seed), bool(flip), bool(elastic)
        self.scales = np.asarray(scales, dtype=np.float64)
        self.degrees = np.asarray(degrees, dtype=np.float64)
        self.cp = None if cp is None else np.ascontiguousarray(cp, dtype=np.float32)
        if len(self.shape) != 3 or self.bias.shape != (20,) or (self.elastic and (self.cp is None or self.cp.shape != (3, 7, 7, 7))):
            raise ValueError("AugmentParams: expected a 3D shape, 20 bias coefficients and, for an elastic visit, cp [3,7,7,7]")
        self.matrix = self._matrix()

    @classmethod
    def identity(cls, shape, flip=False):
        """No intensity change beyond the z-normalisation and no resampling beyond the optional flip (tests, debugging)."""
        return cls(shape, np.zeros(20, np.float32), 0.0, 0, flip, False)

    @classmethod
    def draw(cls, rng, shape):
        """One visit's parameters from ``rng`` (a ``np.random.Generator``); needs no GPU."""
        bias = rng.uniform(-0.5, 0.5, 20)
        sigma = rng.uniform(0.0, 0.25)
        seed = int(rng.integers(0, 1 << 63))
        flip = bool(rng.random() < 0.5)
        if rng.random() < 0.8:
            return cls(shape, bias, sigma, seed, flip, False, scales=rng.uniform(0.9, 1.1, 3), degrees=rng.uniform(-10.0, 10.0, 3))
        cp = rng.uniform(-7.5, 7.5, (3, 7, 7, 7))
        locked = np.ones((7, 7, 7), dtype=bool)
        locked[2:5, 2:5, 2:5] = False
        cp[:, locked] = 0.0
        return cls(shape, bias, sigma, seed, flip, True, cp=cp)

    def _matrix(self):
        n = np.asarray(self.shape, dtype=np.float64)
        c = (n - 1.0) / 2.0
        a0, a1, a2 = np.deg2rad(self.degrees)
        r0 = np.array([[1, 0, 0], [0, np.cos(a0), -np.sin(a0)], [0, np.sin(a0), np.cos(a0)]])
        r1 = np.array([[np.cos(a1), 0, np.sin(a1)], [0, 1, 0], [-np.sin(a1), 0, np.cos(a1)]])
        r2 = np.array([[np.cos(a2), -np.sin(a2), 0], [np.sin(a2), np.cos(a2), 0], [0, 0, 1]])
        a = np.diag(1.0 / self.scales) @ (r2 @ r1 @ r0).T
        m = np.concatenate([a, (c - a @ c)[:, None]], axis=1)
        if self.flip:
            m[0] = -m[0]
            m[0, 3] += n[0] - 1.0
        return np.ascontiguousarray(m, dtype=np.float32)


class SyntheticPatches:
    """x ~ N(0,1) (mimics ZNormalization), labels from a thresholded low-frequency field; generated on the
    device so no host->device copy sits in the step.  ``aug=True``: every generated sample is a one-patch subject (volume = patch,
    origin 0) put through the training augmentation of ``AugmentParams`` (dataloader.py:69-86), one sampling launch per batch."""

    def __init__(self, patch_size, in_channels, batch_size, iters, device, seed=1234, n_labels=2, aug=False):
        self.ps = (patch_size,) * 3 if isinstance(patch_size, int) else tuple(patch_size)
        self.cin, self.bs, self.iters, self.device = in_channels, batch_size, iters, device
        self.aug = bool(aug)
        if self.aug:
            _require_device(device, "SyntheticPatches")
            self.rng = np.random.default_rng(seed)
        self.gen = torch.Generator(device=device).manual_seed(seed)
        self.n_labels = n_labels

    def __len__(self):
        return self.iters

    def __iter__(self):
        for _ in range(self.iters):
            x = torch.randn((self.bs, self.cin) + self.ps, generator=self.gen, device=self.device)
            coarse = torch.rand((self.bs, 1) + tuple(max(2, p // 8) for p in self.ps), generator=self.gen, device=self.device)
            field = torch.nn.functional.interpolate(coarse, size=self.ps, mode="trilinear", align_corners=False)
            gt = (field > 0.6).to(torch.float32)
            if self.aug:
                x, gt = self._augment(x, gt)
            yield {"source": {"data": x}, "gt": {"data": gt}}

    def _augment(self, x, gt):
        from . import functional as F
        patches = []
        for xi, yi in zip(x, gt):
            prm = AugmentParams.draw(self.rng, self.ps)
            cp = torch.from_numpy(prm.cp).to(self.device) if prm.elastic else None
            patches.append((xi, yi, F.augment_stats(xi, prm), cp, (0, 0, 0), prm))
        return F.augment_sample(patches, self.ps)


class DevicePatchQueue:
    """UNPINNED restatement of tio.Queue / tio.UniformSampler / tio.ZNormalization semantics (torchio is absent from the build image
    and the reference holds no fixtures for its data pipeline; tests/test_data_queue.py checks the properties stated here).
    The reference's patch pipeline (dataloader.py:52-67: ``tio.Queue(training_set, queue_length=10,
    samples_per_volume=10, UniformSampler(patch_size))`` over ``ZNormalization()``-transformed subjects), kept on the
    device.  Volumes ``<data_path>/*.npy`` (labels ``<gt_path>/<same name>.npy``; [C,D,H,W] or [D,H,W]) are uploaded
    once, z-normalised per volume over all their voxels (mean / unbiased std, tio's ZNormalization without a mask)
    and cached in HBM up to ``cache_gb`` -- 288 GB per MI355X holds whole cohorts -- so a step costs no host I/O and
    no host->device copy.  Queue semantics as torchio's: subjects are visited in a shuffled order, each contributes
    ``samples_per_volume`` uniformly placed patches, the queue is refilled to ``queue_length`` patches and shuffled
    whenever it runs dry, and a batch pops ``batch_size`` patches.

    ``aug=True`` (dataloader.py:69-86, ``config.aug``; UNPINNED like the rest, see ``AugmentParams``): the RAW volumes are cached, every
    subject visit draws one ``AugmentParams`` from the queue's generator (after which its ``samples_per_volume`` origins are drawn as
    before) and has its statistics computed on the device (``functional.augment_stats``), the queue holds patch descriptors instead
    of views, and a batch is one small table upload and one resampling launch (``functional.augment_sample``); ``last_patches`` keeps
    the descriptors of the batch yielded last.  With ``aug=False`` nothing changes.

    ``sampler="label"`` (tio.LabelSampler(patch_size, label_probabilities) in the place of the UniformSampler; UNPINNED, the
    definitions of include/mi355seg.h): a subject's label index is built on the device once (``functional.label_index``, kept in
    ``label_indices`` for subjects that are themselves cached), every visit draws its ``samples_per_volume`` picks on the host
    (``draw_label_picks``: per patch ``u`` then ``r``, nothing else), one select launch turns them into origins
    (``functional.label_pick``), which are copied to the host once and cut as before.  ``label_probabilities``: ``None`` or
    ``{label: weight}`` (``parse_label_probabilities``).  Labels must have one channel and hold integers 0 .. 15 inside the region of
    valid patch centres.  With ``sampler="uniform"`` (the default) nothing changes.

    ``resample`` (a ``resample.ResampleSpec``, ``config.resample_spacing``; tio.Resample, UNPINNED: the definitions of resample.py):
    right after the upload image and labels are resampled from the volume's own spacing (``resample.spacings.of(file)``) to the
    common one on the device (``functional.resample_volume`` at ``resample.order``, ``functional.resample_labels`` with
    ``resample.labels``), once per cached subject; everything above -- the patch-size check, ``aug``, ``intensity``, the z-score and
    both samplers -- then sees the resampled volume.  Refused with ``data_path=synthetic``.  With ``None`` nothing changes."""

    def __init__(self, data_path, gt_path, patch_size, batch_size, iters, device, seed=1234, queue_length=10,
                 samples_per_volume=10, cache_gb=200.0, aug=False, sampler="uniform", label_probabilities=None, intensity=None,
                 resample=None):
        self.aug = bool(aug)
        refuse_for_training(intensity, self.aug, data_path)
        self.intensity = intensity
        refuse_resample_for_training(resample, data_path)
        self.resample = resample                          # a resample.ResampleSpec, or None: the volumes stay on their own grids
        if sampler not in ("uniform", "label"):
            raise ValueError(f"DevicePatchQueue: unknown sampler='{sampler}' (expected 'uniform' or 'label')")
        self.sampler = sampler
        self.label_probabilities = parse_label_probabilities(label_probabilities)
        self.label_indices = {}
        if sampler == "label":
            if self.aug:
                raise NotImplementedError("DevicePatchQueue: sampler='label' with aug=True is not implemented: an augmented visit would "
                                          "have to sample from the RESAMPLED labels; use sampler='uniform' with aug=True")
            _require_device(device, "DevicePatchQueue", "sampler='label' selects patch centres with the HIP kernels of csrc/sampler.hip")
        if self.aug:
            _require_device(device, "DevicePatchQueue")
        self.last_patches = None
        self.files = sorted(glob.glob(os.path.join(data_path, "*.npy")))
        if not self.files:
            raise FileNotFoundError(f"no .npy volumes under {data_path}")
        if self.resample is not None:                     # a volume without a spacing is an error of the run, not of its first visit
            for f in self.files:
                self.resample.spacings.of(f)
        self.gt_path, self.bs, self.iters, self.device = gt_path, batch_size, iters, device
        self.ps = (patch_size,) * 3 if isinstance(patch_size, int) else tuple(patch_size)
        self.queue_length, self.spv = int(queue_length), int(samples_per_volume)
        self.rng = np.random.default_rng(seed)
        self.cache, self.cache_bytes, self.cache_cap = {}, 0, int(cache_gb * (1 << 30))
        self._order, self._queue = [], []

    def __len__(self):
        return self.iters

    def _subject(self, idx):
        """(x, y) of subject ``idx`` on the device, x already z-normalised (the raw volume with ``aug=True``: the normalisation is
        then part of the resampling); cached while the budget lasts."""
        hit = self.cache.get(idx)
        if hit is not None:
            return hit
        f = self.files[idx]
        x = torch.from_numpy(np.ascontiguousarray(np.load(f), dtype=np.float32)).to(self.device)
        y = torch.from_numpy(np.ascontiguousarray(np.load(os.path.join(self.gt_path, os.path.basename(f))), dtype=np.float32)).to(self.device)
        x = x[None] if x.dim() == 3 else x
        y = y[None] if y.dim() == 3 else y
        if self.resample is not None:                     # config.resample_spacing: image and labels to the common grid, once
            rs, sp = self.resample, self.resample.spacings.of(f)
            if x.is_cuda:
                from . import functional as F
                x, y = F.resample_volume(x, sp, rs.target, rs.order), F.resample_labels(y, sp, rs.target, rs.labels)
            else:                                         # CPU plumbing tests only: the same definitions in numpy fp64
                x = torch.from_numpy(resample_host(x.numpy(), sp, rs.target, rs.order))
                y = torch.from_numpy(resample_labels_host(y.numpy(), sp, rs.target, rs.labels))
        if any(s < p for s, p in zip(x.shape[1:], self.ps)):
            how = f" (resampled from spacing {sp} to {rs.target})" if self.resample is not None else ""
            raise ValueError(f"{f}: volume {tuple(x.shape[1:])}{how} is smaller than the patch {self.ps}")
        if self.aug:                                      # raw: bias field, z-normalisation and noise ride in the sampling kernel
            x, y = x.contiguous(), y.contiguous()
        elif self.intensity is not None:                  # config.intensity: percentiles / moments / one map pass (csrc/intensity.hip)
            if x.is_cuda:
                from . import functional as F
                x = F.normalize_intensity(x, self.intensity)
            else:                                         # CPU plumbing tests only: the same definitions in numpy fp64
                x = torch.from_numpy(normalize_intensity_host(x.numpy(), self.intensity))
        elif x.is_cuda:                                   # one fused statistics pass + one apply pass (HIP)
            from . import functional as F
            x = F.znormalize(x)
        else:                                             # CPU plumbing tests only
            x = (x - x.mean()) / x.std()
        nbytes = (x.numel() + y.numel()) * 4
        if self.cache_bytes + nbytes <= self.cache_cap:
            self.cache[idx] = (x, y)
            self.cache_bytes += nbytes
        return x, y

    def _label_index(self, idx, y):
        """the label index of subject ``idx`` (labels ``y``); kept while the subject itself is cached"""
        hit = self.label_indices.get(idx)
        if hit is not None:
            return hit
        from . import functional as F
        from ._lib import Mi355SegError
        if y.shape[0] != 1:
            raise Mi355SegError(f"{self.files[idx]}: sampler='label' needs ONE label channel, got labels {tuple(y.shape)}")
        index = F.label_index(y, self.ps)
        if index.counts[N_LABEL_CLASSES] != 0:
            raise ValueError(f"{self.files[idx]}: sampler='label': {int(index.counts[N_LABEL_CLASSES])} label voxels inside the region of "
                             f"valid patch centres are not integers in 0 .. {N_LABEL_CLASSES - 1}")
        if idx in self.cache:
            self.label_indices[idx] = index
        return index

    def _refill(self):
        while len(self._queue) < self.queue_length:
            if not self._order:
                self._order = list(self.rng.permutation(len(self.files)))
            idx = int(self._order.pop())
            x, y = self._subject(idx)
            if self.sampler == "label":
                from . import functional as F
                index = self._label_index(idx, y)
                try:
                    classes, ranks = draw_label_picks(self.rng, index.counts, self.label_probabilities, self.spv)
                except RuntimeError as e:
                    raise RuntimeError(f"{self.files[idx]}: {e}") from None
                for o in F.label_pick(index, classes, ranks).cpu().numpy():     # the visit's one device-to-host copy
                    sl = (slice(None),) + tuple(slice(int(a), int(a) + p) for a, p in zip(o, self.ps))
                    self._queue.append((x[sl], y[sl]))
                continue
            if self.aug:
                from . import functional as F
                prm = AugmentParams.draw(self.rng, x.shape[1:])
                stats = F.augment_stats(x, prm)
                cp = torch.from_numpy(prm.cp).to(self.device) if prm.elastic else None
                for _ in range(self.spv):
                    o = tuple(int(self.rng.integers(0, s - p + 1)) for s, p in zip(x.shape[1:], self.ps))
                    self._queue.append((x, y, stats, cp, o, prm))
                continue
            for _ in range(self.spv):
                o = [int(self.rng.integers(0, s - p + 1)) for s, p in zip(x.shape[1:], self.ps)]
                sl = (slice(None),) + tuple(slice(a, a + p) for a, p in zip(o, self.ps))
                self._queue.append((x[sl], y[sl]))
        perm = self.rng.permutation(len(self._queue))
        self._queue = [self._queue[i] for i in perm]

    def _iter_augmented(self):
        from . import functional as F
        for _ in range(self.iters):
            patches = []
            for _b in range(self.bs):
                if not self._queue:
                    self._refill()
                patches.append(self._queue.pop())
            self.last_patches = patches
            xb, yb = F.augment_sample(patches, self.ps)
            yield {"source": {"data": xb}, "gt": {"data": yb}}

    def __iter__(self):
        if self.aug:
            yield from self._iter_augmented()
            return
        for _ in range(self.iters):
            xs, ys = [], []
            for _b in range(self.bs):
                if not self._queue:
                    self._refill()
                xp, yp = self._queue.pop()
                xs.append(xp)
                ys.append(yp)
            yield {"source": {"data": torch.stack(xs)}, "gt": {"data": torch.stack(ys)}}


NpyPatches = DevicePatchQueue


def make_loader(config, device, in_channels, seed=1234):
    iters = int(getattr(config, "iters_per_epoch", 4))
    aug = bool(getattr(config, "aug", False))             # conf/config.yaml:27; dataloader.py:69
    sampler = str(getattr(config, "sampler", "uniform"))
    label_probabilities = parse_label_probabilities(getattr(config, "label_probabilities", None))
    intensity = parse_intensity(config)                   # config.intensity and its companions; None: the z-score of today
    refuse_for_training(intensity, aug, config.data_path)
    resample = parse_resample(config)                     # config.resample_spacing and its companions; None: off
    refuse_resample_for_training(resample, config.data_path)
    if str(config.data_path) == "synthetic":
        if sampler != "uniform":
            raise ValueError(f"config.sampler={sampler} needs volumes to sample from: with data_path=synthetic every sample is its own "
                             f"volume (use config.sampler=uniform)")
        return SyntheticPatches(config.patch_size, in_channels, config.batch_size, iters, device, seed, aug=aug)
    return DevicePatchQueue(config.data_path, config.gt_path, config.patch_size, config.batch_size, iters, device, seed,
                            queue_length=int(getattr(config, "queue_length", 10)),
                            samples_per_volume=int(getattr(config, "samples_per_volume", 10)), aug=aug, sampler=sampler,
                            label_probabilities=label_probabilities, intensity=intensity, resample=resample)


def train_landmarks(files, mask="none", device="cuda"):
    """Nyul landmark training for ``config.intensity=histogram`` (tio.HistogramStandardization.train, UNPINNED): per ``.npy`` volume
    the percentiles (1, 10, 20, ..., 90, 99) of its masked voxels (``mask``: ``none``, ``mean`` or a number, as
    ``config.intensity_mask``), rescaled affinely so p[0] -> 0 and p[10] -> 100, averaged over the volumes in fp64 -> float64[11].
    On a cuda device the percentiles come from the radix select (``functional.volume_percentiles``); on ``cpu`` from
    ``np.percentile`` (plumbing tests)."""
    per_volume = []
    for f in files:
        v = np.ascontiguousarray(np.load(f), dtype=np.float32)
        if torch.device(device).type == "cuda":
            from . import functional as F
            x = F.aligned_contiguous(torch.from_numpy(v).to(device))
            per_volume.append(F.volume_percentiles(x, NYUL_PERCENTILES, mask))
        else:
            per_volume.append(np.percentile(host_masked(v, mask, f"train_landmarks {f}"), np.asarray(NYUL_PERCENTILES)))
    return landmarks_from_percentiles(per_volume)
