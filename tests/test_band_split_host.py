"""The IS network's frequency-band split as a low-rank projection (csrc/band.hip, functional.frequency_bands), host side: the basis
builder against the mode table of the reference's own float32 comparison, the fp64 operator assembled from it against the fixtures
the reference's low_pass_torch / high_pass_torch produced (train.py:76-88), the ``impl=`` switch on CPU tensors and the library's
shape query.  No GPU: only the built library is needed."""
import os

import numpy as np
import pytest
import torch

import mi355seg
from mi355seg import functional as F
from mi355seg.models.three_d import IS
from oracle.fill import make_input

# n -> (modes in P, modes in E) at limit 0.04: |fftfreq(n)| < 0.04 and not (> 0.04) in float32; n = 25, 50, 100 have a mode AT the limit
MODES = {8: (1, 1), 12: (1, 1), 16: (1, 1), 25: (1, 3), 32: (3, 3), 50: (3, 5), 64: (5, 5), 96: (7, 7), 100: (7, 9), 128: (11, 11),
         160: (13, 13), 192: (15, 15), 256: (21, 21)}


def fp64_bands(x, limit=0.04):
    """low = P_H X P_W, high = (I - E_H) X (I - E_W) per slice in fp64, after the length-2 forward transform the reference leaves on
    the batch and channel axes (slice 0: x0 + x1, slice 1: x0 - x1)."""
    x = x.detach().cpu().double().numpy()
    if x.shape[0] == 2:
        x = np.stack([x[0] + x[1], x[0] - x[1]])
    if x.shape[1] == 2:
        x = np.stack([x[:, 0] + x[:, 1], x[:, 0] - x[:, 1]], axis=1)
    H, W = x.shape[-2:]
    (eh, rh), (ew, rw) = F.band_basis(H, limit), F.band_basis(W, limit)
    ph, pw = eh[:rh].T @ eh[:rh], ew[:rw].T @ ew[:rw]
    qh, qw = np.eye(H) - eh.T @ eh, np.eye(W) - ew.T @ ew
    return ph @ x @ pw, qh @ x @ qw


@pytest.mark.parametrize("n", sorted(MODES))
def test_band_basis_counts_and_orthonormality(n):
    basis, r = F.band_basis(n, 0.04)
    assert basis.dtype == np.float64 and basis.shape[1] == n
    assert (r, basis.shape[0]) == MODES[n]
    assert np.abs(basis @ basis.T - np.eye(basis.shape[0])).max() < 1e-12


def test_band_basis_rows_are_the_documented_modes():
    """n = 50: P = {0, 1}, E adds k = 2 (2/50 compares equal to 0.04 in float32): rows DC, cos 1, sin 1, cos 2, sin 2."""
    basis, r = F.band_basis(50, 0.04)
    j = np.arange(50)
    want = [np.full(50, 1 / np.sqrt(50))] + [np.sqrt(2 / 50) * f(2 * np.pi * k * j / 50) for k in (1, 2) for f in (np.cos, np.sin)]
    assert r == 3 and np.abs(basis - np.stack(want)).max() < 1e-14
    even, _ = F.band_basis(2, 0.75)                        # 2k = n: the alternating row
    assert np.abs(even - np.array([[1.0, 1.0], [1.0, -1.0]]) / np.sqrt(2)).max() < 1e-15


def test_fp64_operator_reproduces_the_reference_fixtures(golden_dir):
    """Bound 5e-6 (the fp32 FFT's own rounding; measured 7.5e-7).  The `b` case has batch 2: the x0 + x1 / x0 - x1 mix."""
    g = np.load(os.path.join(golden_dir, "ovr_isnet.npz"))
    g32 = np.load(os.path.join(golden_dir, "isnet_f4_32.npz"))
    cases = [(make_input((1, 1, 16, 16, 16), freq=0.37), g["band_low_a"], g["band_high_a"]),
             (make_input((2, 1, 8, 12, 16), freq=0.21), g["band_low_b"], g["band_high_b"]),
             (make_input((1, 1, 32, 32, 32), freq=0.37), g32["low"], g32["high"])]
    for x, low_ref, high_ref in cases:
        low, high = fp64_bands(x)
        assert low.shape == low_ref.shape and high.shape == high_ref.shape
        e_low, e_high = np.abs(low - low_ref).max(), np.abs(high - high_ref).max()
        print(tuple(x.shape), "low", e_low, "high", e_high)
        assert e_low < 5e-6 and e_high < 5e-6


def test_default_impl_is_the_fft_path_bitwise():
    x = make_input((2, 1, 4, 12, 16), freq=0.21)
    low, high = IS.frequency_bands(x)
    low_f, high_f = IS.frequency_bands(x, impl="fft")
    assert torch.equal(low, low_f) and torch.equal(high, high_f)
    assert IS.UNet3D.band_split == "fft"
    with pytest.raises(ValueError, match="impl"):
        IS.frequency_bands(x, impl="rocfft")


def test_device_impl_refuses_a_cpu_tensor():
    with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):
        IS.frequency_bands(torch.zeros(1, 1, 2, 8, 8), impl="device")
    with pytest.raises(mi355seg.Mi355SegError, match="no CPU fallback"):
        F.frequency_bands(torch.zeros(1, 1, 2, 8, 8))


def test_config_band_split_sets_the_model_attribute():
    m = IS.UNet3D(1, 2, 4)
    IS.set_band_split(m, {"network": "IS"})
    assert m.band_split == "fft"
    IS.set_band_split(m, {"band_split": "device"})
    assert m.band_split == "device" and IS.UNet3D.band_split == "fft"
    with pytest.raises(ValueError, match="band_split"):
        IS.set_band_split(m, {"band_split": "gpu"})
    plain = torch.nn.Identity()
    IS.set_band_split(plain, {"band_split": "device"})     # a network without bands ignores the key
    assert not hasattr(plain, "band_split")


def test_supported_query_at_the_boundaries():
    q = lambda *a: mi355seg.lib().query("mi355seg_band_split_supported", *a)
    assert q(1, 1, 1, 256, 256, 21, 21, 21, 21) >= 1 and q(1, 1, 1, 257, 256, 21, 21, 21, 21) == 0
    assert q(1, 1, 1, 256, 257, 21, 21, 21, 21) == 0
    assert q(2, 2, 3, 16, 16, 1, 1, 1, 1) >= 1 and q(3, 1, 3, 16, 16, 1, 1, 1, 1) == 0 and q(1, 4, 3, 16, 16, 1, 1, 1, 1) == 0
    assert q(1, 1, 1, 64, 64, 5, 32, 5, 32) >= 1 and q(1, 1, 1, 64, 64, 5, 33, 5, 5) == 0 and q(1, 1, 1, 64, 64, 5, 5, 5, 33) == 0
    assert q(1, 1, 1, 8, 8, 3, 2, 1, 1) == 0 and q(1, 1, 1, 8, 8, 1, 9, 1, 1) == 0 and q(1, 1, 0, 8, 8, 1, 1, 1, 1) == 0
    assert q(1, 1, 1, 8, 8, 0, 0, 0, 0) >= 1 and q(1, 1, 1, 1, 1, 1, 1, 1, 1) >= 1
    # a slice stays in LDS up to 160x192 (one chunk); 256x256 is staged in row chunks
    assert q(1, 1, 1, 128, 128, 11, 11, 11, 11) == 1 and q(1, 1, 1, 160, 192, 13, 13, 15, 15) == 1
    assert q(1, 1, 1, 256, 256, 21, 21, 21, 21) > 1


def test_entry_point_refuses_bad_arguments_without_a_launch():
    L = mi355seg.lib()
    with pytest.raises(mi355seg.Mi355SegError, match="band_split"):
        L.call("mi355seg_band_split_f32", None, 1, 1, 1, 8, 8, None, 1, 1, None, 1, 1, None, None, None)
    for shape in ((3, 1, 1, 8, 8), (1, 4, 1, 8, 8), (1, 1, 1, 257, 8)):     # refused on the shape alone: the pointers are never read
        with pytest.raises(mi355seg.Mi355SegError, match="unsupported shape"):
            L.call("mi355seg_band_split_f32", 16, *shape, 16, 1, 1, 16, 1, 1, 16, 16, None)
