"""The IS network's frequency-band split as one launch of the library (csrc/band.hip, functional.frequency_bands,
``frequency_bands(impl="device")``): against the fixtures the reference's low_pass_torch / high_pass_torch produced
(train.py:76-88), against the fp64 evaluation of the definition at every size class of the kernel, its hygiene (reproducible, in
bounds, slice-independent, capturable), its refusals, and its wiring into the train step and the sliding-window prediction.

fp64 grading bar: |got - fp64| <= 1e-5 * max(1, max|x|) -- the project's 1e-5 band bar (test_gpu_models.py) scaled by the input;
an fp32 emulation of the low-rank form sits at most 1.9e-6 * max|x| from fp64 (256x256, white noise of amplitude 3 on an offset of
1000), about a fifth of the bar.  Each test prints its measured maxima before it asserts."""
import os

import numpy as np
import pytest
import torch

from oracle.fill import fill_module_, make_input, make_input_rough, make_labels
from oracle.step import two_channel_gt

pytestmark = pytest.mark.gpu
BAR = 1e-5

# the issue's shapes, then one slice size on each side of the LDS-resident / row-chunked switch (168x192 is the last resident
# height at width 192, 170x192 the first chunked one) and an odd chunked shape (scalar loads / stores, ragged last row tile)
SHAPES = [(1, 1, 3, 5, 6), (2, 2, 3, 7, 9), (1, 1, 1, 1, 16), (1, 1, 2, 24, 26), (1, 1, 4, 25, 50), (1, 2, 2, 100, 33), (1, 1, 2, 64, 96),
          (1, 1, 2, 128, 128), (1, 1, 2, 160, 192), (1, 1, 2, 256, 256), (1, 1, 1, 168, 192), (1, 1, 1, 170, 192), (2, 1, 1, 255, 253)]
KINDS = ("rough", "rough+1000", "constant", "impulse")


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mi355seg
    mi355seg.lib()
    return mi355seg


def fp64_bands(x, limit=0.04):
    """The definition in fp64 (as tests/test_band_split_host.py pins it to the reference's fixtures)."""
    from mi355seg.functional import band_basis
    x = x.detach().cpu().double().numpy()
    if x.shape[0] == 2:
        x = np.stack([x[0] + x[1], x[0] - x[1]])
    if x.shape[1] == 2:
        x = np.stack([x[:, 0] + x[:, 1], x[:, 0] - x[:, 1]], axis=1)
    H, W = x.shape[-2:]
    (eh, rh), (ew, rw) = band_basis(H, limit), band_basis(W, limit)
    return (eh[:rh].T @ eh[:rh]) @ x @ (ew[:rw].T @ ew[:rw]), (np.eye(H) - eh.T @ eh) @ x @ (np.eye(W) - ew.T @ ew)


def make_case(shape, kind):
    if kind == "rough":
        return make_input_rough(shape) * 3
    if kind == "rough+1000":
        return make_input_rough(shape) * 3 + 1000
    if kind == "constant":
        return torch.full(shape, 7.25)
    x = torch.zeros(shape)                                  # one impulse per slice, walking over rows and columns; the first at the far corner
    B, C, D, H, W = shape
    for s in range(B * C * D):
        x.view(-1, H, W)[s, (H - 1 + 7 * s) % H, (W - 1 + 5 * s) % W] = 2.0
    return x


_REF = {}


def reference(shape, kind):
    """(x, fp64 low, fp64 high), computed once per case and shared read-only"""
    key = (shape, kind)
    if key not in _REF:
        x = make_case(shape, kind)
        _REF[key] = (x,) + fp64_bands(x)
    return _REF[key]


def test_device_split_matches_the_reference_fixtures(seg, golden_dir):
    from mi355seg.models.three_d.IS import frequency_bands
    g = np.load(os.path.join(golden_dir, "ovr_isnet.npz"))
    g32 = np.load(os.path.join(golden_dir, "isnet_f4_32.npz"))
    cases = [(make_input((1, 1, 16, 16, 16), freq=0.37), g["band_low_a"], g["band_high_a"]),
             (make_input((2, 1, 8, 12, 16), freq=0.21), g["band_low_b"], g["band_high_b"]),
             (make_input((1, 1, 32, 32, 32), freq=0.37), g32["low"], g32["high"])]
    for x, low_ref, high_ref in cases:
        low, high = frequency_bands(x.cuda(), impl="device")
        e_low, e_high = np.abs(low.cpu().numpy() - low_ref).max(), np.abs(high.cpu().numpy() - high_ref).max()
        print(tuple(x.shape), "low", e_low, "high", e_high)
        assert e_low < 1e-5 and e_high < 1e-5


def test_chunk_switch_sits_where_the_shapes_assume(seg):
    """SHAPES brackets the switch between the LDS-resident and the row-chunked form; if the kernel's LDS plan moves, move them."""
    from mi355seg.functional import band_basis
    chunks = {}
    for H, W in ((160, 192), (168, 192), (170, 192), (256, 256), (255, 253)):
        (eh, rh), (ew, rw) = band_basis(H), band_basis(W)
        chunks[(H, W)] = seg.lib().query("mi355seg_band_split_supported", 1, 1, 1, H, W, rh, len(eh), rw, len(ew))
    assert chunks[(160, 192)] == 1 and chunks[(168, 192)] == 1 and chunks[(170, 192)] == 2, chunks
    assert chunks[(256, 256)] > 1 and chunks[(255, 253)] > 1, chunks


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_device_split_vs_fp64(seg, shape, kind):
    x, low_ref, high_ref = reference(shape, kind)
    low, high = seg.functional.frequency_bands(x.cuda())
    assert low.shape == x.shape and high.shape == x.shape and low.dtype == torch.float32 and high.dtype == torch.float32
    bar = BAR * max(1.0, float(x.abs().max()))
    e_low, e_high = np.abs(low.cpu().numpy() - low_ref).max(), np.abs(high.cpu().numpy() - high_ref).max()
    print(f"{shape} {kind}: max|low - fp64| = {e_low:.3e}, max|high - fp64| = {e_high:.3e}, bar {bar:.3e}")
    assert e_low <= bar and e_high <= bar
    if kind == "constant" and shape[0] == 1 and shape[1] == 1:
        assert np.abs(low.cpu().numpy() - 7.25).max() <= bar and np.abs(high.cpu().numpy()).max() <= bar


@pytest.mark.parametrize("shape", [(2, 2, 3, 7, 9), (1, 1, 2, 128, 128), (1, 1, 2, 170, 192)], ids=lambda s: "x".join(map(str, s)))
def test_two_calls_are_bitwise_equal(seg, shape):
    x = reference(shape, "rough")[0].cuda()
    a, b = seg.functional.frequency_bands(x), seg.functional.frequency_bands(x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("pad", [64, 3])
@pytest.mark.parametrize("shape", [(2, 2, 3, 7, 9), (1, 1, 1, 1, 16), (1, 2, 2, 100, 33), (1, 1, 2, 128, 128), (1, 1, 1, 170, 192),
                                   (2, 1, 1, 255, 253)], ids=lambda s: "x".join(map(str, s)))
def test_outputs_stay_inside_their_allocations(seg, shape, pad):
    """low and high written through the C entry point into sentinel-padded buffers (pad 3: a misaligned base, the scalar-store
    form): the padding is untouched and the payload equals the op's."""
    F = seg.functional
    x = reference(shape, "rough")[0].cuda()
    B, C, D, H, W = shape
    (eh, rh, qh), (ew, rw, qw) = F._band_basis_device(H, 0.04, x.device), F._band_basis_device(W, 0.04, x.device)
    n, sentinel = x.numel(), -12345.0
    bufs = [torch.full((n + 2 * pad,), sentinel, device="cuda") for _ in range(2)]
    seg.lib().call("mi355seg_band_split_f32", x.data_ptr(), B, C, D, H, W, eh.data_ptr(), rh, qh, ew.data_ptr(), rw, qw,
                   bufs[0][pad:].data_ptr(), bufs[1][pad:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    low, high = F.frequency_bands(x)
    for buf, want in zip(bufs, (low, high)):
        assert bool((buf[:pad] == sentinel).all()) and bool((buf[pad + n:] == sentinel).all())
        assert torch.equal(buf[pad:pad + n].view(shape), want)


@pytest.mark.parametrize("shape", [(1, 1, 4, 25, 50), (1, 1, 3, 64, 96), (1, 1, 2, 170, 192)], ids=lambda s: "x".join(map(str, s)))
def test_volume_equals_its_slices(seg, shape):
    x = make_input_rough(shape, seed=2.0).cuda()
    low, high = seg.functional.frequency_bands(x)
    for d in range(shape[2]):
        lo_d, hi_d = seg.functional.frequency_bands(x[:, :, d:d + 1])
        assert torch.equal(lo_d, low[:, :, d:d + 1]) and torch.equal(hi_d, high[:, :, d:d + 1])


def test_captured_call_replays_bitwise(seg):
    """The op alone in one graph on one stream: after the eager call that warms the basis cache the capture holds the launch only."""
    F = seg.functional
    shape = (2, 1, 3, 64, 96)
    static_x = make_input_rough(shape, seed=1.0).cuda()
    F.frequency_bands(static_x)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        low, high = F.frequency_bands(static_x)
    x2 = (make_input_rough(shape, seed=5.0) * 3 + 2).cuda()
    static_x.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    want = F.frequency_bands(x2)
    assert torch.equal(low, want[0]) and torch.equal(high, want[1])


def test_refusals_launch_nothing(seg):
    F, E = seg.functional, seg.Mi355SegError
    calls = []
    real = seg.lib().call
    seg.lib().call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        with pytest.raises(E, match="all-axes-transform quirk"):
            F.frequency_bands(torch.zeros(3, 1, 2, 8, 8, device="cuda"))
        with pytest.raises(E, match="all-axes-transform quirk"):
            F.frequency_bands(torch.zeros(1, 4, 2, 8, 8, device="cuda"))
        with pytest.raises(E, match="1 .. 256"):
            F.frequency_bands(torch.zeros(1, 1, 1, 257, 8, device="cuda"))
        with pytest.raises(E, match="expected float32"):
            F.frequency_bands(torch.zeros(1, 1, 2, 8, 8, device="cuda", dtype=torch.bfloat16))
        with pytest.raises(NotImplementedError, match="no gradient"):
            F.frequency_bands(torch.zeros(1, 1, 2, 8, 8, device="cuda", requires_grad=True))
    finally:
        del seg.lib().call
    assert calls == []


def test_isnet_fixture_with_device_bands(seg, golden_dir):
    """The body of test_gpu_models.py::test_isnet_vs_reference_fixture with the model fed from the device split."""
    from mi355seg.models.three_d.IS import UNet3D as ISNet, frequency_bands
    g = np.load(os.path.join(golden_dir, "isnet_f4_32.npz"))
    m = fill_module_(ISNet(in_channels=1, out_channels=2, init_features=4)).cuda().train()
    x = make_input((1, 1, 32, 32, 32), freq=0.37).cuda()
    gt2 = two_channel_gt(make_labels((1, 1, 32, 32, 32))).cuda()
    low, high = frequency_bands(x, impl="device")
    assert np.abs(low.cpu().numpy() - g["low"]).max() < 1e-5 and np.abs(high.cpu().numpy() - g["high"]).max() < 1e-5
    out1, out2 = m(x, low, high)
    loss = seg.functional.bce_with_logits(out1, gt2)
    loss.backward()
    assert abs(loss.item() - float(g["loss"])) < 1e-5
    assert np.abs(out1.detach().cpu().numpy() - g["out1"]).max() < 1e-4
    assert np.abs(out2.detach().cpu().numpy() - g["out2"]).max() < 1e-4
    params, bufs = dict(m.named_parameters()), dict(m.named_buffers())
    n_grad = 0
    for k in g.files:
        if k.startswith("hasgrad/"):
            assert (params[k[8:]].grad is not None) == bool(g[k]), k
            n_grad += int(bool(g[k]))
        elif k.startswith("grad/"):
            f = params[k[5:]].grad.detach().reshape(-1)
            got = f[::max(1, f.numel() // 4096)][:4096].cpu().numpy()
            assert np.abs(got - g[k]).max() <= 3e-4 * max(1e-3, np.abs(g[k]).max()), k
        elif k.startswith("buf/") and not k.endswith("num_batches_tracked"):
            assert (np.abs(bufs[k[4:]].cpu().numpy() - g[k]) / np.maximum(1.0, np.abs(g[k]))).max() < 1e-5, k
    assert n_grad == 82


def test_train_step_device_bands_agree_with_fft_bands(seg):
    from mi355seg.engine import train_step
    from mi355seg.models.three_d.IS import UNet3D as ISNet
    x = make_input((1, 1, 32, 32, 32), freq=0.37).cuda()
    gt = make_labels((1, 1, 32, 32, 32)).cuda()
    loss = {}
    for impl in ("device", "fft"):
        m = fill_module_(ISNet(1, 2, 4)).cuda().train()
        m.band_split = impl
        out = train_step(m, torch.optim.Adam(m.parameters(), lr=1e-3), x, gt)
        loss[impl] = out["loss"].item()
    print(loss)
    assert abs(loss["device"] - loss["fft"]) < 1e-5


def test_sliding_window_predict_passes_band_split_through(seg, monkeypatch):
    from mi355seg.models.three_d import IS
    from mi355seg.predict import sliding_window_predict
    seen = []
    real = IS.frequency_bands

    def spy(x, limit=0.04, impl="fft"):
        seen.append(impl)
        return real(x, limit, impl)
    monkeypatch.setattr(IS, "frequency_bands", spy)
    m = fill_module_(IS.UNet3D(1, 2, 4)).cuda()
    vol = make_input((1, 32, 32, 32), freq=0.37).cuda()
    for impl in ("fft", "device"):
        m.band_split = impl
        assert sliding_window_predict(m, vol, (32, 32, 32), (4, 4, 4)).shape == (1, 32, 32, 32)
    assert seen == ["fft", "device"]
    del m.band_split
    sliding_window_predict(m, vol, (32, 32, 32), (4, 4, 4))
    assert seen[-1] == "fft"
