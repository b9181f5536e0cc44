"""Every weight packing of a step in one launch (csrc/prepack.hip, functional.prepacked_weights): a model trained with its packings formed
all at once must end up with bit-identical parameters to the same model packing in place, under every conv math, for the fp32
U-Net (conv_x3s / generic / ConvT packings), the bf16 Residual U-Net (the one packing of a stride-2 input gradient's phases, modules
applied twice per step) and inside a captured HIP graph."""
import pytest
import torch

from oracle.fill import fill_module_, make_input, make_labels

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mi355seg
    mi355seg.lib()
    return mi355seg


def _train(model_fn, x, gt, steps, prepack, monkeypatch, dtype=None, graphed=False):
    from mi355seg import functional as F
    from mi355seg.engine import train_step, GraphedTrainStep
    monkeypatch.setattr(F, "_PREPACK_OFF", not prepack)
    m = fill_module_(model_fn()).cuda().train()
    if graphed:
        opt = torch.optim.Adam(m.parameters(), lr=1e-3, capturable=True)
        g = GraphedTrainStep(m, opt, x, gt, warmup=2, dtype=dtype)
        losses = [float(g.first["loss"])]
        for _ in range(steps - 2):
            losses.append(float(g(x, gt, sync_metric=False)["loss"]))
    else:
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        losses = [float(train_step(m, opt, x, gt, sync_metric=False, dtype=dtype)["loss"]) for _ in range(steps)]
    torch.cuda.synchronize()
    plans = F.prepack_plans(m)
    jobs = sum(F.lib().query("mi355seg_prepack_jobs", r["plan"]) for r in plans.values())
    return [p.detach().clone() for p in m.parameters()], losses, jobs


@pytest.mark.parametrize("math", ["f16x3", "bf16x6", "fp32"])
def test_unet_prepacked_steps_are_bit_identical(seg, monkeypatch, math):
    from mi355seg.models.three_d.unet3d import UNet3D
    seg.set_conv_math(math)
    try:
        x = make_input((2, 1, 32, 32, 32)).cuda()
        gt = make_labels((2, 1, 32, 32, 32)).cuda()
        fn = lambda: UNet3D(in_channels=1, out_channels=2, init_features=16)
        pa, la, ja = _train(fn, x, gt, 4, True, monkeypatch)
        pb, lb, jb = _train(fn, x, gt, 4, False, monkeypatch)
    finally:
        seg.set_conv_math(seg.DEFAULT_CONV_MATH)
    # forward + input-gradient packings of the k3 convolutions and the four ConvT layers (the exact-fp32 MFMA layout is not a replayed one)
    assert ja >= (20 if math != "fp32" else 0) and jb == 0, (ja, jb)
    assert la == lb
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)


def test_res_unet_bf16_prepacked_steps_are_bit_identical(seg, monkeypatch):
    from mi355seg.models.three_d.residual_unet3d import UNet
    x = make_input((1, 4, 32, 48, 32)).cuda()
    gt = make_labels((1, 1, 32, 48, 32)).cuda()
    from mi355seg import functional as F
    # Dropout3d draws from the device generator: the same seed in front of both runs
    fn = lambda: UNet(in_channels=4, n_classes=2, base_n_filter=16)
    torch.manual_seed(7); torch.cuda.manual_seed(7)
    pa, la, ja = _train(fn, x, gt, 3, True, monkeypatch, dtype=torch.bfloat16)
    torch.manual_seed(7); torch.cuda.manual_seed(7)
    pb, lb, jb = _train(fn, x, gt, 3, False, monkeypatch, dtype=torch.bfloat16)
    assert ja >= 20 and jb == 0, (ja, jb)
    assert la == lb
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)


def test_prepacked_steps_inside_a_captured_graph(seg, monkeypatch):
    from mi355seg.models.three_d.unet3d import UNet3D
    x = make_input((2, 1, 32, 32, 32)).cuda()
    gt = make_labels((2, 1, 32, 32, 32)).cuda()
    fn = lambda: UNet3D(in_channels=1, out_channels=2, init_features=16)
    pa, la, ja = _train(fn, x, gt, 5, True, monkeypatch, graphed=True)
    pb, lb, jb = _train(fn, x, gt, 5, False, monkeypatch, graphed=True)
    assert ja >= 20 and jb == 0
    assert la == lb
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)


def test_prepack_plan_follows_the_input_shape(seg, monkeypatch):
    """A second input shape records a second plan; going back to the first replays the first (no stale geometry)."""
    from mi355seg import functional as F
    from mi355seg.engine import train_step
    from mi355seg.models.three_d.unet3d import UNet3D
    monkeypatch.setattr(F, "_PREPACK_OFF", False)
    m = fill_module_(UNet3D(in_channels=1, out_channels=2, init_features=16)).cuda().train()
    ref = fill_module_(UNet3D(in_channels=1, out_channels=2, init_features=16)).cuda().train()
    opt, opt_ref = torch.optim.Adam(m.parameters(), lr=1e-3), torch.optim.Adam(ref.parameters(), lr=1e-3)
    shapes = [(2, 1, 32, 32, 32), (1, 1, 48, 32, 32), (2, 1, 32, 32, 32), (1, 1, 48, 32, 32)]
    for shp in shapes:
        x, gt = make_input(shp).cuda(), make_labels(shp).cuda()
        monkeypatch.setattr(F, "_PREPACK_OFF", False)
        a = train_step(m, opt, x, gt, sync_metric=False)["loss"]
        monkeypatch.setattr(F, "_PREPACK_OFF", True)
        b = train_step(ref, opt_ref, x, gt, sync_metric=False)["loss"]
        assert float(a) == float(b)
    assert len(F.prepack_plans(m)) == 2
    for p, q in zip(m.parameters(), ref.parameters()):
        assert torch.equal(p, q)


# ---- the bracket's contract on the smallest module the matrix-core path takes: two Conv3d(32, 32, 3, padding=1) on 1 x 32 x 16^3, fp32 under
# f16x3 (the implicit-GEMM tiles are 32 output channels wide: a 16-channel layer goes to the small-channel kernels, which pack nothing)
_C, _SHAPE = 32, (1, 32, 16, 16, 16)


class _TwoConvs(torch.nn.Module):
    """x -> conv a -> conv b.  ``a_weight`` picks what conv a is handed as its weight: the parameter itself, or 2 * it (a tensor computed in
    the forward: storage no parameter owns)."""

    def __init__(self, a_weight="param"):
        super().__init__()
        from mi355seg import layers
        self.a, self.b, self.a_weight = layers.Conv3d(_C, _C, 3, padding=1), layers.Conv3d(_C, _C, 3, padding=1), a_weight

    def forward(self, x):
        from mi355seg import functional as F
        h = F.to_channels_last(x)
        h = F.conv3d(h, 2 * self.a.weight if self.a_weight == "computed" else self.a.weight, self.a.bias, 1, 1)
        return F.to_channels_first(self.b(h))


def _bracket(m, x, dy):
    """One prepacked_weights bracket with forward and backward: (y, dx, parameter gradients), the module's gradients cleared again."""
    from mi355seg import functional as F
    x = x.detach().requires_grad_(True)              # (conv a runs its input gradient too)
    with F.prepacked_weights(m, ("test", tuple(x.shape))):
        y = m(x)
        y.backward(dy)
    grads = [p.grad.clone() for p in m.parameters()]
    m.zero_grad(set_to_none=True)
    return y.detach(), x.grad, grads


def _sgd_step(m, x):
    """A whole training iteration inside one bracket; the update keeps the parameters' storage."""
    y, _, grads = _bracket(m, x, torch.ones((x.shape[0], _C) + tuple(x.shape[2:]), device=x.device))
    with torch.no_grad():
        for p, g in zip(m.parameters(), grads):
            p.sub_(g, alpha=1e-4)
    return y


def _plan_ids(F, m):
    return {r["plan"] for r in F.prepack_plans(m).values() if r["plan"]}


@pytest.mark.parametrize("variant", ["channels_last_param", "computed"])
def test_plan_keeps_no_packing_of_a_weight_outside_the_parameters(seg, monkeypatch, variant):
    """A weight pointer that is not parameter storage -- the contiguous copy _w32 makes of a channels_last_3d parameter, 2 * param computed in
    the forward -- is a temporary: its packings must not enter the plan (every later step would read freed memory).  The contiguous conv
    beside it keeps its forward and input-gradient packings; results are bit-equal to packing in place."""
    from mi355seg import functional as F
    seg.set_conv_math("f16x3")
    try:
        x, dy = make_input(_SHAPE).cuda(), make_input(_SHAPE, freq=0.02).cuda()

        def run(prepack):
            monkeypatch.setattr(F, "_PREPACK_OFF", not prepack)
            m = fill_module_(_TwoConvs("computed" if variant == "computed" else "param")).cuda().train()
            if variant == "channels_last_param":
                m.a.weight.data = m.a.weight.data.to(memory_format=torch.channels_last_3d)
                assert not m.a.weight.is_contiguous()
            _bracket(m, x, dy)                       # records
            out = _bracket(m, x, dy)                 # replays
            torch.cuda.synchronize()
            return out, sum(F.lib().query("mi355seg_prepack_jobs", i) for i in _plan_ids(F, m))
        (ya, dxa, ga), ja = run(True)
        (yb, dxb, gb), jb = run(False)
    finally:
        seg.set_conv_math(seg.DEFAULT_CONV_MATH)
    assert (ja, jb) == (2, 0)                        # conv b forward + input gradient; nothing of conv a's weight
    assert torch.equal(ya, yb) and torch.equal(dxa, dxb)
    for a, b in zip(ga, gb):
        assert torch.equal(a, b)


def test_deepcopy_records_its_own_plans_and_leaves_the_originals_alone(seg, monkeypatch):
    """A deep copy starts without plans; its evictions (four plans kept) free none of the original's."""
    import copy
    from mi355seg import functional as F
    monkeypatch.setattr(F, "_PREPACK_OFF", False)
    x = make_input(_SHAPE).cuda()
    m, twin = (fill_module_(_TwoConvs()).cuda().train() for _ in range(2))
    for _ in range(2):
        _sgd_step(m, x)
    c = copy.deepcopy(m)
    assert F.prepack_plans(c) == {} and _plan_ids(F, m)
    for d in (20, 24, 28, 32, 36):                   # five new shapes: the copy's table evicts
        _sgd_step(c, make_input((1, _C, d, 16, 16)).cuda())
    assert len(F.prepack_plans(c)) == 4 and not (_plan_ids(F, c) & _plan_ids(F, m))
    _sgd_step(m, x)
    for _ in range(3):
        _sgd_step(twin, x)
    torch.cuda.synchronize()
    for p, q in zip(m.parameters(), twin.parameters()):
        assert torch.equal(p, q)


def test_bracket_closes_when_the_body_raises(seg, monkeypatch):
    from mi355seg import functional as F
    monkeypatch.setattr(F, "_PREPACK_OFF", False)
    x = make_input(_SHAPE).cuda()
    m = fill_module_(_TwoConvs()).cuda().train()
    _sgd_step(m, x)                                  # records
    with pytest.raises(RuntimeError, match="in the body"):
        with F.prepacked_weights(m, ("test", tuple(x.shape))) as pp:
            assert pp.replaying and F.lib().query("mi355seg_prepack_active") == 1
            m(x)
            raise RuntimeError("in the body")
    assert F.lib().query("mi355seg_prepack_active") == 0 and not F.prepacked_weights.active
    _sgd_step(m, x)                                  # the next step finds no open bracket
    torch.cuda.synchronize()
