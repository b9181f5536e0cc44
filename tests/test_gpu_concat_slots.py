"""The concat-slot forms of functional.py against the same nodes without a slot followed by cat_channels.

A slot is the right channel slice of a buffer with ``left_pad`` free channels on its left (functional._concat_out): a producer --
instance_norm_act, activation_fork, conv_bn_act(left_pad=) -- writes its result there, and a filler -- conv_transpose3d_k2s2_cat,
conv_in_act(cat_right=) -- writes the left channels in place and returns the whole buffer: cat((filler, producer), channels) without
the copies.  Both chains run the same kernels on the same values, only the pitch of what the forward writes differs, so

* element-wise results -- the concatenated activation, and the input gradient of activation_fork, which no reduction feeds -- must
  be ``torch.equal``;
* reduced results (dgamma, dbeta, bias and weight gradients, input gradients behind batch / instance statistics or a contraction over
  channels) take the tolerance tests/test_gpu_ops.py applies to these nodes' gradients: fp32 ``rel_err < TOL`` with TOL = 1e-4
  (test_gpu_ops.py:12, applied at :118-120 to the convolution, :183-185 to the up-convolution and :273 to the norm gradients); bf16
  ``<= 2 ** -7 * max(1, max |ref|)`` (test_gpu_ops.py:1205-1208, the one bf16 bound that file has: activation_fork's).

Shapes: N = 1, extents 4 x 6 x 8; 8 channels behind a 4-channel slot (16-byte quads throughout), then 6 behind 6 (the scalar row
paths)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4                     # tests/test_gpu_ops.py:12
TOL_BF16 = 2.0 ** -7           # tests/test_gpu_ops.py:1205
LEAD = (1, 4, 6, 8)
CZ = 5                         # channels of the filler's own input


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mi355seg
    mi355seg.lib()
    return mi355seg


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def leaf(t, dtype):
    return t.to(dtype).cuda().requires_grad_(True)


def close(name, got, ref, exact, dtype):
    got, ref = got.detach(), ref.detach()
    diff, top = float((got.float() - ref.float()).abs().max()), float(ref.float().abs().max())
    print(f"{name}: max |slot - dense| = {diff:.3e}, max |dense| = {top:.3e}")
    if exact:
        assert torch.equal(got, ref), f"{name}: the slot form differs from the dense form by {diff:.3e}"
    elif dtype == torch.float32:
        assert diff / max(1e-12, top) < TOL, name
    else:
        assert diff <= TOL_BF16 * max(1.0, top), name


def run_chain(F, producer, filler, slot, C, P, dtype, mods):
    """One chain, forward and backward: {name: (tensor, element-wise?)}."""
    from mi355seg.layers import InstanceNorm3d
    conv_p, bn_p, conv_f = (copy.deepcopy(m) for m in mods)
    x = leaf(rnd(*LEAD, C, seed=1), dtype)
    out, grads, res = {}, [], {}
    lp = P if slot else 0
    if producer == "instance_norm_act":
        skip = F.instance_norm_act(x, 1e-5, F.ACT_LRELU, 0.01, left_pad=lp)
    elif producer == "activation_fork":
        skip, passed = F.activation_fork(x, F.ACT_LRELU, 0.01, left_pad=lp)
        out["pass"], grads = passed, [rnd(*LEAD, C, seed=5).to(dtype).cuda()]
    else:
        skip = F.conv_bn_act(x, conv_p, bn_p, F.ACT_RELU, left_pad=lp)
        res.update({"producer running_mean": (bn_p.running_mean, False), "producer running_var": (bn_p.running_var, False)})
    assert tuple(skip.shape) == LEAD + (C,) and (skip._base is not None) == slot
    if filler == "conv_transpose3d_k2s2_cat":
        z = leaf(rnd(1, 2, 3, 4, CZ, seed=2), dtype)
        w, b = leaf(rnd(CZ, P, 2, 2, 2, seed=3, scale=0.2), torch.float32), leaf(rnd(P, seed=4, scale=0.1), torch.float32)
        cat = F.conv_transpose3d_k2s2_cat(z, w, b, skip) if slot else F.cat_channels(F.conv_transpose3d_k2s2(z, w, b), skip)
    else:
        z = leaf(rnd(*LEAD, CZ, seed=2), dtype)
        w, b = conv_f.weight, conv_f.bias
        cat = F.conv_in_act(z, conv_f, InstanceNorm3d(P), F.ACT_LRELU, 0.01, cat_right=skip)
    assert tuple(cat.shape) == LEAD + (P + C,)
    if slot:
        assert cat.data_ptr() == skip._base.data_ptr(), "the filler did not write the slot in place"
    out["cat"] = cat
    torch.autograd.backward([out["cat"]] + [out[k] for k in out if k != "cat"], [rnd(*LEAD, P + C, seed=6).to(dtype).cuda()] + grads)
    res["cat"] = (cat, True)
    res["producer dx"] = (x.grad, producer == "activation_fork")
    res.update({"filler dx": (z.grad, False), "filler dw": (w.grad, False), "filler db": (b.grad, False)})
    if producer == "conv_bn_act":
        res.update({"producer " + n: (p.grad, False) for n, p in list(conv_p.named_parameters()) + [("gamma", bn_p.weight), ("beta", bn_p.bias)]})
    return res


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C,P", [(8, 4), (6, 6)], ids=["c8_slot4", "c6_slot6"])
@pytest.mark.parametrize("filler", ["conv_transpose3d_k2s2_cat", "conv_in_act"])
@pytest.mark.parametrize("producer", ["instance_norm_act", "activation_fork", "conv_bn_act"])
def test_slot_chain_equals_the_dense_chain_with_cat_channels(seg, producer, filler, C, P, dtype):
    F = seg.functional
    from mi355seg.layers import BatchNorm3d, Conv3d
    torch.manual_seed(11)
    mods = (Conv3d(C, C, 3, padding=1).cuda(), BatchNorm3d(C).cuda().train(), Conv3d(CZ, P, 3, padding=1).cuda())
    with torch.no_grad():
        mods[1].weight.copy_(1.0 + 0.1 * rnd(C, seed=7)), mods[1].bias.copy_(0.1 * rnd(C, seed=8))
    dense = run_chain(F, producer, filler, False, C, P, dtype, mods)
    slot = run_chain(F, producer, filler, True, C, P, dtype, mods)
    assert slot.keys() == dense.keys()
    for name, (got, exact) in slot.items():
        close(f"{producer} -> {filler} {name}", got, dense[name][0], exact, dtype)
