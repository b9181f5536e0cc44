"""Host logic around the convolution nodes of functional.py (no GPU, the library is never loaded): which Conv3d modules the fused
entry points refuse, the concat-slot predicate, and the switches that are gone."""
import inspect
import os
import re

import pytest
import torch

import mi355seg
from mi355seg import functional as F
from mi355seg.layers import BatchNorm3d, Conv3d, InstanceNorm3d

UNSUPPORTED = {"stride": dict(stride=(1, 2, 2)), "padding": dict(padding=(0, 1, 1)), "dilation": dict(dilation=2),
               "groups": dict(groups=2), "padding_mode": dict(padding_mode="reflect")}


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(F, "lib", refuse)


@pytest.mark.parametrize("entry", ["conv_bn_act", "conv_in_act", "double_conv_bn_act_first", "double_conv_bn_act_second"])
@pytest.mark.parametrize("what", sorted(UNSUPPORTED))
def test_fused_entries_refuse_what_conv3d_refuses_before_touching_anything(no_library, entry, what):
    """layers.Conv3d.forward raises NotImplementedError for these modules; so do the fused entries -- on a CPU tensor, i.e. before any
    device or library call -- and a refused call leaves num_batches_tracked alone."""
    bad = Conv3d(4, 4, kernel_size=3, **{"padding": 1, **UNSUPPORTED[what]})
    good = Conv3d(4, 4, kernel_size=3, padding=1)
    bn1, bn2 = BatchNorm3d(4).train(), BatchNorm3d(4).train()
    x = torch.zeros(1, 8, 8, 8, 4)
    with pytest.raises(NotImplementedError):
        bad(x)
    with pytest.raises(NotImplementedError):
        if entry == "conv_bn_act":
            F.conv_bn_act(x, bad, bn1, F.ACT_RELU)
        elif entry == "conv_in_act":
            F.conv_in_act(x, bad, InstanceNorm3d(4), F.ACT_LRELU)
        elif entry == "double_conv_bn_act_first":
            F.double_conv_bn_act(x, bad, bn1, good, bn2, F.ACT_RELU)
        else:
            F.double_conv_bn_act(x, good, bn1, bad, bn2, F.ACT_RELU)
    assert int(bn1.num_batches_tracked) == 0 and int(bn2.num_batches_tracked) == 0


def test_concat_base_accepts_only_the_right_slice_of_a_matching_buffer():
    lead, Cout, Cs = (1, 4, 4, 4), 3, 5
    buf = torch.zeros(lead + (Cout + Cs,))
    assert F._concat_base(buf[..., Cout:], Cout, lead, torch.float32) is buf
    assert F._concat_base(buf[..., :Cs], Cout, lead, torch.float32) is None                                 # a left slice
    assert F._concat_base(torch.zeros(lead + (Cout + Cs + 1,))[..., Cout + 1:], Cout, lead, torch.float32) is None    # one channel too wide
    assert F._concat_base(buf[..., Cout:], Cout, lead, torch.bfloat16) is None                              # dtype mismatch
    assert F._concat_base(buf[..., Cout:], Cout, (1, 4, 4, 2), torch.float32) is None                       # other extents
    pitch = 2 * (Cout + Cs)
    wide = torch.empty_strided(lead + (Cout + Cs,), (64 * pitch, 16 * pitch, 4 * pitch, pitch, 1))
    assert wide._base is None and not wide.is_contiguous()
    assert F._concat_base(wide[..., Cout:], Cout, lead, torch.float32) is None                              # non-contiguous base
    assert F._concat_base(torch.zeros(lead + (Cs,)), Cout, lead, torch.float32) is None                     # no base at all


def _source(name):
    return open(os.path.join(os.path.dirname(os.path.abspath(mi355seg.functional.__file__)), name)).read()


# entry-point stem -> the one function of functional.py that names it (the _add_ forms are spelt by their base launcher);
# norm_stats_from_sums is another entry point, with a launcher of its own (_stats_from_sums)
LAUNCHERS = {"norm_stats_(?!from_sums)": "_batch_stats", "rstd_from_var": "_running_stats", "norm_act_fwd": "_norm_act_fwd",
             "norm_act_bwd_colsum": "_norm_act_bwd", "maxpool2_fwd": "_maxpool2_fwd", "maxpool2_bwd": "_maxpool2_bwd",
             "upsample2_bwd": "_upsample2_bwd", "act_bwd_": "_act_bwd",
             # the fused forms of the conv + BatchNorm nodes
             "conv3d_fwd_pro_ax": "_conv_fwd_pro", "conv3d_fwd_yamax_ax": "_conv_fwd_yamax", "norm_fold_": "_norm_fold",
             "bn_act_head_fwd": "_bn_act_head_fwd", "bn_act_head_bwd_sums": "_bn_act_head_bwd", "bn_act_head_bwd_apply": "_bn_act_head_bwd",
             "bn_act_pool_fwd": "_bn_act_pool_fwd", "bn_act_pool_bwd": "_bn_act_pool_bwd",
             "conv3d_dgrad_bnsums_ax": "_conv_dgrad_bnsums", "conv3d_wgrad_pro_ax": "_conv_wgrad_pro", "stem_wgrad_bnbwd_f32": "_stem_wgrad_bnbwd",
             "norm_act_bwd_apply_ax": "_norm_act_bwd_apply", "bn_fold_": "_conv_fwd_folded", "conv3d_fwd_fused_": "_conv_fwd_folded",
             "convt3d_k2s2_fwd": "_convt_k2s2_fwd"}


@pytest.mark.parametrize("stem", sorted(LAUNCHERS))
def test_each_norm_act_pool_entry_is_named_by_its_launcher_alone(stem):
    src, pattern = _source("functional.py"), '"mi355seg_' + stem
    hits = [m.start() for m in re.finditer(pattern, src)]
    assert len(hits) == 1, f"{pattern} occurs {len(hits)} times in functional.py"
    begin = src.index(f"\ndef {LAUNCHERS[stem]}(")
    assert begin < hits[0] < src.index("\n\n\n", begin + 1), f"{pattern} is named outside {LAUNCHERS[stem]}"
    assert not re.search(pattern, _source("custom_ops.py"))
    assert not re.search(r"mi355seg_(norm|maxpool2|upsample2|act)_", _source("custom_ops.py"))


@pytest.mark.parametrize("node,names", [(F._Conv3d, F._CONV3D_ARGS), (F._ConvBnAct, F._CONV_BN_ACT_ARGS),
                                        (F._DoubleConvBnAct, F._DOUBLE_CONV_BN_ACT_ARGS)], ids=lambda v: getattr(v, "__name__", ""))
def test_backward_results_are_named_after_the_forward_parameters(no_library, node, names):
    """A node's backward fills its result by parameter name (F._grads): the name list must be forward's parameters after ctx, in order."""
    assert list(names) == list(inspect.signature(node.forward).parameters)[1:]
    assert F._grads(names, **{names[0]: 1, names[-1]: 2}) == (1,) + (None,) * (len(names) - 2) + (2,)
    with pytest.raises(ValueError):
        F._grads(names, no_such_parameter=1)


def test_concat_out_is_the_slice_concat_base_recognises():
    lead, dtype = (1, 2, 3, 4), torch.float32
    full, y, pitch = F._concat_out(lead, 0, 10, dtype, "cpu")
    assert full is None and tuple(y.shape) == lead + (10,) and y.is_contiguous() and y._base is None and pitch == 10
    full, y, pitch = F._concat_out(lead, 6, 10, torch.bfloat16, "cpu")
    assert tuple(full.shape) == lead + (16,) and full.is_contiguous() and full.dtype == torch.bfloat16 and pitch == 16
    assert tuple(y.shape) == lead + (10,) and y.stride(3) == 16 and y.data_ptr() == full.data_ptr() + 6 * full.element_size()
    assert F._concat_base(y, 6, lead, torch.bfloat16) is full


def test_opt_view_of_an_absent_tensor(no_library):
    assert F._opt_view(None, "residual") == (None, 0)


def test_unread_fusion_switches_are_gone():
    src = open(os.path.join(os.path.dirname(os.path.abspath(mi355seg.functional.__file__)), "functional.py")).read()
    for name in ("RES_EPILOGUE", "CAT_FUSION", "STEM_FUSION", "HEAD_FUSION", "POOL_FUSION"):
        assert "MI355SEG_NO_" + name not in src
    assert set(re.findall(r"MI355SEG_NO_\w+", src)) == {"MI355SEG_NO_PREPACK", "MI355SEG_NO_PRO_FUSION", "MI355SEG_NO_MASK_POOL", "MI355SEG_NO_GEMM_PAIRS"}
