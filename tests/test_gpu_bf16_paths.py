"""Every branch of the bf16-storage Conv3d / ConvTranspose3d k2 s2 dispatch (csrc/conv_bf16_api.hip, csrc/convt_api.inc) against an
fp64 convolution of the same bf16-rounded activations, by name.

Each row is a small geometry that satisfies the predicate of one rung of FWD_B16 / DGRAD_B16 / WGRAD_B16 and fails the rungs in front
of it; after every call ``mi355seg_last_conv_path()`` names the branch (MI355SEG_PATH_B16_*: family, tiles, K form), so a row that stops
reaching its branch fails with the name of the one it reached.  The conventions are those of test_gpu_conv_paths.py:

  * the entry points are called through the C ABI on seeded tensors; every output lands in a buffer of 7.0 at pitch > channels with
    guard rows in front and behind, every input has NaN in its pad columns and guard rows;
  * the workspace is exactly mi355seg_conv3d_ws_bytes_bf16 / mi355seg_convt3d_k2s2_ws_bytes, cut from a larger buffer whose next
    1 MiB must come back untouched;
  * ONE reference per row: fp64 on the bf16-rounded activations with the weights as the reported family uses them -- rounded to bf16
    where it packs bf16 weights for the matrix cores (ROUNDS_WEIGHTS: igemm, gather, head2, stem1k5, stem4, headpw, the ConvT direct
    and igemm forms; read off pack_wq_*_kernel / pack_wq_lowp_body / the kernels' own staging loops), the fp32 masters where the
    kernel multiplies fp32 weights (stem, head, tinypw, the ConvT plain kernels, the cast fall-back);
  * the witness is ATen-CPU fp32 on the same rounded inputs, rounded once to bf16; kernel error, witness error and the
    error-to-bound ratio are printed per output (pytest -rA).

Bounds (those of test_gpu_bf16.py, unchanged): stored bf16 outputs  2^-8 |ref| + 4e-6 sqrt(K)  (K = k^3 Cin forward, k^3 Cout input
gradient; ConvT: sqrt(Cin) forward, 4e-5 flat for the input gradient); dw  2e-5 max(max |dw|, sqrt(nv)); db  1e-4 sqrt(nv).  The
activations of the fused forward are 1-Lipschitz, so the same bound holds behind them.

Statistics (stats_sum / stats_sq of mi355seg_conv3d_fwd_bf16) have TWO definitions, and each row names the one its branch uses:
  * "stored": split-K, every conv_stats_tail<bf16> family and the small stems sum the stored, rounded y through channel_sums -- held
    against the fp64 sums of exactly the y that came back, bound 2^-22 sum |addend| (the column-sum bar of test_gpu_norm_paths.py);
  * "acc": the whole-K igemm / b16s / gather epilogues sum the unrounded fp32 accumulators, and the cast fall-back sums the fp32 y of the
    staged call -- held against the fp64 sums of the unrounded reference y*, with a = 4e-6 sqrt(K) per element:
    |S1 - S1*| <= n a + 2^-22 sum |y*|,  |S2 - S2*| <= 2 a sum |y*| + n a^2 + 2^-22 sum y*^2.
  The mean / variance the two definitions give (mean = S1 / n, var = S2 / n - mean^2, as mi355seg_norm_stats_from_sums_f32) are
  printed side by side per row: the gap is the deviation from the reference framework, whose BatchNorm reads the stored tensor.

What the grading changed in the library: split K is chosen only when the written tensor is aligned to the four-element
store of splitk_reduce_kernel (rows y+1/2/4-*, dx+1/2/4-*, gather-y+*, gather-dx+*), and channel_sums on bf16 tensors combines the row
slots of colreduce2_kernel in fp64: with the fp32 chain the "stored" sums of squares of the narrow forwards (rows stem / headpw / head) came out at 1.33 / 1.68 / 1.93
of the 2^-22 bar while the ATen-CPU fp32 sum of the same values stood at 0.31 / 0.24 / 0.31 of it; the bar was left where it is.

Codes of the bf16 block no row reaches (UNREACHABLE below, each with the predicate that shadows it):
  * B16_WGRAD_LOWP_SWAPPED -- conv_wgrad_lowp forms ``swap`` only under ``math == MATH_X3 && x3_f16()``: the swapped-role wide kernel
    has no bf16-tensor instantiation, and Cin % 64 == 0 with Cout = 32 runs the narrow kernel.
"""
import functools
import re
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as TF

from stream_grading import (ACT_ELU, ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, EPS16, HEADER, SENTINEL, SUM_BOUND, Buf, Flat, Workspace, act_both, pick,
                            rnd, stream)

gpu = pytest.mark.gpu           # per test: the table check at the end of the file needs no GPU and runs with -m "not gpu"

BF = torch.bfloat16
ACC = 4e-6                      # x sqrt(K): fp32 accumulation of K bf16 products (test_gpu_bf16.py)
DW_BOUND, DB_BOUND = 2e-5, 1e-4
CONVT_DGRAD_ACC = 4e-5          # test_conv_transpose_k2s2_bf16
PAD = 8                         # pitch - channels of the 16-byte staged families


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mi355seg
    mi355seg.lib()
    return mi355seg


@pytest.fixture(autouse=True)
def end_the_session_after_a_gpu_fault():
    """A kernel fault leaves the device context unusable: nothing more is started on the GPU after one (exit code 3)."""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"GPU fault, session ended: {e}", returncode=3)


@functools.lru_cache(maxsize=None)
def b16_codes():
    """name (without MI355SEG_PATH_) -> value of every code of the header's bf16 block"""
    return {k: int(v) for k, v in re.findall(r"MI355SEG_PATH_(B16_\w+)\s*=\s*(\d+)", open(HEADER).read())}


def last_path(L):
    code = L.query("mi355seg_last_conv_path")
    names = {v: k for k, v in b16_codes().items()}
    return names.get(code, f"code {code} (not of the bf16 block)")


def expect_path(L, want, what):
    got = last_path(L)
    assert got == want, f"{what} ran {got}, the row was built for {want}"


# families that pack bf16 weights for the matrix cores; every other code multiplies the fp32 masters
ROUNDS_WEIGHTS = {"IGEMM_S", "IGEMM_S_SPLITK", "IGEMM_G", "IGEMM_G_SPLITK", "GATHER", "GATHER_SPLITK", "GATHER_PHASES", "HEAD2", "STEM1K5", "STEM4", "HEADPW",
                  "K2S2_CONVT", "DIRECT", "STREAM", "MFMA"}


def rounds(code):
    return re.sub(r"B16_(CONVT_)?(FWD|DGRAD)_", "", code) in ROUNDS_WEIGHTS


# name, (N, D, H, W, Cin, Cout, k, s, p), pitch - channels of x and of y, expected forward / input-gradient / weight-gradient code
# (a pair: accumulate 0, 1), set_b16_tiles, set_wgrad_wide, element offset of the x-side tensor (x, dx) and of the y-side one (y, dy)
Row = namedtuple("Row", "name geom ex ey fwd dgrad wgrad tiles wide xo yo", defaults=(0, 1, 0, 0))
F, G_, W_ = "B16_FWD_", "B16_DGRAD_", "B16_WGRAD_"

G_RAGGED = (1, 5, 7, 9, 32, 32, 3, 1, 1)        # ragged on every axis; Cin = Cout = 32: two K chunks, whole K in both directions
G_SPLIT = (2, 5, 6, 20, 64, 64, 3, 1, 1)        # two samples; Cin = Cout = 64: four K chunks and < 512 tiles, split K in both directions
G_SUBTILE = (1, 2, 3, 5, 32, 32, 3, 1, 1)       # smaller than one tile of either tiling
G_K5 = (1, 6, 9, 18, 32, 64, 5, 1, 2)           # k5: whole K forward (Cin = 32), split K input gradient (Cout = 64)
G_K1 = (1, 6, 6, 12, 64, 32, 1, 1, 0)           # k1: one 64-channel chunk
G_PW = (2, 5, 7, 9, 96, 48, 1, 1, 0)            # k1, Cout % 32 != 0: no forward igemm; the input gradient has Nc = 96
G_GATHER = (1, 16, 16, 16, 32, 64, 3, 2, 1)     # k3 s2: 54 chunks, split K; eight input-gradient phases of one plan
G_GATHER_ODD = (2, 9, 11, 18, 16, 32, 3, 2, 1)  # 27 chunks (odd): whole K; Cin = 16 is no N-tile of the gather input gradient
G_GATHER_W17 = (1, 8, 9, 17, 32, 64, 3, 2, 1)   # W = 17: the phases' base widths 9 | 8 pick BX = 16 | 8 -> one launch per phase
G_K2S2 = (1, 16, 16, 32, 16, 32, 2, 2, 0)       # V-Net down-convolution: dgrad = ConvT forward, wgrad = ConvT wgrad with swapped roles
G_STEM4, G_STEM4_RAGGED, G_STEM4_SUB = (1, 8, 12, 16, 4, 32, 3, 1, 1), (2, 9, 7, 45, 4, 32, 3, 1, 1), (1, 2, 2, 3, 4, 32, 3, 1, 1)
G_STEM = (1, 5, 6, 7, 1, 8, 3, 1, 1)
G_HEADPW, G_HEADPW4, G_HEADPW_SUB = (1, 5, 7, 9, 32, 2, 1, 1, 0), (2, 8, 8, 16, 32, 4, 1, 1, 0), (1, 1, 2, 3, 32, 4, 1, 1, 0)
G_HEAD256 = (1, 4, 4, 8, 256, 4, 1, 1, 0)       # Cin > 128: off headpw, on the plain head
G_HEAD2, G_HEAD2_RAGGED, G_HEAD2_SUB = (1, 8, 8, 16, 32, 2, 5, 1, 2), (2, 9, 7, 45, 32, 2, 5, 1, 2), (1, 2, 3, 5, 32, 2, 5, 1, 2)
G_HEADK = (1, 8, 8, 16, 16, 2, 5, 1, 2)         # Cin % 32 != 0: off head2, the named cast rung (headk_wgrad behind the fall-back)
G_STEM1K5, G_STEM1K5_RAGGED, G_STEM1K5_SUB = (1, 8, 8, 16, 1, 16, 5, 1, 2), (2, 9, 7, 45, 1, 16, 5, 1, 2), (1, 1, 1, 3, 1, 16, 5, 1, 2)
G_TINY = (2, 6, 8, 10, 2, 2, 1, 1, 0)
G_SMALLCOUT = (1, 8, 8, 16, 32, 4, 5, 1, 2)
G_RAGGED_CH = (1, 6, 6, 6, 24, 40, 3, 1, 1)

CAST3 = (F + "CAST", G_ + "CAST", W_ + "CAST")
CONV_ROWS = [
    # ---- igemm: both tilings x both K forms; ragged extents, two samples, a volume below one tile
    Row("b16s-whole", G_RAGGED, PAD, PAD, F + "IGEMM_S", G_ + "IGEMM_S", W_ + "LOWP_NARROW", tiles=1),
    Row("generic-whole", G_RAGGED, PAD, PAD, F + "IGEMM_G", G_ + "IGEMM_G", W_ + "LOWP_NARROW", tiles=2),
    Row("b16s-split", G_SPLIT, PAD, PAD, F + "IGEMM_S_SPLITK", G_ + "IGEMM_S_SPLITK", W_ + "LOWP_NARROW", tiles=1),
    Row("generic-split", G_SPLIT, PAD, PAD, F + "IGEMM_G_SPLITK", G_ + "IGEMM_G_SPLITK", W_ + "LOWP_NARROW", tiles=2),
    Row("b16s-subtile", G_SUBTILE, PAD, PAD, F + "IGEMM_S", G_ + "IGEMM_S", W_ + "LOWP_NARROW", tiles=1),
    Row("generic-subtile", G_SUBTILE, PAD, PAD, F + "IGEMM_G", G_ + "IGEMM_G", W_ + "LOWP_NARROW", tiles=2),
    Row("b16s-k5", G_K5, PAD, PAD, F + "IGEMM_S", G_ + "IGEMM_S_SPLITK", W_ + "LOWP_NARROW", tiles=1),
    Row("generic-k5", G_K5, PAD, PAD, F + "IGEMM_G", G_ + "IGEMM_G_SPLITK", W_ + "LOWP_NARROW", tiles=2),
    Row("k1", G_K1, PAD, PAD, F + "IGEMM_G", G_ + "IGEMM_G", W_ + "PW_LOWP"),
    Row("wide-wgrad", G_SPLIT, PAD, PAD, F + "IGEMM_G_SPLITK", G_ + "IGEMM_G_SPLITK", W_ + "LOWP_WIDE", tiles=2, wide=2),
    Row("wide-wgrad-k5", G_K5, PAD, PAD, F + "IGEMM_G", G_ + "IGEMM_G_SPLITK", W_ + "LOWP_WIDE", tiles=2, wide=2),
    # ---- the written tensor off its 8-byte store: no rung's `aligned` looks at it.  conv_b16s.hip declines (b16s_plan asks y % 16), the
    # generic whole-K epilogue stores element by element; splitk_reduce_kernel's st4 needs 8 bytes, so offsets 1 and 2 keep the whole K
    *[Row(f"y+{o}-whole", G_RAGGED, PAD, PAD, F + "IGEMM_G", G_ + "CAST", W_ + "CAST", yo=o) for o in (1, 2, 4)],
    *[Row(f"y+{o}-split", G_SPLIT, PAD, PAD, F + ("IGEMM_G_SPLITK" if o == 4 else "IGEMM_G"), G_ + "CAST", W_ + "CAST", yo=o) for o in (1, 2, 4)],
    *[Row(f"dx+{o}-whole", G_RAGGED, PAD, PAD, F + "CAST", G_ + "IGEMM_G", W_ + "CAST", xo=o) for o in (1, 2, 4)],
    *[Row(f"dx+{o}-split", G_SPLIT, PAD, PAD, F + "CAST", G_ + ("IGEMM_G_SPLITK" if o == 4 else "IGEMM_G"), W_ + "CAST", xo=o) for o in (1, 2, 4)],
    # ---- gather igemm
    Row("gather-split", G_GATHER, PAD, PAD, F + "GATHER_SPLITK", G_ + "GATHER_PHASES", W_ + "LOWP_NARROW"),
    Row("gather-whole", G_GATHER_ODD, PAD, PAD, F + "GATHER", G_ + "CAST", W_ + "GWGRAD"),
    Row("gather-per-phase", G_GATHER_W17, PAD, PAD, F + "GATHER_SPLITK", G_ + "GATHER", W_ + "LOWP_NARROW"),
    Row("gather-subtile", (1, 3, 3, 9, 16, 32, 3, 2, 1), PAD, PAD, F + "GATHER", G_ + "CAST", W_ + "GWGRAD"),                     # 2 x 2 x 5 outputs
    Row("gather-phases-subtile", (1, 2, 2, 8, 32, 32, 3, 2, 1), PAD, PAD, F + "GATHER_SPLITK", G_ + "GATHER_PHASES", W_ + "LOWP_NARROW"),   # 1 x 1 x 4 per phase
    *[Row(f"gather-y+{o}", G_GATHER, PAD, PAD, F + ("GATHER_SPLITK" if o == 4 else "GATHER"), G_ + "CAST", W_ + "CAST", yo=o) for o in (1, 2, 4)],
    *[Row(f"gather-dx+{o}", G_GATHER, PAD, PAD, F + "CAST", G_ + "GATHER_PHASES", W_ + "CAST", xo=o) for o in (1, 2, 4)],
    # ---- k2 s2: both aliases of the ConvT kernels (NB_CONVT, NB_K2S2W; the latter cannot accumulate)
    Row("k2s2", G_K2S2, PAD, PAD, F + "GATHER_SPLITK", G_ + "K2S2_CONVT", (W_ + "K2S2_CONVT", W_ + "CAST")),
    Row("k2s2-pitch4", G_K2S2, 4, 4, F + "CAST", G_ + "CAST", W_ + "GWGRAD"),
    # ---- small-channel stems and heads
    Row("stem4", G_STEM4_RAGGED, 0, PAD, F + "STEM4", G_ + "CAST", W_ + "STEM4"),
    Row("stem4-subtile", G_STEM4_SUB, 0, PAD, F + "STEM4", G_ + "CAST", W_ + "STEM4"),
    Row("stem4-x-pitch8", G_STEM4, 4, PAD, F + "STEM", G_ + "CAST", W_ + "STEM"),
    Row("stem", G_STEM, 1, PAD, F + "STEM", G_ + "CAST", W_ + "STEM"),
    Row("headpw", G_HEADPW, PAD, 2, F + "HEADPW", G_ + "HEAD", W_ + "HEADPW"),
    Row("headpw-cout4", G_HEADPW4, PAD, 4, F + "HEADPW", G_ + "HEAD", W_ + "HEADPW"),
    Row("headpw-subtile", G_HEADPW_SUB, PAD, 4, F + "HEADPW", G_ + "HEAD", W_ + "HEADPW"),
    Row("headpw-x+4", G_HEADPW, PAD, 2, F + "HEAD", G_ + "HEAD", W_ + "HEAD", xo=4),           # x % 16 == 8: headpw -> plain head (its own test is x % 8)
    Row("head-cin256", G_HEAD256, PAD, 4, F + "HEAD", G_ + "HEAD", W_ + "HEAD"),
    Row("head2", G_HEAD2_RAGGED, PAD, 2, F + "HEAD2", G_ + "HEAD2", W_ + "HEAD2"),
    Row("head2-subtile", G_HEAD2_SUB, PAD, 2, F + "HEAD2", G_ + "HEAD2", W_ + "HEAD2"),
    Row("headk-cast", G_HEADK, PAD, 2, *CAST3),
    Row("stem1k5", G_STEM1K5_RAGGED, 0, PAD, F + "STEM1K5", G_ + "CAST", W_ + "STEM1K5"),
    Row("stem1k5-subtile", G_STEM1K5_SUB, 0, PAD, F + "STEM1K5", G_ + "CAST", W_ + "STEM1K5"),
    Row("stem1k5-y-pitch20", G_STEM1K5, 0, 4, F + "CAST", G_ + "CAST", W_ + "SMALLCIN"),
    Row("tinypw", G_TINY, 1, 1, F + "TINYPW", G_ + "TINYPW", W_ + "TINYPW", xo=1, yo=1),
    # ---- pointwise weight gradients, the small-Cout one, the cast fall-back
    Row("pw-lowp", G_PW, PAD, PAD, F + "CAST", G_ + "IGEMM_G", W_ + "PW_LOWP"),
    Row("pw-mfma", G_PW, PAD, PAD, F + "CAST", G_ + "IGEMM_G", W_ + "PW_MFMA", xo=4),
    Row("smallcout", G_SMALLCOUT, PAD, 4, F + "CAST", G_ + "CAST", W_ + "SMALLCOUT"),
    Row("ragged-channels", G_RAGGED_CH, 0, 0, F + "CAST", G_ + "CAST", W_ + "GWGRAD"),
    Row("x+4", G_RAGGED, PAD, PAD, F + "CAST", G_ + "IGEMM_G", W_ + "CAST", xo=4),              # igemm -> cast: x % 16 == 8
]

# name, geom, ex, ey, set_b16_tiles, forward code, which sums the branch forms
STATS_ROWS = [
    ("b16s-whole", G_RAGGED, PAD, PAD, 1, F + "IGEMM_S", "acc"),
    ("generic-whole", G_RAGGED, PAD, PAD, 2, F + "IGEMM_G", "acc"),
    ("b16s-split", G_SPLIT, PAD, PAD, 1, F + "IGEMM_S_SPLITK", "stored"),
    ("generic-split", G_SPLIT, PAD, PAD, 2, F + "IGEMM_G_SPLITK", "stored"),
    ("gather-whole", G_GATHER_ODD, PAD, PAD, 0, F + "GATHER", "acc"),
    ("gather-split", G_GATHER, PAD, PAD, 0, F + "GATHER_SPLITK", "stored"),
    ("head2", G_HEAD2_RAGGED, PAD, 2, 0, F + "HEAD2", "stored"),
    ("stem1k5", G_STEM1K5_RAGGED, 0, PAD, 0, F + "STEM1K5", "stored"),
    ("stem4", G_STEM4_RAGGED, 0, PAD, 0, F + "STEM4", "stored"),
    ("stem", G_STEM, 1, PAD, 0, F + "STEM", "stored"),
    ("headpw", G_HEADPW4, PAD, 4, 0, F + "HEADPW", "stored"),
    ("head", G_HEAD256, PAD, 4, 0, F + "HEAD", "stored"),
    ("tinypw", G_TINY, 1, 1, 0, F + "TINYPW", "stored"),
    ("cast", G_RAGGED_CH, 0, 0, 0, F + "CAST", "acc"),
]

FUSED_ROWS = [("b16s-whole", G_RAGGED, 1, F + "IGEMM_S"), ("generic-whole", G_RAGGED, 2, F + "IGEMM_G"),
              ("b16s-split", G_SPLIT, 1, F + "IGEMM_S_SPLITK"), ("generic-split", G_SPLIT, 2, F + "IGEMM_G_SPLITK")]

# name, (N, D, H, W, Cin, Cout), ex, ey, forward / input-gradient / weight-gradient code
CT = "B16_CONVT_"
CONVT_ROWS = [
    ("stream-k256", (2, 8, 8, 8, 256, 64), PAD, PAD, CT + "FWD_STREAM", CT + "DGRAD_DIRECT", CT + "WGRAD_LOWP"),       # input gradient: K = 8 Cout = 512, GEMM form
    ("stream-both", (1, 8, 8, 8, 64, 16), PAD, PAD, CT + "FWD_STREAM", CT + "DGRAD_STREAM", CT + "WGRAD_LOWP"),        # K = 64 | 128, 512 voxels
    ("direct-ragged", (1, 6, 6, 6, 64, 32), PAD, PAD, CT + "FWD_DIRECT", CT + "DGRAD_DIRECT", CT + "WGRAD_LOWP"),      # 216 voxels: partial tiles, GEMM form
    ("direct-subtile", (1, 1, 2, 3, 64, 32), PAD, PAD, CT + "FWD_DIRECT", CT + "DGRAD_DIRECT", CT + "WGRAD_LOWP"),     # six voxels
    ("mfma", (2, 3, 5, 8, 32, 16), PAD, PAD, CT + "FWD_MFMA", CT + "DGRAD_MFMA", CT + "WGRAD_LOWP"),                   # K = 32: off the direct kernels
    ("mfma-wgrad", (1, 3, 5, 4, 24, 20), 4, 4, CT + "FWD_PLAIN", CT + "DGRAD_PLAIN", CT + "WGRAD_MFMA"),               # Cin % 32 != 0: off convt_wgrad_lowp
    ("plain", (1, 3, 5, 4, 6, 10), 2, 2, CT + "FWD_PLAIN", CT + "DGRAD_PLAIN", CT + "WGRAD_PLAIN"),
]

UNREACHABLE = {"B16_WGRAD_LOWP_SWAPPED": "conv_wgrad_lowp: swap needs math == MATH_X3 && x3_f16()"}


# ----------------------------------------------------------------------------- references, once per (geometry, weight treatment)
class Ref:
    pass


def r16(t):
    return t.to(BF).double()


def ncdhw(t):
    return t.permute(0, 4, 1, 2, 3)


def cl(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


@functools.lru_cache(maxsize=None)
def conv_inputs(geom, shifted=False):
    N, D, H, W, Cin, Cout, k, s, p = geom
    r = Ref()
    r.x = rnd(N, D, H, W, Cin, seed=1).to(BF)                     # what the tensors hold
    r.w = rnd(Cout, Cin, k, k, k, seed=2, scale=(2.0 / (Cin * k ** 3)) ** 0.5)
    r.b = rnd(Cout, seed=3, scale=0.1)
    if shifted:                                                   # channel 0: mean 50, std about 0.5 (SHIFTED_STATS_CASE of test_gpu_conv_paths.py)
        r.w[0] *= 0.5 / float((r.w[0] ** 2).sum().sqrt())
        r.b[0] = 50.0
    r.out = tuple((e + 2 * p - k) // s + 1 for e in (D, H, W))
    r.g = rnd(N, *r.out, Cout, seed=4).to(BF)
    r.nv = N * r.out[0] * r.out[1] * r.out[2]
    return r


@functools.lru_cache(maxsize=None)
def conv_reference(geom, rounded, shifted=False):
    """fp64 forward and gradients of one geometry on the bf16 activations, with the weights rounded to bf16 or left as fp32 masters;
    the fp32 ATen run of the same graph, rounded once to bf16, is the witness.  Computed once, shared, never modified."""
    N, D, H, W, Cin, Cout, k, s, p = geom
    i = conv_inputs(geom, shifted)
    r = Ref()
    res = {}
    for dt in (torch.float64, torch.float32):
        xd = ncdhw(i.x).to(dt).requires_grad_(True)
        wd = (i.w.to(BF) if rounded else i.w).to(dt).clone().requires_grad_(True)         # (a copy: the cached inputs stay leaves without a graph)
        y = TF.conv3d(xd, wd, i.b.to(dt), stride=s, padding=p)
        y.backward(ncdhw(i.g).to(dt))
        res[dt] = (cl(y.detach()), cl(xd.grad), wd.grad)
    r.y, r.dx, r.dw = res[torch.float64]
    r.db = i.g.double().reshape(-1, Cout).sum(0)
    wy, wdx, wdw = res[torch.float32]
    r.wit_y, r.wit_dx, r.wit_dw = r16(wy), r16(wdx), wdw.double()
    r.wit_db = i.g.float().reshape(-1, Cout).sum(0).double()
    return r


@functools.lru_cache(maxsize=None)
def convt_reference(geom, rounded):
    N, D, H, W, Cin, Cout = geom
    r = Ref()
    r.x = rnd(N, D, H, W, Cin, seed=1).to(BF)
    r.w = rnd(Cin, Cout, 2, 2, 2, seed=2, scale=(1.0 / Cin) ** 0.5)
    r.b = rnd(Cout, seed=3, scale=0.1)
    r.g = rnd(N, 2 * D, 2 * H, 2 * W, Cout, seed=4).to(BF)
    res = {}
    for dt in (torch.float64, torch.float32):
        xd = ncdhw(r.x).to(dt).requires_grad_(True)
        wd = (r.w.to(BF) if rounded else r.w).to(dt).clone().requires_grad_(True)
        y = TF.conv_transpose3d(xd, wd, r.b.to(dt), stride=2)
        y.backward(ncdhw(r.g).to(dt))
        res[dt] = (cl(y.detach()), cl(xd.grad), wd.grad)
    r.y, r.dx, r.dw = res[torch.float64]
    r.db = r.g.double().reshape(-1, Cout).sum(0)
    wy, wdx, wdw = res[torch.float32]
    r.wit_y, r.wit_dx, r.wit_dw = r16(wy), r16(wdx), wdw.double()
    r.wit_db = r.g.float().reshape(-1, Cout).sum(0).double()
    return r


# ----------------------------------------------------------------------------- graders
def grade_stored(name, branch, what, got, ref, wit, acc_abs):
    """A stored bf16 tensor: |got - ref| <= 2^-8 |ref| + acc_abs per element."""
    got = got.reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name} {what} ({branch}): not finite"
    bound = EPS16 * ref.abs() + acc_abs
    err, werr = (got - ref).abs(), (wit - ref).abs()
    ratio, wratio = float((err / bound).max()), float((werr / bound).max())
    print(f"{name:22s} {branch:28s} {what:10s} kernel {float(err.max()):9.2e}  witness {float(werr.max()):9.2e}  err/bound {ratio:6.3f}  witness/bound {wratio:6.3f}")
    assert ratio <= 1.0, f"{name} {what} ({branch}): {ratio:.3f} of the bound (witness {wratio:.3f} of it), {int((err > bound).sum())} elements over"


def grade_flat(name, branch, what, got, ref, wit, bound):
    """An fp32 gradient: max |got - ref| <= bound."""
    got = got.reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name} {what} ({branch}): not finite"
    err, werr = float((got - ref).abs().max()), float((wit - ref).abs().max())
    print(f"{name:22s} {branch:28s} {what:10s} kernel {err:9.2e}  witness {werr:9.2e}  err/bound {err / bound:6.3f}  witness/bound {werr / bound:6.3f}")
    assert err <= bound, f"{name} {what} ({branch}): {err:.3e}, bound {bound:.3e} (witness {werr:.3e})"


def per_acc(spec):
    return (spec, spec) if isinstance(spec, str) else tuple(spec)


def row_id(r):
    return r.name if isinstance(r, Row) else r[0]


class Modes:
    """set_b16_tiles / set_wgrad_wide for one row, restored on the way out"""

    def __init__(self, seg, tiles=0, wide=1):
        self.seg, self.tiles, self.wide = seg, tiles, wide

    def __enter__(self):
        self.seg.set_b16_tiles(self.tiles)
        self.seg.set_wgrad_wide(self.wide)

    def __exit__(self, *exc):
        self.seg.set_b16_tiles(0)
        self.seg.set_wgrad_wide(1)


def fused_refused(L, xb, w, yb_args, geom, ws, what):
    """mi355seg_conv3d_fwd_fused_bf16 on a call whose ladder does not end on the igemm: the documented argument error, nothing launched
    (the output buffer and the workspace band keep their fill, the recorded branch stays)."""
    from mi355seg import Mi355SegError
    Cout = geom[5]
    y = Buf(*yb_args)
    one = torch.ones(Cout, device="cuda")
    before = L.query("mi355seg_last_conv_path")
    with pytest.raises(Mi355SegError, match=r"rc=-1.*no fused form"):
        L.call("mi355seg_conv3d_fwd_fused_bf16", xb.ptr, xb.ld, w.data_ptr(), one.data_ptr(), one.data_ptr(), ACT_RELU, 0.0, y.ptr, y.ld, *geom, ws.ptr, ws.n, stream())
    assert L.query("mi355seg_last_conv_path") == before, f"{what}: a refused fused call recorded a branch"
    assert bool((y.buf == SENTINEL).all()), f"{what}: a refused fused call wrote to y"
    ws.check(what)


@gpu
@pytest.mark.parametrize("row", CONV_ROWS, ids=row_id)
def test_conv3d_bf16_branch_against_fp64(seg, row):
    """Forward, input gradient and weight gradient (accumulate = 0 over NaN, = 1 over seeded values) of one row: the reported branch,
    the values against the one reference its family calls for, guards, pad columns and the workspace band."""
    geom = row.geom
    N, D, H, W, Cin, Cout, k, s, p = geom
    L = seg.lib()
    i = conv_inputs(geom)
    rows_in, rows_out = N * D * H * W, i.nv
    w, b = i.w.cuda(), i.b.cuda()
    ws = Workspace(L.query("mi355seg_conv3d_ws_bytes_bf16", *geom))
    xin = Buf(rows_in, Cin, row.ex, "bf16", data=i.x.cuda(), off=row.xo)
    gin = Buf(rows_out, Cout, row.ey, "bf16", data=i.g.cuda(), off=row.yo)
    st = stream()
    with Modes(seg, row.tiles, row.wide):
        # ---- forward
        y = Buf(rows_out, Cout, row.ey, "bf16", off=row.yo)
        L.call("mi355seg_conv3d_fwd_bf16", xin.ptr, xin.ld, w.data_ptr(), b.data_ptr(), y.ptr, y.ld, *geom, None, None, ws.ptr, ws.n, st)
        expect_path(L, row.fwd, f"{row.name}: forward")
        ws.check("forward")
        ref = conv_reference(geom, rounds(row.fwd))
        grade_stored(row.name, row.fwd, "y", y.check("forward"), ref.y, ref.wit_y, ACC * (k ** 3 * Cin) ** 0.5)
        is_igemm = row.fwd.startswith(F + "IGEMM")
        if row.xo == 0:         # (the query sees pitches, not pointers)
            assert bool(L.query("mi355seg_conv3d_fused_supported_bf16", *geom, xin.ld, y.ld)) == is_igemm, f"{row.name}: fused_supported disagrees with {row.fwd}"
        if not is_igemm:
            fused_refused(L, xin, w, (rows_out, Cout, row.ey, "bf16", None, row.yo), geom, ws, f"{row.name}: fused forward")
        # ---- input gradient
        dx = Buf(rows_in, Cin, row.ex, "bf16", off=row.xo)
        L.call("mi355seg_conv3d_dgrad_bf16", gin.ptr, gin.ld, w.data_ptr(), dx.ptr, dx.ld, *geom, ws.ptr, ws.n, st)
        expect_path(L, row.dgrad, f"{row.name}: input gradient")
        ws.check("input gradient")
        ref = conv_reference(geom, rounds(row.dgrad))
        grade_stored(row.name, row.dgrad, "dx", dx.check("input gradient"), ref.dx, ref.wit_dx, ACC * (k ** 3 * Cout) ** 0.5)
        # ---- weight gradient: no weights enter it, the reference is the same under either treatment
        scale = float(ref.dw.abs().max())
        g0w = rnd(*ref.dw.shape, seed=5, scale=float(ref.dw.pow(2).mean().sqrt()))
        g0b = rnd(Cout, seed=6, scale=float(ref.db.pow(2).mean().sqrt()) + 1e-3)
        for accumulate, want in zip((0, 1), per_acc(row.wgrad)):
            dw, db = Flat(ref.dw.numel(), g0w if accumulate else None), Flat(Cout, g0b if accumulate else None)
            L.call("mi355seg_conv3d_wgrad_bf16", gin.ptr, gin.ld, xin.ptr, xin.ld, dw.ptr, db.ptr, *geom, accumulate, ws.ptr, ws.n, st)
            expect_path(L, want, f"{row.name}: weight gradient, accumulate {accumulate}")
            ws.check("weight gradient")
            add_w, add_b = (g0w.double(), g0b.double()) if accumulate else (0.0, 0.0)
            tag = "+G0" if accumulate else ""
            grade_flat(row.name, want, "dw" + tag, dw.check("weight gradient"), ref.dw + add_w, ref.wit_dw + add_w, DW_BOUND * max(scale, rows_out ** 0.5))
            grade_flat(row.name, want, "db" + tag, db.check("bias gradient"), ref.db + add_b, ref.wit_db + add_b, DB_BOUND * rows_out ** 0.5)
    xin.check("x"), gin.check("dy")         # (the inputs and their NaN surroundings are as they were)


def moments(S1, S2, n):
    mean = S1 / n
    return mean, (S2 / n - mean * mean).clamp_min(0.0)


@gpu
@pytest.mark.parametrize("row", STATS_ROWS, ids=row_id)
def test_conv3d_fwd_bf16_statistics_by_definition(seg, row):
    """stats_sum / stats_sq per forward branch, channel 0 shifted to mean 50 / std 0.5: against the definition the branch uses (see the
    module docstring); asking for them leaves y bit-identical."""
    name, geom, ex, ey, tiles, code, kind = row
    N, D, H, W, Cin, Cout, k, s, p = geom
    L = seg.lib()
    i = conv_inputs(geom, True)
    ref = conv_reference(geom, rounds(code), True)
    n = i.nv
    w, b = i.w.cuda(), i.b.cuda()
    ws = Workspace(L.query("mi355seg_conv3d_ws_bytes_bf16", *geom))
    xin = Buf(N * D * H * W, Cin, ex, "bf16", data=i.x.cuda())
    outs = []
    with Modes(seg, tiles):
        for stats in (True, False):
            y = Buf(n, Cout, ey, "bf16")
            ss = Flat(2 * Cout, dtype=torch.float64)
            L.call("mi355seg_conv3d_fwd_bf16", xin.ptr, xin.ld, w.data_ptr(), b.data_ptr(), y.ptr, y.ld, *geom,
                   ss.ptr if stats else None, ss.ptr + 8 * Cout if stats else None, ws.ptr, ws.n, stream())
            expect_path(L, code, f"{name}: forward {'with' if stats else 'without'} statistics")
            ws.check("forward")
            outs.append((y.check("forward"), ss.check("statistics")))
    (y, ss), (y_plain, _) = outs
    assert torch.equal(y, y_plain), f"{name} ({code}): asking for the statistics changed y"
    grade_stored(name, code, "y", y, ref.y, ref.wit_y, ACC * (k ** 3 * Cin) ** 0.5)
    S1, S2 = ss[:Cout], ss[Cout:]
    yk, ys = y.reshape(n, Cout), ref.y.reshape(n, Cout)
    a = ACC * (k ** 3 * Cin) ** 0.5
    if kind == "stored":
        want1, want2 = yk.sum(0), (yk * yk).sum(0)
        b1, b2 = SUM_BOUND * yk.abs().sum(0), SUM_BOUND * (yk * yk).sum(0)
    else:
        want1, want2 = ys.sum(0), (ys * ys).sum(0)
        b1 = n * a + SUM_BOUND * ys.abs().sum(0)
        b2 = 2 * a * ys.abs().sum(0) + n * a * a + SUM_BOUND * (ys * ys).sum(0)
    e1, e2 = float(((S1 - want1).abs() / b1).max()), float(((S2 - want2).abs() / b2).max())
    m_st, v_st = moments(yk.sum(0), (yk * yk).sum(0), n)             # what a BatchNorm that reads the stored tensor sees
    m_k, v_k = moments(S1, S2, n)
    print(f"{name:22s} {code:28s} {kind:6s} sum err/bound {e1:6.3f}  sum of squares err/bound {e2:6.3f}  |  against the stored tensor's moments: "
          f"|d mean| {float((m_k - m_st).abs().max()):9.2e}  |d var| / var {float(((v_k - v_st).abs() / v_st).max()):9.2e}  (channel 0: {float((v_k - v_st).abs()[0] / v_st[0]):9.2e})")
    assert e1 <= 1.0 and e2 <= 1.0, f"{name} ({code}, {kind}): statistics at {e1:.3f} / {e2:.3f} of their bounds"


@gpu
@pytest.mark.parametrize("act", [ACT_NONE, ACT_RELU, ACT_ELU, ACT_LRELU, ACT_SIGMOID], ids=["none", "relu", "elu", "lrelu", "sigmoid"])
@pytest.mark.parametrize("row", FUSED_ROWS, ids=row_id)
def test_conv3d_fwd_fused_bf16_against_fp64(seg, row, act):
    """act(conv(x, bf16(w * oscale)) + oshift): the pack kernels multiply the fp32 master by oscale[co] in fp32 and round the product to
    bf16 once (pack_wq_b16s_kernel, pack_wq_lowp_body); the activation sits in the epilogue (whole K) or in splitk_reduce_kernel."""
    name, geom, tiles, code = row
    N, D, H, W, Cin, Cout, k, s, p = geom
    L = seg.lib()
    i = conv_inputs(geom)
    osc, osh, slope = 1.0 + 0.2 * rnd(Cout, seed=7), 0.3 * rnd(Cout, seed=8), 0.01
    wq = (i.w * osc.view(-1, 1, 1, 1, 1)).to(BF)                  # one fp32 product, one rounding
    res = {}
    for dt in (torch.float64, torch.float32):
        z = cl(TF.conv3d(ncdhw(i.x).to(dt), wq.to(dt), osh.to(dt), stride=s, padding=p))
        res[dt] = pick(z, act_both(z, act, slope))
    want, wit = res[torch.float64], r16(res[torch.float32])
    ws = Workspace(L.query("mi355seg_conv3d_ws_bytes_bf16", *geom))
    xin = Buf(N * D * H * W, Cin, PAD, "bf16", data=i.x.cuda())
    y = Buf(i.nv, Cout, PAD, "bf16")
    w, oscg, oshg = i.w.cuda(), osc.cuda(), osh.cuda()
    with Modes(seg, tiles):
        assert L.query("mi355seg_conv3d_fused_supported_bf16", *geom, xin.ld, y.ld)
        L.call("mi355seg_conv3d_fwd_fused_bf16", xin.ptr, xin.ld, w.data_ptr(), oscg.data_ptr(), oshg.data_ptr(), act, slope, y.ptr, y.ld, *geom, ws.ptr, ws.n, stream())
        expect_path(L, code, f"{name}: fused forward")
    ws.check("fused forward")
    grade_stored(f"fused-{name}-act{act}", code, "y", y.check("fused forward"), want, wit, ACC * (k ** 3 * Cin) ** 0.5)


@gpu
@pytest.mark.parametrize("row", CONVT_ROWS, ids=row_id)
def test_conv_transpose3d_k2s2_bf16_branch_against_fp64(seg, row):
    """fwd, fwd_ax, dgrad and wgrad of ConvTranspose3d k2 s2 on bf16 tensors at a pitch; the weight gradient overwrites NaN."""
    name, geom, ex, ey, pf, pd, pw = row
    N, D, H, W, Cin, Cout = geom
    L = seg.lib()
    from mi355seg import Mi355SegError
    i = convt_reference(geom, True)           # (the inputs are the same under either treatment)
    rows_in, rows_out = N * D * H * W, 8 * N * D * H * W
    w, b = i.w.cuda(), i.b.cuda()
    ws = Workspace(L.query("mi355seg_convt3d_k2s2_ws_bytes", *geom))
    xin = Buf(rows_in, Cin, ex, "bf16", data=i.x.cuda())
    gin = Buf(rows_out, Cout, ey, "bf16", data=i.g.cuda())
    st = stream()
    ref = convt_reference(geom, rounds(pf))
    ys = []
    for entry, extra in (("mi355seg_convt3d_k2s2_fwd_bf16", ()), ("mi355seg_convt3d_k2s2_fwd_ax_bf16", (None,))):
        y = Buf(rows_out, Cout, ey, "bf16")
        L.call(entry, xin.ptr, xin.ld, w.data_ptr(), b.data_ptr(), y.ptr, y.ld, *geom, *extra, ws.ptr, ws.n, st)
        expect_path(L, pf, f"{name}: {entry}")
        ws.check("forward")
        ys.append(y.check("forward"))
    grade_stored(name, pf, "y", ys[0], ref.y, ref.wit_y, ACC * Cin ** 0.5)
    assert torch.equal(ys[0], ys[1]), f"{name}: fwd_ax without a slot differs from fwd"
    y, slot = Buf(rows_out, Cout, ey, "bf16"), torch.zeros(1, device="cuda")
    with pytest.raises(Mi355SegError, match=r"rc=-1.*y_amax is for fp32 tensors"):        # bf16 tensors carry no operand maximum
        L.call("mi355seg_convt3d_k2s2_fwd_ax_bf16", xin.ptr, xin.ld, w.data_ptr(), b.data_ptr(), y.ptr, y.ld, *geom, slot.data_ptr(), ws.ptr, ws.n, st)
    assert bool((y.buf == SENTINEL).all()) and float(slot) == 0.0, f"{name}: the refused fwd_ax call wrote something"
    dx = Buf(rows_in, Cin, ex, "bf16")
    L.call("mi355seg_convt3d_k2s2_dgrad_bf16", gin.ptr, gin.ld, w.data_ptr(), dx.ptr, dx.ld, *geom, ws.ptr, ws.n, st)
    expect_path(L, pd, f"{name}: input gradient")
    ws.check("input gradient")
    ref = convt_reference(geom, rounds(pd))
    grade_stored(name, pd, "dx", dx.check("input gradient"), ref.dx, ref.wit_dx, CONVT_DGRAD_ACC)
    dw, db = Flat(ref.dw.numel()), Flat(Cout)
    L.call("mi355seg_convt3d_k2s2_wgrad_bf16", gin.ptr, gin.ld, xin.ptr, xin.ld, dw.ptr, db.ptr, *geom, ws.ptr, ws.n, st)
    expect_path(L, pw, f"{name}: weight gradient")
    ws.check("weight gradient")
    grade_flat(name, pw, "dw", dw.check("weight gradient"), ref.dw, ref.wit_dw, DW_BOUND * max(float(ref.dw.abs().max()), rows_in ** 0.5))
    grade_flat(name, pw, "db", db.check("bias gradient"), ref.db, ref.wit_db, DB_BOUND * rows_out ** 0.5)
    xin.check("x"), gin.check("dy")


def test_every_bf16_code_is_a_rows_expectation_or_listed_unreachable():
    """Host only: every MI355SEG_PATH_B16_* code of the header is the expected branch of some row above or is in UNREACHABLE (and in
    the module docstring, with the predicate that shadows it); every row's expectation is a code of the header."""
    codes = set(b16_codes())
    assert len(codes) >= 50 and len(set(b16_codes().values())) == len(codes)
    expected = set()
    for r in CONV_ROWS:
        expected |= {r.fwd, r.dgrad, *per_acc(r.wgrad)}
    expected |= {r[5] for r in STATS_ROWS} | {r[3] for r in FUSED_ROWS}
    for r in CONVT_ROWS:
        expected |= set(r[4:7])
    assert not (expected - codes), f"rows expect codes the header does not have: {sorted(expected - codes)}"
    assert not (expected & set(UNREACHABLE)), sorted(expected & set(UNREACHABLE))
    assert set(UNREACHABLE) <= codes
    for name in UNREACHABLE:
        assert name in __doc__, f"{name} is not accounted for in the module docstring"
    missing = codes - expected - set(UNREACHABLE)
    assert not missing, f"no row asserts {sorted(missing)}"
    for pass_ in ("FWD", "DGRAD"):                # every family with tiles: ragged extents, two samples, a volume below one tile
        for fam in ("IGEMM_S", "IGEMM_G"):
            geoms = {r.geom for r in CONV_ROWS if getattr(r, pass_.lower()) == f"B16_{pass_}_{fam}"}
            assert G_RAGGED in geoms and G_SUBTILE in geoms, (pass_, fam)
