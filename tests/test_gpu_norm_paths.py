"""Every selection the launchers of csrc/norm.hip / csrc/norm_api.inc make -- vector, scalar or 8-wide kernel, lanes, rows per block
iteration, capped grid, second trip of the channel loop, fused or fall-back column sum -- against the same operation written plainly
in float64 on the values the kernel reads (for bf16 storage: the bf16-rounded inputs).

THE SELECTION TABLES ARE A MIRROR.  The library does not report which streaming kernel ran (unlike mi355seg_last_conv_path for the
convolutions), so ``red_plan`` / ``ew_map`` / ``ew_map8`` / ``vec_ok`` / ``vec8_ok`` / ``row_grid`` / the ``fused_sum`` predicate and
the 8-wide alignment conditions are re-written below in Python, with every constant (kRedThreads, kMaxRedBlocks, the 8192-block cap,
the 1024-block cap under dx_colsum, the eight rows per thread) read from the sources by regex.  Each case states the selection it was
built for; the host-only tests assert that the mirror agrees and that every selection of the lists REQUIRED_* is reached for every
entry point and storage type.  A changed constant or predicate in the sources makes those tests fail instead of un-covering a branch
(as long as the mirror is kept in step with the launchers: that is the reviewer's part, the tables are written to be checked by eye).

Conventions (those of test_gpu_conv_paths.py): C ABI on seeded tensors; every output in a buffer pre-filled with 7.0 at pitch > C with
guard rows in front and behind (inputs: NaN in the pad columns); the workspace exactly mi355seg_norm_ws_bytes with a guarded band
behind it; mean / rstd / s1 / s2 handed to the element-wise entry points as given fp32 arrays and used verbatim by the reference.

Bounds.
  * element-wise, fp32: |got - ref| <= 8 * 2^-24 * S, S = the fp64 sum of |every term that enters the element| + |result| (+ 1 where
    expf / expm1f is taken: the negative ELU side, the sigmoid).  Forward: |x al| + |mean al| + |beta| + |res| + |y|.  Backward:
    |gamma rstd| (|dz| + |k1| + |xhat k2|) + |dx|, + |gamma rstd dz| (S_z + 1) where act' goes through expf (its relative error is the
    absolute error of z), + |gamma rstd dy| s (1 + s) for the sigmoid (act' = s (1 - s): 1 and s enter 1 - s, which cancels for large z).  At most five roundings and a few-ulp expf enter an element; 8 is the margin.
    The composed norm_act_bwd uses the kernel's own s1 / s2, each within 2^-22 sum |addend| of the given ones: S grows by
    0.5 |gamma rstd| (sum |a| + |xhat| sum |b|) / rows (= that error over 8 * 2^-24).
  * bf16: + 2^-8 |ref| for the one output rounding (``close()`` of test_gpu_bf16.py).
  * witness: the same formulas through ATen-CPU in fp32; where the witness passes the bound, the case's bound is 4 x its error.
    Each printed line ends in WIT where the term was taken (pytest -rA); the tables mark those cases (column sums only).
  * branch points: an element with |z_ref| <= 8 * 2^-24 * S_z may carry either side's value; asserted <= 1e-4 of a case from the
    reference alone.  In a column sum such an element may move the sum by the difference of its two addends.
  * statistics: the bars of test_norm_statistics_are_accurate_and_shift_invariant, unchanged: mean 1e-6 of |m| + sigma, rstd 2e-6,
    running variance 1e-6.  A constant channel: rstd == 1/sqrt(eps) exactly.
  * column sums (s1, s2, dgamma, dbeta, dslope, group_sums, dx_colsum): max(2^-22 sum |addend|, 4 x witness error), in fp32 and bf16
    alike.  The fused dx_colsum sums the kernel's fp32 dx values before they are stored: against the fp64 chain's column sum, the fp32
    chain's as witness.  The fall-back (channel_sums) reads the stored dx: against the fp64 sum of exactly those values, no slack.  The
    composed norm_act_bwd_colsum(_ax) use their own s1 / s2 (each within 2^-22 sum |addend| of the given ones = d1, d2): their fused
    column sum may move by |gamma rstd| (d1 + mean |xhat| d2) more.
    Measured on the MI355X, as shares of sum |addend| (the bound is 2.4e-7): the kernels' s1 / s2 / dslope / group sums at most
    2.0e-7, the ATen-fp32 witness at most 1.8e-7; where 4 x the witness error passes 2^-22 (short sums: c4-7rows, c32-p36, c32-p33,
    c24-chunks, c256-p257, c1024, c4-1row's one-addend dgamma / dbeta, dgamma of c24-colsum / c6-colsum, the bf16 dx_colsum of c32-colsum, and group_sums with its
    offset channel) the witness term decides
    -- WIT in the tables.  No element-wise case takes the witness term (largest fp32 err / bound 0.32).  Statistics: mean 1.1e-7,
    rstd 2.7e-7, running variance 7.3e-8 of their bars' scales.
"""
import functools
import math
from collections import namedtuple
from types import SimpleNamespace

import pytest
import torch

from stream_grading import (ACT_ELU, ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, DT, EINVAL, GUARD_ROWS, HEADER, Buf, Flat, Report,
                            Workspace, act_both, ambiguous, constant, grad_both, grade_elem, grade_sum, header_constants, other, pick, pinned,
                            rnd, smooth_extra, source, stored, stream)

gpu = pytest.mark.gpu           # per test: the table checks need no GPU and run with -m "not gpu"
STORAGE = ("f32", "bf16")
ESIZE = {"f32": 4, "bf16": 2}
SLOPE = 0.1
EPS = 1e-5
MOMENTUM = 0.1
ALL_ACTS = (ACT_NONE, ACT_RELU, ACT_ELU, ACT_LRELU, ACT_SIGMOID)


@pytest.fixture(scope="module")
def seg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mi355seg
    mi355seg.lib()
    return mi355seg


@pytest.fixture(autouse=True)
def end_the_session_after_a_gpu_fault():
    """A kernel fault leaves the device context unusable: nothing more is started on the GPU after one.  This ends the WHOLE pytest
    session with exit code 3 ("GPU fault, session ended: ..."), also when the file runs as part of the full suite."""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"GPU fault, session ended: {e}", returncode=3)


# ----------------------------------------------------------------------------- the mirror
@functools.lru_cache(maxsize=None)
def K():
    norm, api = source("norm.hip"), source("norm_api.inc")
    k = SimpleNamespace()
    k.red_threads = constant(r"constexpr int kRedThreads = (\d+);", norm, "kRedThreads")
    k.max_red_blocks = constant(r"constexpr int kMaxRedBlocks = (\d+);", norm, "kMaxRedBlocks")
    k.red_iters_per_block = constant(r"long long nb = \(iters \+ \d+\) / (\d+);", norm, "red_plan: iterations per block")
    k.red_vec_max_c = constant(r"is_pow2\(C\) && C >= 4 && C <= (\d+) && \(ld % 4\) == 0", norm, "red_plan: widest vector C")
    k.ew_threads = constant(r"static RowMap ew_map\(int C, bool vec\) \{.*?int lanes = cw > (\d+) \? (\d+) : cw;.*?if \((\d+) % lanes == 0\) \{ m\.lanes = lanes; m\.rpi = (\d+) / lanes; \}",
                            norm, "ew_map: threads per block")
    k.ew8_threads = constant(r"static RowMap ew_map8\(int C\) \{.*?int lanes = cw > (\d+) \? (\d+) : cw;.*?if \((\d+) % lanes == 0\) \{ m\.lanes = lanes; m\.rpi = (\d+) / lanes; \}",
                             norm, "ew_map8: threads per block")
    k.rows_per_thread = constant(r"static int row_grid\(long long rows, int rpi\) \{\s*long long b = \(rows \+ \(long long\)rpi \* (\d+) - 1\) / \(\(long long\)rpi \* (\d+)\);",
                                 norm, "row_grid: rows per thread")
    k.row_grid_cap = constant(r"static int row_grid\(.*?b > (\d+) \? (\d+) : b\)\);", norm, "row_grid: block cap")
    k.colsum_cap = constant(r"if \(dx_colsum && nrb > (\d+)\) nrb = (\d+);", api, "norm_act_bwd_apply: block cap under dx_colsum")
    # the predicates the mirror re-writes, pinned as text: an edit to one of them fails here and sends the editor to the mirror
    for what, pat, text in (("fused_sum", r"const bool fused_sum = dx_colsum && rm\.lanes == \(v \? C / 4 : C\) && \(256 % rm\.lanes\) == 0;", api),
                            ("norm_act_fwd 8-wide", r"sizeof\(TT\) == 2 && !ao && vec8_ok\(C, \{ldx, ldy, res \? ldres : 8\}\) && \(\(\(uintptr_t\)x \| \(uintptr_t\)y \| \(uintptr_t\)\(res \? res : x\)\) % \(8 \* sizeof\(TT\)\)\) == 0", api),
                            ("act_fwd 8-wide", r"sizeof\(TT\) == 2 && vec8_ok\(C, \{ldx, ldy, res \? ldres : 8\}\) && \(\(uintptr_t\)x % 16\) == 0 && \(\(uintptr_t\)y % 16\) == 0", api),
                            ("act_bwd 8-wide", r"sizeof\(TT\) == 2 && vec8_ok\(C, \{lddy, ldx, lddx, res \? ldres : 8\}\) && \(\(uintptr_t\)dy % 16\) == 0", api),
                            ("act_bwd_add 8-wide", r"if \(vec8_ok\(C, \{lddy, ldx, lddx, res \? ldres : 8, addend \? ldadd : 8\}\) && \(\(uintptr_t\)dy % al\) == 0", api),
                            ("vec_ok", r"static bool vec_ok\(int C, std::initializer_list<int> lds\) \{\s*if \(C % 4\) return false;\s*for \(int l : lds\) if \(l % 4\) return false;", norm),
                            ("vec8_ok", r"static bool vec8_ok\(int C, std::initializer_list<int> lds\) \{\s*if \(C % 8\) return false;\s*for \(int l : lds\) if \(l % 8\) return false;", norm),
                            ("channel_sums chunks", r"if \(rem >= 4 && \(ldx % 4\) == 0 && \(c0 % 4\) == 0 && \(\(uintptr_t\)x % \(4 \* sizeof\(T\)\)\) == 0\) \{\s*take = 4;\s*while \(take \* 2 <= rem && take \* 2 <= 1024\) take \*= 2;\s*\} else \{\s*take = rem < 256 \? rem : 256;", norm)):
        pinned(pat, text, what)
    return k


def is_pow2(v):
    return v > 0 and v & (v - 1) == 0


def red_plan(rows, C, ld):
    """-> (kind, lanes, rpi, capped) or None: red_plan of norm.hip."""
    k = K()
    if is_pow2(C) and 4 <= C <= k.red_vec_max_c and ld % 4 == 0:
        kind, lanes = "vec", C // 4
    elif C <= k.red_threads:
        kind, lanes = "scalar", C
    else:
        return None
    rpi = k.red_threads // lanes
    iters = -(-rows // rpi)
    nb = -(-iters // k.red_iters_per_block)
    return kind, lanes, rpi, nb > k.max_red_blocks


def sum_chunks(C, ld, ptr_mod):
    """channel_sums_t: the (kind, width) of every chunk it walks; ptr_mod = the base address modulo 4 elements' bytes."""
    out, c0 = [], 0
    while c0 < C:
        rem = C - c0
        if rem >= 4 and ld % 4 == 0 and c0 % 4 == 0 and ptr_mod == 0:
            take = 4
            while take * 2 <= rem and take * 2 <= 1024:
                take *= 2
        else:
            take = min(rem, 256)
        out.append((red_plan(1, take, ld)[0], take))
        c0 += take
    return tuple(out)


def vec_ok(C, lds):
    return C % 4 == 0 and all(l % 4 == 0 for l in lds)


def vec8_ok(C, lds):
    return C % 8 == 0 and all(l % 8 == 0 for l in lds)


def ew_map(C, vec, threads=None, width=None):
    threads = threads or K().ew_threads
    cw = C // (width or (4 if vec else 1))
    lanes = min(cw, threads)
    rpi = threads // lanes if threads % lanes == 0 else 1
    return lanes, rpi, -(-cw // lanes)


def ew_map8(C):
    return ew_map(C, True, K().ew8_threads, 8)


def row_grid(rows, rpi, cap=None):
    cap = cap or K().row_grid_cap
    b = max(1, -(-rows // (rpi * K().rows_per_thread)))
    return min(b, cap), b > cap


def ptr_mod16(ld, off, st):
    """Byte address of a Buf's first payload element modulo 16 (the allocation itself is 256-byte aligned)."""
    return ((GUARD_ROWS * ld + off) * ESIZE[st]) % 16


WIDE8 = {"norm_act_fwd": ("bf16",), "act_fwd": ("bf16",), "act_bwd": ("bf16",), "act_bwd_add": ("f32", "bf16")}
EW_ENTRIES = ("norm_act_fwd", "norm_act_fwd_ax", "norm_act_bwd_apply", "norm_act_bwd_apply_ax", "norm_act_bwd", "act_fwd", "act_bwd", "act_bwd_add",
              "prelu_fwd", "prelu_bwd", "scale_channels")
COLSUM_ENTRIES = ("norm_act_bwd_apply", "norm_act_bwd_colsum", "norm_act_bwd_colsum_ax")
RED_ENTRIES = ("norm_stats", "norm_act_bwd_sums", "prelu_bwd")


def ew_select(entry, st, C, ld, off, rows):
    """-> (kind, lanes, rpi, trips of the channel loop, grid capped) of one element-wise entry point; every tensor of a case has the
    same pitch and the same offset into its rows."""
    if st in WIDE8.get(entry, ()) and vec8_ok(C, [ld]) and ptr_mod16(ld, off, st) == 0:
        lanes, rpi, trips = ew_map8(C)
        kind = "wide8"
    else:
        v = vec_ok(C, [ld])
        lanes, rpi, trips = ew_map(C, v)
        kind = "vec" if v else "scalar"
    return kind, lanes, rpi, trips, row_grid(rows, rpi)[1]


def colsum_select(C, ld, rows):
    """-> ("fused" | "fallback", grid capped at the dx_colsum cap)."""
    v = vec_ok(C, [ld])
    lanes, rpi, _ = ew_map(C, v)
    fused = lanes == (C // 4 if v else C) and K().ew_threads % lanes == 0
    return ("fused" if fused else "fallback"), row_grid(rows, rpi, K().colsum_cap)[1]


# ----------------------------------------------------------------------------- case tables
# sel: what red_plan gives norm_stats / norm_act_bwd_sums / prelu_bwd at this pitch (kind, lanes, rpi, block count capped);
# sums: the chunks channel_sums walks for group_sums on the same tensor.  kRedThreads = 256, eight iterations per block, kMaxRedBlocks = 1024.
Red = namedtuple("Red", "name rows groups C pad sel sums")
RED_CASES = [
    # C = 4 is a power of two in 4..1024 and ld = 8 % 4 == 0: vector, lanes = C / 4 = 1, rpi = 256.  1000 rows = 4 iterations = 1 block,
    # stride 256: row slots < 232 take two pairs (even number of strides), the others a pair and the tail (odd); 1000 % 256 != 0
    Red("c4", 1000, 1, 4, 4, ("vec", 1, 256, False), (("vec", 4),)),
    # rows = 1 at ld = C + 4: one thread works, the pivot's eight samples are the same row
    Red("c4-1row", 1, 1, 4, 4, ("vec", 1, 256, False), (("vec", 4),)),
    # rows = 7 < the 8 pivot samples; three groups start at rows 0, 7, 14
    Red("c4-7rows", 7, 3, 4, 4, ("vec", 1, 256, False), (("vec", 4),)),   # WIT s2, group_sums
    # C = 1024 = the widest vector C: lanes = 256, rpi = 1; 43 rows = 6 blocks of 8 or 7 rows: four pairs, or three pairs and the tail
    Red("c1024", 43, 1, 1024, 4, ("vec", 256, 1, False), (("vec", 1024),)),   # WIT s1, s2, dslope, group_sums
    # C = 32 at pitch 36 (36 % 4 == 0): vector, lanes = 8, rpi = 32.  45 rows per group (45 % 32 != 0, another remainder in each group)
    Red("c32-p36", 45, 3, 32, 4, ("vec", 8, 32, False), (("vec", 32),)),   # WIT s1 (bf16), s2, group_sums
    # the same over 1100 rows: 35 iterations, 5 blocks, stride 160, 6 or 7 rows per thread (3 pairs | 3 pairs + tail)
    Red("c32-p36-long", 1100, 1, 32, 4, ("vec", 8, 32, False), (("vec", 32),)),
    # C = 32 at pitch 33: is_pow2 holds, ld % 4 fails -> scalar by the pitch alone, lanes = 32, rpi = 8
    Red("c32-p33", 45, 1, 32, 1, ("scalar", 32, 8, False), (("scalar", 32),)),   # WIT dslope, group_sums
    # C = 6: is_pow2 fails -> scalar, lanes = 6, rpi = 256 / 6 = 42, threads 252..255 idle; 100 % 42 != 0
    Red("c6", 100, 3, 6, 1, ("scalar", 6, 42, False), (("scalar", 6),)),   # WIT group_sums
    # C = 200 <= 256, no power of two: scalar, rpi = 1; 8300 iterations / 8 = 1038 blocks > kMaxRedBlocks: capped, blocks stride twice
    Red("c200-cap", 8300, 1, 200, 1, ("scalar", 200, 1, True), (("scalar", 200),)),   # WIT group_sums
    # C = 256 at pitch 257: scalar at the full 256 lanes
    Red("c256-p257", 19, 1, 256, 1, ("scalar", 256, 1, False), (("scalar", 256),)),   # WIT s1, s2, dslope, group_sums
    # C = 24 at pitch 28: scalar for red_plan (rpi = 10, 16 idle threads); channel_sums walks it as a 16-wide and an 8-wide vector chunk
    Red("c24-chunks", 50, 1, 24, 4, ("scalar", 24, 10, False), (("vec", 16), ("vec", 8))),   # WIT s2 (bf16), group_sums
]
RED_REJECTED = (320, 2048)          # neither a power of two <= 1024 nor <= kRedThreads: MI355SEG_EINVAL, nothing launched
REQUIRED_RED = {("vec", 1, 256, False), ("vec", 256, 1, False), ("vec", 8, 32, False), ("scalar", 32, 8, False), ("scalar", 6, 42, False),
                ("scalar", 200, 1, True), ("scalar", 256, 1, False)}
REQUIRED_SUMS = {("vec", 4), ("vec", 1024), ("scalar", 32), ("scalar", 6), ("scalar", 200), ("scalar", 256), ("vec", 16), ("vec", 8)}

# sel: ew_map / row_grid for the 4-wide and scalar kernels (kind, lanes, rpi, channel-loop trips, grid capped); wide: the same for the
# 8-wide kernels where the entry point has one for the storage type (bf16: norm_act_fwd, act_fwd, act_bwd; both: act_bwd_add), else None;
# colsum: (fused | fallback, capped at 1024 blocks) where the case also asks for dx_colsum (groups == 1).  256 threads, 8 rows per thread.
Ew = namedtuple("Ew", "name rows groups C pad off sel wide colsum acts")
EW_CASES = [
    # C = 1, 3, 6 fail C % 4: scalar.  lanes = C; 256 % 3 and 256 % 6 != 0 -> rpi = 1 and 253 / 250 idle threads (the !active && amax_out path)
    Ew("c1", 37, 2, 1, 2, 0, ("scalar", 1, 256, 1, False), None, None, ALL_ACTS),
    Ew("c3-odd-pitch", 37, 1, 3, 2, 0, ("scalar", 3, 1, 1, False), None, None, ALL_ACTS),
    Ew("c6", 37, 2, 6, 1, 0, ("scalar", 6, 1, 1, False), None, None, ALL_ACTS),
    # C = 4 at pitch 12 (4-aligned, not 8-aligned): vector, one channel slot, rpi = 256; rows = 1
    Ew("c4-1row", 1, 1, 4, 8, 0, ("vec", 1, 256, 1, False), None, None, ALL_ACTS),   # WIT dgamma / dbeta of the composed backward
    # C = 32 at pitch 36: vector, lanes = 8, rpi = 32; 36 % 8 != 0 keeps bf16 off the 8-wide kernels; 301 rows: the row-pair tail
    Ew("c32-p36", 301, 2, 32, 4, 0, ("vec", 8, 32, 1, False), None, None, ALL_ACTS),
    # the same with dx_colsum: lanes == C / 4 and 256 % 8 == 0 -> fused
    Ew("c32-colsum", 301, 1, 32, 4, 0, ("vec", 8, 32, 1, False), None, ("fused", False), (ACT_RELU, ACT_SIGMOID)),   # WIT dx_colsum (bf16)
    # C = 32 at pitch 40, pointers 16-byte aligned: bf16 (and act_bwd_add in fp32) 8-wide, lanes = 4, rpi = 64
    Ew("c32-p40", 301, 2, 32, 8, 0, ("vec", 8, 32, 1, False), ("wide8", 4, 64, 1, False), None, ALL_ACTS),
    # read 4 elements into the rows: bf16 pointers 8-byte aligned -> vec8 alignment fails -> 4-wide (fp32: 16 bytes in, act_bwd_add stays 8-wide)
    Ew("c32-p40-off4", 301, 2, 32, 8, 4, ("vec", 8, 32, 1, False), "f32", None, (ACT_ELU, ACT_LRELU)),
    # read 1 element in: 4-wide accesses on 2- (bf16) / 4-byte (fp32) aligned addresses; the values must still be right
    Ew("c32-p40-off1", 301, 2, 32, 8, 1, ("vec", 8, 32, 1, False), None, None, (ACT_ELU, ACT_LRELU)),
    # C = 24 at pitch 28: vector, six channel slots, 256 % 6 != 0 -> rpi = 1; dx_colsum: lanes == 6 but 256 % 6 != 0 -> fall-back (channel_sums)
    Ew("c24-colsum", 301, 1, 24, 4, 0, ("vec", 6, 1, 1, False), None, ("fallback", False), ALL_ACTS),   # WIT dgamma
    # C = 6 at pitch 7 with dx_colsum: scalar, lanes == C but 256 % 6 != 0 -> fall-back, channel_sums' scalar form (one 6-wide chunk)
    Ew("c6-colsum", 37, 1, 6, 1, 0, ("scalar", 6, 1, 1, False), None, ("fallback", False), (ACT_ELU, ACT_SIGMOID)),   # WIT dgamma
    # the same at 66000 rows: 66000 / 8 = 8250 blocks > 8192: capped, 58 blocks take a second stride
    Ew("c24-capped", 66000, 1, 24, 4, 0, ("vec", 6, 1, 1, True), None, None, (ACT_ELU, ACT_SIGMOID)),
    # C = 1028: vector, 257 channel slots over 256 lanes: lane 0 takes a second trip
    Ew("c1028", 9, 1, 1028, 4, 0, ("vec", 256, 1, 2, False), None, None, ALL_ACTS),
    # C = 300 at pitch 301: the scalar form of the second trip (44 lanes take it)
    Ew("c300", 9, 2, 300, 1, 0, ("scalar", 256, 1, 2, False), None, None, ALL_ACTS),
    # C = 256 at pitch 257, dx_colsum: scalar, lanes == C and 256 % 256 == 0 -> fused; 8300 / 8 = 1038 blocks > 1024: capped
    Ew("c256-p257-colsum", 8300, 1, 256, 1, 0, ("scalar", 256, 1, 1, False), None, ("fused", True), (ACT_RELU, ACT_SIGMOID)),
]
REQUIRED_EW = {("scalar", 1, 256, 1, False), ("scalar", 3, 1, 1, False), ("scalar", 6, 1, 1, False), ("vec", 1, 256, 1, False),
               ("vec", 8, 32, 1, False), ("vec", 6, 1, 1, False), ("vec", 6, 1, 1, True), ("vec", 256, 1, 2, False), ("scalar", 256, 1, 2, False)}
REQUIRED_WIDE = {("wide8", 4, 64, 1, False)}
# a second trip needs more than 256 channel slots: C > 1024 (vector) or C > 256 off the vector form -- exactly the channel counts red_plan
# has no plan for.  norm_act_bwd* (its sums pass) and prelu_bwd (its slope gradient) reduce first: in the two-trip cases they must
# return MI355SEG_EINVAL and write nothing, and no geometry takes their element-wise kernels on a second trip.
TWO_TRIP = {("vec", 256, 1, 2, False), ("scalar", 256, 1, 2, False)}
TWO_TRIP_CASES = ("c1028", "c300")
REDUCE_FIRST = ("norm_act_bwd", "prelu_bwd")
REQUIRED_COLSUM = {("fused", False), ("fallback", False), ("fused", True)}
REQUIRED_COLSUM_KERNELS = {("vec", 8, 32, 1, False), ("vec", 6, 1, 1, False), ("scalar", 6, 1, 1, False), ("scalar", 256, 1, 1, False)}
REQUIRED_COLSUM_CHUNKS = {("vec", 16), ("vec", 8), ("scalar", 6)}        # what channel_sums walks behind the fall-back, fp32 and bf16
# activation codes: those act_host_dispatch gives an instantiation of their own, and the one left to the run-time switch
INSTANTIATED, SWITCHED = (ACT_NONE, ACT_RELU, ACT_ELU, ACT_LRELU), (ACT_SIGMOID,)


def cid(c):
    return c.name


def wide_for(case, entry, st):
    if st not in WIDE8.get(entry, ()):
        return None
    if case.wide == "f32":          # an offset that keeps 16-byte alignment in fp32 only
        return ("wide8", 4, 64, 1, False) if st == "f32" else None
    return case.wide


# ----------------------------------------------------------------------------- host-only table checks
def test_constants_are_the_ones_the_tables_were_written_for():
    k = K()
    assert (k.red_threads, k.max_red_blocks, k.red_iters_per_block, k.red_vec_max_c) == (256, 1024, 8, 1024)
    assert (k.ew_threads, k.ew8_threads, k.rows_per_thread, k.row_grid_cap, k.colsum_cap) == (256, 256, 8, 8192, 1024)
    acts = header_constants("MI355SEG_ACT_")
    assert acts == {"NONE": ACT_NONE, "RELU": ACT_RELU, "ELU": ACT_ELU, "LRELU": ACT_LRELU, "SIGMOID": ACT_SIGMOID}, acts
    assert set(ALL_ACTS) == set(acts.values()) == set(INSTANTIATED) | set(SWITCHED)
    common = source("common.h")
    for a in ("NONE", "RELU", "ELU", "LRELU"):
        assert f"case MI355SEG_ACT_{a}: f(std::integral_constant<int, MI355SEG_ACT_{a}>{{}}); break;" in common, a
    assert "MI355SEG_ACT_SIGMOID>" not in common          # the sigmoid takes the run-time switch
    assert constant(r"#define MI355SEG_EINVAL \((-?\d+)\)", open(HEADER).read(), "MI355SEG_EINVAL") == EINVAL


@pytest.mark.parametrize("case", RED_CASES, ids=cid)
def test_reduction_case_reaches_the_selection_it_names(case):
    ld = case.C + case.pad
    assert red_plan(case.rows, case.C, ld) == case.sel
    for st in STORAGE:      # a Buf's payload starts GUARD_ROWS rows in: 4-element aligned at every pitch of the table
        assert (GUARD_ROWS * ld * ESIZE[st]) % (4 * ESIZE[st]) == 0
    assert sum_chunks(case.C, ld, 0) == case.sums
    if case.sel[0] == "vec":            # the two-row loop: some thread sees an even and some thread an odd number of strides (or one row)
        _, lanes, rpi, _ = case.sel
        nblk = min(K().max_red_blocks, max(1, -(-(-(-case.rows // rpi)) // K().red_iters_per_block)))
        counts = {len(range(b * rpi + s, case.rows, nblk * rpi)) for b in range(nblk) for s in range(rpi)}
        assert case.rows < 8 or ({n % 2 for n in counts if n} == {0, 1}), counts


def test_rejected_channel_counts():
    for C in RED_REJECTED:
        assert red_plan(100, C, C + 4) is None and red_plan(100, C, C + 1) is None


@pytest.mark.parametrize("case", EW_CASES, ids=cid)
def test_elementwise_case_reaches_the_selection_it_names(case):
    ld = case.C + case.pad
    for st in STORAGE:
        for entry in EW_ENTRIES:
            want = wide_for(case, entry, st) or case.sel
            assert ew_select(entry, st, case.C, ld, case.off, case.rows) == want, (entry, st)
    assert (red_plan(case.rows, case.C, ld) is None) == (case.sel in TWO_TRIP) == (case.name in TWO_TRIP_CASES)
    if case.colsum:
        assert case.groups == 1 and colsum_select(case.C, ld, case.rows) == case.colsum
    assert set(case.acts) <= set(ALL_ACTS) and set(case.acts) & set(INSTANTIATED)


def ew_entries(case):
    """The entry points the GPU test runs on an element-wise case (it asserts at its end that it called exactly these)."""
    return EW_ENTRIES + (COLSUM_ENTRIES[1:] if case.colsum else ())


def red_entries(case, st):
    """The same for a reduction case: group_sums has an fp32 form only."""
    return RED_ENTRIES + (("group_sums",) if st == "f32" else ())


def test_every_listed_selection_is_reached_for_every_entry_point_and_storage_type():
    """Per (entry point, storage type), over the cases that run that entry point (ew_entries / red_entries, which the GPU tests check
    against the calls they made).  Not covered, by construction of the table: norm_act_bwd_colsum(_ax) run on the dx_colsum cases only
    (REQUIRED_COLSUM_KERNELS is all their apply kernel reaches: no rpi = 256, no second trip, no 8192-block cap); channel_sums behind
    the fall-back walks a 16- and an 8-wide vector chunk and one 6-wide scalar chunk, its 256-wide scalar chunks and capped grid are
    reached through group_sums in fp32 only."""
    for st in STORAGE:
        for entry in RED_ENTRIES:
            got = {red_plan(c.rows, c.C, c.C + c.pad) for c in RED_CASES if entry in red_entries(c, st)}
            assert REQUIRED_RED <= got, (entry, st, REQUIRED_RED - got)
            shapes = {(c.rows, c.groups) for c in RED_CASES if entry in red_entries(c, st)}
            assert shapes >= {(1, 1), (7, 3)} and {g for _, g in shapes} == {1, 3}
        for entry in EW_ENTRIES:
            cases = [c for c in EW_CASES if entry in ew_entries(c)]
            got = {ew_select(entry, st, c.C, c.C + c.pad, c.off, c.rows) for c in cases}
            need = (REQUIRED_EW - (TWO_TRIP if entry in REDUCE_FIRST else set())) | (REQUIRED_WIDE if st in WIDE8.get(entry, ()) else set())
            assert need <= got, (entry, st, need - got)
            assert {a for c in cases for a in c.acts} == set(ALL_ACTS)
            assert {c.rows for c in cases} >= {1} and any(c.rows % 2 for c in cases if c.sel[0] == "vec")
        for entry in COLSUM_ENTRIES:
            cases = [c for c in EW_CASES if c.colsum and entry in ew_entries(c)]
            got = {colsum_select(c.C, c.C + c.pad, c.rows) for c in cases}
            assert REQUIRED_COLSUM <= got, (entry, st, REQUIRED_COLSUM - got)
            assert {c.sel for c in cases} == REQUIRED_COLSUM_KERNELS
            chunks = {ch for c in cases if c.colsum[0] == "fallback" for ch in sum_chunks(c.C, c.C + c.pad, ptr_mod16(c.C + c.pad, c.off, st) % (4 * ESIZE[st]))}
            assert chunks == REQUIRED_COLSUM_CHUNKS, (entry, st, chunks)
        # bf16, C = 32: 16-byte aligned pointers 8-wide, 4 elements in 4-wide, 1 element in 4-wide on a 2-byte aligned address
        by_off = {c.off: ew_select("act_fwd", "bf16", c.C, c.C + c.pad, c.off, c.rows)[0] for c in EW_CASES if c.C == 32 and c.pad == 8}
        assert by_off == {0: "wide8", 4: "vec", 1: "vec"}, by_off
    got = {ch for c in RED_CASES if "group_sums" in red_entries(c, "f32") for ch in sum_chunks(c.C, c.C + c.pad, 0)}       # group_sums: fp32 only
    assert REQUIRED_SUMS <= got, REQUIRED_SUMS - got


# ----------------------------------------------------------------------------- data and the plain fp64 (/ fp32 witness) formulas
def ws_for(L, rows, groups, C):
    return Workspace(L.query("mi355seg_norm_ws_bytes", rows, groups, C))


def moments(x, groups, rows, C):
    xd = x.double().reshape(groups, rows, C)
    return xd.mean(1), xd.var(1, unbiased=False)


@functools.lru_cache(maxsize=None)
def case_data(kind, index, st):
    """Seeded inputs of one case, as the fp32 values the storage type holds; mean / rstd as given fp32 arrays."""
    c = (RED_CASES if kind == "red" else EW_CASES)[index]
    R, C = c.groups * c.rows, c.C
    seed = 1000 * index + (500 if kind == "red" else 0)
    d = SimpleNamespace()
    x = rnd(R, C, seed=seed + 1) * 1.5 + 0.25
    if kind == "red" and C >= 4:
        x[:, 0] = 50.0 + 0.5 * rnd(R, seed=seed + 7)       # |mean| = 100 sigma
        x[:, 1] = 1e4 + rnd(R, seed=seed + 8)              # offset 1e4
        x[:, 2] = 3.25                                     # exactly constant
    d.x = stored(x, st)
    d.dy = stored(rnd(R, C, seed=seed + 2), st)
    d.res = stored(rnd(R, C, seed=seed + 3), st)
    d.addend = stored(rnd(R, C, seed=seed + 4), st)
    d.gamma = 1.0 + 0.3 * rnd(C, seed=seed + 5)
    d.beta = 0.2 * rnd(C, seed=seed + 6)
    d.slopes = 0.25 + 0.2 * rnd(C, seed=seed + 9)
    d.scale = (torch.rand(c.groups, C, generator=torch.Generator().manual_seed(seed + 10)) > 0.3).float() * 1.25
    if kind == "red":
        m, v = moments(d.x, c.groups, c.rows, C)
        d.mean, d.rstd = m.float(), (1.0 / (v + EPS).sqrt()).float()
    else:           # the element-wise entry points take mean / rstd as given arrays: any will do, and rows = 1 has no statistics of its own
        d.mean = 0.25 + 0.3 * rnd(c.groups, C, seed=seed + 11)
        d.rstd = 0.5 + torch.rand(c.groups, C, generator=torch.Generator().manual_seed(seed + 12))
    return d


def chain(d, c, act, slope, use_res, use_aff, dt, given=None):
    """Normalise + residual + activation and its backward, written plainly in ``dt``.  Forward as the library documents it,
    y = act((x - mean) rstd gamma + beta + res) with al = rstd gamma folded; backward dx = rstd gamma (dz - s1 / rows - xhat s2 / rows)."""
    G, rows, C = c.groups, c.rows, c.C
    v = lambda t: t.to(dt).reshape(G, rows, C)
    x, dy = v(d.x), v(d.dy)
    res = v(d.res) if use_res else torch.zeros((), dtype=dt)
    m, rs = d.mean.to(dt).reshape(G, 1, C), d.rstd.to(dt).reshape(G, 1, C)
    ga = d.gamma.to(dt) if use_aff else torch.ones((), dtype=dt)
    be = d.beta.to(dt) if use_aff else torch.zeros((), dtype=dt)
    o = SimpleNamespace()
    al = rs * ga
    o.zf = x * al + (be - m * al) + res
    o.Szf = (x * al).abs() + (m * al).abs() + be.abs() + res.abs()
    fb = act_both(o.zf, act, slope)
    o.y, o.y_alt = pick(o.zf, fb), other(o.zf, fb)
    o.Sy = o.Szf + o.y.abs() + smooth_extra(o.zf, act)
    o.xh = (x - m) * rs
    o.z = o.xh * ga + be + res
    o.Sz = (o.xh * ga).abs() + be.abs() + res.abs()
    gb = grad_both(o.z, act, slope)
    o.dz, o.dz_alt = dy * pick(o.z, gb), dy * other(o.z, gb)
    sm = smooth_extra(o.z, act) * o.dz.abs() * (o.Sz + 1.0)
    if act == ACT_SIGMOID:          # act' = s (1 - s): the terms 1 and s enter 1 - s, which cancels for large z
        sg = torch.sigmoid(o.z)
        sm = sm + dy.abs() * sg * (1.0 + sg)
    o.Sdz = o.dz.abs() + sm
    o.a, o.b, o.a_alt, o.b_alt = o.dz, o.dz * o.xh, o.dz_alt, o.dz_alt * o.xh
    if given is None:
        given = (o.a.sum(1).float(), o.b.sum(1).float())
    o.given = given
    k1, k2 = (t.to(dt).reshape(G, 1, C) / rows for t in given)
    o.gr = ga * rs
    o.dx, o.dx_alt = o.gr * (o.dz - k1 - o.xh * k2), o.gr * (o.dz_alt - k1 - o.xh * k2)
    o.Sdx = o.gr.abs() * (o.dz.abs() + k1.abs() + (o.xh * k2).abs()) + o.dx.abs() + o.gr.abs() * sm
    return o


def plain_act(d, c, act, slope, use_res, dt, addend):
    """y = act(x + res), dx = addend + dy act'(x + res); slope a scalar or the per-channel PReLU slopes."""
    R, C = c.groups * c.rows, c.C
    x, dy = d.x.to(dt), d.dy.to(dt)
    res = d.res.to(dt) if use_res else torch.zeros((), dtype=dt)
    ad = d.addend.to(dt) if addend else torch.zeros((), dtype=dt)
    sl = slope.to(dt) if torch.is_tensor(slope) else slope
    o = SimpleNamespace()
    o.z = x + res
    o.Sz = x.abs() + res.abs()
    fb, gb = act_both(o.z, act, sl), grad_both(o.z, act, sl)
    o.y, o.y_alt = pick(o.z, fb), other(o.z, fb)
    o.Sy = o.Sz + o.y.abs() + smooth_extra(o.z, act)
    t, t_alt = dy * pick(o.z, gb), dy * other(o.z, gb)
    o.dx, o.dx_alt = ad + t, ad + t_alt
    o.Sdx = t.abs() + ad.abs() + o.dx.abs() + smooth_extra(o.z, act) * t.abs() * (o.Sz + 1.0)
    if act == ACT_SIGMOID:          # act' = s (1 - s): the terms 1 and s enter 1 - s, which cancels for large z
        sg = torch.sigmoid(o.z)
        o.Sdx = o.Sdx + dy.abs() * sg * (1.0 + sg)
    o.ds_addend = dy * torch.clamp(o.z, max=0.0)        # the PReLU slope gradient's addends
    return o


def amb_slack(amb, a, a_alt):
    return ((a - a_alt).abs() * amb).sum(1)


def grade_colsum(rep, what, got, kind, o, w, amb, written, moved=None):
    """dx_colsum at the column-sum bar.  Fused: the kernel sums its fp32 dx values before they are stored, whatever the storage type:
    against the fp64 chain's column sum, the fp32 chain's sum as witness (+ what branch-point elements may move).  Fall-back:
    channel_sums reads the dx that was stored and sums exactly those values: against their fp64 sum, ATen's fp32 sum of them as witness."""
    if kind == "fused":
        slack = amb_slack(amb, o.dx, o.dx_alt)[0] + (moved if moved is not None else 0.0)
        grade_sum(rep, what, got, o.dx.sum(1)[0], o.dx.abs().sum(1)[0], wit=w.dx.sum(1)[0], slack=slack)
    else:
        grade_sum(rep, what, got, written.sum(0), written.abs().sum(0), wit=written.float().sum(0))


class Recorder:
    """The library handle, noting which entry points a test called."""

    def __init__(self, L):
        self.L, self.names = L, set()

    def call(self, name, *args):
        self.names.add(name)
        return self.L.call(name, *args)

    def query(self, name, *args):
        self.names.add(name)
        return self.L.query(name, *args)

    def ran(self, entries, st):
        want = {f"mi355seg_{e}_{st}" for e in entries}
        got = {n for n in self.names if n not in ("mi355seg_norm_ws_bytes", "mi355seg_last_error")}
        assert got == want, (got ^ want)


def bits(t):
    return t.view(torch.int32)


def expect_amax(L, call, written, what):
    """The by-product equals the maximum magnitude of what the call wrote, bit for bit; max-combined, so a larger value already in
    the slot survives."""
    slot = Flat(1, init=torch.zeros(1))
    call(slot.ptr)
    out = written()
    got = slot.check(what + " amax")
    want = out.abs().max().float()
    assert bits(got.float())[0] == bits(want.reshape(1))[0], f"{what}: amax {float(got):.9g}, wrote {float(want):.9g}"
    big = Flat(1, init=torch.full((1,), 3.0e30))
    call(big.ptr)
    assert float(big.check(what + " preset amax")) == float(torch.tensor(3.0e30, dtype=torch.float32)), f"{what}: a larger value in the slot did not survive"
    return out


# ----------------------------------------------------------------------------- reductions
@gpu
@pytest.mark.parametrize("st", STORAGE)
@pytest.mark.parametrize("index", range(len(RED_CASES)), ids=[c.name for c in RED_CASES])
def test_reduction_entry_points_against_fp64(seg, index, st):
    """norm_stats (running statistics present and absent), norm_act_bwd_sums, the slope gradient of prelu_bwd and group_sums on one
    geometry of the table."""
    L = Recorder(seg.lib())
    c = RED_CASES[index]
    G, rows, C, R = c.groups, c.rows, c.C, c.groups * c.rows
    d = case_data("red", index, st)
    rep = Report(f"{c.name}/{st}")
    X, DY, RES = (Buf(R, C, c.pad, st, data=t) for t in (d.x, d.dy, d.res))
    ws = ws_for(L, rows, G, C)

    # ---- norm_stats
    m64, v64 = moments(d.x, G, rows, C)
    sig = v64.sqrt()
    runs = []
    for running in ((True, False) if G == 1 else (False,)):
        mean, rstd = Flat(G * C), Flat(G * C)
        rm, rv = Flat(C, init=torch.full((C,), 0.5)), Flat(C, init=torch.ones(C))
        L.call(f"mi355seg_norm_stats_{st}", X.ptr, X.ld, rows, G, C, EPS, mean.ptr, rstd.ptr, rm.ptr if running else None, rv.ptr if running else None,
               MOMENTUM, ws.ptr, ws.n, stream())
        gm, gr = mean.check("mean").reshape(G, C), rstd.check("rstd").reshape(G, C)
        ws.check("norm_stats")
        assert bool(torch.isfinite(gm).all() & torch.isfinite(gr).all())
        e_mean = float(((gm - m64).abs() / (m64.abs() + sig)).max())
        e_rstd = float((gr * (v64 + float(torch.tensor(EPS, dtype=torch.float32))).sqrt() - 1).abs().max())
        print(f"{rep.name:40s} norm_stats running={running!s:5s} mean {e_mean:9.2e} (bar 1e-6)  rstd {e_rstd:9.2e} (bar 2e-6)")
        assert e_mean < 1e-6 and e_rstd < 2e-6
        if C >= 4:          # the constant channel: variance exactly 0
            flat = 1.0 / math.sqrt(float(torch.tensor(EPS, dtype=torch.float32)))
            assert bool((gr[:, 2].float() == torch.tensor(flat, dtype=torch.float32)).all()), gr[:, 2]
            assert bool((gm[:, 2] == 3.25).all())
        if running:
            unb = v64[0] * rows / (rows - 1) if rows > 1 else v64[0]
            ref_rv, ref_rm = (1 - MOMENTUM) + MOMENTUM * unb, (1 - MOMENTUM) * 0.5 + MOMENTUM * m64[0]
            e_rv = float(((rv.check("running_var") - ref_rv).abs() / ref_rv).max())
            e_rm = float(((rm.check("running_mean") - ref_rm).abs() / (m64[0].abs() + sig[0] + 0.5)).max())
            print(f"{rep.name:40s} running_var {e_rv:9.2e} (bar 1e-6)  running_mean {e_rm:9.2e} (bar 1e-6)")
            assert e_rv < 1e-6 and e_rm < 1e-6
        else:
            assert bool((rm.check("running_mean") == 0.5).all() & (rv.check("running_var") == 1.0).all())
        runs.append((gm, gr))
    assert len(runs) == 1 or (torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]))

    # ---- norm_act_bwd_sums: activation, affine pair and residual rotate through the table
    act, use_aff, use_res = ALL_ACTS[index % 5], index % 2 == 0, index % 3 != 0
    o = chain(d, c, act, SLOPE, use_res, use_aff, torch.float64)
    w = chain(d, c, act, SLOPE, use_res, use_aff, torch.float32, given=o.given)
    amb = ambiguous(o.z, o.Sz, act, f"{c.name} bwd_sums")
    mean, rstd = Flat(G * C, init=d.mean), Flat(G * C, init=d.rstd)
    gamma, beta = Flat(C, init=d.gamma), Flat(C, init=d.beta)
    s1, s2, dgamma, dbeta = Flat(G * C), Flat(G * C), Flat(C), Flat(C)
    affine_grads = G == 1
    L.call(f"mi355seg_norm_act_bwd_sums_{st}", DY.ptr, DY.ld, X.ptr, X.ld, mean.ptr, rstd.ptr, gamma.ptr if use_aff else None, beta.ptr if use_aff else None,
           RES.ptr if use_res else None, RES.ld, s1.ptr, s2.ptr, dgamma.ptr if affine_grads else None, dbeta.ptr if affine_grads else None,
           rows, G, C, act, SLOPE, ws.ptr, ws.n, stream())
    ws.check("norm_act_bwd_sums")
    g1, g2 = s1.check("s1").reshape(G, C), s2.check("s2").reshape(G, C)
    grade_sum(rep, "bwd_sums s1", g1, o.a.sum(1), o.a.abs().sum(1), wit=w.a.sum(1), slack=amb_slack(amb, o.a, o.a_alt))
    grade_sum(rep, "bwd_sums s2", g2, o.b.sum(1), o.b.abs().sum(1), wit=w.b.sum(1), slack=amb_slack(amb, o.b, o.b_alt))
    if affine_grads:
        assert torch.equal(dbeta.check("dbeta").reshape(G, C), g1) and torch.equal(dgamma.check("dgamma").reshape(G, C), g2)

    # ---- prelu_bwd's slope gradient over all G * rows rows (its dx is graded with the element-wise cases)
    flat = c._replace(rows=R, groups=1)
    p = plain_act(d, flat, ACT_LRELU, d.slopes, use_res, torch.float64, False)
    pw = plain_act(d, flat, ACT_LRELU, d.slopes, use_res, torch.float32, False)
    wsp = ws_for(L, R, 1, C)
    slopes, dslope, DX = Flat(C, init=d.slopes), Flat(C), Buf(R, C, c.pad, st)
    L.call(f"mi355seg_prelu_bwd_{st}", DY.ptr, DY.ld, X.ptr, X.ld, RES.ptr if use_res else None, RES.ld, slopes.ptr, DX.ptr, DX.ld, dslope.ptr,
           R, C, wsp.ptr, wsp.n, stream())
    wsp.check("prelu_bwd")
    DX.check("prelu_bwd dx")
    grade_sum(rep, "prelu_bwd dslope", dslope.check("dslope"), p.ds_addend.sum(0), p.ds_addend.abs().sum(0), wit=pw.ds_addend.sum(0))

    # ---- group_sums (fp32 tensors only): out[g, c] (+)= alpha sum_r x[g, r, c]
    if st == "f32":
        xd = d.x.double().reshape(G, rows, C)
        for accumulate in (0, 1):
            init = rnd(G, C, seed=77)
            out = Flat(G * C, init=init)
            L.call("mi355seg_group_sums_f32", X.ptr, X.ld, rows, G, C, 0.5, out.ptr, accumulate, ws.ptr, ws.n, stream())
            ws.check("group_sums")
            ref = 0.5 * xd.sum(1) + (init.double() if accumulate else 0.0)
            wit = 0.5 * d.x.reshape(G, rows, C).sum(1) + (init if accumulate else 0.0)
            grade_sum(rep, f"group_sums acc={accumulate}", out.check("group_sums").reshape(G, C), ref, 0.5 * xd.abs().sum(1) + init.double().abs() * accumulate, wit=wit)
    L.ran(red_entries(c, st), st)


@gpu
@pytest.mark.parametrize("st", STORAGE)
@pytest.mark.parametrize("C", RED_REJECTED)
def test_reductions_refuse_channel_counts_without_a_plan(seg, C, st):
    """C = 320 / 2048: MI355SEG_EINVAL with a message, nothing launched, every output and the workspace untouched."""
    L = seg.lib()
    rows = 40
    x = Buf(rows, C, 4, st, data=stored(rnd(rows, C, seed=5), st))
    dx = Buf(rows, C, 4, st)
    a, b, e, f, g, h = (Flat(C) for _ in range(6))
    par = Flat(C, init=torch.ones(C))
    ws = ws_for(L, rows, 1, C)
    ws.buf[:ws.n] = 0x5A
    calls = {
        "norm_stats": (x.ptr, x.ld, rows, 1, C, EPS, a.ptr, b.ptr, None, None, MOMENTUM, ws.ptr, ws.n, stream()),
        "norm_act_bwd_sums": (x.ptr, x.ld, x.ptr, x.ld, par.ptr, par.ptr, None, None, None, 0, a.ptr, b.ptr, e.ptr, f.ptr, rows, 1, C, ACT_RELU, 0.0,
                              ws.ptr, ws.n, stream()),
        "prelu_bwd": (x.ptr, x.ld, x.ptr, x.ld, None, 0, par.ptr, dx.ptr, dx.ld, g.ptr, rows, C, ws.ptr, ws.n, stream()),
        "norm_act_bwd": (x.ptr, x.ld, x.ptr, x.ld, par.ptr, par.ptr, None, None, None, 0, dx.ptr, dx.ld, e.ptr, f.ptr, None, 0, rows, 1, C, ACT_RELU, 0.0,
                         ws.ptr, ws.n, stream()),
    }
    for name, args in calls.items():
        rc = L.query(f"mi355seg_{name}_{st}", *args)
        msg = L.query("mi355seg_last_error").decode()
        assert rc == EINVAL and "unsupported channel count" in msg and str(C) in msg, (name, rc, msg)
    torch.cuda.synchronize()
    for t in (a, b, e, f, g, h):
        assert bool(torch.isnan(t.check("rejected")).all())
    dx.check("rejected dx")
    assert bool((ws.buf[:ws.n] == 0x5A).all())
    ws.check("rejected")


# ----------------------------------------------------------------------------- element-wise
@gpu
@pytest.mark.parametrize("st", STORAGE)
@pytest.mark.parametrize("index", range(len(EW_CASES)), ids=[c.name for c in EW_CASES])
def test_elementwise_entry_points_against_fp64(seg, index, st):
    """Every element-wise entry point of norm_api.inc on one geometry of the table, in each activation the case lists; with and without
    residual / dres / affine pair / addend as the activation code and the case index rotate."""
    L = Recorder(seg.lib())
    c = EW_CASES[index]
    G, rows, C, R = c.groups, c.rows, c.C, c.groups * c.rows
    d = case_data("ew", index, st)
    rep = Report(f"{c.name}/{st}")
    new = lambda: Buf(R, C, c.pad, st, off=c.off)
    X, DY, RES, ADD = (Buf(R, C, c.pad, st, data=t, off=c.off) for t in (d.x, d.dy, d.res, d.addend))
    mean, rstd = Flat(G * C, init=d.mean), Flat(G * C, init=d.rstd)
    gamma, beta = Flat(C, init=d.gamma), Flat(C, init=d.beta)
    ws = ws_for(L, rows, G, C)
    flat = c._replace(rows=R, groups=1)
    full = lambda t: t.reshape(R, C)
    no_plan = red_plan(rows, C, X.ld) is None
    assert no_plan == (c.name in TWO_TRIP_CASES)

    for act in c.acts:
        use_res, use_aff = (act + index) % 2 == 1, (act + index) % 3 != 0
        o = chain(d, c, act, SLOPE, use_res, use_aff, torch.float64)
        w = chain(d, c, act, SLOPE, use_res, use_aff, torch.float32, given=o.given)
        amb_f = ambiguous(o.zf, o.Szf, act, f"{c.name} act {act} forward")
        amb_b = ambiguous(o.z, o.Sz, act, f"{c.name} act {act} backward")
        ga, be = (gamma.ptr, beta.ptr) if use_aff else (None, None)
        rs = RES.ptr if use_res else None
        tag = f"[act {act}{' res' if use_res else ''}{' aff' if use_aff else ''}]"

        # norm_act_fwd, and its _ax form: the same y, and max |y| as written
        Y = new()
        L.call(f"mi355seg_norm_act_fwd_{st}", X.ptr, X.ld, mean.ptr, rstd.ptr, ga, be, rs, RES.ld, Y.ptr, Y.ld, rows, G, C, act, SLOPE, stream())
        y = Y.check("norm_act_fwd")
        grade_elem(rep, "norm_act_fwd " + tag, y, full(o.y), full(o.Sy), st, alt=full(o.y_alt), amb=full(amb_f), wit=full(w.y))
        Y2 = new()
        y2 = expect_amax(L, lambda slot: L.call(f"mi355seg_norm_act_fwd_ax_{st}", X.ptr, X.ld, mean.ptr, rstd.ptr, ga, be, rs, RES.ld, Y2.ptr, Y2.ld, rows, G, C,
                                                act, SLOPE, slot, stream()), lambda: Y2.check("norm_act_fwd_ax"), f"{rep.name} norm_act_fwd_ax {tag}")
        grade_elem(rep, "norm_act_fwd_ax " + tag, y2, full(o.y), full(o.Sy), st, alt=full(o.y_alt), amb=full(amb_f), wit=full(w.y))

        # norm_act_bwd_apply on the given s1 / s2 (+ dres with a residual, + dx_colsum where the case asks), and its _ax form
        s1, s2 = Flat(G * C, init=o.given[0]), Flat(G * C, init=o.given[1])
        DX, DR = new(), new()
        colsum = Flat(C) if c.colsum else None
        L.call(f"mi355seg_norm_act_bwd_apply_{st}", DY.ptr, DY.ld, X.ptr, X.ld, mean.ptr, rstd.ptr, ga, be, rs, RES.ld, s1.ptr, s2.ptr, DX.ptr, DX.ld,
               DR.ptr if use_res else None, DR.ld, colsum.ptr if colsum else None, rows, G, C, act, SLOPE, ws.ptr, ws.n, stream())
        ws.check("norm_act_bwd_apply")
        dx = DX.check("norm_act_bwd_apply dx")
        grade_elem(rep, "norm_act_bwd_apply dx " + tag, dx, full(o.dx), full(o.Sdx), st, alt=full(o.dx_alt), amb=full(amb_b), wit=full(w.dx))
        dr = DR.check("norm_act_bwd_apply dres")
        if use_res:
            grade_elem(rep, "norm_act_bwd_apply dres " + tag, dr, full(o.dz), full(o.Sdz), st, alt=full(o.dz_alt), amb=full(amb_b), wit=full(w.dz))
        else:
            assert bool((dr == 7.0).all())
        if colsum:
            grade_colsum(rep, "bwd_apply dx_colsum " + tag, colsum.check("dx_colsum"), c.colsum[0], o, w, amb_b, dx)
        DX2, DR2 = new(), new()
        colsum2 = Flat(C) if c.colsum else None
        dx2 = expect_amax(L, lambda slot: L.call(f"mi355seg_norm_act_bwd_apply_ax_{st}", DY.ptr, DY.ld, X.ptr, X.ld, mean.ptr, rstd.ptr, ga, be, rs, RES.ld, s1.ptr,
                                                 s2.ptr, DX2.ptr, DX2.ld, DR2.ptr if use_res else None, DR2.ld, colsum2.ptr if colsum2 else None, slot,
                                                 rows, G, C, act, SLOPE, ws.ptr, ws.n, stream()), lambda: DX2.check("norm_act_bwd_apply_ax dx"),
                          f"{rep.name} norm_act_bwd_apply_ax {tag}")
        ws.check("norm_act_bwd_apply_ax")
        assert torch.equal(dx2, dx) and torch.equal(DR2.check("norm_act_bwd_apply_ax dres"), dr)
        if colsum:
            assert torch.equal(colsum2.check("dx_colsum"), colsum.check("dx_colsum"))

        # the composed backward against the fp64 chain: its own s1 / s2 sit inside the workspace
        S_comp = o.Sdx + 0.5 * o.gr.abs() * (o.a.abs().sum(1, keepdim=True) + o.xh.abs() * o.b.abs().sum(1, keepdim=True)) / rows
        S_comp = S_comp + o.gr.abs() * (amb_slack(amb_b, o.a, o.a_alt).unsqueeze(1) + o.xh.abs() * amb_slack(amb_b, o.b, o.b_alt).unsqueeze(1)) / rows / (8 * 2.0 ** -24)
        affine_grads = G == 1 and use_aff
        for entry in ("norm_act_bwd",) + (("norm_act_bwd_colsum", "norm_act_bwd_colsum_ax") if c.colsum else ()):
            DX3, DR3, dg, db, cs, am = new(), new(), Flat(C), Flat(C), Flat(C), Flat(1, init=torch.zeros(1))
            args = [DY.ptr, DY.ld, X.ptr, X.ld, mean.ptr, rstd.ptr, ga, be, rs, RES.ld, DX3.ptr, DX3.ld, dg.ptr if affine_grads else None,
                    db.ptr if affine_grads else None, DR3.ptr if use_res else None, DR3.ld]
            args += {"norm_act_bwd": [], "norm_act_bwd_colsum": [cs.ptr], "norm_act_bwd_colsum_ax": [cs.ptr, am.ptr]}[entry]
            if no_plan:         # the reduction in front of the apply pass has no plan for this C: refused as a whole, nothing written
                assert L.query(f"mi355seg_{entry}_{st}", *args, rows, G, C, act, SLOPE, ws.ptr, ws.n, stream()) == EINVAL
                assert "unsupported channel count" in L.query("mi355seg_last_error").decode()
                assert bool((DX3.check(entry + " refused") == 7.0).all())
                continue
            L.call(f"mi355seg_{entry}_{st}", *args, rows, G, C, act, SLOPE, ws.ptr, ws.n, stream())
            ws.check(entry)
            dx3 = DX3.check(entry + " dx")
            grade_elem(rep, f"{entry} dx {tag}", dx3, full(o.dx), full(S_comp), st, alt=full(o.dx_alt), amb=full(amb_b), wit=full(w.dx))
            if use_res:
                assert torch.equal(DR3.check(entry + " dres"), dr)
            if affine_grads:
                grade_sum(rep, f"{entry} dbeta {tag}", db.check("dbeta"), o.a.sum(1)[0], o.a.abs().sum(1)[0], wit=w.a.sum(1)[0], slack=amb_slack(amb_b, o.a, o.a_alt)[0])
                grade_sum(rep, f"{entry} dgamma {tag}", dg.check("dgamma"), o.b.sum(1)[0], o.b.abs().sum(1)[0], wit=w.b.sum(1)[0], slack=amb_slack(amb_b, o.b, o.b_alt)[0])
            if entry != "norm_act_bwd":
                # the composed form's own s1 / s2 lie within 2^-22 sum |addend| (+ what branch-point addends move) of the given ones; through
                # dx = gr (dz - s1 / rows - xhat s2 / rows) a fused column sum moves by at most |gr| (d1 + mean |xhat| d2)
                d1 = 2.0 ** -22 * o.a.abs().sum(1)[0] + amb_slack(amb_b, o.a, o.a_alt)[0]
                d2 = 2.0 ** -22 * o.b.abs().sum(1)[0] + amb_slack(amb_b, o.b, o.b_alt)[0]
                moved = (o.gr.abs() * (d1 + o.xh.abs().mean(1, keepdim=True) * d2)).reshape(-1, C)[0]
                grade_colsum(rep, f"{entry} dx_colsum {tag}", cs.check("dx_colsum"), c.colsum[0], o, w, amb_b, dx3, moved)
            if entry.endswith("_ax"):
                assert bits(am.check("dx_amax").float())[0] == bits(dx3.abs().max().float().reshape(1))[0]

        # act_fwd / act_bwd / act_bwd_add on z = x (+ res): z is one correctly rounded sum, its sign is the fp64 sign -- no branch points
        p = plain_act(d, flat, act, SLOPE, use_res, torch.float64, False)
        pw = plain_act(d, flat, act, SLOPE, use_res, torch.float32, False)
        YA, DXA, DXB = new(), new(), new()
        L.call(f"mi355seg_act_fwd_{st}", X.ptr, X.ld, rs, RES.ld, YA.ptr, YA.ld, R, C, act, SLOPE, stream())
        grade_elem(rep, "act_fwd " + tag, YA.check("act_fwd"), p.y, p.Sy, st, wit=pw.y)
        L.call(f"mi355seg_act_bwd_{st}", DY.ptr, DY.ld, X.ptr, X.ld, rs, RES.ld, DXA.ptr, DXA.ld, R, C, act, SLOPE, stream())
        grade_elem(rep, "act_bwd " + tag, DXA.check("act_bwd"), p.dx, p.Sdx, st, wit=pw.dx)
        q = plain_act(d, flat, act, SLOPE, use_res, torch.float64, True)
        qw = plain_act(d, flat, act, SLOPE, use_res, torch.float32, True)
        L.call(f"mi355seg_act_bwd_add_{st}", DY.ptr, DY.ld, X.ptr, X.ld, rs, RES.ld, ADD.ptr, ADD.ld, DXB.ptr, DXB.ld, R, C, act, SLOPE, stream())
        got_add = DXB.check("act_bwd_add")
        grade_elem(rep, "act_bwd_add " + tag, got_add, q.dx, q.Sdx, st, wit=qw.dx)
        # exactly the fp32 product, rounded, then ONE fp32 sum, stored once: what the former two passes gave on fp32 tensors.  act' is
        # exact for NONE / RELU on every kernel; with the leaky slope the product rounds, so a sum fused into it (fma) would show -- held
        # for the 4-wide / scalar kernel (act_bwd_rows), which is what replaced the two passes; the 8-wide kernel is as it was
        off_wide = ew_select("act_bwd_add", st, C, X.ld, c.off, R)[0] != "wide8"
        if act in (ACT_NONE, ACT_RELU) or (act == ACT_LRELU and off_wide):
            g32 = {ACT_NONE: torch.ones_like(pw.z), ACT_RELU: (pw.z > 0).float(), ACT_LRELU: torch.where(pw.z > 0, 1.0, SLOPE).float()}[act]
            once = (d.dy * g32 + d.addend).to(DT[st]).double()
            assert torch.equal(got_add, once), f"{rep.name} act_bwd_add {tag}: not the rounded product plus the addend, stored once"
        DXC = new()
        L.call(f"mi355seg_act_bwd_add_{st}", DY.ptr, DY.ld, X.ptr, X.ld, rs, RES.ld, None, 0, DXC.ptr, DXC.ld, R, C, act, SLOPE, stream())
        assert torch.equal(DXC.check("act_bwd_add without addend"), DXA.check("act_bwd"))

    # PReLU (per-channel slopes) and the channel scaling, once per case
    for use_res in (False, True):
        p = plain_act(d, flat, ACT_LRELU, d.slopes, use_res, torch.float64, False)
        pw = plain_act(d, flat, ACT_LRELU, d.slopes, use_res, torch.float32, False)
        rs = RES.ptr if use_res else None
        slopes, dslope, YP, DXP = Flat(C, init=d.slopes), Flat(C), new(), new()
        wsp = ws_for(L, R, 1, C)
        L.call(f"mi355seg_prelu_fwd_{st}", X.ptr, X.ld, rs, RES.ld, slopes.ptr, YP.ptr, YP.ld, R, C, stream())
        grade_elem(rep, f"prelu_fwd res={use_res}", YP.check("prelu_fwd"), p.y, p.Sy, st, wit=pw.y)
        if no_plan:
            assert L.query(f"mi355seg_prelu_bwd_{st}", DY.ptr, DY.ld, X.ptr, X.ld, rs, RES.ld, slopes.ptr, DXP.ptr, DXP.ld, dslope.ptr, R, C, wsp.ptr, wsp.n, stream()) == EINVAL
            assert bool((DXP.check("prelu_bwd refused") == 7.0).all()) and bool(torch.isnan(dslope.check("dslope refused")).all())
            continue
        L.call(f"mi355seg_prelu_bwd_{st}", DY.ptr, DY.ld, X.ptr, X.ld, rs, RES.ld, slopes.ptr, DXP.ptr, DXP.ld, dslope.ptr, R, C, wsp.ptr, wsp.n, stream())
        wsp.check("prelu_bwd")
        grade_elem(rep, f"prelu_bwd dx res={use_res}", DXP.check("prelu_bwd"), p.dx, p.Sdx, st, wit=pw.dx)
        grade_sum(rep, f"prelu_bwd dslope res={use_res}", dslope.check("dslope"), p.ds_addend.sum(0), p.ds_addend.abs().sum(0), wit=pw.ds_addend.sum(0))
    scale, YS = Flat(G * C, init=d.scale), new()
    L.call(f"mi355seg_scale_channels_{st}", X.ptr, X.ld, scale.ptr, YS.ptr, YS.ld, rows, G, C, stream())
    ref = (d.x.double().reshape(G, rows, C) * d.scale.double().reshape(G, 1, C)).reshape(R, C)
    grade_elem(rep, "scale_channels", YS.check("scale_channels"), ref, 2 * ref.abs(), st, wit=(d.x.reshape(G, rows, C) * d.scale.reshape(G, 1, C)).reshape(R, C))
    L.ran(ew_entries(c), st)
    worst = {}
    for what, ratio in rep.lines:
        worst[what.split(" [")[0]] = max(worst.get(what.split(" [")[0], 0.0), ratio)
    print(f"{rep.name}: largest err / bound per entry point: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
