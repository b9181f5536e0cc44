"""The pooling kernels (csrc/pool.hip, csrc/pool_api.inc) and the row / channel glue of csrc/api.hip against the same operation
written plainly on the CPU, in fp32 and bf16 storage, through the C ABI with guarded, pitched outputs (test_gpu_conv_paths.py's
conventions; the typed buffers are in stream_grading.py).

THE SELECTION TABLE IS A MIRROR: the library does not say which pooling kernel ran.  ``pool_select`` re-writes the launchers' choice
(4-wide when C and every pitch are multiples of 4 -- and, for maxpool2_bwd_add, the ``add`` pointer is aligned to four elements --
else scalar; the grid capped at 8192 blocks of 256 threads, past which the grid-stride loops take a second trip) with the cap read from
pool.hip by regex; the host-only tests assert each case reaches what it names and every listed selection is reached per kernel and
storage type.

References and bounds.
  * max-pool forward (values and argmax codes), its backward, the upsampling forward, copies, channel repeats, casts of representable
    values and the layout transposes select or move values: bit-exact (torch.equal).  The max-pool reference is ATen-CPU max_pool3d
    with indices: the first maximum in scan order wins, a NaN wins over everything and takes the gradient.
  * maxpool2_bwd_add, add_rows, add_bias are one correctly rounded sum per element: bit-exact against that sum in fp32, rounded once to
    the storage type.  On odd extents the trailing planes get exactly 0, or exactly ``add``.
  * sums of a few terms (upsample2_bwd: 8, repeat_channels_bwd: rep) and the products of mix / broadcast / gate:
    |got - ref| <= 8 * 2^-24 * S, S = the fp64 sum of |every term| + |result| (bf16: + 2^-8 |ref|), fp64 reference.
    gate: g = 2 - sigmoid(t) goes through expf: S = |enc| (g + 1); dt = -s (1 - s) sum_c dy enc: C products and C - 1 sums are at
    most 2 C roundings = C / 4 units of S, and 1 - s cancels for large t (the terms 1 and s enter it): S = (C / 4) s (1 + s) sum |dy enc|.
"""
import functools
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as TF

from stream_grading import EINVAL, GUARD_ELEMS, Buf, Flat, Report, constant, grade_elem, pinned, rnd, source, stored, stream, DT

gpu = pytest.mark.gpu           # per test: the table checks need no GPU and run with -m "not gpu"
STORAGE = ("f32", "bf16")
ESIZE = {"f32": 4, "bf16": 2}
POOL_KERNELS = ("maxpool2_fwd", "maxpool2_bwd", "maxpool2_bwd_add", "upsample2_fwd", "upsample2_bwd")


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
    pool, api = source("pool.hip"), source("pool_api.inc")
    cap = constant(r"static int pgrid\(long long total\) \{.*?b > (\d+) \? (\d+) : b\)\);", pool, "pgrid: block cap")
    threads = constant(r"static int pgrid\(long long total\) \{\s*long long b = \(total \+ \d+\) / (\d+);", pool, "pgrid: threads per block")
    pinned(r"hipLaunchKernelGGL\(\(KERN<TT, true>\), dim3\(pgrid\(total\)\), dim3\(256\)", pool, "POOL_DISPATCH: block size")
    for what, pat in (("maxpool2_fwd", r"bool v = \(C % 4 == 0\) && \(ldx % 4 == 0\) && \(ldy % 4 == 0\);\s*long long total = \(long long\)N \* \(D / 2\) \* \(H / 2\) \* \(W / 2\) \* \(v \? C / 4 : C\);"),
                      ("maxpool2_bwd", r"bool v = \(C % 4 == 0\) && \(lddy % 4 == 0\) && \(lddx % 4 == 0\);\s*long long total = \(long long\)N \* D \* H \* W \* \(v \? C / 4 : C\);"),
                      ("maxpool2_bwd_add", r"bool v = \(C % 4 == 0\) && \(lddy % 4 == 0\) && \(lddx % 4 == 0\) && \(ldadd % 4 == 0\) && \(\(uintptr_t\)add % \(4 \* sizeof\(TT\)\)\) == 0;"),
                      ("upsample2_fwd", r"bool v = \(C % 4 == 0\) && \(ldx % 4 == 0\) && \(ldy % 4 == 0\);\s*long long total = \(long long\)N \* D \* H \* W \* 8 \* \(v \? C / 4 : C\);"),
                      ("upsample2_bwd", r"bool v = \(C % 4 == 0\) && \(lddy % 4 == 0\) && \(lddx % 4 == 0\);\s*long long total = \(long long\)N \* D \* H \* W \* \(v \? C / 4 : C\);\s*ProfScope[^\n]*\n\s*POOL_DISPATCH\(upsample2_bwd_kernel")):
        pinned(pat, api, what + ": vector predicate and thread count")
    return cap, threads


def pool_select(kernel, N, D, H, W, C, ld, add_off=0, st="f32"):
    """-> (kind, grid capped).  D, H, W are the extents of the FULL-resolution tensor (max-pool input, upsampling output)."""
    v = C % 4 == 0 and ld % 4 == 0
    if kernel == "maxpool2_bwd_add":
        v = v and (add_off * ESIZE[st]) % (4 * ESIZE[st]) == 0
    cw = C // 4 if v else C
    threads = {"maxpool2_fwd": N * (D // 2) * (H // 2) * (W // 2), "maxpool2_bwd": N * D * H * W, "maxpool2_bwd_add": N * D * H * W,
               "upsample2_fwd": N * D * H * W, "upsample2_bwd": N * (D // 2) * (H // 2) * (W // 2)}[kernel] * cw
    cap, per = K()
    return ("vec" if v else "scalar"), -(-threads // per) > cap


# name, N, D, H, W (full resolution), C, pad, selection of every kernel at this pitch
Pool = namedtuple("Pool", "name N D H W C pad kind")
POOL_CASES = [
    # C = 32 at pitch 36: C % 4 == 0 and 36 % 4 == 0 -> 4-wide.  2x2x2: one window per sample; 7x5x9: every extent odd, the trailing
    # planes lie outside the pooled grid (inside == false); 8x6x10: even
    Pool("2x2x2-c32", 2, 2, 2, 2, 32, 4, "vec"),
    Pool("7x5x9-c32", 2, 7, 5, 9, 32, 4, "vec"),
    Pool("8x6x10-c32", 2, 8, 6, 10, 32, 4, "vec"),
    # C = 3 fails C % 4 -> scalar (pitch 5)
    Pool("2x2x2-c3", 2, 2, 2, 2, 3, 2, "scalar"),
    Pool("7x5x9-c3", 2, 7, 5, 9, 3, 2, "scalar"),
    Pool("8x6x10-c3", 2, 8, 6, 10, 3, 2, "scalar"),
    # C = 32 at pitch 33: 33 % 4 != 0 -> scalar by the pitch alone
    Pool("2x2x2-c32-p33", 2, 2, 2, 2, 32, 1, "scalar"),
    Pool("7x5x9-c32-p33", 2, 7, 5, 9, 32, 1, "scalar"),
    Pool("8x6x10-c32-p33", 2, 8, 6, 10, 32, 1, "scalar"),
]
# one scalar case per kernel past 8192 * 256 = 2,097,152 threads (C = 33): the kernels with one thread per full-resolution element
# (maxpool2_bwd, maxpool2_bwd_add, upsample2_fwd) at 40x40x42 = 2,217,600 threads, those with one thread per pooled element
# (maxpool2_fwd, upsample2_bwd) at 80x80x84 -> 40x40x42
BIG = {"maxpool2_bwd": (1, 40, 40, 42, 33, 1), "maxpool2_bwd_add": (1, 40, 40, 42, 33, 1), "upsample2_fwd": (1, 40, 40, 42, 33, 1),
       "maxpool2_fwd": (1, 80, 80, 84, 33, 1), "upsample2_bwd": (1, 80, 80, 84, 33, 1)}
GLUE_C = (1, 3, 5, 8, 33)
GLUE_SPATIAL = (5, 7, 9)         # S = 315: no multiple of the 32-voxel transpose tile, of 4 (narrow_layout) or of 256
GLUE_N = 2


def cid(c):
    return c.name


@pytest.mark.parametrize("case", POOL_CASES, ids=cid)
def test_pool_case_reaches_the_selection_it_names(case):
    ld = case.C + case.pad
    for st in STORAGE:
        for kernel in POOL_KERNELS:
            assert pool_select(kernel, case.N, case.D, case.H, case.W, case.C, ld, 0, st) == (case.kind, False), (kernel, st)
        # maxpool2_bwd_add with ``add`` one element into its rows: not aligned to four elements -> scalar whatever C and the pitches are
        assert pool_select("maxpool2_bwd_add", case.N, case.D, case.H, case.W, case.C, ld, 1, st) == ("scalar", False)


def test_every_pool_selection_is_reached_per_kernel_and_storage_type():
    assert K() == (8192, 256)
    for st in STORAGE:
        for kernel in POOL_KERNELS:
            got = {pool_select(kernel, c.N, c.D, c.H, c.W, c.C, c.C + c.pad, 0, st) for c in POOL_CASES}
            N, D, H, W, C, pad = BIG[kernel]
            got.add(pool_select(kernel, N, D, H, W, C, C + pad, 0, st))
            assert got == {("vec", False), ("scalar", False), ("scalar", True)}, (kernel, st, got)
        assert {(c.D, c.H, c.W) for c in POOL_CASES} == {(2, 2, 2), (7, 5, 9), (8, 6, 10)} and {c.N for c in POOL_CASES} == {2}
    S = GLUE_SPATIAL[0] * GLUE_SPATIAL[1] * GLUE_SPATIAL[2]
    assert S % 32 and S % 4 and S % 256


# ----------------------------------------------------------------------------- references
class Bytes:
    """The argmax codes: n bytes between two guard runs of 0xEE (no code is above 7)."""

    def __init__(self, n, init=None):
        self.buf = torch.full((n + 2 * GUARD_ELEMS,), 0xEE, dtype=torch.uint8, device="cuda")
        self.t = self.buf[GUARD_ELEMS:GUARD_ELEMS + n]
        if init is not None:
            self.t.copy_(init.reshape(-1))
        self.ptr = self.t.data_ptr()

    def check(self, what):
        assert bool((self.buf[:GUARD_ELEMS] == 0xEE).all() & (self.buf[-GUARD_ELEMS:] == 0xEE).all()), f"{what}: wrote outside the index buffer"
        return self.t.cpu()


def same(a, b):
    """Bit-for-bit as values: equal where neither is NaN, NaN in the same places."""
    return bool((torch.isnan(a) == torch.isnan(b)).all()) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def pool_reference(x, g):
    """x [N, D, H, W, C] (fp64) -> y, codes (dz * 4 + dy * 2 + dx of the argmax inside its window), and the gradient of g at x."""
    N, D, H, W, C = x.shape
    xc = x.permute(0, 4, 1, 2, 3).contiguous()
    y, ind = TF.max_pool3d(xc, 2, 2, return_indices=True)
    iz, iy, ix = ind // (H * W), (ind // W) % H, ind % W
    code = ((iz % 2) * 4 + (iy % 2) * 2 + (ix % 2)).to(torch.uint8)
    dx = torch.zeros(N, C, D * H * W, dtype=x.dtype)
    dx.scatter_(2, ind.reshape(N, C, -1), g.permute(0, 4, 1, 2, 3).reshape(N, C, -1))     # windows do not overlap: no two writes meet
    cl = lambda t: t.permute(0, 2, 3, 4, 1).contiguous()
    return cl(y), cl(code), cl(dx.reshape(N, C, D, H, W))


def run_pool(L, rep, st, N, D, H, W, C, pad, x, only=None):
    """All five kernels on one geometry; ``only``: just that kernel (the cases past the grid cap)."""
    Do, Ho, Wo = D // 2, H // 2, W // 2
    full, pooled = N * D * H * W, N * Do * Ho * Wo
    want = lambda k: only is None or only == k
    g = stored(rnd(N, Do, Ho, Wo, C, seed=21), st)
    add = stored(rnd(N, D, H, W, C, seed=22), st)
    if only is None or only.startswith("maxpool2"):
        y_ref, code_ref, dx_ref = pool_reference(x.double(), g.double())
    X = Buf(full, C, pad, st, data=x)
    if want("maxpool2_fwd") or only in ("maxpool2_bwd", "maxpool2_bwd_add"):
        Y, IDX = Buf(pooled, C, pad, st), Bytes(pooled * C)
        L.call(f"mi355seg_maxpool2_fwd_{st}", X.ptr, X.ld, Y.ptr, Y.ld, IDX.ptr, N, D, H, W, C, stream())
        assert same(Y.check("maxpool2_fwd y"), y_ref.reshape(pooled, C)), f"{rep.name}: maxpool2_fwd values"
        assert torch.equal(IDX.check("maxpool2_fwd idx"), code_ref.reshape(-1)), f"{rep.name}: maxpool2_fwd argmax codes"
    G = Buf(pooled, C, pad, st, data=g)
    if want("maxpool2_bwd"):
        DX = Buf(full, C, pad, st)
        L.call(f"mi355seg_maxpool2_bwd_{st}", G.ptr, G.ld, IDX.ptr, DX.ptr, DX.ld, N, D, H, W, C, stream())
        dx = DX.check("maxpool2_bwd dx")
        assert torch.equal(dx, dx_ref.reshape(full, C)), f"{rep.name}: maxpool2_bwd"
        outside = torch.zeros(N, D, H, W, dtype=torch.bool)
        outside[:, 2 * Do:], outside[:, :, 2 * Ho:], outside[:, :, :, 2 * Wo:] = True, True, True
        assert bool((dx.reshape(N, D, H, W, C)[outside] == 0).all())
        IDX.check("maxpool2_bwd idx")
    if want("maxpool2_bwd_add"):
        once = (dx_ref.float() + add.float()).to(DT[st]).double().reshape(full, C)        # one fp32 sum, one rounding to the storage type
        for off in ((0, 1) if only is None else (0,)):
            ADD = Buf(full, C, pad + (4 if off else 0), st, data=add, off=off)           # (pitch + 4: the offset fits, pitch % 4 unchanged)
            DX = Buf(full, C, pad, st)
            L.call(f"mi355seg_maxpool2_bwd_add_{st}", G.ptr, G.ld, IDX.ptr, ADD.ptr, ADD.ld, DX.ptr, DX.ld, N, D, H, W, C, stream())
            assert torch.equal(DX.check("maxpool2_bwd_add dx"), once), f"{rep.name}: maxpool2_bwd_add, add {off} elements into its rows"
    if want("upsample2_fwd"):           # the pooled-resolution g, doubled to D', H', W' = 2 Do, 2 Ho, 2 Wo
        UP = Buf(pooled * 8, C, pad, st)
        L.call(f"mi355seg_upsample2_fwd_{st}", G.ptr, G.ld, UP.ptr, UP.ld, N, Do, Ho, Wo, C, stream())
        ref = g.double().repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3)
        assert torch.equal(UP.check("upsample2_fwd"), ref.reshape(pooled * 8, C)), f"{rep.name}: upsample2_fwd"
    if want("upsample2_bwd"):           # the adjoint on the even part of x: each pooled voxel sums its 8 children
        xe = torch.nan_to_num(x[:, :2 * Do, :2 * Ho, :2 * Wo], nan=0.5, posinf=2.0, neginf=-2.0).contiguous()     # (the special-value case: a sum wants finite terms)
        XE = Buf(pooled * 8, C, pad, st, data=xe)
        DG = Buf(pooled, C, pad, st)
        L.call(f"mi355seg_upsample2_bwd_{st}", XE.ptr, XE.ld, DG.ptr, DG.ld, N, Do, Ho, Wo, C, stream())
        w = xe.reshape(N, Do, 2, Ho, 2, Wo, 2, C)
        ref, S = w.double().sum((2, 4, 6)), w.double().abs().sum((2, 4, 6))
        grade_elem(rep, "upsample2_bwd", DG.check("upsample2_bwd"), ref.reshape(pooled, C), (S + ref.abs()).reshape(pooled, C), st, wit=w.sum((2, 4, 6)).reshape(pooled, C))


@gpu
@pytest.mark.parametrize("st", STORAGE)
@pytest.mark.parametrize("case", POOL_CASES, ids=cid)
def test_pool_kernels_are_exact(seg, case, st):
    x = stored(rnd(case.N, case.D, case.H, case.W, case.C, seed=20), st)
    run_pool(seg.lib(), Report(f"{case.name}/{st}"), st, case.N, case.D, case.H, case.W, case.C, case.pad, x)


@gpu
@pytest.mark.parametrize("st", STORAGE)
@pytest.mark.parametrize("kernel", POOL_KERNELS)
def test_pool_kernel_past_the_grid_cap(seg, kernel, st):
    """More threads than 8192 blocks hold: the grid-stride loop's second trip, scalar form (C = 33)."""
    N, D, H, W, C, pad = BIG[kernel]
    x = stored(rnd(N, D, H, W, C, seed=23), st)
    run_pool(seg.lib(), Report(f"{kernel}-big/{st}"), st, N, D, H, W, C, pad, x, only=kernel)


@gpu
@pytest.mark.parametrize("st", STORAGE)
@pytest.mark.parametrize("C,pad", [(4, 4), (3, 2)])
def test_pool_ties_infinities_and_nan(seg, C, pad, st):
    """Exact ties (the first in scan order wins), a window of all -inf, +inf, one NaN in a window (it wins and takes the gradient),
    two NaNs in a window -- in the 4-wide and the scalar kernel."""
    N, D, H, W = 1, 4, 4, 4
    x = stored(rnd(N, D, H, W, C, seed=24), st)
    inf, nan = float("inf"), float("nan")
    x[0, 0:2, 0:2, 0:2] = 1.5                    # window (0, 0, 0): all equal
    x[0, 0:2, 0:2, 2:4] = -inf                   # window (0, 0, 1): all -inf
    x[0, 0, 3, 1] = inf                          # window (0, 1, 0): +inf
    x[0, 1, 2, 3] = nan                          # window (0, 1, 1): one NaN, in front of and behind larger finite values
    x[0, 1, 3, 3] = 100.0
    x[0, 0, 2, 2] = 100.0
    x[0, 2, 0, 1], x[0, 3, 1, 0] = nan, nan      # window (1, 0, 0): two NaNs
    x[0, 2:4, 0:2, 2:4, 0] = 0.25                # window (1, 0, 1), channel 0 only: a tie beside untied channels
    x[0, 3, 2, 0], x[0, 2, 3, 1] = 9.0, 9.0      # window (1, 1, 0): the maximum twice
    run_pool(seg.lib(), Report(f"special-c{C}/{st}"), st, N, D, H, W, C, pad, x)


@gpu
@pytest.mark.parametrize("st", STORAGE)
def test_maxpool_refuses_a_single_plane(seg, st):
    """D = 1: MI355SEG_EINVAL with a message, nothing written."""
    L = seg.lib()
    N, D, H, W, C = 2, 1, 4, 4, 4
    X = Buf(N * D * H * W, C, 4, st, data=stored(rnd(N * D * H * W, C, seed=1), st))
    Y, IDX = Buf(N * 4, C, 4, st), Bytes(N * 4 * C)
    for name, args in (("maxpool2_fwd", (X.ptr, X.ld, Y.ptr, Y.ld, IDX.ptr, N, D, H, W, C, stream())),
                       ("maxpool2_bwd", (Y.ptr, Y.ld, IDX.ptr, X.ptr, X.ld, N, D, H, W, C, stream())),
                       ("maxpool2_bwd_add", (Y.ptr, Y.ld, IDX.ptr, X.ptr, X.ld, X.ptr, X.ld, N, D, H, W, C, stream()))):
        rc = L.query(f"mi355seg_{name}_{st}", *args)
        msg = L.query("mi355seg_last_error").decode()
        assert rc == EINVAL and name in msg, (name, rc, msg)
    torch.cuda.synchronize()
    assert bool((Y.check("refused") == 7.0).all()) and bool((IDX.check("refused") == 0xEE).all())


# ----------------------------------------------------------------------------- glue
def exact_sum(a, b, st):
    return (a.float() + b.float()).to(DT[st]).double()


@gpu
@pytest.mark.parametrize("st", STORAGE)
@pytest.mark.parametrize("C", GLUE_C)
def test_row_and_channel_glue(seg, C, st):
    """copy_rows, add_rows, add_bias, repeat_channels and its adjoint, the casts and the layout transposes, N = 2, 315 voxels per
    sample, every destination pitched; for fp32 also mix_channels, broadcast_channels and (C % 4 == 0) the reverse-attention gate."""
    L = seg.lib()
    N, S = GLUE_N, GLUE_SPATIAL[0] * GLUE_SPATIAL[1] * GLUE_SPATIAL[2]
    R, pad, rep_n = N * S, 3 if C % 4 else 4, 3
    rep = Report(f"glue-c{C}/{st}")
    a, b = stored(rnd(R, C, seed=31), st), stored(rnd(R, C, seed=32), st)
    A = Buf(R, C, pad, st, data=a)

    DST = Buf(R, C, pad + 1, st)                                   # another pitch than the source's
    L.call(f"mi355seg_copy_rows_{st}", A.ptr, A.ld, DST.ptr, DST.ld, R, C, stream())
    assert torch.equal(DST.check("copy_rows"), a.double())
    ACC = Buf(R, C, pad, st)
    ACC.t.copy_(b)
    L.call(f"mi355seg_add_rows_{st}", A.ptr, A.ld, ACC.ptr, ACC.ld, R, C, stream())
    assert torch.equal(ACC.check("add_rows"), exact_sum(a, b, st))
    bias = 0.5 * rnd(C, seed=33)
    ACC.t.copy_(b)
    BIAS = Flat(C, init=bias)
    L.call(f"mi355seg_add_bias_{st}", ACC.ptr, ACC.ld, BIAS.ptr, R, C, stream())
    BIAS.check("add_bias bias")
    assert torch.equal(ACC.check("add_bias"), exact_sum(b, bias.expand(R, C), st))

    REP = Buf(R, C * rep_n, pad, st)
    L.call(f"mi355seg_repeat_channels_{st}", A.ptr, A.ld, REP.ptr, REP.ld, R, C, rep_n, stream())
    assert torch.equal(REP.check("repeat_channels"), a.double().repeat(1, rep_n))
    wide = stored(rnd(R, C * rep_n, seed=34), st)
    WIDE, BACK = Buf(R, C * rep_n, pad, st, data=wide), Buf(R, C, pad, st)
    L.call(f"mi355seg_repeat_channels_bwd_{st}", WIDE.ptr, WIDE.ld, BACK.ptr, BACK.ld, R, C, rep_n, stream())
    w3 = wide.reshape(R, rep_n, C)
    ref = w3.double().sum(1)
    grade_elem(rep, "repeat_channels_bwd", BACK.check("repeat_channels_bwd"), ref, w3.double().abs().sum(1) + ref.abs(), st, wit=w3.sum(1))

    # casts of values both types hold, and the transposes between [N, C, S] and [N, S, ld]
    v = stored(rnd(R, C, seed=35), "bf16")
    V32, V16 = Buf(R, C, pad, "f32", data=v), Buf(R, C, pad, "bf16", data=v)
    if st == "bf16":
        TO16, TO32 = Buf(R, C, pad + 1, "bf16"), Buf(R, C, pad + 1, "f32")
        L.call("mi355seg_cast_f32_to_bf16", V32.ptr, V32.ld, TO16.ptr, TO16.ld, R, C, stream())
        L.call("mi355seg_cast_bf16_to_f32", V16.ptr, V16.ld, TO32.ptr, TO32.ld, R, C, stream())
        assert torch.equal(TO16.check("cast_f32_to_bf16"), v.double()) and torch.equal(TO32.check("cast_bf16_to_f32"), v.double())
    ncs = v.reshape(N, S, C).permute(0, 2, 1).contiguous()         # [N, C, S], the same values channel-first
    NCS = Flat(N * C * S, init=ncs)
    CL = Buf(R, C, pad, st)
    L.call("mi355seg_ncdhw_to_ndhwc_f32" if st == "f32" else "mi355seg_ncdhw_f32_to_ndhwc_bf16", NCS.ptr, CL.ptr, CL.ld, N, C, S, stream())
    assert torch.equal(CL.check("to channel-last"), v.double())
    OUT = Flat(N * C * S)
    SRC = V32 if st == "f32" else V16
    L.call("mi355seg_ndhwc_to_ncdhw_f32" if st == "f32" else "mi355seg_ndhwc_bf16_to_ncdhw_f32", SRC.ptr, SRC.ld, OUT.ptr, N, C, S, stream())
    assert torch.equal(OUT.check("to channel-first"), ncs.double().reshape(-1))

    if st != "f32":
        return
    a1, b1 = rnd(N, C, seed=36), rnd(N, C, seed=37)
    B, MIX, A1, B1 = Buf(R, C, pad + 1, st, data=b), Buf(R, C, pad, st), Flat(N * C, init=a1), Flat(N * C, init=b1)
    L.call("mi355seg_mix_channels_f32", A.ptr, A.ld, A1.ptr, B.ptr, B.ld, B1.ptr, MIX.ptr, MIX.ld, S, N, C, stream())
    t1, t2 = a.double().reshape(N, S, C) * a1.double().reshape(N, 1, C), b.double().reshape(N, S, C) * b1.double().reshape(N, 1, C)
    wit = a.reshape(N, S, C) * a1.reshape(N, 1, C) + b.reshape(N, S, C) * b1.reshape(N, 1, C)
    grade_elem(rep, "mix_channels", MIX.check("mix_channels"), (t1 + t2).reshape(R, C), (t1.abs() + t2.abs() + (t1 + t2).abs()).reshape(R, C), st, wit=wit.reshape(R, C))
    BC = Buf(R, C, pad, st)
    L.call("mi355seg_broadcast_channels_f32", A1.ptr, 0.3, BC.ptr, BC.ld, S, N, C, stream())
    alpha = float(torch.tensor(0.3, dtype=torch.float32))
    ref = (alpha * a1.double()).reshape(N, 1, C).expand(N, S, C).reshape(R, C)
    grade_elem(rep, "broadcast_channels", BC.check("broadcast_channels"), ref, 2 * ref.abs(), st)
    if C % 4 == 0:
        run_gate(L, rep, R, C, pad, a, b)


def run_gate(L, rep, R, C, pad, a, b):
    """gate_fwd / gate_bwd (fp32 only) on R rows of C channels at pitch C + pad."""
    st = "f32"
    t = 2.0 * rnd(R, seed=38)
    A, T = Buf(R, C, pad, st, data=a), Buf(R, 1, 1, st, data=t.reshape(R, 1))
    Y, DE, DT_, DYB = Buf(R, C, pad, st), Buf(R, C, pad, st), Flat(R), Buf(R, C, pad, st, data=b)
    L.call("mi355seg_gate_fwd_f32", A.ptr, A.ld, T.ptr, T.ld, Y.ptr, Y.ld, R, C, stream())
    s = torch.sigmoid(t.double()).reshape(R, 1)
    gate = 2.0 - s
    grade_elem(rep, "gate_fwd", Y.check("gate_fwd"), a.double() * gate, a.double().abs() * (gate + 1.0), st, wit=a * (2.0 - torch.sigmoid(t)).reshape(R, 1))
    L.call("mi355seg_gate_bwd_f32", DYB.ptr, DYB.ld, A.ptr, A.ld, T.ptr, T.ld, DE.ptr, DE.ld, DT_.ptr, R, C, stream())
    grade_elem(rep, "gate_bwd denc", DE.check("gate_bwd denc"), b.double() * gate, b.double().abs() * (gate + 1.0), st)
    prod = b.double() * a.double()
    coef = s * (1.0 - s)
    # C products and C - 1 sums: at most 2 C roundings, 8 per unit of S -> C / 4 units; 1 - s has the terms 1 and s entering it (it cancels
    # for large t), so the coefficient's magnitude for S is s (1 + s), which also covers the coefficient's own few roundings
    grade_elem(rep, "gate_bwd dt", DT_.check("gate_bwd dt").reshape(R, 1), -coef * prod.sum(1, keepdim=True), (C / 4.0) * s * (1.0 + s) * prod.abs().sum(1, keepdim=True), st)


@gpu
@pytest.mark.parametrize("C", (4, 12, 64, 512))
def test_gate_lanes_per_row(seg, C):
    """gate_bwd gives a row LPV lanes, the largest power of two <= min(C / 4, 64): 1 (C = 4), 2 with a second quad on one lane (C = 12:
    three quads), 16 (C = 64), 64 with two quads per lane (C = 512); 37 rows leave the last wavefront partly idle."""
    pinned(r"int LPV = 1;\s*while \(LPV \* 2 <= C / 4 && LPV \* 2 <= 64\) LPV \*= 2;", source("api.hip"), "gate_bwd: lanes per row")
    R = 37
    run_gate(seg.lib(), Report(f"gate-c{C}/f32"), R, C, 4, rnd(R, C, seed=51), rnd(R, C, seed=52))


@gpu
def test_gate_refuses_channel_counts_off_four(seg):
    """C % 4 != 0 (and a pitch % 4 != 0): MI355SEG_EINVAL with a message, nothing written."""
    L = seg.lib()
    R = 9
    for C, pad in ((6, 2), (8, 1)):
        A, T, Y, DT_ = Buf(R, C, pad, "f32", data=rnd(R, C, seed=53)), Buf(R, 1, 1, "f32", data=rnd(R, 1, seed=54)), Buf(R, C, pad, "f32"), Flat(R)
        assert L.query("mi355seg_gate_fwd_f32", A.ptr, A.ld, T.ptr, T.ld, Y.ptr, Y.ld, R, C, stream()) == EINVAL
        assert "gate_fwd" in L.query("mi355seg_last_error").decode()
        assert L.query("mi355seg_gate_bwd_f32", A.ptr, A.ld, A.ptr, A.ld, T.ptr, T.ld, Y.ptr, Y.ld, DT_.ptr, R, C, stream()) == EINVAL
        assert "gate_bwd" in L.query("mi355seg_last_error").decode()
        torch.cuda.synchronize()
        assert bool((Y.check("refused") == 7.0).all()) and bool(torch.isnan(DT_.check("refused")).all())


@gpu
@pytest.mark.parametrize("st", STORAGE)
def test_narrow_layout_transposes(seg, st):
    """C = 3 with a dense channel-last side and S % 4 == 0: narrow_layout's kernel (four voxels of all channels per thread) instead of the
    32 x 32 tile; S = 316 leaves the last thread group of a sample short of nothing and 2 x 79 groups over two samples."""
    L = seg.lib()
    N, C, S = 2, 3, 316
    pinned(r"if \(C < 2 \|\| C > 4 \|\| ld != C \|\| \(S % 4\) \|\| \(\(\(uintptr_t\)src \| \(uintptr_t\)dst\) % 16\)\) return false;", source("api.hip"), "narrow_layout")
    v = stored(rnd(N * S, C, seed=41), "bf16")
    ncs = v.reshape(N, S, C).permute(0, 2, 1).contiguous()
    NCS, CL = Flat(N * C * S, init=ncs), Buf(N * S, C, 0, st)
    assert NCS.ptr % 16 == 0 and CL.ptr % 16 == 0
    L.call("mi355seg_ncdhw_to_ndhwc_f32" if st == "f32" else "mi355seg_ncdhw_f32_to_ndhwc_bf16", NCS.ptr, CL.ptr, CL.ld, N, C, S, stream())
    assert torch.equal(CL.check("to channel-last"), v.double())
    SRC, OUT = Buf(N * S, C, 0, st, data=v), Flat(N * C * S)
    L.call("mi355seg_ndhwc_to_ncdhw_f32" if st == "f32" else "mi355seg_ndhwc_bf16_to_ncdhw_f32", SRC.ptr, SRC.ld, OUT.ptr, N, C, S, stream())
    assert torch.equal(OUT.check("to channel-first"), ncs.double().reshape(-1))
