"""Every branch of the fp32 Conv3d / ConvTranspose3d k2 s2 dispatch (csrc/conv_generic.hip, csrc/convt_api.inc) against an fp64
convolution of the same unrounded inputs, in all three conv maths.

Each case is the smallest geometry found that satisfies the predicate of one branch and fails the predicates in front of it; after
every call ``mi355seg_last_conv_path()`` says which branch ran, so a case that stops reaching its branch fails with the name of the
branch it reached.  The entry points are called through the C ABI on seeded fp32 tensors:

  * every output lands in a buffer filled with 7.0 that is wider (pitch > channels) and longer (guard rows in front and behind) than
    needed: what the kernel has no business writing must come back untouched;
  * the workspace is exactly what the size query returns, cut from a larger buffer whose next 4 MiB must come back untouched;
  * the reference is torch.nn.functional.conv3d / conv_transpose3d and its autograd in float64 on the CPU; ATen-CPU fp32 on the same
    inputs is the witness, printed beside the kernel's error and its bound (pytest -rA).

Bound (a): max |kernel - fp64| <= max(3e-6, 4 x witness error) x max(1, max |fp64|).  3e-6 is the project's bar for an fp32-accurate
convolution (test_split_precision_conv_is_fp32_accurate); the witness term is for long sums, where ATen's own fp32 error passes that
bar (cases marked "WIT y/dx/dw" below: measured on the CPU, the witness error of those outputs is above 0.75e-6 of the scale, so the
second term decides; every other bound is the plain 3e-6), and the factor 4 is what that test gives the split maths over exact fp32.

Branches no geometry reaches in some math (each a row of DESIGN.md 2.1):
  * WGRAD_MFMA under bf16x6 / f16x3: wgrad_lowp_supported(MATH_X3) in front of it accepts a superset of wgrad_mfma_supported's
    geometries whenever Cin and Cout are multiples of 32, and the fp32 MFMA plan needs exactly that;
  * WGRAD_LOWP_WIDE / WGRAD_LOWP_SWAPPED under fp32 and bf16x6: the wide kernel has only an f16x3 form on fp32 tensors;
  * WGRAD_LOWP_*, WGRAD_PW_LOWP, FWD/DGRAD_MFMA_X3[S], CONVT_*_DIRECT, CONVT_WGRAD_LOWP under fp32: split-precision kernels;
  * FWD/DGRAD_MFMA_X3S under bf16x6 with MFMA shape 32: the shape switch keeps the 16x16x32 tiles off;
  * CONVT_FWD_MFMA / CONVT_DGRAD_MFMA / CONVT_WGRAD_MFMA under the split maths: convt_direct_supported / convt_wgrad_lowp_supported in
    front of them take every geometry whose channel counts the igemm tiles can cut (Cin % 32 == 0, 8 Cout % 32 == 0).
"""
import functools
import re

import pytest
import torch
import torch.nn.functional as TF

gpu = pytest.mark.gpu           # per test: the table check at the end of the file needs no GPU and runs with -m "not gpu"

DEFAULT_MATH = "f16x3"
MATHS = (("fp32", 16), ("bf16x6", 16), ("bf16x6", 32), ("f16x3", 16))
BOUND = 3e-6            # of max(1, max |reference|)
WITNESS_FACTOR = 4.0
SENTINEL = 7.0
GUARD_ROWS = 4          # 4 rows x pitch x 4 bytes: the first row of the payload stays 16-byte aligned
GUARD_ELEMS = 64
BAND = 4 << 20
EPS32 = 2.0 ** -24      # one fp32 rounding


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
    session with exit code 3 ("GPU fault, session ended: ..."), also when the file runs as part of the full suite: read that code as a
    faulted device, not as a collection error."""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"GPU fault, session ended: {e}", returncode=3)


@functools.lru_cache(maxsize=None)
def path_names():
    from mi355seg._lib import HEADER
    return {int(v): k for k, v in re.findall(r"MI355SEG_PATH_(\w+)\s*=\s*(\d+)", open(HEADER).read())}


def last_path(L):
    return path_names()[L.query("mi355seg_last_conv_path")]


def per_math(spec):
    """"NAME" -> the same branch in every math; (fp32, bf16x6 shape 16, bf16x6 shape 32, f16x3) otherwise."""
    return (spec,) * 4 if isinstance(spec, str) else tuple(spec)


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# the k3 / k5 / k1 stride-1 matrix-core family: fp32 MFMA | conv_x3s.hip | the generic split-precision tiles | conv_x3s.hip
IG_FWD = ("FWD_MFMA_F32", "FWD_MFMA_X3S", "FWD_MFMA_X3", "FWD_MFMA_X3S")
IG_DGRAD = ("DGRAD_MFMA_F32", "DGRAD_MFMA_X3S", "DGRAD_MFMA_X3", "DGRAD_MFMA_X3S")
IG_FWD_SMALL = ("FWD_MFMA_F32", "FWD_MFMA_X3", "FWD_MFMA_X3", "FWD_MFMA_X3")                 # W < 8: no 16-wide tiles
IG_DGRAD_SMALL = ("DGRAD_MFMA_F32", "DGRAD_MFMA_X3", "DGRAD_MFMA_X3", "DGRAD_MFMA_X3")
LOWP_WGRAD = ("WGRAD_MFMA", "WGRAD_LOWP_NARROW", "WGRAD_LOWP_NARROW", "WGRAD_LOWP_NARROW")
PW_WGRAD = ("WGRAD_PW_MFMA", "WGRAD_PW_LOWP", "WGRAD_PW_LOWP", "WGRAD_PW_LOWP")

# (N, D, H, W, Cin, Cout, k, s, p), ldx - Cin, ldy - Cout, forward branch, input-gradient branch, weight-gradient branch
CONV_CASES = [
    # ---- matrix-core igemm
    ((1, 6, 6, 6, 64, 64, 3, 1, 1), 4, 4, IG_FWD_SMALL, IG_DGRAD_SMALL, LOWP_WGRAD),
    ((1, 5, 7, 9, 32, 32, 3, 1, 1), 4, 4, IG_FWD, IG_DGRAD, LOWP_WGRAD),                              # odd extents, 16-wide tiles
    ((1, 6, 6, 6, 64, 32, 1, 1, 0), 4, 4, "FWD_MFMA_F32", "DGRAD_MFMA_F32", PW_WGRAD),               # k1: fp32 MFMA in every math
    ((2, 6, 6, 6, 8, 32, 5, 1, 2), 4, 4, "FWD_MFMA_F32", "DGRAD_GENERIC", "WGRAD_GWGRAD"),           # k5, CK = 8; Cin = 8 is no dgrad N-tile  WIT y/dx
    ((1, 8, 8, 16, 32, 32, 5, 1, 2), 4, 4, "FWD_MFMA_F32", "DGRAD_MFMA_F32", LOWP_WGRAD),             # k5: no split igemm, split wgrad  WIT y/dx
    # the same 32 -> 32 k3 layer read through an odd pitch: off the 16-byte staged tiles
    ((1, 5, 7, 9, 32, 32, 3, 1, 1), 1, 4, "FWD_GENERIC", IG_DGRAD_SMALL, "WGRAD_GENERIC"),
    # ---- kernel = stride as a GEMM (k4 s4 with Cin k^3 >= 256 goes here too, in front of the gather igemm)
    ((1, 16, 16, 16, 1, 8, 16, 16, 0), 1, 4, "FWD_PATCH_EMBED", "DGRAD_GENERIC", "WGRAD_PATCH_EMBED"),
    ((1, 8, 8, 32, 16, 32, 4, 4, 0), 4, 4, "FWD_PATCH_EMBED", "DGRAD_GENERIC", "WGRAD_PATCH_EMBED"),   # WIT y
    # ---- gather igemm; its dgrad needs Cin % 32 == 0 (the N-tiles) and four W groups per phase
    ((1, 9, 11, 34, 16, 32, 3, 2, 1), 4, 4, "FWD_GATHER", "DGRAD_GENERIC", "WGRAD_GWGRAD"),
    ((1, 9, 11, 34, 32, 32, 3, 2, 1), 4, 4, "FWD_GATHER", "DGRAD_GATHER", "WGRAD_GWGRAD"),
    ((1, 9, 11, 7, 32, 32, 3, 2, 1), 4, 4, "FWD_GATHER", "DGRAD_GENERIC", "WGRAD_GWGRAD"),           # W / stride = 3 groups
    ((1, 6, 6, 12, 16, 32, 2, 1, 0), 4, 4, "FWD_GATHER", "DGRAD_GENERIC", "WGRAD_GWGRAD"),           # even kernel, stride 1
    ((1, 9, 9, 17, 64, 32, 3, 2, 0), 4, 4, "FWD_GATHER", "DGRAD_GATHER", "WGRAD_GWGRAD"),            # no padding, CK = 64
    ((2, 8, 8, 16, 16, 32, 2, 2, 0), 4, 4, "FWD_GATHER", "DGRAD_K2S2_CONVT", "WGRAD_GWGRAD"),        # k2 s2 dgrad = ConvT forward
    # ---- z-marching head, Cout = 2
    ((2, 9, 10, 33, 16, 2, 3, 1, 1), 4, 2, "FWD_HEADK", "DGRAD_HEADK", "WGRAD_HEADK"),   # WIT y
    ((1, 6, 9, 7, 48, 2, 5, 1, 2), 4, 2, "FWD_HEADK", "DGRAD_HEADK", "WGRAD_HEADK"),                  # three channel passes  WIT y
    ((1, 37, 11, 45, 32, 2, 5, 1, 2), 4, 2, "FWD_HEADK", "DGRAD_HEADK", "WGRAD_HEADK"),               # two z segments meet  WIT y/dx
    # ---- k5 stem, Cin 1 | 2
    ((1, 8, 8, 64, 1, 16, 5, 1, 2), 1, 4, "FWD_STEMK", "DGRAD_GENERIC", "WGRAD_SMALLCIN_K5_TILED"),   # WIT dx
    ((2, 6, 8, 64, 1, 16, 5, 1, 2), 1, 4, "FWD_STEMK", "DGRAD_GENERIC", "WGRAD_SMALLCIN_K5_TILED"),   # WIT dx
    ((2, 8, 8, 16, 1, 16, 5, 1, 2), 1, 4, "FWD_STEMK", "DGRAD_GENERIC", "WGRAD_SMALLCIN"),            # W % 64: the untiled sibling  WIT dx
    ((1, 35, 9, 37, 2, 8, 5, 1, 2), 2, 4, "FWD_STEMK", "DGRAD_GENERIC", "WGRAD_SMALLCIN"),   # WIT dx
    # ---- k3 stem
    ((1, 5, 6, 7, 1, 8, 3, 1, 1), 1, 4, "FWD_STEM_C1", "DGRAD_GENERIC", "WGRAD_STEM"),
    ((1, 5, 6, 7, 2, 8, 3, 1, 1), 1, 4, "FWD_STEM_C2", "DGRAD_GENERIC", "WGRAD_STEM"),
    ((1, 8, 8, 16, 4, 32, 3, 1, 1), 4, 4, "FWD_STEM_C4", "DGRAD_GENERIC", "WGRAD_STEM_C4"),
    ((1, 8, 8, 16, 4, 32, 3, 1, 1), 2, 4, "FWD_STEM_C4", "DGRAD_GENERIC", "WGRAD_STEM"),              # ldx = 6: off stem4_wgrad_kernel
    ((1, 4, 8, 32, 1, 32, 3, 1, 1), 1, 4, "FWD_STEM_TILED", "DGRAD_GENERIC", "WGRAD_STEM_TILED"),     # 16 tiles
    ((1, 32, 48, 48, 1, 64, 3, 1, 1), 1, 4, "FWD_STEM_TILED_STATS", "DGRAD_GENERIC", "WGRAD_STEM_TILED"),   # 576 tiles  WIT dw
    ((1, 32, 64, 64, 1, 64, 3, 1, 1), 1, 4, "FWD_STEM_TILED_STATS", "DGRAD_GENERIC", "WGRAD_STEM_TILED"),   # 1,024 tiles > 768 blocks  WIT dw
    # ---- pointwise with at most 4 channels on either side, k1 heads
    ((1, 4, 6, 8, 3, 4, 1, 1, 0), 1, 1, "FWD_TINYPW", "DGRAD_TINYPW", "WGRAD_TINYPW"),
    ((2, 6, 8, 10, 2, 2, 1, 1, 0), 1, 1, "FWD_TINYPW", "DGRAD_TINYPW", "WGRAD_TINYPW"),
    ((2, 8, 8, 8, 32, 2, 1, 1, 0), 4, 2, "FWD_HEAD", "DGRAD_HEAD", "WGRAD_HEAD"),
    ((1, 4, 4, 8, 256, 4, 1, 1, 0), 4, 4, "FWD_HEAD", "DGRAD_HEAD", "WGRAD_HEAD"),
    # ---- smallcout_wgrad: at an even dy pitch headk_wgrad in front of it takes 32 -> 2 k5, so the odd pitch, Cin = 8 and Cout = 4
    ((1, 8, 8, 16, 32, 2, 5, 1, 2), 4, 1, "FWD_HEADK", "DGRAD_GENERIC", "WGRAD_SMALLCOUT"),   # WIT y
    ((1, 8, 8, 16, 8, 2, 5, 1, 2), 4, 2, "FWD_GENERIC", "DGRAD_HEADK", "WGRAD_SMALLCOUT"),   # WIT y
    ((1, 8, 8, 16, 32, 4, 5, 1, 2), 4, 4, "FWD_GENERIC", "DGRAD_GENERIC", "WGRAD_SMALLCOUT"),   # WIT y
    # ---- pointwise weight gradient: split planes where 32-channel blocks cut, fp32 MFMA otherwise
    ((2, 5, 7, 9, 96, 48, 1, 1, 0), 4, 4, "FWD_GENERIC", "DGRAD_MFMA_F32", PW_WGRAD),
    ((1, 6, 6, 6, 16, 16, 1, 1, 0), 4, 4, "FWD_GENERIC", "DGRAD_GENERIC", "WGRAD_PW_MFMA"),
    # ---- generic
    ((1, 7, 9, 11, 3, 5, 3, 1, 1), 1, 1, "FWD_GENERIC", "DGRAD_GENERIC", "WGRAD_GENERIC"),
    # ---- the wide f16x3 weight gradient needs twelve 128-voxel tiles per strip: 384 tiles at 8 channel-block pairs
    ((1, 16, 48, 64, 128, 128, 3, 1, 1), 4, 4, IG_FWD, IG_DGRAD, ("WGRAD_MFMA", "WGRAD_LOWP_NARROW", "WGRAD_LOWP_NARROW", "WGRAD_LOWP_WIDE")),   # WIT y/dx/dw
    ((1, 16, 48, 64, 512, 32, 3, 1, 1), 4, 4, IG_FWD, IG_DGRAD, ("WGRAD_MFMA", "WGRAD_LOWP_NARROW", "WGRAD_LOWP_NARROW", "WGRAD_LOWP_SWAPPED")),   # WIT y/dx/dw
]
SHIFTED_STATS_CASE = (1, 32, 64, 64, 1, 64, 3, 1, 1)      # channel 0 gets mean 50, std 0.5: a plain fp32 sum of squares would fail (b)

# (N, D, H, W, Cin, Cout), ldx - Cin, ldy - Cout, forward, input gradient, weight gradient
DIRECT = lambda what: (f"CONVT_{what}_MFMA", f"CONVT_{what}_DIRECT", f"CONVT_{what}_DIRECT", f"CONVT_{what}_DIRECT")
CT_WGRAD = ("CONVT_WGRAD_MFMA", "CONVT_WGRAD_LOWP", "CONVT_WGRAD_LOWP", "CONVT_WGRAD_LOWP")
CONVT_CASES = [
    ((1, 8, 8, 8, 256, 64), 4, 4, DIRECT("FWD"), DIRECT("DGRAD"), CT_WGRAD),          # streaming form at K = 256
    ((1, 6, 6, 6, 64, 32), 4, 4, DIRECT("FWD"), DIRECT("DGRAD"), CT_WGRAD),           # partial tiles
    ((1, 4, 4, 4, 128, 128), 4, 4, DIRECT("FWD"), DIRECT("DGRAD"), CT_WGRAD),         # split-K input gradient
    ((1, 3, 5, 4, 6, 10), 1, 1, "CONVT_FWD_PLAIN", "CONVT_DGRAD_PLAIN", "CONVT_WGRAD_PLAIN"),
]


def case_id(c):
    return "x".join(map(str, c[0])) + f"-ld+{c[1]}+{c[2]}"


# ----------------------------------------------------------------------------- references (once per case, shared by every math)
class Ref:
    pass


def _witness(got32, want64):
    return float((got32.double() - want64).abs().max()) / max(1.0, float(want64.abs().max()))


@functools.lru_cache(maxsize=None)
def conv_reference(geom, ex, ey):
    N, D, H, W, Cin, Cout, k, s, p = geom
    r = Ref()
    r.ldx, r.ldy = Cin + ex, Cout + ey
    r.x = rnd(N, D, H, W, r.ldx, seed=1)                       # channel-last at its pitch; the columns beyond Cin are not the kernel's to read
    r.w = rnd(Cout, Cin, k, k, k, seed=2, scale=(2.0 / (Cin * k ** 3)) ** 0.5)
    r.b = rnd(Cout, seed=3, scale=0.1)
    if geom == SHIFTED_STATS_CASE:
        r.w[0] *= 0.5 / float((r.w[0] ** 2).sum().sqrt())
        r.b[0] = 50.0
    Do, Ho, Wo = [(e + 2 * p - k) // s + 1 for e in (D, H, W)]
    r.out_shape = (N, Do, Ho, Wo)
    r.g = rnd(N, Do, Ho, Wo, r.ldy, seed=4)
    ncdhw = lambda t, C: t[..., :C].permute(0, 4, 1, 2, 3)
    res = {}
    for dt in (torch.float64, torch.float32):
        xd, wd, bd = (t.to(dt).clone().requires_grad_(True) for t in (ncdhw(r.x, Cin), r.w, r.b))
        y0 = TF.conv3d(xd, wd, None, stride=s, padding=p)
        y = y0 + bd.view(1, -1, 1, 1, 1)
        y.backward(ncdhw(r.g, Cout).to(dt))
        res[dt] = tuple(t.detach() for t in (y.permute(0, 2, 3, 4, 1), y0.permute(0, 2, 3, 4, 1), xd.grad.permute(0, 2, 3, 4, 1), wd.grad, bd.grad))
    r.y, r.y0, r.dx, r.dw, r.db = [t.contiguous() for t in res[torch.float64]]
    r.wit = dict(zip(("y", "y0", "dx", "dw", "db"), (_witness(a, b) for a, b in zip(res[torch.float32], res[torch.float64]))))
    return r


@functools.lru_cache(maxsize=None)
def convt_reference(geom, ex, ey):
    N, D, H, W, Cin, Cout = geom
    r = Ref()
    r.ldx, r.ldy = Cin + ex, Cout + ey
    r.x = rnd(N, D, H, W, r.ldx, seed=1)
    r.w = rnd(Cin, Cout, 2, 2, 2, seed=2, scale=(2.0 / (Cin * 8)) ** 0.5)
    r.b = rnd(Cout, seed=3, scale=0.1)
    r.out_shape = (N, 2 * D, 2 * H, 2 * W)
    r.g = rnd(N, 2 * D, 2 * H, 2 * W, r.ldy, seed=4)
    ncdhw = lambda t, C: t[..., :C].permute(0, 4, 1, 2, 3)
    res = {}
    for dt in (torch.float64, torch.float32):
        xd, wd, bd = (t.to(dt).clone().requires_grad_(True) for t in (ncdhw(r.x, Cin), r.w, r.b))
        y0 = TF.conv_transpose3d(xd, wd, None, stride=2)
        y = y0 + bd.view(1, -1, 1, 1, 1)
        y.backward(ncdhw(r.g, Cout).to(dt))
        res[dt] = tuple(t.detach() for t in (y.permute(0, 2, 3, 4, 1), y0.permute(0, 2, 3, 4, 1), xd.grad.permute(0, 2, 3, 4, 1), wd.grad, bd.grad))
    r.y, r.y0, r.dx, r.dw, r.db = [t.contiguous() for t in res[torch.float64]]
    r.wit = dict(zip(("y", "y0", "dx", "dw", "db"), (_witness(a, b) for a, b in zip(res[torch.float32], res[torch.float64]))))
    return r


# ----------------------------------------------------------------------------- guarded buffers
class Rows:
    """rows x ld floats with GUARD_ROWS sentinel rows in front and behind; ``t`` is the payload, of which the kernel owns [:, :C]."""

    def __init__(self, rows, ld, C):
        self.buf = torch.full((rows + 2 * GUARD_ROWS, ld), SENTINEL, device="cuda")
        self.t = self.buf[GUARD_ROWS:GUARD_ROWS + rows]
        self.C = C
        self.ptr = self.t.data_ptr()

    def check(self, what):
        ok = (self.buf[:GUARD_ROWS] == SENTINEL).all() & (self.buf[-GUARD_ROWS:] == SENTINEL).all() & (self.t[:, self.C:] == SENTINEL).all()
        assert bool(ok), f"{what}: wrote outside its rows x channels"
        return self.t[:, :self.C].cpu().double()


class Flat:
    """n floats (a weight or bias gradient) between two sentinel runs, pre-filled with ``init`` (a tensor) or NaN."""

    def __init__(self, n, init=None):
        self.buf = torch.full((n + 2 * GUARD_ELEMS,), SENTINEL, device="cuda")
        self.t = self.buf[GUARD_ELEMS:GUARD_ELEMS + n]
        self.t.copy_(init.reshape(-1).cuda()) if init is not None else self.t.fill_(float("nan"))
        self.ptr = self.t.data_ptr()

    def check(self, what):
        assert bool((self.buf[:GUARD_ELEMS] == SENTINEL).all() & (self.buf[-GUARD_ELEMS:] == SENTINEL).all()), f"{what}: wrote outside its buffer"
        return self.t.cpu().double()


class Workspace:
    """Exactly the queried size, cut from a larger buffer; the BAND bytes behind it are the kernels' to leave alone."""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = torch.empty(self.n + BAND, dtype=torch.uint8, device="cuda")
        self.buf[self.n:] = 0xA5
        self.ptr = self.buf.data_ptr()

    def check(self, what):
        assert bool((self.buf[self.n:] == 0xA5).all()), f"{what}: wrote past the {self.n} bytes the workspace query asked for"


def stream():
    return torch.cuda.current_stream().cuda_stream


class Grader:
    """Collects (pass, math) -> error relative to the scale, asserts bound (a), prints kernel error | witness | bound."""

    def __init__(self, ref, name):
        self.ref, self.name, self.err = ref, name, {}

    def scale(self, what):
        return max(1.0, float(getattr(self.ref, what).abs().max()))

    def bound(self, what):
        return max(BOUND, WITNESS_FACTOR * self.ref.wit[what])

    def grade(self, what, got, key, tag="", want=None, extra_abs=0.0):
        want = getattr(self.ref, what) if want is None else want
        e = got.reshape(want.shape) - want
        assert bool(torch.isfinite(e).all()), f"{self.name} {what}{tag} {key}: not finite"
        rel = float(e.abs().max()) / self.scale(what)
        bound = self.bound(what) + extra_abs / self.scale(what)
        print(f"{self.name:44s} {key[0]:>7s}/{key[1]:<2d} {what + tag:10s} kernel {rel:9.2e}  witness {self.ref.wit[what]:9.2e}  bound {bound:9.2e}")
        assert rel <= bound, f"{self.name} {what}{tag} under {key}: {rel:.3e} of the scale, bound {bound:.3e} (witness {self.ref.wit[what]:.3e})"
        return e

    def spread(self, what, errs, paths):
        """Where a math runs another kernel than the fp32 math: the error's rms within 1.25x of the fp32-math run's (+ 1e-9 of the scale,
        the slack of test_bf16x6_16x16x32_kernel_...), |mean error| <= 2e-7 of the scale -- a lost low-order product shows here first."""
        sc = self.scale(what)
        rms = lambda e: float(e.pow(2).mean().sqrt())
        base = rms(errs[MATHS[0]])
        for key in MATHS[1:]:
            if paths[key] == paths[MATHS[0]]:
                continue
            r, m = rms(errs[key]), abs(float(errs[key].mean()))
            print(f"{self.name:44s} {key[0]:>7s}/{key[1]:<2d} {what:10s} rms {r / sc:9.2e}  fp32-math rms {base / sc:9.2e}  |mean| {m / sc:9.2e}")
            assert r <= 1.25 * base + 1e-9 * sc, f"{self.name} {what} {key} ({paths[key]}): rms {r:.3e} against {base:.3e} of the fp32 math ({paths[MATHS[0]]})"
            assert m <= 2e-7 * sc, f"{self.name} {what} {key} ({paths[key]}): mean error {m:.3e}, scale {sc:.3e}"


def expect_path(L, want, what, key):
    got = last_path(L)
    assert got == want, f"{what} under {key[0]}/{key[1]} ran {got}, the case was built for {want}"


def amax_slot(value):
    return torch.tensor([float(value)], dtype=torch.float32, device="cuda")


@gpu
@pytest.mark.parametrize("case", CONV_CASES, ids=case_id)
def test_conv3d_branch_against_fp64_in_every_math(seg, case):
    """(a) values with and without bias, (b) epilogue statistics against fp64 sums of the kernel's own y, (d) f16x3 operand maxima handed
    over as the true maxima, as 8x bounds and not at all, (e) accumulate = 0 over NaN and accumulate = 1 over seeded gradients,
    (f) bit-identical weight gradients and statistics on a second run -- for the branch ``mi355seg_last_conv_path`` confirms."""
    geom, ex, ey, pf, pd, pw = case
    N, D, H, W, Cin, Cout, k, s, p = geom
    L = seg.lib()
    ref = conv_reference(geom, ex, ey)
    G = Grader(ref, case_id(case))
    ldx, ldy = ref.ldx, ref.ldy
    rows_in, rows_out = N * D * H * W, ref.y.numel() // Cout
    x, w, b, g = ref.x.cuda(), ref.w.cuda(), ref.b.cuda(), ref.g.cuda()
    ws = Workspace(L.query("mi355seg_conv3d_ws_bytes", *geom))
    g0w, g0b = rnd(*ref.dw.shape, seed=5, scale=float(ref.dw.pow(2).mean().sqrt())), rnd(Cout, seed=6, scale=float(ref.db.pow(2).mean().sqrt()))
    acc_w, acc_b = g0w.double() + ref.dw, g0b.double() + ref.db
    st = stream()

    def fwd(key, bias, stats, xa=None, wa=None):
        y = Rows(rows_out, ldy, Cout)
        ss = torch.zeros(2, Cout, dtype=torch.float64, device="cuda") if stats else None
        L.call("mi355seg_conv3d_fwd_ax_f32", x.data_ptr(), ldx, w.data_ptr(), b.data_ptr() if bias else None, y.ptr, ldy, *geom,
               ss[0].data_ptr() if stats else None, ss[1].data_ptr() if stats else None, xa, wa, ws.ptr, ws.n, st)
        want = pf_[key] if stats else pf_[key].replace("_TILED_STATS", "_TILED")           # the in-kernel statistics form only runs when asked for them
        expect_path(L, want, "forward", key)
        ws.check("forward")
        return y.check("forward"), ss

    def dgrad(key, ga=None, wa=None):
        dx = Rows(rows_in, ldx, Cin)
        L.call("mi355seg_conv3d_dgrad_ax_f32", g.data_ptr(), ldy, w.data_ptr(), dx.ptr, ldx, *geom, ga, wa, ws.ptr, ws.n, st)
        expect_path(L, pd_[key], "input gradient", key)
        ws.check("input gradient")
        return dx.check("input gradient")

    def wgrad(key, accumulate, ga=None, xa=None):
        dw, db = Flat(ref.dw.numel(), g0w if accumulate else None), Flat(Cout, g0b if accumulate else None)
        L.call("mi355seg_conv3d_wgrad_ax_f32", g.data_ptr(), ldy, x.data_ptr(), ldx, dw.ptr, db.ptr, *geom, accumulate, ga, xa, ws.ptr, ws.n, st)
        expect_path(L, pw_[key], "weight gradient", key)
        ws.check("weight gradient")
        return dw.check("weight gradient"), db.check("bias gradient")

    pf_, pd_, pw_ = (dict(zip(MATHS, per_math(spec))) for spec in (pf, pd, pw))
    errs = {"y": {}, "dx": {}, "dw": {}}
    try:
        for key in MATHS:
            seg.set_conv_math(key[0])
            seg.set_x3_shape(key[1])
            y, ss = fwd(key, True, True)
            errs["y"][key] = G.grade("y", y, key)
            yd = y.reshape(-1, Cout)                                                            # (b): the 1e-6 bar of test_conv3d_fused_batch_statistics
            e1 = float(((ss[0].cpu() - yd.sum(0)).abs() / yd.abs().sum(0)).max())
            e2 = float(((ss[1].cpu() - (yd * yd).sum(0)).abs() / (yd * yd).sum(0)).max())
            print(f"{G.name:44s} {key[0]:>7s}/{key[1]:<2d} statistics sum {e1:9.2e}  sum of squares {e2:9.2e}  bound  1.00e-06")
            assert e1 < 1e-6 and e2 < 1e-6, f"{G.name} epilogue statistics under {key} ({pf_[key]}): {e1:.3e}, {e2:.3e}"
            y2, ss2 = fwd(key, True, True)
            assert torch.equal(ss, ss2) and torch.equal(y, y2), f"{G.name} {key}: the forward and its statistics are not reproducible"      # (f)
            G.grade("y0", fwd(key, False, False)[0], key)
            errs["dx"][key] = G.grade("dx", dgrad(key), key)
            dw, db = wgrad(key, 0)                                                              # (e): over NaN
            errs["dw"][key] = G.grade("dw", dw, key)
            G.grade("db", db, key)
            dw2, db2 = wgrad(key, 0)
            assert torch.equal(dw, dw2) and torch.equal(db, db2), f"{G.name} {key} ({pw_[key]}): the weight gradient is not reproducible"  # (f)
            dwa, dba = wgrad(key, 1)                                                            # (e): one fp32 rounding of the sum on top of (a)
            G.grade("dw", dwa, key, "+G0", want=acc_w, extra_abs=EPS32 * float(acc_w.abs().max()))
            G.grade("db", dba, key, "+G0", want=acc_b, extra_abs=EPS32 * float(acc_b.abs().max()))
            if L.query("mi355seg_conv_math_takes_amax"):                                        # (d); NULL maxima are every call above
                for f in (1.0, 8.0):
                    xa, wa, ga = (amax_slot(f * float(t.abs().max())) for t in (ref.x[..., :Cin], ref.w, ref.g[..., :Cout]))
                    G.grade("y", fwd(key, True, True, xa.data_ptr(), wa.data_ptr())[0], key, f" ax{f:g}")
                    G.grade("dx", dgrad(key, ga.data_ptr(), wa.data_ptr()), key, f" ax{f:g}")
                    G.grade("dw", wgrad(key, 0, ga.data_ptr(), xa.data_ptr())[0], key, f" ax{f:g}")
    finally:
        seg.set_conv_math(DEFAULT_MATH)
        seg.set_x3_shape(16)
    G.spread("y", errs["y"], pf_)
    G.spread("dx", errs["dx"], pd_)
    G.spread("dw", errs["dw"], pw_)


@gpu
@pytest.mark.parametrize("case", CONVT_CASES, ids=case_id)
def test_conv_transpose3d_k2s2_branch_against_fp64_in_every_math(seg, case):
    """The three ConvTranspose3d k2 s2 entry points by the same rules; the weight gradient has no accumulate flag and must overwrite NaN."""
    geom, ex, ey, pf, pd, pw = case
    N, D, H, W, Cin, Cout = geom
    L = seg.lib()
    ref = convt_reference(geom, ex, ey)
    G = Grader(ref, "convt-" + case_id(case))
    ldx, ldy = ref.ldx, ref.ldy
    rows_in, rows_out = N * D * H * W, 8 * N * D * H * W
    x, w, b, g = ref.x.cuda(), ref.w.cuda(), ref.b.cuda(), ref.g.cuda()
    ws = Workspace(L.query("mi355seg_convt3d_k2s2_ws_bytes", *geom))
    st = stream()
    pf_, pd_, pw_ = (dict(zip(MATHS, per_math(spec))) for spec in (pf, pd, pw))
    errs = {"y": {}, "dx": {}, "dw": {}}

    def fwd(key, bias):
        y = Rows(rows_out, ldy, Cout)
        L.call("mi355seg_convt3d_k2s2_fwd_f32", x.data_ptr(), ldx, w.data_ptr(), b.data_ptr() if bias else None, y.ptr, ldy, *geom, ws.ptr, ws.n, st)
        expect_path(L, pf_[key], "forward", key)
        ws.check("forward")
        return y.check("forward")

    def wgrad(key):
        dw, db = Flat(ref.dw.numel()), Flat(Cout)
        L.call("mi355seg_convt3d_k2s2_wgrad_f32", g.data_ptr(), ldy, x.data_ptr(), ldx, dw.ptr, db.ptr, *geom, ws.ptr, ws.n, st)
        expect_path(L, pw_[key], "weight gradient", key)
        ws.check("weight gradient")
        return dw.check("weight gradient"), db.check("bias gradient")

    try:
        for key in MATHS:
            seg.set_conv_math(key[0])
            seg.set_x3_shape(key[1])
            errs["y"][key] = G.grade("y", fwd(key, True), key)
            G.grade("y0", fwd(key, False), key)
            dx = Rows(rows_in, ldx, Cin)
            L.call("mi355seg_convt3d_k2s2_dgrad_f32", g.data_ptr(), ldy, w.data_ptr(), dx.ptr, ldx, *geom, ws.ptr, ws.n, st)
            expect_path(L, pd_[key], "input gradient", key)
            ws.check("input gradient")
            errs["dx"][key] = G.grade("dx", dx.check("input gradient"), key)
            dw, db = wgrad(key)
            errs["dw"][key] = G.grade("dw", dw, key)
            G.grade("db", db, key)
            dw2, db2 = wgrad(key)
            assert torch.equal(dw, dw2) and torch.equal(db, db2), f"{G.name} {key} ({pw_[key]}): the weight gradient is not reproducible"
    finally:
        seg.set_conv_math(DEFAULT_MATH)
        seg.set_x3_shape(16)
    G.spread("y", errs["y"], pf_)
    G.spread("dx", errs["dx"], pd_)
    G.spread("dw", errs["dw"], pw_)


SLICE_CASE = ((1, 5, 7, 9, 32, 32, 3, 1, 1), 4, 4)        # the igemm case of CONV_CASES, its operand read at channel offset 1 of the pitch-36 rows


@gpu
@pytest.mark.parametrize("which, want", [("fwd", "FWD_GENERIC"), ("dgrad", "DGRAD_GENERIC")])
def test_conv3d_misaligned_channel_slice_falls_through(seg, which, want):
    """An fp32 channel slice that starts at channel 1: x (forward) / dy (input gradient) sits 4 bytes off a 16-byte boundary at a pitch
    that is a multiple of 4.  The igemm rungs ask for the 16-byte alignment their launcher demands, so the call goes down the ladder --
    gather, headk, stems and heads do not fit a 32 -> 32 k3 layer -- to the generic kernel instead of being refused, in every math, within
    bound (a), inside its rows x channels and inside the queried workspace."""
    geom, ex, ey = SLICE_CASE
    N, D, H, W, Cin, Cout, k, s, p = geom
    L = seg.lib()
    ref = conv_reference(geom, ex, ey)
    G = Grader(ref, f"slice-{which}-" + case_id(SLICE_CASE))
    ldx, ldy = ref.ldx, ref.ldy
    rows_in, rows_out = N * D * H * W, ref.y.numel() // Cout
    src, C, ld = (ref.x, Cin, ldx) if which == "fwd" else (ref.g, Cout, ldy)
    buf = torch.full((src.numel() // ld + 1, ld), SENTINEL, device="cuda")
    buf[:-1, 1:1 + C] = src.reshape(-1, ld)[:, :C].cuda()
    ptr = buf.data_ptr() + 4
    assert ptr % 16 == 4 and ld % 4 == 0
    w, b = ref.w.cuda(), ref.b.cuda()
    ws = Workspace(L.query("mi355seg_conv3d_ws_bytes", *geom))
    try:
        for key in MATHS:
            seg.set_conv_math(key[0])
            seg.set_x3_shape(key[1])
            if which == "fwd":
                out = Rows(rows_out, ldy, Cout)
                L.call("mi355seg_conv3d_fwd_ax_f32", ptr, ldx, w.data_ptr(), b.data_ptr(), out.ptr, ldy, *geom, None, None, None, None, ws.ptr, ws.n, stream())
            else:
                out = Rows(rows_in, ldx, Cin)
                L.call("mi355seg_conv3d_dgrad_ax_f32", ptr, ldy, w.data_ptr(), out.ptr, ldx, *geom, None, None, ws.ptr, ws.n, stream())
            expect_path(L, want, which, key)
            ws.check(which)
            G.grade("y" if which == "fwd" else "dx", out.check(which), key)
    finally:
        seg.set_conv_math(DEFAULT_MATH)
        seg.set_x3_shape(16)


def _amax_rules(run, what):
    """(c): ``run(slot)`` writes y and max-combines max |y| into the device scalar; returns y.  The scalar equals max |y| of the tensor
    the call wrote bit for bit; a larger value already in the slot stays, a smaller one is raised."""
    slot = amax_slot(0.0)
    y = run(slot)
    true = float(y.abs().max().float())
    assert true > 0 and float(slot) == true, f"{what}: y_amax {float(slot)!r}, max |y| {true!r}"
    slot = amax_slot(2.0 * true)
    run(slot)
    assert float(slot) == 2.0 * true, f"{what}: a larger maximum in the slot was replaced by {float(slot)!r}"
    slot = amax_slot(0.5 * true)
    run(slot)
    assert float(slot) == true, f"{what}: a smaller maximum in the slot became {float(slot)!r}, max |y| {true!r}"


YAMAX_CASES = [
    ((1, 8, 8, 16, 32, 32, 3, 1, 1), 4, 4, IG_FWD),                                   # conv_x3s.hip: from the kernel's epilogue
    ((1, 32, 48, 48, 1, 64, 3, 1, 1), 1, 4, "FWD_STEM_TILED_STATS"),                   # the tiled stem's own epilogue
    ((1, 32, 64, 64, 1, 64, 3, 1, 1), 1, 4, "FWD_STEM_TILED_STATS"),                   # ... with blocks that walk more than one tile
    ((1, 7, 9, 11, 3, 5, 3, 1, 1), 1, 1, "FWD_GENERIC"),                               # a branch without one: a pass over y
]


@gpu
@pytest.mark.parametrize("case", YAMAX_CASES, ids=case_id)
def test_conv3d_fwd_yamax_is_the_maximum_of_what_it_wrote(seg, case):
    geom, ex, ey, pf = case
    N, D, H, W, Cin, Cout, k, s, p = geom
    L = seg.lib()
    ref = conv_reference(geom, ex, ey)
    x, w, b = ref.x.cuda(), ref.w.cuda(), ref.b.cuda()
    ws = Workspace(L.query("mi355seg_conv3d_ws_bytes", *geom))
    G = Grader(ref, "yamax-" + case_id(case))
    try:
        for key, want in zip(MATHS, per_math(pf)):
            seg.set_conv_math(key[0])
            seg.set_x3_shape(key[1])

            def run(slot):
                y = Rows(ref.y.numel() // Cout, ref.ldy, Cout)
                ss = torch.zeros(2, Cout, dtype=torch.float64, device="cuda")
                L.call("mi355seg_conv3d_fwd_yamax_ax_f32", x.data_ptr(), ref.ldx, w.data_ptr(), b.data_ptr(), y.ptr, ref.ldy, *geom,
                       ss[0].data_ptr(), ss[1].data_ptr(), None, None, slot.data_ptr(), ws.ptr, ws.n, stream())
                expect_path(L, want, "forward", key)
                ws.check("forward")
                got = y.check("forward")
                G.grade("y", got, key)
                return got

            _amax_rules(run, f"{G.name} {key} ({want})")
    finally:
        seg.set_conv_math(DEFAULT_MATH)
        seg.set_x3_shape(16)


@gpu
@pytest.mark.parametrize("case", [CONVT_CASES[0], CONVT_CASES[3]], ids=case_id)
def test_conv_transpose3d_fwd_ax_yamax_is_the_maximum_of_what_it_wrote(seg, case):
    geom, ex, ey, pf, _, _ = case
    Cout = geom[5]
    L = seg.lib()
    ref = convt_reference(geom, ex, ey)
    x, w, b = ref.x.cuda(), ref.w.cuda(), ref.b.cuda()
    ws = Workspace(L.query("mi355seg_convt3d_k2s2_ws_bytes", *geom))
    G = Grader(ref, "yamax-convt-" + case_id(case))
    try:
        for key, want in zip(MATHS, per_math(pf)):
            seg.set_conv_math(key[0])
            seg.set_x3_shape(key[1])

            def run(slot):
                y = Rows(ref.y.numel() // Cout, ref.ldy, Cout)
                L.call("mi355seg_convt3d_k2s2_fwd_ax_f32", x.data_ptr(), ref.ldx, w.data_ptr(), b.data_ptr(), y.ptr, ref.ldy, *geom,
                       slot.data_ptr(), ws.ptr, ws.n, stream())
                expect_path(L, want, "forward", key)
                ws.check("forward")
                got = y.check("forward")
                G.grade("y", got, key)
                return got

            _amax_rules(run, f"{G.name} {key} ({want})")
    finally:
        seg.set_conv_math(DEFAULT_MATH)
        seg.set_x3_shape(16)


@gpu
def test_conv3d_fwd_fused_records_its_branch_and_matches_fp64(seg):
    """mi355seg_conv3d_fwd_fused_f32 (inference: eval-mode BatchNorm folded in, relu in the epilogue) chooses between the same igemm
    kernels as the plain forward: the read-back names them, the values are held against fp64 relu(conv3d(x, w) * oscale + oshift)."""
    geom = (1, 8, 8, 16, 32, 32, 3, 1, 1)
    N, D, H, W, Cin, Cout, k, s, p = geom
    L, F = seg.lib(), seg.functional
    ldx, ldy = Cin + 4, Cout + 4
    x, w = rnd(N, D, H, W, ldx, seed=1), rnd(Cout, Cin, 3, 3, 3, seed=2, scale=(2.0 / (27 * Cin)) ** 0.5)
    osc, osh = 1.0 + 0.2 * rnd(Cout, seed=3), 0.3 * rnd(Cout, seed=4)
    ref = Ref()
    res = {}
    for dt in (torch.float64, torch.float32):
        y = TF.conv3d(x[..., :Cin].permute(0, 4, 1, 2, 3).to(dt), w.to(dt), None, padding=1)
        res[dt] = torch.relu(y * osc.to(dt).view(1, -1, 1, 1, 1) + osh.to(dt).view(1, -1, 1, 1, 1)).permute(0, 2, 3, 4, 1)
    ref.y = res[torch.float64].contiguous()
    ref.wit = {"y": _witness(res[torch.float32], res[torch.float64])}
    G = Grader(ref, "fused-" + "x".join(map(str, geom)))
    xg, wg, oscg, oshg = (t.cuda() for t in (x, w, osc, osh))
    ws = Workspace(L.query("mi355seg_conv3d_ws_bytes", *geom))
    try:
        for key, want in zip(MATHS, IG_FWD):
            seg.set_conv_math(key[0])
            seg.set_x3_shape(key[1])
            assert L.query("mi355seg_conv3d_fused_supported_f32", *geom, ldx, ldy)
            y = Rows(N * D * H * W, ldy, Cout)
            L.call("mi355seg_conv3d_fwd_fused_f32", xg.data_ptr(), ldx, wg.data_ptr(), oscg.data_ptr(), oshg.data_ptr(), F.ACT_RELU, 0.0, y.ptr, ldy, *geom,
                   ws.ptr, ws.n, stream())
            expect_path(L, want, "fused forward", key)
            ws.check("fused forward")
            G.grade("y", y.check("fused forward"), key)
    finally:
        seg.set_conv_math(DEFAULT_MATH)
        seg.set_x3_shape(16)


@gpu
def test_conv3d_pro_entries_against_fp64(seg):
    """mi355seg_conv3d_fwd_pro_ax_f32 / mi355seg_conv3d_wgrad_pro_ax_f32 (f16x3: the norm + relu of the layer in front as a prologue of
    the tile staging) against fp64 conv3d(relu(al x + be), w) and its weight gradient: accumulate = 0 over NaN, = 1 over seeded values."""
    geom = (1, 8, 8, 16, 32, 32, 3, 1, 1)
    N, D, H, W, Cin, Cout, k, s, p = geom
    L, F = seg.lib(), seg.functional
    assert seg.get_conv_math() == "f16x3" and L.query("mi355seg_conv3d_pro_supported_f32", *geom, F.ACT_RELU)
    ex = ey = 4
    ldx, ldy = Cin + ex, Cout + ey
    x, w, b, g = rnd(N, D, H, W, ldx, seed=1), rnd(Cout, Cin, 3, 3, 3, seed=2, scale=(2.0 / (27 * Cin)) ** 0.5), rnd(Cout, seed=3, scale=0.1), rnd(N, D, H, W, ldy, seed=4)
    al, be = 1.0 + 0.2 * rnd(Cin, seed=7), 0.3 * rnd(Cin, seed=8)
    ref = Ref()
    res = {}
    for dt in (torch.float64, torch.float32):
        a = torch.relu(x[..., :Cin].to(dt) * al.to(dt) + be.to(dt)).permute(0, 4, 1, 2, 3)
        wd, bd = w.to(dt).clone().requires_grad_(True), b.to(dt).clone().requires_grad_(True)
        y = TF.conv3d(a, wd, bd, padding=1)
        y.backward(g[..., :Cout].permute(0, 4, 1, 2, 3).to(dt))
        res[dt] = (y.detach().permute(0, 2, 3, 4, 1), wd.grad, bd.grad)
        amax = float(a.abs().max())
    ref.y, ref.dw, ref.db = res[torch.float64]
    ref.wit = dict(zip(("y", "dw", "db"), (_witness(a_, b_) for a_, b_ in zip(res[torch.float32], res[torch.float64]))))
    G = Grader(ref, "pro-" + "x".join(map(str, geom)))
    key = ("f16x3", 16)
    xg, wg, bg, gg, alg, beg = (t.cuda() for t in (x, w, b, g, al, be))
    xa = amax_slot(amax * (1.0 + 1e-6))                            # bounds the prologue's OUTPUT (the kernel forms it with its own fp32 rounding)
    ws = Workspace(L.query("mi355seg_conv3d_ws_bytes", *geom))
    y = Rows(N * D * H * W, ldy, Cout)
    L.call("mi355seg_conv3d_fwd_pro_ax_f32", xg.data_ptr(), ldx, alg.data_ptr(), beg.data_ptr(), F.ACT_RELU, 0.0, wg.data_ptr(), bg.data_ptr(), y.ptr, ldy, *geom,
           None, None, xa.data_ptr(), None, ws.ptr, ws.n, stream())
    expect_path(L, "FWD_PRO_X3S", "forward", key)
    ws.check("forward")
    G.grade("y", y.check("forward"), key)
    g0w, g0b = rnd(*ref.dw.shape, seed=5, scale=float(ref.dw.pow(2).mean().sqrt())), rnd(Cout, seed=6, scale=float(ref.db.pow(2).mean().sqrt()))
    for accumulate in (0, 0, 1):
        dw, db = Flat(ref.dw.numel(), g0w if accumulate else None), Flat(Cout, g0b if accumulate else None)
        L.call("mi355seg_conv3d_wgrad_pro_ax_f32", gg.data_ptr(), ldy, xg.data_ptr(), ldx, alg.data_ptr(), beg.data_ptr(), F.ACT_RELU, 0.0, dw.ptr, db.ptr, *geom,
               accumulate, None, xa.data_ptr(), ws.ptr, ws.n, stream())
        expect_path(L, "WGRAD_LOWP_NARROW", "weight gradient", key)
        ws.check("weight gradient")
        got_w, got_b = dw.check("weight gradient"), db.check("bias gradient")
        if accumulate:
            want_w, want_b = g0w.double() + ref.dw, g0b.double() + ref.db
            G.grade("dw", got_w, key, "+G0", want=want_w, extra_abs=EPS32 * float(want_w.abs().max()))
            G.grade("db", got_b, key, "+G0", want=want_b, extra_abs=EPS32 * float(want_b.abs().max()))
        else:
            G.grade("dw", got_w, key)
            G.grade("db", got_b, key)
            if "first" in res:
                assert torch.equal(res["first"][0], got_w) and torch.equal(res["first"][1], got_b), "wgrad_pro is not reproducible"
            res["first"] = (got_w, got_b)


# (N, D, H, W, Cin, Cout, Cskip, scale of the up-convolution's weights: the first buffer's maximum sits in the skip half, the second's in the other)
@gpu
@pytest.mark.parametrize("case", [(1, 4, 4, 8, 64, 32, 32, 1.0), (1, 3, 5, 4, 6, 10, 8, 8.0)], ids=lambda c: "x".join(map(str, c)))
def test_conv_transpose3d_k2s2_cat_against_fp64(seg, case):
    """(g) The up-convolution written into the left channels of the concat buffer whose right channels conv_bn_act(..., left_pad=Cout)
    filled (unet3d.py:77-81): forward and every gradient against fp64 cat(conv_transpose3d(x), skip) in all maths; the skip half is
    bit-identical before and after; under f16x3 the buffer carries max(max |up|, max |skip|) as its operand maximum."""
    N, D, H, W, Cin, Cout, Cs, up = case
    F = seg.functional
    from mi355seg.layers import BatchNorm3d, Conv3d
    x, w, b = rnd(N, D, H, W, Cin, seed=1), rnd(Cin, Cout, 2, 2, 2, seed=2, scale=up * (2.0 / (Cin * 8)) ** 0.5), rnd(Cout, seed=3, scale=0.1)
    xs = rnd(N, 2 * D, 2 * H, 2 * W, Cs, seed=4)
    cw, cb = rnd(Cs, Cs, 3, 3, 3, seed=5, scale=(2.0 / (27 * Cs)) ** 0.5), rnd(Cs, seed=6, scale=0.1)
    gam, bet = 1.0 + 0.1 * rnd(Cs, seed=7), 0.1 * rnd(Cs, seed=8)
    g = rnd(N, 2 * D, 2 * H, 2 * W, Cout + Cs, seed=9)
    nc = lambda t: t.permute(0, 4, 1, 2, 3)
    cl = lambda t: t.permute(0, 2, 3, 4, 1)
    res = {}
    for dt in (torch.float64, torch.float32):
        leaves = [t.to(dt).clone().requires_grad_(True) for t in (nc(x), w, b, nc(xs), cw, cb, gam, bet)]
        xd, wd, bd, xsd, cwd, cbd, gd, btd = leaves
        skip = torch.relu(TF.batch_norm(TF.conv3d(xsd, cwd, cbd, padding=1), None, None, gd, btd, training=True, eps=1e-5))
        cat = torch.cat((TF.conv_transpose3d(xd, wd, bd, stride=2), skip), dim=1)
        cat.backward(nc(g).to(dt))
        res[dt] = [cl(cat.detach()), cl(xd.grad), wd.grad, bd.grad, cl(xsd.grad), cwd.grad]
    names = ("cat", "dx", "dw", "db", "dxs", "dcw")
    ref = Ref()
    for n_, t in zip(names, res[torch.float64]):
        setattr(ref, n_, t.contiguous())
    ref.wit = dict(zip(names, (_witness(a_, b_) for a_, b_ in zip(res[torch.float32], res[torch.float64]))))
    G = Grader(ref, "cat-" + "x".join(map(str, case)))
    try:
        for key in MATHS:
            seg.set_conv_math(key[0])
            seg.set_x3_shape(key[1])
            conv, bn = Conv3d(Cs, Cs, 3, padding=1).cuda(), BatchNorm3d(Cs).cuda().train()
            with torch.no_grad():
                conv.weight.copy_(cw), conv.bias.copy_(cb), bn.weight.copy_(gam), bn.bias.copy_(bet)
            xg, wg, bg, xsg = (t.cuda().requires_grad_(True) for t in (x, w, b, xs))
            skip = F.conv_bn_act(xsg, conv, bn, F.ACT_RELU, left_pad=Cout)
            before = skip.detach().clone()
            cat = F.conv_transpose3d_k2s2_cat(xg, wg, bg, skip)
            assert tuple(cat.shape) == (N, 2 * D, 2 * H, 2 * W, Cout + Cs) and cat.data_ptr() == skip._base.data_ptr()
            assert torch.equal(cat.detach()[..., Cout:], before), f"{G.name} {key}: the skip half of the concat buffer changed"
            if key[0] == "f16x3":
                carried = F._get_amax(cat)
                assert carried is not None, "the concat buffer carries no operand maximum under f16x3"
                m_up, m_skip = float(cat.detach()[..., :Cout].abs().max()), float(before.abs().max())
                assert (m_up > m_skip) == (up > 1.0), "the case no longer puts the maximum in the half it was built for"
                assert float(carried) == max(m_up, m_skip), f"{G.name}: carried {float(carried)!r}, halves {m_up!r} / {m_skip!r}"
            cat.backward(g.cuda())
            G.grade("cat", cat.detach().cpu().double(), key)
            G.grade("dx", xg.grad.cpu().double(), key)
            G.grade("dw", wg.grad.cpu().double(), key)
            G.grade("db", bg.grad.cpu().double(), key)
            G.grade("dxs", xsg.grad.cpu().double(), key)
            G.grade("dcw", conv.weight.grad.cpu().double(), key)
    finally:
        seg.set_conv_math(DEFAULT_MATH)
        seg.set_x3_shape(16)


def test_every_path_code_is_asserted_or_listed_unreachable():
    """Every MI355SEG_PATH_* code of the header is the expectation of at least one case above in every math that can reach it."""
    seen = {m: set() for m in MATHS}
    for c in CONV_CASES + CONVT_CASES:
        for spec in c[3:6]:
            for m, name in zip(MATHS, per_math(spec)):
                seen[m].add(name)
                seen[m].add(name.replace("_TILED_STATS", "_TILED"))
    seen[("f16x3", 16)].add("FWD_PRO_X3S")                         # test_conv3d_pro_entries_against_fp64
    split_only = {"FWD_MFMA_X3S", "FWD_MFMA_X3", "DGRAD_MFMA_X3S", "DGRAD_MFMA_X3", "WGRAD_LOWP_NARROW", "WGRAD_PW_LOWP", "CONVT_FWD_DIRECT",
                  "CONVT_DGRAD_DIRECT", "CONVT_WGRAD_LOWP"}
    f16_only = {"WGRAD_LOWP_WIDE", "WGRAD_LOWP_SWAPPED", "FWD_PRO_X3S"}
    shadowed_in_split = {"WGRAD_MFMA", "CONVT_FWD_MFMA", "CONVT_DGRAD_MFMA", "CONVT_WGRAD_MFMA"}       # see the module docstring
    unreachable = {
        ("fp32", 16): split_only | f16_only,
        ("bf16x6", 16): f16_only | shadowed_in_split,
        ("bf16x6", 32): f16_only | shadowed_in_split | {"FWD_MFMA_X3S", "DGRAD_MFMA_X3S"},
        ("f16x3", 16): shadowed_in_split,
    }
    # (the bf16-storage block of the header, MI355SEG_PATH_B16_*, is no fp32 math's to reach: tests/test_gpu_bf16_paths.py accounts for it)
    names = {n for n in path_names().values() if not n.startswith("B16_")} - {"NONE"}
    for m in MATHS:
        assert not (seen[m] & unreachable[m]), (m, seen[m] & unreachable[m])
        missing = names - seen[m] - unreachable[m]
        assert not missing, f"no case asserts {sorted(missing)} under {m}"
