"""torch.autograd wrappers over the C-ABI (libmi355seg.so).

PyTorch is plumbing here: device memory (caching allocator), the current HIP stream and
the autograd graph.  Every numeric kernel is a hand-written gfx950 kernel behind
include/mi355seg.h; nothing in this file computes with torch ops on the hot path.

Activations inside the package are channel-last: a 5-D fp32 tensor of logical shape
[N, D, H, W, C] whose last stride is 1 and whose voxel pitch (stride of W) may exceed C
(a channel slice of a wider concat buffer).
"""
import collections
import ctypes
import os
import threading
import weakref

import numpy as np
import torch
from torch.autograd import Function

from ._lib import lib, Mi355SegError

ACT_NONE, ACT_RELU, ACT_ELU, ACT_LRELU, ACT_SIGMOID = 0, 1, 2, 3, 4

_WS = {}

# ---- activation storage type.  fp32 by default; inside ``autocast(torch.bfloat16)`` the models' entry layout conversion
# (to_channels_last) produces bf16 activations and every op below follows its input's dtype: what
# ``Accelerator(mixed_precision="bf16")`` / torch.autocast does for the reference (parameters, their gradients, norm
# statistics and the loss stay fp32; conv products are bf16 MFMAs with fp32 accumulation).
class _AutocastState(threading.local):
    """Per-thread stack (a worker thread's forward must not inherit or leak another thread's bf16 mode)."""

    def __init__(self):
        self.stack = [torch.float32]


_AUTOCAST = _AutocastState()
_SFX = {torch.float32: "f32", torch.bfloat16: "bf16"}


class autocast:
    """``with mi355seg.functional.autocast(torch.bfloat16): pred = model(x)`` -- activations in bf16 (NDHWC in HBM)."""

    def __init__(self, dtype=torch.bfloat16, enabled=True):
        if dtype not in _SFX:
            raise Mi355SegError(f"autocast: dtype must be torch.float32 or torch.bfloat16, got {dtype}")
        self.dtype = dtype if enabled else torch.float32

    def __enter__(self):
        _AUTOCAST.stack.append(self.dtype)
        return self

    def __exit__(self, *exc):
        _AUTOCAST.stack.pop()
        return False


class _CounterBatch(threading.local):
    active = False
    seen = None


_COUNTERS = _CounterBatch()


class counters_batched:
    """While active, the fused BatchNorm entry points leave ``num_batches_tracked`` alone: engine.train_step has advanced the
    counters of ``modules`` (every training-mode BatchNorm of the model) with ONE multi-tensor launch (18-24 one-element torch
    kernels per step otherwise).  Calls are tallied, so a module used twice in one forward, or not at all, still ends with exactly
    the count nn.BatchNorm3d would hold."""

    def __init__(self, modules=()):
        self.modules = list(modules)

    def __enter__(self):
        self.prev = (_COUNTERS.active, _COUNTERS.seen)
        _COUNTERS.active, _COUNTERS.seen = True, {}

    def __exit__(self, *exc):
        seen = _COUNTERS.seen
        _COUNTERS.active, _COUNTERS.seen = self.prev
        for m in self.modules:
            k = seen.pop(id(m), (m, 0))[1]
            if k != 1:
                m.num_batches_tracked.add_(k - 1)
        for m, k in seen.values():                      # a BatchNorm outside the advanced set
            m.num_batches_tracked.add_(k)


_DEFERRED_WAITS = []


def defer_wait(work):
    """A collective launched ahead of the forward (distributed.broadcast_buffers(async_op=True)): waited for by the first norm layer."""
    _DEFERRED_WAITS.append(work)


def flush_deferred_waits():
    while _DEFERRED_WAITS:
        _DEFERRED_WAITS.pop().wait()


def bump_counter(bn):
    """nn.BatchNorm3d's per-forward ``num_batches_tracked += 1`` (training mode).  Also the point where a forward first touches a
    module buffer: a buffer broadcast launched ahead of the step is waited for here."""
    if _DEFERRED_WAITS:
        flush_deferred_waits()
    if bn.num_batches_tracked is None:
        return
    if _COUNTERS.active:
        _COUNTERS.seen[id(bn)] = (bn, _COUNTERS.seen.get(id(bn), (bn, 0))[1] + 1)
    else:
        bn.num_batches_tracked.add_(1)


def compute_dtype():
    return _AUTOCAST.stack[-1]


def _sfx(t):
    return _SFX[t.dtype]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def workspace(nbytes, device):
    """Per-device scratch buffer, grown on demand.  Stream-ordered reuse: all kernels of
    one process run on the current stream, so consecutive ops may share it."""
    buf = _WS.get(device)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _WS[device] = buf
    return buf


# ----------------------------------------------------------------------------- a step's weight packings in one launch (csrc/prepack.hip)
_PREPACK_OFF = bool(os.environ.get("MI355SEG_NO_PREPACK"))
_PREPACK_PLANS = weakref.WeakKeyDictionary()       # model -> {signature: {"plan": library plan id, "arena": uint8 tensor}}


def prepack_plans(model):
    """The prepack plans recorded for ``model``, or an empty dict.  Kept beside the models, not in them: a deep copy or an unpickled
    model starts without plans and records its own, and nothing of the arenas is serialised with a model."""
    return _PREPACK_PLANS.get(model, {})


def conv_math_signature():
    """The process-wide kernel policies that decide which packings a step's convolutions read (part of a prepack plan's key)."""
    L = lib()
    return (L.query("mi355seg_get_conv_math"), L.query("mi355seg_get_x3_shape"), L.query("mi355seg_get_b16_tiles"))


def _prepack_free(plans):
    try:
        L = lib()
        for rec in plans.values():
            L.call("mi355seg_prepack_free", rec["plan"])
    except Exception:            # interpreter shutdown
        pass


class prepacked_weights:
    """Context manager around ONE training iteration of ``model`` (forward AND backward inside it; engine.train_step).  The first
    iteration at a signature (``key`` = whatever fixes the kernels' plans: dtype, conv math, input shape; plus the parameters' storage
    addresses) runs as always while the library records every weight packing its convolutions launch (kept: those of the model's own
    parameter storage); each later one starts with
    ALL of those packings formed by one launch into an arena this object owns (include/mi355seg.h, mi355seg_prepack_run) and its
    convolutions read them there -- 44 small launches off the cfg-2 step's stream, ~50 off UNETR's.  Bit-identical results.
    One bracket per process at a time (the library refuses a second one).  MI355SEG_NO_PREPACK=1 turns it off."""

    # A recorded plan is being replayed for the running step: set and cleared here only.  Process-wide like the library's bracket, not
    # threading.local like _AUTOCAST / _COUNTERS: a step's backward runs on autograd's device thread, not on the one that entered.
    active = False

    def __init__(self, model, key):
        self.model, self.key, self.mode = model, key, None

    @property
    def replaying(self):
        return self.mode == "run" and prepacked_weights.active

    def __enter__(self):
        if _PREPACK_OFF:
            return self
        self.params = [p for p in self.model.parameters()]
        if not self.params or not self.params[0].is_cuda:
            return self
        sig = (self.key, tuple(p.data_ptr() for p in self.params))
        plans = _PREPACK_PLANS.get(self.model)
        if plans is None:
            plans = _PREPACK_PLANS[self.model] = {}
            weakref.finalize(self.model, _prepack_free, plans)
        rec = plans.get(sig)
        L = lib()
        if rec is None:
            if torch.cuda.is_current_stream_capturing():     # (a capture without eager warm-up: nothing recorded, the packings stay in place)
                return self
            if len(plans) >= 4:                              # shapes keep changing: forget the oldest
                old = next(iter(plans))
                L.call("mi355seg_prepack_free", plans.pop(old)["plan"])
            L.call("mi355seg_prepack_record_begin")
            self.mode, self.sig, self.plans = "record", sig, plans
        elif rec["plan"]:
            L.call("mi355seg_prepack_run", rec["plan"], _p(rec["arena"]), rec["arena"].numel(), _stream())
            self.mode = "run"
            prepacked_weights.active = L.query("mi355seg_prepack_active") != 0
        return self

    def __exit__(self, *exc):
        L = lib()
        mode, self.mode = self.mode, None
        if mode == "record":
            n = len(self.params)                             # the plan keeps what was packed out of these ranges (a copy _w32 made is gone by the next step)
            base = (ctypes.c_void_p * n)(*[p.data_ptr() for p in self.params])
            size = (ctypes.c_size_t * n)(*[p.numel() * p.element_size() for p in self.params])
            plan, nbytes = ctypes.c_int(0), ctypes.c_size_t(0)
            L.call("mi355seg_prepack_record_end", ctypes.byref(plan), ctypes.byref(nbytes), base, size, n)
            if exc[0] is not None:
                if plan.value:
                    L.call("mi355seg_prepack_free", plan.value)
            else:
                arena = torch.empty(max(int(nbytes.value), 256), dtype=torch.uint8, device=self.params[0].device) if plan.value else None
                self.plans[self.sig] = {"plan": plan.value, "arena": arena}
        elif mode == "run":                                  # (also when the body raised: the next step must find no open bracket)
            prepacked_weights.active = False
            L.call("mi355seg_prepack_done", _stream())
        return False


def _require_cuda(t, what, allow_bf16=False):
    if not t.is_cuda:
        raise Mi355SegError(f"{what}: expected a tensor on an MI355X (cuda/HIP) device, got {t.device}; "
                            "there is no CPU fallback in this package")
    if t.dtype != torch.float32 and not (allow_bf16 and t.dtype == torch.bfloat16):
        raise Mi355SegError(f"{what}: expected float32{' or bfloat16' if allow_bf16 else ''}, got {t.dtype}")


def aligned_contiguous(t):
    """``t.contiguous()`` at a 16-byte aligned address.  ``.contiguous()`` alone returns an already contiguous tensor as it is, and
    with it a misaligned storage offset (``x[1:]`` of a batch, a view into a flat buffer); the kernels' 16 B/lane paths need the
    alignment, so such a tensor is copied into storage of its own (the allocator hands out 256-byte aligned blocks)."""
    t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone(memory_format=torch.contiguous_format)
    return t


def cl_view(t, what="tensor", allow_bf16=True):
    """Return (tensor, ld) with tensor laid out NDHWC (last stride 1, dense in N,D,H,W with
    voxel pitch ld >= C).  Copies only if the given tensor does not already satisfy that."""
    _require_cuda(t, what, allow_bf16=allow_bf16)
    if t.dim() != 5:
        raise Mi355SegError(f"{what}: expected 5-D [N,D,H,W,C], got shape {tuple(t.shape)}")
    N, D, H, W, C = t.shape
    s = t.stride()
    ld = s[3]
    ok = (C == 1 or s[4] == 1) and ld >= C and W > 1
    ok = ok and (H == 1 or s[2] == W * ld) and (D == 1 or s[1] == H * W * ld) and (N == 1 or s[0] == D * H * W * ld)
    ok = ok and t.data_ptr() % 16 == 0          # the float4 paths assume a 16-byte aligned base
    if not ok:
        t = aligned_contiguous(t)
        ld = C
    return t, ld


def _p(t):
    return None if t is None else t.data_ptr()


def _like(g, x):
    """An incoming gradient in the storage type of the tensor it belongs to (autograd may hand over fp32 zeros)."""
    return g if g.dtype == x.dtype else g.to(x.dtype)


def _w32(w, what):
    if w.dtype != torch.float32:
        raise Mi355SegError(f"{what}: parameters are fp32 masters, got {w.dtype}")
    return w.contiguous()


def _iso(v, what):
    if isinstance(v, (tuple, list)):
        if len(set(v)) != 1:
            raise NotImplementedError(f"{what} must be isotropic, got {v}")
        return int(v[0])
    return int(v)


class _ConvGeom:
    """A Conv3d's geometry.  ``*g`` is (N, D, H, W, Cin, Cout, k, stride, pad): the nine arguments every mi355seg_conv3d_* entry point
    takes, in its order.  What the nodes read again and again on a launch-bound step is worked out once, here."""
    __slots__ = ("N", "D", "H", "W", "Cin", "Cout", "k", "stride", "pad", "args", "out_shape", "rows_in", "rows_out")

    def __init__(self, N, D, H, W, Cin, Cout, k, stride, pad):
        self.N, self.D, self.H, self.W, self.Cin, self.Cout, self.k, self.stride, self.pad = self.args = (N, D, H, W, Cin, Cout, k, stride, pad)
        Do, Ho, Wo = [(e + 2 * pad - k) // stride + 1 for e in (D, H, W)]
        self.out_shape = (N, Do, Ho, Wo, Cout)
        self.rows_in, self.rows_out = N * D * H * W, N * Do * Ho * Wo

    def __iter__(self):
        return iter(self.args)

    def ws_bytes(self, L, dtype):
        return L.query("mi355seg_conv3d_ws_bytes_bf16" if dtype == torch.bfloat16 else "mi355seg_conv3d_ws_bytes", *self.args)


def _conv_geom(x, w, stride, pad, what):
    """(geometry, contiguous fp32 weight) of ``what`` = a convolution of x -- a channel-last [N, D, H, W, Cin] tensor, or that shape --
    with the weight w (Cout, Cin, k, k, k)."""
    N, D, H, W, Cin = getattr(x, "shape", x)
    Cout, Cin_w, k, kh, kw = w.shape
    if Cin_w != Cin or kh != k or kw != k:
        raise Mi355SegError(f"{what}: weight {tuple(w.shape)} does not match input channels {Cin} / cubic kernel")
    return _ConvGeom(N, D, H, W, Cin, Cout, k, int(stride), int(pad)), _w32(w, what + " weight")


def _module_stride_pad(conv, what):
    """(stride, padding) of the nn.Conv3d module ``conv``; what the kernels do not implement is refused here, for every entry that takes a module."""
    if conv.groups != 1 or _iso(conv.dilation, "dilation") != 1 or conv.padding_mode != "zeros":
        raise NotImplementedError(f"{what}: only groups=1, dilation=1, zero padding are implemented")
    return _iso(conv.stride, "stride"), _iso(conv.padding, "padding")


def _module_geom(x, conv, what):
    """The geometry of the nn.Conv3d module ``conv`` applied to x (as _conv_geom, behind the checks of _module_stride_pad)."""
    return _conv_geom(x, conv.weight, *_module_stride_pad(conv, what), what)[0]


def to_channels_last(x, dtype=None):
    """fp32 [N,C,D,H,W] -> [N,D,H,W,C] in ``dtype`` (default: the autocast compute dtype; a free view when C == 1 and
    the result stays fp32).  This is where a model's activations take their storage type."""
    return _ToNDHWC.apply(x, dtype or compute_dtype())


def to_channels_first(x):
    """[N,D,H,W,C] (fp32 or bf16) -> fp32 [N,C,D,H,W] contiguous (free view when C == 1 and fp32): the model boundary
    always hands fp32 NCDHW tensors to the caller (logits go to an fp32 loss, as under torch autocast)."""
    return _ToNCDHW.apply(x)


class _ToNDHWC(Function):
    @staticmethod
    def forward(ctx, x, dtype):
        _require_cuda(x, "to_channels_last")
        if x.dtype != torch.float32:
            raise Mi355SegError(f"to_channels_last: the NCDHW side is fp32, got {x.dtype}")
        N, C, D, H, W = x.shape
        x = x.contiguous()
        if dtype == torch.float32:
            if C == 1:
                return x.view(N, D, H, W, 1)
            y = torch.empty((N, D, H, W, C), dtype=x.dtype, device=x.device)
            lib().call("mi355seg_ncdhw_to_ndhwc_f32", _p(x), _p(y), C, N, C, D * H * W, _stream())
            return y
        y = torch.empty((N, D, H, W, C), dtype=torch.bfloat16, device=x.device)
        lib().call("mi355seg_ncdhw_f32_to_ndhwc_bf16", _p(x), _p(y), C, N, C, D * H * W, _stream())
        return y

    @staticmethod
    def backward(ctx, g):
        return _ToNCDHW.apply(g), None


class _ToNCDHW(Function):
    @staticmethod
    def forward(ctx, x):
        x, ld = cl_view(x, "to_channels_first")
        N, D, H, W, C = x.shape
        ctx.src_dtype = x.dtype
        if x.dtype == torch.float32:
            if C == 1 and ld == 1:
                return x.view(N, 1, D, H, W)
            y = torch.empty((N, C, D, H, W), dtype=x.dtype, device=x.device)
            lib().call("mi355seg_ndhwc_to_ncdhw_f32", _p(x), ld, _p(y), N, C, D * H * W, _stream())
            return y
        y = torch.empty((N, C, D, H, W), dtype=torch.float32, device=x.device)
        lib().call("mi355seg_ndhwc_bf16_to_ncdhw_f32", _p(x), ld, _p(y), N, C, D * H * W, _stream())
        return y

    @staticmethod
    def backward(ctx, g):
        return _ToNDHWC.apply(g, ctx.src_dtype)


class _Cast(Function):
    """Storage-type change of a channel-last tensor (an autocast boundary inside a model, e.g. UNETR's fp32 token
    tensors entering the bf16 convolutional decoder); the gradient takes the opposite cast."""

    @staticmethod
    def forward(ctx, x, dtype):
        _require_cuda(x, "cast input", allow_bf16=True)
        ctx.src_dtype = x.dtype
        if x.dtype == dtype:
            return x.view_as(x)
        xc = x.contiguous()
        C = xc.shape[-1]
        rows = xc.numel() // C
        y = torch.empty(xc.shape, dtype=dtype, device=x.device)
        name = "mi355seg_cast_f32_to_bf16" if dtype == torch.bfloat16 else "mi355seg_cast_bf16_to_f32"
        lib().call(name, _p(xc), C, _p(y), C, rows, C, _stream())
        return y

    @staticmethod
    def backward(ctx, g):
        return _Cast.apply(g, ctx.src_dtype), None


def cast(x, dtype=None):
    """x in the storage type ``dtype`` (default: the autocast compute dtype)."""
    return _Cast.apply(x, dtype or compute_dtype())


# ----------------------------------------------------------------------------- f16x3 operand maxima
# The default conv math on fp32 tensors ("f16x3", include/mi355seg.h) splits every operand into two fp16 parts under a per-tensor
# power-of-two scale and needs max |.| of both operands as device scalars.  The plain entry points measure them with a pass of
# their own; here they ride along instead: the norm + activation kernels emit the maximum of what they write, a max-pool keeps
# its input's maximum, and a tensor carries its scalar as the attribute ``_seg_amax`` = (1-element fp32 tensor, tensor version)
# to whatever convolution reads it (a missing / stale attribute only means that the library measures).  Weight maxima are taken
# in the forward (one small launch per layer) and reused by that layer's backward.
_AMAX_POOL = {}


def _amax_slot(device):
    """A zeroed 1-element fp32 device tensor (the kernels max-combine into it), cut from a chunk that is zero-filled once."""
    st = _AMAX_POOL.get(device)
    if st is None or st[1] >= st[0].numel():
        st = [torch.zeros(2048, dtype=torch.float32, device=device), 0]
        _AMAX_POOL[device] = st
    slot = st[0][st[1]:st[1] + 1]
    st[1] += 1
    return slot


def amax_pool_reset():
    """Forget the current slot chunks (engine.GraphedTrainStep: a captured step must zero-fill the chunk it draws from inside the capture)."""
    _AMAX_POOL.clear()


def _takes_amax(x):
    return x.dtype == torch.float32 and lib().query("mi355seg_conv_math_takes_amax") != 0


_AMAX_USE = {}


def _amax_use(x, N, D, H, W, Cin, Cout, k, stride, pad):
    """Which passes of this layer read operand maxima under the selected conv math (bit 0 forward, 1 input gradient, 2 weight gradient)."""
    if x.dtype != torch.float32:
        return 0
    L = lib()
    key = (L.query("mi355seg_get_conv_math"), L.query("mi355seg_get_x3_shape"), N, D, H, W, Cin, Cout, k, stride, pad)
    use = _AMAX_USE.get(key)
    if use is None:
        use = _AMAX_USE[key] = L.query("mi355seg_conv3d_amax_use_f32", N, D, H, W, Cin, Cout, k, stride, pad)
    return use


_CHECK_AMAX = bool(os.environ.get("MI355SEG_CHECK_AMAX"))


def check_amax(enable=True):
    """Debug mode (also MI355SEG_CHECK_AMAX=1): every operand maximum a convolution is handed is compared with the tensor's true
    maximum (one synchronising reduction per use).  INVARIANT the carried scalars rest on: ``_seg_amax`` is keyed by the tensor's
    version counter, and the library's kernels write through ``data_ptr()`` without bumping it -- so whatever writes an fp32
    activation in place through a raw pointer AFTER its maximum was recorded must delete or refresh the attribute.  A too-SMALL
    maximum makes the f16x3 high part overflow fp16 silently; a too-large one only costs headroom."""
    global _CHECK_AMAX
    _CHECK_AMAX = bool(enable)


def _assert_amax(value, slot, what):
    """value: the operand tensor (any layout; only its values matter) or its true maximum as a float."""
    if not _CHECK_AMAX or slot is None:
        return
    true = float(value.detach().abs().max()) if torch.is_tensor(value) else float(value)
    have = float(slot.reshape(-1)[0])
    if not (have >= true * (1.0 - 1e-6)):
        raise Mi355SegError(f"operand maximum handed to {what} is too small: carried {have!r}, tensor has {true!r}")


def _get_amax(t):
    rec = getattr(t, "_seg_amax", None)
    if rec is None or rec[1] != t._version or rec[0].device != t.device:
        return None
    _assert_amax(t, rec[0], "a convolution (the tensor's _seg_amax attribute)")
    return rec[0]


def _set_amax(t, slot):
    if slot is not None:
        t._seg_amax = (slot, t._version)
    return t


def _measure_amax(t, ld, rows, C, slot=None):
    """max |t| over rows x C at pitch ld into a fresh slot (or max-combined into ``slot``)."""
    if slot is None:
        slot = _amax_slot(t.device)
    lib().call("mi355seg_amax_f32", _p(t), ld, rows, C, _p(slot), _stream())
    return slot


_WEIGHT_AMAX = {}


def prefetch_weight_amax(model):
    """max |w| of every 3x3x3 convolution weight of ``model`` by ONE multi-tensor launch (torch._foreach_norm, inf-norm) instead of
    one small launch per layer and forward (19 per U-Net step).  engine.train_step calls it ahead of the forward and drops the
    table (clear_weight_amax) when the step ends: the entries never outlive the weights they were measured on.  Keyed by the
    storage address, so stand-in leaves that alias a parameter (engine.GraphedTrainStep) find their entry too."""
    _WEIGHT_AMAX.clear()
    if lib().query("mi355seg_conv_math_takes_amax") == 0:
        return
    ws = [m.weight for m in model.modules()
          if isinstance(m, torch.nn.Conv3d) and m.weight is not None and m.weight.is_cuda and m.weight.dtype == torch.float32
          and m.weight.is_contiguous() and tuple(m.weight.shape[2:]) == (3, 3, 3)]
    if len(ws) < 2:
        return
    with torch.no_grad():
        norms = torch._foreach_norm(ws, float("inf"))
    for w, a in zip(ws, norms):
        _WEIGHT_AMAX[w.data_ptr()] = (a.reshape(1), w.numel())


def clear_weight_amax():
    _WEIGHT_AMAX.clear()


def _weight_amax(w):
    if prepacked_weights.active:       # the step's packings (and max |w| with them) were formed up front: the library hands the kernels its own scalars
        return None              # (a weight tensor the plan does not hold is measured by the entry point: NULL = measure)
    rec = _WEIGHT_AMAX.get(w.data_ptr())
    if rec is not None and rec[1] == w.numel() and rec[0].device == w.device:
        return rec[0]
    return _measure_amax(w, w.numel(), 1, w.numel())


# ----------------------------------------------------------------------------- conv
# The three passes of a convolution, then their fused forms (yamax / pro / folded forward, bnsums input gradient, pro / stem weight
# gradient).  These launchers are the only places that name a mi355seg_conv3d_* launch; what a fused form computes is in its
# launcher's docstring.  fp32 tensors always take the _ax entry: the library defines each plain fp32 entry as exactly that call with
# NULL maxima (NULL = the pass measures what it needs).
def _sums_ptrs(sums, C):
    """(sum, sum of squares): the two halves of an fp64 [2 * C] buffer a convolution's epilogue reduces its output into."""
    return (None, None) if sums is None else (sums.data_ptr(), sums.data_ptr() + 8 * C)


def _conv_fwd(L, g, x, ldx, w, b, y, ldy, ws, sums=None, xa=None, wa=None, res=None):
    """y = conv(x) + b.  sums: see _sums_ptrs (the batch statistics of y); xa / wa: f16x3 operand maxima; res = (tensor, ld), bf16
    only: y = conv(x) + b + res, the sum in the convolution's epilogue where the launch allows."""
    if x.dtype == torch.float32:
        if res is not None:
            raise Mi355SegError("conv3d: the residual epilogue exists for bf16 tensors only")
        L.call("mi355seg_conv3d_fwd_ax_f32", _p(x), ldx, _p(w), _p(b), _p(y), ldy, *g, *_sums_ptrs(sums, g.Cout), _p(xa), _p(wa),
               _p(ws), ws.numel(), _stream())
    elif res is not None:
        L.call("mi355seg_conv3d_fwd_res_bf16", _p(x), ldx, _p(w), _p(b), _p(res[0]), res[1], _p(y), ldy, *g, _p(ws), ws.numel(), _stream())
    else:
        L.call("mi355seg_conv3d_fwd_bf16", _p(x), ldx, _p(w), _p(b), _p(y), ldy, *g, *_sums_ptrs(sums, g.Cout), _p(ws), ws.numel(), _stream())


def _conv_dgrad(L, g, dy, lddy, w, dx, lddx, ws, da=None, wa=None, res=None):
    """dx = the input gradient of the convolution g.  res = (tensor, ld), bf16 only: dx = that + res (a second gradient of the same input)."""
    if dy.dtype == torch.float32:
        if res is not None:
            raise Mi355SegError("conv3d: the residual epilogue exists for bf16 tensors only")
        L.call("mi355seg_conv3d_dgrad_ax_f32", _p(dy), lddy, _p(w), _p(dx), lddx, *g, _p(da), _p(wa), _p(ws), ws.numel(), _stream())
    elif res is not None:
        L.call("mi355seg_conv3d_dgrad_res_bf16", _p(dy), lddy, _p(w), _p(res[0]), res[1], _p(dx), lddx, *g, _p(ws), ws.numel(), _stream())
    else:
        L.call("mi355seg_conv3d_dgrad_bf16", _p(dy), lddy, _p(w), _p(dx), lddx, *g, _p(ws), ws.numel(), _stream())


def _conv_wgrad(L, g, dy, lddy, x, ldx, dw, db, ws, da=None, xa=None):
    """dw (and db = the column sums of dy, where given) of the convolution g."""
    if x.dtype == torch.float32:
        L.call("mi355seg_conv3d_wgrad_ax_f32", _p(dy), lddy, _p(x), ldx, _p(dw), _p(db), *g, 0, _p(da), _p(xa), _p(ws), ws.numel(), _stream())
    else:
        L.call("mi355seg_conv3d_wgrad_bf16", _p(dy), lddy, _p(x), ldx, _p(dw), _p(db), *g, 0, _p(ws), ws.numel(), _stream())


def _conv_fwd_yamax(L, g, x, ldx, w, b, y, ldy, ws, sums, xa, wa, ya):
    """_conv_fwd (fp32 tensors, f16x3) whose epilogue also max-combines max |y| into the zeroed slot ya: what _norm_fold turns into a
    bound on the maximum of the activation that a norm-prologue convolution behind this one never sees written."""
    L.call("mi355seg_conv3d_fwd_yamax_ax_f32", _p(x), ldx, _p(w), _p(b), _p(y), ldy, *g, *_sums_ptrs(sums, g.Cout), _p(xa), _p(wa), _p(ya),
           _p(ws), ws.numel(), _stream())


def _conv_fwd_pro(L, g, x, ldx, alpha, beta, act, slope, w, b, y, ldy, ws, sums, xa, wa):
    """y = conv(act(x * alpha + beta)) + b (fp32 tensors, f16x3): x is the RAW output of the layer in front, normalised (in the folded
    per-channel form of _norm_fold) and activated while the tiles are staged, so that activation is never written; zero padding stays
    zero behind the prologue.  xa: a bound on max |act(x * alpha + beta)|."""
    L.call("mi355seg_conv3d_fwd_pro_ax_f32", _p(x), ldx, _p(alpha), _p(beta), act, slope, _p(w), _p(b), _p(y), ldy, *g,
           *_sums_ptrs(sums, g.Cout), _p(xa), _p(wa), _p(ws), ws.numel(), _stream())


def _conv_fwd_folded(L, g, x, ldx, w, b, gamma, beta, rmean, rvar, eps, act, slope, left_pad, ws):
    """act(BatchNorm(conv(x) + b)) under running statistics in one pass over x (inference: nothing is kept for a backward): a small launch
    folds the statistics, the affine parameters and the bias into a per-channel (scale, shift), which the convolution applies with the
    activation in its epilogue.  Returns the activation, the right channel slice of a concat buffer where left_pad (_concat_out)."""
    Cout = g.Cout
    fold = torch.empty(2 * Cout, dtype=torch.float32, device=x.device)
    L.call("mi355seg_bn_fold_f32", _p(gamma), _p(beta), _p(rmean), _p(rvar), _p(b), eps, Cout, fold.data_ptr(), fold.data_ptr() + 4 * Cout, _stream())
    _, a, lda = _concat_out(g.out_shape[:4], left_pad, Cout, x.dtype, x.device)
    L.call("mi355seg_conv3d_fwd_fused_" + _sfx(x), _p(x), ldx, _p(w), fold.data_ptr(), fold.data_ptr() + 4 * Cout, act, slope,
           a.data_ptr(), lda, *g, _p(ws), ws.numel(), _stream())
    return a


def _conv_dgrad_bnsums(L, g, dy, lddy, w, y_in, mean, rstd, gamma, beta, act, slope, ws, da=None, wa=None):
    """(dx, sums, dgamma, dbeta) of a convolution g whose input is act(norm(y_in)) with exactly this one consumer (fp32): dx is the input
    gradient, i.e. d(that activation), and the kernel's epilogue reduces the norm backward's two column sums over it and y_in -- sums,
    fp32 [2 * Cin], which _norm_act_bwd_apply or _stem_wgrad_bnbwd goes on from -- and the norm's affine gradients, instead of a pass of
    their own over dx and y_in."""
    Cin, dev = g.Cin, dy.device
    dx = torch.empty((g.N, g.D, g.H, g.W, Cin), dtype=dy.dtype, device=dev)
    sums = torch.empty(2 * Cin, dtype=torch.float32, device=dev)
    dgamma, dbeta = torch.empty(Cin, dtype=torch.float32, device=dev), torch.empty(Cin, dtype=torch.float32, device=dev)
    L.call("mi355seg_conv3d_dgrad_bnsums_ax_f32", _p(dy), lddy, _p(w), _p(dx), Cin, *g, _p(y_in), Cin, _p(mean), _p(rstd), _p(gamma), _p(beta),
           act, slope, sums.data_ptr(), sums.data_ptr() + 4 * Cin, _p(dgamma), _p(dbeta), _p(da), _p(wa), _p(ws), ws.numel(), _stream())
    return dx, sums, dgamma, dbeta


def _conv_wgrad_pro(L, g, dy, lddy, x, ldx, alpha, beta, act, slope, w, ws, da=None, xa=None):
    """dw of _conv_fwd_pro: the weight gradient against act(x * alpha + beta), formed from the raw x while the tiles are staged.  The
    form exists under the conv math of its forward only and the entry point refuses under another (the activation the plain form would
    need was never written): _DoubleConvBnAct.backward runs under the forward's math for that reason."""
    dw = torch.empty_like(w)
    L.call("mi355seg_conv3d_wgrad_pro_ax_f32", _p(dy), lddy, _p(x), ldx, _p(alpha), _p(beta), act, slope, _p(dw), None, *g,
           0, _p(da), _p(xa), _p(ws), ws.numel(), _stream())
    return dw


def _stem_wgrad_bnbwd(L, lay, da, y, mean, rstd, gamma, beta, act, slope, sums, x, w, ws):
    """(dw, db) of the 1-channel stem ``lay`` behind a norm + activation whose gradient da = d(activation) has ONE consumer, this weight
    gradient (the stem's input needs none): the kernel forms d(conv output) from da, y and the norm backward's column sums
    (_conv_dgrad_bnsums) on the fly -- the apply half of the norm backward and the tensor it would write are gone.  db: None without a bias."""
    g, C = lay.g, lay.g.Cout
    dw = torch.empty_like(w)
    db = torch.empty(C, dtype=torch.float32, device=x.device) if lay.has_bias else None
    L.call("mi355seg_stem_wgrad_bnbwd_f32", _p(da), C, _p(y), C, _p(mean), _p(rstd), _p(gamma), _p(beta), act, slope,
           sums.data_ptr(), sums.data_ptr() + 4 * C, _p(x), lay.ldx, _p(dw), _p(db), *g, _p(ws), ws.numel(), _stream())
    return dw, db


class _ConvLayer:
    """What one conv (+ norm) layer of a node keeps for its backward beside the saved tensors: g the _ConvGeom, ldx the input's pitch,
    has_bias, amax = the f16x3 operand slots (xa, wa) of (input, weight) -- None where the backward hands its convolutions no maxima and
    draws no slot for max |dy| -- and out_amax, the slot with the maximum of the activation the layer hands on (None: nothing carried)."""
    __slots__ = ("g", "ldx", "has_bias", "amax", "out_amax")

    def __init__(self, g, ldx, has_bias, amax=None, out_amax=None):
        self.g, self.ldx, self.has_bias, self.amax, self.out_amax = g, ldx, has_bias, amax, out_amax


def _conv_stats_fwd(L, g, x, ldx, w, b, ws, xa_in, ya=None, pro=None):
    """(y, sums, layer record) of a training-mode conv + BatchNorm layer: y = conv(x) + b with the batch statistics' fp64 column sums
    (_sums_ptrs) from the convolution's epilogue and the f16x3 operand maxima riding along (xa_in: what x carries).  ya: the yamax form
    (_conv_fwd_yamax); pro = (alpha, beta, act, slope): the norm-prologue form (_conv_fwd_pro; x is raw, xa_in bounds its activation)."""
    Cout = g.Cout
    y = torch.empty(g.out_shape, dtype=x.dtype, device=x.device)
    sums = torch.empty(2 * Cout, dtype=torch.float64, device=x.device)
    xa, wa = _operand_amax(g, x, ldx, w, xa_in, True) or (None, None)
    if _CHECK_AMAX:
        _assert_amax(w, wa, "conv weights")
        if pro is not None:              # the bound on the prologue's output against the activation it stands for
            z = x * pro[0] + pro[1]
            _assert_amax(torch.where(z > 0, z, z * (pro[3] if pro[2] == ACT_LRELU else 0.0)), xa, "the norm prologue's bound")
        elif xa is not None:
            _assert_amax(x, xa, "conv input")
    if pro is not None:
        _conv_fwd_pro(L, g, x, ldx, *pro, w, b, y, Cout, ws, sums, xa, wa)
    elif ya is not None:
        _conv_fwd_yamax(L, g, x, ldx, w, b, y, Cout, ws, sums, xa, wa, ya)
    else:
        _conv_fwd(L, g, x, ldx, w, b, y, Cout, ws, sums, xa, wa)
    return y, sums, _ConvLayer(g, ldx, b is not None, (xa, wa) if (xa is not None or wa is not None) else None)


def _conv_grads(L, lay, dy, lddy, x, w, need_dx, need_dw, ws, da=None, add=None, bias_grad=False):
    """(dx, dw, db) of the convolution ``lay`` from one dy, each None unless needed; db -- the column sums of dy, from the weight gradient --
    only with bias_grad (behind a norm the bias gradient comes out of the norm backward).  da: the slot with max |dy| where something
    carried it; where the layer's passes read maxima (lay.amax), nothing carried dy's and both gradients read it, it is measured here,
    once.  add = (tensor, ld): a second gradient of x summed into dx, bf16 in the input gradient's epilogue, fp32 by a pass straight after."""
    g = lay.g
    xa, wa = lay.amax or (None, None)
    if lay.amax is not None and da is None and need_dx and need_dw:
        da = _measure_amax(dy, lddy, g.rows_out, g.Cout)
    dx = dw = db = None
    if need_dx:
        dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        res = add if x.dtype == torch.bfloat16 else None
        _conv_dgrad(L, g, dy, lddy, w, dx, g.Cin, ws, da, wa, res)
        if add is not None and res is None:
            L.call("mi355seg_act_fwd_" + _sfx(x), _p(dx), g.Cin, _p(add[0]), add[1], _p(dx), g.Cin, g.rows_in, g.Cin, ACT_NONE, 0.0, _stream())
    if need_dw:
        dw = torch.empty_like(w)
        db = torch.empty(g.Cout, dtype=torch.float32, device=x.device) if bias_grad and lay.has_bias else None
        _conv_wgrad(L, g, dy, lddy, x, lay.ldx, dw, db, ws, da, xa)
    return dx, dw, db


def _grads(names, **by_name):
    """A backward's result: for each forward parameter in ``names`` the gradient given under its name, None for the rest."""
    out = [None] * len(names)
    for name, grad in by_name.items():
        out[names.index(name)] = grad
    return tuple(out)


def _operand_amax(g, x, ldx, w, xa_in, measure_x):
    """The f16x3 operand maxima (xa, wa) that the three passes of the layer g are handed -- or None where none of them reads maxima (bf16
    tensors, the other conv maths, a layer without an f16x3 form).  xa_in: the maximum x carries, if any; it is kept whenever some
    pass reads maxima and dropped otherwise (_Conv3d, _ConvBnAct and _DoubleConvBnAct always agreed on that).  max |w| is taken
    where the forward or the input gradient reads it.  measure_x: x is measured here, once, when nothing carried its maximum and
    both its readers -- the forward and the weight gradient -- want it; a caller passes False when its weight gradient will not run
    (_Conv3d: the weight may need no gradient), and either reader then measures for itself.  A member that stays None means the same."""
    use = _amax_use(x, *g)
    if not use:
        return None
    wa = _weight_amax(w) if use & 3 else None
    xa = xa_in
    if xa is None and measure_x and (use & 1) and (use & 4):
        xa = _measure_amax(x, ldx, g.rows_in, g.Cin)
    return xa, wa


def _stats_from_sums(L, sums, rows, C, eps, running_mean, running_var, momentum):
    """(mean, rstd) fp32 [C] from the fp64 column sums a convolution's epilogue left (_sums_ptrs); running statistics, where given, are
    updated in place as nn.BatchNorm3d does in training mode."""
    mean = torch.empty(C, dtype=torch.float32, device=sums.device)
    rstd = torch.empty(C, dtype=torch.float32, device=sums.device)
    L.call("mi355seg_norm_stats_from_sums_f32", *_sums_ptrs(sums, C), rows, C, eps, _p(mean), _p(rstd), _p(running_mean), _p(running_var),
           momentum, _stream())
    return mean, rstd


def _norm_fold(L, sums, rows, C, eps, gamma, beta, act, running_mean, running_var, momentum, ya):
    """(mean, rstd, alpha, shift, bound) by one small launch: _stats_from_sums, the normalisation folded into the per-channel form
    y * alpha + shift that a norm-prologue convolution applies (_conv_fwd_pro), and -- from ya, the slot with max |y| (_conv_fwd_yamax) --
    a fresh slot with a bound on max |act(y * alpha + shift)|, the maximum of the activation that is never written."""
    dev = sums.device
    mean = torch.empty(C, dtype=torch.float32, device=dev)
    rstd = torch.empty(C, dtype=torch.float32, device=dev)
    fold = torch.empty(2 * C, dtype=torch.float32, device=dev)
    bound = _amax_slot(dev)
    L.call("mi355seg_norm_fold_f32", *_sums_ptrs(sums, C), rows, C, eps, _p(gamma), _p(beta), act, _p(mean), _p(rstd), _p(running_mean),
           _p(running_var), momentum, _p(ya), fold.data_ptr(), fold.data_ptr() + 4 * C, _p(bound), _stream())
    return mean, rstd, fold[:C], fold[C:], bound


def _concat_base(t, Cout, lead_shape, dtype):
    """The concat buffer that ``t`` is the right channel slice of -- a contiguous 5-D ``dtype`` tensor of shape lead_shape + (Cout + C_t,)
    with exactly Cout free channels on t's left -- or None if t is no such slice."""
    base = getattr(t, "_base", None)
    ok = (base is not None and base.dim() == 5 and base.is_contiguous() and tuple(base.shape) == tuple(lead_shape) + (Cout + t.shape[-1],)
          and base.dtype == dtype and t.data_ptr() == base.data_ptr() + base.element_size() * Cout and t.stride() == base.stride())
    return base if ok else None


def _concat_out(lead_shape, left_pad, C, dtype, device):
    """(buffer, result, pitch) of a node whose C-channel result is the RIGHT channel slice of a fresh buffer with left_pad free channels on
    its left, which a later node fills (_concat_base recognises the slice): the skip concatenations without the copies.  left_pad = 0: no
    buffer (None), a dense result."""
    full = torch.empty(tuple(lead_shape) + (left_pad + C,), dtype=dtype, device=device)
    return (full, full[..., left_pad:], left_pad + C) if left_pad else (None, full, C)


# ----------------------------------------------------------------------------- norm / activation / pool launchers
# As for the convolutions: the only places that name a mi355seg_norm_stats_*, rstd_from_var, norm_act_fwd*, norm_act_bwd_colsum*,
# norm_act_bwd_apply*, bn_act_head_*, bn_act_pool_*, maxpool2_{fwd,bwd}*, upsample2_bwd_* or act_bwd_* entry point (norm_fold sits beside
# _stats_from_sums).  The norm passes always take the widest entry (_ax / _colsum_ax): the library defines the narrower ones as exactly
# that call with a NULL maximum and / or a NULL column sum.  An optional tensor travels as the pair (tensor, ld) that _opt_view returns.
_NO_RES = (None, 0)
_EVAL_BN_BACKWARD = "backward through eval-mode BatchNorm (running statistics) is not supported"


def _opt_view(t, what):
    """cl_view of an optional tensor: (t, ld), or (None, 0) for an absent one."""
    return _NO_RES if t is None else cl_view(t, what)


def _norm_rows(shape, instance):
    """(rows, groups) a norm reduces over for a channel-last ``shape``: every voxel of the batch in one group (BatchNorm), or one group per sample."""
    N, D, H, W, _ = shape
    return (D * H * W, N) if instance else (N * D * H * W, 1)


def _norm_ws(L, rows, groups, C, device):
    """The workspace of a norm pass (statistics, backward) over rows x C in ``groups`` groups."""
    return workspace(L.query("mi355seg_norm_ws_bytes", rows, groups, C), device)


def _conv_norm_ws(L, g, dtype, rows, C):
    """Bytes of the one workspace a convolution g and the norm passes over its rows x C output share."""
    return max(g.ws_bytes(L, dtype), L.query("mi355seg_norm_ws_bytes", rows, 1, C))


def _batch_stats(L, x, ldx, rows, groups, C, eps, rm, rv, momentum, ws):
    """(mean, rstd) fp32 [groups * C] of x by a pass over it; rm / rv: running statistics to update in place as nn.BatchNorm3d does in
    training mode (None: leave them alone)."""
    mean = torch.empty(groups * C, dtype=torch.float32, device=x.device)
    rstd = torch.empty(groups * C, dtype=torch.float32, device=x.device)
    L.call("mi355seg_norm_stats_" + _sfx(x), _p(x), ldx, rows, groups, C, eps, _p(mean), _p(rstd), _p(rm), _p(rv), momentum,
           _p(ws), ws.numel(), _stream())
    return mean, rstd


def _running_stats(L, rm, rv, eps, C):
    """(mean, rstd) of eval-mode BatchNorm: the running mean itself and 1 / sqrt(running_var + eps)."""
    rstd = torch.empty(C, dtype=torch.float32, device=rv.device)
    L.call("mi355seg_rstd_from_var_f32", _p(rv), eps, _p(rstd), C, _stream())
    return rm, rstd


def _norm_act_fwd(L, x, ldx, mean, rstd, gamma, beta, res, y_ptr, ldy, rows, groups, C, act, slope, amax=None):
    """act((x - mean) * rstd * gamma + beta [+ res]) written at the address y_ptr with pitch ldy; amax: a zeroed slot that receives max |y|."""
    L.call("mi355seg_norm_act_fwd_ax_" + _sfx(x), _p(x), ldx, _p(mean), _p(rstd), _p(gamma), _p(beta), _p(res[0]), res[1],
           y_ptr, ldy, rows, groups, C, act, slope, _p(amax), _stream())


def _norm_act_bwd(L, dy, lddy, x, ldx, mean, rstd, gamma, beta, res, rows, groups, C, act, slope, ws, colsum=False, amax=None):
    """(dx, dgamma, dbeta, dres, db) of _norm_act_fwd under batch / instance statistics, all allocated here: dgamma / dbeta are None without
    affine parameters, dres without a residual, and db -- the column sums of dx, the bias gradient of the convolution in front of the
    norm -- unless ``colsum``; amax: a zeroed slot that receives max |dx|."""
    dev = x.device
    dx = torch.empty(x.shape, dtype=x.dtype, device=dev)
    dgamma = torch.empty(C, dtype=torch.float32, device=dev) if gamma is not None else None
    dbeta = torch.empty(C, dtype=torch.float32, device=dev) if gamma is not None else None
    dres = torch.empty(x.shape, dtype=x.dtype, device=dev) if res[0] is not None else None
    db = torch.empty(C, dtype=torch.float32, device=dev) if colsum else None
    L.call("mi355seg_norm_act_bwd_colsum_ax_" + _sfx(x), _p(dy), lddy, _p(x), ldx, _p(mean), _p(rstd), _p(gamma), _p(beta), _p(res[0]), res[1],
           _p(dx), C, _p(dgamma), _p(dbeta), _p(dres), C, _p(db), _p(amax), rows, groups, C, act, slope, _p(ws), ws.numel(), _stream())
    return dx, dgamma, dbeta, dres, db


def _norm_act_bwd_apply(L, dy, lddy, x, mean, rstd, gamma, beta, sums, act, slope, ws, colsum=False, amax=None):
    """(dx, db): the second half of _norm_act_bwd for a dense fp32 x under batch statistics, where the first half -- the two column sums,
    ``sums`` fp32 [2 * C], and with them dgamma / dbeta -- came out of another kernel (_conv_dgrad_bnsums).  db: the column sums of dx
    with ``colsum``, else None; amax: a zeroed slot that receives max |dx|."""
    C = x.shape[-1]
    dx = torch.empty_like(x)
    db = torch.empty(C, dtype=torch.float32, device=x.device) if colsum else None
    L.call("mi355seg_norm_act_bwd_apply_ax_f32", _p(dy), lddy, _p(x), C, _p(mean), _p(rstd), _p(gamma), _p(beta), None, 0,
           sums.data_ptr(), sums.data_ptr() + 4 * C, _p(dx), C, None, 0, _p(db), _p(amax), x.numel() // C, 1, C, act, slope, _p(ws), ws.numel(), _stream())
    return dx, db


def _layer_norm_act_bwd(L, lay, da, ldda, y, mean, rstd, gamma, beta, act, slope, ws, amax=None):
    """(dy, dgamma, dbeta, db) of the norm + activation behind the convolution ``lay`` under batch statistics (_norm_act_bwd over that
    layer's dense output y): dy = d(conv output), db the convolution's bias gradient (None without a bias)."""
    g = lay.g
    dy, dgamma, dbeta, _, db = _norm_act_bwd(L, da, ldda, y, g.Cout, mean, rstd, gamma, beta, _NO_RES, g.rows_out, 1, g.Cout, act, slope, ws,
                                             lay.has_bias, amax)
    return dy, dgamma, dbeta, db


def _bn_act_head_fwd(L, y, mean, rstd, gamma, beta, act, slope, wh, bh):
    """The logits head(act(norm(y))) of a 1x1x1 head (weight wh [K, C, 1, 1, 1], bias bh or None) behind a norm + activation, as one
    kernel over the dense fp32 y (csrc/bn_head.hip): the activation itself is never written."""
    C, K = y.shape[-1], wh.shape[0]
    logits = torch.empty(y.shape[:4] + (K,), dtype=y.dtype, device=y.device)
    L.call("mi355seg_bn_act_head_fwd_f32", _p(y), C, _p(mean), _p(rstd), _p(gamma), _p(beta), act, slope, _p(wh), _p(bh),
           _p(logits), K, y.numel() // C, C, K, _stream())
    return logits


def _bn_act_head_bwd(L, dlogits, lddl, y, mean, rstd, gamma, beta, act, slope, wh, head_bias, colsum, ws, amax=None):
    """(dy, dgamma, dbeta, db, dwh, dbh) of _bn_act_head_fwd in two launches: one pass over y and d(logits) for the norm backward's column
    sums (with them dgamma / dbeta) and the head's weight / bias gradients (dbh: None unless head_bias), a second one for dy with db, its
    column sums (the bias gradient of the convolution in front; None unless ``colsum``); amax: a zeroed slot that receives max |dy|."""
    C, K = y.shape[-1], wh.shape[0]
    rows = y.numel() // C
    f32 = dict(dtype=torch.float32, device=y.device)
    dy = torch.empty_like(y)
    dgamma, dbeta = torch.empty(C, **f32), torch.empty(C, **f32)
    db = torch.empty(C, **f32) if colsum else None
    sums = torch.empty(2 * C, **f32)
    dwh = torch.empty_like(wh)
    dbh = torch.empty(K, **f32) if head_bias else None
    L.call("mi355seg_bn_act_head_bwd_sums_f32", _p(dlogits), lddl, _p(y), C, _p(mean), _p(rstd), _p(gamma), _p(beta), act, slope, _p(wh),
           sums.data_ptr(), sums.data_ptr() + 4 * C, _p(dgamma), _p(dbeta), _p(dwh), _p(dbh), rows, C, K, _p(ws), ws.numel(), _stream())
    L.call("mi355seg_bn_act_head_bwd_apply_f32", _p(dlogits), lddl, _p(y), C, _p(mean), _p(rstd), _p(gamma), _p(beta), act, slope, _p(wh),
           sums.data_ptr(), sums.data_ptr() + 4 * C, _p(dy), C, _p(db), _p(amax), rows, C, K, _p(ws), ws.numel(), _stream())
    return dy, dgamma, dbeta, db, dwh, dbh


def _bn_act_pool_fwd(L, y, mean, rstd, gamma, beta, act, slope, left_pad, amax=None):
    """(a, pooled, idx) as one kernel over the dense fp32 y: a = act(norm(y)) -- the right channel slice of a concat buffer where left_pad
    (_concat_out) --, pooled = MaxPool3d(2, 2)(a) and the uint8 argmax codes of its windows (_maxpool2_fwd); amax: a zeroed slot that
    receives max |a|."""
    N, D, H, W, C = y.shape
    _, a, lda = _concat_out((N, D, H, W), left_pad, C, y.dtype, y.device)
    pooled = torch.empty((N, D // 2, H // 2, W // 2, C), dtype=y.dtype, device=y.device)
    idx = torch.empty((N, D // 2, H // 2, W // 2, C), dtype=torch.uint8, device=y.device)
    L.call("mi355seg_bn_act_pool_fwd_f32", _p(y), C, _p(mean), _p(rstd), _p(gamma), _p(beta), act, slope, a.data_ptr(), lda,
           _p(pooled), _p(idx), _p(amax), N, D, H, W, C, _stream())
    return a, pooled, idx


def _bn_act_pool_bwd(L, da, dpooled, idx, y, mean, rstd, gamma, beta, act, slope, colsum, ws, amax=None):
    """(dy, dgamma, dbeta, db) of _bn_act_pool_fwd: d(activation) = da + pool_backward(dpooled) exists only inside the two passes of the
    norm backward.  da / dpooled: None for an unused output (its gradient is zero); db: the column sums of dy with ``colsum``, else None;
    amax: a zeroed slot that receives max |dy|."""
    N, D, H, W, C = y.shape
    f32 = dict(dtype=torch.float32, device=y.device)
    dy = torch.empty_like(y)
    dgamma, dbeta = torch.empty(C, **f32), torch.empty(C, **f32)
    db = torch.empty(C, **f32) if colsum else None
    if da is None:
        da = torch.zeros(y.shape, **f32)
    if dpooled is None:
        dpooled = torch.zeros(idx.shape, **f32)
    da, ldda = cl_view(_like(da, y), "skip grad")
    dpooled = dpooled.contiguous()
    sums = torch.empty(2 * C, **f32)
    L.call("mi355seg_bn_act_pool_bwd_f32", _p(da), ldda, _p(dpooled), _p(idx), _p(y), C, _p(mean), _p(rstd), _p(gamma), _p(beta), act, slope,
           sums.data_ptr(), sums.data_ptr() + 4 * C, _p(dgamma), _p(dbeta), _p(dy), C, _p(db), _p(amax), N, D, H, W, C, _p(ws), ws.numel(), _stream())
    return dy, dgamma, dbeta, db


def _act_bwd(dy, lddy, x, ldx, res, rows, C, act, slope, add=None):
    """dx = dy * act'(x [+ res]); add = (tensor, ld): the one-pass form that also sums a second gradient of x in (a NULL tensor adds nothing)."""
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    extra = () if add is None else (_p(add[0]), add[1])
    lib().call("mi355seg_act_bwd_" + ("add_" if extra else "") + _sfx(x), _p(dy), lddy, _p(x), ldx, _p(res[0]), res[1], *extra, _p(dx), C,
               rows, C, act, slope, _stream())
    return dx


def _maxpool2_fwd(x, ldx):
    """(pooled, uint8 argmax codes 0..7 of each 2x2x2 window) of MaxPool3d(2, 2)."""
    N, D, H, W, C = x.shape
    y = torch.empty((N, D // 2, H // 2, W // 2, C), dtype=x.dtype, device=x.device)
    idx = torch.empty((N, D // 2, H // 2, W // 2, C), dtype=torch.uint8, device=x.device)
    lib().call("mi355seg_maxpool2_fwd_" + _sfx(x), _p(x), ldx, _p(y), C, _p(idx), N, D, H, W, C, _stream())
    return y, idx


def _maxpool2_bwd(dy, lddy, idx, shape, add=None):
    """dx of the pooled tensor's input of ``shape``; add = (tensor, ld): a second gradient of that input, summed in the same pass."""
    N, D, H, W, C = shape
    dx = torch.empty((N, D, H, W, C), dtype=dy.dtype, device=dy.device)
    extra = () if add is None else (_p(add[0]), add[1])
    lib().call("mi355seg_maxpool2_bwd_" + ("add_" if extra else "") + _sfx(dy), _p(dy), lddy, _p(idx), *extra, _p(dx), C, N, D, H, W, C, _stream())
    return dx


def _upsample2_bwd(dy, lddy):
    """dx of nearest-neighbour upsampling by two: the sums of dy's 2x2x2 windows."""
    N, D2, H2, W2, C = dy.shape
    dx = torch.empty((N, D2 // 2, H2 // 2, W2 // 2, C), dtype=dy.dtype, device=dy.device)
    lib().call("mi355seg_upsample2_bwd_" + _sfx(dy), _p(dy), lddy, _p(dx), C, N, D2 // 2, H2 // 2, W2 // 2, C, _stream())
    return dx


class _Conv3d(Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, pad, res=None):
        xa_in = _get_amax(x)
        x, ldx = cl_view(x, "conv3d input")
        g, w = _conv_geom(x, w, stride, pad, "conv3d")
        y = torch.empty(g.out_shape, dtype=x.dtype, device=x.device)
        L = lib()
        ws = workspace(g.ws_bytes(L, x.dtype), x.device)
        if res is not None:                  # bf16: conv(x) + res, the sum in the convolution's epilogue where the launch allows
            res, ldres = cl_view(res, "conv3d residual")
            if res.shape != y.shape or res.dtype != x.dtype:
                raise Mi355SegError(f"conv3d: residual {tuple(res.shape)} {res.dtype} does not match the output {tuple(y.shape)} {x.dtype}")
            res = (res, ldres)
        # (a pair without members still says that some pass reads maxima: the backward then measures dy once for its two readers)
        amax = _operand_amax(g, x, ldx, w, xa_in, ctx.needs_input_grad[1])
        xa, wa = amax or (None, None)
        _conv_fwd(L, g, x, ldx, w, b, y, g.Cout, ws, None, xa, wa, res)
        ctx.save_for_backward(x, w)
        ctx.layer = _ConvLayer(g, ldx, b is not None, amax)
        ctx.has_res = res is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        lay = ctx.layer
        dy, lddy = cl_view(_like(dy, x), "conv3d grad")
        L = lib()
        ws = workspace(lay.g.ws_bytes(L, x.dtype), x.device)
        need_dw = ctx.needs_input_grad[1] or (lay.has_bias and ctx.needs_input_grad[2])
        da = _get_amax(dy) if lay.amax is not None else None
        dx, dw, db = _conv_grads(L, lay, dy, lddy, x, w, ctx.needs_input_grad[0], need_dw, ws, da, bias_grad=True)
        return _grads(_CONV3D_ARGS, x=dx, w=dw, b=db, res=dy if ctx.has_res else None)      # d(conv + res) / d res = dy itself


_CONV3D_ARGS = ("x", "w", "b", "stride", "pad", "res")


def conv3d(x, weight, bias=None, stride=1, padding=0, residual=None):
    """nn.Conv3d on a channel-last tensor (cubic kernel, isotropic stride/padding); residual: conv(x) + residual (bf16 tensors: one
    launch where the convolution's epilogue can take the sum, mi355seg_conv3d_fwd_res_bf16)."""
    if residual is None:
        return _Conv3d.apply(x, weight, bias, int(stride), int(padding))
    if x.dtype == torch.bfloat16 and residual.dtype == torch.bfloat16:
        return _Conv3d.apply(x, weight, bias, int(stride), int(padding), residual)
    return activation(_Conv3d.apply(x, weight, bias, int(stride), int(padding)), ACT_NONE, residual=residual)


def _convt_k2s2_ws(L, x, Cout):
    N, D, H, W, Cin = x.shape
    return workspace(L.query("mi355seg_convt3d_k2s2_ws_bytes", N, D, H, W, Cin, Cout), x.device)


def _convt_k2s2_fwd(L, x, ldx, w, b, y_ptr, ldy, amax=None):
    """ConvTranspose3d k2 s2 of x, written at the address y_ptr with voxel pitch ldy (a dense result, or the left channels of a concat
    buffer); amax (fp32 tensors): a zeroed slot into which the kernel's epilogue max-combines the maximum of what it writes."""
    N, D, H, W, Cin = x.shape
    Cout = w.shape[1]
    ws = _convt_k2s2_ws(L, x, Cout)
    extra = () if amax is None else (_p(amax),)
    L.call("mi355seg_convt3d_k2s2_fwd_" + ("ax_f32" if extra else _sfx(x)), _p(x), ldx, _p(w), _p(b), y_ptr, ldy, N, D, H, W, Cin, Cout, *extra,
           _p(ws), ws.numel(), _stream())


def _convt_k2s2_bwd(L, x, ldx, dy, lddy, w, has_b, need_dx, need_dw):
    """(dx, dw, db) of ConvTranspose3d k2 s2: x the layer's input, dy the gradient of its output -- possibly the left channel slice of a
    wider gradient at pitch lddy; whatever is not needed (or does not exist: db without a bias) comes back as None."""
    N, D, H, W, Cin = x.shape
    Cout = w.shape[1]
    ws = _convt_k2s2_ws(L, x, Cout)
    dx = dw = db = None
    if need_dx:
        dx = torch.empty((N, D, H, W, Cin), dtype=x.dtype, device=x.device)
        L.call("mi355seg_convt3d_k2s2_dgrad_" + _sfx(x), _p(dy), lddy, _p(w), _p(dx), Cin, N, D, H, W, Cin, Cout,
               _p(ws), ws.numel(), _stream())
    if need_dw:
        dw = torch.empty_like(w)
        db = torch.empty(Cout, dtype=torch.float32, device=x.device) if has_b else None
        L.call("mi355seg_convt3d_k2s2_wgrad_" + _sfx(x), _p(dy), lddy, _p(x), ldx, _p(dw), _p(db), N, D, H, W, Cin, Cout,
               _p(ws), ws.numel(), _stream())
    return dx, dw, db


class _ConvT3dK2S2(Function):
    @staticmethod
    def forward(ctx, x, w, b):
        x, ldx = cl_view(x, "conv_transpose3d input")
        N, D, H, W, Cin = x.shape
        if tuple(w.shape[2:]) != (2, 2, 2) or w.shape[0] != Cin:
            raise Mi355SegError(f"conv_transpose3d_k2s2: weight {tuple(w.shape)} must be (Cin={Cin}, Cout, 2, 2, 2)")
        Cout = w.shape[1]
        w = w.contiguous()
        y = torch.empty((N, 2 * D, 2 * H, 2 * W, Cout), dtype=x.dtype, device=x.device)
        _convt_k2s2_fwd(lib(), x, ldx, w, b, y.data_ptr(), Cout)
        ctx.save_for_backward(x, w)
        ctx.geom = (ldx, b is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        ldx, has_b = ctx.geom
        dy, lddy = cl_view(_like(dy, x), "conv_transpose3d grad")
        return _convt_k2s2_bwd(lib(), x, ldx, dy, lddy, w, has_b, ctx.needs_input_grad[0],
                               ctx.needs_input_grad[1] or (has_b and ctx.needs_input_grad[2]))


class _ConvT3dK2S2Cat(Function):
    """cat(conv_transpose3d_k2s2(x), skip) along channels without the copy: ``skip`` must be the right channel slice
    of a buffer with exactly Cout free channels on its left (conv_bn_act(..., left_pad=Cout)); the up-convolution is
    written into those channels and the whole buffer is returned."""

    @staticmethod
    def forward(ctx, x, w, b, skip):
        x, ldx = cl_view(x, "conv_transpose3d input")
        N, D, H, W, Cin = x.shape
        Cout = w.shape[1]
        base = _concat_base(skip, Cout, (N, 2 * D, 2 * H, 2 * W), x.dtype)
        if base is None:
            raise Mi355SegError("conv_transpose3d_k2s2_cat: `skip` is not the right channel slice of a matching concat buffer")
        w = w.contiguous()
        sa = _get_amax(skip) if _takes_amax(x) else None
        # max |cat| = max(max |up-convolution| (from that kernel's epilogue), max |skip| (its own scalar, max-combined))
        ca = _amax_slot(x.device) if sa is not None else None
        _convt_k2s2_fwd(lib(), x, ldx, w, b, base.data_ptr(), base.shape[-1], ca)
        if sa is not None:
            _measure_amax(sa, 1, 1, 1, ca)
            _set_amax(base, ca)
        ctx.save_for_backward(x, w)
        ctx.geom = (Cout, ldx, b is not None)
        return base

    @staticmethod
    def backward(ctx, dcat):
        x, w = ctx.saved_tensors
        Cout, ldx, has_b = ctx.geom
        dcat, ldd = cl_view(_like(dcat, x), "conv_transpose3d grad")
        return _convt_k2s2_bwd(lib(), x, ldx, dcat, ldd, w, has_b, ctx.needs_input_grad[0],
                               ctx.needs_input_grad[1] or (has_b and ctx.needs_input_grad[2])) + (dcat[..., Cout:],)


def conv_transpose3d_k2s2_cat(x, weight, bias, skip):
    return _ConvT3dK2S2Cat.apply(x, weight, bias, skip)


class _ConvT3dAdjoint(Function):
    """nn.ConvTranspose3d with kernel_size = stride = k, no padding (csrnet.py:121-137 uses k = 4), computed as the
    adjoint of the Conv3d with the same weight tensor: forward = that conv's dgrad, input gradient = its forward,
    weight gradient = its wgrad with the operands swapped.  (Cin, Cout, k, k, k) of the transposed conv IS the
    (Cout_c, Cin_c, k, k, k) layout of the conv, so no repacking is involved."""

    @staticmethod
    def forward(ctx, x, w, b, k):
        x, ldx = cl_view(x, "conv_transpose3d input", allow_bf16=False)
        N, D, H, W, Cin = x.shape
        if w.shape[0] != Cin or tuple(w.shape[2:]) != (k, k, k):
            raise Mi355SegError(f"conv_transpose3d: weight {tuple(w.shape)} does not match input channels {Cin} / kernel {k}")
        w = w.contiguous()
        Cout = w.shape[1]
        g = _ConvGeom(N, k * D, k * H, k * W, Cout, Cin, k, k, 0)             # the adjoint conv: Cout -> Cin channels, stride k
        y = torch.empty((N, k * D, k * H, k * W, Cout), dtype=x.dtype, device=x.device)
        L = lib()
        ws = workspace(g.ws_bytes(L, x.dtype), x.device)
        _conv_dgrad(L, g, x, ldx, w, y, Cout, ws)
        if b is not None:
            L.call("mi355seg_add_bias_f32", _p(y), Cout, _p(b), y.numel() // Cout, Cout, _stream())
        ctx.save_for_backward(x, w)
        ctx.cfg = (g, ldx, b is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        g, ldx, has_b = ctx.cfg
        dy, lddy = cl_view(dy, "conv_transpose3d grad")
        L = lib()
        ws = workspace(g.ws_bytes(L, x.dtype), x.device)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
            _conv_fwd(L, g, dy, lddy, w, None, dx, g.Cout, ws)
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(w)
            _conv_wgrad(L, g, x, ldx, dy, lddy, dw, None, ws)
        if has_b and ctx.needs_input_grad[2]:
            cws = workspace(L.query("mi355seg_norm_ws_bytes", g.rows_in, 1, g.Cin), x.device)
            db = torch.empty(g.Cin, dtype=x.dtype, device=x.device)
            L.call("mi355seg_colsum_f32", _p(dy), lddy, g.rows_in, g.Cin, _p(db), _p(cws), cws.numel(), _stream())
        return dx, dw, db, None


def conv_transpose3d_adjoint(x, weight, bias, k):
    return _ConvT3dAdjoint.apply(x, weight, bias, int(k))


def conv_transpose3d_k2s2(x, weight, bias=None):
    """nn.ConvTranspose3d(kernel_size=2, stride=2) on a channel-last tensor."""
    return _ConvT3dK2S2.apply(x, weight, bias)


# ----------------------------------------------------------------------------- norm + activation
class _NormAct(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, res, running_mean, running_var, training, momentum, eps, act, slope, instance, left_pad=0):
        # left_pad > 0: the result is the RIGHT channel slice of a buffer with left_pad free channels on its left, which a later node
        # fills (conv_in_act(..., cat_right=)): the skip concatenation of residual_unet3d.py:174-209 without the copies
        x, ldx = cl_view(x, "norm input")
        C = x.shape[-1]
        rows, groups = _norm_rows(x.shape, instance)
        L = lib()
        ws = _norm_ws(L, rows, groups, C, x.device)
        res, ldres = _opt_view(res, "norm residual")
        if training or instance:
            upd = training and (running_mean is not None) and not instance
            mean, rstd = _batch_stats(L, x, ldx, rows, groups, C, eps, running_mean if upd else None, running_var if upd else None, momentum, ws)
        else:
            mean, rstd = _running_stats(L, running_mean, running_var, eps, C)
        _, y, ldy = _concat_out(x.shape[:4], left_pad, C, x.dtype, x.device)
        _norm_act_fwd(L, x, ldx, mean, rstd, gamma, beta, (res, ldres), y.data_ptr(), ldy, rows, groups, C, act, slope)
        ctx.save_for_backward(x, mean, rstd, gamma, beta, res)
        ctx.cfg = (ldx, ldres, rows, groups, C, act, slope, bool(training or instance))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, gamma, beta, res = ctx.saved_tensors
        ldx, ldres, rows, groups, C, act, slope, batch_stats = ctx.cfg
        if not batch_stats:
            raise Mi355SegError(_EVAL_BN_BACKWARD)
        dy, lddy = cl_view(_like(dy, x), "norm grad")
        L = lib()
        ws = _norm_ws(L, rows, groups, C, x.device)
        dx, dgamma, dbeta, dres, _ = _norm_act_bwd(L, dy, lddy, x, ldx, mean, rstd, gamma, beta, (res, ldres), rows, groups, C, act, slope, ws)
        return dx, dgamma, dbeta, dres, None, None, None, None, None, None, None, None, None


def batch_norm_act(x, gamma, beta, running_mean, running_var, training, momentum=0.1, eps=1e-5,
                   act=ACT_NONE, slope=0.01, residual=None):
    """act(BatchNorm3d(x) [+ residual]); training mode updates running stats in place."""
    return _NormAct.apply(x, gamma, beta, residual, running_mean, running_var, bool(training), float(momentum),
                          float(eps), int(act), float(slope), False, 0)


def instance_norm_act(x, eps=1e-5, act=ACT_NONE, slope=0.01, left_pad=0):
    """act(InstanceNorm3d(x)) with affine=False, track_running_stats=False.  ``left_pad``: see _NormAct (the result is the right channel
    slice of a concat buffer)."""
    return _NormAct.apply(x, None, None, None, None, None, True, 0.0, float(eps), int(act), float(slope), True, int(left_pad))


class _ConvBnAct(Function):
    """act(BatchNorm3d(conv3d(x))) as one autograd node: the batch statistics come out of the convolution's
    epilogue (no separate pass over y) and the convolution's bias gradient comes out of the BatchNorm backward
    pass (no separate pass over dy).  Training mode only updates running stats exactly as nn.BatchNorm3d."""

    @staticmethod
    def forward(ctx, x, w, b, gamma, beta, rmean, rvar, stride, pad, training, momentum, eps, act, slope, left_pad, inference=False, fork=False, cat_right=None):
        # cat_right (training): a tensor that IS the right channel slice of a concat buffer with exactly Cout free channels on its left
        # (instance_norm_act / activation_fork(..., left_pad=Cout)): the activation is written into those channels and the whole buffer
        # is returned -- cat((act(norm(conv(x))), cat_right), channels) without the two copies
        # fork (training): the result is (act(bn(conv(x))), x) -- x also continues unchanged (a residual block's input, vnet3d.py:61-104), and
        # the backward sums the pass-through's gradient into the input gradient it computes (bf16: in that kernel's epilogue)
        xa_in = _get_amax(x)
        x_arg = x
        x, ldx = cl_view(x, "conv3d input")
        g, w = _conv_geom(x, w, stride, pad, "conv3d")
        Cout, rows = g.Cout, g.rows_out
        dev = x.device
        L = lib()
        ws = workspace(_conv_norm_ws(L, g, x.dtype, rows, Cout), dev)
        if (not training) and inference and x.data_ptr() % 16 == 0 and \
                L.query("mi355seg_conv3d_fused_supported_" + _sfx(x), *g, ldx, left_pad + Cout):
            # inference (model.eval() under no_grad, predict.py:79-81,133): eval-mode BatchNorm folded into the packed weights and
            # the bias slot, the activation in the convolution's epilogue -- one pass, nothing saved for a backward
            return _conv_fwd_folded(L, g, x, ldx, w, b, gamma, beta, rmean, rvar, eps, act, slope, left_pad, ws)
        if training:                              # f16x3: operand maxima ride along (this layer's input, weights, and its output for the next layer)
            y, sums, lay = _conv_stats_fwd(L, g, x, ldx, w, b, ws, xa_in)
            mean, rstd = _stats_from_sums(L, sums, rows, Cout, eps, rmean, rvar, momentum)
        else:
            y, lay = torch.empty(g.out_shape, dtype=x.dtype, device=dev), _ConvLayer(g, ldx, b is not None)
            _conv_fwd(L, g, x, ldx, w, b, y, Cout, ws)
            mean, rstd = _running_stats(L, rmean, rvar, eps, Cout)
        ctx.cat = 0
        if cat_right is not None:
            full = None if left_pad else _concat_base(cat_right, Cout, g.out_shape[:4], x.dtype)
            if full is None:
                raise Mi355SegError("conv_bn_act: `cat_right` is not the right channel slice of a matching concat buffer")
            a, lda = full[..., :Cout], full.shape[-1]
            ctx.cat = lda - Cout
        else:
            # left_pad: the activation lands in the RIGHT channel slice of a wider buffer whose left `left_pad` channels a later
            # up-convolution fills (conv_transpose3d_k2s2_cat): the skip concatenation then costs no copy
            full, a, lda = _concat_out(g.out_shape[:4], left_pad, Cout, x.dtype, dev)
        lay.out_amax = _amax_slot(dev) if training and _takes_amax(x) else None
        _norm_act_fwd(L, y, Cout, mean, rstd, gamma, beta, _NO_RES, a.data_ptr(), lda, rows, 1, Cout, act, slope, lay.out_amax)
        if not ctx.cat:
            _set_amax(a, lay.out_amax)
        ctx.save_for_backward(x, w, y, mean, rstd, gamma, beta)
        ctx.cfg = (lay, act, slope, bool(training))
        if fork:
            ctx.set_materialize_grads(False)
            return a, x_arg.view_as(x_arg)
        if ctx.cat:
            return full
        return a

    @staticmethod
    def backward(ctx, da, dpass=None):
        x, w, y, mean, rstd, gamma, beta = ctx.saved_tensors
        lay, act, slope, training = ctx.cfg
        g, Cout = lay.g, lay.g.Cout
        if not training:
            raise Mi355SegError(_EVAL_BN_BACKWARD)
        if da is None:                       # (fork, only the pass-through was used)
            return _grads(_CONV_BN_ACT_ARGS, x=dpass)
        add = None if dpass is None else cl_view(_like(dpass, x), "pass-through grad")
        dcat = None
        if ctx.cat:                          # da is the gradient of the whole concat buffer: ours is its left slice, the right one goes back to cat_right
            da = _like(da, x)
            dcat, da = da[..., Cout:], da[..., :Cout]
        da, ldda = cl_view(_like(da, x), "conv+norm grad")
        L = lib()
        ws = workspace(_conv_norm_ws(L, g, x.dtype, g.rows_out, Cout), x.device)
        dya = _amax_slot(x.device) if lay.amax is not None else None       # f16x3: max |dy| from the kernel that writes dy
        dy, dgamma, dbeta, db = _layer_norm_act_bwd(L, lay, da, ldda, y, mean, rstd, gamma, beta, act, slope, ws, dya)
        # (the pass-through's gradient is summed into the input gradient; an input that needs none hands it on as it is)
        dx, dw, _ = _conv_grads(L, lay, dy, Cout, x, w, ctx.needs_input_grad[0], ctx.needs_input_grad[1], ws, dya, add)
        if dx is None and add is not None:
            dx = add[0]
        return _grads(_CONV_BN_ACT_ARGS, x=dx, w=dw, b=db, gamma=dgamma, beta=dbeta, cat_right=dcat)


_CONV_BN_ACT_ARGS = ("x", "w", "b", "gamma", "beta", "rmean", "rvar", "stride", "pad", "training", "momentum", "eps", "act", "slope", "left_pad",
                     "inference", "fork", "cat_right")


def conv_in_act(x, conv, norm, act=ACT_NONE, slope=0.01, cat_right=None):
    """act(InstanceNorm3d(conv(x))) (residual_unet3d.py:82-107: conv_norm_lrelu and the tail of norm_lrelu_upscale_conv_norm_lrelu;
    affine=False, no running statistics).  With ONE sample per batch -- cfg 4 -- the per-(sample, channel) statistics are per-channel
    statistics over the whole tensor, i.e. exactly what the convolution's epilogue already reduces for BatchNorm: the node of
    conv_bn_act without affine parameters and buffers (no separate statistics pass over y).  N > 1: convolution, then the
    instance-norm node."""
    g = _module_geom(x, conv, "conv_in_act")
    if g.N != 1 or norm.affine or norm.track_running_stats or not torch.is_grad_enabled():
        a = norm.forward_act(conv(x), act, slope)
        return a if cat_right is None else cat_channels(a, cat_right)
    # cat_right: cat((result, cat_right), channels) -- written in place when cat_right is the right slice of a matching concat buffer
    # (instance_norm_act / activation_fork(..., left_pad=)), by two slice copies otherwise
    inplace = cat_right is not None and _concat_base(cat_right, g.Cout, g.out_shape[:4], x.dtype) is not None
    out = _ConvBnAct.apply(x, conv.weight, conv.bias, None, None, None, None, g.stride, g.pad, True, 0.0, float(norm.eps),
                           int(act), float(slope), 0, False, False, cat_right if inplace else None)
    return out if (cat_right is None or inplace) else cat_channels(out, cat_right)


def conv_bn_act(x, conv, bn, act=ACT_NONE, slope=0.01, left_pad=0, fork=False):
    """act(bn(conv(x))) for a layers.Conv3d / layers.BatchNorm3d pair (module objects carry the parameters).  ``fork`` (training mode):
    returns (act(bn(conv(x))), x) -- x continues unchanged beside the convolution (the input of a residual block) and the node's backward
    adds the pass-through's gradient to the input gradient it computes instead of leaving the sum to autograd."""
    if bn.momentum is None or not bn.affine or not bn.track_running_stats:
        raise NotImplementedError("conv_bn_act: BatchNorm3d must be affine with running statistics and a momentum")
    stride, pad = _module_stride_pad(conv, "conv_bn_act")         # (checked before the counter moves: a refused call changes nothing)
    if bn.training:
        bump_counter(bn)
    # eval mode under torch.no_grad() (predict.py:79-81,133) takes the folded one-pass form where the layer has one
    forked = bool(fork) and bn.training and torch.is_grad_enabled()
    out = _ConvBnAct.apply(x, conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, stride, pad,
                           bool(bn.training), float(bn.momentum), float(bn.eps), int(act), float(slope), int(left_pad),
                           not torch.is_grad_enabled(), forked)
    return (out, x) if (fork and not forked) else out


class _DoubleConvBnAct(Function):
    """act(BN2(conv2(act(BN1(conv1(x)))))) -- the double-conv block of unet3d.py:73-104 -- as ONE autograd node (training mode, fp32
    tensors).  Forward is the two fused layers of _ConvBnAct back to back.  Because the activation between the two convolutions
    has exactly one consumer here, the backward can let conv2's input-gradient kernel reduce BN1's two backward column sums in its
    epilogue (_conv_dgrad_bnsums) instead of a separate pass over d(act) and y1."""

    @staticmethod
    def forward(ctx, x, w1, b1, g1, be1, rm1, rv1, w2, b2, g2, be2, rm2, rv2, geo1, geo2, mom1, eps1, mom2, eps2, act, slope, left_pad,
                wh=None, bh=None, pool=False):
        """wh / bh: the 1x1x1 output head behind the block (unet3d.py:46-48,71).  The node then returns the head's LOGITS
        (_bn_act_head_fwd); the block's activation is never written.
        pool: the MaxPool3d(2, 2) behind an encoder block (unet3d.py:51-58).  The node then returns (pooled, activation)
        (_bn_act_pool_fwd), and the backward forms d(activation) = d(skip) + pool_backward(d(pooled)) inside the norm backward."""
        xa_in = _get_amax(x)
        x, ldx = cl_view(x, "conv3d input")
        L = lib()
        dev = x.device
        ax = _takes_amax(x)           # f16x3: operand maxima ride along
        cg1, w1 = _conv_geom(x, w1, *geo1, "conv3d")
        cg2, w2 = _conv_geom(cg1.out_shape, w2, *geo2, "conv3d")
        C1, C2, rows1, rows2 = cg1.Cout, cg2.Cout, cg1.rows_out, cg2.rows_out
        if wh is not None:
            wh = wh.contiguous()
        # norm1 + activation as a PROLOGUE of conv2 (its forward and its weight gradient read conv1's raw output): where both run the
        # f16x3 kernels the activation between the two convolutions is never written
        fuse1 = ax and not os.environ.get("MI355SEG_NO_PRO_FUSION") and L.query("mi355seg_conv3d_pro_supported_f32", *cg2, act) != 0
        # layer 1: convolution + statistics, then either the folded norm for conv2's prologue or the activation itself
        ws = workspace(_conv_norm_ws(L, cg1, x.dtype, rows1, C1), dev)
        a1 = al1 = bl1 = None
        if fuse1:
            ya1 = _amax_slot(dev)
            y1, sums1, lay1 = _conv_stats_fwd(L, cg1, x, ldx, w1, b1, ws, xa_in, ya=ya1)
            mean1, rstd1, al1, bl1, lay1.out_amax = _norm_fold(L, sums1, rows1, C1, eps1, g1, be1, act, rm1, rv1, mom1, ya1)
        else:
            y1, sums1, lay1 = _conv_stats_fwd(L, cg1, x, ldx, w1, b1, ws, xa_in)
            mean1, rstd1 = _stats_from_sums(L, sums1, rows1, C1, eps1, rm1, rv1, mom1)
            a1 = torch.empty(cg1.out_shape, dtype=x.dtype, device=dev)
            lay1.out_amax = _amax_slot(dev) if ax else None
            _norm_act_fwd(L, y1, C1, mean1, rstd1, g1, be1, _NO_RES, a1.data_ptr(), C1, rows1, 1, C1, act, slope, lay1.out_amax)
        # layer 2: convolution (of the activation, or of y1 through the prologue) + statistics, then norm + activation (+ head / pool)
        ws = workspace(_conv_norm_ws(L, cg2, x.dtype, rows2, C2), dev)
        if fuse1:
            y2, sums2, lay2 = _conv_stats_fwd(L, cg2, y1, C1, w2, b2, ws, lay1.out_amax, pro=(al1, bl1, act, slope))
        else:
            y2, sums2, lay2 = _conv_stats_fwd(L, cg2, a1, C1, w2, b2, ws, lay1.out_amax)
        mean2, rstd2 = _stats_from_sums(L, sums2, rows2, C2, eps2, rm2, rv2, mom2)
        idx = None
        if wh is not None:
            out = _bn_act_head_fwd(L, y2, mean2, rstd2, g2, be2, act, slope, wh, bh)
        else:
            aa = lay2.out_amax = _amax_slot(dev) if ax else None
            if pool:                         # max |max_pool(a)| <= max |a| (equal for the non-negative outputs of a ReLU)
                a2, pooled, idx = _bn_act_pool_fwd(L, y2, mean2, rstd2, g2, be2, act, slope, left_pad, aa)
                out = _set_amax(pooled, aa), _set_amax(a2, aa)
            else:
                _, a2, lda2 = _concat_out(cg2.out_shape[:4], left_pad, C2, x.dtype, dev)
                _norm_act_fwd(L, y2, C2, mean2, rstd2, g2, be2, _NO_RES, a2.data_ptr(), lda2, rows2, 1, C2, act, slope, aa)
                out = _set_amax(a2, aa)
        ctx.save_for_backward(x, w1, y1, mean1, rstd1, g1, be1, a1, al1, bl1, w2, y2, mean2, rstd2, g2, be2, wh, idx)
        ctx.cfg = (lay1, lay2, act, slope)
        # the math the prologue form ran under: the backward runs under it too (_conv_wgrad_pro exists under no other)
        ctx.math = L.query("mi355seg_get_conv_math") if fuse1 else None
        ctx.head_bias = wh is not None and bh is not None
        return out

    @staticmethod
    def backward(ctx, da2, dskip=None):
        """A prologue-fused block kept no activation between its convolutions, so its backward cannot follow a set_conv_math that came
        after the forward: ALL of it runs under the forward's math (the maxima in the layer records are that math's), and the policy
        found is put back."""
        now = lib().query("mi355seg_get_conv_math") if ctx.math is not None else None
        if now == ctx.math:
            return _DoubleConvBnAct._backward(ctx, da2, dskip)
        lib().call("mi355seg_set_conv_math", ctx.math)
        try:
            return _DoubleConvBnAct._backward(ctx, da2, dskip)
        finally:
            lib().call("mi355seg_set_conv_math", now)

    @staticmethod
    def _backward(ctx, da2, dskip):
        x, w1, y1, mean1, rstd1, g1, be1, a1, al1, bl1, w2, y2, mean2, rstd2, g2, be2, wh, idx = ctx.saved_tensors
        lay1, lay2, act, slope = ctx.cfg
        cg1, cg2 = lay1.g, lay2.g
        C1, C2 = cg1.Cout, cg2.Cout
        L = lib()
        dev = x.device
        if da2 is not None:
            da2, ldda2 = cl_view(_like(da2, x), "conv+norm grad")
        ws = workspace(max(_conv_norm_ws(L, cg1, x.dtype, cg1.rows_out, C1), _conv_norm_ws(L, cg2, y1.dtype, cg2.rows_out, C2),
                           L.query("mi355seg_bn_act_head_ws_bytes", C2, wh.shape[0]) if wh is not None else 0,
                           L.query("mi355seg_bn_act_pool_ws_bytes", C2) if idx is not None else 0), dev)
        # f16x3: the two gradients d(conv output) take their maxima from the norm-backward kernels that write them
        dya2 = _amax_slot(dev) if lay2.amax is not None else None
        dya1 = _amax_slot(dev) if lay1.amax is not None else None
        xa2, wa2 = lay2.amax or (None, None)
        # layer 2: norm + activation backward (its dx column sums are conv2's bias gradient); da2 is d(pooled) beside the skip connection's
        # gradient behind a max-pool, d(logits) behind the head
        dwh = dbh = None
        if idx is not None:
            dy2, dg2, dbe2, db2 = _bn_act_pool_bwd(L, dskip, da2, idx, y2, mean2, rstd2, g2, be2, act, slope, lay2.has_bias, ws, dya2)
        elif wh is not None:
            dy2, dg2, dbe2, db2, dwh, dbh = _bn_act_head_bwd(L, da2, ldda2, y2, mean2, rstd2, g2, be2, act, slope, wh, ctx.head_bias,
                                                            lay2.has_bias, ws, dya2)
        else:
            dy2, dg2, dbe2, db2 = _layer_norm_act_bwd(L, lay2, da2, ldda2, y2, mean2, rstd2, g2, be2, act, slope, ws, dya2)
        # conv2: its input gradient = d(act1) with BN1's two column sums, then its weight gradient against act1 (written, or the prologue's)
        da1, s12, dg1, dbe1 = _conv_dgrad_bnsums(L, cg2, dy2, C2, w2, y1, mean1, rstd1, g1, be1, act, slope, ws, dya2, wa2)
        if al1 is not None:
            dw2 = _conv_wgrad_pro(L, cg2, dy2, C2, y1, C1, al1, bl1, act, slope, w2, ws, dya2, xa2)
        else:
            _, dw2, _ = _conv_grads(L, lay2, dy2, C2, a1, w2, False, True, ws, dya2)
        del dy2
        grads = dict(w2=dw2, b2=db2, g2=dg2, be2=dbe2, g1=dg1, be1=dbe1, wh=dwh, bh=dbh)
        # the 1-channel stem whose input needs no gradient (enc1conv1, unet3d.py:80-89): no apply pass, no d(conv1 output) (537 MB at 128^3)
        if not ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and cg1.Cin == 1 and \
                L.query("mi355seg_stem_wgrad_bnbwd_supported_f32", *cg1) != 0:
            dw1, db1 = _stem_wgrad_bnbwd(L, lay1, da1, y1, mean1, rstd1, g1, be1, act, slope, s12, x, w1, ws)
            return _grads(_DOUBLE_CONV_BN_ACT_ARGS, w1=dw1, b1=db1, **grads)
        # layer 1: the apply half of the norm backward (+ conv1's bias gradient), then conv1's gradients
        dy1, db1 = _norm_act_bwd_apply(L, da1, C1, y1, mean1, rstd1, g1, be1, s12, act, slope, ws, lay1.has_bias, dya1)
        del da1
        dx, dw1, _ = _conv_grads(L, lay1, dy1, C1, x, w1, ctx.needs_input_grad[0], ctx.needs_input_grad[1], ws, dya1)
        return _grads(_DOUBLE_CONV_BN_ACT_ARGS, x=dx, w1=dw1, b1=db1, **grads)


_DOUBLE_CONV_BN_ACT_ARGS = ("x", "w1", "b1", "g1", "be1", "rm1", "rv1", "w2", "b2", "g2", "be2", "rm2", "rv2", "geo1", "geo2", "mom1", "eps1", "mom2", "eps2",
                            "act", "slope", "left_pad", "wh", "bh", "pool")


def double_conv_bn_act(x, conv1, bn1, conv2, bn2, act=ACT_NONE, slope=0.01, left_pad=0, head=None, pool=False):
    """act(bn2(conv2(act(bn1(conv1(x)))))): training mode on fp32 tensors runs as one autograd node (_DoubleConvBnAct), everything
    else as two conv_bn_act layers.  ``head`` (a layers.Conv3d with kernel_size 1: the output head behind the LAST block,
    unet3d.py:46-48,71): the result is ``head(block(x))``; in the fused node norm2 + activation + head are one kernel."""
    g1 = _module_geom(x, conv1, "double_conv_bn_act")           # (checked before a counter moves: a refused call changes nothing)
    g2 = _module_geom(g1.out_shape, conv2, "double_conv_bn_act")
    fused = bn1.training and bn2.training and torch.is_grad_enabled() and compute_dtype() == torch.float32 and x.dtype == torch.float32
    for bn in (bn1, bn2):
        fused = fused and bn.momentum is not None and bn.affine and bn.track_running_stats
    if pool and head is not None:
        raise Mi355SegError("double_conv_bn_act: a block feeds either the output head or a max-pool, not both")
    if not fused:
        a = conv_bn_act(conv_bn_act(x, conv1, bn1, act, slope), conv2, bn2, act, slope, left_pad=left_pad)
        if pool:
            return max_pool3d_2x_and_skip(a)
        return a if head is None else head(a)
    head_fused = False
    if head is not None:
        hk, hs, hp = _iso(head.kernel_size, "kernel_size"), _iso(head.stride, "stride"), _iso(head.padding, "padding")
        head_fused = (hk, hs, hp) == (1, 1, 0) and head.groups == 1 and head.weight.dtype == torch.float32 and left_pad == 0 and \
            head.in_channels == g2.Cout and \
            lib().query("mi355seg_bn_act_head_supported_f32", 1, g2.Cout, head.out_channels, g2.Cout) != 0
    bump_counter(bn1)
    bump_counter(bn2)
    args = (x, conv1.weight, conv1.bias, bn1.weight, bn1.bias, bn1.running_mean, bn1.running_var,
            conv2.weight, conv2.bias, bn2.weight, bn2.bias, bn2.running_mean, bn2.running_var,
            (g1.stride, g1.pad), (g2.stride, g2.pad), float(bn1.momentum), float(bn1.eps), float(bn2.momentum), float(bn2.eps),
            int(act), float(slope), int(left_pad))
    if head_fused:
        return _DoubleConvBnAct.apply(*args, head.weight, head.bias)
    if pool:
        # ``pool``: (max_pool3d_2x(block(x)), block(x)) -- in the fused node norm2 + activation + pooling are one kernel and the pool's
        # backward rides in the norm backward; geometry the fused kernels do not take (odd extents) pools separately
        # (the fused kernels address the skip slice -- full[..., left_pad:] -- and its gradient by 16-byte quads: left_pad and the buffer's
        # channel pitch must be multiples of four, else the separate pool node below takes the shape)
        if left_pad % 4 == 0 and (left_pad + g2.Cout) % 4 == 0 and \
                lib().query("mi355seg_bn_act_pool_supported_f32", *g2.out_shape, g2.Cout) != 0:
            return _DoubleConvBnAct.apply(*args, None, None, True)
        return max_pool3d_2x_and_skip(_DoubleConvBnAct.apply(*args))
    a = _DoubleConvBnAct.apply(*args)
    return a if head is None else head(a)


class _Act(Function):
    @staticmethod
    def forward(ctx, x, res, act, slope):
        x, ldx = cl_view(x, "activation input")
        N, D, H, W, C = x.shape
        res, ldres = _opt_view(res, "activation residual")
        y = torch.empty((N, D, H, W, C), dtype=x.dtype, device=x.device)
        rows = N * D * H * W
        lib().call("mi355seg_act_fwd_" + _sfx(x), _p(x), ldx, _p(res), ldres, _p(y), C, rows, C, act, slope, _stream())
        ctx.cfg = (ldx, ldres, rows, C, act, slope)
        ctx.has_res = res is not None
        ctx.x_dtype = x.dtype
        if act != ACT_NONE:                  # a plain sum needs nothing for its backward
            ctx.save_for_backward(x, res)
        return y

    @staticmethod
    def backward(ctx, dy):
        ldx, ldres, rows, C, act, slope = ctx.cfg
        if act == ACT_NONE:                  # x + residual: the gradient of both is dy itself -- no kernel, no copy
            g = dy if dy.dtype == ctx.x_dtype else dy.to(ctx.x_dtype)
            return g, (g if ctx.has_res else None), None, None
        x, res = ctx.saved_tensors
        dy, lddy = cl_view(_like(dy, x), "activation grad")
        dx = _act_bwd(dy, lddy, x, ldx, (res, ldres), rows, C, act, slope)
        return dx, (dx if res is not None else None), None, None


def activation(x, act, slope=0.01, residual=None):
    """act(x [+ residual]) for ReLU / ELU / LeakyReLU."""
    return _Act.apply(x, residual, int(act), float(slope))


class _ActFork(Function):
    """(act(x), x): the activation of a tensor that ALSO continues unchanged (a residual fork, residual_unet3d.py:110-121).  The backward forms
    d(x) = d(pass-through) + d(act) * act'(x) in one pass (mi355seg_act_bwd_add_*) -- autograd would run the activation's backward and then
    add the two gradients with a kernel of its own."""

    @staticmethod
    def forward(ctx, x, act, slope, left_pad=0):
        xv, ldx = cl_view(x, "activation input")
        N, D, H, W, C = xv.shape
        # left_pad: the activation is the RIGHT channel slice of a concat buffer a later node fills on the left
        _, y, ldy = _concat_out((N, D, H, W), left_pad, C, xv.dtype, xv.device)
        rows = N * D * H * W
        lib().call("mi355seg_act_fwd_" + _sfx(xv), _p(xv), ldx, None, 0, y.data_ptr(), ldy, rows, C, act, slope, _stream())
        ctx.cfg = (ldx, rows, C, act, slope)
        ctx.save_for_backward(xv)
        ctx.set_materialize_grads(False)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dpass):
        ldx, rows, C, act, slope = ctx.cfg
        (x,) = ctx.saved_tensors
        if dy is None:
            return dpass, None, None, None
        dy, lddy = cl_view(_like(dy, x), "activation grad")
        add = _opt_view(None if dpass is None else _like(dpass, x), "pass-through grad")
        return _act_bwd(dy, lddy, x, ldx, _NO_RES, rows, C, act, slope, add), None, None, None


def activation_fork(x, act, slope=0.01, left_pad=0):
    """(act(x), x) for a tensor that feeds an activation and continues unchanged; see _ActFork.  ``left_pad``: act(x) is the right channel
    slice of a concat buffer with that many free channels on its left."""
    return _ActFork.apply(x, int(act), float(slope), int(left_pad))


class _PReLU(Function):
    @staticmethod
    def forward(ctx, x, res, slope):
        x, ldx = cl_view(x, "prelu input")
        N, D, H, W, C = x.shape
        res, ldres = _opt_view(res, "prelu residual")
        slope = slope.contiguous().to(torch.float32)
        if slope.numel() != C:
            raise Mi355SegError(f"prelu: {slope.numel()} slopes for {C} channels")
        y = torch.empty((N, D, H, W, C), dtype=x.dtype, device=x.device)
        rows = N * D * H * W
        lib().call("mi355seg_prelu_fwd_" + _sfx(x), _p(x), ldx, _p(res), ldres, _p(slope), _p(y), C, rows, C, _stream())
        ctx.save_for_backward(x, res, slope)
        ctx.cfg = (ldx, ldres, rows, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, res, slope = ctx.saved_tensors
        ldx, ldres, rows, C = ctx.cfg
        dy, lddy = cl_view(_like(dy, x), "prelu grad")
        L = lib()
        dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        dslope = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = _norm_ws(L, rows, 1, C, x.device)
        L.call("mi355seg_prelu_bwd_" + _sfx(x), _p(dy), lddy, _p(x), ldx, _p(res), ldres, _p(slope), _p(dx), C, _p(dslope), rows, C,
               _p(ws), ws.numel(), _stream())
        return dx, (dx if res is not None else None), dslope


def prelu(x, weight, residual=None):
    """nn.PReLU(C)(x [+ residual]) with one learnable slope per channel (vnet3d.py:14-18, elu=False)."""
    return _PReLU.apply(x, residual, weight)


class _ScaleChannels(Function):
    @staticmethod
    def forward(ctx, x, scale):
        x, ldx = cl_view(x, "dropout input")
        N, D, H, W, C = x.shape
        scale = scale.contiguous().to(torch.float32)
        if scale.numel() != N * C:
            raise Mi355SegError(f"scale_channels: scale must hold N*C = {N * C} values, got {scale.numel()}")
        y = torch.empty((N, D, H, W, C), dtype=x.dtype, device=x.device)
        lib().call("mi355seg_scale_channels_" + _sfx(x), _p(x), ldx, _p(scale), _p(y), C, D * H * W, N, C, _stream())
        ctx.save_for_backward(scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        (scale,) = ctx.saved_tensors
        dy, lddy = cl_view(dy, "dropout grad")
        N, D, H, W, C = dy.shape
        dx = torch.empty((N, D, H, W, C), dtype=dy.dtype, device=dy.device)
        lib().call("mi355seg_scale_channels_" + _sfx(dy), _p(dy), lddy, _p(scale), _p(dx), C, D * H * W, N, C, _stream())
        return dx, None


def scale_channels(x, scale):
    """y[n,...,c] = x[n,...,c] * scale[n,c] -- the arithmetic of nn.Dropout3d given its mask."""
    return _ScaleChannels.apply(x, scale)


# ----------------------------------------------------------------------------- pool / upsample
def _pool_forward(ctx, x):
    """The forward the two pooling nodes share: the pooled tensor; the argmax codes and the input's shape are kept for the backward."""
    x, ldx = cl_view(x, "max_pool3d input")
    y, idx = _maxpool2_fwd(x, ldx)
    ctx.save_for_backward(idx)
    ctx.geom = tuple(x.shape)
    return y


class _MaxPool2(Function):
    @staticmethod
    def forward(ctx, x):
        xa = _get_amax(x)
        return _set_amax(_pool_forward(ctx, x), xa)             # max |max_pool(x)| <= max |x|

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        return _maxpool2_bwd(*cl_view(dy, "max_pool3d grad"), idx, ctx.geom)


class _PoolAndSkip(Function):
    """(max_pool3d_2x(x), x): the pooled tensor for the next level and x itself for the skip connection, as ONE
    autograd node so that the two incoming gradients are summed inside the pool-backward kernel."""

    @staticmethod
    def forward(ctx, x):
        y = _pool_forward(ctx, x)
        skip = x.view_as(x)
        xa = _get_amax(x)
        if xa is not None:              # max |max_pool(x)| <= max |x| (equal for the non-negative outputs of a ReLU)
            _set_amax(y, xa)
            _set_amax(skip, xa)
        return y, skip

    @staticmethod
    def backward(ctx, dy, dskip):
        (idx,) = ctx.saved_tensors
        dy, lddy = cl_view(dy, "max_pool3d grad")
        return _maxpool2_bwd(dy, lddy, idx, ctx.geom, cl_view(dskip, "skip grad"))


def max_pool3d_2x_and_skip(x):
    return _PoolAndSkip.apply(x)


def max_pool3d_2x(x):
    """nn.MaxPool3d(kernel_size=2, stride=2)."""
    return _MaxPool2.apply(x)


class _Upsample2(Function):
    @staticmethod
    def forward(ctx, x):
        x, ldx = cl_view(x, "upsample input")
        N, D, H, W, C = x.shape
        y = torch.empty((N, 2 * D, 2 * H, 2 * W, C), dtype=x.dtype, device=x.device)
        lib().call("mi355seg_upsample2_fwd_" + _sfx(x), _p(x), ldx, _p(y), C, N, D, H, W, C, _stream())
        return y

    @staticmethod
    def backward(ctx, dy):
        return _upsample2_bwd(*cl_view(dy, "upsample grad"))


def upsample_nearest_2x(x):
    """nn.Upsample(scale_factor=2, mode='nearest')."""
    return _Upsample2.apply(x)


# ----------------------------------------------------------------------------- losses / metric kernels
class _BCEWithLogits(Function):
    @staticmethod
    def forward(ctx, logits, target):
        _require_cuda(logits, "bce_with_logits input")
        logits = aligned_contiguous(logits)
        target = aligned_contiguous(target.to(torch.float32))
        if logits.shape != target.shape:
            raise ValueError(f"Target size ({tuple(target.shape)}) must be the same as input size ({tuple(logits.shape)})")
        L = lib()
        ws = workspace(L.query("mi355seg_loss_ws_bytes", logits.numel()), logits.device)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        L.call("mi355seg_bce_logits_fwd_f32", _p(logits), _p(target), logits.numel(), _p(loss), _p(ws), ws.numel(), _stream())
        ctx.save_for_backward(logits, target)
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, target = ctx.saved_tensors
        g = g.contiguous().to(torch.float32)
        d = torch.empty_like(logits)
        lib().call("mi355seg_bce_logits_bwd_f32", _p(logits), _p(target), _p(g), logits.numel(), _p(d), _stream())
        return d, None


def bce_with_logits(logits, target):
    """nn.BCEWithLogitsLoss() (mean reduction)."""
    return _BCEWithLogits.apply(logits, target)


def argmax_channels(logits):
    """pred.argmax(dim=1, keepdim=True) on an NCDHW tensor -> int64 [N,1,D,H,W]."""
    _require_cuda(logits, "argmax input")
    logits = logits.contiguous()
    N, K = logits.shape[0], logits.shape[1]
    S = logits[0, 0].numel()
    mask = torch.empty((N, 1) + tuple(logits.shape[2:]), dtype=torch.int64, device=logits.device)
    lib().call("mi355seg_argmax_ch_f32", _p(logits), N, K, S, _p(mask), _stream())
    return mask


OVERLAP_MODES = ("crop", "average", "hann", "gaussian")     # sliding-window aggregation (predict.py); all but "crop" blend probabilities
MAX_AGGREGATE_CLASSES = 16
TTA_AXES = ("z", "y", "x")                                   # mirror test-time augmentation: flip code = 4 * z + 2 * y + 1 * x


def tta_flip_codes(axes=TTA_AXES):
    """The flip codes of mirror test-time augmentation over ``axes`` (a non-empty subset of TTA_AXES, no duplicates): the ascending
    tuple of every code 0..7 whose set bits (4 mirrors z, 2 mirrors y, 1 mirrors x) lie within the chosen axes.  The identity 0 is
    always first; there are 2, 4 or 8 codes."""
    axes = (axes,) if isinstance(axes, str) else tuple(axes)
    if not axes or any(a not in TTA_AXES for a in axes) or len(set(axes)) != len(axes):
        raise ValueError(f"tta_flip_codes: axes must be a non-empty subset of {TTA_AXES} without duplicates, got {axes!r}")
    mask = sum(4 >> TTA_AXES.index(a) for a in axes)
    return tuple(c for c in range(8) if c & ~mask == 0)


def _flip_code(flip, what):
    if isinstance(flip, bool) or not isinstance(flip, int) or not 0 <= flip <= 7:
        raise Mi355SegError(f"{what}: flip must be an integer in 0..7 (bit 2 mirrors z, bit 1 y, bit 0 x), got {flip!r}")
    return flip


def gather_patches(volume, table, first, count, patch, flip=0):
    """``count`` grid patches of ``volume`` [C, D, H, W] (fp32, GPU, contiguous), rows ``first`` .. of the int32 window ``table``
    [P, 9] on the device, as one batch [count, C, pd, ph, pw]; one launch.  ``flip`` (0..7: bit 2 mirrors z, bit 1 y, bit 0 x) reads
    every patch mirrored inside its window (mi355seg_gather_patches_flip_f32); 0 is mi355seg_gather_patches_f32."""
    flip = _flip_code(flip, "gather_patches")
    _require_cuda(volume, "gather_patches volume")
    if volume.dim() != 4 or volume.dtype != torch.float32 or not volume.is_contiguous():
        raise Mi355SegError(f"gather_patches: expected a contiguous float32 volume [C, D, H, W], got {volume.dtype} {tuple(volume.shape)}")
    if not table.is_cuda or table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != 9 or not table.is_contiguous():
        raise Mi355SegError("gather_patches: expected the contiguous int32 window table [P, 9] on the GPU")
    ps = (patch,) * 3 if isinstance(patch, int) else tuple(int(p) for p in patch)
    C, D, H, W = volume.shape
    if len(ps) != 3 or any(p < 1 for p in ps):
        raise Mi355SegError(f"gather_patches: patch must be three positive extents, got {patch!r}")
    if ps[0] > D or ps[1] > H or ps[2] > W:
        raise Mi355SegError(f"gather_patches: patch {ps} larger than the volume {(D, H, W)}")
    if any(isinstance(v, bool) or not isinstance(v, int) for v in (first, count)) or first < 0 or count < 1 or first + count > table.shape[0]:
        raise Mi355SegError(f"gather_patches: patches {first!r} .. +{count!r} are not rows of a table of {table.shape[0]}")
    out = torch.empty((count, C) + ps, dtype=torch.float32, device=volume.device)
    if flip:
        lib().call("mi355seg_gather_patches_flip_f32", _p(volume), C, D, H, W, _p(table), first, count, ps[0], ps[1], ps[2], flip, _p(out), _stream())
    else:
        lib().call("mi355seg_gather_patches_f32", _p(volume), C, D, H, W, _p(table), first, count, ps[0], ps[1], ps[2], _p(out), _stream())
    return out


def _axis_vectors(vectors, extents, device, what):
    """three 1-D arrays (numpy / lists / tensors), one per axis, of the given lengths -> float32 tensors on ``device``"""
    if len(vectors) != 3:
        raise Mi355SegError(f"{what}: expected three per-axis arrays (z, y, x), got {len(vectors)}")
    out = []
    for v, n in zip(vectors, extents):
        v = torch.as_tensor(v)
        if v.dim() != 1 or v.numel() != n:
            raise Mi355SegError(f"{what}: expected per-axis arrays of {tuple(extents)} values, got one of shape {tuple(v.shape)}")
        out.append(v.to(torch.float32).to(device).contiguous())       # rounded to fp32 where it lives, then uploaded (a no-op for a device tensor)
    return out


def _accumulator(acc, what):
    _require_cuda(acc, what)
    if acc.dim() != 4 or not acc.is_contiguous():
        raise Mi355SegError(f"{what}: expected a contiguous accumulator [K, D, H, W], got shape {tuple(acc.shape)}")
    if not 2 <= acc.shape[0] <= MAX_AGGREGATE_CLASSES:
        raise Mi355SegError(f"{what}: K must lie in 2..{MAX_AGGREGATE_CLASSES}, got {acc.shape[0]}")
    return acc


def aggregate_patches(acc, logits, table, first, weights, flip=0):
    """One batch of torchio's GridAggregator.add_batch in a soft mode (predict.py:141), in place: for every patch ``b`` of ``logits``
    [count, K, pd, ph, pw] (fp32, GPU), placed at the origin of row ``first + b`` of the int32 window ``table`` [P, 9] on the device,
    ``acc[k, origin + v] += ((wz[z] * wy[y]) * wx[x]) * softmax(logits[b])[k, v]``.  acc: fp32 [K, D, H, W], zeroed by the caller
    before the first batch; weights: the three per-axis windows (``predict.window_weights``).  Per element the additions happen in
    ascending patch index, so the result does not depend on how the patches are batched and is bitwise reproducible.
    ``flip`` (0..7, as in gather_patches): the logits are those of the mirrored patches and are un-mirrored as they are read
    (mi355seg_aggregate_patches_flip_f32) -- bitwise the call with ``torch.flip(logits, axes)`` and flip=0; weights and destination
    keep the un-mirrored coordinates."""
    flip = _flip_code(flip, "aggregate_patches")
    acc = _accumulator(acc, "aggregate_patches")
    _require_cuda(logits, "aggregate_patches logits")
    if logits.dim() != 5 or logits.shape[0] == 0 or logits.shape[1] != acc.shape[0]:
        raise Mi355SegError(f"aggregate_patches: expected logits [count, {acc.shape[0]}, pd, ph, pw], got shape {tuple(logits.shape)}")
    if not table.is_cuda or table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != 9 or not table.is_contiguous():
        raise Mi355SegError("aggregate_patches: expected the contiguous int32 window table [P, 9] on the GPU")
    count, K, pd, ph, pw = logits.shape
    _, D, H, W = acc.shape
    if isinstance(first, bool) or not isinstance(first, int) or first < 0 or first + count > table.shape[0]:
        raise Mi355SegError(f"aggregate_patches: patches {first!r} .. +{count} are not rows of a table of {table.shape[0]}")
    if pd > D or ph > H or pw > W:
        raise Mi355SegError(f"aggregate_patches: patch {(pd, ph, pw)} larger than the volume {(D, H, W)}")
    wz, wy, wx = _axis_vectors(weights, (pd, ph, pw), acc.device, "aggregate_patches weights")
    logits = logits.contiguous()
    if flip:
        lib().call("mi355seg_aggregate_patches_flip_f32", _p(logits), K, _p(table), first, count, pd, ph, pw, _p(wz), _p(wy), _p(wx),
                   flip, _p(acc), D, H, W, _stream())
    else:
        lib().call("mi355seg_aggregate_patches_f32", _p(logits), K, _p(table), first, count, pd, ph, pw, _p(wz), _p(wy), _p(wx),
                   _p(acc), D, H, W, _stream())
    return acc


def aggregate_finalize(acc, axis_sums, probabilities=False):
    """GridAggregator.get_output_tensor of a soft mode, then the argmax (predict.py:146,139): acc fp32 [K, D, H, W] -> int64 labels
    [1, D, H, W] (first maximum on ties), or (labels, prob) with prob fp32 [K, D, H, W] = acc / ((sz[z] * sy[y]) * sx[x]);
    axis_sums: the three per-axis normalisers (``predict.axis_weight_sums``)."""
    acc = _accumulator(acc, "aggregate_finalize")
    K, D, H, W = acc.shape
    sz, sy, sx = _axis_vectors(axis_sums, (D, H, W), acc.device, "aggregate_finalize axis_sums")
    labels = torch.empty((1, D, H, W), dtype=torch.int64, device=acc.device)
    prob = torch.empty_like(acc) if probabilities else None
    lib().call("mi355seg_aggregate_finalize_f32", _p(acc), K, D, H, W, _p(sz), _p(sy), _p(sx), _p(labels), _p(prob), _stream())
    return (labels, prob) if probabilities else labels


def dice_counts(gt, pred):
    """Integer counters of utils/metric.py on two int64 device tensors -> int64[4]
    (sum gt, sum pred, nnz(gt & pred), nnz(gt | pred))."""
    if not gt.is_cuda or gt.dtype != torch.int64 or pred.dtype != torch.int64:
        raise Mi355SegError("dice_counts: expected int64 tensors on the GPU")
    gt, pred = gt.contiguous(), pred.contiguous()
    L = lib()
    ws = workspace(L.query("mi355seg_loss_ws_bytes", gt.numel()), gt.device)
    out = torch.empty(4, dtype=torch.int64, device=gt.device)
    L.call("mi355seg_dice_counts_i64", _p(gt), _p(pred), gt.numel(), _p(out), _p(ws), ws.numel(), _stream())
    return out


def _label_volume(t, what):
    """int64 GPU label volume -> contiguous [D, H, W] (leading singleton dimensions, the reference's [C=1, D, H, W] and
    [1, 1, D, H, W], are dropped)."""
    if not t.is_cuda or t.dtype != torch.int64:
        raise Mi355SegError(f"{what}: expected int64 tensors on the GPU")
    if t.dim() < 3 or t.numel() != t.shape[-3] * t.shape[-2] * t.shape[-1] or t.numel() == 0:
        raise Mi355SegError(f"{what}: expected one label volume [D, H, W] (leading dimensions of size 1 allowed), got {tuple(t.shape)}")
    return t.reshape(t.shape[-3:]).contiguous()


def _spacing3(spacing, what):
    sp = tuple(float(v) for v in (spacing if hasattr(spacing, "__len__") else (spacing,) * 3))
    if len(sp) != 3 or not all(v > 0 and v < float("inf") for v in sp):
        raise Mi355SegError(f"{what}: spacing must be three positive numbers (sz, sy, sx), got {spacing!r}")
    return sp


def confusion_counts(gt, pred):
    """utils/metric.py:34-55 on two int64 device tensors -> int64[8]: the four counters of ``dice_counts`` followed by
    tp, fp, fn, tn (value sums of the reference's tp_array, fp_array, fn_array, tn_array)."""
    if not gt.is_cuda or gt.dtype != torch.int64 or pred.dtype != torch.int64 or gt.numel() != pred.numel():
        raise Mi355SegError("confusion_counts: expected two int64 tensors of one size on the GPU")
    gt, pred = gt.contiguous(), pred.contiguous()
    L = lib()
    ws = workspace(L.query("mi355seg_confusion_counts_ws_bytes", gt.numel()), gt.device)
    out = torch.empty(8, dtype=torch.int64, device=gt.device)
    L.call("mi355seg_confusion_counts_i64", _p(gt), _p(pred), gt.numel(), _p(out), _p(ws), ws.numel(), _stream())
    return out


def mask_edges(gt, pred):
    """Surface voxels of two label volumes (foreground != 0) -> (edges uint8 [2, D, H, W], info int64[8]).  A foreground voxel is an
    edge voxel when one of its six face neighbours is background, outside the array counting as background.  info = (edge voxels of
    gt, of pred, box lo z, y, x, box hi z, y, x) with the box around both edge sets, hi exclusive."""
    gt, pred = _label_volume(gt, "mask_edges"), _label_volume(pred, "mask_edges")
    if gt.shape != pred.shape:
        raise Mi355SegError(f"mask_edges: shapes differ, {tuple(gt.shape)} and {tuple(pred.shape)}")
    D, H, W = gt.shape
    edges = torch.empty((2, D, H, W), dtype=torch.uint8, device=gt.device)
    info = torch.empty(8, dtype=torch.int64, device=gt.device)
    lib().call("mi355seg_mask_edges_i64", _p(gt), _p(pred), D, H, W, _p(edges), _p(info), _stream())
    return edges, info


def _full_box(shape):
    return (0, 0, 0) + tuple(int(v) for v in shape)


def edt3d(sites, spacing, box=None):
    """Exact SQUARED Euclidean distance to the nearest non-zero voxel of each of the two site maps: uint8 [2, D, H, W] on the GPU ->
    fp64 [2, bd, bh, bw].  ``box`` = (z0, y0, x0, bd, bh, bw) restricts the transform to a part of the volume that holds every site
    (default: the whole volume); +inf where a map has no site."""
    if not sites.is_cuda or sites.dtype != torch.uint8 or sites.dim() != 4 or sites.shape[0] != 2 or sites.numel() == 0:
        raise Mi355SegError("edt3d: expected a uint8 tensor [2, D, H, W] on the GPU")
    sz, sy, sx = _spacing3(spacing, "edt3d")
    sites = sites.contiguous()
    D, H, W = sites.shape[1:]
    z0, y0, x0, bd, bh, bw = box or _full_box(sites.shape[1:])
    L = lib()
    ws = workspace(L.query("mi355seg_edt3d_ws_bytes", bd, bh, bw), sites.device)
    dt2 = torch.empty((2, bd, bh, bw), dtype=torch.float64, device=sites.device)
    L.call("mi355seg_edt3d_f64", _p(sites), D, H, W, z0, y0, x0, bd, bh, bw, sz, sy, sx, _p(dt2), _p(ws), ws.numel(), _stream())
    return dt2


def surface_distances(edges, dt2, n_gt, n_pred, box=None):
    """(distances from the edge voxels of gt to the surface of pred, and from those of pred to the surface of gt): two fp64 vectors
    of n_gt / n_pred elements in no particular order.  ``edges`` and the counts come from ``mask_edges``, ``dt2`` from ``edt3d``."""
    if not edges.is_cuda or edges.dtype != torch.uint8 or edges.dim() != 4 or dt2.dtype != torch.float64 or not dt2.is_cuda:
        raise Mi355SegError("surface_distances: expected uint8 edges [2, D, H, W] and fp64 squared distances on the GPU")
    D, H, W = edges.shape[1:]
    z0, y0, x0, bd, bh, bw = box or _full_box(edges.shape[1:])
    if tuple(dt2.shape) != (2, bd, bh, bw):
        raise Mi355SegError(f"surface_distances: squared distances of shape {tuple(dt2.shape)} do not match the box {(2, bd, bh, bw)}")
    n_gt, n_pred = int(n_gt), int(n_pred)
    stride = max(n_gt, n_pred, 1)
    dist = torch.empty((2, stride), dtype=torch.float64, device=edges.device)
    cursor = torch.empty(2, dtype=torch.int64, device=edges.device)
    lib().call("mi355seg_surface_distances_f64", _p(edges.contiguous()), D, H, W, z0, y0, x0, bd, bh, bw, _p(dt2.contiguous()), n_gt, n_pred,
               _p(dist), stride, _p(cursor), _stream())
    return dist[0, :n_gt], dist[1, :n_pred]


def _percentile(v, q):
    """np.percentile(v, q) with linear interpolation between the order statistics at position q/100 * (n - 1); NaN for no samples."""
    n = v.numel()
    if n == 0:
        return torch.full((), float("nan"), dtype=torch.float64, device=v.device)
    s = torch.sort(v).values
    pos = q / 100.0 * (n - 1)
    lo = min(int(pos), n - 1)
    hi = min(lo + 1, n - 1)
    a, b = s[lo], s[hi]
    return torch.where(a == b, a, a + (b - a) * (pos - lo))      # a == b: also keeps inf - inf out of it


def hd95(gt, pred, spacing, percentile=95.0):
    """Symmetric percentile Hausdorff distance between the surfaces of two int64 label volumes on the GPU, in the units of
    ``spacing`` = (sz, sy, sx): what ``compute_hausdorff_distance(pred, gdth, percentile=95, spacing=spacing)`` of
    utils/metric.py:32 returns.  -> 0-dim fp64 device tensor; not finite when either mask has no foreground.
    The eight integers of ``mask_edges`` (edge counts and box) are read back to size the launches; nothing else leaves the device.
    The transforms run on the bounding box of the two surfaces only: no site lies outside it and no distance is read outside it."""
    sp = _spacing3(spacing, "hd95")
    if not 0 <= float(percentile) <= 100:
        raise Mi355SegError(f"hd95: percentile must lie in [0, 100], got {percentile}")
    edges, info = mask_edges(gt, pred)
    n_gt, n_pred, z0, y0, x0, z1, y1, x1 = info.tolist()
    if n_gt == 0 or n_pred == 0:
        return torch.full((), float("nan"), dtype=torch.float64, device=edges.device)
    box = (z0, y0, x0, z1 - z0, y1 - y0, x1 - x0)
    dt2 = edt3d(edges, sp, box)
    d_gt, d_pred = surface_distances(edges, dt2, n_gt, n_pred, box)
    return torch.maximum(_percentile(d_gt, float(percentile)), _percentile(d_pred, float(percentile)))


CONNECTIVITIES = (6, 18, 26)
MAX_KEEP_LARGEST = 16


def components_tile():
    """(tz, ty, tx): the tile the library cuts a volume into before it merges components across tiles (csrc/components.hip)."""
    L = lib()
    return tuple(int(L.query("mi355seg_components_tile_extent", a)) for a in range(3))


def _connectivity(connectivity, what):
    if isinstance(connectivity, bool) or not isinstance(connectivity, int) or connectivity not in CONNECTIVITIES:
        raise Mi355SegError(f"{what}: connectivity must be 6, 18 or 26, got {connectivity!r}")
    return connectivity


def _component_counts(min_voxels, keep_largest, what):
    for name, v in (("min_voxels", min_voxels), ("keep_largest", keep_largest)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise Mi355SegError(f"{what}: {name} must be a non-negative integer, got {v!r}")
    if keep_largest > MAX_KEEP_LARGEST:
        raise Mi355SegError(f"{what}: keep_largest must lie in 0..{MAX_KEEP_LARGEST}, got {keep_largest!r}")
    return min_voxels, keep_largest


def connected_components(mask, connectivity=26):
    """Connected components of an int64 label volume on the GPU (foreground != 0; scipy.ndimage.label with the 6-, 18- or
    26-neighbourhood) -> (labels int32 [D, H, W], sizes int32 [D*H*W], info int64[4]).  labels: 0 on background, else 1 + the raster
    index of the first voxel of the component; sizes[r]: voxels of the component labelled r + 1, 0 elsewhere; info = (foreground
    voxels, components, size of the largest component, its label; equal sizes: the smaller label).  Nothing is copied to the host."""
    connectivity = _connectivity(connectivity, "connected_components")
    mask = _label_volume(mask, "connected_components")
    D, H, W = mask.shape
    L = lib()
    need = L.query("mi355seg_components_ws_bytes", D, H, W)
    if need == 0:
        raise Mi355SegError(f"connected_components: a volume of {D * H * W} voxels is refused (labels are int32: at most 2^31 - 2)")
    ws = workspace(need, mask.device)
    labels = torch.empty((D, H, W), dtype=torch.int32, device=mask.device)
    sizes = torch.empty(D * H * W, dtype=torch.int32, device=mask.device)
    info = torch.empty(4, dtype=torch.int64, device=mask.device)
    L.call("mi355seg_components_label_i64", _p(mask), D, H, W, connectivity, _p(labels), _p(sizes), _p(info), _p(ws), ws.numel(), _stream())
    return labels, sizes, info


def select_components(labels_of_roots, sizes_of_roots, min_voxels=0, keep_largest=0):
    """Which components stay: the compact table of components (their labels and sizes, e.g. ``r = torch.nonzero(sizes)[:, 0]``,
    ``r + 1`` and ``sizes[r]``) -> int32 labels to keep.  Components below ``min_voxels`` go; then, with ``keep_largest`` = K > 0,
    the K largest of the rest stay (largest first; equal sizes: the smaller label first), all of them where fewer than K remain.
    Plain tensor code on the table's device, CPU tensors included."""
    min_voxels, keep_largest = _component_counts(min_voxels, keep_largest, "select_components")
    lab, sz = labels_of_roots.reshape(-1).to(torch.int64), sizes_of_roots.reshape(-1).to(torch.int64)
    if lab.numel() != sz.numel():
        raise Mi355SegError(f"select_components: {lab.numel()} labels and {sz.numel()} sizes")
    big = sz >= min_voxels
    lab, sz = lab[big], sz[big]
    if keep_largest > 0:
        key = (sz << 32) | (0xFFFFFFFF - lab)              # larger size first, then the smaller label
        lab = lab[torch.sort(key, descending=True).indices[:keep_largest]]
    return lab.to(torch.int32)


def filter_components(mask, min_voxels=0, keep_largest=0, connectivity=26, inplace=False):
    """Connected-component clean-up of an int64 label volume on the GPU -> (mask_out int64 of mask's shape, stats).  Components
    below ``min_voxels`` voxels are set to 0; with ``keep_largest`` = K in 1..16 only the K largest of the rest survive (equal sizes:
    the one that starts first in raster order).  Label values of kept voxels are preserved.  stats = {components, kept,
    voxels_removed, largest}: components found, components kept, voxels set to 0, size of the largest component found.  The four
    integers of stats are the only values copied to the host.  With both thresholds 0 the mask itself is returned; ``inplace`` writes
    the result into ``mask`` (contiguous) and returns it."""
    min_voxels, keep_largest = _component_counts(min_voxels, keep_largest, "filter_components")
    vol = _label_volume(mask, "filter_components")
    labels, sizes, info = connected_components(vol, connectivity)
    if min_voxels == 0 and keep_largest == 0:
        comps, largest = info[1:3].tolist()
        return mask, {"components": comps, "kept": comps, "voxels_removed": 0, "largest": largest}
    roots = torch.nonzero(sizes)[:, 0]
    keep = select_components(roots + 1, sizes[roots], min_voxels, keep_largest)
    listed = keep_largest > 0
    if inplace and vol.data_ptr() != mask.data_ptr():
        raise Mi355SegError("filter_components: inplace needs a contiguous mask")
    out = vol if inplace else torch.empty_like(vol)
    removed = torch.empty(1, dtype=torch.int64, device=vol.device)
    keep_dev = keep.contiguous() if keep.numel() else torch.zeros(1, dtype=torch.int32, device=vol.device)
    lib().call("mi355seg_components_filter_i64", _p(vol), _p(labels), _p(sizes), vol.numel(), min_voxels,
               _p(keep_dev) if listed else None, keep.numel() if listed else 0, _p(out), _p(removed), _stream())
    comps, kept, gone, largest = torch.stack([info[1], torch.full_like(info[1], keep.numel()), removed[0], info[2]]).tolist()
    return out.reshape(mask.shape), {"components": comps, "kept": kept, "voxels_removed": gone, "largest": largest}


MAX_COMPONENT_CLASS = 255


def connected_components_by_class(mask, connectivity=26):
    """Class-aware connected components of an int64 label volume on the GPU: two voxels are joined only when they are neighbours
    and carry the same value 1..255 (``scipy.ndimage.label(mask == k, ...)`` for every k != 0 that occurs), all classes in ONE
    labelling call -> (labels int32 [D, H, W], sizes int32 [D*H*W], info int64[8]).  labels and sizes as ``connected_components``
    (a component belongs to one class: the mask value at its first voxel); info[:4] as there over all classes, info[4] = voxels
    outside 0..255, which raise here (that one integer is read back)."""
    connectivity = _connectivity(connectivity, "connected_components_by_class")
    mask = _label_volume(mask, "connected_components_by_class")
    D, H, W = mask.shape
    L = lib()
    need = L.query("mi355seg_components_classes_ws_bytes", D, H, W)
    if need == 0:
        raise Mi355SegError(f"connected_components_by_class: a volume of {D * H * W} voxels is refused (labels are int32: at most 2^31 - 2)")
    ws = workspace(need, mask.device)
    labels = torch.empty((D, H, W), dtype=torch.int32, device=mask.device)
    sizes = torch.empty(D * H * W, dtype=torch.int32, device=mask.device)
    info = torch.empty(8, dtype=torch.int64, device=mask.device)
    L.call("mi355seg_components_label_classes_i64", _p(mask), D, H, W, connectivity, _p(labels), _p(sizes), _p(info), _p(ws), ws.numel(), _stream())
    bad = int(info[4])
    if bad:
        raise Mi355SegError(f"connected_components_by_class: {bad} voxels hold values outside 0..{MAX_COMPONENT_CLASS}")
    return labels, sizes, info


def component_table(mask, labels, sizes, info):
    """The compact table of a labelling (``connected_components`` or ``connected_components_by_class`` of ``mask``) and consecutive
    labels -> (labels_consecutive int32 [D, H, W], first int32[n], size int32[n], cls int64[n]).  Components are ranked by their
    first voxel in raster order, which is the order scipy.ndimage.label numbers them in: labels_consecutive is 1..n (0 on
    background), first / size / cls[k] the first voxel's raster index, the voxel count and the mask value at the first voxel of the
    component labelled k + 1.  Nothing but n = info[1] goes to the host."""
    vol = _label_volume(mask, "component_table")
    for t, name, dt in ((labels, "labels", torch.int32), (sizes, "sizes", torch.int32), (info, "info", torch.int64)):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or t.device != vol.device:
            raise Mi355SegError(f"component_table: {name} must be a {dt} tensor on the mask's GPU")
    if labels.numel() != vol.numel() or sizes.numel() != vol.numel() or info.numel() < 4:
        raise Mi355SegError(f"component_table: the mask holds {vol.numel()} voxels, labels {labels.numel()}, sizes {sizes.numel()}, info {info.numel()} entries")
    labels, sizes = aligned_contiguous(labels), aligned_contiguous(sizes)
    L = lib()
    n = int(info[1])
    ws = workspace(L.query("mi355seg_components_table_ws_bytes", vol.numel()), vol.device)
    lc = torch.empty(tuple(vol.shape), dtype=torch.int32, device=vol.device)
    first = torch.empty(n, dtype=torch.int32, device=vol.device)
    size = torch.empty(n, dtype=torch.int32, device=vol.device)
    cls = torch.empty(n, dtype=torch.int64, device=vol.device)
    L.call("mi355seg_components_table_i64", _p(vol), _p(labels), _p(sizes), vol.numel(), n, _p(lc), _p(first) if n else None,
           _p(size) if n else None, _p(cls) if n else None, _p(ws), ws.numel(), _stream())
    return lc, first, size, cls


def _per_class(v, name, what, top=None):
    """an int (every class) or a {class: value} dict of non-negative ints -> the same, checked"""
    def ok(x, hi):
        return not isinstance(x, bool) and isinstance(x, int) and 0 <= x and (hi is None or x <= hi)
    if isinstance(v, dict):
        for k, x in v.items():
            if not ok(k, None) or k == 0:
                raise Mi355SegError(f"{what}: {name} names class {k!r}; classes are positive integers")
            if not ok(x, top):
                raise Mi355SegError(f"{what}: {name}[{k}] must be " + (f"an integer in 0..{top}" if top is not None else "a non-negative integer") + f", got {x!r}")
        return dict(v)
    if not ok(v, top):
        raise Mi355SegError(f"{what}: {name} must be " + (f"an integer in 0..{top}" if top is not None else "a non-negative integer") +
                            f" or a {{class: value}} dict, got {v!r}")
    return v


def _per_component(v, cls):
    """the per-class argument spread over the components of the table: int64 [n]"""
    if not isinstance(v, dict):
        return torch.full_like(cls, v)
    out = torch.zeros_like(cls)
    for k, x in v.items():
        out = torch.where(cls == k, torch.full_like(cls, x), out)
    return out


def select_components_by_class(cls, size, min_voxels=0, keep_largest=0):
    """Which components of a compact table stay, class by class: (cls[n], size[n]) in rank order (``component_table``) -> bool
    keep[n].  ``min_voxels`` and ``keep_largest`` are each an int (every class) or a ``{class: value}`` dict (a class that is absent:
    0); ``keep_largest`` lies in 0..MAX_KEEP_LARGEST.  Within a class: components below ``min_voxels`` go; then, with ``keep_largest``
    = K > 0, the K largest of the rest stay (equal sizes: the smaller rank), all of them where fewer remain.  Plain tensor code on
    the table's device, CPU tensors included."""
    what = "select_components_by_class"
    min_voxels, keep_largest = _per_class(min_voxels, "min_voxels", what), _per_class(keep_largest, "keep_largest", what, MAX_KEEP_LARGEST)
    if not torch.is_tensor(cls) or not torch.is_tensor(size) or cls.is_floating_point() or size.is_floating_point():
        raise Mi355SegError(f"{what}: cls and size must be integer tensors")
    if cls.numel() != size.numel():
        raise Mi355SegError(f"{what}: {cls.numel()} classes and {size.numel()} sizes")
    cls, size = cls.reshape(-1).to(torch.int64), size.reshape(-1).to(torch.int64)
    n = cls.numel()
    big = size >= _per_component(min_voxels, cls)
    top = _per_component(keep_largest, cls)
    # the components of each class side by side, the ones that pass min_voxels first, larger first, equal sizes by rank: three
    # stable sorts, the last key first
    order = torch.sort(size, descending=True, stable=True).indices
    order = order[torch.sort((~big[order]).to(torch.int8), stable=True).indices]
    order = order[torch.sort(cls[order], stable=True).indices]
    pos = torch.arange(n, dtype=torch.int64, device=cls.device)
    c = cls[order]
    starts = torch.ones(n, dtype=torch.bool, device=cls.device)
    starts[1:] = c[1:] != c[:-1]
    place = pos - torch.cummax(torch.where(starts, pos, torch.zeros_like(pos)), 0).values if n else pos      # place within the class
    stay = big[order] & ((top[order] == 0) | (place < top[order]))
    keep = torch.zeros(n, dtype=torch.bool, device=cls.device)
    keep[order] = stay
    return keep


def class_component_stats(cls, size, keep, classes=()):
    """{class: {components, kept, voxels_removed, largest}} from the n-entry table and its keep flags, for every class of the
    table and of ``classes``; one [4, 256] copy to the host (and the table's smallest and largest class, which must lie in 0..255)."""
    K = MAX_COMPONENT_CLASS + 1
    cls, size, keep = cls.reshape(-1).to(torch.int64), size.reshape(-1).to(torch.int64), keep.reshape(-1).to(torch.int64)
    if cls.numel():                                  # (a table of the binary labelling may hold any value at a root)
        lo, hi = torch.stack([cls.min(), cls.max()]).tolist()
        if lo < 0 or hi > MAX_COMPONENT_CLASS:
            raise Mi355SegError(f"class_component_stats: classes lie in 0..{MAX_COMPONENT_CLASS}, the table holds {lo}..{hi}")
    zero = torch.zeros(K, dtype=torch.int64, device=cls.device)
    rows = torch.stack([zero.index_add(0, cls, torch.ones_like(cls)), zero.index_add(0, cls, keep),
                        zero.index_add(0, cls, size * (1 - keep)), zero.scatter_reduce(0, cls, size, "amax")]).tolist()
    present = sorted({k for k in range(K) if rows[0][k]} | {int(k) for k in classes})
    return {k: {"components": rows[0][k], "kept": rows[1][k], "voxels_removed": rows[2][k], "largest": rows[3][k]} for k in present}


def filter_components_by_class(mask, min_voxels=0, keep_largest=0, connectivity=26, inplace=False):
    """Connected-component clean-up of a multi-class int64 label volume on the GPU, class by class -> (mask_out, stats).  Components
    are those of ``connected_components_by_class``; ``min_voxels`` / ``keep_largest`` as ``select_components_by_class`` (an int for
    every class or a ``{class: value}`` dict).  Kept voxels keep their class value.  stats[k] = {components, kept, voxels_removed,
    largest} for every class in the arguments or the mask, from the n-entry table.  With both thresholds 0 the mask itself is
    returned; ``inplace`` writes the result into ``mask`` (contiguous) and returns it."""
    what = "filter_components_by_class"
    min_voxels, keep_largest = _per_class(min_voxels, "min_voxels", what), _per_class(keep_largest, "keep_largest", what, MAX_KEEP_LARGEST)
    for arg in (min_voxels, keep_largest):
        if isinstance(arg, dict) and any(k > MAX_COMPONENT_CLASS for k in arg):
            raise Mi355SegError(f"{what}: classes lie in 1..{MAX_COMPONENT_CLASS}, got {sorted(arg)}")
    vol = _label_volume(mask, what)
    if inplace and vol.data_ptr() != mask.data_ptr():
        raise Mi355SegError(f"{what}: inplace needs a contiguous mask")
    labels, sizes, info = connected_components_by_class(vol, connectivity)
    lc, first, size, cls = component_table(vol, labels, sizes, info)
    keep = select_components_by_class(cls, size, min_voxels, keep_largest)
    named = {k for arg in (min_voxels, keep_largest) if isinstance(arg, dict) for k in arg}
    stats = class_component_stats(cls, size, keep, named)
    if not any(any(arg.values()) if isinstance(arg, dict) else arg for arg in (min_voxels, keep_largest)):
        return mask, stats
    return filter_by_component_table(mask, lc, keep, inplace=inplace)[0], stats


def filter_by_component_table(mask, labels_consecutive, keep, inplace=False):
    """``out[v] = (lc[v] == 0 or keep[lc[v] - 1]) ? mask[v] : 0`` on the GPU with the consecutive labels of ``component_table`` and one
    flag per component (bool or uint8 [n]) -> (mask_out, removed int64[1] on the device: the voxels set to 0).  Nothing goes to the
    host.  ``inplace`` writes into ``mask`` (contiguous) and returns it."""
    what = "filter_by_component_table"
    vol = _label_volume(mask, what)
    lc = labels_consecutive
    if not torch.is_tensor(lc) or not lc.is_cuda or lc.dtype != torch.int32 or lc.numel() != vol.numel():
        raise Mi355SegError(f"{what}: labels_consecutive must be an int32 GPU tensor of the mask's {vol.numel()} voxels")
    if not torch.is_tensor(keep) or not keep.is_cuda or keep.dtype not in (torch.bool, torch.uint8) or keep.dim() != 1:
        raise Mi355SegError(f"{what}: keep must be a bool or uint8 GPU tensor [n]")
    if inplace and vol.data_ptr() != mask.data_ptr():
        raise Mi355SegError(f"{what}: inplace needs a contiguous mask")
    lc = aligned_contiguous(lc)
    out = vol if inplace else torch.empty_like(vol)
    removed = torch.empty(1, dtype=torch.int64, device=vol.device)
    flags = keep.to(torch.uint8).contiguous()
    lib().call("mi355seg_components_filter_table_i64", _p(vol), _p(lc), _p(flags) if flags.numel() else None, flags.numel(), vol.numel(),
               _p(out), _p(removed), _stream())
    return out.reshape(mask.shape), removed


class _BCEArgmaxDice(Function):
    """train.py:204,209,221 in ONE pass over the logits: BCE-with-logits mean loss (differentiable w.r.t. the logits),
    pred.argmax(1, keepdim) and the four integer Dice counters of metric(gt.argmax, mask)."""

    @staticmethod
    def forward(ctx, logits, target):
        _require_cuda(logits, "bce_argmax_dice input")
        logits, target = aligned_contiguous(logits), aligned_contiguous(target.to(torch.float32))     # (the backward is the float4 BCE kernel)
        if logits.shape != target.shape:
            raise ValueError(f"Target size ({tuple(target.shape)}) must be the same as input size ({tuple(logits.shape)})")
        N, K = logits.shape[0], logits.shape[1]
        S = logits[0, 0].numel()
        L = lib()
        ws = workspace(L.query("mi355seg_loss_ws_bytes", logits.numel()), logits.device)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        mask = torch.empty((N, 1) + tuple(logits.shape[2:]), dtype=torch.int64, device=logits.device)
        counts = torch.empty(4, dtype=torch.int64, device=logits.device)
        L.call("mi355seg_bce_argmax_dice_f32", _p(logits), _p(target), N, K, S, _p(loss), _p(mask), _p(counts),
               _p(ws), ws.numel(), _stream())
        ctx.save_for_backward(logits, target)
        ctx.mark_non_differentiable(mask, counts)
        return loss, mask, counts

    @staticmethod
    def backward(ctx, g, _gmask, _gcounts):
        logits, target = ctx.saved_tensors
        g = g.contiguous().to(torch.float32)
        d = torch.empty_like(logits)
        lib().call("mi355seg_bce_logits_bwd_f32", _p(logits), _p(target), _p(g), logits.numel(), _p(d), _stream())
        return d, None


def bce_argmax_dice(logits, target):
    """Fused tail of the train step: (loss, mask int64 [N,1,...], counts int64[4]); the loss carries the autograd
    edge of nn.BCEWithLogitsLoss()."""
    return _BCEArgmaxDice.apply(logits, target)


# ----------------------------------------------------------------------------- compound losses (config.loss; csrc/loss_tail.hip)
LOSS_MODES = ("dice", "dice_bce", "ce", "dice_ce", "focal", "dice_focal", "tversky")
LOSS_VOXEL_TERMS = {None: 0, "bce": 1, "focal": 2, "ce": 3}          # the C-ABI's voxel_term / region_term selectors
LOSS_REGION_TERMS = {None: 0, "dice": 1, "tversky": 2}
_LOSS_MODE_TERMS = {"dice": (None, "dice"), "dice_bce": ("bce", "dice"), "ce": ("ce", None), "dice_ce": ("ce", "dice"),
                    "focal": ("focal", None), "dice_focal": ("focal", "dice"), "tversky": (None, "tversky")}
MAX_LOSS_CLASSES = 16
FOCAL_GAMMA, TVERSKY_ALPHA, TVERSKY_BETA = 2.0, 0.3, 0.7        # the defaults of LossSpec.from_mode / CompoundLoss


class LossSpec(collections.namedtuple("LossSpec", "voxel region gamma alpha beta w_voxel w_region")):
    """What mi355seg_loss_tail_*_f32 computes: loss = w_voxel * voxel + w_region * region with voxel in (None, "bce", "focal", "ce")
    and region in (None, "dice", "tversky"); gamma is the focal exponent (0 or 1..8), alpha / beta the Tversky weights of false
    positives / false negatives.  Definitions: DESIGN.md 4.16."""
    __slots__ = ()

    @classmethod
    def from_mode(cls, mode, weights=(1.0, 1.0), focal_gamma=FOCAL_GAMMA, tversky_alpha=TVERSKY_ALPHA, tversky_beta=TVERSKY_BETA):
        if not isinstance(mode, str) or mode not in _LOSS_MODE_TERMS:
            raise ValueError(f"loss mode must be one of {', '.join(LOSS_MODES)}, got {mode!r}")
        voxel, region = _LOSS_MODE_TERMS[mode]
        try:
            wv, wr = (float(w) for w in weights)
        except (TypeError, ValueError):
            raise ValueError(f"loss weights must be two numbers (voxel term, region term), got {weights!r}") from None
        return cls(voxel, region, float(focal_gamma), float(tversky_alpha), float(tversky_beta), wv, wr).checked()

    def checked(self):
        """The refusals of the C entry points, as ValueError before anything reaches the device."""
        if self.voxel not in LOSS_VOXEL_TERMS or self.region not in LOSS_REGION_TERMS:
            raise ValueError(f"unknown loss term in {tuple(self)!r}: voxel in (None, 'bce', 'focal', 'ce'), region in (None, 'dice', 'tversky')")
        if self.voxel is None and self.region is None:
            raise ValueError("a loss needs a voxel term or a region term")
        if not (self.w_voxel >= 0 and self.w_region >= 0):
            raise ValueError(f"loss weights must be >= 0, got {(self.w_voxel, self.w_region)!r}")
        if not (self.gamma == 0 or 1 <= self.gamma <= 8):
            raise ValueError(f"focal gamma must be 0 or in [1, 8], got {self.gamma!r}")
        if not (self.alpha >= 0 and self.beta >= 0) or (self.region == "tversky" and not self.alpha + self.beta > 0):
            raise ValueError(f"tversky alpha and beta must be >= 0 with alpha + beta > 0, got {(self.alpha, self.beta)!r}")
        return self


class _LossTail(Function):
    """The fused tail for a LossSpec: (loss, mask, counts, terms, sums) from one pass over logits and target plus a one-block
    finalise; the backward is one pass.  The coefficients of the backward stay on the device (coef), so the pair is capturable
    in a HIP graph exactly like _BCEArgmaxDice.  ``labels``: the target is a uint8 label map [N,...] in place of the float one-hot
    [N,K,...] (the *_lab entry points), and class_counts int64 [K,3] (tp, pred, gt) is a sixth output."""

    @staticmethod
    def forward(ctx, logits, target, spec, labels):
        what, form = ("loss_tail_labels", "_lab") if labels else ("loss_tail", "")
        _require_cuda(logits, f"{what} input")
        logits = aligned_contiguous(logits)
        target = _checked_label_map(target, what) if labels else aligned_contiguous(target.to(torch.float32))
        if not labels and logits.shape != target.shape:
            raise ValueError(f"Target size ({tuple(target.shape)}) must be the same as input size ({tuple(logits.shape)})")
        if logits.dim() < 3:
            raise Mi355SegError(f"{what}: expected [N,K,...], got {tuple(logits.shape)}")
        if labels and (logits.shape[0],) + tuple(logits.shape[2:]) != tuple(target.shape):
            raise ValueError(f"Label size ({tuple(target.shape)}) must be the input size ({tuple(logits.shape)}) without its channels")
        N, K = logits.shape[0], logits.shape[1]
        S = logits[0, 0].numel()
        dev = logits.device
        L = lib()
        ws = workspace(L.query(f"mi355seg_loss_tail{form}_ws_bytes", N, K, S), dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        mask = torch.empty((N, 1) + tuple(logits.shape[2:]), dtype=torch.int64, device=dev)
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        terms = torch.empty(2, dtype=torch.float64, device=dev)
        sums = torch.empty((K, 5), dtype=torch.float64, device=dev)
        extra = (torch.empty((K, 3), dtype=torch.int64, device=dev),) if labels else ()
        coef = torch.empty(1 + 2 * MAX_LOSS_CLASSES, dtype=torch.float64, device=dev)
        args = (LOSS_VOXEL_TERMS[spec.voxel], LOSS_REGION_TERMS[spec.region], spec.gamma)
        L.call(f"mi355seg_loss_tail_fwd{form}_f32", _p(logits), _p(target), N, K, S, *args, spec.alpha, spec.beta, spec.w_voxel, spec.w_region,
               _p(loss), _p(terms), _p(sums), _p(mask), _p(counts), _p(coef), *(_p(t) for t in extra), _p(ws), ws.numel(), _stream())
        ctx.save_for_backward(logits, target, coef)
        ctx.args, ctx.form = args, form
        ctx.mark_non_differentiable(mask, counts, terms, sums, *extra)
        ctx.set_materialize_grads(False)         # (or autograd zero-fills a gradient for each of them, the int64 mask included, per backward)
        return (loss, mask, counts, terms, sums) + extra

    @staticmethod
    def backward(ctx, g, *_):
        if g is None:
            return None, None, None, None
        logits, target, coef = ctx.saved_tensors
        g = g.contiguous().to(torch.float32)
        N, K = logits.shape[0], logits.shape[1]
        d = torch.empty_like(logits)
        lib().call(f"mi355seg_loss_tail_bwd{ctx.form}_f32", _p(logits), _p(target), _p(coef), _p(g), N, K, logits[0, 0].numel(), *ctx.args, _p(d), _stream())
        return d, None, None, None


def _loss_tail(logits, target, spec, labels):
    if not isinstance(spec, LossSpec):
        raise TypeError(f"{'loss_tail_labels' if labels else 'loss_tail'}: spec must be a functional.LossSpec, got {type(spec).__name__}")
    return _LossTail.apply(logits, target, spec.checked(), labels)


def loss_tail_full(logits, target, spec):
    """loss_tail plus the per-class sums: (loss, mask, counts, terms, sums fp64 [K,5]) -- sums[k] = (sum p t, sum p, sum t, sum p^2,
    sum t^2) with p = sigmoid(logits[:, k]), what dice_sums gives for class k."""
    return _loss_tail(logits, target, spec, False)


def loss_tail(logits, target, spec):
    """Fused tail of the train step for a compound loss: (loss, mask int64 [N,1,...], counts int64[4], terms fp64[2]).  ``loss`` =
    spec.w_voxel * terms[0] + spec.w_region * terms[1] carries the autograd edge; mask, counts and terms do not.  logits and
    target [N,K,...] float32, 1 <= K <= 16 (target: the K-channel float target bce_argmax_dice takes)."""
    return loss_tail_full(logits, target, spec)[:4]


# ----------------------------------------------------------------------------- label-map targets (config.multiclass)
LABEL_OUT_OF_RANGE = 255            # what labels_u8 stores for a value that is no integer in [0, K)


def _require_device(t, what):
    if not t.is_cuda:
        raise Mi355SegError(f"{what}: expected a tensor on an MI355X (cuda/HIP) device, got {t.device}; there is no CPU fallback in this package")


def _checked_classes(K, what):
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= MAX_LOSS_CLASSES:
        raise ValueError(f"{what}: K must be an integer in 1..{MAX_LOSS_CLASSES}, got {K!r}")
    return K


def labels_u8(gt, K, bad=None):
    """The float label map ``gt`` [N,1,...] as uint8 labels [N,...] in one launch.  A value that is not an integer in [0, K) is
    stored as 255 and counted: the count is ADDED to ``bad`` (int64[1] on the device; a fresh zeroed one when None).  Returns
    (labels, bad); nothing is read back."""
    _require_device(gt, "labels_u8 input")
    _checked_classes(K, "labels_u8")
    gt = aligned_contiguous(gt.to(torch.float32))
    if gt.dim() < 3 or gt.shape[1] != 1:
        raise Mi355SegError(f"labels_u8: expected [N,1,...], got {tuple(gt.shape)}")
    if bad is None:
        bad = torch.zeros(1, dtype=torch.int64, device=gt.device)
    elif bad.dtype != torch.int64 or bad.numel() != 1 or bad.device != gt.device:
        raise Mi355SegError("labels_u8: bad must be an int64[1] tensor on the input's device")
    out = torch.empty((gt.shape[0],) + tuple(gt.shape[2:]), dtype=torch.uint8, device=gt.device)
    lib().call("mi355seg_labels_u8_f32", _p(gt), gt.numel(), K, _p(out), _p(bad), _stream())
    return out, bad


def _checked_label_map(labels, what):
    _require_device(labels, f"{what} labels")
    if labels.dtype != torch.uint8 or labels.dim() < 2:
        raise Mi355SegError(f"{what}: labels must be uint8 [N,...], got {labels.dtype} {tuple(labels.shape)}")
    return aligned_contiguous(labels)


def one_hot_labels(labels, K):
    """float32 one-hot [N,K,...] of uint8 labels [N,...]; a label >= K gives an all-zero column."""
    labels = _checked_label_map(labels, "one_hot_labels")
    _checked_classes(K, "one_hot_labels")
    N = labels.shape[0]
    out = torch.empty((N, K) + tuple(labels.shape[1:]), dtype=torch.float32, device=labels.device)
    lib().call("mi355seg_onehot_u8_f32", _p(labels), N, K, labels[0].numel(), _p(out), _stream())
    return out


def loss_tail_labels_full(logits, labels, spec):
    """loss_tail_labels plus the per-class sums: (loss, mask, counts, terms, sums fp64 [K,5], class_counts int64 [K,3])."""
    return _loss_tail(logits, labels, spec, True)


def loss_tail_labels(logits, labels, spec):
    """loss_tail on a label map: logits [N,K,...] float32, labels uint8 [N,...] (labels_u8).  Returns (loss, mask, counts, terms,
    class_counts): the first four with the bits loss_tail gives on one_hot_labels(labels, K), and class_counts int64 [K,3] = per
    class (tp, pred, gt) for utils.metric.class_metrics_from_counts.  A label >= K belongs to no class."""
    out = loss_tail_labels_full(logits, labels, spec)
    return out[:4] + (out[5],)


def class_counts(gt, pred, K):
    """int64 [K,3] = per class (tp, pred, gt) of two int64 label volumes of equal size, on the device."""
    _require_device(gt, "class_counts gt")
    _require_device(pred, "class_counts pred")
    _checked_classes(K, "class_counts")
    gt, pred = gt.to(torch.int64).contiguous(), pred.to(torch.int64).contiguous()
    if gt.numel() != pred.numel() or gt.numel() < 1:
        raise ValueError(f"class_counts: gt {tuple(gt.shape)} and pred {tuple(pred.shape)} must hold the same number of voxels (>= 1)")
    L = lib()
    ws = workspace(L.query("mi355seg_class_counts_ws_bytes", gt.numel(), K), gt.device)
    out = torch.empty((K, 3), dtype=torch.int64, device=gt.device)
    L.call("mi355seg_class_counts_i64", _p(gt), _p(pred), gt.numel(), K, _p(out), _p(ws), ws.numel(), _stream())
    return out


# ----------------------------------------------------------------------------- soft-clDice (config.cldice_weight; csrc/cldice.hip)
CLDICE_ITERS, CLDICE_SMOOTH = 3, 1.0
MAX_SKEL_ITERS = 32


def checked_skel_iters(iters, what):
    """The C entry points' refusal of ``iters``, as ValueError before anything reaches the device."""
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 1 <= iters <= MAX_SKEL_ITERS:
        raise ValueError(f"{what}: iters must be an integer in 1..{MAX_SKEL_ITERS}, got {iters!r}")
    return int(iters)


def _skel_volume(x, what):
    _require_cuda(x, what)
    if x.dim() != 5:
        raise Mi355SegError(f"{what}: expected [N,C,D,H,W], got {tuple(x.shape)}")
    return x.contiguous()


def _skel_forward(x, iters):
    """Levels 0 .. iters over the contiguous volume x: (level stack, skeleton).  The stack (E_1 .. E_{iters+1} and the skeleton after
    every level) is what the backward reads; the skeleton is a view of its last slot, which the backward does not read."""
    L = lib()
    N, C, D, H, W = x.shape
    nbytes = L.query("mi355seg_soft_skel_ws_bytes", N * C, D, H, W, iters)
    stack = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
    for j in range(iters + 1):
        L.call("mi355seg_soft_skel_step_fwd_f32", _p(x), N * C, D, H, W, iters, j, _p(stack), nbytes, _stream())
    slot = nbytes // (2 * (iters + 1))
    return stack, stack[(2 * iters + 1) * slot:][:x.numel() * 4].view(torch.float32).view(x.shape)


def _skel_backward(x, stack, iters, g):
    """d(sum g * soft_skel(x)) / dx: levels iters .. 0, one launch each; the two gradients ping-pong between two buffers each."""
    L = lib()
    N, C, D, H, W = x.shape
    ge, gs = (torch.empty_like(x), torch.empty_like(x)), (torch.empty_like(x), torch.empty_like(x))
    g_skel, g_next = g, None
    for j in range(iters, -1, -1):
        out_e, out_s = ge[j & 1], (gs[j & 1] if j else None)
        L.call("mi355seg_soft_skel_step_bwd_f32", _p(x), _p(g_skel), _p(g_next), _p(out_e), _p(out_s), N * C, D, H, W, iters, j,
               _p(stack), stack.numel(), _stream())
        g_skel, g_next = out_s, out_e
    return g_next


class _SoftSkeleton(Function):
    @staticmethod
    def forward(ctx, x, iters):
        x = _skel_volume(x, "soft_skeleton input")
        stack, skel = _skel_forward(x, iters)
        if not ctx.needs_input_grad[0]:
            return skel.clone()                  # (nothing to keep: the stack goes)
        ctx.save_for_backward(x, stack)
        ctx.iters = iters
        return skel

    @staticmethod
    def backward(ctx, g):
        x, stack = ctx.saved_tensors
        return _skel_backward(x, stack, ctx.iters, g.contiguous().to(torch.float32)), None


def soft_skeleton(x, iters=CLDICE_ITERS):
    """The soft skeleton of clDice (Shit et al., CVPR 2021) of a float32 volume [N,C,D,H,W] on the device, one launch per level
    forward and one backward: E_{j+1} = erode(E_j), delta = relu(E_j - dilate(E_{j+1})), skel += relu(delta - skel * delta) for
    j = 0 .. iters.  The forward has the bits of the ATen fp32 composition; at ties the backward routes a minimum's or maximum's
    gradient to the candidate with the lowest raster index."""
    return _SoftSkeleton.apply(x, checked_skel_iters(iters, "soft_skeleton"))


class _SoftClDice(Function):
    """(cldice fp32 scalar, fp64[3] = cldice, tprec, tsens).  The coefficients of the backward stay on the device (coef), as
    _LossTail's do: capturable in a HIP graph."""

    @staticmethod
    def forward(ctx, logits, target, iters, smooth):
        _require_cuda(logits, "soft_cldice input")
        logits, target = logits.contiguous(), target.to(torch.float32).contiguous()
        if logits.shape != target.shape:
            raise ValueError(f"Target size ({tuple(target.shape)}) must be the same as input size ({tuple(logits.shape)})")
        if logits.dim() != 5:
            raise Mi355SegError(f"soft_cldice: expected [N,K,D,H,W], got {tuple(logits.shape)}")
        N, K = logits.shape[:2]
        S = logits[0, 0].numel()
        dev = logits.device
        L = lib()
        shape = (N, K - (1 if K > 1 else 0)) + tuple(logits.shape[2:])
        P, T = torch.empty(shape, dtype=torch.float32, device=dev), torch.empty(shape, dtype=torch.float32, device=dev)
        L.call("mi355seg_cldice_probs_f32", _p(logits), _p(target), N, K, S, _p(P), _p(T), _stream())
        stack, skel_p = _skel_forward(P, iters)
        skel_t = _skel_forward(T, iters)[1].clone()           # (the target's skeleton has no backward: its stack goes)
        n = P.numel()
        ws = workspace(L.query("mi355seg_cldice_ws_bytes", n), dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        parts, coef = torch.empty(3, dtype=torch.float64, device=dev), torch.empty(3, dtype=torch.float64, device=dev)
        L.call("mi355seg_cldice_sums_f32", _p(skel_p), _p(skel_t), _p(P), _p(T), n, _p(ws), ws.numel(), _stream())
        L.call("mi355seg_cldice_finalize", _p(ws), ws.numel(), n, smooth, _p(loss), _p(parts), _p(coef), _stream())
        ctx.save_for_backward(P, T, skel_t, stack, coef)
        ctx.iters, ctx.dims = iters, (N, K, S)
        ctx.mark_non_differentiable(parts)
        ctx.set_materialize_grads(False)
        return loss, parts

    @staticmethod
    def backward(ctx, g, _gparts):
        if g is None:
            return None, None, None, None
        P, T, skel_t, stack, coef = ctx.saved_tensors
        N, K, S = ctx.dims
        L = lib()
        g = g.contiguous().to(torch.float32)
        g_skel = torch.empty_like(P)
        L.call("mi355seg_cldice_bwd_head_f32", _p(T), _p(coef), P.numel(), _p(g_skel), _stream())
        g_p = _skel_backward(P, stack, ctx.iters, g_skel)
        d = torch.empty((N, K) + tuple(P.shape[2:]), dtype=torch.float32, device=P.device)
        L.call("mi355seg_cldice_bwd_tail_f32", _p(g_p), _p(skel_t), _p(P), _p(coef), _p(g), N, K, S, _p(d), _stream())
        return d, None, None, None


def soft_cldice_full(logits, target, iters=CLDICE_ITERS, smooth=CLDICE_SMOOTH):
    """soft_cldice with the term itself in fp64: (cldice fp32 scalar with the autograd edge, fp64[3] = cldice, tprec, tsens)."""
    iters = checked_skel_iters(iters, "soft_cldice")
    if isinstance(smooth, bool) or not isinstance(smooth, (int, float)) or not smooth > 0:
        raise ValueError(f"soft_cldice: smooth must be a number > 0, got {smooth!r}")
    return _SoftClDice.apply(logits, target, iters, float(smooth))


def soft_cldice(logits, target, iters=CLDICE_ITERS, smooth=CLDICE_SMOOTH):
    """The soft-clDice term on logits and target [N,K,D,H,W]: (cldice, parts).  With P = sigmoid(logits[:, 1:]), T = target[:, 1:]
    (the single channel when K = 1), S_P = soft_skeleton(P, iters), S_T = soft_skeleton(T, iters): tprec = (sum S_P T + smooth) /
    (sum S_P + smooth), tsens = (sum S_T P + smooth) / (sum S_T + smooth), cldice = 1 - 2 tprec tsens / (tprec + tsens), sums over
    batch, channels and voxels.  ``cldice`` is a float32 scalar carrying the autograd edge to ``logits``; ``parts`` is fp64[2] =
    (tprec, tsens), non-differentiable."""
    loss, parts = soft_cldice_full(logits, target, iters, smooth)
    return loss, parts[1:]


# ----------------------------------------------------------------------------- boundary loss (config.boundary_weight; csrc/boundary.hip)
MAX_SDM_AXIS = 2047


def checked_spacing(spacing, what):
    """(sz, sy, sx) as three positive finite floats, or ValueError before anything reaches the device."""
    try:
        vals = [spacing] if isinstance(spacing, (bool, str)) else list(spacing)
        ok = len(vals) == 3 and all(not isinstance(v, (bool, str)) for v in vals)
        vals = tuple(float(v) for v in vals) if ok else ()
    except (TypeError, ValueError):
        vals = ()
    if len(vals) != 3 or not all(0 < v < float("inf") for v in vals):
        raise ValueError(f"{what}: spacing must be three positive numbers (sz, sy, sx), got {spacing!r}")
    return vals


def _signed_distance_map(target, spacing, what):
    _require_cuda(target, f"{what} input")
    target = target.to(torch.float32).contiguous()
    if target.dim() != 5:
        raise Mi355SegError(f"{what}: expected [N,K,D,H,W], got {tuple(target.shape)}")
    N, K, D, H, W = target.shape
    L = lib()
    phi = torch.empty((N, K - (1 if K > 1 else 0), D, H, W), dtype=torch.float32, device=target.device)
    nbytes = L.query("mi355seg_sdm_ws_bytes", N, K, D, H, W)
    ws = workspace(nbytes, target.device)
    sz, sy, sx = spacing
    L.call("mi355seg_sdm_f32", _p(target), N, K, D, H, W, sz, sy, sx, min(spacing), _p(phi), _p(ws), ws.numel(), _stream())
    return phi


def signed_distance_map(target, spacing=(1, 1, 1)):
    """The signed Euclidean distance map of every class of a one-hot target [N,K,D,H,W] on the device (one_hot2dist of the official
    boundary loss): float32 [N, K - c0, D, H, W], c0 = 1 for K > 1 (no background channel), 0 for K = 1.  A voxel belongs to class k
    when target[n, k] > 0.5.  Outside the class phi = +distance to the nearest voxel of the class, inside phi = -(distance to the
    nearest voxel outside the class - min(spacing)), and phi = 0 for a whole (n, k) volume whose class is absent or fills the patch;
    distances under the voxel ``spacing`` (sz, sy, sx), inside the patch only.  Not differentiable.  DESIGN.md 4.21."""
    return _signed_distance_map(target, checked_spacing(spacing, "signed_distance_map"), "signed_distance_map")


class _BoundaryLoss(Function):
    """(boundary fp32 scalar, fp64[1] = the same in fp64).  The coefficient of the backward stays on the device (coef), as
    _SoftClDice's do: capturable in a HIP graph."""

    @staticmethod
    def forward(ctx, logits, target, spacing):
        _require_cuda(logits, "boundary_loss input")
        logits, target = logits.contiguous(), target.to(torch.float32).contiguous()
        if logits.shape != target.shape:
            raise ValueError(f"Target size ({tuple(target.shape)}) must be the same as input size ({tuple(logits.shape)})")
        if logits.dim() != 5:
            raise Mi355SegError(f"boundary_loss: expected [N,K,D,H,W], got {tuple(logits.shape)}")
        N, K = logits.shape[:2]
        S = logits[0, 0].numel()
        dev = logits.device
        L = lib()
        phi = _signed_distance_map(target, spacing, "boundary_loss")
        ws = workspace(L.query("mi355seg_boundary_ws_bytes", phi.numel()), dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        parts, coef = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
        L.call("mi355seg_boundary_fwd_f32", _p(logits), _p(phi), N, K, S, _p(loss), _p(parts), _p(coef), _p(ws), ws.numel(), _stream())
        ctx.save_for_backward(phi, logits, coef)
        ctx.dims = (N, K, S)
        ctx.mark_non_differentiable(parts)
        ctx.set_materialize_grads(False)
        return loss, parts

    @staticmethod
    def backward(ctx, g, _gparts):
        if g is None:
            return None, None, None
        phi, logits, coef = ctx.saved_tensors
        N, K, S = ctx.dims
        g = g.contiguous().to(torch.float32)
        d = torch.empty_like(logits)
        lib().call("mi355seg_boundary_bwd_f32", _p(logits), _p(phi), _p(coef), _p(g), N, K, S, _p(d), _stream())
        return d, None, None


def boundary_loss_full(logits, target, spacing=(1, 1, 1)):
    """boundary_loss with the term itself in fp64: (boundary fp32 scalar with the autograd edge, fp64[1] = boundary)."""
    return _BoundaryLoss.apply(logits, target, checked_spacing(spacing, "boundary_loss"))


def boundary_loss(logits, target, spacing=(1, 1, 1)):
    """The boundary loss term (Kervadec et al., MIDL 2019) on logits and one-hot target [N,K,D,H,W]: mean(sigmoid(logits[:, 1:]) *
    phi) with phi = signed_distance_map(target, spacing) (the single channel when K = 1), the mean over batch, channels and voxels.
    A float32 scalar carrying the autograd edge to ``logits``; the map is recomputed on the device at every call."""
    return boundary_loss_full(logits, target, spacing)[0]


def two_channel_gt(gt):
    """train.py:190-193 as one kernel: cat([(gt == 0), gt], dim=1) as float for a single-channel label volume."""
    if not gt.is_cuda:
        raise Mi355SegError(f"two_channel_gt input: expected a tensor on an MI355X (cuda/HIP) device, got {gt.device}")
    gt = gt.contiguous().to(torch.float32)
    if gt.dim() < 3 or gt.shape[1] != 1:
        raise Mi355SegError(f"two_channel_gt: expected [N,1,...], got {tuple(gt.shape)}")
    N = gt.shape[0]
    S = gt[0].numel()
    out = torch.empty((N, 2) + tuple(gt.shape[2:]), dtype=torch.float32, device=gt.device)
    lib().call("mi355seg_two_channel_gt_f32", _p(gt), _p(out), N, S, _stream())
    return out


def znormalize(x):
    """tio.ZNormalization() of one volume on the device: (x - mean) / std over all voxels (unbiased std)."""
    _require_cuda(x, "znormalize input")
    x = aligned_contiguous(x.to(torch.float32))
    L = lib()
    ws = workspace(L.query("mi355seg_znorm_ws_bytes", x.numel()), x.device)
    y = torch.empty_like(x)
    L.call("mi355seg_znorm_f32", _p(x), x.numel(), _p(y), _p(ws), ws.numel(), _stream())
    return y


PERCENTILES_MAX = 16            # MI355SEG_PERCENTILES_MAX: percentiles per call
Percentiles = collections.namedtuple("Percentiles", "values order counts")


def _mask_args(mask_gt):
    return (0, 0.0) if mask_gt is None else (1, float(mask_gt))


def percentiles(x, qs, mask_gt=None):
    """Exact percentiles of one volume on the device (csrc/intensity.hip, radix select): ``np.percentile(v, qs)`` (method ``linear``)
    of v = every voxel of ``x``, or with ``mask_gt`` the voxels with ``x > mask_gt``.  Returns device tensors, without synchronising:
    ``values`` float64 [nq], the interpolated percentiles; ``order`` float32 [nq, 2], the two order statistics behind each (exact
    voxel values, at the ranks floor(q / 100 * (m - 1)) and that + 1 clamped to m - 1); ``counts`` int64 [2] = (m, the number of
    non-finite voxels).  ``x``: float32, contiguous and 16-byte aligned (a misaligned view is refused, not copied), fewer than 2^31
    elements; at most 16 percentiles per call, each in 0 .. 100."""
    _require_cuda(x, "percentiles input")
    if not x.is_contiguous() or x.numel() < 1:
        raise Mi355SegError(f"percentiles: expected a contiguous, non-empty volume, got shape {tuple(x.shape)} strides {x.stride()}")
    q = np.ascontiguousarray(np.asarray(qs, dtype=np.float64).reshape(-1))
    L = lib()
    ws = workspace(L.query("mi355seg_percentiles_ws_bytes", x.numel()), x.device)
    values = torch.empty(max(q.size, 1), dtype=torch.float64, device=x.device)
    order = torch.empty((max(q.size, 1), 2), dtype=torch.float32, device=x.device)
    counts = torch.empty(2, dtype=torch.int64, device=x.device)
    use, t = _mask_args(mask_gt)
    L.call("mi355seg_percentiles_f32", _p(x), x.numel(), q.ctypes.data, int(q.size), use, t, _p(values), _p(order), _p(counts), _p(ws),
           ws.numel(), _stream())
    return Percentiles(values, order, counts)


def _map_args(imap):
    kx, ky, slope, lo, hi = imap.f32()
    return (kx, ky, slope), (kx.ctypes.data, ky.ctypes.data, slope.ctypes.data, int(kx.size), lo, hi)


def intensity_moments(x, imap, mask_gt=None, pivot=0.0):
    """Count, mean and unbiased variance of ``imap(x)`` over the voxels with ``x > mask_gt`` (the RAW x; every voxel without a mask):
    float64 [4] on the device = (count, mean, variance, sum of imap(x) - pivot), fp64 sums pivoted on ``pivot`` (any value near the
    mapped data keeps them well conditioned).  ``imap``: an ``intensity.IntensityMap`` (``intensity.IDENTITY`` for the raw voxels)."""
    _require_cuda(x, "intensity_moments input")
    if not x.is_contiguous() or x.numel() < 1:
        raise Mi355SegError(f"intensity_moments: expected a contiguous, non-empty volume, got shape {tuple(x.shape)}")
    L = lib()
    ws = workspace(L.query("mi355seg_intensity_moments_ws_bytes", x.numel()), x.device)
    out = torch.empty(4, dtype=torch.float64, device=x.device)
    keep, args = _map_args(imap)
    L.call("mi355seg_intensity_moments_f32", _p(x), x.numel(), *args, *_mask_args(mask_gt), float(pivot), _p(out), _p(ws), ws.numel(), _stream())
    return out


def intensity_map(x, imap, out=None):
    """``imap`` (an ``intensity.IntensityMap``) applied to every voxel of ``x`` in one streaming pass; ``out=x`` maps in place."""
    _require_cuda(x, "intensity_map input")
    if not x.is_contiguous() or x.numel() < 1:
        raise Mi355SegError(f"intensity_map: expected a contiguous, non-empty volume, got shape {tuple(x.shape)}")
    y = torch.empty_like(x) if out is None else out
    if y.shape != x.shape or y.dtype != x.dtype or y.device != x.device or not y.is_contiguous():
        raise Mi355SegError(f"intensity_map: out must be a contiguous float32 tensor of x's shape on its device, got {tuple(y.shape)} {y.dtype}")
    keep, args = _map_args(imap)
    lib().call("mi355seg_intensity_map_f32", _p(x), x.numel(), *args, _p(y), _stream())
    return y


def intensity_mask_gt(x, mask):
    """``config.intensity_mask`` -> the threshold of the mask ``x > T`` (``None`` for no mask): ``mean`` is the mean of all voxels from
    a device reduction, rounded to fp32; a number is rounded to fp32."""
    if mask == "none":
        return None
    if mask != "mean":
        return float(np.float32(mask))
    from .intensity import IDENTITY
    x0 = float(x.view(-1)[0])
    mean = float(intensity_moments(x, IDENTITY, pivot=x0)[1]) if np.isfinite(x0) else float("nan")
    if not np.isfinite(mean):
        raise ValueError("intensity: the volume holds non-finite voxels (NaN or infinity); clean the data first")
    return float(np.float32(mean))


def volume_percentiles(x, qs, mask="none"):
    """``np.percentile`` of the masked voxels of ``x`` (``mask``: ``none``, ``mean`` or a threshold, as ``config.intensity_mask``) as
    float64 on the HOST (one device-to-host copy per 16 percentiles), after the checks of ``normalize_intensity``: no non-finite
    voxel, at least two voxels under the mask."""
    from .intensity import check_counts
    t = intensity_mask_gt(x, mask)
    qs = list(qs)
    vals = []
    for i in range(0, len(qs), PERCENTILES_MAX):
        r = percentiles(x, qs[i:i + PERCENTILES_MAX], t)
        m, nonfinite = (int(c) for c in r.counts.cpu())
        check_counts(m, nonfinite)
        vals.append(r.values.cpu().numpy())
    return np.concatenate(vals)


def normalize_intensity(x, spec, landmarks=None):
    """One volume through ``config.intensity`` on the device: ``spec`` an ``intensity.IntensitySpec`` (``intensity.parse_intensity``;
    the definitions of every mode and mask are in that module's docstring), ``landmarks`` replaces ``spec.landmarks``.  All elements
    of ``x`` are one volume, as ``znormalize``.  Percentiles (radix select) and moments come from the device, the map's knots are
    formed on the host in fp64 (``intensity.build_map``), and ONE streaming pass writes the result.  Raises ``Mi355SegError`` for a CPU
    tensor and ``ValueError`` for a non-finite voxel, a mask that leaves fewer than two voxels, a zero range or a zero deviation."""
    from .intensity import IntensitySpec, build_map
    if not isinstance(spec, IntensitySpec):
        raise TypeError(f"normalize_intensity: spec must be an intensity.IntensitySpec, got {type(spec).__name__}")
    _require_cuda(x, "normalize_intensity input")
    if landmarks is not None:
        spec = IntensitySpec(spec.mode, spec.percentiles, spec.out, spec.mask, landmarks)
    x = aligned_contiguous(x.to(torch.float32))
    if x.numel() < 2:
        raise ValueError(f"intensity: the volume holds {x.numel()} voxels, the statistics need at least 2")
    t = intensity_mask_gt(x, spec.mask)

    def moments(imap):
        pivot = float(imap(float(x.view(-1)[0])))
        c, mean, var, _ = intensity_moments(x, imap, t, pivot).cpu().tolist()
        return c, mean, var

    imap = build_map(spec, lambda qs: volume_percentiles(x, qs, "none" if t is None else t), moments)
    return intensity_map(x, imap)


# ----------------------------------------------------------------------------- resampling to a target spacing (csrc/resample.hip)
from .resample import resample_axis_table, resampled_shape  # noqa: E402,F401  (host-only, numpy fp64; part of this module's interface)

RESAMPLE_ORDERS = (0, 1, 3)
RESAMPLE_LABEL_MODES = ("nearest", "linear")    # MI355SEG_RESAMPLE_LABELS_NEAREST / _LINEAR
RESAMPLE_MAX_CLASSES = 16                       # MI355SEG_RESAMPLE_MAX_CLASSES


class ResampleTables:
    """The three per-axis tables of one resampling, packed z, y, x: ``base`` int32 and ``frac`` float32 on the device (each
    Do + Ho + Wo long), ``base_host`` the numpy copy the library validates, ``in_shape`` / ``out_shape`` = (D, H, W) / (Do, Ho, Wo)."""

    def __init__(self, in_shape, out_shape, ratios, order, device):
        self.in_shape, self.out_shape, self.order = tuple(int(n) for n in in_shape), tuple(int(n) for n in out_shape), order
        if len(self.in_shape) != 3 or len(self.out_shape) != 3:
            raise Mi355SegError(f"resample: expected (D, H, W) shapes, got {in_shape} -> {out_shape}")
        tabs = [resample_axis_table(n, no, r, order) for n, no, r in zip(self.in_shape, self.out_shape, ratios)]
        self.base_host = np.ascontiguousarray(np.concatenate([t[0] for t in tabs]), dtype=np.int32)
        self.frac_host = np.ascontiguousarray(np.concatenate([t[1] for t in tabs]), dtype=np.float32)
        self.base = torch.from_numpy(self.base_host).to(device)
        self.frac = torch.from_numpy(self.frac_host).to(device)

    def args(self):
        return _p(self.base), _p(self.frac), self.base_host.ctypes.data


def _volume4(t, what, dtype=torch.float32):
    """[D,H,W] or [C,D,H,W] device tensor -> (contiguous [C,D,H,W], had a channel axis)"""
    if not t.is_cuda:
        raise Mi355SegError(f"{what}: expected a tensor on an MI355X (cuda/HIP) device, got {t.device}; there is no CPU fallback in this package")
    if t.dtype != dtype:
        raise Mi355SegError(f"{what}: expected {dtype}, got {t.dtype}")
    if t.dim() not in (3, 4) or t.numel() == 0:
        raise Mi355SegError(f"{what}: expected a non-empty volume [D,H,W] or [C,D,H,W], got {tuple(t.shape)}")
    return (t[None] if t.dim() == 3 else t).contiguous(), t.dim() == 4


def bspline3_prefilter(x, out=None, axis=None):
    """Cubic B-spline coefficients of ``x`` ([D,H,W] or [C,D,H,W], float32) per channel: scipy.ndimage.spline_filter(order=3,
    mode='mirror') along W, H and D (mi355seg_bspline3_prefilter_f32; fp32, bitwise reproducible).  ``out=x`` filters in place;
    ``axis`` = 0 | 1 | 2 runs the one pass along D | H | W only."""
    x4, _ = _volume4(x, "bspline3_prefilter input")
    y = torch.empty_like(x4) if out is None else out
    if y.dtype != x4.dtype or y.device != x4.device or y.numel() != x4.numel() or not y.is_contiguous():
        raise Mi355SegError(f"bspline3_prefilter: out must be a contiguous float32 tensor of x's shape on its device, got {tuple(y.shape)} {y.dtype}")
    if out is not None and out.data_ptr() == x.data_ptr() and x4.data_ptr() != x.data_ptr():
        raise Mi355SegError("bspline3_prefilter: in place needs a contiguous input")
    C, D, H, W = x4.shape
    L = lib()
    ws = workspace(L.query("mi355seg_bspline3_prefilter_ws_bytes", C, D, H, W), x.device)
    if axis is None:
        L.call("mi355seg_bspline3_prefilter_f32", _p(x4), C, D, H, W, _p(y), _p(ws), ws.numel(), _stream())
    else:
        L.call("mi355seg_bspline3_prefilter_axis_f32", _p(x4), C, D, H, W, int(axis), _p(y), _p(ws), ws.numel(), _stream())
    return y.view(x.shape) if out is None else out


def resample3d(x, tables, order=None):
    """``x`` [C,D,H,W] or [D,H,W] through ``tables`` (a ``ResampleTables`` of x's spatial shape) at ``order`` 0 | 1 | 3 (default: the
    tables' own) in one launch (mi355seg_resample3d_f32).  At order 3 ``x`` must hold the coefficients of ``bspline3_prefilter``."""
    order = tables.order if order is None else order
    x4, had_c = _volume4(x, "resample3d input")
    if tuple(x4.shape[1:]) != tables.in_shape:
        raise Mi355SegError(f"resample3d: the tables are for a volume {tables.in_shape}, got {tuple(x4.shape[1:])}")
    C = x4.shape[0]
    y = torch.empty((C,) + tables.out_shape, dtype=torch.float32, device=x.device)
    lib().call("mi355seg_resample3d_f32", _p(x4), C, *tables.in_shape, int(order), *tables.args(), _p(y), *tables.out_shape, _stream())
    return y if had_c else y[0]


def resample3d_labels(y, tables, mode):
    """Label volume ``y`` ([C,D,H,W] or [D,H,W]; float32 holding integers, or int64) through ``tables`` (order 0 for ``nearest``,
    order 1 for ``linear``) -> (labels of y's dtype, ``bad``: device int64 [1], the number of output voxels that read a value that is
    no integer in 0 .. 15).  No synchronisation."""
    if mode not in RESAMPLE_LABEL_MODES:
        raise ValueError(f"resample labels: mode must be one of {RESAMPLE_LABEL_MODES}, got {mode!r}")
    if y.dtype not in (torch.float32, torch.int64):
        raise Mi355SegError(f"resample labels: expected float32 or int64 labels, got {y.dtype}")
    y4, had_c = _volume4(y, "resample labels", y.dtype)
    if tuple(y4.shape[1:]) != tables.in_shape or tables.order != RESAMPLE_LABEL_MODES.index(mode):
        raise Mi355SegError(f"resample labels: the tables are order {tables.order} for a volume {tables.in_shape}, got mode {mode} and "
                            f"{tuple(y4.shape[1:])}")
    C = y4.shape[0]
    L = lib()
    ws = workspace(L.query("mi355seg_resample3d_labels_ws_bytes"), y.device)
    out = torch.empty((C,) + tables.out_shape, dtype=y.dtype, device=y.device)
    bad = torch.empty(1, dtype=torch.int64, device=y.device)
    L.call("mi355seg_resample3d_labels_" + ("f32" if y.dtype == torch.float32 else "i64"), _p(y4), C, *tables.in_shape,
           RESAMPLE_LABEL_MODES.index(mode), *tables.args(), _p(out), *tables.out_shape, _p(bad), _p(ws), ws.numel(), _stream())
    return (out if had_c else out[0]), bad


def _spacings(spacing, target):
    from .resample import _triple
    return _triple(spacing, "spacing"), _triple(target, "target spacing")


def resample_volume(x, spacing, target, order=1):
    """``x`` ([C,D,H,W] or [D,H,W], float32) at voxel ``spacing`` (sz, sy, sx) -> the volume at ``target`` spacing, shape
    ``resampled_shape``; ``order`` 0 (nearest, exact), 1 (trilinear) or 3 (cubic B-spline: prefilter + gather).  Definitions:
    include/mi355seg.h, "Resampling".  Equal spacings return ``x`` itself."""
    if order not in RESAMPLE_ORDERS:
        raise ValueError(f"resample_volume: order must be one of {RESAMPLE_ORDERS}, got {order!r}")
    spacing, target = _spacings(spacing, target)
    _volume4(x, "resample_volume input")
    if spacing == target:
        return x
    shape = tuple(x.shape[-3:])
    tables = ResampleTables(shape, resampled_shape(shape, spacing, target), [t / s for s, t in zip(spacing, target)], order, x.device)
    return resample3d(bspline3_prefilter(x) if order == 3 else x, tables)


def _checked_labels(out, bad, what):
    n = int(bad.cpu()[0])                                    # the one device-to-host copy
    if n:
        raise ValueError(f"{what}: {n} resampled voxels read a label that is not an integer in 0 .. {RESAMPLE_MAX_CLASSES - 1}")
    return out


def resample_labels(y, spacing, target, mode="linear"):
    """Label volume ``y`` at ``spacing`` -> ``target`` spacing: ``nearest`` (order 0, tio.Resample's rule) or ``linear`` (the class of
    largest trilinear weight, lowest class on ties: the argmax of the resampled one-hot volume without that volume).  Raises
    ``ValueError`` when a label read is no integer in 0 .. 15 (one device counter, read once)."""
    spacing, target = _spacings(spacing, target)
    shape = tuple(y.shape[-3:])
    tables = ResampleTables(shape, resampled_shape(shape, spacing, target), [t / s for s, t in zip(spacing, target)],
                            RESAMPLE_LABEL_MODES.index(mode) if mode in RESAMPLE_LABEL_MODES else 1, y.device)
    return _checked_labels(*resample3d_labels(y, tables, mode), "resample_labels")


def resample_back_labels(mask, shape, spacing, target, mode="linear"):
    """The way back of a label mask: ``mask`` (int64 or float32, [C,D',H',W'] or [D',H',W']) on the grid of ``target`` spacing -> the
    original grid ``shape`` = (D, H, W) of ``spacing``, with the rule of ``resample_labels``."""
    spacing, target = _spacings(spacing, target)
    tables = ResampleTables(tuple(mask.shape[-3:]), shape, [s / t for s, t in zip(spacing, target)],
                            RESAMPLE_LABEL_MODES.index(mode) if mode in RESAMPLE_LABEL_MODES else 1, mask.device)
    return _checked_labels(*resample3d_labels(mask, tables, mode), "resample_back_labels")


def resample_back_argmax(prob, shape, spacing, target, return_probabilities=False):
    """The way back of a blended prediction: ``prob`` float32 [K,D',H',W'] (K <= 16) on the grid of ``target`` spacing -> int64 labels
    [1,D,H,W] on the original grid ``shape`` of ``spacing``: trilinear per class and the argmax (lowest class on ties) in one launch
    (mi355seg_resample3d_argmax_f32); with ``return_probabilities`` also the interpolated float32 [K,D,H,W]."""
    spacing, target = _spacings(spacing, target)
    _require_cuda(prob, "resample_back_argmax input")
    if prob.dim() != 4 or prob.numel() == 0:
        raise Mi355SegError(f"resample_back_argmax: expected probabilities [K,D,H,W], got {tuple(prob.shape)}")
    prob = prob.contiguous()
    K = prob.shape[0]
    tables = ResampleTables(tuple(prob.shape[1:]), shape, [s / t for s, t in zip(spacing, target)], 1, prob.device)
    labels = torch.empty((1,) + tables.out_shape, dtype=torch.int64, device=prob.device)
    out = torch.empty((K,) + tables.out_shape, dtype=torch.float32, device=prob.device) if return_probabilities else None
    lib().call("mi355seg_resample3d_argmax_f32", _p(prob), K, *tables.in_shape, *tables.args(), _p(labels), _p(out), *tables.out_shape, _stream())
    return (labels, out) if return_probabilities else labels


AUG_DESC_WORDS = 64             # MI355SEG_AUG_DESC_WORDS: int32 words of one patch descriptor (layout in include/mi355seg.h)


def augment_stats(x, params):
    """The intensity statistics of one subject visit (dataloader.py:71-73: RandomBiasField -> ZNormalization -> RandomNoise) of the
    raw volume ``x`` [C,D,H,W]: float32[4] = (mu, rho, min V, sigma) on the device, in three launches and without a host round
    trip (``augment_sample`` reads them through the descriptor).  ``params``: the visit's ``data.AugmentParams`` (``bias`` float32[20],
    ``sigma``, ``seed``).  UNPINNED, as the rest of the data path: the definitions in include/mi355seg.h are the specification."""
    _require_cuda(x, "augment_stats volume")
    if x.dim() != 4 or min(x.shape[1:]) < 2 or x[0].numel() >= 1 << 31:
        raise Mi355SegError(f"augment_stats: expected a volume [C,D,H,W] with every spatial dim >= 2 and D*H*W < 2^31, got {tuple(x.shape)}")
    if not x.is_contiguous():
        raise Mi355SegError("augment_stats: the volume must be contiguous (the patch descriptors address it as it is)")
    bias = np.ascontiguousarray(params.bias, dtype=np.float32)
    if bias.shape != (20,):
        raise Mi355SegError(f"augment_stats: expected 20 bias-field coefficients, got {bias.shape}")
    L = lib()
    ws = workspace(L.query("mi355seg_augment_ws_bytes", x.numel()), x.device)
    stats = torch.empty(4, dtype=torch.float32, device=x.device)
    C, D, H, W = x.shape
    L.call("mi355seg_augment_stats_f32", _p(x), C, D, H, W, bias.ctypes.data, float(params.sigma), int(params.seed), _p(stats), _p(ws),
           ws.numel(), _stream())
    return stats


def augment_sample(patches, patch_size):
    """One augmented batch (dataloader.py:69-86 with config.aug=True, then the queue's patch cut) in ONE launch:
    ``patches`` is a sequence of ``(x [C,D,H,W], y [Cy,D,H,W], stats, cp, origin, params)`` -- the raw device volume and its labels,
    ``augment_stats(x, params)``, the visit's control points as a device float32 [3,7,7,7] (``None`` for an affine visit), the patch
    origin (z, y, x) in the augmented volume and the visit's ``data.AugmentParams`` (``matrix`` float32 [3,4] output -> source,
    ``elastic``, ``bias``, ``sigma``, ``seed``).  Returns ``(xb [B,C,pd,ph,pw], yb [B,Cy,pd,ph,pw])``.  One small table upload, no
    synchronisation.  UNPINNED (see ``augment_stats``)."""
    ps = tuple(int(p) for p in ((patch_size,) * 3 if isinstance(patch_size, int) else patch_size))
    if not patches:
        raise Mi355SegError("augment_sample: no patches")
    x0, y0 = patches[0][0], patches[0][1]
    _require_cuda(x0, "augment_sample volume")
    C, Cy, dev = x0.shape[0], y0.shape[0], x0.device
    tab = np.zeros((len(patches), AUG_DESC_WORDS), dtype=np.int32)
    t64, tf = tab.view(np.int64), tab.view(np.float32)
    for i, (x, y, stats, cp, origin, prm) in enumerate(patches):
        _require_cuda(x, "augment_sample volume")
        _require_cuda(y, "augment_sample labels")
        _require_cuda(stats, "augment_sample stats")
        if x.dim() != 4 or y.dim() != 4 or x.shape[0] != C or y.shape[0] != Cy or x.shape[1:] != y.shape[1:] or x.device != dev \
                or y.device != dev or stats.device != dev or not (x.is_contiguous() and y.is_contiguous()) or stats.numel() != 4:
            raise Mi355SegError(f"augment_sample: patch {i}: expected contiguous x [{C},D,H,W] / y [{Cy},D,H,W] of one spatial shape on "
                                f"{dev} and float32[4] stats, got {tuple(x.shape)} / {tuple(y.shape)}")
        if min(x.shape[1:]) < 2 or x[0].numel() >= 1 << 31:
            raise Mi355SegError(f"augment_sample: patch {i}: every spatial dim must be >= 2 and D*H*W < 2^31, got {tuple(x.shape)}")
        if len(origin) != 3 or any(int(o) < 0 or int(o) + p > 1 << 24 for o, p in zip(origin, ps)):
            raise Mi355SegError(f"augment_sample: patch {i}: origin {tuple(origin)} must be non-negative (and below 2^24)")
        m = np.ascontiguousarray(prm.matrix, dtype=np.float32)
        bias = np.ascontiguousarray(prm.bias, dtype=np.float32)
        if m.shape != (3, 4) or bias.shape != (20,) or not np.isfinite(m).all():
            raise Mi355SegError(f"augment_sample: patch {i}: expected a finite 3x4 matrix and 20 bias coefficients")
        t64[i, 0], t64[i, 1], t64[i, 2] = x.data_ptr(), y.data_ptr(), stats.data_ptr()
        if prm.elastic:
            if cp is None or not cp.is_cuda or cp.device != dev or cp.dtype != torch.float32 or cp.numel() != 3 * 343 or not cp.is_contiguous():
                raise Mi355SegError(f"augment_sample: patch {i}: an elastic visit needs its control points as a device float32 [3,7,7,7]")
            t64[i, 3] = cp.data_ptr()
        tab[i, 8:11] = x.shape[1:]
        tab[i, 11:14] = [int(o) for o in origin]
        tab[i, 14] = 1 if prm.elastic else 0
        tf[i, 16:28] = m.reshape(-1)
        tf[i, 28:48] = bias
        tf[i, 48] = float(prm.sigma)
        t64[i, 25] = int(prm.seed)
    table = torch.from_numpy(tab).to(dev)
    xb = torch.empty((len(patches), C) + ps, dtype=torch.float32, device=dev)
    yb = torch.empty((len(patches), Cy) + ps, dtype=torch.float32, device=dev)
    lib().call("mi355seg_augment_sample_f32", _p(table), len(patches), C, Cy, ps[0], ps[1], ps[2], _p(xb), _p(yb), _stream())
    return xb, yb


LABEL_CHUNK = 1024              # MI355SEG_LABEL_CHUNK: region-linear voxels per chunk of a label index
LABEL_BINS = 17                 # MI355SEG_LABEL_BINS: classes 0 .. 15 and the `bad` bin


class LabelIndex:
    """What ``label_index`` built for one (label volume, patch size) pair and ``label_pick`` selects from:
    ``labels`` the contiguous device volume [D,H,W] the index belongs to (kept alive here: a select re-reads one chunk of it),
    ``shape`` = (D, H, W), ``patch`` = (pd, ph, pw), ``region`` = (m_d, m_h, m_w) the extents of the box of valid patch centres,
    ``index`` the device int64 [17, chunks] of exclusive per-class chunk prefixes, ``counts`` a HOST ``np.int64[17]``: the number of
    region voxels of classes 0 .. 15, then ``bad`` (values that are no integer in [0, 16))."""

    def __init__(self, labels, patch, index, counts):
        self.labels, self.patch, self.index, self.counts = labels, patch, index, counts
        self.shape = tuple(int(s) for s in labels.shape)
        self.region = tuple(n - p + 1 for n, p in zip(self.shape, patch))


def label_index(y, patch_size):
    """The sampling index of tio.LabelSampler(patch_size) over the label volume ``y`` ([1,D,H,W] or [D,H,W], float32 holding integers):
    per-class counts of the region of valid patch centres and their per-chunk prefixes, built in two launches
    (mi355seg_label_index_build_f32) -> ``LabelIndex``.  One device-to-host copy of the 17 totals, the only synchronisation.
    UNPINNED (torchio is absent): the definitions in include/mi355seg.h are the specification."""
    _require_cuda(y, "label_index labels")
    if y.dim() == 4 and y.shape[0] != 1:
        raise Mi355SegError(f"label_index: expected ONE label channel, got {tuple(y.shape)} (multi-channel label maps are not sampled)")
    v = y[0] if y.dim() == 4 else y
    ps = tuple(int(p) for p in ((patch_size,) * 3 if isinstance(patch_size, int) else patch_size))
    if v.dim() != 3 or len(ps) != 3 or v.numel() >= 1 << 31 or any(p < 1 or p > n for p, n in zip(ps, v.shape)):
        raise Mi355SegError(f"label_index: expected labels [1,D,H,W] or [D,H,W] with D*H*W < 2^31 and a patch 1 <= p <= n per axis, "
                            f"got {tuple(y.shape)} and patch {ps}")
    v = v.contiguous()
    D, H, W = v.shape
    L = lib()
    nbytes = L.query("mi355seg_label_index_bytes", D, H, W, *ps)
    index = torch.empty((LABEL_BINS, nbytes // (8 * LABEL_BINS)), dtype=torch.int64, device=v.device)
    counts = torch.empty(LABEL_BINS, dtype=torch.int64, device=v.device)
    L.call("mi355seg_label_index_build_f32", _p(v), D, H, W, *ps, _p(index), nbytes, _p(counts), _stream())
    return LabelIndex(v, ps, index, counts.cpu().numpy())


def label_pick(index, classes, ranks):
    """Patch origins of the picks ``(classes[i], ranks[i])`` -- the voxel of that class with that rank in region-linear order, see
    include/mi355seg.h -- from a ``LabelIndex``: int32 [n, 3] (z, y, x) on the device, one small table upload and one launch
    (mi355seg_label_index_select), no synchronisation.  ``classes`` / ``ranks``: host integer arrays, validated against
    ``index.counts`` here because the kernel trusts them: class in 0 .. 15 and 0 <= rank < counts[class], else ``Mi355SegError``
    before any launch."""
    if not isinstance(index, LabelIndex):
        raise Mi355SegError(f"label_pick: expected the LabelIndex of label_index, got {type(index).__name__}")
    cl, rk = np.asarray(classes), np.asarray(ranks)
    if cl.ndim != 1 or cl.shape != rk.shape or cl.size < 1 or cl.dtype.kind not in "iu" or rk.dtype.kind not in "iu":
        raise Mi355SegError(f"label_pick: expected two equally long 1-D integer arrays of at least one pick, got {cl.dtype}{cl.shape} "
                            f"and {rk.dtype}{rk.shape}")
    cl, rk = cl.astype(np.int64), rk.astype(np.int64)
    if ((cl < 0) | (cl >= LABEL_BINS - 1)).any():
        raise Mi355SegError(f"label_pick: class {int(cl[(cl < 0) | (cl >= LABEL_BINS - 1)][0])} is outside 0 .. 15")
    bad = (rk < 0) | (rk >= index.counts[cl])
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise Mi355SegError(f"label_pick: pick {i}: rank {int(rk[i])} is outside the {int(index.counts[cl[i]])} region voxels of class "
                            f"{int(cl[i])}")
    v = index.labels
    picks = torch.from_numpy(np.ascontiguousarray(np.stack([cl, rk], axis=1))).to(v.device)
    origins = torch.empty((cl.size, 3), dtype=torch.int32, device=v.device)
    D, H, W = index.shape
    lib().call("mi355seg_label_index_select", _p(v), D, H, W, *index.patch, _p(index.index), _p(picks), int(cl.size), _p(origins), _stream())
    return origins


_BAND_BASIS = {}                # (n, limit, device) -> (float32 [q, n] on the device, r, q)


def band_basis(n, limit=0.04):
    """Orthonormal real Fourier basis of the modes of a length-``n`` axis that the IS band split (train.py:76-88) does not let into
    its high band: ``(E float64 [q, n], r)``; the first ``r`` rows span the low band (``|f| < limit``), all ``q`` rows the modes that
    are not ``> limit``.  Membership is the reference's own comparison -- ``torch.fft.fftfreq(n).abs()`` against ``limit`` in
    float32 on the CPU -- so a mode exactly at the limit (n = 25, 50, 100 at 0.04) sits in neither band.  Per kept mode k:
    ``1/sqrt(n)`` for k = 0, ``(-1)^j/sqrt(n)`` for 2k = n, else the pair ``sqrt(2/n) cos(2 pi k j / n)``, ``sqrt(2/n) sin(...)``."""
    n = int(n)
    f = torch.fft.fftfreq(n).abs()
    below, above = (f < limit).tolist(), (f > limit).tolist()

    def rows(k):
        if k == 0:
            return [np.full(n, 1.0 / np.sqrt(n))]
        if 2 * k == n:
            return [np.where(np.arange(n) % 2 == 0, 1.0, -1.0) / np.sqrt(n)]
        w = 2.0 * np.pi * ((k * np.arange(n)) % n) / n
        return [np.sqrt(2.0 / n) * np.cos(w), np.sqrt(2.0 / n) * np.sin(w)]

    low, edge = [], []
    for k in range(n // 2 + 1):
        if below[k]:
            low += rows(k)
        elif not above[k]:
            edge += rows(k)
    basis = np.stack(low + edge) if low or edge else np.zeros((0, n))
    return basis, len(low)


def _band_basis_device(n, limit, device):
    key = (int(n), float(limit), device)
    hit = _BAND_BASIS.get(key)
    if hit is None:
        basis, r = band_basis(n, limit)
        hit = (torch.from_numpy(np.ascontiguousarray(basis, dtype=np.float32)).to(device), r, basis.shape[0])
        _BAND_BASIS[key] = hit
    return hit


def frequency_bands(x, limit=0.04):
    """The IS network's input split (train.py:76-88,198-201: low_pass_torch / high_pass_torch) of ``x`` [B,C,D,H,W] as ONE launch:
    ``(low, high)`` with ``low = P_H X P_W`` and ``high = (I - E_H) X (I - E_W)`` per [H,W] slice (definitions in
    include/mi355seg.h; ``high`` is not ``x - low``).  The per-axis bases come from ``band_basis`` and are uploaded once per
    (n, limit, device): the first eager call warms that cache, after which a call copies nothing and may be captured.  B and C
    may be 1 or 2 (for 2 the slices filter x0 + x1 and x0 - x1, the reference's all-axes forward transform)."""
    if x.requires_grad:
        raise NotImplementedError("frequency_bands: the bands are inputs of the network; no gradient flows through the split")
    _require_cuda(x, "frequency_bands input")
    if x.dim() != 5:
        raise Mi355SegError(f"frequency_bands: expected [B,C,D,H,W], got {tuple(x.shape)}")
    B, C, D, H, W = x.shape
    L = lib()
    if not (1 <= H <= 256 and 1 <= W <= 256 and D >= 1):
        raise Mi355SegError(f"frequency_bands: unsupported shape {tuple(x.shape)}: the device split filters axes of 1 .. 256 elements")
    if B not in (1, 2) or C not in (1, 2):
        raise Mi355SegError(f"frequency_bands: unsupported shape {tuple(x.shape)}: B and C must be 1 or 2 -- the reference's forward "
                            "transform also covers the batch and channel axes and is never inverted there (the upstream "
                            "all-axes-transform quirk), which is defined for lengths 1 and 2 only")
    (eh, rh, qh), (ew, rw, qw) = _band_basis_device(H, limit, x.device), _band_basis_device(W, limit, x.device)
    if not L.query("mi355seg_band_split_supported", B, C, D, H, W, rh, qh, rw, qw):
        raise Mi355SegError(f"frequency_bands: unsupported shape {tuple(x.shape)} at limit {limit}: an axis may keep at most 32 modes "
                            f"(H keeps {qh}, W keeps {qw})")
    x = x.contiguous()
    low, high = torch.empty_like(x), torch.empty_like(x)
    L.call("mi355seg_band_split_f32", _p(x), B, C, D, H, W, _p(eh), rh, qh, _p(ew), rw, qw, _p(low), _p(high), _stream())
    return low, high


def dice_sums(x, t, apply_sigmoid=False):
    """(sum a*b, sum a, sum b, sum a*a, sum b*b) as float64[5], a = sigmoid(x) if asked."""
    _require_cuda(x, "dice_sums input")
    x, t = x.contiguous(), t.contiguous().to(torch.float32)
    L = lib()
    ws = workspace(L.query("mi355seg_loss_ws_bytes", x.numel()), x.device)
    out = torch.empty(5, dtype=torch.float64, device=x.device)
    L.call("mi355seg_dice_sums_f32", _p(x), _p(t), x.numel(), int(bool(apply_sigmoid)), _p(out), _p(ws), ws.numel(), _stream())
    return out


class _DiceSums(Function):
    """S = (sum a*t, sum a, sum t, sum a*a, sum t*t) with autograd w.r.t. x (a = sigmoid(x) or x)."""

    @staticmethod
    def forward(ctx, x, t, apply_sigmoid):
        x, t = x.contiguous(), t.contiguous().to(torch.float32)
        out = dice_sums(x, t, apply_sigmoid)
        ctx.save_for_backward(x, t)
        ctx.apply_sigmoid = bool(apply_sigmoid)
        return out

    @staticmethod
    def backward(ctx, g):
        x, t = ctx.saved_tensors
        g = g.contiguous().to(torch.float64)
        dx = torch.empty_like(x)
        lib().call("mi355seg_dice_sums_bwd_f32", _p(x), _p(t), _p(g), x.numel(), int(ctx.apply_sigmoid), _p(dx), _stream())
        return dx, None, None


def dice_sums_autograd(x, t, apply_sigmoid=False):
    return _DiceSums.apply(x, t, apply_sigmoid)


class _DiceRows(Function):
    """S[r] = (sum a*t, sum a, sum t, sum a^p, sum t^p) over row r of a [R, L] view, every row in one launch, with autograd
    w.r.t. x (a = sigmoid(x) or x)."""

    @staticmethod
    def forward(ctx, x, t, apply_sigmoid, p):
        _require_cuda(x, "dice_rows input")
        x, t = x.contiguous().to(torch.float32), t.contiguous().to(torch.float32)
        R, Ln = x.shape
        if tuple(t.shape) != (R, Ln):
            raise Mi355SegError(f"dice_rows: target {tuple(t.shape)} must match input {tuple(x.shape)}")
        L = lib()
        ws = workspace(L.query("mi355seg_dice_rows_ws_bytes", R, Ln), x.device)
        out = torch.empty((R, 5), dtype=torch.float64, device=x.device)
        L.call("mi355seg_dice_rows_f32", _p(x), _p(t), R, Ln, int(bool(apply_sigmoid)), float(p), _p(out), _p(ws), ws.numel(), _stream())
        ctx.save_for_backward(x, t)
        ctx.cfg = (R, Ln, int(bool(apply_sigmoid)), float(p))
        return out

    @staticmethod
    def backward(ctx, g):
        x, t = ctx.saved_tensors
        R, Ln, sg, p = ctx.cfg
        g = g.contiguous().to(torch.float64)
        dx = torch.empty_like(x)
        lib().call("mi355seg_dice_rows_bwd_f32", _p(x), _p(t), _p(g), R, Ln, sg, float(p), _p(dx), _stream())
        return dx, None, None, None


def dice_rows_autograd(x, t, apply_sigmoid=False, p=2.0):
    """Per-row Dice sums of a [R, L] pair as float64 [R, 5] (one reduction launch + one finalise for all rows; more rows than
    a launch grid holds -- 65535 -- go in slices)."""
    R = x.shape[0]
    if R <= 65535:
        return _DiceRows.apply(x, t, apply_sigmoid, p)
    return torch.cat([_DiceRows.apply(x[i:i + 65535], t[i:i + 65535], apply_sigmoid, p) for i in range(0, R, 65535)], dim=0)


class _SoftmaxCh(Function):
    @staticmethod
    def forward(ctx, x):
        _require_cuda(x, "softmax input")
        x = x.contiguous()
        N, K = x.shape[0], x.shape[1]
        S = x[0, 0].numel()
        y = torch.empty_like(x)
        lib().call("mi355seg_softmax_ch_f32", _p(x), _p(y), N, K, S, _stream())
        ctx.save_for_backward(y)
        ctx.geom = (N, K, S)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        N, K, S = ctx.geom
        dy = dy.contiguous()
        dx = torch.empty_like(y)
        lib().call("mi355seg_softmax_ch_bwd_f32", _p(y), _p(dy), _p(dx), N, K, S, _stream())
        return dx


def softmax_channels(x):
    """torch.softmax(x, dim=1) for an NCDHW tensor of at most 16 classes (more: Mi355SegError)."""
    return _SoftmaxCh.apply(x)


class _CE3D(Function):
    @staticmethod
    def forward(ctx, logits, labels, weight, size_average):
        _require_cuda(logits, "cross_entropy_3D input")
        logits = logits.contiguous()
        labels = labels.contiguous().to(torch.int64)
        N, K = logits.shape[0], logits.shape[1]
        S = logits[0, 0].numel()
        if labels.numel() != N * S:
            raise ValueError(f"Expected target size {N * S}, got {labels.numel()}")
        if weight is not None:
            weight = weight.to(device=logits.device, dtype=torch.float32).contiguous()
        L = lib()
        ws = workspace(L.query("mi355seg_loss_ws_bytes", logits.numel()), logits.device)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        L.call("mi355seg_ce3d_fwd_f32", _p(logits), _p(labels), _p(weight), N, K, S, int(bool(size_average)), _p(loss),
               _p(ws), ws.numel(), _stream())
        ctx.save_for_backward(logits, labels, weight)
        ctx.cfg = (N, K, S, int(bool(size_average)))
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, labels, weight = ctx.saved_tensors
        N, K, S, sa = ctx.cfg
        g = g.contiguous().to(torch.float32)
        d = torch.empty_like(logits)
        lib().call("mi355seg_ce3d_bwd_f32", _p(logits), _p(labels), _p(weight), _p(g), N, K, S, sa, _p(d), _stream())
        return d, None, None, None


def cross_entropy_3d(logits, labels, weight=None, size_average=True):
    """loss_function.py:8-16: ``F.nll_loss(log_softmax(logits, 1), labels, weight, reduction="sum")``, divided by ``labels.numel()``
    when ``size_average``.  Labels: a voxel whose label lies outside ``[0, K)`` is IGNORED -- it adds nothing to the sum, its
    gradient row is exactly zero and the divisor stays ``labels.numel()``.  For ``-100`` that is F.nll_loss's own rule (its default
    ``ignore_index``); for any other such value (``K``, ``-1``, ``2**40``), where F.nll_loss raises, this call does NOT raise: a
    check would cost a device-to-host read per step, and the kernels never index the logits or ``weight`` with such a label."""
    return _CE3D.apply(logits, labels, weight, size_average)


# ----------------------------------------------------------------------------- reverse-attention gate
class _Gate(Function):
    """enc * (2 - sigmoid(t)) with a one-channel ``t``: ``(1 - sigmoid(t)).expand(C).mul(enc) + enc`` of
    RE_net.py:104-107 / ER_net.py in one pass (and one backward pass with the per-voxel channel reduction for dt)."""

    @staticmethod
    def forward(ctx, enc, t):
        enc, lde = cl_view(enc, "gate features", allow_bf16=False)
        t, ldt = cl_view(t, "gate map", allow_bf16=False)
        N, D, H, W, C = enc.shape
        if tuple(t.shape) != (N, D, H, W, 1):
            raise Mi355SegError(f"gate: map {tuple(t.shape)} must be one channel over the voxels of {tuple(enc.shape)}")
        y = torch.empty((N, D, H, W, C), dtype=enc.dtype, device=enc.device)
        lib().call("mi355seg_gate_fwd_f32", _p(enc), lde, _p(t), ldt, _p(y), C, N * D * H * W, C, _stream())
        ctx.save_for_backward(enc, t)
        ctx.cfg = (lde, ldt, N * D * H * W, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        enc, t = ctx.saved_tensors
        lde, ldt, rows, C = ctx.cfg
        dy, lddy = cl_view(dy, "gate grad")
        denc = torch.empty(enc.shape, dtype=enc.dtype, device=enc.device)
        dt = torch.empty(t.shape, dtype=t.dtype, device=t.device)
        lib().call("mi355seg_gate_bwd_f32", _p(dy), lddy, _p(enc), lde, _p(t), ldt, _p(denc), C, _p(dt), rows, C, _stream())
        return denc, dt


def reverse_attention_gate(enc, t):
    return _Gate.apply(enc, t)


# ----------------------------------------------------------------------------- selective fusion (ER_Net's SFConv)
class _SFPool(Function):
    """(x1 + x2).mean over the voxels -> [N, C]  (``fea_U.mean(-1).mean(-1).mean(-1)`` of ER_net.py:57-58)."""

    @staticmethod
    def forward(ctx, x1, x2):
        x1, ld1 = cl_view(x1, "sf_pool input", allow_bf16=False)
        x2, ld2 = cl_view(x2, "sf_pool input", allow_bf16=False)
        N, D, H, W, C = x1.shape
        if x2.shape != x1.shape:
            raise Mi355SegError(f"sf_pool: shapes differ: {tuple(x1.shape)} vs {tuple(x2.shape)}")
        V = D * H * W
        s = torch.empty((N, C), dtype=x1.dtype, device=x1.device)
        L = lib()
        ws = workspace(L.query("mi355seg_norm_ws_bytes", V, 1, C) + 8 * C + 512, x1.device)
        L.call("mi355seg_group_sums_f32", _p(x1), ld1, V, N, C, 1.0 / V, _p(s), 0, _p(ws), ws.numel(), _stream())
        L.call("mi355seg_group_sums_f32", _p(x2), ld2, V, N, C, 1.0 / V, _p(s), 1, _p(ws), ws.numel(), _stream())
        ctx.shape = (N, D, H, W, C)
        return s

    @staticmethod
    def backward(ctx, gs):
        N, D, H, W, C = ctx.shape
        V = D * H * W
        g = torch.empty((N, D, H, W, C), dtype=gs.dtype, device=gs.device)
        lib().call("mi355seg_broadcast_channels_f32", _p(gs.contiguous()), 1.0 / V, _p(g), C, V, N, C, _stream())
        return g, g


class _SFMix(Function):
    """x1 * a[n, c] + x2 * b[n, c]  (``(feas * attention_vectors).sum(dim=1)`` of ER_net.py:67-69)."""

    @staticmethod
    def forward(ctx, x1, x2, a, b):
        x1, ld1 = cl_view(x1, "sf_mix input", allow_bf16=False)
        x2, ld2 = cl_view(x2, "sf_mix input", allow_bf16=False)
        N, D, H, W, C = x1.shape
        a, b = a.contiguous(), b.contiguous()
        if x2.shape != x1.shape or a.numel() != N * C or b.numel() != N * C:
            raise Mi355SegError("sf_mix: x1 / x2 must match and the two attention vectors hold N*C values each")
        y = torch.empty((N, D, H, W, C), dtype=x1.dtype, device=x1.device)
        lib().call("mi355seg_mix_channels_f32", _p(x1), ld1, _p(a), _p(x2), ld2, _p(b), _p(y), C, D * H * W, N, C, _stream())
        ctx.save_for_backward(x1, x2, a, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        x1, x2, a, b = ctx.saved_tensors
        N, D, H, W, C = x1.shape
        V = D * H * W
        dy, lddy = cl_view(dy, "sf_mix grad")
        L = lib()
        dx1, dx2 = torch.empty_like(dy.contiguous()), None
        dx2 = torch.empty_like(dx1)
        L.call("mi355seg_scale_channels_f32", _p(dy), lddy, _p(a), _p(dx1), C, V, N, C, _stream())
        L.call("mi355seg_scale_channels_f32", _p(dy), lddy, _p(b), _p(dx2), C, V, N, C, _stream())
        ws = workspace(L.query("mi355seg_norm_ws_bytes", V, 1, C) + 8 * C + 512, dy.device)
        dyc = dy.contiguous()
        grads = []
        for x in (x1, x2):                                   # da[n, c] = sum_v dy * x
            prod = _mul(dyc, x.contiguous())
            d = torch.empty((N, C), dtype=dy.dtype, device=dy.device)
            L.call("mi355seg_group_sums_f32", _p(prod), C, V, N, C, 1.0, _p(d), 0, _p(ws), ws.numel(), _stream())
            grads.append(d.view_as(a))
        return dx1, dx2, grads[0], grads[1]


class _SoftmaxLast(Function):
    """softmax over the last dimension of a small 2-D tensor (the two-branch attention softmax, ER_net.py:66)."""

    @staticmethod
    def forward(ctx, x):
        _require_cuda(x, "softmax input")
        x = x.contiguous()
        y = torch.empty_like(x)
        lib().call("mi355seg_softmax_rows_f32", _p(x), _p(y), x.shape[0], x.shape[1], _stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dx = torch.empty_like(y)
        lib().call("mi355seg_softmax_rows_bwd_f32", _p(y), _p(dy.contiguous()), _p(dx), y.shape[0], y.shape[1], _stream())
        return dx


def sf_pool(x1, x2):
    return _SFPool.apply(x1, x2)


def sf_mix(x1, x2, a, b):
    return _SFMix.apply(x1, x2, a, b)


def softmax_last(x):
    return _SoftmaxLast.apply(x)


# ----------------------------------------------------------------------------- channel concat / repeat
class _CatChannels(Function):
    """torch.cat((a, b), dim=1) of the reference (vnet3d.py:101, residual_unet3d.py:183-209, unetr.py:286-293) in
    channel-last form: two strided slice copies into one buffer; the backward hands out the two slices as views."""

    @staticmethod
    def forward(ctx, a, b):
        a, lda = cl_view(a, "cat_channels first input")
        b, ldb = cl_view(b, "cat_channels second input")
        if a.shape[:4] != b.shape[:4]:
            raise Mi355SegError(f"cat_channels: spatial shapes differ: {tuple(a.shape)} vs {tuple(b.shape)}")
        N, D, H, W, Ca = a.shape
        Cb = b.shape[4]
        out = torch.empty((N, D, H, W, Ca + Cb), dtype=a.dtype, device=a.device)
        rows = N * D * H * W
        L = lib()
        if a.dtype != b.dtype:
            raise Mi355SegError(f"cat_channels: storage types differ: {a.dtype} vs {b.dtype}")
        L.call("mi355seg_copy_rows_" + _sfx(a), _p(a), lda, _p(out), Ca + Cb, rows, Ca, _stream())
        L.call("mi355seg_copy_rows_" + _sfx(a), _p(b), ldb, out.data_ptr() + out.element_size() * Ca, Ca + Cb, rows, Cb, _stream())
        ctx.ca = Ca
        return out

    @staticmethod
    def backward(ctx, dcat):
        return dcat[..., :ctx.ca], dcat[..., ctx.ca:]


def cat_channels(a, b):
    return _CatChannels.apply(a, b)


class _BnActCatScaled(Function):
    """cat((act(BatchNorm3d(y)), skip * scale), channels) -- V-Net's up-transition head (vnet3d.py:97-101: relu1(bn1(up_conv(x))),
    do2(skipx), torch.cat) -- as one node: the normalise pass writes the left channel slice of the concat buffer and the dropout
    scaling the right one (no separate Dropout3d tensor, no concat copies); the backward reads the two slices of the incoming
    gradient in place.  ``scale`` None: the skip is copied (eval mode / p = 0)."""

    @staticmethod
    def forward(ctx, y, gamma, beta, rmean, rvar, skip, scale, training, momentum, eps, act, slope):
        y, ldy = cl_view(y, "norm input")
        skip, lds = cl_view(skip, "concat skip input")
        if y.shape[:4] != skip.shape[:4] or y.dtype != skip.dtype:
            raise Mi355SegError(f"up-transition concat: {tuple(y.shape)} {y.dtype} vs {tuple(skip.shape)} {skip.dtype}")
        N, D, H, W, Cu = y.shape
        Cs = skip.shape[4]
        rows = N * D * H * W
        L = lib()
        dev = y.device
        ws = _norm_ws(L, rows, 1, Cu, dev)
        if training:
            mean, rstd = _batch_stats(L, y, ldy, rows, 1, Cu, eps, rmean, rvar, momentum, ws)
        else:
            mean, rstd = _running_stats(L, rmean, rvar, eps, Cu)
        both = torch.empty((N, D, H, W, Cu + Cs), dtype=y.dtype, device=dev)
        right = both.data_ptr() + both.element_size() * Cu
        _norm_act_fwd(L, y, ldy, mean, rstd, gamma, beta, _NO_RES, both.data_ptr(), Cu + Cs, rows, 1, Cu, act, slope)
        if scale is not None:
            scale = scale.contiguous().to(torch.float32)
            L.call("mi355seg_scale_channels_" + _sfx(y), _p(skip), lds, _p(scale), right, Cu + Cs, D * H * W, N, Cs, _stream())
        else:
            L.call("mi355seg_copy_rows_" + _sfx(y), _p(skip), lds, right, Cu + Cs, rows, Cs, _stream())
        ctx.save_for_backward(y, mean, rstd, gamma, beta, scale)
        ctx.cfg = (ldy, rows, Cu, Cs, act, slope, bool(training), (N, D, H, W))
        return both

    @staticmethod
    def backward(ctx, dboth):
        y, mean, rstd, gamma, beta, scale = ctx.saved_tensors
        ldy, rows, Cu, Cs, act, slope, training, (N, D, H, W) = ctx.cfg
        if not training:
            raise Mi355SegError(_EVAL_BN_BACKWARD)
        dboth, ldd = cl_view(_like(dboth, y), "up-transition concat grad")
        L = lib()
        dev = y.device
        ws = _norm_ws(L, rows, 1, Cu, dev)
        dy, dgamma, dbeta, _, _ = _norm_act_bwd(L, dboth, ldd, y, ldy, mean, rstd, gamma, beta, _NO_RES, rows, 1, Cu, act, slope, ws)
        right = dboth.data_ptr() + dboth.element_size() * Cu
        if scale is not None:
            dskip = torch.empty((N, D, H, W, Cs), dtype=y.dtype, device=dev)
            L.call("mi355seg_scale_channels_" + _sfx(y), right, ldd, _p(scale), _p(dskip), Cs, D * H * W, N, Cs, _stream())
        else:
            dskip = dboth[..., Cu:]
        return dy, dgamma, dbeta, None, None, dskip, None, None, None, None, None, None


def bn_act_cat_scaled(y, bn, skip, scale, act=ACT_NONE, slope=0.01):
    """cat((act(bn(y)), skip * scale), channel axis) for a layers.BatchNorm3d; ``scale`` = Dropout3d.draw_scale(...) or None."""
    if bn.momentum is None or not bn.affine or not bn.track_running_stats:
        raise NotImplementedError("bn_act_cat_scaled: BatchNorm3d must be affine with running statistics and a momentum")
    if bn.training:
        bump_counter(bn)
    return _BnActCatScaled.apply(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, skip, scale, bool(bn.training),
                                 float(bn.momentum), float(bn.eps), int(act), float(slope))


class _RepeatChannels(Function):
    """x.repeat(1, rep, 1, 1, 1) (vnet3d.py:55-56) in channel-last form."""

    @staticmethod
    def forward(ctx, x, rep):
        x, ldx = cl_view(x, "repeat_channels input")
        N, D, H, W, C = x.shape
        y = torch.empty((N, D, H, W, C * rep), dtype=x.dtype, device=x.device)
        lib().call("mi355seg_repeat_channels_" + _sfx(x), _p(x), ldx, _p(y), C * rep, N * D * H * W, C, rep, _stream())
        ctx.cfg = (C, rep)
        return y

    @staticmethod
    def backward(ctx, dy):
        C, rep = ctx.cfg
        dy, lddy = cl_view(dy, "repeat_channels grad")
        N, D, H, W, _ = dy.shape
        dx = torch.empty((N, D, H, W, C), dtype=dy.dtype, device=dy.device)
        lib().call("mi355seg_repeat_channels_bwd_" + _sfx(dy), _p(dy), lddy, _p(dx), C, N * D * H * W, C, rep, _stream())
        return dx, None


def repeat_channels(x, rep):
    return _RepeatChannels.apply(x, int(rep))


def _mul(a, b, out=None):
    """Elementwise product of two equally shaped contiguous fp32 tensors (no autograd; used inside Functions)."""
    a, b = a.contiguous(), b.contiguous()
    if a.shape != b.shape:
        raise Mi355SegError(f"mul: shapes differ: {tuple(a.shape)} vs {tuple(b.shape)}")
    if out is None:
        out = torch.empty_like(a)
    lib().call("mi355seg_mul_f32", _p(a), _p(b), _p(out), a.numel(), _stream())
    return out


def _softmax_keep(scores, keep, rows, Lr):
    """(softmax(scores), softmax(scores) * keep) over the last dim -- one launch; keep None: the second is the first."""
    probs = torch.empty_like(scores)
    if keep is None:
        lib().call("mi355seg_softmax_rows_f32", _p(scores), _p(probs), rows, Lr, _stream())
        return probs, probs
    keep = keep.contiguous()
    if keep.shape != scores.shape:
        raise Mi355SegError(f"attention: dropout mask {tuple(keep.shape)} does not match the scores {tuple(scores.shape)}")
    pd = torch.empty_like(scores)
    lib().call("mi355seg_softmax_rows_keep_f32", _p(scores), _p(keep), _p(probs), _p(pd), rows, Lr, _stream())
    return probs, pd


def _softmax_keep_bwd(probs, dpd, keep, rows, Lr):
    ds = torch.empty_like(probs)
    if keep is None:
        lib().call("mi355seg_softmax_rows_bwd_f32", _p(probs), _p(dpd), _p(ds), rows, Lr, _stream())
    else:
        lib().call("mi355seg_softmax_rows_keep_bwd_f32", _p(probs), _p(dpd), _p(keep.contiguous()), _p(ds), rows, Lr, _stream())
    return ds


# ---- element-wise dropout masks of one training step from ONE draw (r5).  nn.Dropout layers on token tensors (unetr.py:70-71,93,100,
# 124,133,149) each drew their keep / (1 - p) mask with a launch of their own: 37 per UNETR step.  Between two `dropout_pool_begin_step()`
# calls (engine.train_step makes them) the layers' requests are tallied; from the next step on one launch draws that many values and the
# layers take consecutive slices.  A request the pool cannot serve (no begin_step caller, a first step, a changed shape) draws by itself.
class _MaskPool(threading.local):
    def __init__(self):
        self.pools = {}                      # (p, device) -> [buffer or None, offset, values taken since the last begin_step]


_MASKS = _MaskPool()
# (values, device) -> the tensor of ones the pooled draw reads.  Entries are never dropped: a captured GraphedTrainStep has the buffer's
# address baked into its dropout node, so freeing it on a later request of another size (another model or patch shape in the same process)
# would let replays draw their masks from recycled memory.  One float per mask value and distinct size: a few MB per model.
_POOL_ONES = {}


def dropout_pool_begin_step():
    for (p, dev), st in _MASKS.pools.items():
        need = st[2]
        st[0], st[1], st[2] = None, 0, 0
        if need > 0 and not os.environ.get("MI355SEG_NO_MASK_POOL"):
            ones = _POOL_ONES.get((need, dev))
            if ones is None:
                ones = _POOL_ONES.setdefault((need, dev), torch.ones(need, device=dev))
            st[0] = torch.nn.functional.dropout(ones, p, True)       # keep / (1 - p), one launch for the whole step


def dropout_pool_take(shape, p, device, fallback):
    """A keep / (1 - p) mask of ``shape``: a slice of the step's pooled draw, else ``fallback()`` (an individual draw)."""
    n = 1
    for e in shape:
        n *= int(e)
    st = _MASKS.pools.setdefault((float(p), str(device)), [None, 0, 0])
    st[2] += n
    if st[0] is not None and st[1] + n <= st[0].numel() and n % 4 == 0:
        m = st[0][st[1]:st[1] + n].view(*shape)
        st[1] += n
        return m
    return fallback()


# ----------------------------------------------------------------------------- UNETR encoder ops
def _require_param(t, n, what):
    """A parameter the kernels read as ``n`` consecutive floats on the activations' device: checked here, before any launch (the kernels
    take a bare pointer, so a shorter / narrower / host tensor would be read out of bounds)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous():
        got = f"{tuple(t.shape)} {t.dtype} on {t.device}{'' if t.is_contiguous() else ', not contiguous'}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise Mi355SegError(f"{what}: expected {n} contiguous float32 values on the device, got {got}")


def _check_heads(E, heads, what):
    if heads <= 0 or E % heads:
        raise Mi355SegError(f"{what}: {heads} heads do not divide the embedding width {E}")


def _check_keep(keep, shape):
    if keep is not None:
        _require_cuda(keep, "attention dropout mask")
        if tuple(keep.shape) != tuple(shape):
            raise Mi355SegError(f"attention: dropout mask {tuple(keep.shape)} does not match the scores {tuple(shape)}")


def _lowp_now():
    """Inside autocast(torch.bfloat16) the token path's GEMMs take bf16 products (fp32 accumulate), as the reference's nn.Linear / matmul do
    under torch.autocast; a Function records the mode at its forward and keeps it for its backward."""
    return _AUTOCAST.stack[-1] == torch.bfloat16 and not os.environ.get("MI355SEG_TOKEN_GEMM_FP32")       # (the variable: fp32 products, for A/B timing)


def _gemm(A, a_rs, a_cs, a_b0, a_b1, B, b_rs, b_cs, b_b0, b_b1, C, c_rs, c_b0, c_b1, bias, M, N, K, nb0=1, nb1=1,
          alpha=1.0, relu=0, accumulate=0, lowp=False):
    L = lib()
    need = L.query("mi355seg_gemm_ws_bytes", M, N, K, nb0, nb1)
    ws = workspace(need, torch.device("cuda", torch.cuda.current_device())) if need else None
    L.call("mi355seg_gemm_lowp_f32" if lowp else "mi355seg_gemm_f32", A, a_rs, a_cs, a_b0, a_b1, B, b_rs, b_cs, b_b0, b_b1, C, c_rs, c_b0, c_b1, bias,
           M, N, K, nb0, nb1, alpha, relu, accumulate, _p(ws), ws.numel() if ws is not None else 0, _stream())


class _Linear(Function):
    """y[M,N] = x[M,K] @ W[N,K]^T + b, optionally followed -- inside the GEMM's epilogue -- by ReLU, an element-wise factor ``mask``
    (a dropout layer's keep / (1 - p)) and the sum with ``residual``: y = relu?(x W^T + b) * mask + residual (r5,
    mi355seg_linear_fwd_f32: the token encoder's out-projection + dropout + residual and its two feed-forward layers, unetr.py:98-100,
    120-138,159-166, as one launch each)."""

    @staticmethod
    def forward(ctx, x, w, b, relu, mask=None, residual=None):
        lowp = ctx.lowp = _lowp_now()
        _require_cuda(x, "linear input")
        shp = x.shape
        x2 = x.contiguous().view(-1, shp[-1])
        if w.dim() != 2 or w.shape[1] != shp[-1]:
            raise Mi355SegError(f"linear: weight {tuple(w.shape)} does not match an input of width {shp[-1]} (expected [N, {shp[-1]}])")
        w = w.contiguous()
        M, K, N = x2.shape[0], x2.shape[1], w.shape[0]
        _require_param(w, N * K, "linear weight")
        if b is not None:
            _require_param(b, N, "linear bias")
        y = torch.empty((M, N), dtype=x.dtype, device=x.device)
        if relu and residual is not None:
            raise Mi355SegError("linear: ReLU and a residual sum in one call are not supported (the backward keys the ReLU on the output)")
        if mask is None and residual is None:
            _gemm(_p(x2), K, 1, 0, 0, _p(w), 1, K, 0, 0, _p(y), N, 0, 0, _p(b), M, N, K, relu=int(relu), lowp=lowp)
        else:
            if mask is not None:
                mask = mask.contiguous()
                if mask.numel() != M * N or mask.dtype != x.dtype:
                    raise Mi355SegError(f"linear: mask of {mask.numel()} {mask.dtype} values for an output of {M} x {N} {x.dtype}")
            if residual is not None:
                residual = residual.contiguous()
                if residual.numel() != M * N or residual.dtype != x.dtype:
                    raise Mi355SegError(f"linear: residual of {residual.numel()} {residual.dtype} values for an output of {M} x {N} {x.dtype}")
            L = lib()
            need = L.query("mi355seg_gemm_ws_bytes", M, N, K, 1, 1)
            ws = workspace(need, x.device) if need else None
            L.call("mi355seg_linear_fwd_f32", int(lowp), _p(x2), K, _p(w), _p(b), int(relu), _p(mask), _p(residual), _p(y), M, N, K,
                   _p(ws), ws.numel() if ws is not None else 0, _stream())
        ctx.save_for_backward(x2, w, y if relu else None, mask)
        ctx.cfg = (shp, M, N, K, bool(relu), b is not None, residual is not None)
        return y.view(*shp[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        lowp = ctx.lowp
        x2, w, yrelu, mask = ctx.saved_tensors
        shp, M, N, K, relu, has_b, has_res = ctx.cfg
        dy2 = dy.contiguous().view(M, N)
        dres = dy if has_res else None                       # d(... + residual) / d residual = dy itself: no kernel
        L = lib()
        # r6: the whole backward as ONE launch -- dx = dyf W and dw = dyf^T x (+ db) are independent, latency-bound GEMMs at the token
        # encoder's sizes and run as two problems of one grid; the dropout factors and the ReLU gate (dyf = dy * mask * [y > 0]) are folded
        # into their loads of dy (mi355seg_linear_bwd_f32; bit-identical to the separate launches)
        if lowp and not os.environ.get("MI355SEG_NO_GEMM_PAIRS") and L.query("mi355seg_linear_bwd_supported_f32", 1, M, N, K) != 0 and \
                all(t is None or (t.is_contiguous() and t.data_ptr() % 16 == 0) for t in (dy2, mask, yrelu if relu else None, x2, w)):
            dx = torch.empty((M, K), dtype=dy2.dtype, device=dy2.device)
            dw = torch.empty_like(w)
            db = torch.empty(N, dtype=dy2.dtype, device=dy2.device) if has_b else None
            L.call("mi355seg_linear_bwd_f32", 1, _p(dy2), N, _p(mask), _p(yrelu) if relu else None, _p(x2), K, _p(w), _p(dx), _p(dw), _p(db), M, N, K, _stream())
            return dx.view(*shp), dw, db, None, None, dres
        if mask is not None:
            dy2 = _mul(dy2, mask.view(M, N))
        if relu:                                            # dy * 1[y > 0]: the ReLU backward kernel, keyed on the saved output (mask 0 => y 0 and dy 0)
            dy2 = _act_bwd(dy2, N, yrelu, N, _NO_RES, M, N, ACT_RELU, 0.0)
        dx = torch.empty((M, K), dtype=dy2.dtype, device=dy2.device)
        _gemm(_p(dy2), N, 1, 0, 0, _p(w), K, 1, 0, 0, _p(dx), K, 0, 0, None, M, K, N, lowp=lowp)
        # weight gradient; the bias gradient (column sums of dy) rides in the same launch on the token encoder's shapes
        dw = torch.empty_like(w)
        db = torch.empty(N, dtype=dy2.dtype, device=dy2.device) if has_b else None
        ws = workspace(max(L.query("mi355seg_gemm_ws_bytes", N, K, M, 1, 1), L.query("mi355seg_norm_ws_bytes", M, 1, N)), dy2.device)
        L.call("mi355seg_linear_wgrad_f32", int(lowp), _p(dy2), N, _p(x2), K, _p(dw), _p(db), M, N, K, _p(ws), ws.numel(), _stream())
        return dx.view(*shp), dw, db, None, None, dres


def linear(x, weight, bias=None, relu=False, mask=None, residual=None):
    """nn.Linear; ``mask`` / ``residual``: see _Linear (y = relu?(x W^T + b) * mask + residual in one launch)."""
    return _Linear.apply(x, weight, bias, relu, mask, residual)


def qkv_params_are_fused(wq, wk, wv, bq, bk, bv):
    """The three projections' parameters are consecutive slices of ONE buffer (models.three_d.unetr.SelfAttention seats them so): the
    [3E, K] weight and the [3E] bias of the fused projection exist in place."""
    if bq is None or bk is None or bv is None or wq.dim() != 2 or wq.shape != wk.shape or wq.shape != wv.shape:
        return False
    E, K = wq.shape
    ts = (wq, wk, wv, bq, bk, bv)
    if not all(t.is_contiguous() and t.dtype == torch.float32 and t.is_cuda for t in ts) or bq.numel() != E or bk.numel() != E or bv.numel() != E:
        return False
    if wk.data_ptr() != wq.data_ptr() + 4 * E * K or wv.data_ptr() != wq.data_ptr() + 8 * E * K:
        return False
    if bk.data_ptr() != bq.data_ptr() + 4 * E or bv.data_ptr() != bq.data_ptr() + 8 * E:
        return False
    room = lambda t, n: t.untyped_storage().nbytes() >= 4 * (t.storage_offset() + n)
    return room(wq, 3 * E * K) and room(bq, 3 * E)


class _LinearQKV(Function):
    """The query / key / value projections of unetr.py:60-75 as ONE GEMM on parameters that are slices of one buffer
    (qkv_params_are_fused): no concatenation of the weights in the forward, and the backward hands each parameter its rows of the fused
    weight / bias gradient as views (r6; the concatenated form cost two copy launches per layer and step)."""

    @staticmethod
    def forward(ctx, x, wq, wk, wv, bq, bk, bv):
        E, K = wq.shape
        wf = torch.as_strided(wq.detach(), (3 * E, K), (K, 1))
        bf = torch.as_strided(bq.detach(), (3 * E,), (1,))
        ctx.E = E
        return _Linear.forward(ctx, x, wf, bf, False)

    @staticmethod
    def backward(ctx, dy):
        dx, dw, db = _Linear.backward(ctx, dy)[:3]
        E = ctx.E
        return dx, dw[:E], dw[E:2 * E], dw[2 * E:], db[:E], db[E:2 * E], db[2 * E:]


def linear_qkv(x, wq, wk, wv, bq, bk, bv):
    """[x Wq^T + bq | x Wk^T + bk | x Wv^T + bv] for parameters seated as slices of one buffer; see _LinearQKV."""
    return _LinearQKV.apply(x, wq, wk, wv, bq, bk, bv)


class _LayerNorm(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        _require_cuda(x, "layer_norm input")
        shp = x.shape
        E = shp[-1]
        _require_param(gamma, E, "layer_norm weight")
        _require_param(beta, E, "layer_norm bias")
        x2 = x.contiguous().view(-1, E)
        rows = x2.shape[0]
        y = torch.empty_like(x2)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        lib().call("mi355seg_layernorm_fwd_f32", _p(x2), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, E, eps, _stream())
        ctx.save_for_backward(x2, gamma, mean, rstd)
        ctx.shp = shp
        return y.view(*shp)

    @staticmethod
    def backward(ctx, dy):
        x2, gamma, mean, rstd = ctx.saved_tensors
        rows, E = x2.shape
        dy2 = dy.contiguous().view(rows, E)
        dx = torch.empty_like(x2)
        dg = torch.empty(E, dtype=torch.float32, device=x2.device)
        db = torch.empty(E, dtype=torch.float32, device=x2.device)
        lib().call("mi355seg_layernorm_bwd_f32", _p(dy2), _p(x2), _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dg), _p(db), rows, E, _stream())
        return dx.view(*ctx.shp), dg, db, None


class _LayerNormFork(Function):
    """(LayerNorm(x), x): the norm of a tensor that also continues unchanged -- a pre-norm transformer block's x + f(LN(x)) (unetr.py:159-166).
    The backward writes d(x) = d(pass-through) + LN-backward(d(norm)) from the kernel that forms the LayerNorm gradient
    (mi355seg_layernorm_bwd_add_f32); autograd would add the two with a launch of its own."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        _require_cuda(x, "layer_norm input")
        shp = x.shape
        E = shp[-1]
        _require_param(gamma, E, "layer_norm weight")
        _require_param(beta, E, "layer_norm bias")
        x2 = x.contiguous().view(-1, E)
        rows = x2.shape[0]
        y = torch.empty_like(x2)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        lib().call("mi355seg_layernorm_fwd_f32", _p(x2), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, E, eps, _stream())
        ctx.save_for_backward(x2, gamma, mean, rstd)
        ctx.shp = shp
        ctx.set_materialize_grads(False)
        return y.view(*shp), x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dpass):
        x2, gamma, mean, rstd = ctx.saved_tensors
        rows, E = x2.shape
        if dy is None:
            return dpass, None, None, None
        dy2 = dy.contiguous().view(rows, E)
        add = dpass.contiguous().view(rows, E) if dpass is not None else None
        dx = torch.empty_like(x2)
        dg = torch.empty(E, dtype=torch.float32, device=x2.device)
        db = torch.empty(E, dtype=torch.float32, device=x2.device)
        lib().call("mi355seg_layernorm_bwd_add_f32", _p(dy2), _p(x2), _p(gamma), _p(mean), _p(rstd), _p(add), _p(dx), _p(dg), _p(db), rows, E, _stream())
        return dx.view(*ctx.shp), dg, db, None


def layer_norm_fork(x, gamma, beta, eps=1e-5):
    """(LayerNorm(x), x) for a tensor that is normalised and also continues unchanged; see _LayerNormFork."""
    return _LayerNormFork.apply(x, gamma, beta, float(eps))


def layer_norm(x, gamma, beta, eps=1e-5):
    return _LayerNorm.apply(x, gamma, beta, float(eps))


class _Attention(Function):
    """softmax(Q K^T / sqrt(d)) V per (batch, head) with Q,K,V stored [B, P, H*d] (unetr.py:74-98).
    ``keep`` (optional, [B,H,P,P], already divided by 1-p) is the attention-dropout mask."""

    @staticmethod
    def forward(ctx, q, k, v, heads, keep):
        lowp = ctx.lowp = _lowp_now()
        _require_cuda(q, "attention input")
        if q.dim() != 3 or k.shape != q.shape or v.shape != q.shape:
            raise Mi355SegError(f"attention: q, k, v must be three [B, P, E] tensors of one shape, got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
        _require_cuda(k, "attention input")
        _require_cuda(v, "attention input")
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        B, P, E = q.shape
        _check_heads(E, heads, "attention")
        _check_keep(keep, (B, heads, P, P))
        d = E // heads
        alpha = 1.0 / (d ** 0.5)
        scores = torch.empty((B, heads, P, P), dtype=q.dtype, device=q.device)
        _gemm(_p(q), E, 1, P * E, d, _p(k), 1, E, P * E, d, _p(scores), P, heads * P * P, P * P, None, P, P, d, B, heads, alpha, lowp=lowp)
        probs, pd = _softmax_keep(scores, keep, B * heads * P, P)
        ctxl = torch.empty((B, P, E), dtype=q.dtype, device=q.device)
        _gemm(_p(pd), P, 1, heads * P * P, P * P, _p(v), E, 1, P * E, d, _p(ctxl), E, P * E, d, None, P, d, P, B, heads, lowp=lowp)
        ctx.save_for_backward(q, k, v, probs, keep, pd if keep is not None else None)
        ctx.cfg = (B, P, E, heads, d, alpha)
        return ctxl

    @staticmethod
    def backward(ctx, do):
        lowp = ctx.lowp
        q, k, v, probs, keep, pd = ctx.saved_tensors
        B, P, E, heads, d, alpha = ctx.cfg
        do = do.contiguous()
        if pd is None:
            pd = probs
        HPP, PP = heads * P * P, P * P
        dpd = torch.empty_like(probs)                                   # dP = dO V^T
        _gemm(_p(do), E, 1, P * E, d, _p(v), 1, E, P * E, d, _p(dpd), P, HPP, PP, None, P, P, d, B, heads, lowp=lowp)
        dv = torch.empty_like(v)                                        # dV = Pd^T dO
        _gemm(_p(pd), 1, P, HPP, PP, _p(do), E, 1, P * E, d, _p(dv), E, P * E, d, None, P, d, P, B, heads, lowp=lowp)
        ds = _softmax_keep_bwd(probs, dpd, keep, B * heads * P, P)
        dq = torch.empty_like(q)                                        # dQ = alpha dS K
        _gemm(_p(ds), P, 1, HPP, PP, _p(k), E, 1, P * E, d, _p(dq), E, P * E, d, None, P, d, P, B, heads, alpha, lowp=lowp)
        dk = torch.empty_like(k)                                        # dK = alpha dS^T Q
        _gemm(_p(ds), 1, P, HPP, PP, _p(q), E, 1, P * E, d, _p(dk), E, P * E, d, None, P, d, P, B, heads, alpha, lowp=lowp)
        return dq, dk, dv, None, None


class _AttentionQKV(Function):
    """_Attention on a FUSED projection output qkv[B, P, 3E] = (Q | K | V) (one GEMM for the three projections of unetr.py:60-75):
    the batched GEMMs read the three channel slices in place (row pitch 3E) and the backward writes dQ | dK | dV into the slices of
    one [B, P, 3E] gradient, so the projection's backward is one input-gradient GEMM, one weight-gradient GEMM and one bias sum."""

    @staticmethod
    def forward(ctx, qkv, heads, keep):
        lowp = ctx.lowp = _lowp_now()
        _require_cuda(qkv, "attention input")
        if qkv.dim() != 3 or qkv.shape[2] % 3:
            raise Mi355SegError(f"attention_qkv: expected the fused projection [B, P, 3E], got {tuple(qkv.shape)}")
        qkv = qkv.contiguous()
        B, P, E3 = qkv.shape
        E = E3 // 3
        _check_heads(E, heads, "attention_qkv")
        _check_keep(keep, (B, heads, P, P))
        d = E // heads
        alpha = 1.0 / (d ** 0.5)
        q, k, v = _p(qkv), _p(qkv) + 4 * E, _p(qkv) + 8 * E
        scores = torch.empty((B, heads, P, P), dtype=qkv.dtype, device=qkv.device)
        _gemm(q, E3, 1, P * E3, d, k, 1, E3, P * E3, d, _p(scores), P, heads * P * P, P * P, None, P, P, d, B, heads, alpha, lowp=lowp)
        probs, pd = _softmax_keep(scores, keep, B * heads * P, P)
        ctxl = torch.empty((B, P, E), dtype=qkv.dtype, device=qkv.device)
        _gemm(_p(pd), P, 1, heads * P * P, P * P, v, E3, 1, P * E3, d, _p(ctxl), E, P * E, d, None, P, d, P, B, heads, lowp=lowp)
        ctx.save_for_backward(qkv, probs, keep, pd if keep is not None else None)
        ctx.cfg = (B, P, E, heads, d, alpha)
        return ctxl

    @staticmethod
    def backward(ctx, do):
        lowp = ctx.lowp
        qkv, probs, keep, pd = ctx.saved_tensors
        B, P, E, heads, d, alpha = ctx.cfg
        E3 = 3 * E
        q, k, v = _p(qkv), _p(qkv) + 4 * E, _p(qkv) + 8 * E
        do = do.contiguous()
        if pd is None:
            pd = probs
        HPP, PP = heads * P * P, P * P
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = _p(dqkv), _p(dqkv) + 4 * E, _p(dqkv) + 8 * E
        dpd = torch.empty_like(probs)                                   # dP = dO V^T
        L = lib()
        # r6: the two pairs of independent GEMMs (dP with dV: both read dO; dQ with dK: both read dS) as one launch each
        # (the query looks at sizes only; the pair kernel also reads 16 bytes per lane along k, so every operand must start on a 16-byte boundary
        # with pitches that keep its rows there -- a contiguous view at an odd offset into a larger buffer takes the two launches)
        pairs = lowp and not os.environ.get("MI355SEG_NO_GEMM_PAIRS") and E % 4 == 0 and P % 4 == 0 and \
            all(t.data_ptr() % 16 == 0 for t in (qkv, do, pd, probs)) and \
            L.query("mi355seg_gemm_pair_supported_f32", P, P, d, P, d, P, B, heads) != 0 and L.query("mi355seg_gemm_pair_supported_f32", P, d, P, P, d, P, B, heads) != 0
        if pairs:
            L.call("mi355seg_gemm_pair_lowp_f32", _p(do), E, 1, P * E, d, v, 1, E3, P * E3, d, _p(dpd), P, HPP, PP, P, P, d, 1.0,
                   _p(pd), 1, P, HPP, PP, _p(do), E, 1, P * E, d, dv, E3, P * E3, d, P, d, P, 1.0, B, heads, _stream())
        else:
            _gemm(_p(do), E, 1, P * E, d, v, 1, E3, P * E3, d, _p(dpd), P, HPP, PP, None, P, P, d, B, heads, lowp=lowp)
            _gemm(_p(pd), 1, P, HPP, PP, _p(do), E, 1, P * E, d, dv, E3, P * E3, d, None, P, d, P, B, heads, lowp=lowp)         # dV = Pd^T dO
        ds = _softmax_keep_bwd(probs, dpd, keep, B * heads * P, P)
        if pairs:
            L.call("mi355seg_gemm_pair_lowp_f32", _p(ds), P, 1, HPP, PP, k, E3, 1, P * E3, d, dq, E3, P * E3, d, P, d, P, alpha,
                   _p(ds), 1, P, HPP, PP, q, E3, 1, P * E3, d, dk, E3, P * E3, d, P, d, P, alpha, B, heads, _stream())
        else:
            _gemm(_p(ds), P, 1, HPP, PP, k, E3, 1, P * E3, d, dq, E3, P * E3, d, None, P, d, P, B, heads, alpha, lowp=lowp)      # dQ = alpha dS K
            _gemm(_p(ds), 1, P, HPP, PP, q, E3, 1, P * E3, d, dk, E3, P * E3, d, None, P, d, P, B, heads, alpha, lowp=lowp)      # dK = alpha dS^T Q
        return dqkv, None, None


def attention_qkv(qkv, heads, keep=None):
    """Multi-head attention on the fused projection output [B, P, 3E] (fp32)."""
    return _AttentionQKV.apply(qkv, int(heads), keep)


def attention(q, k, v, heads, keep=None):
    return _Attention.apply(q, k, v, int(heads), keep)
