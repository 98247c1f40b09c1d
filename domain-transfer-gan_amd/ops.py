"""torch.autograd.Function wrappers over the C ABI (libacgan_hip.so).

PyTorch is plumbing here: it owns device memory (caching allocator), the stream and the
autograd tape; every forward/backward computation on activations is a HIP kernel reached
through ctypes.  Internal activation layout: fp32 NHWC with channels padded to 16 ("C16"),
carried as torch tensors of shape (N, H, W, Cp) — or (N, Cp) for latent / MLP activations.

There is no CPU path: tensors must live on a ROCm device and the library must load.
"""
import collections
import ctypes

import torch

from . import _lib
from ._lib import ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_SIGMOID, PAD_ZERO, PAD_REFLECT, ConvDesc  # noqa: F401

_VP = ctypes.c_void_p


def cpad(c):
    """stored channel count for `c` real channels (feature maps, latents: multiples of 16)"""
    return (int(c) + 15) // 16 * 16


def cimg(c):
    """stored channel count of an IMAGE tensor (network inputs / outputs, their gradients): 4 for up to 4 real channels
    ("C4": one 16-byte load per pixel instead of a 64-byte row that is three quarters padding), else as cpad.  Only the thin
    side of a thin convolution layer reads or writes such a tensor (conv_thin_sides); everything else sees multiples of 16."""
    return 4 if int(c) <= 4 else cpad(c)


def conv_thin_sides(Or, Ir, K):
    """-> (input may be stored C4, output is stored C4) for a Conv2d of real widths Ir -> Or: the library's thin-channel
    kernels (K flattened over (tap, 4 channels)) take the thin side of a layer with K > 1 whose other side is wider"""
    ti, to = 1 <= Ir <= 4, 1 <= Or <= 4
    return (ti and not to and K > 1), (to and not ti and K > 1)


def _ptr(t):
    return None if t is None else _VP(t.data_ptr())


def _stream():
    return _VP(torch.cuda.current_stream().cuda_stream)


_NO_CPU_PATH = "acgan_hip kernels need tensors on a ROCm device (got %s); there is no CPU path"


def _check(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.AcgError(_NO_CPU_PATH % t.device)
        if t.dtype != torch.float32:
            raise _lib.AcgError("acgan_hip kernels are fp32 (got %s)" % t.dtype)
        if not t.is_contiguous():
            raise _lib.AcgError("non-contiguous tensor reached a kernel")


def channel_table(what, error, noun, table, C, most, device, none_if_empty=False, ordered=False, cast=False):
    """A per-channel table (C, T) - the thresholds of fss and minkowski, the edges of the marginal scores - as the kernels
    take it -> a contiguous float32 tensor on `device`, moved there once (None: left where it is, so that an entry point which
    takes host arrays or device tensors uploads the former itself and lets _check refuse a tensor on the host);
    error("<what>: <noun> ...") unless it is (C, T) with 1 <= T <= most (none_if_empty: T = 0 passes and gives None).  A host
    array is copied to float32 (the caller's may be read-only) and fully checked: where `ordered`, every channel finite and
    non-decreasing (repeats allowed).  A tensor is checked for its shape and for float32 (cast: converted instead) and is
    otherwise taken as it is: its order is the caller's contract, nothing is read back to inspect it."""
    import numpy as np
    host = None
    if not torch.is_tensor(table):
        host = np.array(table, dtype=np.float32, order="C")
        table = torch.from_numpy(host)
    elif cast:
        table = table.to(torch.float32)
    least = 0 if none_if_empty else 1
    if table.dim() != 2 or table.size(0) != C or not least <= table.size(1) <= most or table.dtype != torch.float32:
        raise error("%s: %s must be (C, T) float32 with C=%d and %d <= T <= %d (got %s %s)"
                    % (what, noun, C, least, most, tuple(table.shape), table.dtype))
    if ordered and host is not None and (not np.all(np.isfinite(host)) or np.any(host[:, 1:] < host[:, :-1])):
        raise error("%s: %s must be finite and non-decreasing per channel" % (what, noun))
    if not table.size(1):
        return None
    table = table.detach().contiguous()
    return table if device is None else table.to(device)


_WS = {}


def workspace(nbytes, slot=0):
    """Stream-ordered scratch (one buffer per device/slot, grown on demand)."""
    dev = torch.cuda.current_device()
    buf = _WS.get((dev, slot))
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device="cuda")
        _WS[(dev, slot)] = buf
    return buf


CONFIG_EPOCH = 0  # bumped whenever the packed-weight format changes (impl / precision switch)
_PRECISION = "bf16x3"  # the library default (acg_set_conv_precision)


def set_conv_impl(name):
    """'mfma' (product path) or 'direct' (naive HIP kernels, cross-check only)."""
    global CONFIG_EPOCH
    _lib.call("acg_set_conv_impl", {"mfma": _lib.IMPL_MFMA, "direct": _lib.IMPL_DIRECT}[name])
    CONFIG_EPOCH += 1


def set_precision(name):
    """Arithmetic of the MFMA convolution kernels: 'bf16x3' (default: each fp32 operand split into bf16 hi + lo in
    LDS, lo*hi + hi*lo + hi*hi on the bf16 matrix pipe, fp32 accumulate — operands keep 16 mantissa bits, ~4e-6 rms
    per conv, well inside the 1e-3 parity bar), 'f32' (exact-fp32 matrix pipe, the strict mode the tight tests pin the
    kernels with) or 'bf16' (operands rounded to bf16, fp32 accumulate: a numerics PROBE for tests/test_hip_bf16.py, not offered by
    bench.py / options.py — no faster than bf16x3 with fp32 tensors, DESIGN_LOG.md A.4).  HBM
    tensors stay fp32 in every mode."""
    global CONFIG_EPOCH, _PRECISION
    _lib.call("acg_set_conv_precision", {"f32": _lib.PREC_F32, "bf16": _lib.PREC_BF16, "bf16x3": _lib.PREC_BF16X3}[name])
    _PRECISION = name
    CONFIG_EPOCH += 1


def get_precision():
    return _PRECISION


# ----------------------------------------------------------------------------------------------
# layout
# ----------------------------------------------------------------------------------------------
class ToNHWC(torch.autograd.Function):
    """(N,C,H,W) -> (N,H,W,Cp)"""

    @staticmethod
    def forward(ctx, x, img=False):
        """img: the tensor is an image that goes into a convolution (cimg: C4 storage for <= 4 channels)"""
        x = x.contiguous()
        _check(x)
        N, C, H, W = x.shape
        ctx.C = C
        Cp = cimg(C) if img else cpad(C)
        y = torch.empty((N, H, W, Cp), device=x.device, dtype=torch.float32)
        _lib.call("acg_nchw_to_nhwc16", _ptr(x), _ptr(y), N, C, H, W, Cp, _stream())
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        N, H, W, Cp = g.shape
        d = torch.empty((N, ctx.C, H, W), device=g.device, dtype=torch.float32)
        _lib.call("acg_nhwc16_to_nchw", _ptr(g), _ptr(d), N, ctx.C, H, W, Cp, _stream())
        return d, None


class ToNCHW(torch.autograd.Function):
    """(N,H,W,Cp) -> (N,C,H,W)"""

    @staticmethod
    def forward(ctx, x, C):
        x = x.contiguous()
        _check(x)
        N, H, W, Cp = x.shape
        ctx.Cp = Cp
        y = torch.empty((N, C, H, W), device=x.device, dtype=torch.float32)
        _lib.call("acg_nhwc16_to_nchw", _ptr(x), _ptr(y), N, C, H, W, Cp, _stream())
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        N, C, H, W = g.shape
        d = torch.empty((N, H, W, ctx.Cp), device=g.device, dtype=torch.float32)
        _lib.call("acg_nchw_to_nhwc16", _ptr(g), _ptr(d), N, C, H, W, ctx.Cp, _stream())
        return d, None


class Concat(torch.autograd.Function):
    """torch.cat((a, b), 1) on C16 tensors (model.py:410, 472)."""

    @staticmethod
    def forward(ctx, a, b, Ca, Cb):
        a, b = a.contiguous(), b.contiguous()
        _check(a, b)
        N, H, W, Cap = a.shape
        Cbp = b.shape[3]
        Cdp = cimg(Ca + Cb)   # (an image again: the encoder's first layer takes it)
        ctx.dims = (Ca, Cap, Cb, Cbp, Cdp)
        y = torch.empty((N, H, W, Cdp), device=a.device, dtype=torch.float32)
        _lib.call("acg_concat_channels", _ptr(a), Ca, Cap, _ptr(b), Cb, Cbp, _ptr(y), Cdp, N * H * W, _stream())
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        Ca, Cap, Cb, Cbp, Cdp = ctx.dims
        N, H, W, _ = g.shape
        ga = torch.empty((N, H, W, Cap), device=g.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        gb = torch.empty((N, H, W, Cbp), device=g.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        if ga is not None or gb is not None:
            _lib.call("acg_split_channels", _ptr(g), Cdp, _ptr(ga), Ca, Cap, _ptr(gb), Cb, Cbp, N * H * W, _stream())
        return ga, gb, None, None


# ----------------------------------------------------------------------------------------------
# convolutions
# ----------------------------------------------------------------------------------------------
class PackedConv(object):
    """Device-side packed forms of one conv weight (+ padded bias); see acg_pack_conv_weight."""

    def __init__(self, weight, bias, Ci, Co):
        Or, Ir, K, _ = weight.shape
        self.Or, self.Ir, self.K, self.Ci, self.Co = Or, Ir, K, Ci, Co   # Ci / Co: the PACKED widths (multiples of 16)
        # stored widths of the layer's input / output tensors: C4 on the thin side of a thin layer (image tensors)
        tin, tout = conv_thin_sides(Or, Ir, K)
        self.Cis, self.Cos = (4 if tin else Ci), (4 if tout else Co)
        dev = weight.device
        self.wf = torch.empty(_lib.query("acg_packed_wf_elems", K, Ci, Co), device=dev, dtype=torch.float32)
        self.wb = torch.empty(_lib.query("acg_packed_wb_elems", K, Ci, Co), device=dev, dtype=torch.float32)
        self.bias = None
        self.refresh(weight, bias)

    def refresh(self, weight, bias):
        w = weight.detach().contiguous()
        _check(w)
        _lib.call("acg_pack_conv_weight", _ptr(w), self.Or, self.Ir, self.K, self.Ci, self.Co, _ptr(self.wf), _ptr(self.wb),
                  _stream())
        self.refresh_bias(bias)

    def refresh_bias(self, bias):
        w = self.wf
        if bias is not None:
            n = bias.numel()
            npad = cpad(n)
            if n == npad and bias.is_contiguous() and bias.dtype == torch.float32:
                self.bias = bias.detach()   # no padding needed: the kernels read the parameter itself
            else:
                if self.bias is None or self.bias.data_ptr() == bias.data_ptr():
                    self.bias = torch.empty(npad, device=w.device, dtype=torch.float32)
                _lib.call("acg_pad_vector", _ptr(bias.detach()), n, _ptr(self.bias), npad, _stream())


def repack_many(entries):
    """entries: [(PackedConv, weight, bias)] whose parameters the optimiser just changed: refresh the packed copies IN PLACE —
    the regular layers of the list in one launch (acg_pack_conv_weights_multi), thin layers and the exact-fp32 mode layer by
    layer.  (In place: nothing of a step reads a network's old weights after its Adam update.)"""
    multi = []
    for pk, w, b in entries:
        if _lib.query("acg_pack_conv_weights_multi_supported", pk.Or, pk.Ir, pk.K):
            multi.append((pk, w, b))
        else:
            pk.refresh(w, b)
    if not multi:
        return
    arr = (_lib.PackItem * len(multi))()
    keep = []
    for i, (pk, w, b) in enumerate(multi):
        wd = w.detach().contiguous()
        _check(wd)
        keep.append(wd)
        arr[i].w, arr[i].wf, arr[i].wb = wd.data_ptr(), pk.wf.data_ptr(), pk.wb.data_ptr()
        arr[i].Or, arr[i].Ir, arr[i].K, arr[i].Ci, arr[i].Co = pk.Or, pk.Ir, pk.K, pk.Ci, pk.Co
    _lib.call("acg_pack_conv_weights_multi", arr, len(multi), _stream())
    _fused("packed_weights_multi", len(multi))
    for pk, w, b in multi:
        pk.refresh_bias(b)


class ConvTimer(object):
    """bench.py hook: HIP events (on the launch stream) around the launches of ONE pass ("fwd", "dgrad", "wgrad", or
    "dgrad_sums": the data-gradient launches that also emit the backward sums of the norm in front, ops.NormSums) of ONE
    conv shape, so the roofline numerator/denominator come from the live timed region."""

    def __init__(self, match, kind="fwd"):
        self.match, self.kind, self.events, self.kernel = match, kind, [], None

    class _Span(object):
        def __init__(self, timers, mid=False):
            self.timers, self.em = timers, None
            if timers:
                self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if mid:   # weight gradient: the library records this event between its main kernel and the split-K reduction
                    self.em = torch.cuda.Event(enable_timing=True)
                    self.em.record()   # (creates the hipEvent_t; the library's record replaces this timestamp)
                    _lib.call("acg_debug_mid_event", ctypes.c_void_p(self.em.cuda_event))
                self.e0.record()

        def done(self):
            if self.timers:
                self.e1.record()
                if self.em is not None:
                    _lib.call("acg_debug_mid_event", None)   # (an entry point without a reduction must not leave it armed)
                k = _lib.query("acg_last_kernel").decode()   # what the dispatcher actually launched
                for t in self.timers:
                    t.events.append((self.e0, self.e1, k, self.em))
                    t.kernel = k

    @staticmethod
    def span(kind, d):
        """-> object whose done() closes the bracket (a no-op unless a timer of this kind matches descriptor d)"""
        return ConvTimer._Span([t for t in CONV_TIMERS if t.kind == kind and t.match(d)], mid=(kind == "wgrad"))

    def ms(self):
        return [a.elapsed_time(b) for a, b, _, _ in self.events]

    def ms_main(self):
        """the main kernel alone where the pass has a second launch behind it (weight gradient: its split-K reduction)"""
        return [self._main(a, b, m) for a, b, _, m in self.events]

    @staticmethod
    def _main(a, b, m):
        v = a.elapsed_time(m) if m is not None else -1.0
        return v if v > 0.0 else a.elapsed_time(b)   # (not recorded by the library: the place-holder stamp lies before `a`)

    def by_kernel(self, main=False):
        """-> {kernel label: [ms per launch]} (one pass of one layer can be served by several template instances)"""
        out = {}
        for a, b, k, m in self.events:
            out.setdefault(k, []).append(self._main(a, b, m) if main else a.elapsed_time(b))
        return out


CONV_TIMERS = []   # bench.py appends ConvTimer objects; every matching forward launch is bracketed by HIP events


def conv_desc(N, Hi, Wi, Ci, Co, K, stride, pad, pad_mode, Cir=0, Cor=0):
    """Cir / Cor: real (unpadded) channel counts — let the library pick the thin-channel kernels (0 = unknown)."""
    Ho = (Hi + 2 * pad - K) // stride + 1
    Wo = (Wi + 2 * pad - K) // stride + 1
    return ConvDesc(N, Hi, Wi, Ci, Ho, Wo, Co, K, stride, pad, pad_mode, Cir, Cor)


STATS_ROWS = 128
CONV_STATS_ENABLED = True  # False: the unfused path (the tests' reference)


class ConvStats(object):
    """Slot the caller hands to a convolution AND to the (Cond)InstanceNorm behind it (modules._run_stages / _run_block): where the
    kernel supports it the convolution's epilogue emits the norm's per-tile statistics (acg_conv2d_fwd_stats) and leaves
    them here: `part` [N][Ho*Wo/STATS_ROWS][2][Co] (mean, M2 per 128-pixel tile), else None."""

    def __init__(self):
        self.part = None


class SkipGrad(object):
    """Slot shared by a residual block's first convolution (whose identity output feeds the skip connection) and the
    block's last norm: the norm's backward returns dy itself as the gradient of the skip input and leaves the sign bitmask
    of the block output here; the convolution's data-gradient epilogue adds dy where the bit is set — the skip gradient
    dy * (y > 0) is never written to memory."""

    def __init__(self):
        self.mask = self.dy = None

    def take(self, dskip):
        """-> (skip gradient, sign bitmask or None).  When the norm left its gradient un-materialised (mask set), what autograd
        delivers must be that very tensor: anything else (a hook, a clone, a sum with another gradient) cannot be told apart
        from dy * mask any more, so it is refused instead of being added unmasked."""
        mask, dy = self.mask, self.dy
        self.mask = self.dy = None
        if mask is None:
            return dskip, None
        if dy is None or dy.data_ptr() != dskip.data_ptr() or dy.shape != dskip.shape:
            raise _lib.AcgError("the un-materialised skip gradient of a residual block was altered on its way to the block's "
                                "first convolution (tensor hook / extra consumer of the skip tensor); set ops.LAZY_DRES = False")
        return dskip, mask


# Parameter gradients straight into .grad: a model.FlatNet marks its parameters `_acg_direct_grad`; their .grad tensors are
# preset views of the network's flat gradient buffer, and the weight-gradient / norm-parameter kernels ADD into them
# (accumulate=1) instead of returning a fresh tensor for autograd's AccumulateGrad to add with one more kernel per parameter
# (564 five-microsecond launches per training step).  The Function then returns None for that parameter, so the
# post-accumulate hooks of the data-parallel exchange (dist.hook_params) are fired by hand.
DIRECT_GRAD = True   # False: the unfused path (the tests' reference)


def _direct_grad(*params):
    """-> list of .grad targets when EVERY given parameter (None entries skipped) takes direct accumulation, else None"""
    if not DIRECT_GRAD:
        return None
    out = []
    for p in params:
        if p is None:
            out.append(None)
            continue
        g = getattr(p, "grad", None)
        if not getattr(p, "_acg_direct_grad", False) or g is None or not g.is_contiguous() or g.dtype != torch.float32:
            return None
        out.append(g)
    return out


def _grads_done(*params):
    for p in params:
        if p is not None:
            h = getattr(p, "_acg_grad_hook", None)
            if h is not None:
                h(p)


LAZY_DRES = True   # False: the unfused path (the tests' reference; SkipGrad)


class NormSums(object):
    """Slot shared by a (Cond)InstanceNorm and THE convolution that consumes its output (modules._run_stages / _run_block): the
    convolution's data gradient is the gradient w.r.t. the norm's output, and where its kernel supports it
    (acg_conv2d_bwd_data_s16_sums) the epilogue leaves the first pass of the norm's backward — per-tile sums of gy and
    gy * xhat — in `part`, so the norm's backward skips its own pass over dy and x.  The norm fills what the kernel needs at
    forward time; `dx` remembers the tensor the sums belong to: a gradient that reaches the norm as anything else (another
    consumer of the norm's output, a hook) makes the norm recompute them."""

    def __init__(self):
        self.clear()

    def clear(self):
        self.x = self.mean = self.rstd = self.gp = self.bp = self.mask = None
        self.gstride = self.act = 0
        self.part = self.dx = None

    def desc(self, part):
        d = _lib.NormSumsDesc()
        d.x, d.mean, d.rstd = _ptr(self.x), _ptr(self.mean), _ptr(self.rstd)
        d.gamma, d.beta, d.gstride = _ptr(self.gp), _ptr(self.bp), self.gstride
        d.sign_mask, d.act, d.part = _ptr(self.mask), self.act, _ptr(part)
        return d


NORM_SUMS = True   # False: the unfused path (the tests' reference)
NORM_SUMS_USED = 0   # norm backward passes that took their sums from a data-gradient epilogue (tests read it)
# Which fused paths the step actually took (bench.py prints them per step as `fused_paths`, so a fusion that a torch-side
# change — a hook, a clone, a shape — silently turned off shows in the bench line): launches per key since the last clear()
FUSED = {}


def _fused(key, n=1):
    FUSED[key] = FUSED.get(key, 0) + n


class ReluLink(object):
    """Hand-off between the two convolutions of a pad-conv-ReLU-pad-conv chain (ResnetBlock, modules.py:211-227): the
    SECOND convolution's data-gradient epilogue can mask its result with the sign of its own input (= the first one's ReLU
    output), which makes it the gradient w.r.t. the first convolution's pre-activation; it then sets `done`, and the first
    convolution's backward skips its activation-backward pass (3 tensor streams).  Valid only where the ReLU output has no
    other consumer."""

    def __init__(self):
        self.done = False
        self.mask = None   # sign bitmask of the ReLU output where the producing convolution stored one (pre-split trunk)


RELU_LINK = True   # False: the unfused path (the tests' reference)
RELU_MASK = True   # False: the unfused path (the tests' reference); True: the link carries a sign bitmask instead of the activation


# Pre-split ("S16") activation storage of the residual trunk (include/acgan_hip.h, acg_s16_encode): an S16 tensor is carried
# as an fp32-typed torch tensor of the same shape whose BYTES are (bf16 hi, bf16 lo) groups, tagged `_acg_s16`; only the
# Functions below read or write it, and every one of them knows from its forward-time plan which of its tensors are S16
# (autograd only ever hands such a gradient from the one Function that wrote it to the one that reads it).
S16_ENABLED = True   # False: the unfused path (the tests' reference)


def is_s16(t):
    return getattr(t, "_acg_s16", False)


def tag_s16(t):
    t._acg_s16 = True
    return t


class S16Plan(object):
    """which tensors of one convolution are pre-split: x (input), y (output; then dy arrives pre-split and already masked
    by the consumer's data gradient), gy (dy arrives pre-split from the norm behind the convolution), dx (what the data
    gradient writes: pre-split with the ReLU mask of x, or fp32)"""

    def __init__(self, x=False, y=False, gy=False, dx=False):
        self.x, self.y, self.gy, self.dx = x, y, gy, dx


def conv_s16_supported(N, Hi, Wi, C, K, pad, pad_mode):
    """can the stride-1 C -> C convolution take pre-split operands in forward, data gradient and weight gradient?"""
    if not S16_ENABLED or _PRECISION != "bf16x3" or not (LAZY_DRES and RELU_LINK and NORM_SIGN_MASK and CONV_STATS_ENABLED):
        return False
    d = conv_desc(N, Hi, Wi, C, C, K, 1, pad, pad_mode, C, C)
    return bool(_lib.query("acg_conv2d_s16_supported", ctypes.byref(d)))


class S16Decode(torch.autograd.Function):
    """pre-split -> fp32 where the residual trunk hands over to a layer that reads fp32 (its gradient is fp32 already)"""

    @staticmethod
    def forward(ctx, x):
        y = torch.empty_like(x)
        _lib.call("acg_s16_decode", _ptr(x), _ptr(y), x.numel(), _stream())
        return y

    @staticmethod
    def backward(ctx, g):
        return g


class S16Encode(torch.autograd.Function):
    """fp32 -> pre-split (a trunk entered from a tensor that was not written pre-split)"""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        y = torch.empty_like(x)
        _lib.call("acg_s16_encode", _ptr(x), _ptr(y), x.numel(), _stream())
        return y

    @staticmethod
    def backward(ctx, g):
        return g


# What a Conv2d shares with its neighbours (None in place of the record = a plain convolution): the slots documented at
# ConvStats (want_stats), SkipGrad, ReluLink (link_out / link_in), S16Plan (s16) and NormSums; no_grad: the grad mode was off
# at the call (Conv2d.forward_nhwc fills it in: inside Function.forward it is always off).  want_identity: also return x
# itself as a second output; a ResnetBlock feeds that alias to its skip connection, so the skip gradient arrives at the
# convolution and is added inside the data-gradient epilogue (acg_conv2d_bwd_data_add) instead of by an autograd accumulation.
ConvFusion = collections.namedtuple("ConvFusion", "want_stats want_identity link_out link_in skip_grad s16 norm_sums no_grad",
                                    defaults=(None, False, None, None, None, None, None, False))


def _weight_grad(ctx, entry, x, g, nbias, st, timed=True):
    """the weight (and bias, `nbias` long) gradient of a convolution Function through library entry point `entry`: added
    straight into .grad where the parameters take that (-> None, None), else returned as fresh tensors"""
    d, pk = ctx.d, ctx.packed
    direct = _direct_grad(ctx.wparam, ctx.bparam)
    if direct is not None:
        dw, db = direct
    else:
        dw = torch.empty((pk.Or, pk.Ir, pk.K, pk.K), device=x.device, dtype=torch.float32)
        db = torch.empty(nbias, device=x.device, dtype=torch.float32) if ctx.has_bias else None
    nb = _lib.query("acg_conv2d_bwd_weight_workspace_bytes", ctypes.byref(d))
    ws = workspace(nb)
    span = ConvTimer.span("wgrad", d) if timed else None
    _lib.call(entry, ctypes.byref(d), _ptr(x), _ptr(g), _ptr(dw), _ptr(db), pk.Or, pk.Ir, _ptr(ws), nb,
              1 if direct is not None else 0, st)
    if timed:
        span.done()
    if direct is None:
        return dw, db
    _grads_done(ctx.wparam, ctx.bparam)
    return None, None


def _call_with_norm_sums(ns, d, dx, st, entry, *args):
    """a data-gradient entry point whose epilogue leaves the backward sums of the norm in front (NormSums `ns`; dx: the
    tensor they belong to): entry(*args, &acg_norm_sums, st)"""
    part = torch.empty((d.N, (d.Hi * d.Wi) // STATS_ROWS, 2, d.Ci), device=dx.device, dtype=torch.float32)
    _lib.call(entry, *args, ctypes.byref(ns.desc(part)), st)
    ns.part, ns.dx = part, dx


class Conv2dFn(torch.autograd.Function):
    """nn.Conv2d (+ preceding ReflectionPad2d) + bias + fused activation; `fusion`: a ConvFusion or None."""

    @staticmethod
    def forward(ctx, x, weight, bias, packed, stride, pad, pad_mode, act, fusion=None):
        want_stats, want_identity, link_out, link_in, skip_grad, s16, norm_sums, no_grad = fusion or ConvFusion()
        x = x.contiguous()
        _check(x)
        N, Hi, Wi, Ci = x.shape
        if Ci != packed.Cis:
            raise _lib.AcgError("conv: input has %d stored channels, the layer takes %d" % (Ci, packed.Cis))
        d = conv_desc(N, Hi, Wi, Ci, packed.Cos, packed.K, stride, pad, pad_mode, packed.Ir, packed.Or)
        if d.Ho <= 0 or d.Wo <= 0:
            raise _lib.AcgError("conv: input %dx%d too small for kernel %d" % (Hi, Wi, packed.K))
        y = torch.empty((N, d.Ho, d.Wo, packed.Cos), device=x.device, dtype=torch.float32)
        pbias = _ptr(packed.bias if bias is not None else None)
        span = ConvTimer.span("fwd", d)
        if s16 is not None and s16.x:   # pre-split input (and, for a conv + ReLU inside the trunk, output)
            part = None
            if want_stats is not None and act == ACT_NONE and not s16.y:
                part = torch.empty((N, (d.Ho * d.Wo) // STATS_ROWS, 2, packed.Co), device=x.device, dtype=torch.float32)
                want_stats.part = part
            if s16.y and act == ACT_RELU and link_out is not None and RELU_MASK and packed.Co % 32 == 0 and \
                    _lib.query("acg_conv2d_bwd_data_s16_sums_supported", ctypes.byref(d)):
                # conv + ReLU feeding the next trunk convolution: its data gradient needs only the SIGN of y (same shape: d fits both)
                link_out.mask = torch.empty((y.numel() + 31) // 32, device=x.device, dtype=torch.int32)
                _fused("conv_fwd_s16_relu_bitmask")
                _lib.call("acg_conv2d_fwd_s16_mask", ctypes.byref(d), _ptr(x), _ptr(packed.wf), pbias, _ptr(y), _ptr(link_out.mask),
                          _stream())
            else:
                _fused("conv_fwd_s16")
                _lib.call("acg_conv2d_fwd_s16", ctypes.byref(d), _ptr(x), _ptr(packed.wf), pbias, _ptr(y), act, _ptr(part),
                          1 if s16.y else 0, _stream())
        elif want_stats is not None and CONV_STATS_ENABLED and act == ACT_NONE and \
                _lib.query("acg_conv2d_fwd_stats_supported", ctypes.byref(d)) and \
                (not no_grad or _lib.query("acg_conv2d_fwd_stats_per_tile", ctypes.byref(d))):
            # (no_grad: the caller ran under torch.no_grad() - the evaluator's ensemble groups - and such a forward must not
            # depend on how many images share the launch: where the epilogue's entries are joint statistics whose grouping
            # follows the batch, the norm's own pass takes them instead.  A training step keeps the fused statistics.)
            part = torch.empty((N, (d.Ho * d.Wo) // STATS_ROWS, 2, packed.Co), device=x.device, dtype=torch.float32)
            _fused("conv_fwd_tile_stats")
            _lib.call("acg_conv2d_fwd_stats", ctypes.byref(d), _ptr(x), _ptr(packed.wf), pbias, _ptr(y), _ptr(part), _stream())
            want_stats.part = part
        else:
            _lib.call("acg_conv2d_fwd", ctypes.byref(d), _ptr(x), _ptr(packed.wf), pbias, _ptr(y), act, _stream())
        span.done()
        ctx.d, ctx.packed, ctx.act, ctx.has_bias = d, packed, act, bias is not None
        ctx.wparam, ctx.bparam = weight, bias
        ctx.link_out, ctx.link_in = (link_out if act == ACT_RELU else None), link_in
        ctx.skip_grad = skip_grad
        ctx.s16 = s16 if (s16 is not None and s16.x) else None
        ctx.norm_sums = norm_sums if NORM_SUMS else None
        ctx.save_for_backward(x, y if (act != ACT_NONE and ctx.s16 is None) else None)
        if want_identity:
            return y, x.view_as(x)
        return y

    @staticmethod
    def backward(ctx, dy, dskip=None):
        x, y = ctx.saved_tensors
        dy = dy.contiguous()
        st = _stream()
        s16 = ctx.s16 is not None
        g = dy   # the gradient w.r.t. the pre-activation
        if s16:
            # x and dy are pre-split: dy comes from the norm behind this convolution, or (a conv + ReLU: s16.y) from the next
            # convolution's data gradient, which already applied the ReLU mask
            if ctx.s16.y:
                if ctx.link_out is None or not ctx.link_out.done:
                    raise _lib.AcgError("pre-split trunk: the gradient of a conv + ReLU output must come from the next convolution's "
                                        "fused data gradient")
                ctx.link_out.done = False
        elif ctx.link_out is not None and ctx.link_out.done:
            ctx.link_out.done = False   # the consumer's data-gradient epilogue already applied this ReLU's mask
        elif ctx.act != ACT_NONE:
            g = torch.empty_like(dy)
            _lib.call("acg_act_bwd", _ptr(dy), _ptr(y), _ptr(g), dy.numel(), ctx.act, st)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = Conv2dFn._data_grad(ctx, x, g, dskip, st)
        if ctx.needs_input_grad[1]:
            if s16:
                _fused("wgrad_s16")
            dw, db = _weight_grad(ctx, "acg_conv2d_bwd_weight_s16" if s16 else "acg_conv2d_bwd_weight", x, g, ctx.packed.Or, st)
        return dx, dw, db, None, None, None, None, None, None

    @staticmethod
    def _data_grad(ctx, x, g, dskip, st):
        """-> dx from g, the gradient w.r.t. this convolution's pre-activation.  With ctx.s16, x and g are pre-split, and so is
        dx where the plan says so (masked by the ReLU in front for that convolution's own backward)."""
        d, pk, p, D = ctx.d, ctx.packed, ctx.s16, ctypes.byref(ctx.d)
        dx = torch.empty_like(x)
        nb = _lib.query("acg_conv2d_bwd_data_workspace_bytes", D)
        ws = workspace(nb) if nb else None
        # the norm in front whose backward sums this data gradient can leave: dx is the gradient w.r.t. its output
        ns = ctx.norm_sums
        if ns is not None and (ns.x is None or tuple(ns.x.shape) != tuple(dx.shape) or (
                p is not None and (p.dx or not _lib.query("acg_conv2d_bwd_data_s16_sums_supported", D)))):
            ns = None
        span = ConvTimer.span("dgrad_sums" if (p is not None and ns is not None) else "dgrad", d)
        if p is not None and p.dx and (dskip is not None or ctx.link_in is None):
            raise _lib.AcgError("pre-split trunk: unexpected skip gradient / missing ReLU link")
        smask = None
        if dskip is not None:
            dskip = dskip.contiguous()
            if ctx.skip_grad is not None:   # the skip gradient is dskip * sign-bitmask (NormAct lazy_dres)
                dskip, smask = ctx.skip_grad.take(dskip)
        head, tail = (D, _ptr(g), _ptr(pk.wb)), (_ptr(dx), _ptr(ws), nb)
        if p is not None and p.dx:   # the gradient w.r.t. the pre-activation of the conv + ReLU in front, pre-split
            if ctx.link_in.mask is not None and ctx.link_in.mask.numel() == (x.numel() + 31) // 32 and \
                    _lib.query("acg_conv2d_bwd_data_s16_sums_supported", D):
                _fused("dgrad_s16_relu_bitmask")
                _lib.call("acg_conv2d_bwd_data_s16_mask", *head, *tail, _ptr(ctx.link_in.mask), st)
            else:
                _fused("dgrad_s16_relu_src")
                _lib.call("acg_conv2d_bwd_data_s16", *head, *tail, None, None, _ptr(x), 1, st)
            ctx.link_in.done = True
        elif p is not None:
            _fused("dgrad_s16_norm_sums" if ns is not None else "dgrad_s16_plain")
            if smask is not None:
                _fused("dgrad_s16_lazy_skip")
            if ns is not None:
                _call_with_norm_sums(ns, d, dx, st, "acg_conv2d_bwd_data_s16_sums", *head, *tail, _ptr(dskip), _ptr(smask))
            else:
                _lib.call("acg_conv2d_bwd_data_s16", *head, *tail, _ptr(dskip), _ptr(smask), None, 0, st)
        elif dskip is not None and _lib.query("acg_conv2d_bwd_data_add_supported", D) and \
                (smask is None or (d.Hi * d.Wi * (d.Ci // 4)) % 8 == 0):
            _fused("dgrad_skip_addend")
            _lib.call("acg_conv2d_bwd_data_add", *head, _ptr(dskip), _ptr(smask), *tail, st)
        elif dskip is None and ctx.link_in is not None and RELU_LINK and _lib.query("acg_conv2d_bwd_data_add_supported", D):
            _fused("dgrad_relu_link")
            _lib.call("acg_conv2d_bwd_data_relu", *head, _ptr(x), *tail, st)
            ctx.link_in.done = True
        elif dskip is None and ns is not None and ns.mask is None and _lib.query("acg_conv2d_bwd_data_sums_supported", D):
            # the row pipeline, the four-phase stride-2 tile, the generic tile or the thin-row kernel of the head
            _fused("dgrad_f32_norm_sums")
            _call_with_norm_sums(ns, d, dx, st, "acg_conv2d_bwd_data_sums", *head, *tail)
        else:
            _lib.call("acg_conv2d_bwd_data", *head, *tail, st)
            if dskip is not None:
                if smask is not None:   # not fusable here: materialise the masked skip gradient
                    m = torch.empty_like(dskip)
                    _lib.call("acg_mask_apply", _ptr(dskip), _ptr(smask), _ptr(m), dskip.numel(), st)
                    dskip = m
                dx = dx + dskip
        span.done()
        return dx


class ConvTranspose2dFn(torch.autograd.Function):
    """nn.ConvTranspose2d(k3, s2, p1, op1) + bias + fused activation.  `packed` holds the weight
    (Cin_T, Cout_T, k, k) packed as the OIHW weight of the Conv2d it is the adjoint of."""

    @staticmethod
    def forward(ctx, x, weight, bias, packed, stride, pad, out_pad, act, want_stats=None):
        x = x.contiguous()
        _check(x)
        N, H, W, Cs = x.shape
        K = packed.K
        Hl = (H - 1) * stride - 2 * pad + K + out_pad
        Wl = (W - 1) * stride - 2 * pad + K + out_pad
        # underlying conv: large side (Hl, Wl, packed.Ci) -> small side (H, W, packed.Co)
        if Cs != packed.Co:
            raise _lib.AcgError("conv_transpose: input has %d stored channels, expected %d" % (Cs, packed.Co))
        d = conv_desc(N, Hl, Wl, packed.Ci, packed.Co, K, stride, pad, PAD_ZERO)
        if (d.Ho, d.Wo) != (H, W):
            raise _lib.AcgError("conv_transpose: inconsistent geometry")
        y = torch.empty((N, Hl, Wl, packed.Ci), device=x.device, dtype=torch.float32)
        pbias = _ptr(packed.bias if bias is not None else None)
        if want_stats is not None and CONV_STATS_ENABLED and act == ACT_NONE and \
                _lib.query("acg_conv_transpose2d_fwd_stats_supported", ctypes.byref(d)):
            part = torch.empty((N, (Hl * Wl) // STATS_ROWS, 2, packed.Ci), device=x.device, dtype=torch.float32)
            _lib.call("acg_conv_transpose2d_fwd_stats", ctypes.byref(d), _ptr(x), _ptr(packed.wb), pbias, _ptr(y), _ptr(part), _stream())
            want_stats.part = part
        else:
            _lib.call("acg_conv_transpose2d_fwd", ctypes.byref(d), _ptr(x), _ptr(packed.wb), pbias, _ptr(y), act, _stream())
        ctx.d, ctx.packed, ctx.act, ctx.has_bias = d, packed, act, bias is not None
        ctx.wparam, ctx.bparam = weight, bias
        ctx.save_for_backward(x, y if act != ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        d, pk = ctx.d, ctx.packed
        dy = dy.contiguous()
        st = _stream()
        if ctx.act != ACT_NONE:
            g = torch.empty_like(dy)
            _lib.call("acg_act_bwd", _ptr(dy), _ptr(y), _ptr(g), dy.numel(), ctx.act, st)
        else:
            g = dy
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _lib.call("acg_conv_transpose2d_bwd_data", ctypes.byref(d), _ptr(g), _ptr(pk.wf), _ptr(dx), st)
        if ctx.needs_input_grad[1]:
            dw, db = _weight_grad(ctx, "acg_conv_transpose2d_bwd_weight", x, g, pk.Ir, st, timed=False)
        return dx, dw, db, None, None, None, None, None, None


# ----------------------------------------------------------------------------------------------
# normalisation (+ fused activation / residual)
# ----------------------------------------------------------------------------------------------
NORM_SIGN_MASK = True   # False: the unfused path (the tests' reference)


class NormAct(torch.autograd.Function):
    """y = act(norm(x) * gamma + beta [+ res]).

    kind 'in'  : InstanceNorm      (modules.py:64-97)   gamma/beta (C,), biased variance
    kind 'cin' : CondInstanceNorm  (modules.py:104-132) gamma/beta (N, Cp), UNBIASED variance
    kind 'bn'  : BatchNorm2d/1d in train mode           gamma/beta (C,), biased; running stats updated
    x: (N,H,W,Cp) or (N,Cp).  gamma_p / beta_p are the C16-padded device copies for 'in'/'bn'.
    """

    @staticmethod
    def forward(ctx, x, gamma, beta, res, kind, act, eps, gamma_p, beta_p, run_mean, run_var, momentum, lazy_dres=None,
                stats=None, s16_out=False, s16_dx=False, s16_res=False, sums=None):
        """sums: a NormSums slot shared with the consumer of y, or None.  lazy_dres: a SkipGrad slot (the caller guarantees that the gradient w.r.t. `res` goes only to the Conv2dFn holding
        the same slot) or None.  stats: per-tile (mean, M2) partials a convolution epilogue produced (ConvStats.part)."""
        x = x.contiguous()
        _check(x)
        C = x.shape[-1]
        N = x.shape[0]
        rows = x.numel() // C
        if kind in ("bn", "bn_eval"):
            G, P = 1, rows
        else:
            G, P = N, rows // N
        unbiased = 1 if kind == "cin" else (2 if kind == "bn_eval" else 0)
        if kind == "cin":
            # (N, Cp) rows, possibly column blocks of a wider matrix (CondBankFn): the kernels take the row stride
            if gamma.shape != (N, C) or beta.shape != (N, C):
                raise _lib.AcgError("cin: scale/shift must be (N, Cp)")
            ok = gamma.stride(1) == 1 and beta.stride(1) == 1 and gamma.stride(0) == beta.stride(0) and gamma.stride(0) >= C \
                and gamma.stride(0) % 4 == 0 and gamma.data_ptr() % 16 == 0 and beta.data_ptr() % 16 == 0
            if ok:
                gp, bp, gstride = gamma, beta, gamma.stride(0)
            else:
                gp, bp, gstride = gamma.contiguous(), beta.contiguous(), C
        else:
            gp, bp, gstride = gamma_p, beta_p, 0
        _check(gp if gp.is_contiguous() else None, bp if bp.is_contiguous() else None)   # (strided scale / shift: checked above)
        st = _stream()
        mean = torch.empty(G * C, device=x.device, dtype=torch.float32)
        rstd = torch.empty(G * C, device=x.device, dtype=torch.float32)
        if kind == "bn_eval":  # running statistics (real length) -> padded mean / rstd
            _lib.call("acg_bn_eval_stats", _ptr(run_mean), _ptr(run_var), run_mean.numel(), C, eps, _ptr(mean), _ptr(rstd), st)
        else:
            part = stats if kind in ("in", "cin") else None
            if part is not None:  # the producing convolution already reduced 128-pixel tiles: merge only
                _fused("norm_stats_from_conv_epilogue")
                _lib.call("acg_norm_stats_from_partials", _ptr(part), G, P, C, STATS_ROWS, eps, unbiased, _ptr(mean),
                          _ptr(rstd), st)
            else:
                nb = _lib.query("acg_norm_workspace_bytes", G, P, C)
                ws = workspace(nb)
                _lib.call("acg_norm_stats", _ptr(x), G, P, C, eps, unbiased, _ptr(mean), _ptr(rstd), _ptr(run_mean),
                          _ptr(run_var), momentum, _ptr(ws), nb, st)
        y = torch.empty_like(x)
        if res is not None:
            res = res.contiguous()
        # without a residual the backward recomputes the activation mask from x (gamma/beta): y is neither saved nor read.
        # With one it needs sign(y): the apply pass stores it as one bit per element (1/32 of a tensor) where it can.
        need_y = act != ACT_NONE and res is not None
        mask = None
        if need_y and NORM_SIGN_MASK and act in (ACT_RELU, ACT_LRELU) and (P * (C // 4)) % 8 == 0 and any(ctx.needs_input_grad):
            mask = torch.empty((G * P * C + 31) // 32, device=x.device, dtype=torch.int32)
        # pre-split (S16) output for the convolution behind this norm; a residual that arrives tagged S16 is read that way
        fmt = (2 if s16_out else 0) | (1 if (res is not None and s16_res) else 0)
        _lib.call("acg_norm_apply", _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gp), _ptr(bp), gstride, _ptr(res), _ptr(y), _ptr(mask),
                  G, P, C, act, fmt, st)
        ctx.s16_dx = bool(s16_dx)
        ctx.sums = None
        if sums is not None and NORM_SUMS and kind in ("in", "cin") and x.dim() == 4 and act in (ACT_NONE, ACT_RELU) and \
                (act == ACT_NONE or mask is not None or not need_y) and any(ctx.needs_input_grad):
            sums.x, sums.mean, sums.rstd, sums.gp, sums.bp, sums.gstride, sums.mask, sums.act = x, mean, rstd, gp, bp, gstride, mask, act
            ctx.sums = sums
        ctx.cfg = (kind, act, G, P, C, unbiased, gstride, res is not None, gamma.shape)
        ctx.gparam, ctx.bparam = (gamma, beta) if kind != "cin" else (None, None)
        ctx.lazy_dres = lazy_dres if (lazy_dres is not None and LAZY_DRES and mask is not None) else None
        ctx.save_for_backward(x, y if (need_y and mask is None) else None, mean, rstd, gp, bp, mask)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, mean, rstd, gp, bp, mask = ctx.saved_tensors
        kind, act, G, P, C, unbiased, gstride, has_res, gshape = ctx.cfg
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if (has_res and ctx.lazy_dres is None) else None
        if ctx.s16_dx and dres is not None:
            raise _lib.AcgError("norm: a pre-split dx needs the un-materialised skip gradient")
        direct = _direct_grad(ctx.gparam, ctx.bparam) if (kind != "cin" and ctx.needs_input_grad[1] and ctx.needs_input_grad[2]) else None
        if direct is not None:      # shared affine parameters: add into their .grad (first gshape[0] = real channels)
            dgamma, dbeta = direct
        else:
            npar = G * C if gstride else gshape[0]
            dgamma = torch.empty(npar, device=x.device, dtype=torch.float32)
            dbeta = torch.empty(npar, device=x.device, dtype=torch.float32)
        nb = _lib.query("acg_norm_workspace_bytes", G, P, C)
        ws = workspace(nb)
        part = None
        if ctx.sums is not None:   # the consumer's data gradient already summed gy and gy * xhat per tile — of THIS dy?
            s = ctx.sums
            if s.part is not None and s.dx is not None and s.dx.data_ptr() == dy.data_ptr() and s.dx.shape == dy.shape:
                part = s.part
            s.clear()
        if part is not None:
            global NORM_SUMS_USED
            NORM_SUMS_USED += 1
            _fused("norm_bwd_sums_from_dgrad")
            _lib.call("acg_norm_bwd_partials", _ptr(dy), _ptr(y), _ptr(mask), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gp), _ptr(bp),
                      gstride, _ptr(dx), _ptr(dres), _ptr(dgamma), _ptr(dbeta), 0 if gstride else gshape[0],
                      1 if direct is not None else 0, G, P, C, act, unbiased, 1 if ctx.s16_dx else 0, _ptr(part), part.shape[1],
                      _ptr(ws), nb, _stream())
        else:
            _lib.call("acg_norm_bwd", _ptr(dy), _ptr(y), _ptr(mask), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gp), _ptr(bp), gstride, _ptr(dx),
                      _ptr(dres), _ptr(dgamma), _ptr(dbeta), 0 if gstride else gshape[0], 1 if direct is not None else 0, G, P, C,
                      act, unbiased, 1 if ctx.s16_dx else 0, _ptr(ws), nb, _stream())
        if mask is not None:
            _fused("norm_bwd_sign_bitmask")
        if kind == "cin":
            dg, db = dgamma.view(G, C), dbeta.view(G, C)
        elif direct is not None:
            dg = db = None
            _grads_done(ctx.gparam, ctx.bparam)
        else:
            dg, db = dgamma, dbeta
        if has_res and act == ACT_NONE:
            dres = dy
        elif ctx.lazy_dres is not None:
            ctx.lazy_dres.mask, ctx.lazy_dres.dy = mask, dy
            dres = dy
        return dx, dg, db, dres, None, None, None, None, None, None, None, None, None, None, None, None, None, None


# nn.Dropout inside the residual blocks (--use_dropout, options.py:65 -> modules.py:167-168, 214-215).  DROPOUT_SOURCE: None =
# draw the keep bits on the device (torch's Philox generator: 32 Bernoulli(1/2) bits per random word); a callable
# (nhwc_shape, real_channels, p) -> int32 bit words injects the draw (parity tests feed the fixture's masks to both sides)
DROPOUT_SOURCE = None


def dropout_keep_bits(shape, C, p):
    if DROPOUT_SOURCE is not None:
        return DROPOUT_SOURCE(tuple(shape), C, p)
    if p != 0.5:
        raise NotImplementedError("Dropout(p=%g): the device draw implements the reference's p = 0.5 (one random bit per element)" % p)
    n = 1
    for d in shape:
        n *= d
    dev = torch.device("cuda", torch.cuda.current_device())
    return torch.randint(-2 ** 31, 2 ** 31, ((n + 31) // 32,), device=dev, dtype=torch.int64).to(torch.int32)


def pack_keep_bits(keep_nchw, Cp, device):
    """a boolean NCHW keep mask (the reference's layout) -> bit words over the NHWC C16 tensor (pad channels: dropped)"""
    k = torch.as_tensor(keep_nchw, device=device).to(torch.bool)
    N, C, H, W = k.shape
    full = torch.zeros((N, H, W, Cp), device=device, dtype=torch.int64)
    full[..., :C] = k.permute(0, 2, 3, 1).to(torch.int64)
    words = (full.reshape(-1, 32) << torch.arange(32, device=device, dtype=torch.int64)).sum(1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


class DropoutFn(torch.autograd.Function):
    """y = keep ? x / (1 - p) : 0 on an NHWC C16 tensor (acg_dropout_apply); backward: the same map on dy"""

    @staticmethod
    def forward(ctx, x, C, p):
        x = x.contiguous()
        _check(x)
        if x.numel() % 32:
            raise _lib.AcgError("dropout: tensor size must be a multiple of 32 elements")
        bits = dropout_keep_bits(x.shape, C, p)
        if bits.numel() * 32 != x.numel() or bits.dtype != torch.int32 or not bits.is_cuda:
            raise _lib.AcgError("dropout: keep bits must be %d int32 words on the device" % (x.numel() // 32))
        y = torch.empty_like(x)
        ctx.scale = 1.0 / (1.0 - p)
        _lib.call("acg_dropout_apply", _ptr(x), _ptr(bits), ctx.scale, _ptr(y), x.numel(), _stream())
        ctx.save_for_backward(bits)
        return y

    @staticmethod
    def backward(ctx, dy):
        (bits,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        _lib.call("acg_dropout_apply", _ptr(dy), _ptr(bits), ctx.scale, _ptr(dx), dy.numel(), _stream())
        return dx, None, None


class SyncBatchNormAct(torch.autograd.Function):
    """BatchNorm (train mode) with statistics over ALL ranks' batches: per-rank (count, mean, M2) from the stats
    kernel, one all-reduce of [C x 3] floats, Chan-style combination; backward all-reduces the two per-channel sums
    before the apply pass.  With equal shards this makes N ranks == 1 rank on the concatenated batch."""

    @staticmethod
    def forward(ctx, x, gamma, beta, act, eps, gamma_p, beta_p, run_mean, run_var, momentum):
        import torch.distributed as td
        x = x.contiguous()
        _check(x, gamma_p, beta_p)
        C = x.shape[-1]
        P = x.numel() // C
        st = _stream()
        mean = torch.empty(C, device=x.device, dtype=torch.float32)
        rstd = torch.empty(C, device=x.device, dtype=torch.float32)
        nb = _lib.query("acg_norm_workspace_bytes", 1, P, C)
        ws = workspace(nb)
        _lib.call("acg_norm_stats", _ptr(x), 1, P, C, eps, 0, _ptr(mean), _ptr(rstd), None, None, 0.0, _ptr(ws), nb, st)
        # local biased variance back from rstd, then combine across ranks: E[x], E[x^2] weighted by the pixel counts
        var = rstd.pow(-2) - eps
        pack = torch.cat([mean * P, (var + mean * mean) * P, mean.new_full((1,), float(P))])
        if td.get_backend() == "gloo" and pack.is_cuda:
            h = pack.cpu(); td.all_reduce(h); pack = h.to(x.device)
        else:
            td.all_reduce(pack)
        # the global pixel count rides in the same all-reduce and stays on the device (no host sync): the statistics are
        # exact for unequal shards too.  The backward's 1/Ptot is a launch argument and uses the equal-shard contract of
        # the data-parallel step (only then is the mean of the rank gradients the global-batch gradient, dist.py).
        cnt = pack[2 * C:]
        Ptot = float(P) * td.get_world_size()
        gmean = pack[:C] / cnt
        gvar = (pack[C:2 * C] / cnt - gmean * gmean).clamp_(min=0.0)
        grstd = (gvar + eps).rsqrt()
        if run_mean is not None:
            nreal = run_mean.numel()
            with torch.no_grad():
                run_mean.mul_(1 - momentum).add_(gmean[:nreal], alpha=momentum)
                run_var.mul_(1 - momentum).add_(gvar[:nreal] * (cnt / (cnt - 1).clamp(min=1.0)) * momentum)
        gmean, grstd = gmean.contiguous(), grstd.contiguous()
        y = torch.empty_like(x)
        _lib.call("acg_norm_apply", _ptr(x), _ptr(gmean), _ptr(grstd), _ptr(gamma_p), _ptr(beta_p), 0, None, _ptr(y), None, 1, P, C,
                  act, 0, st)
        ctx.cfg = (act, P, int(Ptot), C, gamma.shape)
        ctx.save_for_backward(x, y if act != ACT_NONE else None, gmean, grstd, gamma_p)
        return y

    @staticmethod
    def backward(ctx, dy):
        import torch.distributed as td
        x, y, mean, rstd, gp = ctx.saved_tensors
        act, P, Ptot, C, gshape = ctx.cfg
        dy = dy.contiguous()
        st = _stream()
        sums = torch.empty(2 * C, device=x.device, dtype=torch.float32)
        nb = _lib.query("acg_norm_workspace_bytes", 1, P, C)
        ws = workspace(nb)
        _lib.call("acg_norm_bwd_sums", _ptr(dy), _ptr(y), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(sums), 1, P, C, act, _ptr(ws),
                  nb, st)
        local = sums.clone()  # parameter gradients stay per-rank (the gradient all-reduce averages them later)
        if td.get_backend() == "gloo" and sums.is_cuda:
            h = sums.cpu(); td.all_reduce(h); sums = h.to(x.device)
        else:
            td.all_reduce(sums)
        dx = torch.empty_like(x)
        _lib.call("acg_norm_bwd_apply", _ptr(dy), _ptr(y), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gp), 0, _ptr(sums), _ptr(dx),
                  None, 1, P, Ptot, C, act, 0, st)
        # the later gradient all-reduce takes the MEAN over ranks while the single-process gradient is the SUM over all
        # samples of the global-batch-mean loss; losses here are per-rank means, so local sums are already right.
        return dx, local[C:][:gshape[0]], local[:C][:gshape[0]], None, None, None, None, None, None, None


# ----------------------------------------------------------------------------------------------
# small dense layers
# ----------------------------------------------------------------------------------------------
class LinearFn(torch.autograd.Function):
    """y[N, Op] = act(x[:, :I] @ w.T + b), zero in columns >= O."""

    @staticmethod
    def forward(ctx, x, w, b, act, Op):
        x = x.contiguous()
        w = w.contiguous()
        _check(x, w, b)
        N, ldx = x.shape
        O, I = w.shape[0], w.numel() // w.shape[0]
        if I > ldx:
            raise _lib.AcgError("linear: input has %d columns, weight expects %d" % (ldx, I))
        y = torch.empty((N, Op), device=x.device, dtype=torch.float32)
        _lib.call("acg_linear_fwd", _ptr(x), _ptr(w), _ptr(b), _ptr(y), N, I, ldx, O, Op, act, _stream())
        ctx.cfg = (N, I, ldx, O, Op, act, w.shape)
        ctx.save_for_backward(x, w, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        N, I, ldx, O, Op, act, wshape = ctx.cfg
        dy = dy.contiguous()
        dx = torch.zeros_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty(wshape, device=x.device, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        db = torch.empty(O, device=x.device, dtype=torch.float32) if ctx.needs_input_grad[2] else None
        _lib.call("acg_linear_bwd", _ptr(dy), _ptr(y), _ptr(x), _ptr(w), _ptr(dx), _ptr(dw), _ptr(db), N, I, ldx, O, Op, act,
                  _stream())
        return dx, dw, db, None, None


COND_BANK = True   # False: the unfused path (the tests' reference)


class CondBankFn(torch.autograd.Function):
    """The scale / shift layers of ALL CondInstanceNorms of a generator (modules.py:104-132: two ReLU(1x1 conv(z)) per norm,
    19 norms in the 9-block generator) as ONE dense layer: y = ReLU(z @ Wcat.T + bcat), Wcat = the 2L weights stacked;
    output k of the tuple is the (N, C) column block k of y (row stride 2L*C — NormAct reads scale / shift through that
    stride).  38 forward and 76 backward launches plus the ~80 small additions with which autograd sums the 38 gradients
    w.r.t. z and accumulates the second pass into .grad become 3 + 4.  params = w0, b0, w1, b1, ... (w_k: (C, I, 1, 1))."""

    @staticmethod
    def forward(ctx, z, C, *params):
        z = z.contiguous()
        ws, bs = params[0::2], params[1::2]
        I = ws[0].numel() // C
        O = C * len(ws)
        N, ldx = z.shape
        if any(w.numel() != C * I or b.numel() != C for w, b in zip(ws, bs)) or I > ldx or len(ws) > _lib.MAX_SEGMENTS // 2:
            raise _lib.AcgError("cond bank: layers of different widths")
        wcat = torch.cat([w.detach().reshape(C, I) for w in ws], 0)
        bcat = torch.cat([b.detach() for b in bs], 0)
        y = torch.empty((N, O), device=z.device, dtype=torch.float32)
        _lib.call("acg_linear_fwd", _ptr(z), _ptr(wcat), _ptr(bcat), _ptr(y), N, I, ldx, O, O, ACT_RELU, _stream())
        ctx.cfg = (N, I, ldx, O, C)
        ctx.params = params
        ctx.save_for_backward(z, wcat, y)
        outs = tuple(y[:, k * C:(k + 1) * C] for k in range(len(ws)))
        return outs

    @staticmethod
    def backward(ctx, *grads):
        z, wcat, y = ctx.saved_tensors
        N, I, ldx, O, C = ctx.cfg
        params = ctx.params
        zero = None
        cols = []
        for g in grads:
            if g is None:
                if zero is None:
                    zero = torch.zeros((N, C), device=z.device, dtype=torch.float32)
                g = zero
            cols.append(g)
        dy = torch.cat(cols, 1)
        dz = torch.empty_like(z) if ctx.needs_input_grad[0] else None
        if dz is not None and ldx > I:
            dz.zero_()
        need_p = any(ctx.needs_input_grad[2:])
        dw = torch.empty((O, I), device=z.device, dtype=torch.float32) if need_p else None
        db = torch.empty(O, device=z.device, dtype=torch.float32) if need_p else None
        _lib.call("acg_linear_bwd", _ptr(dy), _ptr(y), _ptr(z), _ptr(wcat), _ptr(dz), _ptr(dw), _ptr(db), N, I, ldx, O, O, ACT_RELU,
                  _stream())
        pg = [None] * len(params)
        if need_p:
            direct = _direct_grad(*params)
            if direct is not None:   # add the slices into the parameters' .grad, all in one launch per source buffer
                for src, tens, width in ((dw, direct[0::2], C * I), (db, direct[1::2], C)):
                    sg = _lib.Segments()
                    for k, t in enumerate(tens):
                        sg.dst[k], sg.off[k], sg.len[k] = t.data_ptr(), k * width, width
                    sg.n = len(tens)
                    _lib.call("acg_segments_accumulate", _ptr(src), ctypes.byref(sg), 1, _stream())
                _grads_done(*params)
            else:
                for k in range(len(params) // 2):
                    pg[2 * k] = dw[k * C:(k + 1) * C].view_as(params[2 * k])
                    pg[2 * k + 1] = db[k * C:(k + 1) * C]
        return (dz, None) + tuple(pg)


LATENT_MLP = True   # False: the unfused path (the tests' reference)


def latent_mlp_supported(N, I, H):
    return LATENT_MLP and bool(_lib.query("acg_latent_mlp_supported", N, I, H))


class LatentMLPFn(torch.autograd.Function):
    """DiscriminatorLatent's whole dense chain (networks.py:396-433) as one launch per direction: three Linear /
    BatchNorm1d(train) / LeakyReLU(0.2) stages and the Linear head, followed by a sigmoid when head_act is ACT_SIGMOID
    (use_sigmoid, networks.py:420-421).  `params` = 4 weights, 4 biases, 3 BN weights, 3 BN biases (autograd inputs);
    `buffers` = 3 running means + 3 running variances, updated in place.  -> (N, 4), column 0 valid (the layout LinearFn
    gives the head), columns 1..3 zero."""

    NPARAM = 14

    @staticmethod
    def forward(ctx, z, eps, momentum, head_act, buffers, *params):
        z = z.contiguous()
        _check(z, *params)
        _check(*buffers)
        N, ldz = z.shape
        H, I = params[0].shape
        for l in range(4):
            want = ((H if l < 3 else 1), (I if l == 0 else H))
            if tuple(params[l].shape) != want or params[4 + l].numel() != want[0] or not params[l].is_contiguous():
                raise _lib.AcgError("latent mlp: layer %d has shape %s, expected %s" % (l, tuple(params[l].shape), want))
        if I > ldz:
            raise _lib.AcgError("latent mlp: input has %d columns, the first layer expects %d" % (ldz, I))
        pp = _lib.LatentMlpParams()
        for l in range(4):
            pp.w[l], pp.b[l] = params[l].data_ptr(), params[4 + l].data_ptr()
        for l in range(3):
            pp.gamma[l], pp.beta[l] = params[8 + l].data_ptr(), params[11 + l].data_ptr()
            pp.run_mean[l], pp.run_var[l] = buffers[l].data_ptr(), buffers[3 + l].data_ptr()
        pp.head_act = head_act
        a_save = torch.empty((3, N, H), device=z.device, dtype=torch.float32)
        stats = torch.empty((3, 2, H), device=z.device, dtype=torch.float32)
        out = torch.empty((N, 4), device=z.device, dtype=torch.float32)
        _lib.call("acg_latent_mlp_fwd", ctypes.byref(pp), _ptr(z), ldz, N, I, H, float(eps), float(momentum), _ptr(a_save),
                  _ptr(stats), _ptr(out), _stream())
        ctx.cfg = (N, ldz, I, H)
        ctx.params = params
        ctx.head_act = head_act
        ctx.save_for_backward(z, a_save, stats, out if head_act == ACT_SIGMOID else None, *[p.detach() for p in params])
        return out

    @staticmethod
    def backward(ctx, dout):
        z, a_save, stats, out = ctx.saved_tensors[:4]
        ws = ctx.saved_tensors[4:]
        N, ldz, I, H = ctx.cfg
        dout = dout.contiguous()
        pp, gg = _lib.LatentMlpParams(), _lib.LatentMlpGrads()
        for l in range(4):
            pp.w[l], pp.b[l] = ws[l].data_ptr(), ws[4 + l].data_ptr()
        for l in range(3):
            pp.gamma[l], pp.beta[l] = ws[8 + l].data_ptr(), ws[11 + l].data_ptr()
        pp.head_act = ctx.head_act
        want = [ctx.needs_input_grad[5 + i] for i in range(LatentMLPFn.NPARAM)]
        direct = _direct_grad(*ctx.params) if all(want) else None
        if direct is not None:
            grads = direct
        else:
            grads = [torch.empty_like(ws[i]) if want[i] else None for i in range(LatentMLPFn.NPARAM)]
        for l in range(4):
            gg.dw[l] = grads[l].data_ptr() if grads[l] is not None else None
            gg.db[l] = grads[4 + l].data_ptr() if grads[4 + l] is not None else None
        for l in range(3):
            gg.dgamma[l] = grads[8 + l].data_ptr() if grads[8 + l] is not None else None
            gg.dbeta[l] = grads[11 + l].data_ptr() if grads[11 + l] is not None else None
        dz = torch.zeros_like(z) if ctx.needs_input_grad[0] else None
        _lib.call("acg_latent_mlp_bwd", ctypes.byref(pp), ctypes.byref(gg), _ptr(z), ldz, N, I, H, _ptr(a_save), _ptr(stats),
                  _ptr(out), _ptr(dout), _ptr(dz), 1 if direct is not None else 0, _stream())
        if direct is not None:
            _grads_done(*ctx.params)
            grads = [None] * LatentMLPFn.NPARAM
        return (dz, None, None, None, None) + tuple(grads)


class SpatialMean(torch.autograd.Function):
    """(N,H,W,Cp) -> (N,Cp): mean over H*W (identity at 1x1; LatentEncoder extension)."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        _check(x)
        N, H, W, Cp = x.shape
        ctx.shape = x.shape
        y = torch.empty((N, Cp), device=x.device, dtype=torch.float32)
        _lib.call("acg_spatial_mean_fwd", _ptr(x), _ptr(y), N, H * W, Cp, _stream())
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        N, H, W, Cp = ctx.shape
        dx = torch.empty(ctx.shape, device=g.device, dtype=torch.float32)
        _lib.call("acg_spatial_mean_bwd", _ptr(g), _ptr(dx), N, H * W, Cp, _stream())
        return dx


# ----------------------------------------------------------------------------------------------
# losses (device scalars; no host sync)
# ----------------------------------------------------------------------------------------------
def _red_ws():
    nb = _lib.query("acg_reduce_workspace_bytes", 0)
    return workspace(nb, slot=1), nb


class MseConst(torch.autograd.Function):
    """F.mse_loss(pred, full_like(pred, target)) over the C valid channels (model.py:65-70)."""

    @staticmethod
    def forward(ctx, p, C, target):
        p = p.contiguous()
        _check(p)
        Cp = p.shape[-1]
        npix = p.numel() // Cp
        out = torch.empty((), device=p.device, dtype=torch.float32)
        ws, nb = _red_ws()
        _lib.call("acg_mse_const_fwd", _ptr(p), npix, C, Cp, float(target), _ptr(out), _ptr(ws), nb, _stream())
        ctx.cfg = (npix, C, Cp, float(target))
        ctx.save_for_backward(p)
        return out

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        npix, C, Cp, target = ctx.cfg
        g = g.contiguous()
        dp = torch.empty_like(p)
        _lib.call("acg_mse_const_bwd", _ptr(p), npix, C, Cp, target, _ptr(g), _ptr(dp), _stream())
        return dp, None, None


class BceConst(torch.autograd.Function):
    """F.binary_cross_entropy(p, full_like(p, target)) over the C valid channels, p a probability (a sigmoid head): the
    reference's use_sigmoid branch (model.py:56-63) with a float target in place of its Long one.  Same shape contract as
    MseConst."""

    @staticmethod
    def forward(ctx, p, C, target):
        p = p.contiguous()
        _check(p)
        Cp = p.shape[-1]
        npix = p.numel() // Cp
        out = torch.empty((), device=p.device, dtype=torch.float32)
        ws, nb = _red_ws()
        _lib.call("acg_bce_const_fwd", _ptr(p), npix, C, Cp, float(target), _ptr(out), _ptr(ws), nb, _stream())
        ctx.cfg = (npix, C, Cp, float(target))
        ctx.save_for_backward(p)
        return out

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        npix, C, Cp, target = ctx.cfg
        g = g.contiguous()
        dp = torch.empty_like(p)
        _lib.call("acg_bce_const_bwd", _ptr(p), npix, C, Cp, target, _ptr(g), _ptr(dp), _stream())
        return dp, None, None


class L1(torch.autograd.Function):
    """F.l1_loss(a, b) (mean) over the C valid channels (model.py:391, 468, 486, 494)."""

    @staticmethod
    def forward(ctx, a, b, C):
        a, b = a.contiguous(), b.contiguous()
        _check(a, b)
        Cp = a.shape[-1]
        npix = a.numel() // Cp
        out = torch.empty((), device=a.device, dtype=torch.float32)
        ws, nb = _red_ws()
        _lib.call("acg_l1_fwd", _ptr(a), _ptr(b), npix, C, Cp, _ptr(out), _ptr(ws), nb, _stream())
        ctx.cfg = (npix, C, Cp)
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        npix, C, Cp = ctx.cfg
        g = g.contiguous()
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        if da is not None or db is not None:
            _lib.call("acg_l1_bwd", _ptr(a), _ptr(b), npix, C, Cp, _ptr(g), _ptr(da), _ptr(db), _stream())
        return da, db, None


def l1_into(a, b, C, out):
    """out[()] = F.l1_loss(a, b) over the C valid channels, written into a given device scalar (no grad)."""
    a, b = a.detach().contiguous(), b.detach().contiguous()
    _check(a, b, out)
    Cp = a.shape[-1]
    ws, nb = _red_ws()
    _lib.call("acg_l1_fwd", _ptr(a), _ptr(b), a.numel() // Cp, C, Cp, _ptr(out), _ptr(ws), nb, _stream())
    return out


# ----------------------------------------------------------------------------------------------
# the variational bound of the evaluator (evaluate.py, test.py)
# ----------------------------------------------------------------------------------------------
NLL_KINDS = {"laplace": _lib.NLL_LAPLACE, "gaussian": _lib.NLL_GAUSSIAN}


class PixelNLL(torch.autograd.Function):
    """-sum over pixels and the C valid channels of log_prob_laplace / log_prob_gaussian(x, mu, logvar) per sample
    (model.py:24-34, summed as evaluate.py:94-95 does): x, mu (N, H, W, Cp) image tensors, logvar ONE (1, H, W, Cp) plane
    broadcast over the batch -> (N,).  Gradients reach mu and logvar; x is data."""

    @staticmethod
    def forward(ctx, x, mu, logvar, C, kind="laplace"):
        x, mu, logvar = x.contiguous(), mu.contiguous(), logvar.contiguous()
        _check(x, mu, logvar)
        N, Cp = mu.shape[0], mu.shape[-1]
        npix = mu.numel() // (N * Cp)
        if x.shape != mu.shape or logvar.numel() != npix * Cp or logvar.shape[-1] != Cp:
            raise _lib.AcgError("PixelNLL: x %s, mu %s and the logvar plane %s disagree" % (tuple(x.shape), tuple(mu.shape),
                                                                                       tuple(logvar.shape)))
        out = torch.empty((N,), device=mu.device, dtype=torch.float32)
        nb = _lib.query("acg_pixel_nll_workspace_bytes", N, npix)
        ws = workspace(nb, slot=1)
        _lib.call("acg_pixel_nll_fwd", NLL_KINDS[kind], _ptr(x), _ptr(mu), _ptr(logvar), N, npix, C, Cp, _ptr(out), _ptr(ws), nb,
                  _stream())
        ctx.cfg = (NLL_KINDS[kind], N, npix, C, Cp)
        ctx.save_for_backward(x, mu, logvar)
        return out

    @staticmethod
    def backward(ctx, g):
        x, mu, logvar = ctx.saved_tensors
        kind, N, npix, C, Cp = ctx.cfg
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("PixelNLL: no gradient w.r.t. the data x")
        g = g.contiguous()
        dmu = torch.empty_like(mu) if ctx.needs_input_grad[1] else None
        dlv = torch.empty_like(logvar) if ctx.needs_input_grad[2] else None
        if dmu is not None or dlv is not None:
            _lib.call("acg_pixel_nll_bwd", kind, _ptr(x), _ptr(mu), _ptr(logvar), N, npix, C, Cp, _ptr(g), _ptr(dmu), _ptr(dlv),
                      _stream())
        return None, dmu, dlv, None, None


def latent_bound_step(mu, logvar, sq_mu, sq_logvar, eps, dz, nll, npx, lr, trace_row=None, eps_next=None, z_next=None,
                      alpha=0.99, rms_eps=1e-8):
    """acg_latent_bound_step: one iterate's latent tail of the bound on (N, L) tensors — KLD, the trace row (mean bound,
    mean KLD, bits per pixel), the gradient of the mean bound through the clamp of the reparametrisation, torch's RMSprop
    on (mu, logvar) in place and the next code z_next from eps_next.  dz None: only z_next from the current parameters."""
    _check(mu, logvar, sq_mu, sq_logvar, eps, dz, nll, trace_row, eps_next, z_next)
    N, L = mu.shape
    _lib.call("acg_latent_bound_step", N, L, int(npx), _ptr(mu), _ptr(logvar), _ptr(sq_mu), _ptr(sq_logvar), _ptr(eps), _ptr(dz),
              _ptr(nll), float(lr), float(alpha), float(rms_eps), _ptr(trace_row), _ptr(eps_next), _ptr(z_next), _stream())


# ----------------------------------------------------------------------------------------------
# ensemble statistics of M translations per input (model.translate_ensemble, eval_metrics.py, --metric ensemble)
# ----------------------------------------------------------------------------------------------
ENSEMBLE_MAX_M, ENSEMBLE_MAX_Q = 64, 8


def check_quantiles(quantiles):
    """-> the levels as a tuple of floats; ValueError unless 1..8 levels, sorted, inside [0, 1]"""
    q = tuple(float(v) for v in quantiles)
    if not 1 <= len(q) <= ENSEMBLE_MAX_Q:
        raise ValueError("need 1 to %d quantile levels (got %d)" % (ENSEMBLE_MAX_Q, len(q)))
    if any(not 0.0 <= v <= 1.0 for v in q) or any(b < a for a, b in zip(q, q[1:])):
        raise ValueError("quantile levels must be sorted inside [0, 1] (got %s)" % (q,))
    return q


def ensemble_outputs(N, M, C, H, W, nq, scored, device):
    """the device tensors acg_ensemble_stats writes for N inputs of M members: mean, std (N, C, H, W), quantiles
    (N, nq, C, H, W) and, when scored, crps_map (N, C, H, W), sums (N, 6) and rank_hist (N, M + 1, int32)"""
    f = dict(device=device, dtype=torch.float32)
    out = dict(mean=torch.empty((N, C, H, W), **f), std=torch.empty((N, C, H, W), **f),
               quantiles=torch.empty((N, nq, C, H, W), **f))
    if scored:
        out.update(crps_map=torch.empty((N, C, H, W), **f), sums=torch.empty((N, 6), **f),
                   rank_hist=torch.empty((N, M + 1), device=device, dtype=torch.int32))
    return out


def ensemble_stats(members_nhwc, target_nhwc, M, C, quantiles, out=None):
    """acg_ensemble_stats: members (N*M, H, W, Cp) NHWC, member m of input n at row n*M + m; target (N, H, W, Cp) or None.
    -> dict of device tensors (ensemble_outputs; `out`: such a dict to write instead, e.g. slices of larger ones).  One
    launch (plus its fold with a target), nothing read back to the host."""
    x = members_nhwc.contiguous()
    y = None if target_nhwc is None else target_nhwc.contiguous()
    _check(x, y)
    q = check_quantiles(quantiles)
    NM, H, W, Cp = x.shape
    if M < 1 or NM % M:
        raise _lib.AcgError("ensemble_stats: %d member rows are not a multiple of M=%d" % (NM, M))
    N, npix = NM // M, H * W
    if y is not None and tuple(y.shape) != (N, H, W, Cp):
        raise _lib.AcgError("ensemble_stats: target %s does not pair with members %s" % (tuple(y.shape), tuple(x.shape)))
    if out is None:
        out = ensemble_outputs(N, M, C, H, W, len(q), y is not None, x.device)
    nb = _lib.query("acg_ensemble_workspace_bytes", N, npix) if y is not None else 0
    ws = workspace(nb, slot=1) if y is not None else None
    levels = (ctypes.c_float * len(q))(*q)
    hist = out.get("rank_hist")
    _lib.call("acg_ensemble_stats", _ptr(x), _ptr(y), N, int(M), npix, int(C), Cp, levels, len(q), _ptr(out.get("mean")),
              _ptr(out.get("std")), _ptr(out.get("quantiles")), _ptr(out.get("crps_map")), _ptr(out.get("sums")), _ptr(hist),
              _ptr(ws), nb, _stream())
    return out


# ----------------------------------------------------------------------------------------------
# windows of native-resolution fields (model.translate_field, train.py --native_res)
# ----------------------------------------------------------------------------------------------
WINDOW_MAX = _lib.WINDOW_MAX


def _window_axis(extent, S, overlap):
    """origins of the windows along one axis: one when the extent is S, else ceil((extent - overlap) / (S - overlap)) of
    them, evenly spread from 0 to extent - S and rounded, so neighbours share at least `overlap` pixels"""
    if extent == S:
        return [0]
    n = -(-(extent - overlap) // (S - overlap))
    if n > WINDOW_MAX:
        raise ValueError("window_plan: %d windows of %d along an extent of %d (at most %d)" % (n, S, extent, WINDOW_MAX))
    return [int(round(k * (extent - S) / (n - 1))) for k in range(n)]


def window_plan(H, W, S, overlap):
    """The separable grid of S x S windows that covers an H x W field -> _lib.WindowPlan (acg_window_plan): H, W, S, the ramp
    R = max(overlap, 1) of the blend weight, ny, nx and the origins oy[:ny], ox[:nx] (_window_axis).  ValueError for an extent
    below S, an overlap outside 0..S//2 and more than WINDOW_MAX windows along an axis.  Pure Python, no device work."""
    H, W, S, overlap = int(H), int(W), int(S), int(overlap)
    if S < 1 or H < S or W < S:
        raise ValueError("window_plan: a %d x %d field is smaller than the %d x %d window" % (H, W, S, S))
    if not 0 <= overlap <= S // 2:
        raise ValueError("window_plan: overlap must lie in 0..%d (got %d)" % (S // 2, overlap))
    oy, ox = _window_axis(H, S, overlap), _window_axis(W, S, overlap)
    plan = _lib.WindowPlan(H=H, W=W, S=S, R=max(overlap, 1), ny=len(oy), nx=len(ox))
    plan.oy[:len(oy)], plan.ox[:len(ox)] = oy, ox
    return plan


def check_window_table(table_rows, N, H, W, S):
    """-> the rows (src, oy, ox, flip) as a (T, 4) int32 host tensor; ValueError unless every row has 0 <= src < N, 0 <= oy <= H-S,
    0 <= ox <= W-S and flip in 0..3 — the kernel does not clamp, this is the only check the rows get"""
    t = torch.as_tensor(table_rows, dtype=torch.int64, device="cpu").reshape(-1, 4)
    if t.size(0) < 1:
        raise ValueError("window table: no rows")
    lo = t.min(0).values.tolist()
    hi = t.max(0).values.tolist()
    if min(lo) < 0 or hi[0] >= N or hi[1] > H - S or hi[2] > W - S or hi[3] > 3:
        raise ValueError("window table: rows (src, oy, ox, flip) span %s..%s, outside %d fields of %d x %d with windows of %d"
                         % (lo, hi, N, H, W, S))
    return t.to(torch.int32).contiguous()


def window_gather(fields, table_rows, S, out=None, upload=None, img=True):
    """acg_window_gather: fields (N, C, H, W) NCHW -> (T, S, S, Cp) NHWC (Cp = cimg(C), or cpad(C) with img=False: ToNHWC's
    rule), row t the S x S window table_rows[t] =
    (src, oy, ox, flip) of field src (flip bit 0 mirrors x, bit 1 mirrors y), padding channels zero.  table_rows: a host
    sequence / array / tensor of T rows, checked here (check_window_table) and uploaded (`upload`: a callable that takes the
    checked (T, 4) int32 host tensor to the device, e.g. through pinned memory; default a plain copy).  `out`: a tensor to
    write instead.  One launch, nothing read back."""
    x = fields.contiguous()
    _check(x)
    N, C, H, W = x.shape
    S = int(S)
    if S < 1 or H < S or W < S:
        raise ValueError("window_gather: fields of %d x %d are smaller than the %d x %d window" % (H, W, S, S))
    tab = check_window_table(table_rows, N, H, W, S)
    tab = upload(tab) if upload is not None else tab.to(x.device)
    T, Cp = tab.size(0), cimg(C) if img else cpad(C)
    if out is None:
        out = torch.empty((T, S, S, Cp), device=x.device, dtype=torch.float32)
    _check(out)
    if tuple(out.shape) != (T, S, S, Cp):
        raise _lib.AcgError("window_gather: out %s is not %s" % (tuple(out.shape), (T, S, S, Cp)))
    _lib.call("acg_window_gather", _ptr(x), _ptr(tab), _ptr(out), N, C, H, W, T, S, Cp, _stream())
    return out


def window_blend(tiles, plan, rows, C, out=None):
    """acg_window_blend: tiles (rows*ny*nx, S, S, Cp) NHWC, tile (ky, kx) of canvas r at row (r*ny + ky)*nx + kx, blended into
    (rows, C, H, W) NCHW (`out`: such a tensor to write instead, e.g. a slice of a larger one) with the weights of `plan`
    (window_plan).  The library checks the plan.  One launch, nothing read back."""
    x = tiles.contiguous()
    _check(x, out)
    rows, C = int(rows), int(C)
    want = (rows * plan.ny * plan.nx, plan.S, plan.S)
    if x.dim() != 4 or tuple(x.shape[:3]) != want:
        raise _lib.AcgError("window_blend: tiles %s are not %s x Cp" % (tuple(x.shape), want))
    if out is None:
        out = torch.empty((rows, C, plan.H, plan.W), device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != (rows, C, plan.H, plan.W):
        raise _lib.AcgError("window_blend: out %s is not %s" % (tuple(out.shape), (rows, C, plan.H, plan.W)))
    _lib.call("acg_window_blend", _ptr(x), ctypes.byref(plan), _ptr(out), rows, C, x.size(3), _stream())
    return out


# ----------------------------------------------------------------------------------------------
# radially averaged power spectra (model.translate_spectrum, eval_metrics.py, --metric spectrum), the spectral loss on them and the
# paired cross-spectra (model.translate_coherence, eval_metrics.py, --metric coherence); both again for whole fields of any H x W
# (model.translate_field_spectrum, eval_metrics.py, --metric field_spectrum)
# ----------------------------------------------------------------------------------------------
SPECTRUM_MIN_S, SPECTRUM_MAX_S = 16, 1024


def _spectrum_size(H, W):
    if H != W or not SPECTRUM_MIN_S <= H <= SPECTRUM_MAX_S or H & (H - 1):
        raise _lib.AcgError("radial_spectrum: fields must be S x S with S a power of two in %d..%d (got %d x %d)"
                            % (SPECTRUM_MIN_S, SPECTRUM_MAX_S, H, W))
    return int(H)


def spectrum_bins(S):
    """the cells of every ring of an S x S plane -> (S/2 + 1,) int64 on the host: the bin of signed integer wavenumbers
    (fx, fy) with s = fx^2 + fy^2 is 0 for s = 0, else the largest b with b (b - 1) < s; the corners beyond S/2 are dropped"""
    import numpy as np
    S = _spectrum_size(S, S)
    f = np.arange(S, dtype=np.int64)
    f = np.where(f < S // 2, f, f - S)
    s = (f[:, None] ** 2 + f[None, :] ** 2).ravel()
    b = np.floor(np.sqrt(s.astype(np.float64))).astype(np.int64)
    b += (b * (b + 1) < s)                                         # the integer rule settles what the float root leaves open
    b -= (b * (b - 1) >= s) & (s > 0)
    return np.bincount(b[b <= S // 2], minlength=S // 2 + 1).astype(np.int64)


def _field_args(x, C, layout, what):
    """(rows, C, Cp, H, W, (row, pixel, channel) strides in floats) of a contiguous tensor in the layout; the caller applies
    its own rule for H x W (_spectrum_size, fss's 1..FSS_MAX_HW)"""
    if x.dim() != 4 or layout not in ("nhwc", "nchw"):
        raise _lib.AcgError("%s: need a 4-d tensor and layout 'nhwc' or 'nchw' (got %s, %r)" % (what, tuple(x.shape), layout))
    C = int(C)
    if layout == "nhwc":
        rows, H, W, Cp = x.shape
        strides = (H * W * Cp, Cp, 1)
    else:
        rows, Cp, H, W = x.shape
        strides = (Cp * H * W, 1, H * W)
    if not 1 <= C <= Cp or rows < 1:
        raise _lib.AcgError("%s: need rows >= 1 and 1 <= C <= %d stored channels (rows=%d, C=%d)" % (what, Cp, rows, C))
    return rows, C, Cp, int(H), int(W), strides


def _check_pairing(what, x_per_y, max_per, rows, rows_y, hw, hw_y):
    """row r of x pairs with row r / x_per_y of y, fields of one size -> x_per_y as an int, or the refusal"""
    x_per_y = int(x_per_y)
    if not 1 <= x_per_y <= max_per or rows % x_per_y:
        raise _lib.AcgError("%s: x_per_y must lie in 1..%d and divide the rows of x (rows=%d, x_per_y=%d)"
                            % (what, max_per, rows, x_per_y))
    if hw_y != hw or rows_y * x_per_y != rows:
        raise _lib.AcgError("%s: %d rows of %d x %d do not pair with %d rows of %d x %d at x_per_y=%d"
                            % ((what, rows) + hw + (rows_y,) + hw_y + (x_per_y,)))
    return x_per_y


def _paired_fields(what, x, y, C, layout_x, layout_y, size, x_per_y, max_per=None, size_y=False):
    """The preamble of the paired wrappers: both operands detached and contiguous, described by _field_args, the caller's rule
    size(H, W) -> the extents that must pair (of x; size_y: of y too), x_per_y in 1..max_per (None: the rows of x) and the
    pairing -> (x, y, rows, rows_y, C, Cp of x, extents, strides of x, strides of y, x_per_y)"""
    x, y = x.detach().contiguous(), y.detach().contiguous()
    rows, C, Cp, H, W, sx = _field_args(x, C, layout_x, what)
    rows_y, _, _, Hy, Wy, sy = _field_args(y, C, layout_y, what)
    hw = size(H, W)
    hw_y = size(Hy, Wy) if size_y else (Hy, Wy)
    x_per_y = _check_pairing(what, x_per_y, rows if max_per is None else max_per, rows, rows_y, hw, hw_y)
    return x, y, rows, rows_y, C, Cp, hw, sx, sy, x_per_y


def _refuse_out(what, out, shape, dtype=torch.float32, name="out"):
    """the refusal, on the host, of an `out` that is not a contiguous tensor of this shape and dtype (None passes)"""
    if out is not None and (tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous()):
        raise _lib.AcgError("%s: %s %s %s is not a contiguous %s %s"
                            % (what, name, tuple(out.shape), out.dtype, str(dtype).replace("torch.", ""), shape))


def _out_or_new(out, shape, dtype, device):
    """once the inputs have passed _check: `out` through its own device check (float32: _check), or a new tensor on `device`"""
    if out is None:
        return torch.empty(shape, device=device, dtype=dtype)
    if dtype == torch.float32:
        _check(out)
    elif not out.is_cuda:
        raise _lib.AcgError(_NO_CPU_PATH % out.device)
    return out


def _out_tensor(what, out, shape, inputs, strict=False, dtype=torch.float32):
    """`out` as the caller gave it, refused unless it has the shape (strict: and is contiguous of the dtype, _refuse_out), or
    a new tensor of the dtype beside inputs[0]; the inputs and out go through _check in between: after the refusals that
    need no device.  A call with several outputs does the three steps itself: _refuse_out each, one _check, _out_or_new each"""
    if strict:
        _refuse_out(what, out, shape, dtype)
    if out is not None and tuple(out.shape) != shape:
        raise _lib.AcgError("%s: out %s is not %s" % (what, tuple(out.shape), shape))
    _check(*inputs)
    return _out_or_new(out, shape, dtype, inputs[0].device)


def _metric_workspace(query, *args):
    """the workspace an entry point asks for -> (its pointer, None where it asks for none; its bytes)"""
    nbytes = _lib.query(query, *args)
    return _ptr(workspace(nbytes, slot=2) if nbytes else None), nbytes


def _radial_spectrum(x, C, layout, out=None):
    x = x.contiguous()
    _check(x, out)
    rows, C, Cp, H, W, strides = _field_args(x, C, layout, "radial_spectrum")
    S = _spectrum_size(H, W)
    out = _out_tensor("radial_spectrum", out, (rows, C, S // 2 + 1), (x,))
    ws, nbytes = _metric_workspace("acg_radial_spectrum_workspace_bytes", rows, C, S)
    _lib.call("acg_radial_spectrum", _ptr(x), rows, C, S, strides[0], strides[1], strides[2], _ptr(out), ws, nbytes, _stream())
    return out


def radial_spectrum_bwd(x, g, C, layout):
    """acg_radial_spectrum_bwd: the gradient of sum(g * radial_spectrum(x)) with respect to x, in x's layout; g (rows, C,
    S/2 + 1).  NHWC: the padded channels are written as 0.  One launch (and the ring counts') up to S = 128, three above."""
    x, g = x.contiguous(), g.contiguous()
    _check(x, g)
    rows, C, Cp, H, W, strides = _field_args(x, C, layout, "radial_spectrum_bwd")
    S = _spectrum_size(H, W)
    if tuple(g.shape) != (rows, C, S // 2 + 1):
        raise _lib.AcgError("radial_spectrum_bwd: the cotangent %s is not (%d, %d, %d)" % (tuple(g.shape), rows, C, S // 2 + 1))
    gx = torch.empty_like(x)
    ws, nbytes = _metric_workspace("acg_radial_spectrum_bwd_workspace_bytes", rows, C, S)
    _lib.call("acg_radial_spectrum_bwd", _ptr(x), _ptr(g), rows, C, Cp if layout == "nhwc" else C, S, strides[0], strides[1],
              strides[2], _ptr(gx), ws, nbytes, _stream())
    return gx


class RadialSpectrum(torch.autograd.Function):
    """radial_spectrum with its data gradient: forward acg_radial_spectrum, backward acg_radial_spectrum_bwd
    (gx = 2 Re ifft2(w fft2(x)), w the cotangent of a cell's ring over the ring's cell count)."""

    @staticmethod
    def forward(ctx, x, C, layout):
        x = x.contiguous()
        ctx.cfg = (int(C), layout)
        ctx.save_for_backward(x)
        return _radial_spectrum(x, C, layout)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        C, layout = ctx.cfg
        return radial_spectrum_bwd(x, g, C, layout), None, None


def radial_spectrum(x, C, layout, out=None):
    """acg_radial_spectrum of the C valid channels of every row of x -> (rows, C, S/2 + 1) float32 on the device.  layout
    "nhwc": x (rows, S, S, Cp) as forward_nhwc / ToNHWC give it (padded channels never reach a result); "nchw": x (rows, C, S, S).
    One launch up to S = 128, a row and a column pass above; nothing is read back to the host.  Differentiable in x
    (RadialSpectrum) when x requires grad, gradients are enabled and no `out` is given."""
    if out is None and torch.is_grad_enabled() and x.requires_grad:
        return RadialSpectrum.apply(x, C, layout)
    return _radial_spectrum(x, C, layout, out)


def spectral_loss(x, y, C, layout, eps=1e-6):
    """The squared log-spectral distance (in nepers) of the batch-mean spectra of x and y -> device scalar, differentiable in
    x: p = radial_spectrum(x).mean(0), q the same of y (detached); mean over the C channels and bins 1 .. S/2 of
    (ln(p + eps) - ln(q + eps))^2.  Bin 0 (the mean) takes no part, as in eval_metrics.log_spectral_distance.  eps belongs to the
    definition: above the forward's absolute floor in an empty bin (~2.8e-7 for fields in [-1, 1]), below any populated bin.
    x and y need not pair (nor hold the same number of rows)."""
    p = radial_spectrum(x, C, layout).mean(0)
    with torch.no_grad():
        q = _radial_spectrum(y.detach(), C, layout).mean(0)
    d = torch.log(p[:, 1:] + eps) - torch.log(q[:, 1:] + eps)
    return (d * d).mean()


def cross_spectrum(x, y, C, layout_x, layout_y, x_per_y=1, out=None):
    """acg_cross_spectrum: the paired cross-spectra of the C valid channels of x and y -> (rows, C, 3, S/2 + 1) float32 on the
    device holding, per ring, the means of Pxx = |X|^2 / S^2, Pyy = |Y|^2 / S^2 and the co-spectrum Cxy = Re(X conj Y) / S^2
    in that order (X = fft2(x), Y = fft2(y); the rings of radial_spectrum).  Row r of x pairs with row r / x_per_y of y: the
    x_per_y members of an ensemble share one truth.  Each operand has its own layout ("nhwc" or "nchw", as radial_spectrum
    takes them).  One launch up to S = 64, a row and a column pass above; nothing is read back to the host.  Not
    differentiable."""
    x, y, rows, _, C, _, (S, _), sx, sy, x_per_y = _paired_fields("cross_spectrum", x, y, C, layout_x, layout_y,
                                                                  lambda H, W: (_spectrum_size(H, W),) * 2, x_per_y, size_y=True)
    out = _out_tensor("cross_spectrum", out, (rows, C, 3, S // 2 + 1), (x, y))
    ws, nbytes = _metric_workspace("acg_cross_spectrum_workspace_bytes", rows, C, S)
    _lib.call("acg_cross_spectrum", _ptr(x), _ptr(y), rows, x_per_y, C, S, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], _ptr(out),
              ws, nbytes, _stream())
    return out


FIELD_SPECTRUM_MIN, FIELD_SPECTRUM_MAX = 16, 1024


def _field_spectrum_size(what, H, W):
    if not (FIELD_SPECTRUM_MIN <= H <= FIELD_SPECTRUM_MAX and FIELD_SPECTRUM_MIN <= W <= FIELD_SPECTRUM_MAX):
        raise _lib.AcgError("%s: fields must be H x W with both extents in %d..%d (got %d x %d)"
                            % (what, FIELD_SPECTRUM_MIN, FIELD_SPECTRUM_MAX, H, W))
    return int(H), int(W)


def field_spectrum_bins(H, W):
    """the rings of an H x W field: bins 0 .. min(H, W) // 2 -> nb.  Pure Python."""
    H, W = _field_spectrum_size("field_spectrum_bins", int(H), int(W))
    return min(H, W) // 2 + 1


def field_spectrum(x, C, layout, out=None):
    """acg_field_spectrum: radial_spectrum for whole fields of any H x W with both extents in 16 .. 1024 -> (rows, C, nb)
    float32 on the device, nb = min(H, W) // 2 + 1.  P = |fft2(x)|^2 / (H W) averaged over elliptical rings: ring b holds the
    cells whose radius L sqrt((fy/H)^2 + (fx/W)^2), L = min(H, W), rounds to b ("b cycles per L pixels" along either axis;
    the integer rule of tests/field_spectrum_ref.py).  Layouts as radial_spectrum takes them.  A length that is no power of
    two is transformed by Bluestein's chirp-z on the HIP FFT's stages; H = W a power of two gives radial_spectrum's bits.
    Nothing is read back to the host.  Not differentiable."""
    x = x.detach().contiguous()
    rows, C, _, H, W, strides = _field_args(x, C, layout, "field_spectrum")
    H, W = _field_spectrum_size("field_spectrum", H, W)
    out = _out_tensor("field_spectrum", out, (rows, C, field_spectrum_bins(H, W)), (x,))
    ws, nbytes = _metric_workspace("acg_field_spectrum_workspace_bytes", rows, C, H, W)
    _lib.call("acg_field_spectrum", _ptr(x), rows, C, H, W, strides[0], strides[1], strides[2], _ptr(out), ws, nbytes, _stream())
    return out


def field_cross_spectrum(x, y, C, layout_x, layout_y, x_per_y=1, out=None):
    """acg_field_cross_spectrum: cross_spectrum for whole fields of any H x W with both extents in 16 .. 1024 ->
    (rows, C, 3, nb) float32 on the device: per ring of field_spectrum the means of Pxx, Pyy and Cxy = Re(X conj Y) / (H W).
    Pairing and layouts as cross_spectrum; Pxx has the bits of field_spectrum(x); H = W a power of two gives
    cross_spectrum's bits.  The triples go to coherence_summary as cross_spectrum's do.  Not differentiable."""
    x, y, rows, _, C, _, (H, W), sx, sy, x_per_y = _paired_fields(
        "field_cross_spectrum", x, y, C, layout_x, layout_y,
        lambda H, W: _field_spectrum_size("field_cross_spectrum", H, W), x_per_y)
    out = _out_tensor("field_cross_spectrum", out, (rows, C, 3, field_spectrum_bins(H, W)), (x, y))
    ws, nbytes = _metric_workspace("acg_field_cross_spectrum_workspace_bytes", rows, C, H, W)
    _lib.call("acg_field_cross_spectrum", _ptr(x), _ptr(y), rows, x_per_y, C, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2],
              _ptr(out), ws, nbytes, _stream())
    return out


def coherence_summary(sums):
    """(..., 3, nb) triples (pxx, pyy, cxy) summed over a set of pairs -> dict of float64 arrays on the host:
      coh   (..., nb)  the spectral coherence (sum cxy)^2 / (sum pxx sum pyy), in [0, 1] by Cauchy-Schwarz, 0 where the
                       denominator is 0;
      r     (..., nb)  the signed correlation sum cxy / sqrt(sum pxx sum pyy), 0 where the denominator is 0;
      perr  (..., nb)  the error spectrum pxx + pyy - 2 cxy: the radial spectrum of x - y (the summed one, as the triples are);
      k_eff (...)      int64, the effective resolution: the smallest bin b >= 1 with coh[b] < 0.5, nb if there is none.
    The sums matter: the ring-wise coherence of ONE pair is noisy where a ring has few cells (independent fields reach 0.3-0.6
    in bins 1-3), so a metric pools the triples over its split before it divides."""
    import numpy as np
    t = np.asarray(sums, dtype=np.float64)
    if t.ndim < 2 or t.shape[-2] != 3:
        raise ValueError("coherence_summary: need (..., 3, nb) triples (got %s)" % (t.shape,))
    pxx, pyy, cxy = t[..., 0, :], t[..., 1, :], t[..., 2, :]
    den = pxx * pyy
    ok = den > 0
    safe = np.where(ok, den, 1.0)
    coh = np.where(ok, np.minimum(cxy * cxy / safe, 1.0), 0.0)
    r = np.where(ok, np.clip(cxy / np.sqrt(safe), -1.0, 1.0), 0.0)
    nb = t.shape[-1]
    low = coh[..., 1:] < 0.5
    k_eff = np.where(low.any(-1), low.argmax(-1) + 1, nb).astype(np.int64)
    return dict(coh=coh, r=r, perr=pxx + pyy - 2.0 * cxy, k_eff=k_eff)


# ----------------------------------------------------------------------------------------------
# the marginal loss (the marg record of losses.py, --lambda_marg_A / --lambda_marg_B): sorted fields and the distance of two
# batches' mean quantile functions
# ----------------------------------------------------------------------------------------------
FIELD_SORT_MAX_P = 1 << 20


def _field_sort_size(what, H, W):
    if H < 1 or W < 1 or H * W > FIELD_SORT_MAX_P:
        raise _lib.AcgError("%s: fields must hold 1 .. %d pixels (got %d x %d)" % (what, FIELD_SORT_MAX_P, H, W))
    return int(H * W)


def field_sort(x, C, layout, want_rank=True):
    """acg_field_sort of the C valid channels of every row of x -> (sorted, rank): sorted (rows, C, H W) float32, each field's
    values in ascending order, and rank (rows, C, H W) int32, the position of every pixel in that order (None with
    want_rank=False).  Pixel p comes before q iff x[p] < x[q], or x[p] == x[q] and p < q (-0.0 and +0.0 tie; a stable
    argsort).  layout "nhwc": x (rows, H, W, Cp), padded channels never read; "nchw": x (rows, C, H, W).  Both outputs are
    planar and hold the same bits in either layout.  H W <= 2^20.  Nothing is read back to the host.  Not differentiable."""
    x = x.detach().contiguous()
    rows, C, Cp, H, W, strides = _field_args(x, C, layout, "field_sort")
    P = _field_sort_size("field_sort", H, W)
    _check(x)
    srt = torch.empty((rows, C, P), device=x.device, dtype=torch.float32)
    rank = torch.empty((rows, C, P), device=x.device, dtype=torch.int32) if want_rank else None
    ws, nbytes = _metric_workspace("acg_field_sort_workspace_bytes", rows, C, H, W)
    _lib.call("acg_field_sort", _ptr(x), rows, C, H, W, strides[0], strides[1], strides[2], _ptr(srt), _ptr(rank), ws, nbytes,
              _stream())
    return srt, rank


class MarginalLoss(torch.autograd.Function):
    """marginal_loss with its data gradient in x: forward acg_field_sort of both batches and acg_marginal_loss_fwd, backward
    acg_marginal_loss_bwd, a gather of the saved quantile differences d through the saved ranks of x, scaled by the upstream
    gradient on the device."""

    @staticmethod
    def forward(ctx, x, y, C, layout):
        x, y = x.detach().contiguous(), y.detach().contiguous()
        rows, C, Cp, H, W, strides = _field_args(x, C, layout, "marginal_loss")
        rows_y, _, _, Hy, Wy, _ = _field_args(y, C, layout, "marginal_loss")
        P = _field_sort_size("marginal_loss", H, W)
        if (Hy, Wy) != (H, W):
            raise _lib.AcgError("marginal_loss: fields of %d x %d against fields of %d x %d" % (H, W, Hy, Wy))
        sx, rank = field_sort(x, C, layout, want_rank=ctx.needs_input_grad[0])
        sy, _ = field_sort(y, C, layout, want_rank=False)
        d = torch.empty((C, P), device=x.device, dtype=torch.float32)
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        ws, nbytes = _metric_workspace("acg_marginal_loss_workspace_bytes", C, P)
        _lib.call("acg_marginal_loss_fwd", _ptr(sx), rows, _ptr(sy), rows_y, C, P, _ptr(d), _ptr(loss), ws, nbytes, _stream())
        ctx.cfg = (rows, C, Cp if layout == "nhwc" else C, H, W, strides, tuple(x.shape))
        if rank is not None:
            ctx.save_for_backward(d, rank)
        return loss

    @staticmethod
    def backward(ctx, g):
        d, rank = ctx.saved_tensors
        rows, C, Cp, H, W, strides, shape = ctx.cfg
        g = g.detach().to(torch.float32).contiguous()
        gx = torch.empty(shape, device=d.device, dtype=torch.float32)
        _lib.call("acg_marginal_loss_bwd", _ptr(d), _ptr(rank), _ptr(g), rows, C, Cp, H, W, strides[0], strides[1], strides[2],
                  _ptr(gx), _stream())
        return gx, None, None, None


def marginal_loss(x, y, C, layout):
    """The squared 2-Wasserstein distance of the value distributions of two batches, averaged over the C channels -> device
    scalar, differentiable in x: with s_x the sorted fields (field_sort), Q_x[c, k] = mean over the rows of s_x[r, c, k] (the
    batch's mean quantile function, its Wasserstein barycentre) and the same for y (detached), mean over c, k of
    (Q_x - Q_y)^2.  d loss / d x[r, c, p] = 2 (Q_x - Q_y)[c, rank_x[r, c, p]] / (C H W rows_x): a gather, deterministic.  x and y
    share the layout and the field size but need not pair (nor hold the same number of rows).  No host synchronisation."""
    return MarginalLoss.apply(x, y, C, layout)


# ----------------------------------------------------------------------------------------------
# the marginal evaluator (model.translate_marginal, eval_metrics.py, --metric marginal): Wasserstein distances, quantiles and counts
# below thresholds from the sorted fields
# ----------------------------------------------------------------------------------------------
MARG_MAX_LEVELS, MARG_MAX_EDGES = 16, 256


def check_levels(levels):
    """-> the quantile levels as a tuple of floats; ValueError unless at most 16 of them, each inside [0, 1] (any order)"""
    q = tuple(float(v) for v in levels)
    if len(q) > MARG_MAX_LEVELS:
        raise ValueError("need at most %d quantile levels (got %d)" % (MARG_MAX_LEVELS, len(q)))
    if any(not 0.0 <= v <= 1.0 for v in q):
        raise ValueError("quantile levels must lie inside [0, 1] (got %s)" % (q,))
    return q


def _marginal_edges(what, edges, C, device):
    """edges as sorted_scores takes them -> channel_table's (C, E) tensor on the device, E <= 256; None for none or for E = 0"""
    if edges is None:
        return None
    return channel_table(what, _lib.AcgError, "edges", edges, C, MARG_MAX_EDGES, device, none_if_empty=True)


def sorted_scores(sx, sy, levels=(), edges=None, x_per_y=1, out=None):
    """acg_marginal_scores on already sorted fields: sx (rows, C, P) float32, every field ascending (field_sort's first
    result), sy (rows / x_per_y, C, P) the same of the paired truths, or None; row r of sx pairs with row r / x_per_y of sy.
    -> dict of device tensors, holding only what was asked for:
      w     (rows, C, 2) float64, with sy: w1 = mean_k |sx[k] - sy[k]| and w2sq = mean_k (sx[k] - sy[k])^2, the 1-Wasserstein
            and the squared 2-Wasserstein distance of the two fields' value distributions, summed in double;
      q     (rows, C, L) float32, with L = len(levels) > 0 (check_levels): np.quantile(field, level, method="linear"),
            evaluated in double and rounded once;
      below (rows, C, E) int32, with edges (C, E) float32 (device tensor or host array), E > 0: the number of values below
            edges[c][e], exact; P - below counts fss's events [x >= thr].
    `out`: such a dict to write instead (e.g. slices of larger tensors), with exactly those entries.  One launch, the same bits
    on every call; nothing is read back to the host.  Not differentiable."""
    what = "sorted_scores"
    if sx.dim() != 3 or (sy is not None and sy.dim() != 3):
        raise _lib.AcgError("%s: sorted fields are (rows, C, P) (got %s, %s)"
                            % (what, tuple(sx.shape), None if sy is None else tuple(sy.shape)))
    sx = sx.detach().contiguous()
    rows, C, P = (int(v) for v in sx.shape)
    if rows < 1 or C < 1 or not 1 <= P <= FIELD_SORT_MAX_P:
        raise _lib.AcgError("%s: need rows >= 1, C >= 1 and fields of 1 .. %d pixels (got %s)" % (what, FIELD_SORT_MAX_P, tuple(sx.shape)))
    if sy is not None:
        sy = sy.detach().contiguous()
        if sy.size(1) != C:
            raise _lib.AcgError("%s: %d channels against %d" % (what, C, sy.size(1)))
        x_per_y = _check_pairing(what, x_per_y, rows, rows, sy.size(0), (1, P), (1, sy.size(2)))
    else:
        x_per_y = 1
    try:
        lv = check_levels(levels)
    except ValueError as e:
        raise _lib.AcgError("%s: %s" % (what, e))
    edges = _marginal_edges(what, edges, C, sx.device)
    L, E = len(lv), 0 if edges is None else int(edges.size(1))
    if sy is None and L == 0 and E == 0:
        raise _lib.AcgError("%s: nothing to compute (no sy, no levels, no edges)" % what)
    want = {}
    if sy is not None:
        want["w"] = ((rows, C, 2), torch.float64)
    if L:
        want["q"] = ((rows, C, L), torch.float32)
    if E:
        want["below"] = ((rows, C, E), torch.int32)
    if out is not None:
        if set(out) != set(want):
            raise _lib.AcgError("%s: out holds %s, the call writes %s" % (what, sorted(out), sorted(want)))
        for k, (shape, dtype) in want.items():
            _refuse_out(what, out[k], shape, dtype, "out[%r]" % k)
    _check(sx, sy, edges)                                          # after the refusals that need no device
    out = {k: _out_or_new(None if out is None else out[k], shape, dtype, sx.device) for k, (shape, dtype) in want.items()}
    _lib.call("acg_marginal_scores", _ptr(sx), _ptr(sy), rows, x_per_y, C, P, (ctypes.c_double * max(L, 1))(*lv), L, _ptr(edges), E,
              _ptr(out.get("w")), _ptr(out.get("q")), _ptr(out.get("below")), _stream())
    return out


def marginal_scores(x, y, C, layout_x, layout_y, levels=(), edges=None, x_per_y=1):
    """The value distribution of the C valid channels of every field of x against its paired truth y (or None): field_sort of
    both operands (no ranks), then sorted_scores -> its dict: w (rows, C, 2) float64 with y, q (rows, C, L) float32 with levels,
    below (rows, C, E) int32 with edges.  Row r of x pairs with row r / x_per_y of y.  Each operand has its own layout ("nhwc"
    or "nchw", as field_sort takes them; padded channels never reach a result).  H W <= 2^20.  Nothing is read back to the
    host.  Not differentiable."""
    what = "marginal_scores"
    if y is None:
        x = x.detach().contiguous()
        rows, C, _, H, W, _ = _field_args(x, C, layout_x, what)
        _field_sort_size(what, H, W)
    else:
        x, y, rows, _, C, _, _, _, _, x_per_y = _paired_fields(what, x, y, C, layout_x, layout_y,
                                                              lambda H, W: (1, _field_sort_size(what, H, W)), x_per_y, size_y=True)
    try:
        lv = check_levels(levels)
    except ValueError as e:
        raise _lib.AcgError("%s: %s" % (what, e))
    edges = _marginal_edges(what, edges, C, x.device)
    if y is None and not lv and edges is None:                     # before the sorts are launched
        raise _lib.AcgError("%s: nothing to compute (no y, no levels, no edges)" % what)
    sx, _ = field_sort(x, C, layout_x, want_rank=False)
    sy = None if y is None else field_sort(y, C, layout_y, want_rank=False)[0]
    return sorted_scores(sx, sy, lv, edges, x_per_y)


def marginal_summary(below, cells, below_real, cells_real):
    """counts below the E edges summed over a set of fields (C, E) int64 with the number of cells they were counted in, of the
    generated and of the real fields -> dict of float64 arrays on the host: cdf, cdf_real (C, E) = below / cells, the pooled
    empirical distribution functions at the edges (strictly below), and ks (C,), the Kolmogorov-Smirnov distance at the edges:
    the maximum over the edges of |cdf - cdf_real| (0 without edges)"""
    import numpy as np
    b, r = np.asarray(below, dtype=np.int64), np.asarray(below_real, dtype=np.int64)
    if b.ndim != 2 or b.shape != r.shape or int(cells) < 1 or int(cells_real) < 1:
        raise ValueError("marginal_summary: need two (C, E) count arrays and positive cell counts (got %s, %s, %s, %s)"
                         % (b.shape, r.shape, cells, cells_real))
    cdf, cdf_real = b.astype(np.float64) / float(int(cells)), r.astype(np.float64) / float(int(cells_real))
    ks = np.abs(cdf - cdf_real).max(axis=1) if b.shape[1] else np.zeros(b.shape[0], dtype=np.float64)
    return dict(cdf=cdf, cdf_real=cdf_real, ks=ks)


# ----------------------------------------------------------------------------------------------
# structural similarity (the ssim record of losses.py, --lambda_ssim_A / --lambda_ssim_B; model.translate_ssim, eval_metrics.py, --metric ssim)
# ----------------------------------------------------------------------------------------------
SSIM_WINDOW, SSIM_MAX_HW = 11, 1024


def _ssim_size(what, H, W):
    if not (SSIM_WINDOW <= H <= SSIM_MAX_HW and SSIM_WINDOW <= W <= SSIM_MAX_HW):
        raise _lib.AcgError("%s: fields must be H x W with %d <= H, W <= %d (got %d x %d)" % (what, SSIM_WINDOW, SSIM_MAX_HW, H, W))
    return int(H), int(W)


def _ssim_range(what, data_range):
    L = float(data_range)
    if not 0.0 < L < float("inf"):
        raise _lib.AcgError("%s: data_range must be positive and finite (got %r)" % (what, data_range))
    return L


def _ssim_call(x, y, sizes, sx, sy, x_per_y, L, out, maps):
    rows, C, H, W = sizes
    ws, nbytes = _metric_workspace("acg_ssim_workspace_bytes", rows, C, H, W)
    _lib.call("acg_ssim", _ptr(x), _ptr(y), rows, x_per_y, C, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], ctypes.c_float(L),
              _ptr(out), _ptr(maps), ws, nbytes, _stream())


def ssim(x, y, C, layout_x, layout_y, x_per_y=1, data_range=2.0, out=None):
    """acg_ssim: the structural similarity of the C valid channels of x against y -> (rows, C, 2) float32 on the device: per
    (row, channel) the mean of S and the mean of the contrast-structure factor cs over the (H - 10) x (W - 10) valid positions
    of the separable 11 x 11 Gaussian window, sigma 1.5 (Wang et al. 2004; C1 = (0.01 L)^2, C2 = (0.03 L)^2, L = data_range, 2
    for fields in [-1, 1]; tests/ssim_ref.py).  Row r of x pairs with row r / x_per_y of y.  Each operand has its own layout
    ("nhwc" or "nchw", as radial_spectrum takes them; padded channels never reach a result).  11 <= H, W <= 1024.  Two
    launches, the same bits for every layout; nothing is read back to the host.  Not differentiable (ssim_loss is)."""
    x, y, rows, _, C, _, (H, W), sx, sy, x_per_y = _paired_fields("ssim", x, y, C, layout_x, layout_y,
                                                                  lambda H, W: _ssim_size("ssim", H, W), x_per_y)
    L = _ssim_range("ssim", data_range)
    out = _out_tensor("ssim", out, (rows, C, 2), (x, y), strict=True)
    _ssim_call(x, y, (rows, C, H, W), sx, sy, x_per_y, L, out, None)
    return out


class SsimLoss(torch.autograd.Function):
    """ssim_loss with its data gradient in x: forward acg_ssim (storing the derivative maps a, b, c of every window position
    only when x needs a gradient), backward acg_ssim_bwd: the maps through the window once more and the point-wise combine
    with x and y, scaled by the upstream gradient on the device."""

    @staticmethod
    def forward(ctx, x, y, C, layout, data_range):
        x, y, rows, _, C, Cp, (H, W), strides, sy, _ = _paired_fields("ssim_loss", x, y, C, layout, layout,
                                                                      lambda H, W: _ssim_size("ssim_loss", H, W), 1, max_per=1)
        L = _ssim_range("ssim_loss", data_range)
        out = _out_tensor("ssim_loss", None, (rows, C, 2), (x, y))
        maps = None
        if ctx.needs_input_grad[0]:
            maps = torch.empty((3, rows, C, H - SSIM_WINDOW + 1, W - SSIM_WINDOW + 1), device=x.device, dtype=torch.float32)
        _ssim_call(x, y, (rows, C, H, W), strides, sy, 1, L, out, maps)
        ctx.cfg = (rows, C, Cp if layout == "nhwc" else C, H, W, strides, sy)
        ctx.has_maps = maps is not None
        if maps is not None:
            ctx.save_for_backward(maps, x, y)
        return 1.0 - out[:, :, 0].mean()

    @staticmethod
    def backward(ctx, g):
        maps, x, y = ctx.saved_tensors
        rows, C, Cp, H, W, sx, sy = ctx.cfg
        g = g.detach().to(torch.float32).contiguous()
        gx = torch.empty_like(x)
        _lib.call("acg_ssim_bwd", _ptr(maps), _ptr(x), _ptr(y), _ptr(g), rows, C, Cp, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2],
                  _ptr(gx), _stream())
        return gx, None, None, None, None


def ssim_loss(x, y, C, layout, data_range=2.0):
    """1 - the mean over the rows and the C valid channels of ssim's mean S -> device scalar, differentiable in x (y is
    detached).  x and y share the layout and pair row by row.  With a = dS/d mu_x (total), b = dS/dE[x^2], c = dS/dE[xy] per
    window position, d loss / d x(q) = -((w * a)(q) + 2 x(q) (w * b)(q) + y(q) (w * c)(q)) / (rows C (H - 10) (W - 10)), * the
    full correlation with the window: gathers, deterministic.  NHWC: the padded channels of the gradient are 0.  No host
    synchronisation.  Under torch.no_grad(), or for an x that needs no gradient, the derivative maps are neither computed nor
    allocated."""
    return SsimLoss.apply(x if torch.is_grad_enabled() else x.detach(), y, C, layout, data_range)


# ----------------------------------------------------------------------------------------------
# the CRPS training loss of M translations per input (losses._crps_term: the paired step under --lambda_crps_B; tests/crps_ref.py)
# ----------------------------------------------------------------------------------------------
CRPS_MAX_HW, CRPS_MAX_M = 1024, 16


def crps_weight(M, alpha):
    """w of the score e1 - w e2 of M members, e2 the sum of |x_i - x_j| over the pairs i < j: alpha / (M (M - 1)) +
    (1 - alpha) / M^2, 0 for M = 1.  alpha = 1: the fair CRPS (Ferro 2014), alpha = 0: the ensemble CRPS, between them the
    almost fair score (Lang et al. 2024).  ValueError for M outside 1..16 or alpha outside [0, 1]."""
    M, a = int(M), float(alpha)
    if not 1 <= M <= CRPS_MAX_M:
        raise ValueError("members must lie in 1..%d (got %d)" % (CRPS_MAX_M, M))
    if not 0.0 <= a <= 1.0:
        raise ValueError("alpha must lie in [0, 1] (got %r)" % (alpha,))
    return 0.0 if M == 1 else a / (M * (M - 1)) + (1.0 - a) / (M * M)


def _crps_size(H, W):
    if not (1 <= H <= CRPS_MAX_HW and 1 <= W <= CRPS_MAX_HW):
        raise _lib.AcgError("crps_loss: fields must be H x W with 1 <= H, W <= %d (got %d x %d)" % (CRPS_MAX_HW, H, W))
    return int(H), int(W)


def _crps_call(x, y, sizes, sx, sy, M, out):
    rows, C, H, W = sizes
    ws, nbytes = _metric_workspace("acg_crps_workspace_bytes", rows, M, C, H, W)
    _lib.call("acg_crps_fwd", _ptr(x), _ptr(y), rows, M, C, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], _ptr(out), ws, nbytes,
              _stream())


class CrpsLoss(torch.autograd.Function):
    """crps_loss with its data gradient in x: forward acg_crps_fwd (the sums of e1 and e2 per input and channel, in double)
    and the scalar combine on the device; backward acg_crps_bwd, which recomputes the signs from x and y (nothing but the two
    operands is kept, and those only when x needs a gradient) and scales by the upstream gradient on the device."""

    @staticmethod
    def forward(ctx, x, y, C, layout_x, layout_y, members, alpha):
        if not 0.0 <= float(alpha) <= 1.0:
            raise _lib.AcgError("crps_loss: alpha must lie in [0, 1] (got %r)" % (alpha,))
        x, y, rows, N, C, Cp, (H, W), sx, sy, M = _paired_fields("crps_loss", x, y, C, layout_x, layout_y, _crps_size, members,
                                                                 max_per=CRPS_MAX_M, size_y=True)
        w = crps_weight(M, alpha)
        out = _out_tensor("crps_loss", None, (N, C, 2), (x, y), dtype=torch.float64)
        _crps_call(x, y, (rows, C, H, W), sx, sy, M, out)
        cells = N * C * H * W
        tot = out.sum((0, 1))
        loss = ((tot[0] - w * tot[1]) / cells).float()
        e1 = (tot[0] / cells).float()
        pair = (tot[1] * (2.0 / (M * (M - 1) * cells))).float() if M > 1 else torch.zeros_like(e1)
        ctx.mark_non_differentiable(e1, pair)
        if ctx.needs_input_grad[0]:
            ctx.cfg = (rows, M, C, Cp, H, W, sx, sy, 1.0 / (M * cells), w / cells)
            ctx.save_for_backward(x, y)
        return loss, e1, pair

    @staticmethod
    def backward(ctx, g, _e1, _pair):
        x, y = ctx.saved_tensors
        rows, M, C, Cp, H, W, sx, sy, coef_y, coef_pair = ctx.cfg
        g = g.detach().to(torch.float32).contiguous()
        dx = torch.empty_like(x)
        _lib.call("acg_crps_bwd", _ptr(x), _ptr(y), _ptr(g), rows, M, C, Cp, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2],
                  ctypes.c_double(coef_y), ctypes.c_double(coef_pair), _ptr(dx), _stream())
        return dx, None, None, None, None, None, None


def crps_loss(x, y, C, layout_x, layout_y, members, alpha=0.95, parts=False):
    """The almost fair CRPS of `members` translations per input against their truth -> float32 device scalar, differentiable in
    x (y is detached).  x holds rows = N members fields, member m of input n at row n members + m (ensemble_stats's order); y
    the N truths; each operand has its own layout ("nhwc" or "nchw").  Per cell (input, valid channel, pixel)
    s = (1/M) sum_i |x_i - y| - w sum_{i<j} |x_i - x_j|, w = crps_weight(M, alpha); the loss is the mean of s over N, the C
    valid channels and the H W pixels (M = 1: the mean absolute error).  alpha = 1 equals ensemble_stats's fair CRPS, alpha = 0
    its crps.  d loss / d x_i = g (sign(x_i - y) / M - w sum_{j != i} sign(x_i - x_j)) / (N C H W) with sign(0) = 0; NHWC: the
    padded channels of the gradient are 0.  parts=True: (loss, e1, pair), the detached scalars e1 = the mean of (1/M) sum_i
    |x_i - y| and pair = the mean over cells of the mean |x_i - x_j| over i != j (0 for M = 1).  1 <= H, W <= 1024, members in
    1..16.  acg_crps_fwd sums in double in a fixed order (the same bits in every layout), acg_crps_bwd recomputes the signs; no
    host synchronisation.  Under torch.no_grad(), or for an x that needs no gradient, nothing is saved."""
    loss, e1, pair = CrpsLoss.apply(x if torch.is_grad_enabled() else x.detach(), y, C, layout_x, layout_y, members, alpha)
    return (loss, e1, pair) if parts else loss


# ----------------------------------------------------------------------------------------------
# neighbourhood fractions skill scores (model.translate_fss, eval_metrics.py, --metric fss)
# ----------------------------------------------------------------------------------------------
FSS_MAX_HW, FSS_MAX_T, FSS_MAX_NW, FSS_MAX_M = 1024, 8, 8, 64


def check_windows(windows):
    """-> the window widths as a tuple of ints; ValueError unless 1..8 odd positive widths"""
    w = tuple(int(v) for v in windows)
    if not 1 <= len(w) <= FSS_MAX_NW:
        raise ValueError("need 1 to %d windows (got %d)" % (FSS_MAX_NW, len(w)))
    if any(v < 1 or v % 2 == 0 or v != f for v, f in zip(w, windows)):
        raise ValueError("windows must be odd positive integers (got %s)" % (tuple(windows),))
    return w


def _fss_size(H, W):
    if not (1 <= H <= FSS_MAX_HW and 1 <= W <= FSS_MAX_HW):
        raise _lib.AcgError("fss: fields must be H x W with 1 <= H, W <= %d (got %d x %d)" % (FSS_MAX_HW, H, W))
    return H, W


def fss(x, y, C, layout_x, layout_y, thresholds, windows, x_per_y=1, ensemble=False, out=None):
    """acg_fss: the fractions-skill-score triples of the C valid channels of x against y -> (rows, C, T, nw, 3) int64 on the
    device: per threshold thresholds[c][t] and odd window n the sums over the H x W cells of cf^2, co^2 and cf co, cf / co the
    counts of the events [x >= t] / [y >= t] (NaN is no event) in the centred n x n window of each cell, cells outside the
    domain counting 0.  Exact integers, the same bits in every layout.  Row r of x pairs with row r / x_per_y of y.
    thresholds: (C, T) float32 on the device, or a host array (copied to the device).  ensemble=True returns (out, ens) with ens
    (rows / x_per_y, C, T, nw, 3) the triples (sum E^2, sum co^2, sum E co) of E = the members' summed counts; with x_per_y = 1
    ens equals out.  `out`: the (rows, C, T, nw, 3) int64 tensor to write, or with ensemble=True the pair (out, ens).
    Sum the triples over a set of pairs, then ops.fss_summary.  Nothing is read back to the host.  Not differentiable."""
    x, y, rows, rows_y, C, _, (H, W), sx, sy, x_per_y = _paired_fields("fss", x, y, C, layout_x, layout_y, _fss_size, x_per_y,
                                                                       max_per=FSS_MAX_M, size_y=True)
    try:
        win = check_windows(windows)
    except ValueError as e:
        raise _lib.AcgError("fss: %s" % e)
    thr = channel_table("fss", _lib.AcgError, "thresholds", thresholds, C, FSS_MAX_T, None)
    T, nw = int(thr.size(1)), len(win)
    o, e = (out if ensemble else (out, None)) if out is not None else (None, None)
    shapes = ((rows, C, T, nw, 3), (rows_y, C, T, nw, 3))
    _refuse_out("fss", o, shapes[0], torch.int64)
    _refuse_out("fss", e, shapes[1], torch.int64, "ens")
    if not torch.is_tensor(thresholds):                            # a host array goes to the device; a tensor is where it has to be
        thr = thr.to(x.device)
    _check(x, y, thr)                                              # after the refusals that need no device
    o = _out_or_new(o, shapes[0], torch.int64, x.device)
    if ensemble:
        e = _out_or_new(e, shapes[1], torch.int64, x.device)
    ws, nbytes = _metric_workspace("acg_fss_workspace_bytes", rows, x_per_y, C, H, W, T, nw, int(ensemble))
    _lib.call("acg_fss", _ptr(x), _ptr(y), rows, x_per_y, C, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], _ptr(thr), T,
              (ctypes.c_int * nw)(*win), nw, _ptr(o), _ptr(e), ws, nbytes, _stream())
    return (o, e) if ensemble else o


def fss_summary(sums, windows, cells, members=1):
    """(..., T, nw, 3) int64 triples (sum cf^2, sum co^2, sum cf co) summed over a set of pairs of `cells` cells in all ->
    dict of float64 arrays on the host:
      fss (..., T, nw)   2 sum cf co / (sum cf^2 + sum co^2), NaN where the denominator is 0 (no event on either side).
                         members = M > 1: the triples are the ensemble's (sum E^2, sum co^2, sum E co) and the score is the
                         probabilistic FSS_prob = 2 M sum E co / (sum E^2 + M^2 sum co^2);
    and, when 1 is among the windows (its counts are the events themselves):
      bias (..., T)      the frequency bias, forecast events / observed events (forecast events / M for an ensemble), NaN
                         without observed events;
      csi (..., T)       hits / (forecast + observed - hits), NaN where that is 0;
      base_rate (..., T) observed events / cells;
      useful_scale (..., T) int64: the smallest listed window with fss >= 0.5 + base_rate / 2, 0 if none qualifies."""
    import numpy as np
    t = np.asarray(sums)
    win = check_windows(windows)
    if t.ndim < 3 or t.shape[-1] != 3 or t.shape[-2] != len(win):
        raise ValueError("fss_summary: need (..., T, %d, 3) triples (got %s)" % (len(win), t.shape))
    M = float(int(members))
    if M < 1:
        raise ValueError("fss_summary: members must be at least 1 (got %s)" % (members,))
    t = t.astype(np.float64)
    ff, oo, fo = t[..., 0], t[..., 1], t[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        den = ff + M * M * oo
        res = dict(fss=np.where(den > 0, 2.0 * M * fo / den, np.nan))
        if 1 in win:
            k = win.index(1)
            f1, o1, h1 = ff[..., k] / M, oo[..., k], fo[..., k] / M
            union = f1 + o1 - h1
            res["bias"] = np.where(o1 > 0, f1 / o1, np.nan)
            res["csi"] = np.where(union > 0, h1 / union, np.nan)
            res["base_rate"] = o1 / float(cells)
            ok = res["fss"] >= (0.5 + res["base_rate"] / 2.0)[..., None]     # NaN compares false
            order = np.argsort(win)
            first = ok[..., order].argmax(-1)
            res["useful_scale"] = np.where(ok.any(-1), np.asarray(win, dtype=np.int64)[order][first], 0).astype(np.int64)
    return res


def fss_scale_levels(H, W):
    """nl = L + 1 levels of fss_scales on H x W cells, L = ceil(log2(max(H, W))): 1 x 1 has one, 1024 eleven"""
    H, W = _fss_size(int(H), int(W))
    return (max(H, W) - 1).bit_length() + 1


def fss_scales(x, y, C, layout_x, layout_y, thresholds, x_per_y=1, ensemble=False, out=None):
    """acg_fss_scales: the intensity-scale triples (Casati et al. 2004) of the events of ops.fss -> (rows, C, T, nl, 3) int64
    on the device, nl = fss_scale_levels(H, W): per threshold and level l = 0 .. nl - 1 the sums of bf^2, bo^2 and bf bo over
    the blocks of 2^l x 2^l cells anchored at cell (0, 0) (edge blocks cut by the domain), bf / bo the events [x >= t] /
    [y >= t] in a block.  Level 0 is ops.fss's window-1 triple, bit for bit.  Operands, thresholds, x_per_y, ensemble (ens:
    bf is the block's events of all members of a truth) and `out` as in ops.fss.  Exact integers, the same bits in every
    layout.  Sum the triples over a set of pairs, then ops.fss_scale_summary.  Nothing is read back to the host.  Not
    differentiable."""
    x, y, rows, rows_y, C, _, (H, W), sx, sy, x_per_y = _paired_fields("fss_scales", x, y, C, layout_x, layout_y, _fss_size, x_per_y,
                                                                       max_per=FSS_MAX_M, size_y=True)
    thr = channel_table("fss_scales", _lib.AcgError, "thresholds", thresholds, C, FSS_MAX_T, None)
    T, nl = int(thr.size(1)), fss_scale_levels(H, W)
    o, e = (out if ensemble else (out, None)) if out is not None else (None, None)
    shapes = ((rows, C, T, nl, 3), (rows_y, C, T, nl, 3))
    _refuse_out("fss_scales", o, shapes[0], torch.int64)
    _refuse_out("fss_scales", e, shapes[1], torch.int64, "ens")
    if not torch.is_tensor(thresholds):
        thr = thr.to(x.device)
    _check(x, y, thr)
    o = _out_or_new(o, shapes[0], torch.int64, x.device)
    if ensemble:
        e = _out_or_new(e, shapes[1], torch.int64, x.device)
    ws, nbytes = _metric_workspace("acg_fss_scales_workspace_bytes", rows, x_per_y, C, H, W, T, int(ensemble))
    _lib.call("acg_fss_scales", _ptr(x), _ptr(y), rows, x_per_y, C, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], _ptr(thr), T,
              _ptr(o), _ptr(e), ws, nbytes, _stream())
    return (o, e) if ensemble else o


def fss_scale_summary(sums, cells, members=1, forecast_events=None):
    """(..., T, nl, 3) int64 triples of ops.fss_scales, (sum bf^2, sum bo^2, sum bf bo) per level, summed over a set of pairs
    of `cells` cells in all (H W per pair) -> dict of arrays on the host, float64 unless said.  L = nl - 1; D_l = ff_l / M^2 +
    oo_l - 2 fo_l / M is the sum over the blocks of level l of the squared block sums of the error field b_x / M - b_y.
      mse (..., T, nl)      j < L: the energy of the Haar component "mean over 2^j blocks minus mean over 2^(j+1) blocks" of
                            the error field on the canvas zero-padded to 2^L x 2^L, (4 D_j - D_{j+1}) / 4^(j+1) / cells (for
                            M = 1 the numerator is formed in int64: exact, never negative); j = L: the mean term
                            D_L / 4^L / cells.  They sum to the plain MSE of the event (or probability) field.
      mse_random (..., T)   the MSE of a forecast with the same events placed at random: ff_0 / (M^2 cells) - 2 e_f e_o + e_o,
                            e_f = n_f / (M cells), e_o = n_o / cells (M = 1: Casati 2010's B e (1 - e) + e (1 - B e)).
      iss (..., T, nl)      1 - mse_j (L + 1) / mse_random: the random error split into L + 1 equal shares; NaN where
                            mse_random is 0.
      en_rel (..., T, nl)   (en_f - en_o) / (en_f + en_o), the component formula applied to ff / M^2 and to oo alone; NaN
                            where the denominator is 0.
      skill_scale (..., T)  int64: the smallest 2^j with iss > 0 at every mother scale j' >= j (j' < L); 2^L if there is none.
    members = M > 1: the triples are an ensemble's (sum E^2, sum bo^2, sum E bo).  Their level 0 no longer holds the forecast
    events n_f = sum E, so forecast_events (..., T) has to give them, summed over the same pairs (the level-0 sum bf^2 of the
    members' own triples); with M = 1 it defaults to ff_0.  ValueError: a last axis that is not 3, cells < 1, members < 1, or
    members > 1 without forecast_events."""
    import numpy as np
    t = np.asarray(sums)
    if t.ndim < 3 or t.shape[-1] != 3:
        raise ValueError("fss_scale_summary: need (..., T, nl, 3) triples (got %s)" % (t.shape,))
    if int(cells) < 1:
        raise ValueError("fss_scale_summary: cells must be at least 1 (got %s)" % (cells,))
    M = int(members)
    if M < 1:
        raise ValueError("fss_scale_summary: members must be at least 1 (got %s)" % (members,))
    if M > 1 and forecast_events is None:
        raise ValueError("fss_scale_summary: members > 1 needs forecast_events, the members' events summed over the same pairs")
    L, cells = t.shape[-2] - 1, float(int(cells))
    quarter = 0.25 ** np.arange(1, L + 2)                          # 4^-(j+1); the mean term takes 4^-L

    def components(s):                                             # s_l (..., nl), summed squared block sums -> energies
        num = np.concatenate([4 * s[..., :-1] - s[..., 1:], 4 * s[..., -1:]], -1)
        return num.astype(np.float64) * quarter / cells

    exact = M == 1 and t.dtype.kind in "iu"
    t = t.astype(np.int64 if exact else np.float64)
    ff, oo, fo = t[..., 0], t[..., 1], t[..., 2]
    res = dict(mse=components(ff + oo - 2 * fo if exact else ff / (M * M) + oo - 2.0 * fo / M))
    n_f = ff[..., 0] if forecast_events is None else np.asarray(forecast_events)
    e_f, e_o = n_f.astype(np.float64) / (M * cells), oo[..., 0].astype(np.float64) / cells
    res["mse_random"] = ff[..., 0].astype(np.float64) / (M * M * cells) - 2.0 * e_f * e_o + e_o
    en_f, en_o = components(ff.astype(np.float64) / (M * M)), components(oo)
    with np.errstate(divide="ignore", invalid="ignore"):
        res["iss"] = np.where(res["mse_random"][..., None] != 0, 1.0 - res["mse"] * (L + 1) / res["mse_random"][..., None], np.nan)
        res["en_rel"] = np.where(en_f + en_o != 0, (en_f - en_o) / (en_f + en_o), np.nan)
    ok = np.logical_and.accumulate((res["iss"][..., :L] > 0)[..., ::-1], -1)      # NaN compares false; from the largest scale down
    res["skill_scale"] = np.left_shift(np.int64(1), L - ok.sum(-1).astype(np.int64))
    return res


# ----------------------------------------------------------------------------------------------
# reliability tables of the fss events (--metric fss --fss_rel 1; include/acgan_verif.h; tests/reliability_ref.py)
# ----------------------------------------------------------------------------------------------
REL_MAX_WINDOW = 65


def check_rel_windows(windows):
    """check_windows with the reliability kernel's cap -> the widths as a tuple of ints; ValueError unless 1..8 odd widths in
    1..65 (a dilated 64-bit word then depends on itself and its two neighbours only)"""
    w = check_windows(windows)
    if any(v > REL_MAX_WINDOW for v in w):
        raise ValueError("windows must be at most %d wide (got %s)" % (REL_MAX_WINDOW, w))
    return w


def reliability(x, y, C, layout_x, layout_y, thresholds, windows, x_per_y=1, out=None):
    """acg_reliability: the reliability tables of the C valid channels of x against y -> (rows / x_per_y, C, T, nw, M + 1, 2)
    int64 on the device, M = x_per_y.  The events are fss's, [x >= thresholds[c][t]] (NaN is no event); the neighbourhood event
    of a cell at the odd window n <= 65 holds iff any cell of the centred n x n window inside the domain is an event (the
    neighbourhood maximum ensemble probability of Schwartz & Sobash 2017; n = 1 is the cell itself).  table[k][o] is the number
    of the H x W cells where k of the M members of a truth have the neighbourhood event and the truth has it (o = 1) or not
    (o = 0): every (M + 1, 2) block sums to H W, and with M = 1 it is the 2 x 2 contingency table.  Exact integers, the same
    bits in every layout.  Row r of x pairs with row r / x_per_y of y.  thresholds: (C, T) float32 on the device, or a host
    array (copied to the device).  `out`: the int64 tensor to write.  Sum the tables over a set of pairs, then
    ops.reliability_summary.  Nothing is read back to the host.  Not differentiable."""
    x, y, rows, rows_y, C, _, (H, W), sx, sy, x_per_y = _paired_fields("reliability", x, y, C, layout_x, layout_y, _fss_size,
                                                                       x_per_y, max_per=FSS_MAX_M, size_y=True)
    try:
        win = check_rel_windows(windows)
    except ValueError as e:
        raise _lib.AcgError("reliability: %s" % e)
    thr = channel_table("reliability", _lib.AcgError, "thresholds", thresholds, C, FSS_MAX_T, None)
    T, nw = int(thr.size(1)), len(win)
    shape = (rows_y, C, T, nw, x_per_y + 1, 2)
    _refuse_out("reliability", out, shape, torch.int64)
    if not torch.is_tensor(thresholds):                            # a host array goes to the device; a tensor is where it has to be
        thr = thr.to(x.device)
    _check(x, y, thr)                                              # after the refusals that need no device
    out = _out_or_new(out, shape, torch.int64, x.device)
    ws, nbytes = _metric_workspace("acg_reliability_workspace_bytes", rows, x_per_y, C, H, W, T, nw)
    _lib.call("acg_reliability", _ptr(x), _ptr(y), rows, x_per_y, C, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], _ptr(thr), T,
              (ctypes.c_int * nw)(*win), nw, _ptr(out), ws, nbytes, _stream())
    return out


def reliability_summary(table):
    """(..., M + 1, 2) int64 tables of ops.reliability summed over a set of pairs -> dict of float64 arrays on the host (n:
    int64).  The forecast probability takes the M + 1 values k / M, so nothing is binned (Murphy 1973):
      n (..., M + 1)        cells with k members in the event; prob (M + 1,) = k / M
      obs_freq (..., M + 1) the observed frequency among them (the reliability diagram), NaN where n_k = 0
      base_rate (...)       observed events / cells
      brier (...)           mean of (k / M - o)^2
      reliability, resolution, uncertainty (...)  sum_k n_k (k / M - obs_freq_k)^2 / cells, sum_k n_k (obs_freq_k - base_rate)^2
                            / cells, base_rate (1 - base_rate): brier = reliability - resolution + uncertainty exactly
      bss (...)             1 - brier / uncertainty, NaN where the uncertainty is 0
      brier_fair (...)      brier - sum_k n_k k (M - k) / (M^2 (M - 1)) / cells, the score an infinite ensemble of the same
                            distribution would get (Ferro 2014); NaN for M = 1
      roc_hit, roc_false (..., M + 2)  hit rate and false-alarm rate of "at least j members", j = M + 1 (none) .. 0 (all); NaN
                            where the class (events, non-events) is empty
      auc (...)             the area under that curve by the trapezoid rule: the Mann-Whitney statistic with ties counted
                            half; NaN where a class is empty."""
    import numpy as np
    t = np.asarray(table)
    if t.ndim < 2 or t.shape[-1] != 2 or t.shape[-2] < 2:
        raise ValueError("reliability_summary: need (..., M + 1, 2) tables with M >= 1 (got %s)" % (t.shape,))
    M = t.shape[-2] - 1
    t = t.astype(np.int64)
    n = t[..., 0] + t[..., 1]
    k = np.arange(M + 1, dtype=np.float64)
    prob = k / M
    t0, t1, nf = t[..., 0].astype(np.float64), t[..., 1].astype(np.float64), n.astype(np.float64)
    cells, events = nf.sum(-1), t1.sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        obs = np.where(n > 0, t1 / nf, np.nan)
        base = events / cells
        brier = (t1 * (prob - 1.0) ** 2 + t0 * prob ** 2).sum(-1) / cells
        rel = np.where(n > 0, nf * (prob - obs) ** 2, 0.0).sum(-1) / cells
        res = np.where(n > 0, nf * (obs - base[..., None]) ** 2, 0.0).sum(-1) / cells
        unc = base * (1.0 - base)
        bss = np.where(unc > 0, 1.0 - brier / unc, np.nan)
        fair = brier - (nf * k * (M - k)).sum(-1) / (float(M) * M * (M - 1)) / cells if M > 1 else np.full(brier.shape, np.nan)
        zero = np.zeros(t.shape[:-2] + (1,))
        hit = np.concatenate([zero, np.cumsum(t1[..., ::-1], -1)], -1) / events[..., None]
        false = np.concatenate([zero, np.cumsum(t0[..., ::-1], -1)], -1) / (cells - events)[..., None]
        hit = np.where((events > 0)[..., None], hit, np.nan)
        false = np.where((cells - events > 0)[..., None], false, np.nan)
        auc = (0.5 * (hit[..., 1:] + hit[..., :-1]) * (false[..., 1:] - false[..., :-1])).sum(-1)
    return dict(n=n, prob=prob, obs_freq=obs, base_rate=base, brier=brier, reliability=rel, resolution=res, uncertainty=unc,
                bss=bss, brier_fair=fair, roc_hit=hit, roc_false=false, auc=auc)


# ----------------------------------------------------------------------------------------------
# per-cell climatology maps of ensembles (--metric ensemble --ens_maps 1; include/acgan_cell.h; tests/cell_stats_ref.py)
# ----------------------------------------------------------------------------------------------
CELL_MAX_HW, CELL_MAX_T, CELL_MAX_E, CELL_MAX_M = 1024, 8, 63, 64
CELL_MOMENTS = ("Sx", "Sxx", "Sy", "Syy", "Sxy", "Sad", "SS", "SSy", "Sw")        # the planes of mom, in order
_CELL_PARTS = (("mom", torch.float64), ("evt", torch.int64), ("hist_x", torch.int32), ("hist_y", torch.int32))


def _cell_size(H, W):
    if not (1 <= H <= CELL_MAX_HW and 1 <= W <= CELL_MAX_HW):
        raise _lib.AcgError("cell_stats: fields must be H x W with 1 <= H, W <= %d (got %d x %d)" % (CELL_MAX_HW, H, W))
    return H, W


def _cell_shapes(C, H, W, T, E):
    return dict(mom=(9, C, H, W), evt=(C, T, 4, H, W) if T else None, hist_x=(C, E + 1, H, W) if E else None,
                hist_y=(C, E + 1, H, W) if E else None)


def cell_state_bytes(C, H, W, T, E):
    """the bytes of a cell_state on the device"""
    return C * H * W * (9 * 8 + 4 * 8 * T + (2 * 4 * (E + 1) if E else 0))


def cell_state(C, H, W, T, E, device):
    """The zeroed state ops.cell_stats adds to: dict mom (9, C, H, W) float64 (the planes CELL_MOMENTS), evt (C, T, 4, H, W)
    int64 (None for T = 0), hist_x, hist_y (C, E + 1, H, W) int32 (None for E = 0), n (the truth rows so far) and M (the
    members per truth, 0 until the first call fixes it), Python ints.  ValueError outside C >= 1, 1 <= H, W <= 1024,
    0 <= T <= 8, 0 <= E <= 63."""
    C, H, W, T, E = (int(v) for v in (C, H, W, T, E))
    if C < 1 or not (1 <= H <= CELL_MAX_HW and 1 <= W <= CELL_MAX_HW) or not 0 <= T <= CELL_MAX_T or not 0 <= E <= CELL_MAX_E:
        raise ValueError("cell_state: need C >= 1, 1 <= H, W <= %d, 0 <= T <= %d, 0 <= E <= %d (got C=%d, %d x %d, T=%d, E=%d)"
                         % (CELL_MAX_HW, CELL_MAX_T, CELL_MAX_E, C, H, W, T, E))
    shapes = _cell_shapes(C, H, W, T, E)
    state = {k: None if shapes[k] is None else torch.zeros(shapes[k], dtype=dt, device=device) for k, dt in _CELL_PARTS}
    state.update(n=0, M=0)
    return state


def cell_stats(x, y, C, layout_x, layout_y, state, thresholds=None, edges=None, x_per_y=1):
    """acg_cell_stats: one launch sequence that ADDS the rows of x (rows = Ny M fields, member m of truth n at row n M + m,
    M = x_per_y) against y (Ny truths) to a state of ops.cell_state, per cell (c, i, j) of the fixed grid, and adds Ny to
    state['n'] -> the state.  mom: the double sums Sx, Sxx, Sy, Syy, Sxy, Sad (|x - y|), SS (S^2, S the members' sum of a truth),
    SSy (S y), Sw (M Q - S^2, Q the members' sum of squares), every float converted to double and every operation rounded
    once, truths in row order and members in order inside: the same bits in every layout and whatever the split of the rows
    into calls.  evt[c][t] += (k, o, k o, k k), k the members with x >= thresholds[c][t] and o = [y >= thresholds[c][t]], in
    float32, NaN no event.  hist_x / hist_y[c][b] += 1 with b = #{e : edges[c][e] <= v}, NaN in bin 0; an int32 count holds
    2^31 - 1 rows.  thresholds (C, T), edges (C, E, ascending): float32 on the device (a tensor's order is the caller's
    contract) or host arrays (checked, copied to the device); None where the state has no such part.  Refused on the host, by
    name (AcgError "cell_stats: ..."): a state of another shape, dtype or M, thresholds or edges that disagree with it,
    operands that do not pair.  Subnormal float32 inputs are outside the equality claim.  Nothing is read back to the host.
    Not differentiable."""
    what = "cell_stats"
    x, y, rows, rows_y, C, _, (H, W), sx, sy, x_per_y = _paired_fields(what, x, y, C, layout_x, layout_y, _cell_size, x_per_y,
                                                                       max_per=CELL_MAX_M, size_y=True)
    if not isinstance(state, dict) or any(k not in state for k in ("mom", "evt", "hist_x", "hist_y", "n", "M")):
        raise _lib.AcgError("%s: state must be a dict of ops.cell_state (mom, evt, hist_x, hist_y, n, M)" % what)
    thr = channel_table(what, _lib.AcgError, "thresholds", [[]] * C if thresholds is None else thresholds, C, CELL_MAX_T, None,
                        none_if_empty=True)
    edg = channel_table(what, _lib.AcgError, "edges", [[]] * C if edges is None else edges, C, CELL_MAX_E, None,
                        none_if_empty=True, ordered=True)
    T, E = 0 if thr is None else int(thr.size(1)), 0 if edg is None else int(edg.size(1))
    shapes = _cell_shapes(C, H, W, T, E)
    for k, dt in _CELL_PARTS:
        t = state[k]
        if (t is None) != (shapes[k] is None):
            raise _lib.AcgError("%s: state[%r] is %s but the call has T=%d thresholds and E=%d edges"
                                % (what, k, "absent" if t is None else "present", T, E))
        if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != shapes[k] or t.dtype != dt or not t.is_contiguous()):
            raise _lib.AcgError("%s: state[%r] %s %s is not a contiguous %s %s"
                                % (what, k, tuple(getattr(t, "shape", ())), getattr(t, "dtype", type(t)),
                                   str(dt).replace("torch.", ""), shapes[k]))
    if state["M"] not in (0, x_per_y):
        raise _lib.AcgError("%s: the state holds ensembles of M=%d members, the call has x_per_y=%d" % (what, state["M"], x_per_y))
    if not torch.is_tensor(thresholds) and thr is not None:       # a host array goes to the device; a tensor is where it has to be
        thr = thr.to(x.device)
    if not torch.is_tensor(edges) and edg is not None:
        edg = edg.to(x.device)
    _check(x, y, thr, edg)                                         # after the refusals that need no device
    for k, _ in _CELL_PARTS:
        if state[k] is not None and not state[k].is_cuda:
            raise _lib.AcgError(_NO_CPU_PATH % state[k].device)
    _lib.call("acg_cell_stats", _ptr(x), _ptr(y), rows, x_per_y, C, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], _ptr(thr), T,
              _ptr(edg), E, _ptr(state["mom"]), _ptr(state["evt"]), _ptr(state["hist_x"]), _ptr(state["hist_y"]), _stream())
    state["n"] += rows_y
    state["M"] = x_per_y
    return state


def cell_summary(state, thresholds=None, edges=None, levels=()):
    """A state of ops.cell_stats whose tensors are host arrays (read back by the caller) -> dict of float64 maps on the host,
    (C, H, W) unless said otherwise.  With n truth rows, M members each and N = n M member rows:
      mean_x = Sx / N, mean_y = Sy / n, bias = mean_x - mean_y
      std_x, std_y     sqrt of the population variances Sxx / N - mean_x^2, Syy / n - mean_y^2, clamped at 0
      std_ratio        std_x / std_y; NaN where the variance of y is 0
      corr             (Sxy / N - mean_x mean_y) / (std_x std_y), members against the truth in time; NaN where a variance is 0
      rmse             sqrt(max(Sxx + M Syy - 2 Sxy, 0) / N); mae = Sad / N
      rmse_mean        the ensemble mean against the truth: sqrt(max((SS / M^2 - 2 SSy / M + Syy) / n, 0))
      corr_mean        (SSy / (M n) - mean_x mean_y) / sqrt(var_mean var_y), var_mean = SS / (M^2 n) - mean_x^2 clamped at 0;
                       NaN where a variance is 0
      spread           sqrt(max(Sw, 0) / (M (M - 1) n)), the root of the mean unbiased ensemble variance; NaN for M = 1
      spread_skill     sqrt((M + 1) / M) spread / rmse_mean; NaN for M = 1 and where rmse_mean is 0
    With events (thresholds (C, T), needed only for its shape), each (C, T, H, W):
      freq_x = sum k / N, freq_y = sum o / n, freq_bias = freq_x / freq_y (NaN where freq_y is 0),
      brier = (sum k^2 - 2 M sum k o + M^2 sum o) / (M^2 n), the mean of (k / M - o)^2,
      hit_rate = sum k o / (M sum o) (NaN where the truth never has the event),
      csi = sum k o / (sum k + M sum o - sum k o) (NaN where neither ever has it)
    With histograms (edges (C, E) required):
      cdf_x, cdf_y (C, E, H, W)  the fraction of values below edge e (the bins 0 .. e; a NaN value lies in bin 0)
      ks                         the largest |cdf_x - cdf_y| over the edges
      q_x, q_y (C, L, H, W)      per level of `levels` the first edge whose CDF reaches it, NaN if none does
    A state with n = 0 gives NaN everywhere (0 / 0).  A NaN in the sums of a cell stays a NaN in its maps.  No map is inf
    where a denominator is 0: it is NaN."""
    import numpy as np
    mom = np.asarray(state["mom"], dtype=np.float64)
    n, M = int(state["n"]), int(state["M"])
    if mom.ndim != 4 or mom.shape[0] != 9:
        raise ValueError("cell_summary: mom must be (9, C, H, W) (got %s)" % (mom.shape,))
    C = mom.shape[1]
    Sx, Sxx, Sy, Syy, Sxy, Sad, SS, SSy, Sw = mom
    N = n * M
    res = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        nf, Nf, Mf = np.float64(n), np.float64(N), np.float64(M)
        mean_x, mean_y = Sx / Nf, Sy / nf
        var_x = np.maximum(Sxx / Nf - mean_x * mean_x, 0.0)     # np.maximum keeps a NaN
        var_y = np.maximum(Syy / nf - mean_y * mean_y, 0.0)
        std_x, std_y = np.sqrt(var_x), np.sqrt(var_y)
        res.update(mean_x=mean_x, mean_y=mean_y, bias=mean_x - mean_y, std_x=std_x, std_y=std_y,
                   std_ratio=np.where(var_y == 0, np.nan, std_x / std_y),
                   corr=np.where((var_x == 0) | (var_y == 0), np.nan, (Sxy / Nf - mean_x * mean_y) / (std_x * std_y)),
                   rmse=np.sqrt(np.maximum(Sxx + Mf * Syy - 2.0 * Sxy, 0.0) / Nf), mae=Sad / Nf)
        rmse_mean = np.sqrt(np.maximum((SS / (Mf * Mf) - 2.0 * SSy / Mf + Syy) / nf, 0.0))
        var_mean = np.maximum(SS / (Mf * Mf * nf) - mean_x * mean_x, 0.0)
        corr_mean = np.where((var_mean == 0) | (var_y == 0), np.nan,
                             (SSy / (Mf * nf) - mean_x * mean_y) / np.sqrt(var_mean * var_y))
        spread = np.sqrt(np.maximum(Sw, 0.0) / (Mf * (Mf - 1.0) * nf)) if M > 1 else np.full(Sw.shape, np.nan)
        skill = np.where(rmse_mean == 0, np.nan, np.sqrt((Mf + 1.0) / Mf) * spread / rmse_mean) if M >= 1 else spread
        res.update(rmse_mean=rmse_mean, corr_mean=corr_mean, spread=spread, spread_skill=skill)
        if state.get("evt") is not None:
            evt = np.asarray(state["evt"]).astype(np.float64)
            if evt.ndim != 5 or evt.shape[0] != C or evt.shape[2] != 4 or evt.shape[3:] != mom.shape[2:]:
                raise ValueError("cell_summary: evt must be (C, T, 4, H, W) (got %s)" % (evt.shape,))
            if thresholds is not None and np.shape(thresholds) != (C, evt.shape[1]):
                raise ValueError("cell_summary: thresholds %s do not match evt %s" % (np.shape(thresholds), evt.shape))
            k, o, ko, kk = evt[:, :, 0], evt[:, :, 1], evt[:, :, 2], evt[:, :, 3]
            freq_x, freq_y = k / Nf, o / nf
            union = k + Mf * o - ko
            res.update(freq_x=freq_x, freq_y=freq_y, freq_bias=np.where(freq_y == 0, np.nan, freq_x / freq_y),
                       brier=(kk - 2.0 * Mf * ko + Mf * Mf * o) / (Mf * Mf * nf),
                       hit_rate=np.where(o == 0, np.nan, ko / (Mf * o)), csi=np.where(union == 0, np.nan, ko / union))
        if state.get("hist_x") is not None:
            hx, hy = np.asarray(state["hist_x"]).astype(np.float64), np.asarray(state["hist_y"]).astype(np.float64)
            if edges is None or hx.shape != hy.shape or hx.ndim != 4 or np.shape(edges) != (C, hx.shape[1] - 1):
                raise ValueError("cell_summary: histograms %s, %s need edges (C, E) with E + 1 bins (got %s)"
                                 % (hx.shape, hy.shape, None if edges is None else np.shape(edges)))
            ed = np.asarray(edges, dtype=np.float64)
            lv = np.asarray(levels, dtype=np.float64).reshape(-1)
            cdf_x = np.cumsum(hx, axis=1)[:, :-1] / hx.sum(axis=1, keepdims=True)
            cdf_y = np.cumsum(hy, axis=1)[:, :-1] / hy.sum(axis=1, keepdims=True)
            res.update(cdf_x=cdf_x, cdf_y=cdf_y, ks=np.abs(cdf_x - cdf_y).max(axis=1))
            for name, cdf in (("q_x", cdf_x), ("q_y", cdf_y)):
                reach = cdf[:, None] >= lv[None, :, None, None, None]                # (C, L, E, H, W)
                first = reach.argmax(axis=2)
                q = np.take_along_axis(np.broadcast_to(ed[:, None, :, None, None], reach.shape), first[:, :, None], axis=2)[:, :, 0]
                res[name] = np.where(reach.any(axis=2), q, np.nan)
    return res


# ----------------------------------------------------------------------------------------------
# the fractions-skill-score training loss (the paired step under --lambda_fss_A / --lambda_fss_B; tests/fss_loss_ref.py)
# ----------------------------------------------------------------------------------------------
FSS_LOSS_MAX_WINDOW = 65


def check_fss_loss_windows(windows):
    """check_windows with the loss's cap -> the widths as a tuple of ints; ValueError unless 1..8 odd widths in 1..65"""
    w = check_windows(windows)
    if max(w) > FSS_LOSS_MAX_WINDOW:
        raise ValueError("windows of the loss must not exceed %d (got %s)" % (FSS_LOSS_MAX_WINDOW, w))
    return w


def fss_loss_inv_tau(tau):
    """1 / tau as the float the kernels take (formed in double, rounded once); ValueError unless both are positive and finite"""
    import numpy as np
    t = float(tau)
    with np.errstate(over="ignore", under="ignore"):
        inv = float(np.float32(1.0 / t)) if 0.0 < t < float("inf") else 0.0
    if not 0.0 < inv < float("inf"):
        raise ValueError("tau must be positive and finite, and so must 1 / tau in float32 (got %r)" % (tau,))
    return inv


def _fss_loss_size(H, W):
    if not (1 <= H <= FSS_MAX_HW and 1 <= W <= FSS_MAX_HW):
        raise _lib.AcgError("fss_loss: fields must be H x W with 1 <= H, W <= %d (got %d x %d)" % (FSS_MAX_HW, H, W))
    return int(H), int(W)


class FssLoss(torch.autograd.Function):
    """fss_loss with its data gradient in x: forward acg_fss_loss_fwd (num and den per row, channel, threshold and window, in
    double) and the pooled combine on the device; backward acg_fss_loss_bwd, which recomputes the soft events from x and y
    (nothing but the two operands, the thresholds and the small pooled tensors is kept, and those only when x needs a
    gradient) and takes the coefficients a, b, scaled by the upstream gradient, from the device."""

    @staticmethod
    def forward(ctx, x, y, C, layout, thresholds, windows, tau):
        x, y, rows, _, C, Cp, (H, W), sx, sy, _ = _paired_fields("fss_loss", x, y, C, layout, layout, _fss_loss_size, 1, max_per=1,
                                                                 size_y=True)
        try:
            win = check_fss_loss_windows(windows)
            inv_tau = fss_loss_inv_tau(tau)
        except ValueError as e:
            raise _lib.AcgError("fss_loss: %s" % e)
        thr = channel_table("fss_loss", _lib.AcgError, "thresholds", thresholds, C, FSS_MAX_T, None)
        T, nw = int(thr.size(1)), len(win)
        if not torch.is_tensor(thresholds):                        # a host array goes to the device; a tensor is where it has to be
            thr = thr.to(x.device)
        out = _out_tensor("fss_loss", None, (rows, C, T, nw, 2), (x, y, thr), dtype=torch.float64)
        cwin = (ctypes.c_int * nw)(*win)
        ws, nbytes = _metric_workspace("acg_fss_loss_workspace_bytes", rows, C, H, W, T, nw)
        _lib.call("acg_fss_loss_fwd", _ptr(x), _ptr(y), rows, C, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], _ptr(thr), T, cwin, nw,
                  ctypes.c_float(inv_tau), _ptr(out), ws, nbytes, _stream())
        tot = out.sum(0)                                           # pooled over the batch before dividing, as fss_summary pools a split
        num, den = tot[..., 0], tot[..., 1]
        some = den != 0                                            # a NaN denominator stays: a diverged run shows
        R = torch.where(some, num / torch.where(some, den, torch.ones_like(den)), torch.zeros_like(den))
        loss = R.mean().float()
        ctx.mark_non_differentiable(R)
        if ctx.needs_input_grad[0]:
            ctx.cfg = (rows, C, Cp, H, W, sx, sy, T, win, inv_tau)
            ctx.save_for_backward(x, y, thr, R, den)
        return loss, R

    @staticmethod
    def backward(ctx, g, _R):
        x, y, thr, R, den = ctx.saved_tensors
        rows, C, Cp, H, W, sx, sy, T, win, inv_tau = ctx.cfg
        nw = len(win)
        some = den != 0
        inv = torch.where(some, 1.0 / torch.where(some, den, torch.ones_like(den)), torch.zeros_like(den))
        inv = inv * (g.detach().to(torch.float64) / (C * T * nw))
        coef = torch.stack((2.0 * (1.0 - R) * inv, 2.0 * inv), -1).contiguous()
        dx = torch.empty_like(x)
        ws, nbytes = _metric_workspace("acg_fss_loss_workspace_bytes", rows, C, H, W, T, nw)
        _lib.call("acg_fss_loss_bwd", _ptr(x), _ptr(y), rows, C, Cp, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], _ptr(thr), T,
                  (ctypes.c_int * nw)(*win), nw, ctypes.c_float(inv_tau), _ptr(coef), _ptr(dx), ws, nbytes, _stream())
        return dx, None, None, None, None, None, None


def fss_loss(x, y, C, layout, thresholds, windows, tau, parts=False):
    """1 - the pooled fractions skill score of soft events, averaged over the C valid channels, the T thresholds and the nw
    windows -> float32 device scalar, differentiable in x (y is detached).  x and y share the layout ("nhwc" or "nchw") and
    pair row by row.  p = 1 / (1 + exp(-(x - thresholds[c][t]) / tau)) in fp32 (q of y), cf / co their sums over the centred
    n x n window of each cell inside the domain (fp32; cells outside count 0), Num = sum over rows and cells of (cf - co)^2,
    Den = of cf^2 + co^2 (double), R = Num / Den = 1 - FSS, 0 where Den == 0 exactly; loss = mean R.  Pooling the batch before
    dividing, as ops.fss_summary pools a split, keeps a rare threshold usable.  NaN is not masked.  With every value at
    least 200 tau from every threshold the events are exactly 0 or 1 and Num, Den equal ff + oo - 2 fo, ff + oo of ops.fss.
    d loss / d x(q) = g / (C T nw) sum_t p_t (1 - p_t) / tau sum_w B_n(a cf - b co)(q), a = 2 (1 - R) / Den, b = 2 / Den (0
    where Den == 0), B_n the window sum over the domain's cells; NHWC: the padded channels of the gradient are 0.
    thresholds: (C, T) float32 on the device, or a host array (copied to the device), 1 <= T <= 8; windows: 1..8 odd widths of
    at most 65; tau > 0; 1 <= H, W <= 1024.  parts=True: (loss, R) with the detached R (C, T, nw) in double.  Sums in a fixed
    order, the same bits in every layout; no host synchronisation.  Under torch.no_grad(), or for an x that needs no
    gradient, nothing is saved."""
    loss, R = FssLoss.apply(x if torch.is_grad_enabled() else x.detach(), y, C, layout, thresholds, windows, tau)
    return (loss, R) if parts else loss


# ----------------------------------------------------------------------------------------------
# Minkowski functionals of excursion sets (model.translate_minkowski, eval_metrics.py, --metric minkowski)
# ----------------------------------------------------------------------------------------------
MINK_MAX_T, MINK_MAX_HW = 255, 1024
MINK_FUNCTIONALS = ("area", "perimeter", "euler4", "euler8")


def check_thresholds(thresholds, C):
    """host thresholds as minkowski takes them -> a contiguous (C, T) float32 array; ValueError unless 1 <= T <= 255 and every
    channel's thresholds are finite and non-decreasing (repeats allowed)"""
    return channel_table("check_thresholds", ValueError, "thresholds", thresholds, C, MINK_MAX_T, None, ordered=True).numpy()


def minkowski(x, C, layout, thresholds, out=None):
    """acg_minkowski: the counts behind the Minkowski functionals of the excursion sets {x >= thresholds[c][t]} of the C valid
    channels of x -> (rows, C, T, 5) int64 on the device: (nF, nE1, nE2, nV1, nV4), the pixels in the set, the unit edges
    with a pixel / both pixels in it and the vertices with a pixel / all four pixels in it, the field standing in a ring of
    cells outside every set (x == threshold is inside, NaN outside, as in fss).  Exact integers, the same bits in every layout;
    linear over fields: sum them over a set of fields, then ops.minkowski_summary.  layout "nhwc": x (rows, H, W, Cp) as
    forward_nhwc / ToNHWC give it (padded channels never reach a result); "nchw": x (rows, C, H, W).  1 <= H, W <= 1024.
    thresholds: (C, T), 1 <= T <= 255, per channel finite and non-decreasing (repeats allowed): a host array is checked
    (channel_table) and copied to the device; a float32 device tensor is taken as it is - its order is the caller's
    contract, nothing is read back to check it.  `out`: the contiguous int64 tensor to write.  One pass over x for all
    thresholds, two launches; nothing is read back to the host.  Not differentiable."""
    x = x.detach().contiguous()
    rows, C, _, H, W, sx = _field_args(x, C, layout, "minkowski")
    if not (1 <= H <= MINK_MAX_HW and 1 <= W <= MINK_MAX_HW):
        raise _lib.AcgError("minkowski: fields must be H x W with 1 <= H, W <= %d (got %d x %d)" % (MINK_MAX_HW, H, W))
    thr = channel_table("minkowski", _lib.AcgError, "thresholds", thresholds, C, MINK_MAX_T, None, ordered=True)
    T = int(thr.size(1))
    _refuse_out("minkowski", out, (rows, C, T, 5), torch.int64)
    if not torch.is_tensor(thresholds):                            # a host array goes to the device; a tensor is where it has to be
        thr = thr.to(x.device)
    out = _out_tensor("minkowski", out, (rows, C, T, 5), (x, thr), dtype=torch.int64)
    ws, nbytes = _metric_workspace("acg_minkowski_workspace_bytes", rows, C, H, W, T)
    _lib.call("acg_minkowski", _ptr(x), rows, C, H, W, sx[0], sx[1], sx[2], _ptr(thr), T, _ptr(out), ws, nbytes, _stream())
    return out


def minkowski_summary(counts, cells):
    """(..., T, 5) int64 counts (nF, nE1, nE2, nV1, nV4) summed over a set of fields of `cells` cells in all -> dict of
    float64 arrays (..., T) on the host:
      area       nF, the cells inside the set;
      perimeter  nE1 - nE2, the unit edges with exactly one side inside (the domain's border counts as outside);
      euler8     nV1 - nE1 + nF, the 8-connected components minus their holes (pixels as closed squares);
      euler4     nF - nE2 + nV4, the 4-connected components minus their holes;
    and each per cell under area_density, perimeter_density, euler4_density, euler8_density."""
    import numpy as np
    n = np.asarray(counts)
    if n.ndim < 2 or n.shape[-1] != 5 or int(cells) < 1:
        raise ValueError("minkowski_summary: need (..., T, 5) counts and a positive cell count (got %s, %s)" % (n.shape, cells))
    n = n.astype(np.int64)
    nF, nE1, nE2, nV1, nV4 = (n[..., k] for k in range(5))
    res = dict(area=nF, perimeter=nE1 - nE2, euler4=nF - nE2 + nV4, euler8=nV1 - nE1 + nF)
    res = {k: v.astype(np.float64) for k, v in res.items()}
    res.update([(k + "_density", v / float(int(cells))) for k, v in res.items()])
    return res


def minkowski_distance(a, b):
    """two minkowski_summary dicts of the same thresholds -> dict of float64 arrays (...): per functional (area, perimeter,
    euler4, euler8) the mean over the thresholds of |density_a - density_b|"""
    import numpy as np
    res = {}
    for k in MINK_FUNCTIONALS:
        da, db = np.asarray(a[k + "_density"], dtype=np.float64), np.asarray(b[k + "_density"], dtype=np.float64)
        if da.shape != db.shape or da.ndim < 1:
            raise ValueError("minkowski_distance: %s densities %s against %s" % (k, da.shape, db.shape))
        res[k] = np.abs(da - db).mean(-1)
    return res


# ----------------------------------------------------------------------------------------------
# Connected components of excursion sets (model.translate_minkowski(components=), --metric minkowski --mink_components)
# ----------------------------------------------------------------------------------------------
COMP_STATS, COMP_BINS = 25, 21


def components(x, C, layout, thresholds, conn=8, out=None, labels=None):
    """acg_components: the connected components of the excursion sets {x >= thresholds[c][t]} of the C valid channels of x,
    under conn = 4 or 8 connectivity -> (rows, C, T, COMP_STATS) int64 on the device: n (the components), area (the cells in
    the set, minkowski's nF), sum_sq (the sum of the components' squared areas), n_border (the components with a cell in the
    first or last row or column) and hist[b], b = 0 .. 20 (the components with 2^b <= area < 2^(b + 1)).  x == threshold is
    inside, NaN outside, as in minkowski.  Exact integers, the same bits in every layout and on every call; linear over
    fields: sum them over a set of fields, then ops.components_summary.  x, C, layout, thresholds: as ops.minkowski takes
    them (1 <= H, W <= 1024; a host table is checked and copied to the device, a float32 device tensor is taken as it is).
    `out`: the contiguous int64 tensor to write.  labels: True, or a contiguous int32 (rows, C, T, H, W) tensor to write: the
    canonical label planes are returned too, (out, labels): 0 outside the set, inside 1 + the row-major index of the first
    cell of the cell's component.  Launches only, in passes over the planes when the workspace (256 MiB at most) does not
    hold them all; nothing is read back to the host.  Not differentiable."""
    x = x.detach().contiguous()
    rows, C, _, H, W, sx = _field_args(x, C, layout, "components")
    if not (1 <= H <= MINK_MAX_HW and 1 <= W <= MINK_MAX_HW):
        raise _lib.AcgError("components: fields must be H x W with 1 <= H, W <= %d (got %d x %d)" % (MINK_MAX_HW, H, W))
    if conn not in (4, 8):
        raise _lib.AcgError("components: connectivity must be 4 or 8 (got %r)" % (conn,))
    thr = channel_table("components", _lib.AcgError, "thresholds", thresholds, C, MINK_MAX_T, None, ordered=True)
    T = int(thr.size(1))
    _refuse_out("components", out, (rows, C, T, COMP_STATS), torch.int64)
    want_labels = labels is not None and labels is not False
    lab = labels if torch.is_tensor(labels) else None
    if want_labels:
        if rows * C * T * H * W > 2 ** 31 - 1:
            raise _lib.AcgError("components: labels of %d planes of %d x %d pass 2^31 - 1 cells" % (rows * C * T, H, W))
        _refuse_out("components", lab, (rows, C, T, H, W), torch.int32, name="labels")
    if not torch.is_tensor(thresholds):                            # a host array goes to the device; a tensor is where it has to be
        thr = thr.to(x.device)
    _check(x, thr)
    out = _out_or_new(out, (rows, C, T, COMP_STATS), torch.int64, x.device)
    if want_labels:
        lab = _out_or_new(lab, (rows, C, T, H, W), torch.int32, x.device)
    ws, nbytes = _metric_workspace("acg_components_workspace_bytes", rows, C, H, W, T)
    _lib.call("acg_components", _ptr(x), rows, C, H, W, sx[0], sx[1], sx[2], _ptr(thr), T, int(conn), _ptr(out),
              _ptr(lab) if want_labels else None, ws, nbytes, _stream())
    return (out, lab) if want_labels else out


def components_summary(stats, counts, fields, cells, conn):
    """(..., T, COMP_STATS) int64 stats of ops.components and (..., T, 5) counts of ops.minkowski, both summed over the same
    `fields` fields of `cells` cells in all -> dict of float64 arrays (..., T) on the host:
      components, holes          n, and n minus minkowski_summary's euler8 (conn = 8) or euler4 (conn = 4);
      components_density, holes_density   the two per cell;
      mean_area                  area / n, NaN where there is no component;
      weighted_area              sum_sq / area, the area of the component an inside cell lies in on average; NaN for an empty set;
      border_fraction            n_border / n, NaN where there is no component;
    and size_pdf (..., T, COMP_BINS) = hist / n (NaN where there is no component)."""
    import numpy as np
    s, n5 = np.asarray(stats), np.asarray(counts)
    if (s.ndim < 2 or s.shape[-1] != COMP_STATS or n5.shape != s.shape[:-1] + (5,) or int(cells) < 1 or int(fields) < 1
            or conn not in (4, 8)):
        raise ValueError("components_summary: need (..., T, %d) stats, (..., T, 5) counts of the same fields, positive field and "
                         "cell counts and conn 4 or 8 (got %s, %s, %s, %s, %r)" % (COMP_STATS, s.shape, n5.shape, fields, cells, conn))
    s = s.astype(np.int64)
    euler = minkowski_summary(n5, cells)["euler%d" % conn]
    n, area = s[..., 0].astype(np.float64), s[..., 1].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        res = dict(components=n, holes=n - euler, mean_area=np.where(n > 0, area / n, np.nan),
                   weighted_area=np.where(area > 0, s[..., 2] / area, np.nan), border_fraction=np.where(n > 0, s[..., 3] / n, np.nan),
                   size_pdf=np.where(n[..., None] > 0, s[..., 4:] / n[..., None], np.nan))
    res["components_density"], res["holes_density"] = res["components"] / float(int(cells)), res["holes"] / float(int(cells))
    return res


def components_distance(a, b):
    """two components_summary dicts of the same thresholds -> dict of float64 arrays (...): dist_components and dist_holes,
    the mean over the thresholds of |density_a - density_b|; dist_size, the mean, over the thresholds where both sides have
    a component, of the total-variation distance 0.5 sum_b |pdf_a - pdf_b| of the size distributions (NaN if none has)"""
    import numpy as np
    res = {}
    for k in ("components", "holes"):
        da, db = np.asarray(a[k + "_density"], dtype=np.float64), np.asarray(b[k + "_density"], dtype=np.float64)
        if da.shape != db.shape or da.ndim < 1:
            raise ValueError("components_distance: %s densities %s against %s" % (k, da.shape, db.shape))
        res["dist_" + k] = np.abs(da - db).mean(-1)
    pa, pb = np.asarray(a["size_pdf"], dtype=np.float64), np.asarray(b["size_pdf"], dtype=np.float64)
    if pa.shape != pb.shape or pa.ndim < 2 or pa.shape[-1] != COMP_BINS:
        raise ValueError("components_distance: size_pdf %s against %s" % (pa.shape, pb.shape))
    tv = 0.5 * np.abs(pa - pb).sum(-1)                             # NaN where either side has no component
    ok = ~np.isnan(tv)
    cnt = ok.sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        res["dist_size"] = np.where(cnt > 0, np.where(ok, tv, 0.0).sum(-1) / cnt, np.nan)
    return res


# ----------------------------------------------------------------------------------------------
# SAL: structure, amplitude and location of the objects (model.translate_sal, eval_metrics.py, --metric fss --fss_sal 1)
# ----------------------------------------------------------------------------------------------
def sal(x, C, layout, thresholds, floor=-1.0, conn=8, out=None):
    """acg_sal: the weighted moments behind the SAL score (Wernli et al. 2008) of the C valid channels of x -> (field, obj,
    shape) on the device.  The mass of a cell is the integer q = clamp(rint((x - floor) 2^20), 0, 2^24) in fp32 (NaN: 0), the
    objects of a plane are the components of {x >= thresholds[c][t]} under conn = 4 or 8 connectivity, as ops.components
    labels them.  field (rows, C, 3) int64: Q, QY, QX, the sums of q, q h, q w over all cells; obj (rows, C, T, 4) int64: n,
    area, Robj (the mass in the set), Rmax (the largest mass of an object); shape (rows, C, T, 2) float64: SV, the sum over the
    objects of R (R / P) with R the mass and P the peak of an object, and SR, the sum of R times the distance of the object's
    centre of mass from the field's.  Exact integers, and doubles summed in a fixed order: the same bits in every layout and
    on every call.  ops.sal_scores turns two triples into scores.  x, C, layout, thresholds: as ops.components takes them
    (1 <= H, W <= 1024; a host table is checked and copied to the device, a float32 device tensor is taken as it is).  floor:
    finite, the lower end of the data range.  `out`: a triple of contiguous tensors to write.  Launches only, in passes over
    the planes when the workspace (256 MiB at most) does not hold them all; nothing is read back.  Not differentiable."""
    import math
    import numbers
    x = x.detach().contiguous()
    rows, C, _, H, W, sx = _field_args(x, C, layout, "sal")
    if not (1 <= H <= MINK_MAX_HW and 1 <= W <= MINK_MAX_HW):
        raise _lib.AcgError("sal: fields must be H x W with 1 <= H, W <= %d (got %d x %d)" % (MINK_MAX_HW, H, W))
    if conn not in (4, 8):
        raise _lib.AcgError("sal: connectivity must be 4 or 8 (got %r)" % (conn,))
    if isinstance(floor, bool) or not isinstance(floor, numbers.Real) or not math.isfinite(floor):
        raise _lib.AcgError("sal: the floor must be a finite number (got %r)" % (floor,))
    thr = channel_table("sal", _lib.AcgError, "thresholds", thresholds, C, MINK_MAX_T, None, ordered=True)
    T = int(thr.size(1))
    shapes = ((rows, C, 3), torch.int64, "field"), ((rows, C, T, 4), torch.int64, "obj"), ((rows, C, T, 2), torch.float64, "shape")
    if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 3):
        raise _lib.AcgError("sal: out must be the triple (field, obj, shape)")
    outs = list(out) if out is not None else [None] * 3
    for o, (shape, dtype, name) in zip(outs, shapes):
        if o is not None and not torch.is_tensor(o):
            raise _lib.AcgError("sal: out must be the triple (field, obj, shape) of tensors")
        _refuse_out("sal", o, shape, dtype, name=name)
    if not torch.is_tensor(thresholds):                            # a host array goes to the device; a tensor is where it has to be
        thr = thr.to(x.device)
    _check(x, thr)
    outs = [_out_or_new(o, shape, dtype, x.device) for o, (shape, dtype, _) in zip(outs, shapes)]
    ws, nbytes = _metric_workspace("acg_sal_workspace_bytes", rows, C, H, W, T)
    _lib.call("acg_sal", _ptr(x), rows, C, H, W, sx[0], sx[1], sx[2], _ptr(thr), T, int(conn), ctypes.c_float(floor), _ptr(outs[0]),
              _ptr(outs[1]), _ptr(outs[2]), ws, nbytes, _stream())
    return tuple(outs)


def sal_scores(f, o, H, W):
    """two triples (field, obj, shape) of ops.sal on the host, the forecast's and the observation's, of H x W fields and the
    same thresholds, that broadcast against each other (members (N, M, ...) against truth (N, 1, ...)) -> dict of float64
    arrays, with d = sqrt((H - 1)^2 + (W - 1)^2):
      A  (..., C)     (Q_f - Q_o) / (0.5 (Q_f + Q_o)), the amplitude; NaN when Q_f + Q_o = 0;
      L1 (..., C)     |c_f - c_o| / d with c = (QY / Q, QX / Q), the centres of mass; NaN when either Q is 0; 0 when d = 0;
      S  (..., C, T)  (V_f - V_o) / (0.5 (V_f + V_o)) with V = SV / Robj, the structure: > 0 for objects too large or too flat;
      L2 (..., C, T)  2 |r_f - r_o| / d with r = SR / Robj, the spread of the objects about the centre; 0 when d = 0;
      L  (..., C, T)  L1 + L2, the location.
    S, L2 and L are NaN when either side has Robj = 0.  S and A lie in [-2, 2], L in [0, 2]."""
    import numpy as np

    def triple(t, who):
        if not isinstance(t, (tuple, list)) or len(t) != 3:
            raise ValueError("sal_scores: %s must be the triple (field, obj, shape)" % who)
        fld, obj, shp = (np.asarray(a) for a in t)
        if (fld.ndim < 2 or fld.shape[-1] != 3 or obj.ndim != fld.ndim + 1 or obj.shape[-1] != 4 or obj.shape[:-2] != fld.shape[:-1]
                or shp.shape != obj.shape[:-1] + (2,)):
            raise ValueError("sal_scores: %s must be field (..., C, 3), obj (..., C, T, 4), shape (..., C, T, 2) (got %s, %s, %s)"
                             % (who, fld.shape, obj.shape, shp.shape))
        return fld.astype(np.float64), obj[..., 2].astype(np.float64), shp.astype(np.float64)

    if int(H) < 1 or int(W) < 1:
        raise ValueError("sal_scores: fields must be H x W with H, W >= 1 (got %s x %s)" % (H, W))
    (ff, rf, sf), (fo, ro, so) = triple(f, "f"), triple(o, "o")
    try:
        np.broadcast_shapes(ff.shape, fo.shape), np.broadcast_shapes(sf.shape, so.shape)
    except ValueError:
        raise ValueError("sal_scores: %s and %s fields with %s and %s planes do not broadcast" % (ff.shape, fo.shape, sf.shape, so.shape))
    d = float(np.sqrt(float((int(H) - 1) ** 2 + (int(W) - 1) ** 2)))
    with np.errstate(invalid="ignore", divide="ignore"):
        qf, qo = ff[..., 0], fo[..., 0]
        A = (qf - qo) / (0.5 * (qf + qo))
        cf, co = ff[..., 1:] / qf[..., None], fo[..., 1:] / qo[..., None]
        dist = np.sqrt(((cf - co) ** 2).sum(-1))
        L1 = np.where(np.isnan(dist), np.nan, dist / d if d > 0 else 0.0)
        both = (rf > 0) & (ro > 0)
        vf, vo = sf[..., 0] / rf, so[..., 0] / ro
        S = np.where(both, (vf - vo) / (0.5 * (vf + vo)), np.nan)
        spread = np.abs(sf[..., 1] / rf - so[..., 1] / ro)
        L2 = np.where(both, 2.0 * spread / d if d > 0 else 0.0, np.nan)
    return dict(S=S, A=A, L1=L1, L2=L2, L=L1[..., None] + L2)


def mean_valid(x, C, out=None):
    """mean over the C valid channels of a C16 tensor -> device scalar (no grad)."""
    x = x.detach().contiguous()
    _check(x)
    Cp = x.shape[-1]
    if out is None:
        out = torch.empty((), device=x.device, dtype=torch.float32)
    ws, nb = _red_ws()
    _lib.call("acg_mean_fwd", _ptr(x), x.numel() // Cp, C, Cp, _ptr(out), _ptr(ws), nb, _stream())
    return out


def sumsq(flat, out):
    """out[0] = sum(flat^2) (first half of clip_grad_norm)."""
    _check(flat)
    ws, nb = _red_ws()
    _lib.call("acg_sumsq", _ptr(flat), flat.numel(), _ptr(out), _ptr(ws), nb, _stream())
    return out


def clip_adam_multi(groups, max_norm, lr, beta1, beta2, eps, step, step_dev=None):
    """clip_grad_norm + Adam for all networks of a phase in three launches; groups = [(p, g, m, v, sumsq), ...] flat fp32
    buffers of each network (sumsq: 1-element tensor that receives the gradient sum of squares).  step_dev: int32 device
    tensor holding the number of COMPLETED steps (graph capture: the kernel reads it instead of `step`)."""
    n = len(groups)
    arr = (_lib.AdamGroup * n)()
    for i, (p, g, m, v, ss) in enumerate(groups):
        _check(p, g, m, v, ss)
        if not (p.numel() == g.numel() == m.numel() == v.numel()):
            raise _lib.AcgError("clip_adam_multi: group %d buffers differ in size" % i)
        arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n, arr[i].sumsq = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                                                           p.numel(), ss.data_ptr())
    nb = _lib.query("acg_clip_adam_multi_workspace_bytes", n)
    ws = workspace(nb, slot=1)
    _lib.call("acg_clip_adam_multi", arr, n, float(max_norm), float(lr), float(beta1), float(beta2), float(eps), int(step),
              _ptr(step_dev), _ptr(ws), nb, _stream())


def _ema_groups(who, groups):
    n = len(groups)
    arr = (_lib.EmaGroup * n)()
    for i, (p, e) in enumerate(groups):
        _check(p, e)
        if p.numel() != e.numel():
            raise _lib.AcgError("%s: group %d buffers differ in size" % (who, i))
        arr[i].p, arr[i].e, arr[i].n = p.data_ptr(), e.data_ptr(), p.numel()
    return arr, n


def ema_multi(groups, decay, step, step_dev=None):
    """the averaged weights of all networks of an optimiser in one launch; groups = [(p, e), ...] flat fp32 buffers:
    e += (1 - d) (p - e), d = min(decay, (1 + t) / (10 + t)), t = `step` (the 1-based step just taken) or, with step_dev
    (int32 device tensor holding the number of COMPLETED steps, graph capture), step_dev + 1 read by the kernel."""
    arr, n = _ema_groups("ema_multi", groups)
    _lib.call("acg_ema_multi", arr, n, float(decay), int(step), _ptr(step_dev), _stream())


def swap_multi(groups):
    """exchange p and e of every group in place, one launch; groups as ema_multi's"""
    arr, n = _ema_groups("swap_multi", groups)
    _lib.call("acg_swap_multi", arr, n, _stream())


def adam_step(p, g, m, v, sumsq_t, max_norm, lr, beta1, beta2, eps, step, scale_grads=True):
    """clip (coefficient from the device-side sum of squares) + Adam on one flat buffer."""
    _check(p, g, m, v)
    _lib.call("acg_adam_step", _ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), _ptr(sumsq_t), float(max_norm), float(lr),
              float(beta1), float(beta2), float(eps), int(step), 1 if scale_grads else 0, _stream())
