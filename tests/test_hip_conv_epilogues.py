"""The convolutions' fused epilogues (bias + ReLU / LeakyReLU(0.2) / tanh in the kernel that computes the layer) and their
no-bias forms (bias == nullptr forward, db == nullptr in the weight gradients), per kernel family, against float64 torch.

Every other convolution parity test drives its layer as conv + bias with ACT_NONE; the networks fuse the activation into
the convolution wherever no norm follows (modules._run_stages), and E_B's stages 2-5 carry no bias.  The cases here are
the smallest shapes each family's dispatch predicate accepts (most of them proven inside the predicate by
test_hip_fastpath_fuzz), built as the networks build them: M.Sequential([ReflectionPad2d], Conv2d, Act) and
ConvTranspose2d.forward_nhwc(x, act).

Inputs: x ~ N(0, 1), w ~ N(0, 1 / sqrt(Ci K^2)) (unit-scale pre-activations: the 0.3 used elsewhere saturates every tanh
at 32 x 49 taps), b ~ N(0, 0.5), dy ~ N(0, 1), rounded to fp32 (the values the kernels consume), seeded from
zlib.crc32 of the shape id.  Reference: float64 torch on the device (on the host if it has no fp64 convolution),
pre = conv(x, w, b), y_ref = act(pre); one reference per (shape, bias), shared by the activations and arithmetics.

Bars, derived and not tuned:
  forward   The bar of the ACT_NONE tests allows an absolute pre-activation error of 2e-5 max|pre|.  ReLU, LeakyReLU and
            tanh are 1-Lipschitz, so  max|y - y_ref| < 2e-5 max|pre| + 4 * 2^-24 ; the last term is tanhf against fp64
            at |y| <= 1.  Absolute, not relative to max|y|: for tanh max|y| ~ 1 while max|pre| ~ 4.5.
  backward  The kernels form the pre-activation gradient from their OWN output (acg_act_bwd, pinned element-wise by
            test_act_bwd), so the reference does the same in float64: g = dy * act'(y_kernel) (slope 1 where y_kernel > 0,
            else 0 / 0.2; 1 - y^2 for tanh), then dx, dw, db = the fp64 adjoints of the convolution at g.  The bars of the
            ACT_NONE tests: 2e-5 on dx, 1e-4 on dw and db (max-abs error / max-abs value).  This pins the linear maps and
            their db == nullptr branches without letting ReLU flips blur them.
  pattern   relu / lrelu: y_kernel > 0 equals pre > 0 everywhere outside the band |pre| < 2e-5 max|pre| (a wrong mask
            fails although the gradient check is conditioned on it); the band holds at most 1e-3 of the cells, asserted
            on the reference alone (about 7e-5 expected for unit-scale Gaussians; at most 2.8e-4 over the seeds here).
  bias=False  conv.bias is None, no bias gradient exists, and y, dx, dw meet the same bars.
  C ABI     y pre-filled with NaN: every stored element finite, the real channels inside the forward bar, the pad
            channels exactly 0.0.

In bf16x3 the forward kernel (for the weight-gradient rows, the weight-gradient kernel) must be the family the row names
(MATRIX / WGRAD, names as acg_last_kernel reports them); in strict f32 none of the bf16x3 fast paths may run, and the
thin-output rows must take the VALU kernel.  The cross-check kernels (ops.set_conv_impl("direct")) run three small shapes,
the pre-split trunk kernel (acg_conv2d_fwd_s16) two of test_hip_fastpath_fuzz.S16_CASES.

397 tests: 20 shapes x 3 activations x bias / no bias x 2 arithmetics through the modules (240), 3 weight-gradient shapes x
{none, relu} x bias / no bias x 2 arithmetics (24), 3 shapes x 3 x 2 on the cross-check kernels (18), 9 shapes x 3 x 2 x 2
through the C ABI (108), 2 x 3 on the pre-split trunk (6), and the band cap.  The whole file takes 6.3 s on one MI355X;
the slowest test, the first, 0.9 s.  Worst errors measured there, over all shapes and both arithmetics (share of the bar):
    relu    y 3.5e-5 absolute (0.35)   dx 9.1e-6 (0.46)   dw 5.8e-6 (0.06)   db 3.9e-6 (0.04)
    lrelu   y 3.5e-5 absolute (0.35)   dx 8.8e-6 (0.44)   dw 5.8e-6 (0.06)   db 3.3e-6 (0.03)
    tanh    y 3.1e-5 absolute (0.31)   dx 1.4e-5 (0.70)   dw 9.7e-6 (0.10)   db 3.1e-6 (0.03)
    none    y 1.9e-5 absolute (0.23)   dx 5.3e-6 (0.26)   dw 4.9e-6 (0.05)   db 2.1e-7 (0.002)   (weight-gradient rows only)
No activation pattern differed outside the band.  The file fails when it should: with the LeakyReLU slope of
conv_igemm.hip's unrolled epilogue branch set to 0.25, all 52 lrelu tests that run that kernel went red (every f32 case
but the thin-output rows, and the discriminator first layers in bf16x3); with conv_patchn_x3 applying the activation
before the bias, all 18 bf16x3 tests of the head rows with a bias did.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conv_cases import FAST, KROW, ROWS, S16_CASES, WS, _dev_t, _match, _nchw, _nhwc, _pad_c, _ref_device

pytestmark = pytest.mark.gpu

GENERIC = "igemm_conv_bf16<128,32,KC=%d,REFLECT=0,SPLIT=1>"    # the generic tile WITHOUT the row-patch stages (",RP=1>")
DIRECT = "direct_fwd_kernel"
VALU = "thin_out_conv<"


def _r(fam, geo, fwd, tr=False, wgrad=None, fwd_f32=None):
    return (fam, geo, tr, fwd, wgrad, fwd_f32)


# (family, (K, stride, pad, mode, Ci, Co, N, H, W), transpose, forward kernel in bf16x3, weight-gradient kernel in bf16x3 or
# None, forward kernel in f32 or None): substrings of the name the dispatcher reports (acg_last_kernel), '=': the whole name.
# transpose: M.ConvTranspose2d(Ci, Co, 3, 2, 1, output_padding=1) on an N x Ci x H x W input.  No activation is sent to
# another kernel than the family's: each row holds for relu, lrelu and tanh, with and without a bias.
MATRIX = [
    _r("rows", (3, 1, 1, "zero", 32, 64, 1, 3, 128), ROWS),
    _r("rows", (3, 1, 1, "zero", 32, 64, 2, 5, 256), ROWS),
    _r("rp", (3, 1, 1, "zero", 64, 32, 1, 4, 128), "igemm_conv_bf16<128,32,KC=32,REFLECT=0,SPLIT=1,RP=1>"),
    _r("ws", (3, 1, 1, "reflect", 96, 192, 2, 13, 40), "igemm_conv_x3_ws<REFLECT=1,STATS=0,ROWP=1>"),
    _r("ws", (3, 1, 1, "reflect", 128, 128, 1, 16, 16), "igemm_conv_x3_ws<REFLECT=1,STATS=0,ROWP=1>"),
    _r("ws", (4, 2, 1, "zero", 64, 128, 2, 34, 50), "igemm_conv_x3_ws<REFLECT=0,STATS=0,ROWP=0>"),
    _r("ws", (3, 2, 1, "zero", 64, 128, 2, 33, 61), "igemm_conv_x3_ws<REFLECT=0,STATS=0,ROWP=0>"),
    _r("ph4", (3, 2, 1, "zero", 128, 64, 1, 5, 128), "igemm_conv_ph4<128,64> (", tr=True),
    _r("ph4", (3, 2, 1, "zero", 96, 64, 3, 4, 384), "igemm_conv_ph4<128,64> (", tr=True),
    _r("stem", (7, 1, 3, "reflect", 3, 32, 1, 45, 130), "conv_thinrow_x3<REFLECT=1> (7x7"),
    _r("stem", (3, 1, 1, "zero", 3, 32, 4, 33, 40), "conv_thinrow_x3<REFLECT=0> (3x3"),
    _r("head", (7, 1, 3, "zero", 32, 3, 3, 37, 50), "conv_patchn_x3<REFLECT=0> (7x7", fwd_f32=VALU),
    _r("head", (4, 1, 1, "zero", 32, 2, 2, 17, 19), "conv_patchn_x3<REFLECT=0> (4x4", fwd_f32=VALU),
    _r("head", (3, 1, 1, "reflect", 32, 3, 1, 48, 200), "conv_patchn_x3<REFLECT=1> (3x3", fwd_f32=VALU),
    # thin fp32 tile with bf16x3 products (C4 image in, stride 2)
    _r("disc", (4, 2, 1, "zero", 3, 64, 2, 16, 16), "igemm_conv_f32<128,64,KC=32,REFLECT=0,THIN=1,X3=1>"),
    _r("disc", (3, 2, 1, "zero", 3, 32, 2, 15, 13), "igemm_conv_f32<128,32,KC=32,REFLECT=0,THIN=1,X3=1>"),
    _r("generic", (3, 1, 1, "zero", 6, 40, 1, 20, 20), GENERIC % 16),
    _r("generic", (1, 1, 0, "zero", 64, 16, 2, 3, 3), GENERIC % 32),
    _r("generic", (3, 2, 1, "zero", 16, 32, 1, 15, 13), GENERIC % 16),
    # the thin-output VALU kernel takes this one in f32 only (bf16x3: the N-packed head kernel)
    _r("valu", (4, 1, 0, "zero", 32, 1, 3, 6, 6), "conv_patchn_x3<REFLECT=0> (4x4", fwd_f32=VALU),
]
# weight-gradient families with db == nullptr
WGRAD = [
    _r("krow", (3, 1, 1, "zero", 128, 128, 1, 3, 32), WS, wgrad=KROW),
    _r("krowg", (4, 1, 1, "zero", 128, 128, 2, 9, 17), WS, wgrad="wgrad_x3_krowg<NT=4,IS=1,BCI=128>"),
    _r("krowg", (3, 2, 1, "zero", 128, 64, 2, 8, 16), GENERIC.replace(",32,", ",64,") % 32, tr=True, wgrad="wgrad_x3_krowg<NT=3,IS=2,BCI=64>"),
]
DIRECT_SHAPES = [MATRIX[16], MATRIX[17], MATRIX[15]]
# one shape per family for the C-ABI forward (NaN pre-fill, pad channels)
ABI = [MATRIX[16], MATRIX[11], MATRIX[0], MATRIX[2], MATRIX[3], MATRIX[10], MATRIX[15], MATRIX[19], MATRIX[7]]

ACTS = {"none": None, "relu": nn.ReLU, "lrelu": lambda: nn.LeakyReLU(0.2), "tanh": nn.Tanh}
SEED_SALT = {}   # shape id -> suffix of the seed string, for a seed whose reference band share exceeded the cap (none did)


def _sid(row):
    K, s, p, mode, Ci, Co, N, H, W = row[1]
    return "%s_%sk%ds%dp%d%s_%dto%d_%dx%dx%d" % (row[0], "T" if row[2] else "", K, s, p, mode, Ci, Co, N, H, W)


def _code(act):
    from dtgan_amd import ops
    return {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU, "tanh": ops.ACT_TANH}[act]


def _inputs(row):
    """seeded x, weight, bias and output gradient (NCHW, float64 holding fp32 values)"""
    K, s, p, mode, Ci, Co, N, H, W = row[1]
    tr = row[2]
    sid = _sid(row)
    rs = np.random.RandomState(zlib.crc32((sid + SEED_SALT.get(sid, "")).encode()))
    x = rs.normal(0, 1, (N, Ci, H, W))
    w = rs.normal(0, 1.0 / np.sqrt(Ci * K * K), (Ci, Co, K, K) if tr else (Co, Ci, K, K))
    b = rs.normal(0, 0.5, (Co,))
    Ho, Wo = (2 * H, 2 * W) if tr else ((H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1)
    dy = rs.normal(0, 1, (N, Co, Ho, Wo))
    return [a.astype(np.float32).astype(np.float64) for a in (x, w, b, dy)]


def _conv64(row, X, Wt, B):
    K, s, p, mode, Ci, Co, N, H, W = row[1]
    if row[2]:
        return F.conv_transpose2d(X, Wt, B, stride=2, padding=1, output_padding=1)
    if mode == "reflect":
        return F.conv2d(F.pad(X, (p, p, p, p), mode="reflect"), Wt, B, stride=s)
    return F.conv2d(X, Wt, B, stride=s, padding=p)


_REFS = {}


def _reference(row, bias, x=None, w=None, b=None):
    """-> (leaves, pre with its graph, pre as numpy, max|pre|) of the fp64 layer; computed once per (shape, bias)"""
    key = (_sid(row), bias) if x is None else None
    if key is None or key not in _REFS:
        if x is None:
            x, w, b, _ = _inputs(row)
        dev = _ref_device()
        leaves = [torch.tensor(a, dtype=torch.float64, device=dev, requires_grad=True) for a in ((x, w, b) if bias else (x, w))]
        pre = _conv64(row, leaves[0], leaves[1], leaves[2] if bias else None)
        pre_n = pre.detach().cpu().numpy()
        ref = (leaves, pre, pre_n, float(np.abs(pre_n).max()))
        if key is None:
            return ref
        _REFS[key] = ref
    return _REFS[key]


def _act64(pre, act):
    if act == "relu":
        return np.maximum(pre, 0.0)
    if act == "lrelu":
        return np.where(pre > 0, pre, 0.2 * pre)
    if act == "tanh":
        return np.tanh(pre)
    return pre


def _slope64(y, act):
    """act'(pre) through the kernel's own output, as acg_act_bwd forms it"""
    y = y.astype(np.float64)
    if act == "relu":
        return (y > 0).astype(np.float64)
    if act == "lrelu":
        return np.where(y > 0, 1.0, 0.2)
    if act == "tanh":
        return 1.0 - y * y
    return np.ones_like(y)


def _band_share(pre_n, pmax):
    return float((np.abs(pre_n) < 2e-5 * pmax).mean())


def _check_forward(tag, y, pre_n, pmax, act):
    """the forward bar, and for relu / lrelu the pattern outside the band; -> error / bar"""
    assert y.shape == pre_n.shape, (y.shape, pre_n.shape)
    assert np.isfinite(y).all(), "y not finite"
    bar = 2e-5 * pmax + 4 * 2.0 ** -24
    err = float(np.abs(y.astype(np.float64) - _act64(pre_n, act)).max())
    print("EPI", tag, act, "y err %.3e bar %.3e ratio %.3f" % (err, bar, err / bar))
    assert err < bar, ("y", err, bar)
    if act in ("relu", "lrelu"):
        assert _band_share(pre_n, pmax) <= 1e-3, "band share of the reference (change the seed)"
        out = np.abs(pre_n) >= 2e-5 * pmax
        wrong = int((((y > 0) != (pre_n > 0)) & out).sum())
        assert wrong == 0, ("activation pattern differs outside the band", wrong)
    return err / bar


def _run_module(row, act, bias, prec, impl="mfma"):
    """the layer as the networks run it -> (y, dx, dw, db or None), (forward, data-gradient, weight-gradient kernels)"""
    from hip_util import t, n, Spy, precision
    from dtgan_amd import modules as M, ops
    K, s, p, mode, Ci, Co, N, H, W = row[1]
    x, w, b, dy = _inputs(row)
    with precision(prec):
        if impl != "mfma":
            ops.set_conv_impl(impl)
        try:
            if row[2]:
                conv = M.ConvTranspose2d(Ci, Co, 3, 2, 1, output_padding=1, bias=bias).cuda()
                entry = "acg_conv_transpose2d_"
            else:
                reflect = mode == "reflect"
                conv = M.Conv2d(Ci, Co, K, stride=s, padding=0 if reflect else p, bias=bias)
                mods = ([nn.ReflectionPad2d(p)] if reflect else []) + [conv] + ([ACTS[act]()] if ACTS[act] else [])
                m, entry = M.Sequential(*mods).cuda(), "acg_conv2d_"
            assert (conv.bias is not None) == bias
            with torch.no_grad():
                conv.weight.copy_(t(w))
                if bias:
                    conv.bias.copy_(t(b))
            xt = t(x, grad=True)
            with Spy() as spy:
                if row[2]:
                    y = ops.ToNCHW.apply(conv.forward_nhwc(ops.ToNHWC.apply(xt), _code(act)), Co)
                else:
                    y = m(xt)
                y.backward(t(dy))
            got = (spy.kernels(entry + "fwd"), spy.kernels(entry + "bwd_data"), spy.kernels(entry + "bwd_weight"))
            if not bias:
                assert conv.bias is None and [k for k, _ in conv.named_parameters()] == ["weight"], "a bias (gradient) exists"
            res = (n(y), n(xt.grad), n(conv.weight.grad), n(conv.bias.grad) if bias else None)
        finally:
            if impl != "mfma":
                ops.set_conv_impl("mfma")
    print("KERNELS", _sid(row), act, bias, prec, impl, got)
    return res, got


def _check_module(row, act, bias, prec, impl="mfma"):
    from hip_util import rel
    (y, dx, dw, db), got = _run_module(row, act, bias, prec, impl)
    if impl == "direct":
        assert got[0] and all(k == DIRECT for k in got[0]), got
    elif prec == "bf16x3":
        assert got[0] and all(_match(row[3], k) for k in got[0]), ("forward", row[3], got[0])
        assert row[4] is None or (got[2] and all(_match(row[4], k) for k in got[2])), ("weight gradient", row[4], got[2])
    else:   # strict f32: the bf16x3-only fast paths must not run
        for have, what in zip(got, ("forward", "data gradient", "weight gradient")):
            assert have and not any(f.lstrip("=") in k for f in FAST for k in have), (what, have)
        assert row[5] is None or all(_match(row[5], k) for k in got[0]), ("forward", row[5], got[0])
    leaves, pre, pre_n, pmax = _reference(row, bias)
    tag = "%s %s %s bias=%d" % (_sid(row), prec, impl, bias)
    _check_forward(tag, y, pre_n, pmax, act)
    g = _inputs(row)[3] * _slope64(y, act)
    grads = torch.autograd.grad(pre, leaves, torch.tensor(g, dtype=torch.float64, device=pre.device), retain_graph=True)
    grads = [v.cpu().numpy() for v in grads]
    have = (dx, dw, db) if bias else (dx, dw)
    for a, r, name, bar in zip(have, grads, ("dx", "dw", "db"), (2e-5, 1e-4, 1e-4)):
        assert a.shape == r.shape, name
        e = rel(a, r)
        print("EPI", tag, act, "%s err %.3e bar %.0e ratio %.3f" % (name, e, bar, e / bar))
        assert e < bar, (name, e)


def test_reference_band_shares_are_under_the_cap():
    """the cells with |pre| < 2e-5 max|pre| are at most 1e-3 of all, for every (shape, bias) a ReLU pattern is checked on"""
    for row in MATRIX + WGRAD:
        for bias in (True, False):
            _, _, pre_n, pmax = _reference(row, bias)
            assert _band_share(pre_n, pmax) <= 1e-3, (_sid(row), bias, _band_share(pre_n, pmax))


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", ["relu", "lrelu", "tanh"])
@pytest.mark.parametrize("row", MATRIX, ids=_sid)
def test_fused_epilogue_against_fp64(row, act, bias, prec):
    _check_module(row, act, bias, prec)


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("row", WGRAD, ids=_sid)
def test_weight_gradient_families_without_bias_against_fp64(row, act, bias, prec):
    """the kernel-row weight gradients at their own dispatch shapes with db == nullptr (and, for comparison, with a bias)"""
    _check_module(row, act, bias, prec)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", ["relu", "lrelu", "tanh"])
@pytest.mark.parametrize("row", DIRECT_SHAPES, ids=_sid)
def test_direct_cross_check_epilogue_against_fp64(row, act, bias):
    """the naive cross-check kernels (ops.set_conv_impl("direct")) have an epilogue of their own"""
    _check_module(row, act, bias, "bf16x3", impl="direct")


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", ["relu", "lrelu", "tanh"])
@pytest.mark.parametrize("row", ABI, ids=_sid)
def test_c_abi_forward_unwritten_elements_and_pad_channels(row, act, bias, prec):
    """acg_conv2d_fwd / acg_conv_transpose2d_fwd into a NaN-filled y: all stored elements finite, real channels inside the
    forward bar, pad channels exactly 0.0"""
    from dtgan_amd import ops, _lib
    from hip_util import precision, n
    K, s, p, mode, Ci, Co, N, H, W = row[1]
    tr = row[2]
    P = ops._ptr
    x, w, b, _ = _inputs(row)
    with precision(prec):
        st = ops._stream()
        bt = _dev_t(b) if bias else None
        if tr:
            pk = ops.PackedConv(_dev_t(w), bt, ops.cpad(Co), ops.cpad(Ci))
            d = ops.conv_desc(N, 2 * H, 2 * W, pk.Ci, pk.Co, 3, 2, 1, ops.PAD_ZERO)
            assert (d.Ho, d.Wo) == (H, W)
            xin = _dev_t(_pad_c(_nhwc(x), pk.Co, 3))
            y = torch.full((N, 2 * H, 2 * W, pk.Ci), float("nan"), device="cuda")
            _lib.call("acg_conv_transpose2d_fwd", ctypes.byref(d), P(xin), P(pk.wb), P(pk.bias if bias else None), P(y), _code(act), st)
        else:
            pk = ops.PackedConv(_dev_t(w), bt, ops.cpad(Ci), ops.cpad(Co))
            d = ops.conv_desc(N, H, W, pk.Cis, pk.Cos, K, s, p, ops.PAD_REFLECT if mode == "reflect" else ops.PAD_ZERO, Ci, Co)
            xin = _dev_t(_pad_c(_nhwc(x), pk.Cis, 3))
            y = torch.full((N, d.Ho, d.Wo, pk.Cos), float("nan"), device="cuda")
            _lib.call("acg_conv2d_fwd", ctypes.byref(d), P(xin), P(pk.wf), P(pk.bias if bias else None), P(y), _code(act), st)
        kern = _lib.query("acg_last_kernel").decode()
        torch.cuda.synchronize()
        y = n(y)
    print("KERNEL", _sid(row), act, bias, prec, kern)
    if prec == "bf16x3":
        assert _match(row[3], kern), (row[3], kern)
    else:
        assert not any(f.lstrip("=") in kern for f in FAST) and (row[5] is None or _match(row[5], kern)), kern
    assert np.isfinite(y).all(), "%d stored elements were not written (or are not finite)" % int((~np.isfinite(y)).sum())
    _, _, pre_n, pmax = _reference(row, bias)
    _check_forward("abi %s %s bias=%d" % (_sid(row), prec, bias), _nchw(y)[:, :Co], pre_n, pmax, act)
    pad = y[..., Co:]
    assert (pad == 0.0).all(), "pad channels must stay exactly 0 (%d do not)" % int((pad != 0.0).sum())


@pytest.mark.parametrize("act", ["relu", "lrelu", "tanh"])
@pytest.mark.parametrize("case", [S16_CASES[0], S16_CASES[5]], ids=lambda c: "%dx%dx%d_%dto%d" % c)
def test_presplit_trunk_forward_epilogue_against_fp64(case, act):
    """acg_conv2d_fwd_s16 with each activation, fp32 output, no statistics, on the pre-split operand decode(encode(x))"""
    from dtgan_amd import ops, _lib
    from hip_util import precision, n
    N, H, W, Ci, Co = case
    P = ops._ptr
    row = _r("s16", (3, 1, 1, "reflect", Ci, Co, N, H, W), None)
    x, w, b, _ = _inputs(row)
    with precision("bf16x3"):
        st = ops._stream()
        d = ops.conv_desc(N, H, W, Ci, Co, 3, 1, 1, ops.PAD_REFLECT, Ci, Co)
        assert _lib.query("acg_conv2d_s16_supported", ctypes.byref(d))
        pk = ops.PackedConv(_dev_t(w), _dev_t(b), Ci, Co)
        xf = _dev_t(_nhwc(x))
        xs, xv = torch.empty_like(xf), torch.empty_like(xf)
        _lib.call("acg_s16_encode", P(xf), P(xs), xf.numel(), st)
        _lib.call("acg_s16_decode", P(xs), P(xv), xs.numel(), st)
        y = torch.full((N, H, W, Co), float("nan"), device="cuda")
        _lib.call("acg_conv2d_fwd_s16", ctypes.byref(d), P(xs), P(pk.wf), P(pk.bias), P(y), _code(act), None, 0, st)
        kern = _lib.query("acg_last_kernel").decode()
        torch.cuda.synchronize()
        y, xv = n(y), n(xv).astype(np.float64)
    print("KERNEL", case, act, kern)
    assert kern.startswith("igemm_conv_x3_pre"), kern
    _, _, pre_n, pmax = _reference(row, True, _nchw(xv), w, b)
    _check_forward("s16 %s" % (case,), _nchw(y), pre_n, pmax, act)
