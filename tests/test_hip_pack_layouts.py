"""The packed weight layouts, pinned bit for bit.

acg_pack_conv_weight / acg_pack_conv_weights_multi against reference packers written in torch on the CPU straight from the
layout comments above the pack kernels (csrc/conv_pack.hip).  Every comparison is on bit patterns: the buffers are
acg_packed_w?_elems floats pre-filled with a NaN sentinel, and outside the extents the layer's forms occupy the sentinel must
still be there afterwards (thin forms are shorter than the buffer; the fp32 packing writes no mirrored-row slabs, ...).
"""
import pytest
import torch

from hip_util import precision

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF   # a quiet NaN no packer produces

# (Or, Ir, K, Ci, Co): the smallest layers that reach every form and every padding rule
LAYERS = [
    (16, 16, 3, 16, 16),     # regular; the three extra wb slabs
    (20, 24, 1, 32, 32),     # K = 1; real counts below the padded ones: zero fill
    (40, 16, 4, 16, 48),     # a column count acg_ncols_pad rounds up
    (3, 3, 3, 16, 16),       # both sides thin: stays regular
    (32, 3, 7, 16, 32),      # the stem: thin-K wf + row-packed tail, wb + N-packed tail
    (64, 3, 4, 16, 64),      # thin-K wf; wb thin-N in the fp32 mode, regular otherwise
    (128, 3, 4, 16, 128),    # wb regular in every mode
    (3, 32, 7, 32, 16),      # the head: N-packed wf tail, row-packed wb tail
    (1, 64, 4, 64, 16),      # PatchGAN head: thin-N forward in the fp32 mode
]
PRECS = ["f32", "bf16", "bf16x3"]
IMPLS = ["mfma", "direct"]


class mode(object):
    """precision + implementation for the duration of a block, both restored afterwards"""

    def __init__(self, prec, impl):
        self.p, self.impl = precision(prec), impl

    def __enter__(self):
        from dtgan_amd import ops
        self.p.__enter__()
        ops.set_conv_impl(self.impl)

    def __exit__(self, *a):
        from dtgan_amd import ops
        try:
            ops.set_conv_impl("mfma")
        finally:
            self.p.__exit__(*a)


def _weights(Or, Ir, K, seed):
    """random normal weights plus values that do not survive bf16 rounding (so the lo halves are non-trivial)"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(Or, Ir, K, K, generator=g, dtype=torch.float32)
    flat = w.view(-1)
    special = torch.tensor([1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -8 + 2.0 ** -16), 3.0 + 2.0 ** -12, 2.0 ** -20 + 2.0 ** -30, -0.1],
                           dtype=torch.float32)
    idx = torch.arange(special.numel()) * 7 % flat.numel()
    flat[idx] = special
    return w


# ------------------------------------------------------------------------------------------------------------------------
# reference packers: index arithmetic copied from the layout comments, gathered through one bounded OIHW fetch
# ------------------------------------------------------------------------------------------------------------------------
def _fetch(w, o, i, kh, kw):
    """w[o][i][kh][kw], or 0 outside the real Or x Ir x K x K block (index tensors of one shape)"""
    Or, Ir, K, _ = w.shape
    ok = (o >= 0) & (o < Or) & (i >= 0) & (i < Ir) & (kh >= 0) & (kh < K) & (kw >= 0) & (kw < K)
    z = torch.zeros_like(o)
    v = w[torch.where(ok, o, z), torch.where(ok, i, z), torch.where(ok, kh, z), torch.where(ok, kw, z)]
    return torch.where(ok, v, torch.zeros((), dtype=torch.float32))


def _grid(*dims):
    return torch.meshgrid(*[torch.arange(d) for d in dims], indexing="ij")


def _bits32(v):
    return v.contiguous().view(torch.int32).reshape(-1)


def _hi_lo(v):
    hi = v.to(torch.bfloat16)
    lo = (v - hi.float()).to(torch.bfloat16)
    return hi.contiguous().view(torch.int16).reshape(-1), lo.contiguous().view(torch.int16).reshape(-1)


def ref_regular_f32(w, C_k, ColP, fwd):
    """wf [tap][Ci/8][CoP][8] (fwd) or wb [tap][Co/8][CiP][8]: k = 8 cb + c8 runs over the gathered channels (C_k of them)"""
    K = w.shape[2]
    tap, cb, col, c8 = _grid(K * K, C_k // 8, ColP, 8)
    k = cb * 8 + c8
    o, i = (col, k) if fwd else (k, col)
    return _bits32(_fetch(w, o, i, tap // K, tap % K))


def ref_regular_bf16(w, C_k, ColP, fwd, split):
    """wf16 [tap][Ci/16][CoP][16] / wb16 [slab][Co/16][CiP][16] as int16 words: hi, and with `split` lo right behind.
    wb of a 3x3 layer carries three more slabs 9 + kw = w[0][kw] + w[2][kw] (an fp32 add)"""
    K = w.shape[2]
    slabs = K * K + (3 if (K == 3 and not fwd) else 0)
    tap, cb, col, c16 = _grid(slabs, C_k // 16, ColP, 16)
    k = cb * 16 + c16
    o, i = (col, k) if fwd else (k, col)
    own = _fetch(w, o, i, tap // K, tap % K)
    v = own
    if slabs > K * K:
        kw = tap - K * K
        z = torch.zeros_like(tap)
        v = torch.where(tap < K * K, own, _fetch(w, o, i, z, kw) + _fetch(w, o, i, z + 2, kw))
    hi, lo = _hi_lo(v)
    return torch.cat([hi, lo]) if split else hi


def ref_thin_k(w, ColP, mode_):
    """out[kc][col][8]: rows k = 8 kc + c8 = tap * 4 + c.  mode 0: w[col][c][tap]; mode 1: w[c][col][tap]"""
    K = w.shape[2]
    nkc = 4 * ((K * K + 7) // 8)
    kc, col, c8 = _grid(nkc, ColP, 8)
    kflat = kc * 8 + c8
    tap, c = kflat >> 2, kflat & 3
    o, i = (col, c) if mode_ == 0 else (c, col)
    v = _fetch(w, o, i, tap // K, tap % K)   # tap >= K*K: kh >= K -> 0
    return _bits32(v)


def ref_thin_n(w, Kc, mode_):
    """out[(tap * Kc + k) * 4 + n].  mode 0: w[n][k][tap]; mode 1: w[k][n][tap]"""
    K = w.shape[2]
    tap, k, n = _grid(K * K, Kc, 4)
    o, i = (n, k) if mode_ == 0 else (k, n)
    return _bits32(_fetch(w, o, i, tap // K, tap % K))


def ref_trow(w, mode_):
    """out[hi | lo][ry][kg (4)][col (32)][8]: kw = 2 kg + (j >> 2), ch = j & 3.  mode 0: w[col][ch][ry][kw];
    mode 1: w[ch][col][K-1-ry][K-1-kw]; zero for kw >= K"""
    K = w.shape[2]
    ry, kg, col, j = _grid(K, 4, 32, 8)
    kw, ch = 2 * kg + (j >> 2), j & 3
    if mode_ == 0:
        v = _fetch(w, col, ch, ry, kw)
    else:
        v = torch.where(kw < K, _fetch(w, ch, col, K - 1 - ry, K - 1 - kw), torch.zeros((), dtype=torch.float32))
    return torch.cat(_hi_lo(v))


def ref_npack(w, mode_):
    """out[hi | lo][ry * (K + 3) + u][kg (4)][col (16)][8]: k = 8 kg + j, col = 4 dxo + c, kw = u - dxo.
    mode 0: w[c][k][ry][kw]; mode 1: w[k][c][K-1-ry][K-1-kw]; zero where kw falls outside the kernel"""
    K = w.shape[2]
    ry, u, kg, col, j = _grid(K, K + 3, 4, 16, 8)
    k, dxo, c = kg * 8 + j, col >> 2, col & 3
    kw = u - dxo
    inside = (kw >= 0) & (kw < K)
    if mode_ == 0:
        v = _fetch(w, c, k, ry, kw)
    else:
        v = _fetch(w, k, c, K - 1 - ry, K - 1 - kw)
    return torch.cat(_hi_lo(torch.where(inside, v, torch.zeros((), dtype=torch.float32))))


# ------------------------------------------------------------------------------------------------------------------------
# which forms a layer carries (DESIGN.md "Dispatch rules"; the comments of the size rules in csrc/conv_internal.h)
# ------------------------------------------------------------------------------------------------------------------------
def _ncols_pad(c):
    from dtgan_amd import _lib
    return int(_lib.query("acg_ncols_pad", c))


def expected(w, Ci, Co, prec, impl):
    """-> (wf, wb) as int32 bit patterns of acg_packed_w?_elems words each, the sentinel wherever nothing is written"""
    from dtgan_amd import _lib
    Or, Ir, K, _ = w.shape
    mfma = impl == "mfma"
    bf16 = mfma and prec != "f32"
    x3 = mfma and prec == "bf16x3"
    thin = lambda c: mfma and K > 1 and 1 <= c <= 4   # noqa: E731
    thin_in, thin_out = thin(Ir) and not thin(Or), thin(Or) and not thin(Ir)
    valu = lambda C: (not bf16) and C in (16, 32, 64)   # noqa: E731  the VALU thin-output kernel: fp32 mode, <= 64 channels
    CoP, CiP = _ncols_pad(Co), _ncols_pad(Ci)
    n_wf = int(_lib.query("acg_packed_wf_elems", K, Ci, Co))
    n_wb = int(_lib.query("acg_packed_wb_elems", K, Ci, Co))
    wb_slabs = K * K + (3 if K == 3 else 0)
    wf_regular, wb_regular = K * K * (Ci // 8) * CoP * 8, wb_slabs * (Co // 8) * CiP * 8
    tail = 1 < K <= 7
    npack_f, trow_b = (tail and Co == 16 and Ci == 32), (tail and Co == 16 and Ci == 32)
    npack_b, trow_f = (tail and Ci == 16 and Co == 32), (tail and Ci == 16 and Co == 32)
    assert n_wf == wf_regular + (K * (K + 3) * 512 if npack_f else 0) + (K * 1024 if trow_f else 0)
    assert n_wb == wb_regular + (K * (K + 3) * 512 if npack_b else 0) + (K * 1024 if trow_b else 0)

    def regular(fwd):
        C_k, ColP = (Ci, CoP) if fwd else (Co, CiP)
        if bf16:
            return ref_regular_bf16(w, C_k, ColP, fwd, x3).view(torch.int32)
        return ref_regular_f32(w, C_k, ColP, fwd)

    if thin_in:
        main_f = ref_thin_k(w, CoP, 0)
        main_b = ref_thin_n(w, Co, 1) if valu(Co) else regular(False)
        tail_f = ref_trow(w, 0).view(torch.int32) if (trow_f and x3) else None
        tail_b = ref_npack(w, 1).view(torch.int32) if (npack_b and x3) else None
    elif thin_out:
        main_f = ref_thin_n(w, Ci, 0) if valu(Ci) else regular(True)
        main_b = ref_thin_k(w, CiP, 1)
        tail_f = ref_npack(w, 0).view(torch.int32) if (npack_f and x3) else None
        tail_b = ref_trow(w, 1).view(torch.int32) if (trow_b and x3) else None
    else:
        main_f, main_b, tail_f, tail_b = regular(True), regular(False), None, None

    def lay(n, main, tail_words, regular_elems):
        buf = torch.full((n,), SENTINEL, dtype=torch.int32)
        assert main.numel() <= regular_elems
        buf[:main.numel()] = main
        if tail_words is not None:
            assert regular_elems + tail_words.numel() == n
            buf[regular_elems:] = tail_words
        return buf
    return lay(n_wf, main_f, tail_f, wf_regular), lay(n_wb, main_b, tail_b, wb_regular)


# ------------------------------------------------------------------------------------------------------------------------
def _sentinel_buf(n):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")


def _pack_one(w, Ci, Co, want_wf=True, want_wb=True):
    """acg_pack_conv_weight into sentinel-filled buffers -> (wf, wb) int32 bit patterns on the CPU"""
    from dtgan_amd import _lib, ops
    Or, Ir, K, _ = w.shape
    wf = _sentinel_buf(int(_lib.query("acg_packed_wf_elems", K, Ci, Co)))
    wb = _sentinel_buf(int(_lib.query("acg_packed_wb_elems", K, Ci, Co)))
    wd = w.cuda().contiguous()
    _lib.call("acg_pack_conv_weight", ops._ptr(wd), Or, Ir, K, Ci, Co, ops._ptr(wf) if want_wf else None,
              ops._ptr(wb) if want_wb else None, ops._stream())
    torch.cuda.synchronize()
    return wf.cpu(), wb.cpu()


def _same(got, exp, what):
    bad = torch.nonzero(got != exp).reshape(-1)
    assert bad.numel() == 0, "%s: %d of %d words differ, first at %d: got %#x, expected %#x" % (
        what, bad.numel(), exp.numel(), int(bad[0]), int(got[bad[0]]) & 0xffffffff, int(exp[bad[0]]) & 0xffffffff)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layer", LAYERS, ids=lambda L: "x".join(map(str, L)))
def test_single_layer_layout(layer, prec, impl):
    Or, Ir, K, Ci, Co = layer
    w = _weights(Or, Ir, K, seed=LAYERS.index(layer))
    with mode(prec, impl):
        exp_f, exp_b = expected(w, Ci, Co, prec, impl)
        got_f, got_b = _pack_one(w, Ci, Co)
    _same(got_f, exp_f, "wf")
    _same(got_b, exp_b, "wb")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layer", [(16, 16, 3, 16, 16), (32, 3, 7, 16, 32)], ids=["regular", "thin"])
def test_null_operand_is_skipped(layer, prec):
    """wf = NULL or wb = NULL: the other buffer is written as before, nothing else is touched"""
    Or, Ir, K, Ci, Co = layer
    w = _weights(Or, Ir, K, seed=11)
    with mode(prec, "mfma"):
        exp_f, exp_b = expected(w, Ci, Co, prec, "mfma")
        got_f, got_b = _pack_one(w, Ci, Co, want_wb=False)
        _same(got_f, exp_f, "wf (wb = NULL)")
        assert bool((got_b == SENTINEL).all())
        got_f, got_b = _pack_one(w, Ci, Co, want_wf=False)
        _same(got_b, exp_b, "wb (wf = NULL)")
        assert bool((got_f == SENTINEL).all())


def _pack_multi(ws, dims):
    from dtgan_amd import _lib, ops
    arr = (_lib.PackItem * len(ws))()
    keep = []
    for i, (w, (Ci, Co)) in enumerate(zip(ws, dims)):
        Or, Ir, K, _ = w.shape
        wd = w.cuda().contiguous()
        wf = _sentinel_buf(int(_lib.query("acg_packed_wf_elems", K, Ci, Co)))
        wb = _sentinel_buf(int(_lib.query("acg_packed_wb_elems", K, Ci, Co)))
        keep.append((wd, wf, wb))
        arr[i].w, arr[i].wf, arr[i].wb = wd.data_ptr(), wf.data_ptr(), wb.data_ptr()
        arr[i].Or, arr[i].Ir, arr[i].K, arr[i].Ci, arr[i].Co = Or, Ir, K, Ci, Co
    _lib.call("acg_pack_conv_weights_multi", arr, len(ws), ops._stream())
    torch.cuda.synchronize()
    return [(wf.cpu(), wb.cpu()) for _, wf, wb in keep]


@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
@pytest.mark.parametrize("which", ["layers", "49_tiny"])
def test_multi_equals_one_by_one(which, prec):
    """acg_pack_conv_weights_multi == the same layers packed one by one; 49 items cross the 48-item table boundary"""
    from dtgan_amd import _lib
    if which == "layers":
        layers = LAYERS
    else:   # K and the real counts vary so that no two neighbours share a size
        layers = [(16 - i % 5, 16 - i % 3, 1 + i % 3, 16, 16 if i % 4 else 32) for i in range(49)]
    with mode(prec, "mfma"):
        layers = [L for L in layers if _lib.query("acg_pack_conv_weights_multi_supported", L[0], L[1], L[2])]
        assert len(layers) == (49 if which == "49_tiny" else 4)
        ws = [_weights(L[0], L[1], L[2], seed=100 + i) for i, L in enumerate(layers)]
        dims = [(L[3], L[4]) for L in layers]
        multi = _pack_multi(ws, dims)
        for i, (w, (Ci, Co)) in enumerate(zip(ws, dims)):
            one_f, one_b = _pack_one(w, Ci, Co)
            _same(multi[i][0], one_f, "item %d wf" % i)
            _same(multi[i][1], one_b, "item %d wb" % i)

