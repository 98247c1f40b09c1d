"""csrc/norm.hip through the C ABI against the fp64 reference of tests/norm_ref.py, variant by variant.

Every template instance the host dispatch can reach (norm_apply_kernel<ACT, HAS_RES, MASK, FMT>, norm_bwd_partial<ACT, MSRC>,
norm_bwd_apply<ACT, MSRC, HAS_DRES, DXS16>) is run on a hand-built shape list that walks the places where the index arithmetic
turns over; the plan is spelled in the test id (tests/norm_cases.py):
    inv<256 % (C/4) == 0>  rp<rows per chunk pass>  idle<idle threads>  nch<chunks of 256 pixels>  eq|chan (branch of
    norm_stats_final)  f4x<float4 per group>  wg<workgroups of the apply pass>  fin<32-channel blocks of the final kernels>
Each case runs statistics -> apply -> backward and compares y, mean, rstd, running statistics, dx, dres, dgamma, dbeta with
fp64; mask bits and pre-split bytes exactly (decoded by the reference's own reader).  Inputs keep every pre-activation
1e-4 away from the activation's kink (asserted in fp64), so that no element is left out of any comparison.  Outputs start
as NaN, every buffer is followed by 64 guard words that must survive (tests/guard_util.py).

Bars: the project's own (tests/test_hip_ops.py: 2e-5 on y, 1e-4 on gradients and statistics, 1e-5 on running statistics)
wherever plain fp32 arithmetic on the same inputs meets them; where it does not, 4x what the fp32 restatement
(norm_ref.forward32 / backward32) needs against fp64 — tiny P (P = 2: dx 1.34e-4 .. 5.75e-4 on the CPU) and the
mean-50 inputs (y 2.3e-5 .. 7.6e-4, rstd up to 1.7e-3, dx up to 8.4e-4 at 70 x 1020).  Pre-split outputs and C = 1020
meet the project's bars on the CPU.  DESIGN_LOG.md lists the CPU figures next to what the kernels need on the MI355X.

On the MI355X the kernels need the same as the fp32 restatement to within a few per cent (P = 2: dx 1.34e-4 .. 5.75e-4;
70 x 1020 at mean 50: y 6.5e-4, rstd 1.7e-3, dx 8.5e-4); at the project's bars the worst case needs y 6.6e-6, dx 5.4e-5,
dgamma 2.8e-5, rstd 6.8e-5.  The P = 1 / P = 2 / P = 3 cases (P <= rows_par: every thread holds one row) are the regression tests of
norm_stats_partial's single-row M2 (rstd was off by 4.5e-3 at P = 1 and 1.9e-4 at P = 2 before).

538 tests, about 6 s on one MI355X (one process; 6.4 s measured for the first 531).
"""
import ctypes

import numpy as np
import pytest

import norm_cases as NC
import norm_ref as R
from guard_util import Buf, rejected

pytestmark = pytest.mark.gpu

EPS = 1e-5
Z, F = ctypes.c_size_t, ctypes.c_float


@pytest.fixture(autouse=True)
def _fresh_buffers():
    Buf.live = []
    yield
    Buf.live = []


def _env():
    from dtgan_amd import _lib, ops
    return _lib, _lib.load(), ops._stream()


def _check(name, got, ref, bars, what=""):
    err = R.rel(got, ref)
    print("%-8s rel err %.2e  bar %.1e  %s" % (name, err, bars[name], what))
    assert np.all(np.isfinite(got)), name
    assert err < bars[name], (name, err, bars[name])


def _affine(c, d):
    """gamma / beta device buffers, their pointers and the row stride"""
    G, C = c["G"], c["C"]
    if c["gs"] == "3C":   # a column block of a (G, 3C) matrix whose other columns are NaN
        bufs = []
        for v in (d["gamma"], d["beta"]):
            m = np.full((G, 3 * C), np.nan, np.float32)
            m[:, C:2 * C] = v
            bufs.append(Buf.of(m))
        return bufs[0].at(C), bufs[1].at(C), 3 * C
    ga, be = Buf.of(d["gamma"]), Buf.of(d["beta"])
    return ga.ptr, be.ptr, (C if c["gs"] == "C" else 0)


def run_case(c):
    _lib, lib, st = _env()
    d = NC.inputs(c)
    f64, b64, cpu, bars = NC.references(c, d)
    G, P, C, act = c["G"], c["P"], c["C"], c["act"]
    n = G * P * C
    x = Buf.of(d["x"])
    wsb = _lib.query("acg_norm_workspace_bytes", G, P, C)
    ws = Buf.out(wsb // 4)
    mean, rstd = Buf.out(G * C), Buf.out(G * C)
    # ---- statistics
    if c["mode"] == 2:
        nreal = c["nreal"] if c["nreal"] is not None else C
        rm, rv = Buf.of(d["mean"][0][:nreal]), Buf.of(d["var"][0][:nreal])
        _lib.call("acg_bn_eval_stats", rm.ptr, rv.ptr, nreal, C, F(EPS), mean.ptr, rstd.ptr, st)
        assert np.all(mean.host()[nreal:] == 0.0)                      # padded channels: exactly zero
        assert np.array_equal(rm.host(), d["mean"][0][:nreal])
    else:
        rmb = rvb = None
        if c["running"]:
            rm0, rv0 = NC.running_init(C)
            rmb, rvb = Buf.of(rm0), Buf.of(rv0)
        _lib.call("acg_norm_stats", x.ptr, G, P, C, F(EPS), c["mode"], mean.ptr, rstd.ptr, rmb.ptr if rmb else None,
                  rvb.ptr if rvb else None, F(0.1), ws.ptr, wsb, st)
        if c["running"]:
            _check("run_mean", rmb.host(), f64["run_mean"], bars)
            _check("run_var", rvb.host(), f64["run_var"], bars)
    _check("mean", mean.host((G, C)), f64["mean"], bars)
    _check("rstd", rstd.host((G, C)), f64["rstd"], bars)
    # ---- apply
    gp, bp, gstride = _affine(c, d)
    res = None
    if c["res"]:
        res = Buf.raw(R.s16_encode(d["res"].reshape(-1))) if c["fmt"] & 1 else Buf.of(d["res"])
    y = Buf.out(n)
    mask = Buf.out(n // 32, np.uint32) if c["mask"] else None
    _lib.call("acg_norm_apply", x.ptr, mean.ptr, rstd.ptr, gp, bp, gstride, res.ptr if res else None, y.ptr,
              mask.ptr if mask else None, G, P, C, act, c["fmt"], st)
    yv = R.s16_decode(y.bytes()).reshape(G, P, C) if c["fmt"] & 2 else y.host((G, P, C))
    _check("y", yv, f64["y"], bars)
    if act in (R.ACT_RELU, R.ACT_LRELU):
        assert np.array_equal(yv > 0, f64["y"] > 0)                    # the margin makes this legitimate
    if mask is not None:
        assert np.array_equal(mask.host(), R.pack_bits(f64["y"] > 0))  # bit for bit
    # ---- backward
    if act != R.ACT_TANH:
        dy = Buf.of(d["dy"])
        ypass = None
        if act != R.ACT_NONE and c["msrc"] == 0:
            ypass = Buf.of(f64["y"]) if c["fmt"] & 2 else y            # a pre-split y is not what the backward reads
        dx = Buf.out(n)
        dres = Buf.out(n) if c["dres"] else None
        shared = c["gs"] == "0"
        npar = C if c["nparam"] is None else c["nparam"]
        if shared:
            pre_g = np.linspace(-1, 1, C).astype(np.float32) if c["accumulate"] else np.full(C, np.nan, np.float32)
            pre_b = np.linspace(2, 3, C).astype(np.float32) if c["accumulate"] else np.full(C, np.nan, np.float32)
            dga, dbe = Buf.of(pre_g), Buf.of(pre_b)
        else:
            dga, dbe = Buf.out(G * C), Buf.out(G * C)
        _lib.call("acg_norm_bwd", dy.ptr, ypass.ptr if ypass else None, mask.ptr if mask else None, x.ptr, mean.ptr, rstd.ptr,
                  gp, bp, gstride, dx.ptr, dres.ptr if dres else None, dga.ptr, dbe.ptr, npar if shared else 0, c["accumulate"],
                  G, P, C, act, c["mode"], 1 if c["dx_s16"] else 0, ws.ptr, wsb, st)
        dxv = R.s16_decode(dx.bytes()).reshape(G, P, C) if c["dx_s16"] else dx.host((G, P, C))
        _check("dx", dxv, b64["dx"], bars)
        if dres is not None:
            _check("dres", dres.host((G, P, C)), b64["dres"], bars)
        if shared:
            for name, buf, pre in (("dgamma", dga, pre_g), ("dbeta", dbe, pre_b)):
                got = buf.host()
                base = pre[:npar].astype(np.float64) if c["accumulate"] else 0.0
                _check(name, got[:npar], b64[name][:npar] + base, bars)
                assert np.array_equal(got[npar:], pre[npar:], equal_nan=True)   # channels past nparam: untouched
        else:
            _check("dgamma", dga.host((G, C)), b64["dgamma"], bars)
            _check("dbeta", dbe.host((G, C)), b64["dbeta"], bars)
    assert np.array_equal(x.host(), d["x"].reshape(-1))
    Buf.check_all()


@pytest.mark.parametrize("c", NC.SHAPE_CASES, ids=NC.case_id)
def test_shape(c):
    run_case(c)


@pytest.mark.parametrize("c", NC.FWD_CASES, ids=NC.case_id)
def test_forward_variant(c):
    run_case(c)


@pytest.mark.parametrize("c", NC.BWD_CASES, ids=NC.case_id)
def test_backward_variant(c):
    run_case(c)


@pytest.mark.parametrize("shape", NC.PARTIAL_STATS, ids=lambda s: "G%d_P%d_C%d_rows%d_nch%d_%s" % (
    s + (-(-s[1] // s[3]), "eq" if s[1] % s[3] == 0 else "chan_last%d" % (s[1] % s[3]))))
@pytest.mark.parametrize("unbiased", [0, 1], ids=["var0", "var1"])
def test_stats_from_partials(shape, unbiased):
    """reference-made (mean, M2) partials per chunk of rows_per_chunk != 256 pixels; the reference merges the same
    fp32-rounded partials in fp64"""
    _lib, lib, st = _env()
    G, P, C, rpc = shape
    rs = np.random.RandomState(P + C + rpc)
    x = rs.normal(0.5, 1.3, (G, P, C)) + rs.normal(0, 1, (G, 1, C))
    nch = -(-P // rpc)
    rows = [min(rpc, P - k * rpc) for k in range(nch)]
    part = np.zeros((G, nch, 2, C), np.float32)
    for k in range(nch):
        ch = x[:, k * rpc:k * rpc + rows[k]]
        part[:, k, 0] = ch.mean(axis=1)
        part[:, k, 1] = ((ch - ch.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)
    m_ref, m2_ref = R.chan_merge_partials(np.moveaxis(part[:, :, 0], 1, 0), np.moveaxis(part[:, :, 1], 1, 0), rows)
    rstd_ref = 1.0 / np.sqrt(m2_ref / (P - 1 if unbiased else P) + EPS)
    pb, mean, rstd = Buf.of(part), Buf.out(G * C), Buf.out(G * C)
    _lib.call("acg_norm_stats_from_partials", pb.ptr, G, P, C, rpc, F(EPS), unbiased, mean.ptr, rstd.ptr, st)
    _check("mean", mean.host((G, C)), m_ref, R.PROJECT_BAR)
    _check("rstd", rstd.host((G, C)), rstd_ref, R.PROJECT_BAR)
    Buf.check_all()


@pytest.mark.parametrize("v", NC.PARTIAL_BWD_CASES, ids=lambda v: "supplied_nch%d_not%d-%s" % (
    v[0], -(-v[1]["P"] // 256), NC.case_id(v[1])))
def test_bwd_from_supplied_partials(v):
    """acg_norm_bwd_partials: S1 / S2 partials made by the reference, in a chunk count of their own"""
    _lib, lib, st = _env()
    nch, c = v
    G, P, C, act = c["G"], c["P"], c["C"], c["act"]
    d = NC.inputs(c)
    f64, b64, cpu, bars = NC.references(c, d)
    edges = np.linspace(0, P, nch + 1).astype(int)
    part = np.zeros((G, nch, 2, C), np.float32)
    for k in range(nch):
        sl = slice(edges[k], edges[k + 1])
        part[:, k, 0] = b64["gy"][:, sl].sum(axis=1)
        part[:, k, 1] = (b64["gy"][:, sl] * f64["xhat"][:, sl]).sum(axis=1)
    wsb = _lib.query("acg_norm_workspace_bytes", G, P, C)
    ws, pb = Buf.out(wsb // 4), Buf.of(part)
    x, dy, mean, rstd = Buf.of(d["x"]), Buf.of(d["dy"]), Buf.of(f64["mean"]), Buf.of(f64["rstd"])
    ga, be = Buf.of(d["gamma"]), Buf.of(d["beta"])
    dx, dga, dbe = Buf.out(G * P * C), Buf.out(C), Buf.out(C)
    _lib.call("acg_norm_bwd_partials", dy.ptr, None, None, x.ptr, mean.ptr, rstd.ptr, ga.ptr, be.ptr, 0, dx.ptr, None, dga.ptr,
              dbe.ptr, C, 0, G, P, C, act, 0, 0, pb.ptr, nch, ws.ptr, wsb, st)
    _check("dx", dx.host((G, P, C)), b64["dx"], bars)
    _check("dgamma", dga.host(), b64["dgamma"], bars)
    _check("dbeta", dbe.host(), b64["dbeta"], bars)
    Buf.check_all()


@pytest.mark.parametrize("c", NC.SYNCBN_CASES, ids=lambda c: "rankP%d_Ptot%d-%s" % (c["P"] // 2, c["P"], NC.case_id(c)))
def test_syncbn_sums_and_apply(c):
    """two ranks of P pixels: acg_norm_bwd_sums per rank, the sums added outside, acg_norm_bwd_apply with Ptot = 2 P"""
    _lib, lib, st = _env()
    P, C, act, unbiased = c["P"] // 2, c["C"], c["act"], c["mode"]
    d = NC.inputs(c)
    f64, b64, ref_halves, cpu, bars = NC.syncbn_references(c, d)
    mean, rstd, ga = Buf.of(f64["mean"]), Buf.of(f64["rstd"]), Buf.of(d["gamma"])
    wsb = _lib.query("acg_norm_workspace_bytes", 1, P, C)
    ws = Buf.out(wsb // 4)
    halves, total = [], np.zeros((2, C), np.float32)
    for h, ref in ref_halves:
        x, dy, y = Buf.of(d["x"][:, h]), Buf.of(d["dy"][:, h]), Buf.of(f64["y"][:, h])
        sums = Buf.out(2 * C)
        _lib.call("acg_norm_bwd_sums", dy.ptr, y.ptr, x.ptr, mean.ptr, rstd.ptr, sums.ptr, 1, P, C, act, ws.ptr, wsb, st)
        s = sums.host((2, C))
        _check("S1", s[0], ref[0], bars)      # this rank's dbeta and dgamma
        _check("S2", s[1], ref[1], bars)
        total += s
        halves.append((x, dy, y, h))
    sb = Buf.of(total)
    for x, dy, y, h in halves:
        dx, dres = Buf.out(P * C), Buf.out(P * C)
        _lib.call("acg_norm_bwd_apply", dy.ptr, y.ptr, x.ptr, mean.ptr, rstd.ptr, ga.ptr, 0, sb.ptr, dx.ptr, dres.ptr, 1, P, 2 * P,
                  C, act, unbiased, st)
        _check("dx", dx.host((1, P, C)), b64["dx"][:, h], bars)
        _check("dres", dres.host((1, P, C)), b64["dres"][:, h], bars)
    Buf.check_all()


def test_rejected_combinations_return_an_error_without_a_launch():
    _lib, lib, st = _env()
    G, P, C = 2, 64, 16
    n = G * P * C
    x, mean, rstd, ga, be, res = (Buf.of(np.ones(k, np.float32)) for k in (n, G * C, G * C, C, C, n))
    y, dx, dres, dga, dbe, mask = Buf.out(n), Buf.out(n), Buf.out(n), Buf.out(C), Buf.out(C), Buf.out(n // 32, np.uint32)
    big = Buf.of(np.ones(1028 * 4, np.float32))
    wsb = 1 << 20
    ws = Buf.out(wsb // 4)

    def apply(act=R.ACT_RELU, fmt=0, gstride=0, r=res, m=None, G=G, P=P, C=C, xx=x):
        return rejected(lib, "acg_norm_apply", xx.ptr, mean.ptr, rstd.ptr, ga.ptr, be.ptr, gstride, r.ptr if r else None, y.ptr,
                        m.ptr if m else None, G, Z(P), C, act, fmt, st)

    assert "sigmoid" in apply(act=4)
    for fmt in (1, 2, 3):
        assert "pre-split" in apply(act=R.ACT_LRELU, fmt=fmt)          # fmt without ReLU
        assert "pre-split" in apply(act=R.ACT_NONE, fmt=fmt)
    assert "pre-split" in apply(fmt=1, r=None) and "pre-split" in apply(fmt=3, r=None)
    assert "pre-split" in apply(fmt=4) and "pre-split" in apply(fmt=2, C=12, P=64)
    assert "bitmask" in apply(r=None, m=mask)                          # the bitmask without a residual
    assert "bitmask" in apply(act=R.ACT_TANH, m=mask) and "bitmask" in apply(act=R.ACT_NONE, m=mask)
    assert "bitmask" in apply(m=mask, P=63)                            # 63 * 4 float4: just outside P*C/4 % 8 == 0
    assert "gstride" in apply(gstride=12) and "gstride" in apply(gstride=18)
    assert "bad shape" in apply(C=1028, P=1, G=1, xx=big)              # C > 1024
    assert "bad shape" in apply(C=18) and "bad shape" in apply(G=0) and "bad shape" in apply(P=0)

    def bwd(act=R.ACT_RELU, yy=y, m=None, gstride=0, dr=None, nparam=C, acc=0, C=C, P=P, unb=0, s16=0, w=wsb, beta=be, name="acg_norm_bwd"):
        a = [x.ptr, yy.ptr if yy else None, m.ptr if m else None, x.ptr, mean.ptr, rstd.ptr, ga.ptr, beta.ptr if beta else None,
             gstride, dx.ptr, dr.ptr if dr else None, dga.ptr, dbe.ptr, nparam, acc, G, Z(P), C, act, unb, s16]
        if name == "acg_norm_bwd_partials":
            a += [None, 3]
        return rejected(lib, name, *(a + [ws.ptr, Z(w), st]))

    assert ": act 3" in bwd(act=R.ACT_TANH) and ": act 4" in bwd(act=4)         # tanh / sigmoid in the backward
    assert "pre-split dx" in bwd(s16=1, yy=None, dr=dres)               # dx_s16 with dres
    assert "pre-split dx" in bwd(s16=1, yy=None, act=R.ACT_LRELU)
    assert "pre-split dx" in bwd(s16=1, yy=y)                           # needs the bitmask or the recomputed mask
    assert "pre-split dx" in bwd(s16=1, yy=None, C=12)
    assert "accumulate" in bwd(acc=1, gstride=C)
    assert "nparam" in bwd(nparam=C + 1) and "nparam" in bwd(nparam=-1)
    assert "gstride" in bwd(gstride=12) and "gstride" in bwd(gstride=18)
    assert "bad shape" in bwd(C=1028, P=1)
    assert "required" in bwd(yy=None, beta=None)
    assert "bitmask" in bwd(yy=None, m=mask, P=63)
    assert "partial" in bwd(name="acg_norm_bwd_partials")
    rc = lib.acg_norm_bwd(x.ptr, y.ptr, None, x.ptr, mean.ptr, rstd.ptr, ga.ptr, be.ptr, 0, dx.ptr, None, dga.ptr, dbe.ptr, C, 0, G,
                          Z(P), C, R.ACT_RELU, 0, 0, ws.ptr, Z(16), st)
    assert rc == -2 and b"workspace" in lib.acg_last_error()
    assert "unbiased" in rejected(lib, "acg_norm_stats", x.ptr, G, Z(1), C, F(EPS), 1, mean.ptr, rstd.ptr, None, None, F(0.1), ws.ptr, Z(wsb), st)
    assert "G == 1" in rejected(lib, "acg_norm_stats", x.ptr, G, Z(P), C, F(EPS), 0, mean.ptr, rstd.ptr, ga.ptr, be.ptr, F(0.1), ws.ptr, Z(wsb), st)
    assert "unbiased" in rejected(lib, "acg_norm_stats_from_partials", x.ptr, G, Z(1), C, 128, F(EPS), 1, mean.ptr, rstd.ptr, st)
    assert "partials" in rejected(lib, "acg_norm_stats_from_partials", x.ptr, G, Z(P), C, 0, F(EPS), 0, mean.ptr, rstd.ptr, st)
    assert "bad dims" in rejected(lib, "acg_bn_eval_stats", ga.ptr, be.ptr, 16, 12, F(EPS), mean.ptr, rstd.ptr, st)
    # nothing was launched: every output is still poisoned, every input intact
    for b in (y, dx, dres, dga, dbe, ws):
        assert np.all(np.isnan(b.host()))
    assert np.all(mask.host() == 0xFFFFFFFF)
    assert np.all(x.host() == 1.0) and np.all(mean.host() == 1.0)
    Buf.check_all()
