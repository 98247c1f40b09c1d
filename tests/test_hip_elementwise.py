"""csrc/elementwise.hip (and the mask kernels of csrc/norm.hip) through the C ABI against fp64 numpy, at the sizes where
the launch arithmetic turns over:
    ew_blocks caps a grid at 4096 x 256 threads: the second grid-stride trip starts at element 1 048 576 ("trip2" in an id);
    reduce_launch takes ceil(total / 2048) blocks, capped at RED_BLOCKS = 1024 (nb in the id), reduce_final_kernel loops when
    nb > 256 ("finloop"); mask_apply_kernel caps at 8192 blocks ("cap8192"); linear_bwd_dx_kernel is chosen when I <= 256 and
    O >= 32 and splits O over 256 / I chunks ("dxwg<chunks>" against "dxflat"); the multi-tensor Adam builds two per-group block
    tables (S.first of the sums pass, A.first of the update pass).
Outputs start as NaN, every buffer ends in 64 guard words (tests/guard_util.py), padded channels the contract writes as zero
must be exactly zero, padded inputs hold NaN / 1e30 so that a kernel which reads them fails.

Bars (tests/test_hip_ops.py::test_losses_and_optimizer / test_linear_and_spatial_mean): reductions 1e-5 — relative to the sum
of the absolute terms, not to the result (the mean of zero-mean data is otherwise ill-conditioned); loss gradients rtol 1e-5;
Adam: parameters 2e-7 absolute (parameters within (-1, 1): half an ulp per step is 3e-8), clipped gradients rtol 1e-5,
gradient norm 1e-4; dense layers and spatial means 1e-5 of the largest value.  Copies, masks, layout changes and the
device-side step counter are exact.

Measured on the MI355X: reductions 1.2e-7 of the sum of absolute terms, Adam parameters 1.0e-7, min-max scaling 2.4e-7
(bar 2e-6: a few fp32 roundings inside [-1, 1]; its plane with both infinities is the regression test of the overflow of
max - min in minmax_scale_kernel).

143 tests, 7.0 s on one MI355X (one process).
"""
import ctypes

import numpy as np
import pytest

from guard_util import Buf, rejected

pytestmark = pytest.mark.gpu

F = ctypes.c_float
GRID_TRIP = 4096 * 256          # elements of one grid-stride trip at the block cap
RED_BLOCKS = 1024


@pytest.fixture(autouse=True)
def _fresh_buffers():
    Buf.live = []
    yield
    Buf.live = []


def _env():
    from dtgan_amd import _lib, ops
    return _lib, _lib.load(), ops._stream()


def _garbage(a, C):
    """padded channels (last axis) hold NaN and 1e30 alternately"""
    if a.shape[-1] > C:
        pad = a[..., C:]
        pad[...] = 1e30
        pad.reshape(-1)[::2] = np.nan
    return a


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


# ---------------------------------------------------------------- reductions
def _red_id(v):
    total, C, Cp = v
    nb = min(RED_BLOCKS, max(1, -(-total // 2048)))
    return "total%d_nb%d%s%s_C%dof%d" % (total, nb, "_finloop" if nb > 256 else "", "_capped" if total > RED_BLOCKS * 2048 else "", C, Cp)


# exact totals with one channel; with Cp = 16 the pixel counts that put total = npix * 16 on both sides of the same block counts
_TOT1 = [1, 2047, 2048, 2049, 256 * 2048 - 1, 256 * 2048 + 1, 1024 * 2048 - 1, 1024 * 2048 + 1, 5000001]
_PIX16 = [1, 127, 128, 129, 256 * 128 - 1, 256 * 128 + 1, 1024 * 128 - 1, 1024 * 128 + 1, 312501]
RED_CASES = [(t, 1, 1) for t in _TOT1] + [(p * 16, C, 16) for p in _PIX16 for C in (1, 3, 16)]


def _bce64(p, t):
    with np.errstate(divide="ignore"):
        lp, lq = np.maximum(np.log(p), -100.0), np.maximum(np.log1p(-p), -100.0)
    return (t - 1.0) * lq - t * lp


@pytest.mark.parametrize("v", RED_CASES, ids=_red_id)
def test_loss_reductions_and_their_gradients(v):
    _lib, lib, st = _env()
    total, C, Cp = v
    npix = total // Cp
    rs = np.random.RandomState(total % 100003 + C)
    a = _garbage(rs.normal(0, 1, (npix, Cp)).astype(np.float32), C)
    b = _garbage(rs.normal(0, 1, (npix, Cp)).astype(np.float32), C)
    b[::7, :C] = a[::7, :C]                                   # ties: sign(0) = 0 in the L1 gradient
    p = rs.uniform(0, 1, (npix, Cp)).astype(np.float32)
    p[::11, 0] = 0.0
    p[5::13, 0] = 1.0                                         # both logarithms reach their clamp at -100
    p = _garbage(p, C)
    flat = rs.normal(0, 1, total).astype(np.float32)
    target = [1.0, 0.0, 0.9][total % 3]
    A, B, Pb, Fl = Buf.of(a), Buf.of(b), Buf.of(p), Buf.of(flat)
    wsb = _lib.query("acg_reduce_workspace_bytes", total)
    assert wsb == RED_BLOCKS * 4
    ws = Buf.out(wsb // 4)
    a64, b64, p64 = (z[:, :C].astype(np.float64) for z in (a, b, p))
    cnt = float(npix * C)
    t32 = float(np.float32(target))
    refs = {
        "acg_mse_const_fwd": ((a64 - t32) ** 2, lambda o: _lib.call("acg_mse_const_fwd", A.ptr, npix, C, Cp, F(target), o.ptr, ws.ptr, wsb, st), 1 / cnt),
        "acg_bce_const_fwd": (_bce64(p64, t32), lambda o: _lib.call("acg_bce_const_fwd", Pb.ptr, npix, C, Cp, F(target), o.ptr, ws.ptr, wsb, st), 1 / cnt),
        "acg_l1_fwd": (np.abs(a64 - b64), lambda o: _lib.call("acg_l1_fwd", A.ptr, B.ptr, npix, C, Cp, o.ptr, ws.ptr, wsb, st), 1 / cnt),
        "acg_mean_fwd": (a64, lambda o: _lib.call("acg_mean_fwd", A.ptr, npix, C, Cp, o.ptr, ws.ptr, wsb, st), 1 / cnt),
        "acg_sumsq": (flat.astype(np.float64) ** 2, lambda o: _lib.call("acg_sumsq", Fl.ptr, total, o.ptr, ws.ptr, wsb, st), 1.0),
    }
    for name, (terms, run, scale) in refs.items():
        out = Buf.out(1)
        run(out)
        got = float(out.host()[0])
        err = abs(got - terms.sum() * scale) / max(np.abs(terms).sum() * scale, 1e-30)
        print("%-18s %.6e  err / sum|terms| %.2e" % (name, got, err))
        assert err < 1e-5, (name, got, terms.sum() * scale)
    # gradients: pads exactly zero, the rest to rtol 1e-5
    gout = Buf.of(np.array([0.5], np.float32))
    pad = np.zeros((npix, Cp))
    dp = Buf.out(total)
    _lib.call("acg_mse_const_bwd", A.ptr, npix, C, Cp, F(target), gout.ptr, dp.ptr, st)
    ref = pad.copy(); ref[:, :C] = 0.5 * 2.0 / cnt * (a64 - t32)
    got = dp.host((npix, Cp))
    assert np.all(got[:, C:] == 0.0) and np.allclose(got, ref, rtol=1e-5, atol=0)
    dp = Buf.out(total)
    _lib.call("acg_bce_const_bwd", Pb.ptr, npix, C, Cp, F(target), gout.ptr, dp.ptr, st)
    ref = pad.copy(); ref[:, :C] = 0.5 / cnt * (p64 - t32) / np.maximum(p64 * (1 - p64), float(np.float32(1e-12)))
    got = dp.host((npix, Cp))
    assert np.all(got[:, C:] == 0.0) and np.allclose(got, ref, rtol=1e-5, atol=0)
    ref = pad.copy(); ref[:, :C] = 0.5 / cnt * np.sign(a64 - b64)
    assert (ref[::7, :C] == 0).all()
    for use_a, use_b in ((True, True),) + (((True, False), (False, True)) if total < 100000 else ()):
        da, db = Buf.out(total) if use_a else None, Buf.out(total) if use_b else None
        _lib.call("acg_l1_bwd", A.ptr, B.ptr, npix, C, Cp, gout.ptr, da.ptr if da else None, db.ptr if db else None, st)
        if da:
            got = da.host((npix, Cp))
            assert np.all(got[:, C:] == 0.0) and np.all(got[::7, :C] == 0.0) and np.allclose(got, ref, rtol=1e-6, atol=0)
        if db:
            got = db.host((npix, Cp))
            assert np.all(got[:, C:] == 0.0) and np.allclose(got, -ref, rtol=1e-6, atol=0)
    rc = lib.acg_sumsq(Fl.ptr, total, gout.ptr, ws.ptr, 16, st)
    assert rc == -2 and b"workspace" in lib.acg_last_error()
    Buf.check_all()


# ---------------------------------------------------------------- Adam
ADAM_SIZES = [1, 255, 256, 257, 2048, 2049, GRID_TRIP + 3]
HYP = dict(max_norm=50.0, lr=2e-4, b1=0.5, b2=0.999, eps=1e-8)


def _adam64(st, g, step):
    """fp64 clip_grad_norm + Adam on the fp32 hyper-parameters the kernels receive"""
    f = lambda k: float(np.float32(HYP[k]))
    ss = float((g ** 2).sum())
    coef = min(1.0, f("max_norm") / (np.sqrt(ss) + float(np.float32(1e-6))))
    g = g * coef
    st["m"] = f("b1") * st["m"] + (1 - f("b1")) * g
    st["v"] = f("b2") * st["v"] + (1 - f("b2")) * g * g
    bc1, bc2 = 1 - f("b1") ** step, 1 - f("b2") ** step
    st["p"] = st["p"] - (f("lr") / bc1) * st["m"] / (np.sqrt(st["v"]) / np.sqrt(bc2) + f("eps"))
    return ss, g


@pytest.mark.parametrize("sizes", [[s] for s in ADAM_SIZES] + [ADAM_SIZES + [4099]],
                         ids=lambda s: "n%d_%s" % (s[0], "trip2" if s[0] > GRID_TRIP else "trip1") if len(s) == 1 else "max_groups8_Sfirst_Afirst")
def test_adam_against_fp64_and_the_device_step_counter(sizes):
    """acg_clip_adam_multi with the host step (set A), with step_dev (set B) and acg_sumsq + acg_adam_step per group (set C):
    A against the fp64 Adam over two steps, clipping active in one of them and not in the other; B and C bit-identical to A"""
    _lib, lib, st = _env()
    ng = len(sizes)
    assert ng <= _lib.ADAM_MAX_GROUPS
    rs = np.random.RandomState(sizes[0] + ng)
    p0 = [rs.uniform(-1, 1, n).astype(np.float32) for n in sizes]
    ref = [dict(p=p.astype(np.float64), m=np.zeros(n), v=np.zeros(n)) for p, n in zip(p0, sizes)]
    sets = []
    for _ in range(3):
        sets.append([dict(p=Buf.of(p), g=Buf.out(n), m=Buf.of(np.zeros(n, np.float32)), v=Buf.of(np.zeros(n, np.float32)),
                          ss=Buf.out(1)) for p, n in zip(p0, sizes)])
    wsb = _lib.query("acg_clip_adam_multi_workspace_bytes", ng)
    ws, rws = Buf.out(wsb // 4), Buf.out(RED_BLOCKS)
    step_dev = Buf.of(np.zeros(1, np.int32), np.int32)
    h = HYP

    def multi(S, step, sd):
        arr = (_lib.AdamGroup * ng)()
        for i, q in enumerate(S):
            arr[i].p, arr[i].g, arr[i].m, arr[i].v, arr[i].n, arr[i].sumsq = (q["p"].ptr.value, q["g"].ptr.value, q["m"].ptr.value,
                                                                              q["v"].ptr.value, sizes[i], q["ss"].ptr.value)
        _lib.call("acg_clip_adam_multi", arr, ng, F(h["max_norm"]), F(h["lr"]), F(h["b1"]), F(h["b2"]), F(h["eps"]), step,
                  sd.ptr if sd else None, ws.ptr, wsb, st)

    for step in (1, 2):
        # gradient norms of 3 x and 0.1 x max_norm, alternating over groups and steps: the clip is active in one, not in the other
        grads = []
        for i, n in enumerate(sizes):
            g = rs.normal(0, 1, n)
            g *= h["max_norm"] * (3.0 if (i + step) % 2 == 0 else 0.1) / np.sqrt((g ** 2).sum())
            grads.append(g.astype(np.float32))
        for S in sets:
            for q, g in zip(S, grads):
                q["g"].put(g)
        multi(sets[0], step, None)
        step_dev.put(np.array([step - 1], np.int32))              # the number of COMPLETED steps
        multi(sets[1], 0, step_dev)
        for q, n in zip(sets[2], sizes):
            _lib.call("acg_sumsq", q["g"].ptr, n, q["ss"].ptr, rws.ptr, RED_BLOCKS * 4, st)
        for q, n in zip(sets[2], sizes):
            _lib.call("acg_adam_step", q["p"].ptr, q["g"].ptr, q["m"].ptr, q["v"].ptr, n, q["ss"].ptr, F(h["max_norm"]), F(h["lr"]),
                      F(h["b1"]), F(h["b2"]), F(h["eps"]), step, 1, st)
        for i, n in enumerate(sizes):
            ss, gc = _adam64(ref[i], grads[i].astype(np.float64), step)
            clipped = np.sqrt(ss) > h["max_norm"]
            assert clipped == ((i + step) % 2 == 0)
            got = {k: sets[0][i][k].host() for k in ("p", "g", "m", "v", "ss")}
            assert abs(np.sqrt(float(got["ss"][0])) - np.sqrt(ss)) < 1e-4 * np.sqrt(ss)
            perr = float(np.max(np.abs(got["p"] - ref[i]["p"])))
            print("step %d group %d n=%d clipped=%d  max |p - p64| %.2e" % (step, i, n, clipped, perr))
            assert perr < 2e-7
            assert np.allclose(got["g"], gc, rtol=1e-5, atol=1e-8)
            assert rel(got["m"], ref[i]["m"]) < 1e-5 and rel(got["v"], ref[i]["v"]) < 1e-5
            for other, what in ((sets[1], "step_dev"), (sets[2], "per-group calls")):
                for k in ("p", "g", "m", "v", "ss"):
                    assert np.array_equal(other[i][k].host(), got[k]), (what, k, i)
    arr = (_lib.AdamGroup * 9)()
    assert "groups" in rejected(lib, "acg_clip_adam_multi", arr, 9, F(50), F(2e-4), F(0.5), F(0.999), F(1e-8), 1, None, ws.ptr, wsb, st)
    assert "step" in rejected(lib, "acg_clip_adam_multi", arr, 1, F(50), F(2e-4), F(0.5), F(0.999), F(1e-8), 0, None, ws.ptr, wsb, st)
    Buf.check_all()


# ---------------------------------------------------------------- layout
@pytest.mark.parametrize("dims", [(1, 1, 1, 1, 16), (2, 3, 3, 5, 16), (3, 16, 7, 9, 16), (2, 17, 4, 4, 32), (1, 1, 300, 300, 16),
                                  (2, 3, 200, 200, 16), (1, 16, 260, 260, 16), (2, 17, 150, 150, 32)],
                         ids=lambda d: "N%d_C%d_%dx%d_Cp%d_%s" % (d + ("trip2" if d[0] * d[2] * d[3] * d[4] > GRID_TRIP else "trip1",)))
def test_nchw_nhwc_layout_changes(dims):
    _lib, lib, st = _env()
    N, C, H, W, Cp = dims
    rs = np.random.RandomState(C + H)
    src = rs.normal(0, 1, (N, C, H, W)).astype(np.float32)
    s, d = Buf.of(src), Buf.out(N * H * W * Cp)
    _lib.call("acg_nchw_to_nhwc16", s.ptr, d.ptr, N, C, H, W, Cp, st)
    ref = np.zeros((N, H, W, Cp), np.float32)
    ref[..., :C] = src.transpose(0, 2, 3, 1)
    got = d.host((N, H, W, Cp))
    assert np.array_equal(got, ref) and np.all(got[..., C:] == 0.0)
    back = Buf.out(N * C * H * W)
    _lib.call("acg_nhwc16_to_nchw", d.ptr, back.ptr, N, C, H, W, Cp, st)
    assert np.array_equal(back.host((N, C, H, W)), src)                      # round trip
    g = Buf.of(_garbage(ref.copy(), C))                                      # padded channels of the source are never read
    back = Buf.out(N * C * H * W)
    _lib.call("acg_nhwc16_to_nchw", g.ptr, back.ptr, N, C, H, W, Cp, st)
    assert np.array_equal(back.host((N, C, H, W)), src)
    if Cp > C:
        assert "Cp" in rejected(lib, "acg_nchw_to_nhwc16", s.ptr, d.ptr, N, Cp + 1, H, W, Cp, st)
        assert "Cp" in rejected(lib, "acg_nhwc16_to_nchw", d.ptr, back.ptr, N, Cp + 1, H, W, Cp, st)
    Buf.check_all()


@pytest.mark.parametrize("dims", [(5, 3, 16, 4, 32, 16), (33, 3, 16, 8, 32, 16), (257, 16, 16, 5, 32, 48), (9, 20, 32, 3, 16, 32),
                                  (70001, 3, 16, 8, 32, 16), (40000, 16, 16, 5, 32, 48)],
                         ids=lambda d: "npix%d_a%dof%d_b%dof%d_dst%d_%s" % (d + ("trip2" if d[0] * d[5] > GRID_TRIP else "trip1",)))
def test_concat_and_split_channels(dims):
    _lib, lib, st = _env()
    npix, Ca, Cap, Cb, Cbp, Cdp = dims
    assert Ca + Cb < Cdp and Cap != Cbp
    rs = np.random.RandomState(npix % 1000 + Cdp)
    a = _garbage(rs.normal(0, 1, (npix, Cap)).astype(np.float32), Ca)
    b = _garbage(rs.normal(0, 1, (npix, Cbp)).astype(np.float32), Cb)
    A, B, D = Buf.of(a), Buf.of(b), Buf.out(npix * Cdp)
    _lib.call("acg_concat_channels", A.ptr, Ca, Cap, B.ptr, Cb, Cbp, D.ptr, Cdp, npix, st)
    ref = np.zeros((npix, Cdp), np.float32)
    ref[:, :Ca], ref[:, Ca:Ca + Cb] = a[:, :Ca], b[:, :Cb]
    got = D.host((npix, Cdp))
    assert np.array_equal(got, ref) and np.all(got[:, Ca + Cb:] == 0.0)
    g = rs.normal(0, 1, (npix, Cdp)).astype(np.float32)
    g[:, Ca + Cb:] = np.nan                                                  # never read
    Gd = Buf.of(g)
    ra, rb = np.zeros((npix, Cap), np.float32), np.zeros((npix, Cbp), np.float32)
    ra[:, :Ca], rb[:, :Cb] = g[:, :Ca], g[:, Ca:Ca + Cb]
    for use_a, use_b in ((True, True), (True, False), (False, True)):
        ga, gb = Buf.out(npix * Cap) if use_a else None, Buf.out(npix * Cbp) if use_b else None
        _lib.call("acg_split_channels", Gd.ptr, Cdp, ga.ptr if ga else None, Ca, Cap, gb.ptr if gb else None, Cb, Cbp, npix, st)
        if ga:
            assert np.array_equal(ga.host((npix, Cap)), ra)
        if gb:
            assert np.array_equal(gb.host((npix, Cbp)), rb)
    assert rejected(lib, "acg_concat_channels", A.ptr, Ca, Cap, B.ptr, Cdp, Cbp, D.ptr, Cdp, npix, st)
    assert rejected(lib, "acg_split_channels", Gd.ptr, Cdp, None, Ca, Cap, None, Cdp, Cbp, npix, st)
    Buf.check_all()


@pytest.mark.parametrize("hw", [(1, 1), (1, 255), (16, 16), (1, 257), (17, 241)], ids=lambda s: "HW%d" % (s[0] * s[1]))
def test_minmax_scale_against_the_host_data_path(hw):
    """raw (N, H, W, Craw) with NaN, +-inf and a constant plane -> dataloader.prepare (nan_to_num, min-max in fp64)"""
    _lib, lib, st = _env()
    from dtgan_amd import dataloader
    H, W = hw
    N, Craw, C = 4, 5, 3
    rs = np.random.RandomState(H * W)
    raw = (rs.normal(3, 2, (N, H, W, Craw)) * rs.uniform(0.1, 100, (N, 1, 1, Craw))).astype(np.float32)
    raw[..., 3:] = np.nan                                       # channels past C: never read
    raw[1, :, :, 1] = 7.25                                      # a constant plane -> 0
    flat = raw.reshape(N, H * W, Craw)
    if H * W > 1:
        flat[0, 0, 0] = np.nan                                  # NaN -> 0, which is then the plane's minimum or not
        flat[2, (H * W) // 2, 2] = np.nan
        flat[0, H * W - 1, 1] = np.inf                          # +-inf -> +-FLT_MAX
        flat[2, 1, 0] = -np.inf
    if H * W > 3:
        flat[3, 0, 0], flat[3, H * W - 1, 0] = np.inf, -np.inf  # both in one plane: max - min overflows fp32
    with np.errstate(over="ignore"):
        ref = dataloader.prepare(raw[..., :C].copy())
    r, o = Buf.of(raw), Buf.out(N * C * H * W)
    _lib.call("acg_minmax_scale_nhwc_to_nchw", r.ptr, o.ptr, N, H, W, Craw, C, st)
    got = o.host((N, C, H, W))
    assert np.all(np.isfinite(got)) and np.all(got[1, 1] == 0.0)
    err = float(np.max(np.abs(got - ref)))
    print("max abs err %.2e" % err)
    assert err < 2e-6                                           # values within [-1, 1]: a few fp32 roundings of 6e-8 each
    if H * W > 3:   # both infinities in one plane: +1, -1, and every finite value half way
        assert abs(got[3, 0].reshape(-1)[0] - 1.0) < 2e-6 and abs(got[3, 0].reshape(-1)[-1] + 1.0) < 2e-6
        assert np.all(np.abs(got[3, 0].reshape(-1)[1:-1]) < 2e-6)
    assert "bad arguments" in rejected(lib, "acg_minmax_scale_nhwc_to_nchw", r.ptr, o.ptr, N, H, W, Craw, Craw + 1, st)
    Buf.check_all()


# ---------------------------------------------------------------- masks and activation backward
MASK_CAP = 8192 * 256 * 4          # floats of one grid-stride trip of mask_apply_kernel at its block cap


def _unpack(words, n):
    w = np.asarray(words, np.uint32).reshape(-1, 1)
    return ((w >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)[:n].astype(bool)


@pytest.mark.parametrize("n", [4, 32, 1020, 8192 * 256 * 4 - 4, MASK_CAP + 4100],
                         ids=lambda n: "n%d_%s" % (n, "cap8192_trip2" if n > MASK_CAP else "trip1"))
def test_mask_and_dropout_apply_are_exact(n):
    _lib, lib, st = _env()
    rs = np.random.RandomState(n % 9973)
    x = rs.normal(0, 1, n).astype(np.float32)
    words = rs.randint(0, 2 ** 32, -(-n // 32), dtype=np.uint64).astype(np.uint32)
    keep = _unpack(words, n)
    X, M = Buf.of(x), Buf.of(words, np.uint32)
    out = Buf.out(n)
    _lib.call("acg_mask_apply", X.ptr, M.ptr, out.ptr, n, st)
    assert np.array_equal(out.host(), np.where(keep, x, np.float32(0)))
    out = Buf.out(n)
    _lib.call("acg_dropout_apply", X.ptr, M.ptr, F(2.0), out.ptr, n, st)
    assert np.array_equal(out.host(), np.where(keep, x * np.float32(2), np.float32(0)))
    assert rejected(lib, "acg_mask_apply", X.ptr, M.ptr, out.ptr, n + 2, st)
    assert rejected(lib, "acg_dropout_apply", X.ptr, M.ptr, F(0.0), out.ptr, n, st)
    Buf.check_all()


@pytest.mark.parametrize("act", [0, 1, 2, 3, 4], ids=["none", "relu", "lrelu", "tanh", "sigmoid"])
@pytest.mark.parametrize("n", [4, 1020, 4 * GRID_TRIP + 1028], ids=lambda n: "n%d_%s" % (n, "trip2" if n > 4 * GRID_TRIP else "trip1"))
def test_act_bwd(n, act):
    _lib, lib, st = _env()
    rs = np.random.RandomState(n % 9973 + act)
    dy = rs.normal(0, 1, n).astype(np.float32)
    pre = rs.normal(0, 1.5, n)
    y = {0: pre, 1: np.maximum(pre, 0), 2: np.where(pre > 0, pre, 0.2 * pre), 3: np.tanh(pre), 4: 1 / (1 + np.exp(-pre))}[act].astype(np.float32)
    y64 = y.astype(np.float64)
    grad = {0: np.ones(n), 1: (y64 > 0) * 1.0, 2: np.where(y64 > 0, 1.0, float(np.float32(0.2))), 3: 1 - y64 * y64, 4: y64 * (1 - y64)}[act]
    D, Y, out = Buf.of(dy), Buf.of(y), Buf.out(n)
    _lib.call("acg_act_bwd", D.ptr, Y.ptr, out.ptr, n, act, st)
    got = out.host()
    # two fp32 roundings (1 - y*y, the product); 1 - y*y cancels near |y| = 1: bound the error by the terms, not the result
    assert np.all(np.abs(got - dy * grad) <= 3e-7 * np.abs(dy) * (1 + y64 * y64))
    assert rejected(lib, "acg_act_bwd", D.ptr, Y.ptr, out.ptr, n + 1, act, st)
    Buf.check_all()


# ---------------------------------------------------------------- small dense layers
def _act64(pre, act):
    return {0: pre, 1: np.maximum(pre, 0), 2: np.where(pre > 0, pre, float(np.float32(0.2)) * pre), 3: np.tanh(pre), 4: 1 / (1 + np.exp(-pre))}[act]


def _grad64(y, act):
    return {0: np.ones_like(y), 1: (y > 0) * 1.0, 2: np.where(y > 0, 1.0, float(np.float32(0.2))), 3: 1 - y * y, 4: y * (1 - y)}[act]


def _lin_id(v):
    N, I, O, act = v
    kern = "dxwg%d" % (256 // I) if (I <= 256 and O >= 32) else "dxflat"
    return "N%d_I%d_O%d_%s_%s" % (N, I, O, ["none", "relu", "lrelu", "tanh", "sigmoid"][act], kern)


LIN_CASES = [(N, I, O, (I + O + N) % 5) for O in (31, 32) for I in (1, 5, 6, 48, 200, 256, 257) for N in (1, 7)] + \
            [(3, 48, 32, a) for a in range(5)] + [(3, 6, 31, a) for a in range(5)] + [(33, 16, 200, 1), (2, 300, 128, 2)]


@pytest.mark.parametrize("v", LIN_CASES, ids=_lin_id)
def test_linear_fwd_bwd_around_the_kernel_choice(v):
    _lib, lib, st = _env()
    N, I, O, act = v
    ldx, Op = I + 3, (O + 16) // 16 * 16          # ldx > I, Op > O
    rs = np.random.RandomState(I * 7 + O + act)
    x = rs.normal(0, 1, (N, ldx)).astype(np.float32)
    x[:, I:] = np.nan                              # beyond I: never read
    w, b = rs.normal(0, 0.5, (O, I)).astype(np.float32), rs.normal(0, 0.5, O).astype(np.float32)
    X, Wb, Bb = Buf.of(x), Buf.of(w), Buf.of(b)
    x64, w64 = x[:, :I].astype(np.float64), w.astype(np.float64)
    for bias in (True, False):
        Y = Buf.out(N * Op)
        _lib.call("acg_linear_fwd", X.ptr, Wb.ptr, Bb.ptr if bias else None, Y.ptr, N, I, ldx, O, Op, act, st)
        y64 = _act64(x64 @ w64.T + (b if bias else 0.0), act)
        got = Y.host((N, Op))
        assert np.all(got[:, O:] == 0.0)           # columns O .. Op-1 are written as zeros
        assert rel(got[:, :O], y64) < 1e-5
    y64 = _act64(x64 @ w64.T + b, act)
    y = np.zeros((N, Op), np.float32)
    y[:, :O] = y64
    y[:, O:] = np.nan                              # padded columns of y and dy: never read
    dy = rs.normal(0, 1, (N, Op)).astype(np.float32)
    dy[:, O:] = np.nan
    Yb, DY = Buf.of(y), Buf.of(dy)
    g = dy[:, :O].astype(np.float64) * _grad64(y[:, :O].astype(np.float64), act)
    refs = dict(dx=g @ w64, dw=g.T @ x64, db=g.sum(axis=0))
    for leave in (None, "dx", "dw", "db"):
        dx = None if leave == "dx" else Buf.out(N * ldx)
        dw = None if leave == "dw" else Buf.out(O * I)
        db = None if leave == "db" else Buf.out(O)
        _lib.call("acg_linear_bwd", DY.ptr, Yb.ptr, X.ptr, Wb.ptr, dx.ptr if dx else None, dw.ptr if dw else None, db.ptr if db else None,
                  N, I, ldx, O, Op, act, st)
        if dx:
            got = dx.host((N, ldx))
            assert np.all(np.isnan(got[:, I:]))    # columns beyond I: untouched
            assert rel(got[:, :I], refs["dx"]) < 1e-5
        if dw:
            assert rel(dw.host((O, I)), refs["dw"]) < 1e-5
        if db:
            assert rel(db.host(), refs["db"]) < 1e-5
    assert "bad dims" in rejected(lib, "acg_linear_fwd", X.ptr, Wb.ptr, Bb.ptr, Yb.ptr, N, I, I - 1, O, Op, act, st)
    assert "bad dims" in rejected(lib, "acg_linear_bwd", DY.ptr, Yb.ptr, X.ptr, Wb.ptr, None, None, None, N, I, ldx, O, O - 1, act, st)
    Buf.check_all()


@pytest.mark.parametrize("P", [1, 255, 256, 257, 4096, 70000], ids=lambda p: "P%d_%s" % (p, "trip2" if 2 * p * 16 > GRID_TRIP else "trip1"))
@pytest.mark.parametrize("mean", [0.0, 50.0], ids=["mean0", "mean50"])
def test_spatial_mean(P, mean):
    _lib, lib, st = _env()
    N, Cp = 2, 16
    rs = np.random.RandomState(P)
    x = rs.normal(mean, 1, (N, P, Cp)).astype(np.float32)
    X, Y = Buf.of(x), Buf.out(N * Cp)
    _lib.call("acg_spatial_mean_fwd", X.ptr, Y.ptr, N, P, Cp, st)
    ref = x.astype(np.float64).mean(axis=1)
    got = Y.host((N, Cp))
    if mean:
        assert rel(got, ref) < 1e-5
    else:   # zero-mean data: relative to the mean of the absolute terms
        assert np.max(np.abs(got - ref) / np.abs(x.astype(np.float64)).mean(axis=1)) < 1e-5
    dy = rs.normal(0, 1, (N, Cp)).astype(np.float32)
    DY, DX = Buf.of(dy), Buf.out(N * P * Cp)
    _lib.call("acg_spatial_mean_bwd", DY.ptr, DX.ptr, N, P, Cp, st)
    ref = np.broadcast_to(dy.astype(np.float64)[:, None, :] / P, (N, P, Cp))
    assert np.allclose(DX.host((N, P, Cp)), ref, rtol=2e-7, atol=0)
    Buf.check_all()


@pytest.mark.parametrize("accumulate", [0, 1], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("nseg", [0, 1, 5, 96], ids=lambda n: "segments%d%s" % (n, "_max" if n == 96 else ""))
def test_segments_accumulate(nseg, accumulate):
    _lib, lib, st = _env()
    assert _lib.MAX_SEGMENTS == 96
    lens = [[255, 256, 257, 0, 1, 513, 4, 1024][i % 8] for i in range(nseg)]
    rs = np.random.RandomState(nseg)
    total = sum(lens) + 40
    src = rs.normal(0, 1, total).astype(np.float32)
    S = Buf.of(src)
    sg = _lib.Segments()
    sg.n = nseg
    dsts, pres, offs = [], [], []
    order = rs.permutation(nseg)                                   # offsets not in segment order
    pos = {}
    o = 17
    for s in order:
        pos[s] = o
        o += lens[s]
    for s in range(nseg):
        pre = rs.normal(0, 1, max(lens[s], 1) + 5).astype(np.float32)   # five more elements than the segment: untouched
        dsts.append(Buf.of(pre)); pres.append(pre); offs.append(pos[s])
        sg.dst[s], sg.off[s], sg.len[s] = dsts[s].ptr.value, pos[s], lens[s]
    _lib.call("acg_segments_accumulate", S.ptr, ctypes.byref(sg), accumulate, st)
    for s in range(nseg):
        ref = pres[s].copy()
        seg = src[offs[s]:offs[s] + lens[s]]
        ref[:lens[s]] = ref[:lens[s]] + seg if accumulate else seg
        assert np.array_equal(dsts[s].host(), ref), s
    sg.n = 97
    assert "segment count" in rejected(lib, "acg_segments_accumulate", S.ptr, ctypes.byref(sg), accumulate, st)
    if nseg:
        sg.n, sg.len[0] = nseg, -1
        assert "bad segment" in rejected(lib, "acg_segments_accumulate", S.ptr, ctypes.byref(sg), accumulate, st)
    Buf.check_all()
