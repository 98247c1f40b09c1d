"""GPU tests of the fractions-skill-score training loss: acg_fss_loss_fwd / acg_fss_loss_bwd through the C ABI and through
ops.fss_loss, against tests/fss_loss_ref.py.

The bars are fss_loss_ref.FWD_BAR and GRAD_BAR: 4 x the error of the float32 restatement of the definition against the fp64
reference on these same cases (num and den relative to den; the gradient relative to the case's largest |gradient|).  The
pooled ratio R = Num / Den of sums within FWD_BAR Den each is within FWD_BAR (1 + R) / (1 - FWD_BAR) <= 2.001 FWD_BAR of the
reference's (R <= 1 since (cf - co)^2 <= cf^2 + co^2 for sums of non-negative events), and so is their mean, the loss, plus its
one rounding to float.  With saturated events everything is integer: equality."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fss_loss_ref as R
import fss_ref as F
from field_cases import field_operand as _device
from guard_util import GUARD, Buf

pytestmark = pytest.mark.gpu

G_UP = 0.375                                                       # the upstream gradient of the backward checks: exact in float
LAYOUTS = (("nchw", 0), ("nhwc", 4), ("nhwc", 16))                 # of x; the truth takes the layouts in another order
MARGIN = 1e-3                                                      # the hard limit: tau = MARGIN / 200


@functools.lru_cache(maxsize=None)
def _case(k):
    H, W, rows, C, T, windows, tau, kind = R.CASES[k]
    x, y, thr = R.make_case(H, W, rows, C, T, kind)
    ref = dict(R.loss(x, y, thr, windows, tau), grad=R.grad(x, y, thr, windows, tau) * G_UP)
    for a in (x, y, thr, ref["num"], ref["den"], ref["grad"], ref["R"], ref["Den"]):
        a.setflags(write=False)
    return x, y, thr, ref


def _strides(t, layout, H, W):
    return (H * W * t.shape[-1], t.shape[-1], 1) if layout == "nhwc" else (t.shape[1] * H * W, 1, H * W)


def _stored(t, layout):
    return t.shape[-1] if layout == "nhwc" else t.shape[1]


def _win(windows):
    return (ctypes.c_int * len(windows))(*windows)


def _fwd_abi(lib, xd, yd, rows, C, H, W, sx, sy, thr, T, windows, tau, out, ws, nbytes):
    from dtgan_amd import ops
    return lib.acg_fss_loss_fwd(ops._ptr(xd), ops._ptr(yd), rows, C, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], ops._ptr(thr), T,
                                _win(windows), len(windows), ctypes.c_float(ops.fss_loss_inv_tau(tau)), out, ws, nbytes, ops._stream())


def _bwd_abi(lib, xd, yd, rows, C, Cp, H, W, sx, sy, thr, T, windows, tau, coef, dx, ws, nbytes):
    from dtgan_amd import ops
    return lib.acg_fss_loss_bwd(ops._ptr(xd), ops._ptr(yd), rows, C, Cp, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], ops._ptr(thr), T,
                                _win(windows), len(windows), ctypes.c_float(ops.fss_loss_inv_tau(tau)), ops._ptr(coef), dx, ws, nbytes,
                                ops._stream())


def _sums(xd, lx, yd, ly, C, thr_d, windows, tau):
    """acg_fss_loss_fwd through the ABI on any pair of layouts -> (rows, C, T, nw, 2) float64 on the host, from a poisoned out"""
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    rows = xd.shape[0]
    H, W = (xd.shape[2], xd.shape[3]) if lx == "nchw" else (xd.shape[1], xd.shape[2])
    T, nw = thr_d.shape[1], len(windows)
    out = torch.full((rows, C, T, nw, 2), float("nan"), dtype=torch.float64, device="cuda")
    need = lib.acg_fss_loss_workspace_bytes(rows, C, H, W, T, nw)
    assert need > 0 and need % 16 == 0
    ws = ops.workspace(need, slot=2)
    rc = _fwd_abi(lib, xd, yd, rows, C, H, W, _strides(xd, lx, H, W), _strides(yd, ly, H, W), thr_d, T, windows, tau, ops._ptr(out),
                  ops._ptr(ws), need)
    assert rc == 0, lib.acg_last_error().decode()
    assert lib.acg_last_kernel().decode() == "fss_loss_fwd + fss_loss_fold"
    return out.cpu().numpy()


def _to_nchw(t, layout, C):
    return (t.permute(0, 3, 1, 2) if layout == "nhwc" else t)[:, :C].cpu().numpy()


@pytest.mark.parametrize("k", range(len(R.CASES)))
def test_sums_loss_and_gradient_lie_within_the_float32_bars_in_every_layout(k):
    from dtgan_amd import ops
    H, W, rows, C, T, windows, tau, kind = R.CASES[k]
    x, y, thr, ref = _case(k)
    thr_d = torch.from_numpy(np.array(thr)).cuda()
    first = None
    for n, (lx, cpx) in enumerate(LAYOUTS):
        ly, cpy = LAYOUTS[(n + 1) % len(LAYOUTS)]                  # a mixed pair through the ABI
        xd, ym = _device(x, lx, C, cpx, seed=1), _device(y, ly, C, cpy, seed=2)
        got = _sums(xd, lx, ym, ly, C, thr_d, windows, tau)
        some = ref["den"] > 0
        assert some.all(), "every case has events"
        e_num = (np.abs(got[..., 0] - ref["num"]) / ref["den"]).max()
        e_den = (np.abs(got[..., 1] - ref["den"]) / ref["den"]).max()
        print("case %d %s: num %.3g den %.3g (bar %.3g)" % (k, lx, e_num, e_den, R.FWD_BAR))
        assert e_num <= R.FWD_BAR and e_den <= R.FWD_BAR, (k, lx, e_num, e_den)
        yd = _device(y, lx, C, cpx, seed=3)                        # the op: one layout for both
        xd.requires_grad_(True)
        loss, Rg = ops.fss_loss(xd, yd, C, lx, thr_d if n else np.array(thr), windows, tau, parts=True)
        (dx,) = torch.autograd.grad(loss * G_UP, xd)
        assert loss.dtype == torch.float32 and Rg.dtype == torch.float64 and tuple(Rg.shape) == (C, T, len(windows))
        assert not Rg.requires_grad
        e_R = np.abs(Rg.cpu().numpy() - ref["R"]).max()
        assert e_R <= 2.001 * R.FWD_BAR, (k, lx, e_R)
        assert abs(loss.item() - ref["loss"]) <= 2.001 * R.FWD_BAR + 2.0 ** -24 * ref["loss"], (k, lx, loss.item(), ref["loss"])
        assert dx.shape == xd.shape and dx.dtype == torch.float32
        gd = _to_nchw(dx, lx, C)
        top = np.abs(ref["grad"]).max()
        e_g = np.abs(gd - ref["grad"]).max() / top
        print("case %d %s: gradient %.3g (bar %.3g)" % (k, lx, e_g, R.GRAD_BAR))
        assert e_g <= R.GRAD_BAR, (k, lx, e_g)
        if lx == "nhwc":
            assert torch.all(dx[..., C:] == 0), (k, lx)            # the padded channels, +-50 garbage in x
        if first is None:
            first = got, gd, loss.item()
        # the same bits in every layout
        assert np.array_equal(got, first[0]) and np.array_equal(gd, first[1]) and loss.item() == first[2], (k, lx)


@pytest.mark.parametrize("H,W", ((1, 1), (5, 7), (33, 31), (65, 130)))
def test_saturated_events_give_the_evaluators_integer_triples_and_a_zero_gradient(H, W):
    from dtgan_amd import ops
    windows = tuple(n for n in F.WINDOWS if n <= R.MAX_WINDOW)
    assert windows == (1, 3, 9, 33, 65)
    for kind in ("noise", "shifted", "ties", "extremes"):
        x, y, thr = F.make_pair(kind, H, W)
        x, y = R.harden(x, thr, MARGIN), R.harden(y, thr, MARGIN)
        want = F.triples(x, y, thr, windows).astype(np.float64)
        thr_d = torch.from_numpy(thr).cuda()
        for lx, cpx in LAYOUTS[:2]:
            xd, yd = _device(x, lx, 3, cpx, seed=1), _device(y, lx, 3, cpx, seed=2)
            tri = ops.fss(xd, yd, 3, lx, lx, thr_d, windows).cpu().numpy().astype(np.float64)
            assert np.array_equal(tri, want)
            got = _sums(xd, lx, yd, lx, 3, thr_d, windows, MARGIN / 200)
            assert np.array_equal(got[..., 0], tri[..., 0] + tri[..., 1] - 2 * tri[..., 2]), (kind, H, W, lx)
            assert np.array_equal(got[..., 1], tri[..., 0] + tri[..., 1]), (kind, H, W, lx)
            xd.requires_grad_(True)
            loss = ops.fss_loss(xd, yd, 3, lx, thr_d, windows, MARGIN / 200)
            (dx,) = torch.autograd.grad(loss, xd)
            assert torch.all(dx == 0) and np.isfinite(loss.item()), (kind, H, W, lx)     # p (1 - p) is exactly 0


def test_no_event_on_either_side_is_a_loss_and_a_gradient_of_exactly_zero():
    from dtgan_amd import ops
    x, y, _ = R.make_case(33, 31, 2, 3, 1)
    thr = np.full((3, 2), 40.0, dtype=np.float32)                  # exp(-(x - 40) / 0.05) overflows: p == 0, Den == 0
    for lx, cpx in LAYOUTS:
        xd, yd = _device(x, lx, 3, cpx, seed=1).requires_grad_(True), _device(y, lx, 3, cpx, seed=2)
        loss, Rg = ops.fss_loss(xd, yd, 3, lx, thr, (3, 9), 0.05, parts=True)
        (dx,) = torch.autograd.grad(loss, xd)
        assert loss.item() == 0.0 and torch.all(Rg == 0) and torch.all(dx == 0)
        got = _sums(xd.detach(), lx, yd, lx, 3, torch.from_numpy(thr).cuda(), (3, 9), 0.05)
        assert np.all(got == 0.0)
    # one threshold with events beside one without: the rule is per (c, t, window)
    thr[:, 0] = 0.5
    xd, yd = _device(x, "nchw", 3).requires_grad_(True), _device(y, "nchw", 3)
    loss, Rg = ops.fss_loss(xd, yd, 3, "nchw", thr, (3, 9), 0.05, parts=True)
    (dx,) = torch.autograd.grad(loss, xd)
    ref = R.loss(x, y, thr, (3, 9), 0.05)
    assert torch.all(Rg[:, 1] == 0) and torch.all(Rg[:, 0] > 0) and torch.isfinite(dx).all() and dx.abs().max() > 0
    assert abs(loss.item() - ref["loss"]) <= 2.001 * R.FWD_BAR + 2.0 ** -24 * ref["loss"]


def test_x_on_the_truth_is_zero_and_nan_reaches_the_loss():
    from dtgan_amd import ops
    x, _, thr = R.make_case(33, 31, 2, 3, 2)
    xd = _device(x, "nhwc", 3, 4, seed=1).requires_grad_(True)
    loss = ops.fss_loss(xd, xd.detach().clone(), 3, "nhwc", thr, (3, 9), 0.25)
    (dx,) = torch.autograd.grad(loss, xd)
    assert loss.item() == 0.0 and torch.all(dx == 0)
    bad = xd.detach().clone()
    bad[1, 5, 5, 2] = float("nan")
    assert torch.isnan(ops.fss_loss(bad, xd.detach(), 3, "nhwc", thr, (3, 9), 0.25))


@pytest.mark.parametrize("k", (2, 7, 9))
def test_guard_words_poisoned_outputs_and_repeatable_bits(k):
    """through the C ABI: out and dx start as NaN and lie between guard words, the workspace has exactly the queried size,
    starts as 0xFF bytes and lies between guard words; NaN garbage in the padded channels changes nothing; a second call
    gives the same bits"""
    from dtgan_amd import _lib
    lib = _lib.load()
    H, W, rows, C, T, windows, tau, kind = R.CASES[k]
    x, y, thr, ref = _case(k)
    nw, Cp = len(windows), 4
    thr_d = torch.from_numpy(np.array(thr)).cuda()
    need = lib.acg_fss_loss_workspace_bytes(rows, C, H, W, T, nw)
    tiles = ((H + R.TILE - 1) // R.TILE) * ((W + R.TILE - 1) // R.TILE)
    assert need == (max(16 * rows * C * T * nw * tiles, 4 * rows * C * T * nw * H * W) + 15) // 16 * 16
    a, b = R.coefficients(ref["R"], ref["Den"])
    coef = torch.from_numpy(np.stack([a, b], -1) * G_UP).cuda().contiguous()
    sx, sy = (H * W * Cp, Cp, 1), (C * H * W, 1, H * W)
    runs = []
    for seed in (0, 1):
        xd, yd = _device(x, "nhwc", C, Cp, seed=seed, nan=0.3 * (seed == 1)), _device(y, "nchw", C)
        out = Buf.out(GUARD + 2 * rows * C * T * nw * 2)           # doubles as pairs of NaN-poisoned words
        ws = Buf(GUARD + need // 4, dtype=np.uint32)               # 0xFFFFFFFF everywhere
        dx = Buf.out(GUARD + rows * H * W * Cp)
        for _ in range(2):
            assert _fwd_abi(lib, xd, yd, rows, C, H, W, sx, sy, thr_d, T, windows, tau, out.at(GUARD), ws.at(GUARD), need) == 0, \
                lib.acg_last_error().decode()
            assert _bwd_abi(lib, xd, yd, rows, C, Cp, H, W, sx, sy, thr_d, T, windows, tau, coef, dx.at(GUARD), ws.at(GUARD),
                            need) == 0, lib.acg_last_error().decode()
            assert lib.acg_last_kernel().decode() == "fss_loss_g + fss_loss_dx"
            o, d = out.host(), dx.host()
            assert np.all(np.isnan(o[:GUARD])) and np.all(np.isnan(d[:GUARD]))
            assert np.all(ws.host()[:GUARD] == 0xFFFFFFFF)
            runs.append((o[GUARD:].copy().view(np.float64).reshape(rows, C, T, nw, 2), d[GUARD:].reshape(rows, H, W, Cp).copy()))
    for o, d in runs:
        assert np.array_equal(o, runs[0][0]) and np.array_equal(d, runs[0][1])
    o, d = runs[0]
    assert (np.abs(o[..., 0] - ref["num"]) / ref["den"]).max() <= R.FWD_BAR and (np.abs(o[..., 1] - ref["den"]) / ref["den"]).max() <= R.FWD_BAR
    # the coefficients are the reference's here, not the device's own forward's: the bar holds all the more
    assert np.abs(np.moveaxis(d[..., :C], 3, 1) - ref["grad"]).max() <= R.GRAD_BAR * np.abs(ref["grad"]).max()
    assert np.all(d[..., C:] == 0.0)
    Buf.check_all()


def test_a_short_workspace_is_minus_two_and_every_refusal_names_its_entry_point():
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    rows, C, H, W, T = 2, 3, 8, 8, 2
    windows = (3, 9)
    xd, yd = torch.zeros(rows, C, H, W, device="cuda"), torch.zeros(rows, C, H, W, device="cuda")
    thr = torch.zeros(C, T, device="cuda")
    out = torch.full((rows, C, T, 2, 2), 7.0, dtype=torch.float64, device="cuda")
    dx = torch.full_like(xd, 7.0)
    coef = torch.ones(C, T, 2, 2, dtype=torch.float64, device="cuda")
    need = lib.acg_fss_loss_workspace_bytes(rows, C, H, W, T, 2)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    s = (C * H * W, 1, H * W)
    P = ops._ptr

    def fwd(x=xd, y=yd, rows=rows, C=C, H=H, W=W, sx=s, sy=s, th=thr, T=T, win=windows, nw=None, it=4.0, o=out, w=ws, nb=need, off=0):
        wp = None if w is None else ctypes.c_void_p(w.data_ptr() + off)
        return lib.acg_fss_loss_fwd(P(x), P(y), rows, C, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], P(th), T,
                                    None if win is None else _win(win), len(win) if nw is None else nw, ctypes.c_float(it), P(o), wp, nb,
                                    ops._stream())

    def bwd(x=xd, y=yd, rows=rows, C=C, Cp=C, H=H, W=W, sx=s, sy=s, th=thr, T=T, win=windows, nw=None, it=4.0, co=coef, d=dx, w=ws,
            nb=need, off=0):
        wp = None if w is None else ctypes.c_void_p(w.data_ptr() + off)
        return lib.acg_fss_loss_bwd(P(x), P(y), rows, C, Cp, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], P(th), T,
                                    None if win is None else _win(win), len(win) if nw is None else nw, ctypes.c_float(it), P(co), P(d),
                                    wp, nb, ops._stream())

    bad = (0, 1, 1)
    common = ((dict(x=None), "null"), (dict(y=None), "null"), (dict(th=None), "null"), (dict(win=None, nw=2), "null"),
              (dict(H=0), "1 <= H, W <= 1024"), (dict(W=1025), "1 <= H, W <= 1024"), (dict(rows=0), "rows >= 1"), (dict(C=0), "C >= 1"),
              (dict(T=0), "1 <= T <= 8"), (dict(T=9), "1 <= T <= 8"), (dict(nw=0), "1 <= nw <= 8"), (dict(nw=9), "1 <= nw <= 8"),
              (dict(win=(3, 4)), "odd"), (dict(win=(0, 3)), "odd"), (dict(win=(-3, 3)), "odd"), (dict(win=(3, 67)), "1..65"),
              (dict(sx=bad), "strides"), (dict(sy=(5, 0, 1)), "strides"), (dict(it=0.0), "inv_tau"), (dict(it=-1.0), "inv_tau"),
              (dict(it=float("inf")), "inv_tau"), (dict(it=float("nan")), "inv_tau"),
              (dict(rows=1 << 30, C=4), "too many fields"), (dict(off=4), "aligned"))
    for call, name, extra in ((fwd, "acg_fss_loss_fwd", ((dict(o=None), "null"), (dict(o=xd), "alias"), (dict(o=yd), "alias"))),
                              (bwd, "acg_fss_loss_bwd", ((dict(co=None), "null"), (dict(d=None), "null"), (dict(Cp=2), "C <= Cp"),
                                                         (dict(d=xd), "alias"), (dict(d=yd), "alias")))):
        for kw, word in common + extra:
            if name.endswith("bwd") and "C" in kw:
                kw = dict(kw, Cp=max(kw["C"], 1))
            assert call(**kw) == -1, (name, kw)
            msg = lib.acg_last_error().decode()
            assert msg.startswith(name + ": ") and word in msg, (kw, msg)
        for kw in (dict(w=None), dict(nb=need - 1), dict(nb=0)):
            assert call(**kw) == -2, (name, kw)
            assert lib.acg_last_error().decode().startswith(name + ": workspace too small"), kw
        # the order: extent, counts, T and nw, windows, strides, inv_tau, aliasing, the workspace
        assert call(H=0, rows=0, nb=0) == -1 and "1 <= H, W" in lib.acg_last_error().decode()
        assert call(rows=0, T=0, nb=0) == -1 and "rows >= 1" in lib.acg_last_error().decode()
        assert call(T=0, win=(2,), nb=0) == -1 and "1 <= T" in lib.acg_last_error().decode()
        assert call(win=(2, 3), sx=bad, nb=0) == -1 and "odd" in lib.acg_last_error().decode()
        assert call(sx=bad, it=0.0, nb=0) == -1 and "strides" in lib.acg_last_error().decode()
        assert call(it=0.0, nb=0) == -1 and "inv_tau" in lib.acg_last_error().decode()
    torch.cuda.synchronize()
    assert torch.all(out == 7.0) and torch.all(dx == 7.0)          # nothing was launched
    for args in ((0, 1, 8, 8, 1, 1), (1, 0, 8, 8, 1, 1), (1, 1, 0, 8, 1, 1), (1, 1, 8, 1025, 1, 1), (1, 1, 8, 8, 0, 1), (1, 1, 8, 8, 9, 1),
                 (1, 1, 8, 8, 1, 0), (1, 1, 8, 8, 1, 9), (1 << 30, 4, 8, 8, 1, 1)):
        assert lib.acg_fss_loss_workspace_bytes(*args) == 0, args
    assert fwd() == 0 and bwd() == 0


@pytest.mark.parametrize("k", (3, 8))
def test_capture_and_replay_in_a_graph(k):
    """launches only: both entry points captured once from the capturing thread into outputs that exist, replayed into
    poisoned outputs, the same bits as the plain calls.  (The op under autograd is captured with the paired step,
    test_hip_fss_loss_step.py.)"""
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    H, W, rows, C, T, windows, tau, kind = R.CASES[k]
    x, y, thr, ref = _case(k)
    nw = len(windows)
    xd, yd = _device(x, "nhwc", C, 4, seed=1), _device(y, "nhwc", C, 4, seed=2)
    thr_d = torch.from_numpy(np.array(thr)).cuda()
    a, b = R.coefficients(ref["R"], ref["Den"])
    coef = torch.from_numpy(np.stack([a, b], -1) * G_UP).cuda().contiguous()
    out = torch.full((rows, C, T, nw, 2), -7.0, dtype=torch.float64, device="cuda")
    dx = torch.full_like(xd, -7.0)
    sx = (H * W * 4, 4, 1)
    need = lib.acg_fss_loss_workspace_bytes(rows, C, H, W, T, nw)
    ws = ops.workspace(need, slot=2)                               # exists before the capture

    def call():
        assert _fwd_abi(lib, xd, yd, rows, C, H, W, sx, sx, thr_d, T, windows, tau, ops._ptr(out), ops._ptr(ws), need) == 0
        assert _bwd_abi(lib, xd, yd, rows, C, 4, H, W, sx, sx, thr_d, T, windows, tau, coef, ops._ptr(dx), ops._ptr(ws), need) == 0

    call()
    first = out.cpu().numpy(), dx.cpu().numpy()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            call()
    torch.cuda.current_stream().wait_stream(s)
    out.fill_(-7.0), dx.fill_(-7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), first[0]) and np.array_equal(dx.cpu().numpy(), first[1])
    assert (np.abs(first[0][..., 1] - ref["den"]) / ref["den"]).max() <= R.FWD_BAR
    assert np.abs(np.moveaxis(first[1][..., :C], 3, 1) - ref["grad"]).max() <= R.GRAD_BAR * np.abs(ref["grad"]).max()


def test_nothing_is_saved_without_a_gradient_and_the_device_refuses_a_host_table():
    from dtgan_amd import _lib, ops
    x, y, thr = R.make_case(33, 31, 2, 3, 2)
    xd, yd = _device(x, "nhwc", 3, 4, seed=1), _device(y, "nhwc", 3, 4, seed=2)
    args = (yd, 3, "nhwc", thr, (3, 9), 0.25)
    loss = ops.fss_loss(xd, *args)
    assert loss.grad_fn is None and not loss.requires_grad
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        with torch.no_grad():
            assert torch.equal(ops.fss_loss(xd.clone().requires_grad_(True), *args), loss)
        ops.fss_loss(xd, *args)
        assert saved == []
        again = ops.fss_loss(xd.clone().requires_grad_(True), *args)
        assert len(saved) == 5 and torch.equal(again, loss)        # x, y, the thresholds and the pooled R and Den: no maps
        assert sorted(t.numel() for t in saved)[:3] == [6, 12, 12]
    with pytest.raises(_lib.AcgError, match="no CPU path"):
        ops.fss_loss(xd, yd, 3, "nhwc", torch.from_numpy(thr), (3, 9), 0.25)
