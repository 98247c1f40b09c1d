"""GPU tests of the CRPS training loss: acg_crps_fwd / acg_crps_bwd and ops.crps_loss against tests/crps_ref.py.

The tolerances follow from the arithmetic.  `out` holds sums of T non-negative terms formed in double (T = M H W for e1,
M (M - 1) / 2 H W for e2): at most T roundings of 2^-53 relative each, the division by M included, so T 2^-52 relative
covers the kernel and the reference's own summation.  dx is the fp64 expression g (coef_y sy - coef_pair sp) of integer sign
sums, rounded once to float: within one float32 ulp of the rounded reference, and exactly 0 where the reference is 0."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import crps_ref as R
from field_cases import PAIR_LAYOUTS as LAYOUTS, field_operand as _device, shifted as _shifted
from guard_util import GUARD, Buf

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (1, 7), (5, 3), (63, 65), (64, 64), (256, 256))
MEMBERS = (1, 2, 3, 4, 16)
ALPHA = 0.95
G_UP = 0.375                                                       # the upstream gradient of the backward checks: exact in float


@functools.lru_cache(maxsize=4)
def _case(M, N, H, W):
    """members (N M, 3, H, W) and truths (N, 3, H, W); input 0 lies on multiples of 1/8 inside [-1, 1], so that members tie
    with each other and with the truth"""
    rs = np.random.RandomState(1000 * M + 100 * N + 31 * H + W)
    x = rs.standard_normal((N * M, 3, H, W)).astype(np.float32)
    y = rs.standard_normal((N, 3, H, W)).astype(np.float32)
    x[:M] = np.clip(np.round(x[:M] * 4) / 8, -1, 1)
    y[0] = np.clip(np.round(y[0] * 4) / 8, -1, 1)
    return x, y


@functools.lru_cache(maxsize=2)
def _reference(M, N, H, W, C):
    x, y = _case(M, N, H, W)
    sums, grad = R.sums(x[:, :C], y[:, :C], M), R.grad(x[:, :C], y[:, :C], M, ALPHA, G_UP)
    sums.setflags(write=False), grad.setflags(write=False)
    return sums, grad


def _mode_names(lx, cpx, off, ly, cpy):
    """x: a C4 pixel's channels at once where it is NHWC of four stored channels on the 16-byte grid; y: likewise beside such an x"""
    mx = "c4" if (lx, cpx, off) == ("nhwc", 4, 0) else "strided"
    return mx, "c4" if mx == "c4" and (ly, cpy) == ("nhwc", 4) else "strided"


def _sum_bound(ref, M, H, W):
    """T 2^-52 relative per entry of (N, C, 2)"""
    T = np.array([M * H * W, M * (M - 1) // 2 * H * W], dtype=np.float64)
    return T * 2.0 ** -52 * np.abs(ref)


def _to_nchw(t, layout, C):
    return (t.permute(0, 3, 1, 2) if layout == "nhwc" else t)[:, :C].cpu().numpy()


def _check_case(M, N, H, W, C, lay):
    from dtgan_amd import _lib, ops
    lx, cpx, off, ly, cpy = lay
    x, y = _case(M, N, H, W)
    want_sums, want_grad = _reference(M, N, H, W, C)
    xd, yd = _shifted(_device(x, lx, C, cpx, seed=1), off), _device(y, ly, C, cpy, seed=2)
    seen = []
    real = ops._crps_call
    ops._crps_call = lambda *a: (real(*a), seen.append(a[-1].clone()))[0]
    try:
        xd.requires_grad_(True)
        loss, e1, pair = ops.crps_loss(xd, yd, C, lx, ly, M, alpha=ALPHA, parts=True)
        fwd_path = _lib.query("acg_last_kernel").decode()
        (dx,) = torch.autograd.grad(loss * G_UP, xd)                # (on the autograd thread: its path is checked through the ABI)
    finally:
        ops._crps_call = real
    tag = (M, N, H, W, C, lay)
    mx, my = _mode_names(lx, cpx, off, ly, cpy)
    assert fwd_path == "crps_fwd<%s, %s> + crps_fold" % (mx, my), (tag, fwd_path)
    # the backward once more from this thread, as the op calls it: its path by name, and the op's bits
    strides = lambda t, lay_: (H * W * t.shape[-1], t.shape[-1], 1) if lay_ == "nhwc" else (t.shape[1] * H * W, 1, H * W)
    sx, sy, cells = strides(xd, lx), strides(yd, ly), N * C * H * W
    again = torch.full_like(xd.detach(), float("nan")).contiguous()
    _lib.call("acg_crps_bwd", ops._ptr(xd), ops._ptr(yd), ops._ptr(torch.tensor([G_UP], device="cuda")), N * M, M, C,
              xd.shape[-1] if lx == "nhwc" else xd.shape[1], H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2],
              ctypes.c_double(1.0 / (M * cells)), ctypes.c_double(R.weight(M, ALPHA) / cells), ops._ptr(again), ops._stream())
    bwd_path = _lib.query("acg_last_kernel").decode()
    assert bwd_path == "crps_bwd<%s, %s>" % (mx, my), (tag, bwd_path)
    assert torch.equal(again, dx), tag
    got = seen[0].cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (N, C, 2)
    err, tol = np.abs(got - want_sums), _sum_bound(want_sums, M, H, W)
    assert np.all(err <= tol), (tag, err.max(), tol.max())
    if M == 1:
        assert np.all(got[..., 1] == 0.0)
    cells = N * C * H * W
    w = R.weight(M, ALPHA)
    ref_loss = (want_sums[..., 0].sum() - w * want_sums[..., 1].sum()) / cells
    # the scalar: the bounded sums combined in double, one rounding to float
    assert abs(loss.item() - ref_loss) <= 2.0 ** -23 * (want_sums[..., 0].sum() + w * want_sums[..., 1].sum()) / cells + 1e-30, tag
    assert not e1.requires_grad and not pair.requires_grad and loss.dtype == e1.dtype == pair.dtype == torch.float32
    assert dx.shape == xd.shape and dx.dtype == torch.float32
    gd = _to_nchw(dx, lx, C)
    want32 = want_grad.astype(np.float32)
    assert np.all(np.abs(gd.astype(np.float64) - want32) <= np.spacing(np.abs(want32))), (tag, np.abs(gd - want32).max())
    assert np.all(gd[want_grad == 0.0] == 0.0), tag
    if lx == "nhwc" and cpx > C:
        assert torch.all(dx[..., C:] == 0), tag                    # the padded channels, +-50 garbage in x
    return got, gd


@pytest.mark.parametrize("N", (1, 3))
@pytest.mark.parametrize("M", MEMBERS)
@pytest.mark.parametrize("H,W", SIZES)
def test_value_and_gradient_equal_the_reference_in_every_layout(H, W, M, N):
    for C in (3, 1):
        first = None
        for lay in LAYOUTS:
            got = _check_case(M, N, H, W, C, lay)
            if first is None:
                first = got
            # the same bits in every layout: the sums by the fixed order, the gradient by the one rounding
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), (M, N, H, W, C, lay)
    x, y = _case(M, N, H, W)
    if H * W >= 15:                                                # the quantised input does tie, with the truth too
        assert np.any(x[:M] == y[:1]) and (M == 1 or np.any(x[0] == x[1]))


def test_one_case_of_321_by_321():
    """an odd extent of a hundred workgroups per input, the last one cut in its third quarter"""
    for lay in LAYOUTS:
        _check_case(4, 3, 321, 321, 3, lay)


def _fwd_abi(lib, xd, yd, rows, M, C, H, W, sx, sy, out, ws, nbytes):
    from dtgan_amd import ops
    return lib.acg_crps_fwd(ops._ptr(xd), ops._ptr(yd), rows, M, C, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], out, ws, nbytes,
                            ops._stream())


def _bwd_abi(lib, xd, yd, g, rows, M, C, Cp, H, W, sx, sy, cy, cp, dx):
    from dtgan_amd import ops
    return lib.acg_crps_bwd(ops._ptr(xd), ops._ptr(yd), ops._ptr(g), rows, M, C, Cp, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2],
                            ctypes.c_double(cy), ctypes.c_double(cp), dx, ops._stream())


@pytest.mark.parametrize("H,W,Cp", ((5, 3, 4), (63, 65, 16), (64, 64, 4), (256, 256, 4)))
def test_guard_words_poisoned_outputs_and_repeatable_bits(H, W, Cp):
    """through the C ABI: out and dx start as NaN and lie between guard words, the workspace has exactly the queried size,
    starts as 0xFF bytes and lies between guard words; NaN garbage in the padded channels changes nothing; a second call
    gives the same bits"""
    from dtgan_amd import _lib
    lib = _lib.load()
    M, N, C = 3, 3, 3
    x, y = _case(M, N, H, W)
    want_sums, want_grad = _reference(M, N, H, W, C)
    rows, cells = N * M, N * C * H * W
    need = lib.acg_crps_workspace_bytes(rows, M, C, H, W)
    assert need == 16 * N * C * ((H * W + 1023) // 1024)
    g = torch.tensor([G_UP], device="cuda")
    sx, sy = (H * W * Cp, Cp, 1), (C * H * W, 1, H * W)
    runs = []
    for seed in (0, 1):
        xd, yd = _device(x, "nhwc", C, Cp, seed=seed, nan=0.3 * (seed == 1)), _device(y, "nchw", C)
        out = Buf.out(GUARD + 2 * N * C * 2)                       # doubles as pairs of NaN-poisoned words
        ws = Buf(GUARD + need // 4, dtype=np.uint32)               # 0xFFFFFFFF everywhere
        dx = Buf.out(GUARD + rows * H * W * Cp)
        for _ in range(2):
            assert _fwd_abi(lib, xd, yd, rows, M, C, H, W, sx, sy, out.at(GUARD), ws.at(GUARD), need) == 0, lib.acg_last_error().decode()
            assert _bwd_abi(lib, xd, yd, g, rows, M, C, Cp, H, W, sx, sy, 1.0 / (M * cells), R.weight(M, ALPHA) / cells,
                            dx.at(GUARD)) == 0, lib.acg_last_error().decode()
            path = lib.acg_last_kernel().decode()
            assert path == "crps_bwd<%s, strided>" % ("c4" if Cp == 4 else "strided"), path
            o, d = out.host(), dx.host()
            assert np.all(np.isnan(o[:GUARD])) and np.all(np.isnan(d[:GUARD]))
            assert np.all(ws.host()[:GUARD] == 0xFFFFFFFF)
            runs.append((o[GUARD:].copy().view(np.float64).reshape(N, C, 2), d[GUARD:].reshape(rows, H, W, Cp).copy()))
    for o, d in runs:
        assert np.array_equal(o, runs[0][0]) and np.array_equal(d, runs[0][1])
    o, d = runs[0]
    assert np.all(np.abs(o - want_sums) <= _sum_bound(want_sums, M, H, W))
    want32 = want_grad.astype(np.float32)
    assert np.all(np.abs(np.moveaxis(d[..., :C], 3, 1).astype(np.float64) - want32) <= np.spacing(np.abs(want32)))
    assert np.all(d[..., C:] == 0.0)
    Buf.check_all()


def test_a_short_workspace_is_minus_two_and_every_refusal_names_its_entry_point():
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    M, N, C, H, W = 2, 2, 3, 8, 8
    rows = N * M
    xd, yd = torch.zeros(rows, C, H, W, device="cuda"), torch.zeros(N, C, H, W, device="cuda")
    out = torch.full((N, C, 2), 7.0, dtype=torch.float64, device="cuda")
    dx = torch.full_like(xd, 7.0)
    g = torch.ones(1, device="cuda")
    need = lib.acg_crps_workspace_bytes(rows, M, C, H, W)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    s = (C * H * W, 1, H * W)
    P = ops._ptr

    def fwd(x=xd, y=yd, rows=rows, M=M, C=C, H=H, W=W, sx=s, sy=s, o=out, w=ws, nb=need, off=0):
        wp = None if w is None else ctypes.c_void_p(w.data_ptr() + off)
        return lib.acg_crps_fwd(P(x), P(y), rows, M, C, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], P(o), wp, nb, ops._stream())

    def bwd(x=xd, y=yd, g=g, rows=rows, M=M, C=C, Cp=C, H=H, W=W, sx=s, sy=s, cy=0.1, cp=0.1, d=dx):
        return lib.acg_crps_bwd(P(x), P(y), P(g), rows, M, C, Cp, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2],
                                ctypes.c_double(cy), ctypes.c_double(cp), P(d), ops._stream())

    bad = (0, 1, 1)
    for kw, word in ((dict(x=None), "null"), (dict(y=None), "null"), (dict(o=None), "null"), (dict(H=0), "1 <= H, W <= 1024"),
                     (dict(W=1025), "1 <= H, W <= 1024"), (dict(rows=0), "rows >= 1"), (dict(C=0), "C >= 1"),
                     (dict(rows=1 << 30, C=4), "too many fields"), (dict(rows=0x7fffffff, C=2, H=1024, W=1024), "too many fields"),
                     (dict(sx=bad), "strides"), (dict(sy=(5, 0, 1)), "strides"), (dict(M=0), "x_per_y"), (dict(M=17, rows=34), "x_per_y"),
                     (dict(M=3), "x_per_y"), (dict(o=xd), "alias"), (dict(o=yd), "alias"), (dict(off=4), "aligned")):
        assert fwd(**kw) == -1, kw
        msg = lib.acg_last_error().decode()
        assert msg.startswith("acg_crps_fwd: ") and word in msg, (kw, msg)
    for kw in (dict(w=None), dict(nb=need - 1), dict(nb=0)):
        assert fwd(**kw) == -2, kw
        assert lib.acg_last_error().decode().startswith("acg_crps_fwd: workspace too small"), kw
    # the order of the refusals: extent, counts, too many fields, strides, pairing, aliasing, the workspace
    many = dict(rows=1 << 30, C=4)
    assert fwd(H=0, rows=0, nb=0) == -1 and "1 <= H, W" in lib.acg_last_error().decode()
    assert fwd(rows=0, C=1 << 30, sx=bad, nb=0) == -1 and "rows >= 1" in lib.acg_last_error().decode()
    assert fwd(sx=bad, M=3, nb=0, **many) == -1 and "too many fields" in lib.acg_last_error().decode()
    assert fwd(sx=bad, M=3, nb=0) == -1 and "strides" in lib.acg_last_error().decode()
    assert fwd(M=3, o=xd, nb=0) == -1 and "x_per_y" in lib.acg_last_error().decode()
    assert fwd(o=yd, nb=0) == -1 and "alias" in lib.acg_last_error().decode()
    for kw, word in ((dict(x=None), "null"), (dict(y=None), "null"), (dict(g=None), "null"), (dict(d=None), "null"),
                     (dict(H=1025), "1 <= H, W <= 1024"), (dict(rows=0), "rows >= 1"), (dict(C=0), "rows >= 1"), (dict(Cp=2), "C <= Cp"),
                     (dict(rows=1 << 30, C=4, Cp=4), "too many fields"), (dict(sx=bad), "strides"), (dict(M=0), "x_per_y"), (dict(M=3), "x_per_y"), (dict(cy=float("nan")), "finite"),
                     (dict(cp=float("inf")), "finite"), (dict(d=xd), "alias"), (dict(d=yd), "alias"), (dict(d=g), "alias")):
        assert bwd(**kw) == -1, kw
        msg = lib.acg_last_error().decode()
        assert msg.startswith("acg_crps_bwd: ") and word in msg, (kw, msg)
    assert bwd(H=0, rows=0) == -1 and "1 <= H, W" in lib.acg_last_error().decode()
    assert bwd(rows=0, C=1 << 30, Cp=1 << 30, sx=bad) == -1 and "rows >= 1" in lib.acg_last_error().decode()
    assert bwd(sx=bad, M=3, Cp=4, **many) == -1 and "too many fields" in lib.acg_last_error().decode()
    assert bwd(sx=bad, M=3) == -1 and "strides" in lib.acg_last_error().decode()
    assert bwd(M=3, cy=float("nan")) == -1 and "x_per_y" in lib.acg_last_error().decode()
    assert bwd(cy=float("nan"), d=yd) == -1 and "finite" in lib.acg_last_error().decode()
    torch.cuda.synchronize()
    assert torch.all(out == 7.0) and torch.all(dx == 7.0)          # nothing was launched
    assert lib.acg_crps_workspace_bytes(rows, 3, C, H, W) == 0 and lib.acg_crps_workspace_bytes(rows, M, C, H, 1025) == 0
    assert fwd() == 0 and bwd() == 0


@pytest.mark.parametrize("H,W", ((63, 65), (64, 64)))
def test_capture_and_replay_in_a_graph(H, W):
    """launches only: both entry points captured once from the capturing thread into outputs that exist, replayed into
    poisoned outputs, the same bits as the plain calls.  (The op under autograd is captured with the paired step,
    test_hip_crps_step.py.)"""
    from dtgan_amd import _lib, ops
    M, N, C = 4, 3, 3
    x, y = _case(M, N, H, W)
    want_sums, want_grad = _reference(M, N, H, W, C)
    xd, yd = _device(x, "nhwc", C, 4, seed=1), _device(y, "nhwc", C, 4, seed=2)
    out = torch.full((N, C, 2), -7.0, dtype=torch.float64, device="cuda")
    dx = torch.full_like(xd, -7.0)
    g = torch.tensor([G_UP], device="cuda")
    cells = N * C * H * W
    sx = (H * W * 4, 4, 1)

    def call():
        ops._crps_call(xd, yd, (N * M, C, H, W), sx, sx, M, out)
        _lib.call("acg_crps_bwd", ops._ptr(xd), ops._ptr(yd), ops._ptr(g), N * M, M, C, 4, H, W, sx[0], sx[1], sx[2], sx[0], sx[1], sx[2],
                  ctypes.c_double(1.0 / (M * cells)), ctypes.c_double(R.weight(M, ALPHA) / cells), ops._ptr(dx), ops._stream())

    call()                                                         # the workspace exists before the capture
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
    assert np.all(np.abs(first[0] - want_sums) <= _sum_bound(want_sums, M, H, W))
    want32 = want_grad.astype(np.float32)
    assert np.all(np.abs(np.moveaxis(first[1][..., :C], 3, 1).astype(np.float64) - want32) <= np.spacing(np.abs(want32)))


@pytest.mark.parametrize("M", (1, 2, 5, 16))
def test_the_parts_equal_the_reference_and_nothing_is_saved_without_a_gradient(M):
    from dtgan_amd import ops
    N, C, H, W = 3, 3, 33, 31
    x, y = _case(M, N, H, W)
    xd, yd = _device(x, "nhwc", C, 4, seed=1), _device(y, "nchw", C)
    for alpha in (0.0, 0.95, 1.0):
        loss, e1, pair = ops.crps_loss(xd, yd, C, "nhwc", "nchw", M, alpha=alpha, parts=True)
        ref = R.parts(x, y, M, alpha)
        # float32 scalars of double sums within T 2^-52: one rounding each, the loss a difference of two of them
        scale = (ref[1] + R.weight(M, alpha) * ref[2] * M * (M - 1) / 2, ref[1], ref[2])
        for got, want, sc in zip((loss, e1, pair), ref, scale):
            assert abs(got.item() - want) <= 2.0 ** -23 * sc + 1e-30, (M, alpha, got.item(), want)
        assert loss.grad_fn is None and not loss.requires_grad
        assert torch.equal(ops.crps_loss(xd, yd, C, "nhwc", "nchw", M, alpha=alpha), loss)
    if M == 1:
        assert pair.item() == 0.0 and loss.item() == e1.item()     # the mean absolute error
        assert abs(loss.item() - np.abs(x.astype(np.float64) - y).mean()) <= 2.0 ** -23 * ref[1]
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        with torch.no_grad():
            ops.crps_loss(xd.clone().requires_grad_(True), yd, C, "nhwc", "nchw", M)
        ops.crps_loss(xd, yd, C, "nhwc", "nchw", M)
        assert saved == []
        ops.crps_loss(xd.clone().requires_grad_(True), yd, C, "nhwc", "nchw", M)
        assert len(saved) == 2                                     # x and y, no maps


@pytest.mark.parametrize("M", (2, 4, 16))
def test_alpha_zero_and_one_equal_the_evaluators_scores(M):
    """ops.ensemble_stats on the same members.  Its crps_map is float32: per cell (double)e1 - E2 / 2 with e1 rounded to
    float first and the difference rounded once more, so a cell is off by at most 2^-24 (e1 + |crps|) <= 2^-23 e1, and so is
    the mean; our scalar adds its own float rounding, 2^-24 of at most e1: 2^-22 mean(e1) in all.  Its fair form comes from
    its float32 sums of e1 and E2, non-negative terms added in float: a cell's rounding, C additions in a thread, the eight
    levels of the workgroup's tree and the final rounding, (C + 10) 2^-24 relative on each sum, plus our scalar's 2^-24."""
    from dtgan_amd import ops
    N, C, H, W = 3, 3, 33, 31
    x, y = _case(M, N, H, W)
    xd, yd = _device(x, "nhwc", C, 4, seed=1), _device(y, "nhwc", C, 4, seed=2)
    st = ops.ensemble_stats(xd, yd, M, C, (0.1, 0.9))
    l0, e1, _ = ops.crps_loss(xd, yd, C, "nhwc", "nhwc", M, alpha=0.0, parts=True)
    l1 = ops.crps_loss(xd, yd, C, "nhwc", "nhwc", M, alpha=1.0)
    e1 = e1.item()
    want0 = st["crps_map"].double().mean().item()
    assert abs(l0.item() - want0) <= 2.0 ** -22 * e1, (l0.item(), want0)
    s = st["sums"].double().cpu().numpy()
    cells = C * H * W
    k = M / (2.0 * (M - 1))
    want1 = ((s[:, 0] - s[:, 1] * k) / cells).mean()
    tol1 = ((C + 10) * 2.0 ** -24 * (s[:, 0] + s[:, 1] * k) / cells).mean() + 2.0 ** -24 * e1
    assert abs(l1.item() - want1) <= tol1, (l1.item(), want1, tol1)
    assert abs(want1 - R.loss(x, y, M, 1.0)) <= tol1 and l1.item() < l0.item()
