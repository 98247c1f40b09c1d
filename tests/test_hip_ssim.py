"""GPU tests of the structural similarity kernels: acg_ssim (with and without the derivative maps) and acg_ssim_bwd through the
C ABI into poisoned, guarded buffers, and ops.ssim / ops.ssim_loss, against tests/ssim_ref.py (float64)."""
import functools

import numpy as np
import pytest
import torch

import ssim_ref as R
from field_cases import field_operand, strides as _strides, valid as _valid
from guard_util import Buf

pytestmark = pytest.mark.gpu

# The bars are measured, not chosen: the same separable formula in NumPy float32 with the textbook E[x^2] - mu^2 needs, over
# ssim_ref.CASES (the near-flat field off zero and the step among them), 6.0130e-05 on the mean S / mean cs (absolute) and
# 1.7730e-04 on the gradient relative to its field's largest entry (tests/test_ssim_ref_cpu.py measures and pins both).  The
# bars (ssim_ref.VALUE_TOL, GRAD_TOL) are 4 x those.
VALUE_TOL, GRAD_TOL = R.VALUE_TOL, R.GRAD_TOL
EPS = 2.0 ** -24
# (layout of x, C, Cp)
LAYOUTS = [("nhwc", 3, 4), ("nhwc", 1, 4), ("nhwc", 1, 16), ("nchw", 3, 3), ("nchw", 1, 1)]
ROWS = (1, 3)


def _device(x, layout, C, Cp, fill="nan"):
    """the first C channels of x (rows, >= C, H, W) on the device in the layout; NHWC: NaN (or 37.5) in the padded channels"""
    return field_operand(x, layout, C, Cp, fill=np.nan if fill == "nan" else 37.5)


@functools.lru_cache(maxsize=None)
def _case(kind, H, W, rows, C):
    """the pair with its float64 values (rows, C, 2), loss gradient and derivative maps; read-only, shared by the tests"""
    x, y = R.make_pair(kind, H, W, rows, C)
    val, _, grad = R.ssim_and_grad(x, y)
    out = (x, y, val, grad)
    for a in out:
        a.setflags(write=False)
    return out


def _fwd(xd, yd, lay_x, lay_y, C, rows, H, W, x_per_y=1, want_maps=False, data_range=2.0):
    """acg_ssim through the C ABI -> (out (rows, C, 2), maps Buf or None, the launch's name)"""
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    sx = _strides(lay_x, C, xd.shape[-1] if lay_x == "nhwc" else C, H, W)
    sy = _strides(lay_y, C, yd.shape[-1] if lay_y == "nhwc" else C, H, W)
    out = Buf.out(rows * C * 2)
    maps = Buf.out(3 * rows * C * (H - 10) * (W - 10)) if want_maps else None
    need = lib.acg_ssim_workspace_bytes(rows, C, H, W)
    tiles = -(-(H - 10) // R.TILE_H) * -(-(W - 10) // R.TILE_W)
    assert need == 16 * rows * C * tiles
    ws = Buf.out(need // 4)
    rc = lib.acg_ssim(ops._ptr(xd), ops._ptr(yd), rows, x_per_y, C, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], data_range,
                      out.ptr, maps.ptr if want_maps else None, ws.ptr, need, ops._stream())
    assert rc == 0, lib.acg_last_error().decode()
    name = _lib.query("acg_last_kernel").decode()
    ws.host()                                                                   # its guard words
    return out.host((rows, C, 2)), maps, name


def _bwd(maps, xd, yd, lay, C, Cp, rows, H, W, g=1.0):
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    st = _strides(lay, C, Cp, H, W)
    gx = Buf.out(xd.numel())
    gd = torch.full((1,), g, device="cuda")
    rc = lib.acg_ssim_bwd(maps.ptr, ops._ptr(xd), ops._ptr(yd), ops._ptr(gd), rows, C, Cp, H, W, st[0], st[1], st[2], st[0], st[1], st[2],
                          gx.ptr, ops._stream())
    assert rc == 0, lib.acg_last_error().decode()
    return gx.host(tuple(xd.shape))


def _cases_of(H, W):
    return [c for c in R.CASES if (c[1], c[2]) == (H, W)]


@pytest.mark.parametrize("H, W", R.SHAPES + R.LARGE_SHAPES)
def test_values_maps_and_gradient_match_the_reference(H, W):
    worst = {}
    for kind, _, _, rows_all, C_all in _cases_of(H, W):
        x, y, val, grad = _case(kind, H, W, rows_all, C_all)
        for lay, C, Cp in LAYOUTS:
            if C > C_all:
                continue
            for rows in sorted({min(r, rows_all) for r in ROWS}):
                xd, yd = _device(x[:rows], lay, C, Cp), _device(y[:rows], lay, C, Cp)
                got, maps, name = _fwd(xd, yd, lay, lay, C, rows, H, W, want_maps=True)
                c4 = "c4" if (lay, Cp) == ("nhwc", 4) else "strided"
                assert name == "ssim_fwd<%s, %s> with maps + ssim_fold" % (c4, c4), name
                ev = np.abs(got - val[:rows, :C]).max()
                assert np.all(np.isfinite(maps.host()))                         # pre-poisoned with NaN: fully overwritten
                gx = _bwd(maps, xd, yd, lay, C, Cp, rows, H, W)
                gref = grad[:rows, :C] * (float(rows_all * C_all) / (rows * C))    # the loss of the first rows and channels alone
                eg = R.field_grad_error(_valid(gx, lay, C), gref)
                worst[kind] = tuple(max(a, b) for a, b in zip(worst.get(kind, (0.0, 0.0)), (ev, eg)))
                assert ev <= VALUE_TOL and eg <= GRAD_TOL, (kind, lay, C, Cp, rows, ev, eg)
                if lay == "nhwc":
                    assert np.all(gx[..., C:] == 0)                             # padded channels: exactly 0, never NaN
                plain, none, name = _fwd(xd, yd, lay, lay, C, rows, H, W)        # dmaps = NULL: the same bits
                assert none is None and name == "ssim_fwd<%s, %s> + ssim_fold" % (c4, c4)
                assert np.array_equal(plain.view(np.uint32), got.view(np.uint32))
    for kind, (ev, eg) in sorted(worst.items()):
        print("%dx%d %s: mean S / cs error %.3e (allowed %.3e; float32 NumPy without the pivot needs %.3e), gradient error %.3e "
              "(allowed %.3e; float32 NumPy needs %.3e)" % (H, W, kind, ev, VALUE_TOL, R.FP32_VALUE_ERR, eg, GRAD_TOL, R.FP32_GRAD_ERR))
    Buf.check_all()


@pytest.mark.parametrize("H, W", R.SHAPES)
def test_repeatable_and_the_same_bits_in_every_layout(H, W):
    x, y, val, _ = _case("smooth_noise", H, W, 3, 3)
    res = {}
    for lay, Cp in (("nhwc", 4), ("nchw", 3), ("nhwc", 16)):
        xd, yd = _device(x, lay, 3, Cp), _device(y, lay, 3, Cp)
        out, maps, _ = _fwd(xd, yd, lay, lay, 3, 3, H, W, want_maps=True)
        gx = _valid(_bwd(maps, xd, yd, lay, 3, Cp, 3, H, W), lay, 3)
        res[lay, Cp] = (out.view(np.uint32), maps.host().view(np.uint32), np.ascontiguousarray(gx).view(np.uint32))
        if (lay, Cp) == ("nhwc", 4):
            out2, maps2, _ = _fwd(xd, yd, lay, lay, 3, 3, H, W, want_maps=True)  # a second run
            gx2 = _valid(_bwd(maps2, xd, yd, lay, 3, Cp, 3, H, W), lay, 3)
            for a, b in zip(res[lay, Cp], (out2.view(np.uint32), maps2.host().view(np.uint32), np.ascontiguousarray(gx2).view(np.uint32))):
                assert np.array_equal(a, b)
    for key in (("nchw", 3), ("nhwc", 16)):
        for a, b in zip(res["nhwc", 4], res[key]):
            assert np.array_equal(a, b), key
    # x NHWC against y NCHW
    mixed, _, name = _fwd(_device(x, "nhwc", 3, 4), _device(y, "nchw", 3, 3), "nhwc", "nchw", 3, 3, H, W)
    assert name == "ssim_fwd<c4, strided> + ssim_fold" and np.array_equal(mixed.view(np.uint32), res["nhwc", 4][0])
    mixed, _, name = _fwd(_device(x, "nchw", 3, 3), _device(y, "nhwc", 3, 4), "nchw", "nhwc", 3, 3, H, W)
    assert name == "ssim_fwd<strided, c4> + ssim_fold" and np.array_equal(mixed.view(np.uint32), res["nhwc", 4][0])
    Buf.check_all()


@pytest.mark.parametrize("H, W", [(12, 17), (R.TILE_H + 11, R.TILE_W + 9), (43, 37)])
def test_pairing_members_with_one_truth(H, W):
    from dtgan_amd import ops
    x, _, _, _ = _case("smooth_noise", H, W, 3, 3)
    y = R.make_pair("smooth_noise", H, W, rows=1, C=3, seed=7)[1]
    want = R.ssim(x, y, x_per_y=3)
    for lay_x, Cp_x, lay_y, Cp_y in (("nhwc", 4, "nchw", 3), ("nchw", 3, "nchw", 3), ("nhwc", 4, "nhwc", 4)):
        xd, yd = _device(x, lay_x, 3, Cp_x), _device(y, lay_y, 3, Cp_y)
        got, _, _ = _fwd(xd, yd, lay_x, lay_y, 3, 3, H, W, x_per_y=3)
        assert np.abs(got - want).max() <= VALUE_TOL
        via_ops = ops.ssim(xd, yd, 3, lay_x, lay_y, x_per_y=3)
        assert via_ops.shape == (3, 3, 2) and via_ops.dtype == torch.float32 and not via_ops.requires_grad
        assert np.array_equal(via_ops.cpu().numpy().view(np.uint32), got.view(np.uint32))
        for r in range(3):                                                      # a member alone against the truth: the same bits
            alone, _, _ = _fwd(xd[r:r + 1].contiguous(), yd, lay_x, lay_y, 3, 1, H, W)
            assert np.array_equal(alone[0].view(np.uint32), got[r].view(np.uint32))
    Buf.check_all()


def test_data_range_and_out():
    from dtgan_amd import ops
    x, y, _, _ = _case("uniform", 43, 37, 3, 3)
    xd, yd = _device(x, "nhwc", 3, 4), _device(y, "nhwc", 3, 4)
    for L in (1.0, 255.0):
        got = ops.ssim(xd, yd, 3, "nhwc", "nhwc", data_range=L).cpu().numpy()
        assert np.abs(got - R.ssim(x, y, data_range=L)).max() <= VALUE_TOL
    out = torch.full((3, 3, 2), float("nan"), device="cuda")
    assert ops.ssim(xd, yd, 3, "nhwc", "nhwc", out=out) is out and torch.equal(out, ops.ssim(xd, yd, 3, "nhwc", "nhwc"))
    same = ops.ssim(xd, xd.clone(), 3, "nhwc", "nhwc").cpu().numpy()
    assert np.abs(same - 1.0).max() <= 4 * EPS                                  # SSIM(x, x) = 1 = cs


def test_an_upstream_gradient_scales_the_gradient():
    x, y, _, _ = _case("smooth_noise", 43, 37, 3, 3)
    for lay, C, Cp in LAYOUTS:
        xd, yd = _device(x, lay, C, Cp), _device(y, lay, C, Cp)
        _, maps, _ = _fwd(xd, yd, lay, lay, C, 3, 43, 37, want_maps=True)
        one = _bwd(maps, xd, yd, lay, C, Cp, 3, 43, 37)
        quarter = _bwd(maps, xd, yd, lay, C, Cp, 3, 43, 37, g=0.25)
        assert np.array_equal(quarter, one * np.float32(0.25)), (lay, C)         # a power of two: exact
        third = _bwd(maps, xd, yd, lay, C, Cp, 3, 43, 37, g=0.37)
        want = one.astype(np.float64) * float(np.float32(0.37))
        assert np.all(np.abs(third - want) <= 4 * EPS * np.abs(want)), (lay, C)
    Buf.check_all()


@pytest.mark.parametrize("kind, H, W", [("smooth_noise", 43, 37), ("near_flat", 64, 64), ("step", 27, 41)])
def test_ops_ssim_loss_and_its_gradient(kind, H, W, monkeypatch):
    from dtgan_amd import ops
    x, y, val, gref = _case(kind, H, W, 3, 3)
    ref = 1.0 - val[..., 0].mean()
    seen = []
    real_call = ops._ssim_call
    monkeypatch.setattr(ops, "_ssim_call", lambda *a: (seen.append(a[-1]), real_call(*a))[1])
    for lay, Cp in (("nhwc", 4), ("nchw", 3)):
        xd = _device(x, lay, 3, Cp).requires_grad_()
        yd = _device(y, lay, 3, Cp)
        loss = ops.ssim_loss(xd, yd, 3, lay)
        assert loss.shape == () and loss.is_cuda and loss.requires_grad
        assert seen[-1] is not None and tuple(seen[-1].shape) == (3, 3, 3, H - 10, W - 10)
        (loss * 0.25).backward()
        ev = abs(float(loss.detach()) - ref)
        gx = xd.grad.cpu().numpy()
        eg = R.field_grad_error(_valid(gx, lay, 3), 0.25 * gref)
        print("%s %dx%d %s: loss %.7f (reference %.7f, error %.3e, allowed %.3e), gradient error %.3e (allowed %.3e)"
              % (kind, H, W, lay, float(loss.detach()), ref, ev, VALUE_TOL, eg, GRAD_TOL))
        assert ev <= VALUE_TOL and eg <= GRAD_TOL
        if lay == "nhwc":
            assert np.all(gx[..., 3:] == 0)
        with torch.no_grad():
            plain = ops.ssim_loss(xd, yd, 3, lay)
        assert seen[-1] is None                                                 # no gradient wanted: no maps are allocated
        assert not plain.requires_grad and torch.equal(plain, loss.detach())
        also = ops.ssim_loss(xd.detach(), yd, 3, lay)
        assert seen[-1] is None and not also.requires_grad
        assert torch.equal(1.0 - ops.ssim(xd, yd, 3, lay, lay)[:, :, 0].mean(), plain)


def test_the_entries_refuse_bad_arguments_before_launching():
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    P = ops._ptr
    x = torch.zeros(1 << 16, device="cuda")
    y = torch.zeros(1 << 16, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    out = torch.full((1 << 16,), -7.0, device="cuda")
    maps = torch.full((1 << 16,), -7.0, device="cuda")
    one = torch.ones(1, device="cuda")
    st = ops._stream()
    need = lib.acg_ssim_workspace_bytes(1, 1, 64, 64)
    assert need == 16 * 4 * 2
    # H, W, rows, x_per_y, C, row stride, pixel stride, data_range, x, y, out, maps, workspace, bytes, rc, what the message names
    cases = ((10, 64, 1, 1, 1, 4096, 1, 2.0, x, y, out, maps, ws, need, -1, "11 <= H, W"), (64, 10, 1, 1, 1, 4096, 1, 2.0, x, y, out, maps, ws, need, -1, "11 <= H, W"),
             (1025, 64, 1, 1, 1, 4096, 1, 2.0, x, y, out, maps, ws, 1 << 20, -1, "1025"), (64, 1025, 1, 1, 1, 4096, 1, 2.0, x, y, out, maps, ws, 1 << 20, -1, "1025"),
             (64, 64, 0, 1, 1, 4096, 1, 2.0, x, y, out, maps, ws, need, -1, "rows >= 1"), (64, 64, 1, 1, 0, 4096, 1, 2.0, x, y, out, maps, ws, need, -1, "C >= 1"),
             (64, 64, 1, 1, 1, 0, 1, 2.0, x, y, out, maps, ws, need, -1, "strides"), (64, 64, 1, 1, 1, 4096, 0, 2.0, x, y, out, maps, ws, need, -1, "strides"),
             (64, 64, 3, 2, 1, 4096, 1, 2.0, x, y, out, maps, ws, 3 * need, -1, "x_per_y"), (64, 64, 1, 0, 1, 4096, 1, 2.0, x, y, out, maps, ws, need, -1, "x_per_y"),
             (64, 64, 1, 1, 1, 4096, 1, 0.0, x, y, out, maps, ws, need, -1, "data_range"), (64, 64, 1, 1, 1, 4096, 1, -2.0, x, y, out, maps, ws, need, -1, "data_range"),
             (64, 64, 1, 1, 1, 4096, 1, float("nan"), x, y, out, maps, ws, need, -1, "data_range"),
             (64, 64, 1, 1, 1, 4096, 1, float("inf"), x, y, out, maps, ws, need, -1, "data_range"),
             (64, 64, 1, 1, 1, 4096, 1, 2.0, None, y, out, maps, ws, need, -1, "null"), (64, 64, 1, 1, 1, 4096, 1, 2.0, x, None, out, maps, ws, need, -1, "null"),
             (64, 64, 1, 1, 1, 4096, 1, 2.0, x, y, None, maps, ws, need, -1, "null"), (64, 64, 1, 1, 1, 4096, 1, 2.0, x, y, x, maps, ws, need, -1, "alias"),
             (64, 64, 1, 1, 1, 4096, 1, 2.0, x, y, out, y, ws, need, -1, "alias"), (64, 64, 1, 1, 1, 4096, 1, 2.0, x, y, out, out, ws, need, -1, "alias"),
             (64, 64, 1, 1, 1, 4096, 1, 2.0, x, y, out, maps, ws, need - 1, -2, "workspace"), (64, 64, 1, 1, 1, 4096, 1, 2.0, x, y, out, maps, None, 0, -2, "workspace"))
    for H, W, rows, per, C, rs, ps, L, xa, ya, oa, ma, wa, nbytes, rc_want, word in cases:
        rc = lib.acg_ssim(P(xa), P(ya), rows, per, C, H, W, rs, ps, 4096, 4096, 1, 4096, L, P(oa), P(ma), P(wa), nbytes, st)
        msg = lib.acg_last_error().decode()
        assert rc == rc_want and msg.startswith("acg_ssim:") and word in msg, (H, W, rows, per, C, L, rc, msg)
    rc = lib.acg_ssim(P(x), P(y), 1, 1, 1, 64, 64, 4096, 1, 4096, 4096, 1, 4096, 2.0, P(out), None, ctypes_at(ws, 4), need, st)
    assert rc == -1 and "aligned" in lib.acg_last_error().decode()
    for args in ((1, 1, 10, 64), (1, 1, 64, 1025), (0, 1, 64, 64), (1, 0, 64, 64)):
        assert lib.acg_ssim_workspace_bytes(*args) == 0
    # rows, C, Cp, H, W, row stride, pixel stride, channel stride, maps, x, y, g, gx, what the message names
    bwd = ((0, 1, 1, 64, 64, 4096, 1, 4096, maps, x, y, one, out, "rows >= 1"), (1, 0, 1, 64, 64, 4096, 1, 4096, maps, x, y, one, out, "C <= Cp"),
           (1, 2, 1, 64, 64, 8192, 1, 4096, maps, x, y, one, out, "C <= Cp"), (1, 1, 1, 10, 64, 4096, 1, 4096, maps, x, y, one, out, "11 <= H, W"),
           (1, 1, 1, 64, 1025, 4096, 1, 4096, maps, x, y, one, out, "1025"), (1, 1, 1, 64, 64, 0, 1, 4096, maps, x, y, one, out, "strides"),
           (1, 1, 1, 64, 64, 4096, 0, 4096, maps, x, y, one, out, "strides"), (1, 1, 1, 64, 64, 4096, 1, 0, maps, x, y, one, out, "strides"),
           (1, 1, 1, 64, 64, 4096, 1, 4096, None, x, y, one, out, "null"), (1, 1, 1, 64, 64, 4096, 1, 4096, maps, None, y, one, out, "null"),
           (1, 1, 1, 64, 64, 4096, 1, 4096, maps, x, None, one, out, "null"), (1, 1, 1, 64, 64, 4096, 1, 4096, maps, x, y, None, out, "null"),
           (1, 1, 1, 64, 64, 4096, 1, 4096, maps, x, y, one, None, "null"), (1, 1, 1, 64, 64, 4096, 1, 4096, maps, x, y, one, x, "alias"),
           (1, 1, 1, 64, 64, 4096, 1, 4096, maps, x, y, one, maps, "alias"))
    for rows, C, Cp, H, W, rs, ps, cs, ma, xa, ya, ga, oa, word in bwd:
        rc = lib.acg_ssim_bwd(P(ma), P(xa), P(ya), P(ga), rows, C, Cp, H, W, rs, ps, cs, 4096, 1, 4096, P(oa), st)
        msg = lib.acg_last_error().decode()
        assert rc == -1 and msg.startswith("acg_ssim_bwd") and word in msg, (rows, C, Cp, H, W, rc, msg)
    torch.cuda.synchronize()
    assert torch.all(out == -7.0) and torch.all(maps == -7.0) and torch.all(x == 0) and torch.all(y == 0)   # nothing was written
    # ops: refused before any device is asked (host tensors)
    small, big, ok = torch.zeros(1, 1, 10, 64), torch.zeros(1, 1, 64, 1025), torch.zeros(2, 1, 16, 16)
    for t in (small, big):
        with pytest.raises(_lib.AcgError, match="11 <= H, W"):
            ops.ssim(t, t, 1, "nchw", "nchw")
        with pytest.raises(_lib.AcgError, match="11 <= H, W"):
            ops.ssim_loss(t, t, 1, "nchw")
    with pytest.raises(_lib.AcgError, match="do not pair"):
        ops.ssim(ok, torch.zeros(2, 1, 16, 17), 1, "nchw", "nchw")                # a size mismatch
    with pytest.raises(_lib.AcgError, match="do not pair"):
        ops.ssim_loss(ok, torch.zeros(1, 1, 16, 16), 1, "nchw")
    with pytest.raises(_lib.AcgError, match="x_per_y"):
        ops.ssim(torch.zeros(3, 1, 16, 16), ok, 1, "nchw", "nchw", x_per_y=2)
    with pytest.raises(_lib.AcgError, match="do not pair"):
        ops.ssim(ok, ok, 1, "nchw", "nchw", x_per_y=2)
    with pytest.raises(_lib.AcgError, match="out"):
        ops.ssim(ok, ok, 1, "nchw", "nchw", out=torch.zeros(2, 1, 3))
    for L in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.AcgError, match="data_range"):
            ops.ssim(ok, ok, 1, "nchw", "nchw", data_range=L)
        with pytest.raises(_lib.AcgError, match="data_range"):
            ops.ssim_loss(ok, ok, 1, "nchw", data_range=L)
    with pytest.raises(_lib.AcgError, match="layout"):
        ops.ssim(ok, ok, 1, "chwn", "nchw")
    with pytest.raises(_lib.AcgError, match="stored channels"):
        ops.ssim(ok, ok, 2, "nchw", "nchw")
    with pytest.raises(_lib.AcgError, match="ROCm device"):
        ops.ssim(ok, ok, 1, "nchw", "nchw")                                     # a host tensor
    with pytest.raises(_lib.AcgError, match="ROCm device"):
        ops.ssim_loss(ok, ok.cuda(), 1, "nchw")


def ctypes_at(t, offset):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + offset)
