"""GPU tests of the marginal loss: acg_field_sort, acg_marginal_loss_fwd and acg_marginal_loss_bwd against
tests/marginal_ref.py, ops.field_sort / ops.marginal_loss against the same, the training step with --lambda_marg_A /
--lambda_marg_B (eager, captured, deferred and under the forced one-rank exchange) and `python -m dtgan_amd.train
--lambda_marg_B` in a child process."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import marginal_ref as R
from field_cases import field_operand as _device, strides as _strides, valid as _valid
from guard_util import Buf
from model_cases import BASE_KEYS, check_captured_and_deferred, flat as _flat, forced_pair, run_module, step_inputs as _inputs, step_model as _model

pytestmark = pytest.mark.gpu

T = 8192                                                            # the shipped LDS chunk, in words (csrc/marginal.hip MS_T)
# (H, W): one pixel; a small power of two; a padded field; Ppad = T unpadded and padded (the largest single launch);
# a padded field whose padding crosses into the chain; Ppad = 2 T (the first global stride); Ppad = 4 T padded (nested stages,
# two global strides in one launch); Ppad = 8 T padded (a stage of a fused pair of strides and a single one)
SHAPES = [(1, 1), (16, 16), (17, 13), (64, 128), (90, 90), (96, 96), (128, 128), (160, 200), (250, 260)]
LAYOUTS = [("nhwc", 3, 4), ("nhwc", 1, 16), ("nchw", 3, 3), ("nchw", 1, 1)]
ROWS = (1, 3)
# |loss - loss64| / loss64 of ops.marginal_loss.  Measured, not chosen: the loss in float32 with torch on the CPU (sort, mean
# over the rows, mean of the squares) needs 1.0973e-7 over the batches of marginal_ref.LOSS_CASES (`python
# tools/marginal_step_cost.py --cpu-tolerance`; the largest is the 17 x 13 batch).  The constant is 4 x that: a different
# summation order.
LOSS_VALUE_TOL = 4 * 1.0973e-7
EPS = 2.0 ** -24


def _ppad(P):
    return 1 << (P - 1).bit_length() if P > 1 else 1


def _launches(Ppad):
    m = max(Ppad // T, 1).bit_length() - 1
    return 1 + sum((s + 1) // 2 + 1 for s in range(1, m + 1))     # per merge stage: its s global strides in pairs, the LDS finish


@functools.lru_cache(maxsize=None)
def _case(kind, H, W):
    """the fields (3, 3, H, W) with their reference values and ranks"""
    x = R.make_fields(kind, H, W, rows=3, C=3)
    x.setflags(write=False)
    return (x,) + R.sort_fields(x)


def _sort(xd, C, layout, want_rank=True):
    """acg_field_sort through the C ABI into poisoned, guarded buffers -> (sorted, rank or None) on the host"""
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    if layout == "nhwc":
        rows, H, W, Cp = xd.shape
    else:
        rows, Cp, H, W = xd.shape
    st = _strides(layout, C, Cp, H, W)
    n = rows * C * H * W
    srt, rank = Buf.out(n), (Buf.out(n, np.int32) if want_rank else None)
    need = lib.acg_field_sort_workspace_bytes(rows, C, H, W)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    rc = lib.acg_field_sort(ops._ptr(xd), rows, C, H, W, st[0], st[1], st[2], srt.ptr, rank.ptr if want_rank else None,
                            ops._ptr(ws) if need else None, need, ops._stream())
    assert rc == 0, lib.acg_last_error().decode()
    return srt.host((rows, C, H * W)), (rank.host((rows, C, H * W)) if want_rank else None)


# --------------------------------------------------------------------------------------------------------------- sort
@pytest.mark.parametrize("H, W", SHAPES)
def test_sort_is_the_reference_bit_for_bit(H, W):
    for kind in R.FIELD_KINDS:
        x, s_ref, r_ref = _case(kind, H, W)
        for rows in ROWS:
            for lay, C, Cp in LAYOUTS:
                s, r = _sort(_device(x[:rows], lay, C, Cp), C, lay)
                assert np.array_equal(s.view(np.uint32), s_ref[:rows, :C].view(np.uint32)), (kind, rows, lay, C, Cp)
                assert np.array_equal(r, r_ref[:rows, :C]), (kind, rows, lay, C, Cp)
    Buf.check_all()


@pytest.mark.parametrize("H, W", SHAPES)
def test_the_path_a_size_takes_and_the_workspaces(H, W):
    from dtgan_amd import _lib
    x = _case("uniform", H, W)[0]
    _sort(_device(x[:1], "nchw", 1, 1), 1, "nchw")
    k = _lib.query("acg_last_kernel").decode()
    Ppad = _ppad(H * W)
    if Ppad <= T:
        assert k == "marginal_sort<x, unpack>" and _launches(Ppad) == 1, k
    else:
        assert k == "marginal_sort<x, words> + marginal_merge chain: %d launches" % _launches(Ppad), k
    assert {T: 1, 2 * T: 3, 4 * T: 5, 8 * T: 8}.get(Ppad, 1) == _launches(Ppad)
    for rows, C in ((1, 1), (3, 3)):
        assert _lib.query("acg_field_sort_workspace_bytes", rows, C, H, W) == (0 if Ppad <= T else 8 * rows * C * Ppad)
    assert _lib.query("acg_marginal_loss_workspace_bytes", 3, H * W) == 4096
    Buf.check_all()


@pytest.mark.parametrize("H, W", SHAPES)
def test_sort_is_repeatable_the_same_in_both_layouts_and_works_without_ranks(H, W):
    x = _case("tanh_normal", H, W)[0]
    nhwc = _device(x, "nhwc", 3, 4)
    a, ra = _sort(nhwc, 3, "nhwc")
    b, rb = _sort(nhwc, 3, "nhwc")
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(ra, rb)
    c, rc = _sort(_device(x, "nchw", 3, 3), 3, "nchw")
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32)) and np.array_equal(ra, rc)
    wide, rw = _sort(_device(x, "nhwc", 3, 16, seed=1), 3, "nhwc")             # other garbage in other padded channels
    assert np.array_equal(a.view(np.uint32), wide.view(np.uint32)) and np.array_equal(ra, rw)
    alone, none = _sort(nhwc, 3, "nhwc", want_rank=False)                      # rank = NULL
    assert none is None and np.array_equal(a.view(np.uint32), alone.view(np.uint32))
    Buf.check_all()


def test_ops_field_sort():
    from dtgan_amd import ops
    x, s_ref, r_ref = _case("masked", 96, 96)
    for lay, C, Cp in LAYOUTS:
        s, r = ops.field_sort(_device(x, lay, C, Cp), C, lay)
        assert s.dtype == torch.float32 and r.dtype == torch.int32 and not s.requires_grad
        assert np.array_equal(s.cpu().numpy().view(np.uint32), s_ref[:, :C].view(np.uint32)) and np.array_equal(r.cpu().numpy(), r_ref[:, :C])
        s2, none = ops.field_sort(_device(x, lay, C, Cp), C, lay, want_rank=False)
        assert none is None and torch.equal(s, s2)


# --------------------------------------------------------------------------------------------------------------- loss
def _loss_abi(x, y, lay, C, Cp, gscale=1.0):
    """the three entries through the C ABI -> (d (C, P), loss, gx in the layout of x), host arrays"""
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    rows, _, H, W = x.shape
    P = H * W
    xd, yd = _device(x, lay, C, Cp), _device(y, lay, C, Cp, seed=4)
    sx, rank = ops.field_sort(xd, C, lay)
    sy, _ = ops.field_sort(yd, C, lay, want_rank=False)
    d, loss, gx = Buf.out(C * P), Buf.out(1), Buf.out(xd.numel())
    need = lib.acg_marginal_loss_workspace_bytes(C, P)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = lib.acg_marginal_loss_fwd(ops._ptr(sx), rows, ops._ptr(sy), y.shape[0], C, P, d.ptr, loss.ptr, ops._ptr(ws), need, ops._stream())
    assert rc == 0, lib.acg_last_error().decode()
    g = torch.full((1,), gscale, device="cuda")
    st = _strides(lay, C, Cp, H, W)
    rc = lib.acg_marginal_loss_bwd(d.ptr, ops._ptr(rank), ops._ptr(g), rows, C, Cp, H, W, st[0], st[1], st[2], gx.ptr, ops._stream())
    assert rc == 0, lib.acg_last_error().decode()
    assert _lib.query("acg_last_kernel").decode() == ("marginal_bwd<c4>" if (lay, Cp) == ("nhwc", 4) else "marginal_bwd<scalar>")
    return d.host((C, P)), float(loss.host()[0]), gx.host(tuple(xd.shape))


@pytest.mark.parametrize("H, W, rows_x, rows_y", R.LOSS_CASES)
def test_loss_difference_and_gradient_match_the_reference(H, W, rows_x, rows_y):
    x, y = R.loss_batches(H, W, rows_x, rows_y)
    for lay, C, Cp in LAYOUTS:
        ref, gref, d64 = R.marginal_loss_and_grad(x[:, :C], y[:, :C])
        d, loss, gx = _loss_abi(x, y, lay, C, Cp)
        top = max(np.abs(x[:, :C]).max(), np.abs(y[:, :C]).max())
        # two fp32 sums of R terms, two divisions and one subtraction
        d_bound = (rows_x + rows_y + 4) * EPS * top
        g_bound = 2.0 / (C * H * W * rows_x) * (d_bound + 4 * EPS * np.abs(d64).max())
        ed, eg, ev = np.abs(d - d64).max(), np.abs(_valid(gx, lay, C) - gref).max(), abs(loss - ref) / ref
        print("%dx%d %s C=%d Cp=%d: d error %.3e (allowed %.3e), gradient error %.3e (allowed %.3e), loss %.6g (reference %.6g, "
              "relative error %.3e, allowed %.3e)" % (H, W, lay, C, Cp, ed, d_bound, eg, g_bound, loss, ref, ev, LOSS_VALUE_TOL))
        assert ed <= d_bound and eg <= g_bound and ev <= LOSS_VALUE_TOL, (H, W, lay, C, Cp, ed, eg, ev)
        if lay == "nhwc":
            assert np.all(gx[..., C:] == 0)                                     # padded channels: exactly 0
    Buf.check_all()


def test_loss_is_repeatable_and_the_same_in_both_layouts():
    x, y = R.loss_batches(96, 96, 3, 2)
    a = _loss_abi(x, y, "nhwc", 3, 4)
    b = _loss_abi(x, y, "nhwc", 3, 4)
    c = _loss_abi(x, y, "nchw", 3, 3)
    assert a[1] == b[1] == c[1]
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[0].view(np.uint32), c[0].view(np.uint32))
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    assert np.array_equal(_valid(a[2], "nhwc", 3).view(np.uint32), c[2].view(np.uint32))
    Buf.check_all()


def test_an_upstream_gradient_scales_the_gradient():
    x, y = R.loss_batches(17, 13)
    for lay, C, Cp in LAYOUTS:
        one = _loss_abi(x, y, lay, C, Cp)[2]
        for g in (0.5, -3.0, 0.37):
            got = _loss_abi(x, y, lay, C, Cp, gscale=g)[2]
            want = one.astype(np.float64) * float(np.float32(g))
            assert np.all(np.abs(got - want) <= EPS * np.abs(want)), (lay, C, g)   # one rounding
    Buf.check_all()


@pytest.mark.parametrize("H, W", [(17, 13), (96, 96)])
def test_ops_marginal_loss_and_its_gradient(H, W):
    from dtgan_amd import ops
    x, y = R.loss_batches(H, W, 3, 2)
    ref, gref, d64 = R.marginal_loss_and_grad(x, y)
    top = max(np.abs(x).max(), np.abs(y).max())
    g_bound = 2.0 / (3 * H * W * 3) * ((3 + 2 + 4) * EPS * top + 4 * EPS * np.abs(d64).max())
    for lay, Cp in (("nhwc", 4), ("nchw", 3)):
        xd = _device(x, lay, 3, Cp).requires_grad_()
        yd = _device(y, lay, 3, Cp, seed=4)
        loss = ops.marginal_loss(xd, yd, 3, lay)
        assert loss.shape == () and loss.is_cuda and loss.requires_grad
        (loss * 2.0).backward()
        assert abs(float(loss.detach()) - ref) / ref <= LOSS_VALUE_TOL
        gx = xd.grad.cpu().numpy()
        assert np.abs(_valid(gx, lay, 3) - 2.0 * gref).max() <= 2.0 * g_bound
        if lay == "nhwc":
            assert np.all(gx[..., 3:] == 0)
        with torch.no_grad():
            plain = ops.marginal_loss(xd, yd, 3, lay)
        assert not plain.requires_grad and torch.equal(plain, loss.detach())
        same = _device(x, lay, 3, Cp).requires_grad_()
        zero = ops.marginal_loss(same, same.detach().clone(), 3, lay)
        zero.backward()
        assert float(zero.detach()) == 0.0 and torch.all(same.grad == 0)        # identical batches: exactly zero


# ---------------------------------------------------------------------------------------------------------- refusals
def test_the_entries_refuse_bad_arguments_before_launching():
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    P = ops._ptr
    x = torch.zeros(1 << 16, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    out = torch.full((1 << 16,), -7.0, device="cuda")
    rank = torch.full((1 << 16,), -7, device="cuda", dtype=torch.int32)
    one = torch.ones(1, device="cuda")
    st = ops._stream()
    need = lib.acg_field_sort_workspace_bytes(1, 1, 128, 128)
    assert need == 8 * 16384
    # H, W, rows, C, row stride, pixel stride, x, sorted, rank, workspace, bytes, rc, what the message names
    sort_cases = ((0, 16, 1, 1, 256, 1, x, out, rank, ws, 0, -1, "pixels"), (2048, 1024, 1, 1, 256, 1, x, out, rank, ws, 0, -1, "pixels"),
                  (1025, 1024, 1, 1, 256, 1, x, out, rank, ws, ws.numel(), -1, "1025"), (16, 16, 0, 1, 256, 1, x, out, rank, ws, 0, -1, "rows >= 1"),
                  (16, 16, 1, 0, 256, 1, x, out, rank, ws, 0, -1, "C >= 1"), (16, 16, 1, 1, 0, 1, x, out, rank, ws, 0, -1, "strides"),
                  (16, 16, 1, 1, 256, 0, x, out, rank, ws, 0, -1, "strides"), (16, 16, 1, 1, 256, 1, None, out, rank, ws, 0, -1, "null"),
                  (16, 16, 1, 1, 256, 1, x, None, rank, ws, 0, -1, "null"), (16, 16, 1, 1, 256, 1, x, x, rank, ws, 0, -1, "alias"),
                  (128, 128, 1, 1, 16384, 1, x, out, rank, ws, need - 1, -2, "workspace"),
                  (128, 128, 1, 1, 16384, 1, x, out, rank, None, 0, -2, "workspace"))
    for H, W, rows, C, rs, ps, xa, sa, ra, wa, nbytes, rc_want, word in sort_cases:
        rc = lib.acg_field_sort(P(xa), rows, C, H, W, rs, ps, max(H * W, 1), P(sa), P(ra), P(wa), nbytes, st)
        msg = lib.acg_last_error().decode()
        assert rc == rc_want and msg.startswith("acg_field_sort") and word in msg, (H, W, rows, C, rc, msg)
    rc = lib.acg_field_sort(P(x), 1, 1, 16, 16, 256, 1, 0, P(out), None, None, 0, st)
    assert rc == -1 and "strides" in lib.acg_last_error().decode()
    for args in ((1, 1, 0, 16), (1, 1, 2048, 1024), (0, 1, 16, 16), (1, 0, 16, 16), (1, 1, 64, 64)):
        assert lib.acg_field_sort_workspace_bytes(*args) == 0
    assert lib.acg_marginal_loss_workspace_bytes(0, 256) == 0 and lib.acg_marginal_loss_workspace_bytes(1, (1 << 20) + 1) == 0
    lneed = lib.acg_marginal_loss_workspace_bytes(1, 256)
    d, loss = out, out[4096:]
    # rows_x, rows_y, C, P, sx, sy, d, loss, workspace, bytes, rc, what the message names
    fwd_cases = ((0, 1, 1, 256, x, x, d, loss, ws, lneed, -1, "rows >= 1"), (1, 0, 1, 256, x, x, d, loss, ws, lneed, -1, "rows >= 1"),
                 (1, 1, 0, 256, x, x, d, loss, ws, lneed, -1, "C >= 1"), (1, 1, 1, 0, x, x, d, loss, ws, lneed, -1, "pixels"),
                 (1, 1, 1, (1 << 20) + 1, x, x, d, loss, ws, lneed, -1, "pixels"), (1, 1, 1, 256, None, x, d, loss, ws, lneed, -1, "null"),
                 (1, 1, 1, 256, x, None, d, loss, ws, lneed, -1, "null"), (1, 1, 1, 256, x, x, None, loss, ws, lneed, -1, "null"),
                 (1, 1, 1, 256, x, x, d, None, ws, lneed, -1, "null"), (1, 1, 1, 256, x, x, x, loss, ws, lneed, -1, "alias"),
                 (1, 1, 1, 256, x, x, d, loss, ws, lneed - 1, -2, "workspace"), (1, 1, 1, 256, x, x, d, loss, None, 0, -2, "workspace"))
    for rx, ry, C, Pn, sxa, sya, da, la, wa, nbytes, rc_want, word in fwd_cases:
        rc = lib.acg_marginal_loss_fwd(P(sxa), rx, P(sya), ry, C, Pn, P(da), P(la), P(wa), nbytes, st)
        msg = lib.acg_last_error().decode()
        assert rc == rc_want and msg.startswith("acg_marginal_loss_fwd") and word in msg, (rx, ry, C, Pn, rc, msg)
    # rows, C, Cp, H, W, row stride, pixel stride, channel stride, d, rank, gscale, gx, what the message names
    bwd_cases = ((0, 1, 1, 16, 16, 256, 1, 256, x, rank, one, out, "rows >= 1"), (1, 0, 1, 16, 16, 256, 1, 256, x, rank, one, out, "C <= Cp"),
                 (1, 2, 1, 16, 16, 512, 1, 256, x, rank, one, out, "C <= Cp"), (1, 1, 1, 0, 16, 256, 1, 256, x, rank, one, out, "pixels"),
                 (1, 1, 1, 2048, 1024, 256, 1, 256, x, rank, one, out, "pixels"), (1, 1, 1, 16, 16, 0, 1, 256, x, rank, one, out, "strides"),
                 (1, 1, 1, 16, 16, 256, 0, 256, x, rank, one, out, "strides"), (1, 1, 1, 16, 16, 256, 1, 0, x, rank, one, out, "strides"),
                 (1, 1, 1, 16, 16, 256, 1, 256, None, rank, one, out, "null"), (1, 1, 1, 16, 16, 256, 1, 256, x, None, one, out, "null"),
                 (1, 1, 1, 16, 16, 256, 1, 256, x, rank, None, out, "null"), (1, 1, 1, 16, 16, 256, 1, 256, x, rank, one, None, "null"),
                 (1, 1, 1, 16, 16, 256, 1, 256, x, rank, one, x, "alias"), (1, 1, 1, 16, 16, 256, 1, 256, x, rank, out, out, "alias"))
    for rows, C, Cp, H, W, rs, ps, cs, da, ra, ga, oa, word in bwd_cases:
        rc = lib.acg_marginal_loss_bwd(P(da), P(ra), P(ga), rows, C, Cp, H, W, rs, ps, cs, P(oa), st)
        msg = lib.acg_last_error().decode()
        assert rc == -1 and msg.startswith("acg_marginal_loss_bwd") and word in msg, (rows, C, Cp, H, W, rc, msg)
    torch.cuda.synchronize()
    assert torch.all(out == -7.0) and torch.all(rank == -7) and torch.all(x == 0)    # nothing was written
    big = torch.zeros(1, 1, 1025, 1024)                                             # a host tensor: refused before any device is asked
    with pytest.raises(_lib.AcgError, match="pixels"):
        ops.field_sort(big, 1, "nchw")
    with pytest.raises(_lib.AcgError, match="pixels"):
        ops.marginal_loss(big, big, 1, "nchw")
    with pytest.raises(_lib.AcgError, match="against fields"):
        ops.marginal_loss(torch.zeros(1, 1, 16, 16, device="cuda"), torch.zeros(1, 1, 16, 8, device="cuda"), 1, "nchw")
    with pytest.raises(_lib.AcgError, match="layout"):
        ops.field_sort(torch.zeros(1, 1, 16, 16, device="cuda"), 1, "chwn")
    with pytest.raises(_lib.AcgError, match="stored channels"):
        ops.field_sort(torch.zeros(1, 1, 16, 16, device="cuda"), 2, "nchw")
    with pytest.raises(_lib.AcgError, match="ROCm device"):
        ops.field_sort(torch.zeros(1, 1, 16, 16), 1, "nchw")


# --------------------------------------------------------------------------------------------------------------- step
MARG = ["Marg_A", "Marg_B"]


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("aug", [True, False])
def test_step_reports_the_reference_losses_and_the_term_enters_loss_G_only(aug, prec):
    from hip_util import precision
    with precision(prec):
        A, B, z = _inputs()
        off, on_B, on_A = _model(aug), _model(aug, lambda_marg_B=0.5), _model(aug, lambda_marg_A=0.5, lambda_marg_B=0.0)
        l0, v0, g0 = off.train_instance(A, B, z)
        assert list(l0.keys()) == BASE_KEYS[aug]                                # the default step: today's dict
        for m in (on_B, on_A):
            l, v, gn = m.train_instance(A, B, z)
            assert list(l.keys()) == BASE_KEYS[aug] + MARG and list(gn.keys()) == list(g0.keys())
            for k in BASE_KEYS[aug]:                                            # the first pass does not see the new term
                assert l[k] == l0[k], (k, l[k], l0[k])
            for k in v0:
                assert torch.equal(v[k], v0[k]), k
            h = {k: t.cpu().numpy() for k, t in v.items()}
            for name, fake, real in (("Marg_A", "fake_A", "real_A"), ("Marg_B", "fake_B", "real_B")):
                ref = R.marginal_loss(h[fake], h[real])
                err = abs(l[name] - ref) / ref
                print("%s %s aug=%d: %.6g (reference %.6g, relative error %.3e, allowed %.3e)" % (name, prec, aug, l[name], ref, err,
                                                                                                 LOSS_VALUE_TOL))
                assert np.isfinite(l[name]) and err <= LOSS_VALUE_TOL, (name, l[name], ref)
        p0, pB, pA = _flat(off), _flat(on_B), _flat(on_A)
        for k in p0:
            if k.startswith("f_D"):                                             # the term enters loss_G only
                assert torch.equal(p0[k], pB[k]) and torch.equal(p0[k], pA[k]), k
        assert not torch.equal(p0["f_G_A_B"], pB["f_G_A_B"])
        assert torch.equal(p0["f_G_B_A"], pB["f_G_B_A"])                        # fake_B does not depend on G_B_A
        assert not torch.equal(p0["f_G_B_A"], pA["f_G_B_A"])


@pytest.mark.parametrize("aug", [True, False])
def test_both_families_name_their_scalars(aug):
    A, B, z = _inputs()
    l, _, _ = _model(aug, lambda_spec_A=0.25, lambda_marg_B=0.5).train_instance(A, B, z)
    assert list(l.keys()) == BASE_KEYS[aug] + ["Spec_A", "Spec_B"] + MARG
    assert all(np.isfinite(l[k]) for k in l)
    l, _, _ = _model(aug, lambda_spec_B=0.25).train_instance(A, B, z)
    assert list(l.keys()) == BASE_KEYS[aug] + ["Spec_A", "Spec_B"]


@pytest.mark.parametrize("aug", [True, False])
def test_captured_and_deferred_steps_with_the_loss_on(aug):
    """two eager warm-up calls, the capture and its replay: the first replayed step runs the eager step's kernels on the eager
    step's numbers, so everything it reports equals the eager model's bit for bit (later steps carry the ulp of the device-side
    bias correction, test_hip_step.py); the deferred scalars are the synchronous graph's; a change of either weight re-captures"""
    check_captured_and_deferred("train_instance", dict(lambda_marg_A=0.25, lambda_marg_B=0.5), BASE_KEYS[aug] + MARG,
                                (("lambda_marg_B", 0.125), ("lambda_marg_A", 0.0)), dict(lambda_marg_B=0.0), BASE_KEYS[aug], aug=aug, steps=5)


def test_the_forced_one_rank_exchange_reports_the_same_scalars(tmp_path):
    """Marg_A / Marg_B ride in the rank-averaged sums of the gradient tail: with one rank and every collective forced
    (test_hip_dp.test_rccl_backend_one_rank_group) the step's scalars are the plain step's.  Step 0 is the same arithmetic on
    the same numbers but for the tail's float64 average of one value: 1e-6 (8 ulp of fp32); step 1 follows an Adam update."""
    plain, forced = forced_pair(tmp_path, "train_instance", dict(lambda_marg_A=0.05, lambda_marg_B=0.1), "29573")
    assert list(plain["s0/names"][-2:]) == MARG and list(forced["s0/names"]) == list(plain["s0/names"])
    print("step 0 largest relative difference %.3e" % np.max(np.abs(forced["s0/losses"] - plain["s0/losses"]) / np.abs(plain["s0/losses"])))
    for k in ("s0/losses", "s0/gnorms"):
        assert np.allclose(forced[k], plain[k], rtol=1e-6, atol=1e-9), (k, forced[k], plain[k])
    for k in ("s1/losses", "s1/gnorms"):
        assert np.allclose(forced[k], plain[k], rtol=3e-3, atol=1e-6), (k, forced[k], plain[k])


# ------------------------------------------------------------------------------------------------------------- driver
def test_train_driver_with_the_marginal_loss(tmp_path):
    out = run_module("train", "--name", "marg", "--checkpoints_dir", tmp_path,
                     "--synthetic", "16", "--grid_size", "64", "--batchSize", "4", "--ngf", "8", "--nef", "8", "--ndf", "8", "--nlatent", "4",
                     "--niter", "1", "--niter_decay", "0", "--print_freq", "8", "--display_freq", "16", "--save_epoch_freq", "1",
                     "--eval_steps", "2", "--num_multi", "2", "--seed", "1", "--lambda_marg_B", "0.1", limit=900)
    d = os.path.join(str(tmp_path), "marg")
    log = open(os.path.join(d, "results.txt")).read()
    lines = [ln for ln in log.splitlines() if re.search(r"\) D_A: ", ln)]          # the loss lines (not the gnorm_D_A ones)
    assert lines and all(re.search(r"P_f_B: \S+ Marg_A: \d+\.\d{3} Marg_B: \d+\.\d{3} $", ln) for ln in lines), lines
    assert "lambda_marg_B: 0.1" in open(os.path.join(d, "opt.txt")).read().splitlines()
    assert re.search(r"Marg_A: \d+\.\d{3}", out) and re.search(r"Marg_B: \d+\.\d{3}", out)   # the print line as well
