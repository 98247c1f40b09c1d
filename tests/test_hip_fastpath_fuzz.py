"""The specialised bf16x3 convolution kernels across the shapes their dispatch predicates accept, against the
same layer in float64 torch (F.conv2d / F.conv_transpose2d, F.pad(mode="reflect"), autograd for dx, dw, db).

Each family has a hand-chosen generator: shapes inside its predicate that walk the free parameters of the kernel's own plan
(conv_rows_x3's rows per workgroup R and chunks per band cpb; the split-K plan of wgrad_plan in conv_api.hip: nsplit, per and
a short last split; workgroup counts on both sides of a multiple of 8 for the XCD-aware tile order, and on both sides of
256 for the persistent kernels), plus neighbours one step outside the predicate, where the family's kernel must NOT run.
The plan is spelled in the test id (R / cpb / wg for the row pipeline, ns / per / last / wg for the kernel-row weight
gradients, mt = 128-pixel output tiles elsewhere), and the row pipeline's R is asserted from its launch note.

Bars (those of test_hip_ops): max-abs error / max-abs value < 2e-5 on y and dx, < 1e-4 on dw and db.  Every module-level case
also runs in strict f32, where none of the fast paths may run and the fallback kernels meet the same bars at the same shapes.

The second half drives the C-ABI entry points with fused side outputs inside their `_supported` predicates: the per-tile
(mean, M2) of acg_conv2d_fwd_stats / acg_conv_transpose2d_fwd_stats merged by acg_norm_stats_from_partials, the
norm-backward sums of acg_conv2d_bwd_data_sums (row pipeline, row-patch tile, four-phase tile, thin-row head) and the
pre-split trunk (acg_conv2d_{fwd,bwd_data,bwd_weight}_s16, _s16_sums, _s16_mask) on frame and un-padded grids.

Seeded: the same cases every run.  The reference runs in float64 on the device (on the host if the device has no fp64
convolution).  243 tests; the whole file takes 22 s on one MI355X (24 s wall with start-up).
"""
import ctypes
import re
import zlib

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conv_cases import (FAST, KROW, KROW_S, KROWG, PATCHN, PH4, ROWS, RP, S16_CASES, THINROW, THINW, WS, _dev_t, _match, _nchw, _nhwc, _pad_c,  # noqa: E402
                        _ref_device)

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------------
# plans, mirrored from the launchers (conv_rows.hip acg_conv_rows_launch, conv_api.hip wgrad_plan)


def _cdiv(a, b):
    return -(-a // b)


def rows_plan(N, H, W):
    """-> (R rows per workgroup, cpb chunks per (image, band), workgroups)"""
    bands = W // 128
    cpb = min(_cdiv(256, N * bands), H // 8)
    cpb = max(cpb, 1)
    R = _cdiv(H, cpb)
    cpb = _cdiv(H, R)
    return R, cpb, N * bands * cpb


def wgrad_plan(fam, K, Cx, Cg, N, Ho, Wo):
    """-> (nsplit, per, pixels of the last split, workgroups) of the kernel-row weight gradients"""
    Mtot = N * Ho * Wo
    if fam == "krow":
        nblk, target, gran = 3 * (Cx // 128) * (Cg // 128), 256, 32
    elif fam == "krow_s":
        nblk, target, gran = 3, 512, 128
    else:   # krowg
        nblk, target, gran = K * (Cx // (64 if Cx == 64 else 128)) * (Cg // 128), 256, Wo
    ns = max(min(target // nblk, Mtot // 1024, 512), 1)
    per = _cdiv(_cdiv(Mtot, ns), gran) * gran
    ns = _cdiv(Mtot, per)
    return ns, per, Mtot - (ns - 1) * per, ns * nblk


# ---------------------------------------------------------------------------------------------------------------------
# module-level cases: (family, inside, K, stride, pad, mode, Ci, Co, N, H, W, transpose)
# transpose: nn.ConvTranspose2d(Ci, Co, 3, 2, 1, output_padding=1) on an N x Ci x H x W input; kernel names: conv_cases

def _c(fam, inside, K, s, p, mode, Ci, Co, N, H, W, tr=False):
    return (fam, inside, K, s, p, mode, Ci, Co, N, H, W, tr)


def _rows_cases():
    out = []
    # forward of the 32 -> 64 layer: H < 8 (one row per chunk), H not a multiple of the chunk, 1 / 2 / 3 / 5 bands,
    # 1, 16, 256 and 270 workgroups
    for N, H, W in [(1, 3, 128), (2, 5, 256), (3, 7, 384), (4, 8, 128), (1, 9, 640), (2, 33, 256), (1, 100, 128),
                    (3, 144, 640), (4, 512, 128)]:
        out.append(_c("rows", True, 3, 1, 1, "zero", 32, 64, N, H, W))
    # data gradient of the 64 -> 32 layer
    for N, H, W in [(1, 4, 128), (2, 6, 384), (3, 17, 256), (4, 40, 640), (1, 200, 256), (2, 260, 640), (4, 63, 128)]:
        out.append(_c("rows", True, 3, 1, 1, "zero", 64, 32, N, H, W))
    # one step outside: width 128 +- 16, 240, reflect padding, 48 written channels
    out += [_c("rows", False, 3, 1, 1, "zero", 32, 64, 2, 9, 112), _c("rows", False, 3, 1, 1, "zero", 32, 64, 1, 10, 144),
            _c("rows", False, 3, 1, 1, "zero", 64, 32, 2, 7, 240), _c("rows", False, 3, 1, 1, "reflect", 32, 64, 1, 9, 128),
            _c("rows", False, 3, 1, 1, "zero", 32, 48, 1, 9, 128)]
    return out


def _ws_cases():
    out = [_c("ws", True, *g) for g in [
        (3, 1, 1, "reflect", 96, 192, 2, 13, 40), (3, 1, 1, "zero", 160, 384, 1, 9, 24), (4, 1, 1, "zero", 128, 128, 3, 11, 19),
        (4, 2, 1, "zero", 64, 128, 2, 34, 50), (3, 2, 1, "zero", 64, 128, 4, 33, 66), (3, 1, 1, "reflect", 32, 128, 1, 64, 72),
        (3, 1, 1, "reflect", 224, 128, 2, 21, 35), (4, 2, 1, "zero", 128, 256, 1, 40, 40), (3, 1, 1, "zero", 128, 160, 3, 7, 129)]]
    # outside: 48 input channels (not a 32-multiple), 96 output columns
    out += [_c("ws", False, 3, 1, 1, "zero", 48, 128, 2, 12, 20), _c("ws", False, 3, 1, 1, "reflect", 128, 96, 1, 14, 18)]
    return out


def _krow_cases():
    out = [_c("krow", True, *g) for g in [
        (3, 1, 1, "zero", 128, 128, 1, 3, 32),       # Mtot 96: nsplit 1
        (3, 1, 1, "reflect", 384, 128, 2, 7, 64),    # 384 channels, nsplit 1
        (3, 1, 1, "reflect", 128, 384, 1, 20, 96),
        (3, 1, 1, "reflect", 128, 128, 3, 45, 96),   # 12 splits of 1088 pixels, a short last one, splits across rows / images
        (3, 1, 1, "zero", 256, 256, 4, 17, 160),
        (3, 1, 1, "zero", 128, 256, 2, 64, 128),
        (3, 1, 1, "reflect", 256, 128, 3, 33, 224)]]
    out += [_c("krow", False, 3, 1, 1, "zero", 128, 128, 2, 10, 48), _c("krow", False, 3, 1, 1, "reflect", 192, 128, 1, 9, 64)]
    return out


def _krows_cases():
    out = [_c("krow_s", True, *g) for g in [
        (3, 1, 1, "reflect", 32, 64, 1, 3, 128), (3, 1, 1, "zero", 64, 32, 3, 11, 384), (3, 1, 1, "reflect", 64, 32, 4, 23, 256),
        (3, 1, 1, "reflect", 32, 64, 2, 51, 640)]]
    out += [_c("krow_s", False, 3, 1, 1, "reflect", 32, 64, 1, 6, 144)]
    return out


def _krowg_cases():
    out = [_c("krowg", True, *g) for g in [
        (4, 1, 1, "zero", 128, 128, 2, 9, 17),      # Wo 16
        (4, 1, 1, "zero", 256, 128, 1, 12, 49),     # Wo 48: a partial last 32-pixel run
        (4, 1, 1, "zero", 128, 256, 3, 10, 64),     # Wo 63
        (4, 1, 1, "zero", 128, 128, 4, 33, 96),     # Wo 95, several splits
        (4, 2, 1, "zero", 128, 128, 2, 32, 64),     # Wo 32
        (4, 2, 1, "zero", 64, 128, 4, 40, 46),      # Wo 23
        (3, 2, 1, "zero", 64, 128, 2, 33, 61),      # Wo 31
        (3, 2, 1, "zero", 64, 256, 1, 64, 96),      # Wo 48
        (3, 2, 1, "zero", 64, 128, 4, 70, 128)]]    # Wo 64, several splits
    # ConvTranspose 128 -> 64 (x-side bias sums): input widths 16, 50, 64
    out += [_c("krowg", True, 3, 2, 1, "zero", 128, 64, 2, 8, 16, True), _c("krowg", True, 3, 2, 1, "zero", 256, 64, 1, 10, 50, True),
            _c("krowg", True, 3, 2, 1, "zero", 128, 64, 3, 21, 64, True)]
    # outside: Wo % 32 == 15, reflect padding, 3x3 stride 2 with 128 input channels, ConvTranspose input width 40 (40 % 32 = 8)
    out += [_c("krowg", False, 4, 1, 1, "zero", 128, 128, 2, 10, 48), _c("krowg", False, 4, 1, 1, "reflect", 128, 128, 1, 9, 33),
            _c("krowg", False, 3, 2, 1, "zero", 128, 128, 1, 20, 64), _c("krowg", False, 3, 2, 1, "zero", 128, 64, 1, 6, 40, True)]
    return out


def _ph4_cases():
    # stride-2 3x3 data gradient with 64 input channels: phase grid width Wo = 128, 256, 384; ConvTranspose ... -> 64
    out = [_c("ph4", True, *g) for g in [
        (3, 2, 1, "zero", 64, 128, 1, 6, 256), (3, 2, 1, "zero", 64, 128, 3, 14, 512), (3, 2, 1, "zero", 64, 96, 2, 10, 256),
        (3, 2, 1, "zero", 64, 256, 1, 8, 768), (3, 2, 1, "zero", 64, 32, 4, 4, 256)]]
    out += [_c("ph4", True, 3, 2, 1, "zero", 128, 64, 1, 5, 128, True), _c("ph4", True, 3, 2, 1, "zero", 256, 64, 2, 3, 256, True),
            _c("ph4", True, 3, 2, 1, "zero", 96, 64, 3, 4, 384, True)]
    # outside: phase grid width 120 / 144, an odd input height, ConvTranspose input width 112
    out += [_c("ph4", False, 3, 2, 1, "zero", 64, 128, 1, 6, 240), _c("ph4", False, 3, 2, 1, "zero", 64, 128, 2, 4, 288),
            _c("ph4", False, 3, 2, 1, "zero", 64, 128, 1, 7, 256), _c("ph4", False, 3, 2, 1, "zero", 128, 64, 1, 4, 112, True)]
    return out


def _thin_cases():
    out = [_c("thin", True, *g) for g in [
        # stem side: C4 image -> 32 channels
        (7, 1, 3, "reflect", 3, 32, 2, 64, 96), (7, 1, 3, "reflect", 3, 32, 1, 45, 130), (3, 1, 1, "zero", 3, 32, 4, 33, 40),
        (5, 1, 2, "reflect", 3, 32, 1, 80, 112), (7, 1, 3, "zero", 1, 32, 2, 20, 28), (2, 1, 0, "zero", 4, 32, 1, 30, 33),
        (7, 1, 3, "reflect", 3, 32, 2, 128, 256),
        # head side: 32 channels -> C4 image
        (7, 1, 3, "zero", 32, 3, 2, 64, 96), (7, 1, 3, "zero", 32, 3, 3, 37, 50), (3, 1, 1, "reflect", 32, 3, 1, 48, 200),
        (6, 1, 2, "zero", 32, 4, 1, 25, 31), (4, 1, 1, "zero", 32, 2, 2, 17, 19), (5, 1, 2, "zero", 32, 1, 1, 96, 160)]]
    # outside: 8 real input channels, 48 on the wide side, a 1x1 head
    out += [_c("thin", False, 7, 1, 3, "reflect", 8, 32, 1, 20, 24), _c("thin", False, 7, 1, 3, "reflect", 3, 48, 1, 20, 24),
            _c("thin", False, 1, 1, 0, "zero", 32, 3, 2, 20, 24)]
    return out


def _expect(case):
    """-> ((forward, data gradient, weight gradient) kernels the case is about, the same passes' kernels it must not run)"""
    fam, inside, K, s, p, mode, Ci, Co, N, H, W, tr = case
    none = (None, None, None)
    if fam == "rows":
        if not inside:   # (the row-patch tile and krow_s need W % 128 == 0 too; at W = 128 they still run)
            other = None if W % 128 == 0 else RP
            krow_s = None if W % 128 == 0 else KROW_S
            return none, ((ROWS, other, krow_s) if Ci == 32 else (other, ROWS, krow_s))
        return ((ROWS, RP, KROW_S) if Ci == 32 else (RP, ROWS, KROW_S)), none
    if fam == "ws":
        dg = WS if (s == 1 and Ci >= 128) else None
        return ((WS, dg, None), none) if inside else (none, (WS, None, None))
    if fam == "krow":
        return ((None, None, KROW), none) if inside else (none, (None, None, KROW))
    if fam == "krow_s":
        return ((None, None, KROW_S), none) if inside else (none, (None, None, KROW_S))
    if fam == "krowg":
        if not inside:
            return none, (None, None, KROWG)
        if tr:
            return (None, None, "wgrad_x3_krowg<NT=3,IS=2,BCI=64>"), none
        return (None, None, "wgrad_x3_krowg<NT=%d,IS=%d,BCI=%d>" % (K, s, 64 if Ci == 64 else 128)), none
    if fam == "ph4":
        if tr:
            return ((PH4, None, None), none) if inside else (none, (PH4, None, None))
        return ((None, PH4, None), none) if inside else (none, (None, PH4, None))
    assert fam == "thin"
    if not inside:
        return none, ((PATCHN, THINROW, THINW) if Co <= 4 else (THINROW, PATCHN, THINW))
    same = 2 * p == K - 1
    if Ci <= 4:   # stem
        return (THINROW, PATCHN, "%s<K=%d,flip=0>" % (THINW, K) if same else None), none
    return (PATCHN, THINROW, "%s<K=%d,flip=1>" % (THINW, K) if same and mode == "zero" else None), none


def _out_hw(case):
    fam, inside, K, s, p, mode, Ci, Co, N, H, W, tr = case
    if tr:
        return 2 * H, 2 * W
    return (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1


def _plan(case):
    fam, inside, K, s, p, mode, Ci, Co, N, H, W, tr = case
    Ho, Wo = _out_hw(case)
    if fam == "rows" and inside:
        Hg, Wg = H, W
        R, cpb, wg = rows_plan(N, Hg, Wg)
        txt = "R%d_cpb%d_wg%d" % (R, cpb, wg)
    else:
        txt = "mt%d" % _cdiv(N * Ho * Wo, 128)
    wfam = {"krow": "krow", "krow_s": "krow_s", "rows": "krow_s", "krowg": "krowg"}.get(fam)
    if inside and wfam is not None:
        if tr:   # the weight gradient of a ConvTranspose is that of the convolution it is the adjoint of
            ns, per, last, wg = wgrad_plan(wfam, K, Co, Ci, N, H, W)
        else:
            ns, per, last, wg = wgrad_plan(wfam, K, Ci, Co, N, Ho, Wo)
        txt += "_ns%d_per%d_last%d_wg%d" % (ns, per, last, wg)
    return txt


def _cid(case):
    fam, inside, K, s, p, mode, Ci, Co, N, H, W, tr = case
    return "%s_%s_%sk%ds%dp%d%s_%dto%d_%dx%dx%d_%s" % (fam, "in" if inside else "out", "T" if tr else "", K, s, p, mode, Ci, Co,
                                                      N, H, W, _plan(case))


CASES = _rows_cases() + _ws_cases() + _krow_cases() + _krows_cases() + _krowg_cases() + _ph4_cases() + _thin_cases()


def test_case_list_is_fixed_and_plans_cover_the_branches():
    """the generators are deterministic and reach the branches the issue names (CPU-side: the plans only)"""
    assert len(set(_cid(c) for c in CASES)) == len(CASES)
    rows = [rows_plan(c[8], c[9], c[10]) for c in CASES if c[0] == "rows" and c[1]]
    assert any(c[9] < 8 for c in CASES if c[0] == "rows" and c[1])
    assert any(wg > 256 for _, _, wg in rows) and any(wg == 256 for _, _, wg in rows) and any(wg < 256 for _, _, wg in rows)
    assert any(wg % 8 for _, _, wg in rows)
    plans = []
    for c in CASES:
        fam, inside, K, s, p, mode, Ci, Co, N, H, W, tr = c
        if inside and fam in ("krow", "krow_s", "krowg"):
            Ho, Wo = _out_hw(c)
            plans.append((fam,) + (wgrad_plan(fam, K, Co, Ci, N, H, W) if tr else wgrad_plan(fam, K, Ci, Co, N, Ho, Wo)))
    for fam in ("krow", "krow_s", "krowg"):
        mine = [q for q in plans if q[0] == fam]
        assert any(ns == 1 for _, ns, _, _, _ in mine), fam
        assert any(ns > 1 and last < per for _, ns, per, last, _ in mine), fam
        assert any(wg % 8 for _, _, _, _, wg in mine), fam
    # a split that crosses an image boundary (kernel-row gradient, 3 x 45 x 96)
    ns, per, last, wg = wgrad_plan("krow", 3, 128, 128, 3, 45, 96)
    assert ns == 12 and per == 1088 and last == 992 and (45 * 96) % per != 0


def _reference(case, x, w, b, r):
    """fp64 forward + autograd for dx, dw, db"""
    fam, inside, K, s, p, mode, Ci, Co, N, H, W, tr = case
    dev = _ref_device()
    X, Wt, B = (torch.tensor(a, dtype=torch.float64, device=dev, requires_grad=True) for a in (x, w, b))
    if tr:
        y = F.conv_transpose2d(X, Wt, B, stride=2, padding=1, output_padding=1)
    elif mode == "reflect":
        y = F.conv2d(F.pad(X, (p, p, p, p), mode="reflect"), Wt, B, stride=s)
    else:
        y = F.conv2d(X, Wt, B, stride=s, padding=p)
    y.backward(torch.tensor(r, dtype=torch.float64, device=dev))
    return [v.detach().cpu().numpy() for v in (y, X.grad, Wt.grad, B.grad)]


def _inputs(case):
    """seeded x, weight, bias and output gradient of a module-level case (NCHW, float64)"""
    fam, inside, K, s, p, mode, Ci, Co, N, H, W, tr = case
    rs = np.random.RandomState(zlib.crc32(_cid(case).encode()))
    x = rs.normal(0, 1, (N, Ci, H, W))
    w = rs.normal(0, 0.3, (Ci, Co, K, K) if tr else (Co, Ci, K, K))
    b = rs.normal(0, 0.5, (Co,))
    Ho, Wo = _out_hw(case)
    r = rs.normal(0, 1, (N, Co, Ho, Wo))
    return x, w, b, r


def _run_module_case(case, prec):
    from hip_util import t, n, Spy, precision
    from dtgan_amd import modules as M
    fam, inside, K, s, p, mode, Ci, Co, N, H, W, tr = case
    x, w, b, r = _inputs(case)
    with precision(prec):
        if tr:
            conv = M.ConvTranspose2d(Ci, Co, 3, stride=2, padding=1, output_padding=1, bias=True).cuda()
            m, pre = conv, "acg_conv_transpose2d_"
        elif mode == "reflect":
            conv = M.Conv2d(Ci, Co, K, stride=s, padding=0, bias=True)
            m, pre = M.Sequential(nn.ReflectionPad2d(p), conv).cuda(), "acg_conv2d_"
        else:
            conv = M.Conv2d(Ci, Co, K, stride=s, padding=p, bias=True)
            m, pre = M.Sequential(conv).cuda(), "acg_conv2d_"
        with torch.no_grad():
            conv.weight.copy_(t(w)); conv.bias.copy_(t(b))
        xt = t(x, grad=True)
        with Spy() as spy:
            y = m(xt)
            y.backward(t(r))
        got = (spy.kernels(pre + "fwd"), spy.kernels(pre + "bwd_data"), spy.kernels(pre + "bwd_weight"))
        res = (n(y), n(xt.grad), n(conv.weight.grad), n(conv.bias.grad))
    print("KERNELS", _cid(case), prec, got)
    return res, got


@pytest.mark.parametrize("prec", ["bf16x3", "f32"])
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_fast_path_against_fp64(case, prec):
    from hip_util import rel
    (y, dx, dw, db), got = _run_module_case(case, prec)
    ref = _reference(case, *_inputs(case))
    want, forbid = _expect(case)
    passes = ("forward", "data gradient", "weight gradient")
    if prec == "bf16x3":
        for wnt, have, what in zip(want, got, passes):
            assert wnt is None or any(_match(wnt, k) for k in have), (what, wnt, have)
        for fb, have, what in zip(forbid, got, passes):
            assert fb is None or not any(_match(fb, k) for k in have), (what, "must not run", fb, have)
        if case[0] == "rows" and case[1]:    # the row pipeline's plan: R rows per workgroup, from its launch note
            R = rows_plan(case[8], case[9], case[10])[0]
            notes = [k for k in got[0] + got[1] if k.startswith(ROWS)]
            assert notes and all(re.search(r"\((\d+) rows per workgroup\)", k).group(1) == str(R) for k in notes), (R, notes)
    else:   # strict f32: the bf16x3-only fast paths must not run
        for have, what in zip(got, passes):
            assert not any(f.lstrip("=") in k for f in FAST for k in have), (what, have)
    for a, b_, name, bar in zip((y, dx, dw, db), ref, ("y", "dx", "dw", "db"), (2e-5, 2e-5, 1e-4, 1e-4)):
        assert a.shape == b_.shape, name
        e = rel(a, b_)
        assert e < bar, (name, e)




# ---------------------------------------------------------------------------------------------------------------------
# fused side outputs through the C ABI

# (K, stride, pad, mode, Ci, Co, N, H, W, transpose) whose forward may emit per-tile statistics
STATS_CASES = [
    (3, 1, 1, "reflect", 96, 192, 2, 16, 40, False),   # wave-specialised, 5 tiles per image
    (3, 1, 1, "reflect", 128, 128, 3, 24, 48, False),  # 9 tiles per image
    (3, 2, 1, "zero", 64, 128, 3, 32, 64, False),      # stride 2: 16 x 32 output
    (4, 2, 1, "zero", 128, 256, 1, 34, 130, False),    # 17 x 65 -> not whole tiles: unsupported (checked below)
    (3, 1, 1, "zero", 32, 64, 2, 9, 256, False),       # row pipeline
    (3, 1, 1, "zero", 32, 64, 4, 40, 384, False),
    (3, 1, 1, "zero", 64, 32, 1, 12, 128, False),      # generic tile (32 written columns)
    (7, 1, 3, "reflect", 3, 32, 2, 16, 32, False),     # thin-row stem: 8 x 16 tiles
    (7, 1, 3, "reflect", 3, 32, 1, 40, 96, False),
    (5, 1, 2, "zero", 3, 32, 3, 24, 48, False),
    (3, 2, 1, "zero", 128, 64, 2, 8, 16, True),        # ConvTranspose: four phase launches, their own chunks each
    (3, 2, 1, "zero", 64, 32, 1, 16, 32, True),
    (3, 2, 1, "zero", 96, 64, 2, 4, 128, True),
]


@pytest.mark.parametrize("case", STATS_CASES, ids=lambda c: "%sk%ds%dp%d%s_%dto%d_%dx%dx%d" % ((("T" if c[9] else ""),) + c[:9]))
def test_forward_tile_statistics_against_fp64(case):
    """acg_conv2d_fwd_stats / acg_conv_transpose2d_fwd_stats: y and the per-tile (mean, M2) the epilogue emits, merged by
    acg_norm_stats_from_partials, against the fp64 mean and biased variance of the fp64 output (1e-4 of the largest)"""
    from dtgan_amd import ops, _lib
    from hip_util import precision, n, rel
    K, s, p, mode, Ci, Co, N, H, W, tr = case
    P = ops._ptr
    rs = np.random.RandomState(zlib.crc32(repr(case).encode()))
    x = rs.normal(0.3, 1, (N, Ci, H, W))
    w = rs.normal(0, 0.2, (Ci, Co, K, K) if tr else (Co, Ci, K, K))
    b = rs.normal(0, 0.5, (Co,))
    with precision("bf16x3"):
        st = ops._stream()
        if tr:
            pk = ops.PackedConv(_dev_t(w), _dev_t(b), ops.cpad(Co), ops.cpad(Ci))
            d = ops.conv_desc(N, 2 * H, 2 * W, pk.Ci, pk.Co, 3, 2, 1, ops.PAD_ZERO)
            assert (d.Ho, d.Wo) == (H, W)
            ok = _lib.query("acg_conv_transpose2d_fwd_stats_supported", ctypes.byref(d))
            Hy, Wy, Cy, Cys = 2 * H, 2 * W, Co, pk.Ci
        else:
            pk = ops.PackedConv(_dev_t(w), _dev_t(b), ops.cpad(Ci), ops.cpad(Co))
            d = ops.conv_desc(N, H, W, pk.Cis, pk.Cos, K, s, p, ops.PAD_REFLECT if mode == "reflect" else ops.PAD_ZERO, Ci, Co)
            ok = _lib.query("acg_conv2d_fwd_stats_supported", ctypes.byref(d))
            Hy, Wy, Cy, Cys = d.Ho, d.Wo, Co, pk.Cos
        whole = (Hy * Wy) % 128 == 0
        assert bool(ok) == whole, (ok, Hy, Wy)
        if not ok:
            return
        xin = _dev_t(_pad_c(_nhwc(x), pk.Co if tr else pk.Cis, 3))
        y = torch.full((N, Hy, Wy, Cys), float("nan"), device="cuda")
        part = torch.full((N, Hy * Wy // 128, 2, Cys), float("nan"), device="cuda")
        if tr:
            _lib.call("acg_conv_transpose2d_fwd_stats", ctypes.byref(d), P(xin), P(pk.wb), P(pk.bias), P(y), P(part), st)
        else:
            _lib.call("acg_conv2d_fwd_stats", ctypes.byref(d), P(xin), P(pk.wf), P(pk.bias), P(y), P(part), st)
        kern = _lib.query("acg_last_kernel").decode()
        mean = torch.empty(N * Cys, device="cuda"); rstd = torch.empty(N * Cys, device="cuda")
        _lib.call("acg_norm_stats_from_partials", P(part), N, Hy * Wy, Cys, 128, 1e-5, 0, P(mean), P(rstd), st)
        torch.cuda.synchronize()
    print("KERNEL", case, kern)
    dev = _ref_device()
    X, Wt, B = (torch.tensor(a, dtype=torch.float64, device=dev) for a in (x, w, b))
    if tr:
        yr = F.conv_transpose2d(X, Wt, B, stride=2, padding=1, output_padding=1)
    elif mode == "reflect":
        yr = F.conv2d(F.pad(X, (p, p, p, p), mode="reflect"), Wt, B, stride=s)
    else:
        yr = F.conv2d(X, Wt, B, stride=s, padding=p)
    yr = yr.cpu().numpy()
    got = _nchw(n(y))[:, :Cy]
    assert rel(got, yr) < 2e-5, "y"
    mu_r = yr.mean((2, 3)); var_r = yr.var((2, 3))
    mu = n(mean).reshape(N, Cys)[:, :Cy].astype(np.float64)
    var = 1.0 / n(rstd).reshape(N, Cys)[:, :Cy].astype(np.float64) ** 2 - 1e-5
    assert np.isfinite(mu).all() and np.isfinite(var).all(), "a tile's statistics were not written"
    assert np.abs(mu - mu_r).max() < 1e-4 * np.abs(mu_r).max(), "mean"
    assert np.abs(var - var_r).max() < 1e-4 * var_r.max(), "variance"


# (kind, K, stride, Ci, Co, N, H, W): zero-padded convolutions whose data gradient emits the norm-backward sums of the norm in
# front (Ci: the channels of dx, i.e. of that norm)
SUMS_CASES = [
    ("rows", 3, 1, 64, 32, 1, 5, 128), ("rows", 3, 1, 64, 32, 3, 19, 384), ("rows", 3, 1, 64, 32, 2, 70, 640),
    ("rows", 3, 1, 64, 32, 4, 130, 256),
    ("rp", 3, 1, 32, 64, 1, 3, 128), ("rp", 3, 1, 32, 64, 2, 13, 384), ("rp", 3, 1, 32, 64, 3, 9, 640),
    ("ph4", 3, 2, 64, 128, 1, 6, 256), ("ph4", 3, 2, 64, 96, 3, 10, 512), ("ph4", 3, 2, 64, 256, 2, 4, 768),
    ("thinrow", 7, 1, 32, 3, 2, 16, 32), ("thinrow", 5, 1, 32, 3, 1, 40, 96), ("thinrow", 3, 1, 32, 1, 3, 24, 48),
]
SUMS_KERNELS = {"rows": ROWS, "rp": RP, "ph4": "igemm_conv_ph4<128,64,SUMS=1>", "thinrow": "conv_thinrow_x3<REFLECT=0,SUMS=1>"}


def _sums_check(dx_k, dx_r, psum, xn, mean, rstd, gamma, beta, act, N, Ci):
    """the test_hip_pin formulas: S1 = sum gy, S2 = sum gy * xhat, gy = dx * [norm output > 0] (ReLU) or dx"""
    from dtgan_amd import ops
    from hip_util import rel
    xh = (xn.astype(np.float32).astype(np.float64) - mean[:, :, None, None]) * rstd[:, :, None, None]
    g_b = np.broadcast_to(gamma, (N, Ci))[:, :, None, None]; b_b = np.broadcast_to(beta, (N, Ci))[:, :, None, None]
    live = (xh * g_b + b_b > 0) if act == ops.ACT_RELU else np.ones_like(xh, dtype=bool)
    edge = (np.abs(xh * g_b + b_b) < 1e-5) if act == ops.ACT_RELU else np.zeros_like(live)
    assert edge.mean() < 1e-4
    assert np.isfinite(psum).all(), "a chunk entry of the sums was not written"
    s1, s2 = psum[:, :, 0, :Ci].sum(1), psum[:, :, 1, :Ci].sum(1)
    gy_k = dx_k.astype(np.float64) * live
    assert rel(s1, gy_k.sum((2, 3))) < 1e-4 and rel(s2, (gy_k * xh).sum((2, 3))) < 1e-4, "norm backward sums (kernel dx)"
    gy = dx_r * live
    assert rel(s1, gy.sum((2, 3))) < 2e-4 and rel(s2, (gy * xh).sum((2, 3))) < 2e-4, "norm backward sums (fp64 dx)"


def _norm_inputs(rs, N, Ci, H, W, per_sample):
    xn = rs.normal(0.2, 1.1, (N, Ci, H, W))
    mean = rs.normal(0.2, 0.1, (N, Ci)); rstd = rs.uniform(0.6, 1.4, (N, Ci))
    gamma = rs.normal(1.0, 0.4, (N if per_sample else 1, Ci)); beta = rs.normal(0.0, 0.5, (N if per_sample else 1, Ci))
    return xn, mean, rstd, gamma, beta


@pytest.mark.parametrize("variant", ["relu_shared", "relu_per_sample", "none_shared"])
@pytest.mark.parametrize("case", SUMS_CASES, ids=lambda c: "%s_k%ds%d_%dto%d_%dx%dx%d" % c)
def test_data_gradient_sums_against_fp64(case, variant):
    """acg_conv2d_bwd_data_sums at drawn shapes inside acg_conv2d_bwd_data_sums_supported: every accepted descriptor launches,
    on the kernel the case is about; dx against the fp64 adjoint (2e-5), the sums against fp64 (1e-4 with the kernel's own dx,
    2e-4 with the fp64 dx), dx and `part` pre-filled with NaN"""
    from dtgan_amd import ops, _lib
    from hip_util import precision, n, rel
    kind, K, s, Ci, Co, N, H, W = case
    P = ops._ptr
    p = K // 2
    rs = np.random.RandomState(zlib.crc32(repr((case, variant)).encode()))
    w = rs.normal(0, 0.06, (Co, Ci, K, K))
    Ho, Wo = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
    dy = rs.normal(0, 1e-2, (N, Co, Ho, Wo))
    per_sample = variant == "relu_per_sample"
    act = ops.ACT_NONE if variant == "none_shared" else ops.ACT_RELU
    xn, mean, rstd, gamma, beta = _norm_inputs(rs, N, Ci, H, W, per_sample)
    with precision("bf16x3"):
        st = ops._stream()
        pk = ops.PackedConv(_dev_t(w), None, ops.cpad(Ci), ops.cpad(Co))
        d = ops.conv_desc(N, H, W, pk.Cis, pk.Cos, K, s, p, ops.PAD_ZERO, Ci, Co)
        D = ctypes.byref(d)
        assert _lib.query("acg_conv2d_bwd_data_sums_supported", D)
        Cx = pk.Cis
        nbw = _lib.query("acg_conv2d_bwd_data_workspace_bytes", D)
        ws = ops.workspace(max(nbw, 1))
        dx = torch.full((N, H, W, Cx), float("nan"), device="cuda")
        psum = torch.full((N, H * W // 128, 2, Cx), float("nan"), device="cuda")
        ns = _lib.NormSumsDesc()
        xn_t, mean_t, rstd_t = _dev_t(_nhwc(xn)), _dev_t(mean.reshape(-1)), _dev_t(rstd.reshape(-1))
        g_t, b_t = _dev_t(gamma.reshape(-1)), _dev_t(beta.reshape(-1))
        ns.x, ns.mean, ns.rstd, ns.gamma, ns.beta = P(xn_t), P(mean_t), P(rstd_t), P(g_t), P(b_t)
        ns.gstride, ns.sign_mask, ns.act, ns.part = (Cx if per_sample else 0), None, act, P(psum)
        dy_t = _dev_t(_pad_c(_nhwc(dy), pk.Cos, 3))
        _lib.call("acg_conv2d_bwd_data_sums", D, P(dy_t), P(pk.wb), P(dx), P(ws), nbw, ctypes.byref(ns), st)
        kern = _lib.query("acg_last_kernel").decode()
        torch.cuda.synchronize()
    assert SUMS_KERNELS[kind] in kern, kern
    dev = _ref_device()
    X = torch.zeros((N, Ci, H, W), dtype=torch.float64, device=dev, requires_grad=True)
    F.conv2d(X, torch.tensor(w, dtype=torch.float64, device=dev), stride=s, padding=p).backward(
        torch.tensor(dy.astype(np.float32), dtype=torch.float64, device=dev))
    dx_r = X.grad.cpu().numpy()
    dx_k = _nchw(n(dx))[:, :Ci]
    assert rel(dx_k, dx_r) < 2e-5, "data gradient"
    _sums_check(dx_k, dx_r, n(psum), xn, mean, rstd, gamma, beta, act, N, Ci)


# ---------------------------------------------------------------------------------------------------------------------
# pre-split trunk: conv_cases.S16_CASES, (N, H, W, Ci, Co) of a 3x3 reflect pad-1 layer inside acg_conv2d_s16_supported
def _unpad(N, H, W, Ci, Co):
    return W % 128 == 0 and H % 32 == 0 and H >= 64


@pytest.mark.parametrize("case", S16_CASES, ids=lambda c: "%dx%dx%d_%dto%d_%s" % (c + ("unpad" if _unpad(*c) else "frame",)))
def test_presplit_trunk_against_fp64(case):
    """acg_conv2d_fwd_s16 (+ tile statistics), acg_conv2d_bwd_data_s16 (frame or un-padded grid: igemm_conv_x3_pre, with
    dgrad_colfix_kernel on the un-padded one), acg_conv2d_bwd_weight_s16 against fp64 on the pre-split operands
    (decode(encode(v)), the values the kernels consume); on un-padded grids also acg_conv2d_bwd_data_s16_sums (the norm
    sums, NaN pre-filled) and acg_conv2d_bwd_data_s16_mask (masked by the sign bitmask of a ReLU output)"""
    from dtgan_amd import ops, _lib
    from hip_util import precision, n, rel
    N, H, W, Ci, Co = case
    P = ops._ptr
    rs = np.random.RandomState(zlib.crc32(repr(case).encode()))
    x = np.maximum(rs.normal(0, 1, (N, H, W, Ci)), 0)
    dy = rs.normal(0, 1e-2, (N, H, W, Co))
    w = rs.normal(0, 0.05, (Co, Ci, 3, 3)); b = rs.normal(0, 0.5, Co)
    unpad = _unpad(*case)

    def enc(v):
        o = torch.empty_like(v)
        _lib.call("acg_s16_encode", P(v), P(o), v.numel(), ops._stream())
        return o

    def dec(v):
        o = torch.empty_like(v)
        _lib.call("acg_s16_decode", P(v), P(o), v.numel(), ops._stream())
        return o

    with precision("bf16x3"):
        st = ops._stream()
        d = ops.conv_desc(N, H, W, Ci, Co, 3, 1, 1, ops.PAD_REFLECT, Ci, Co)
        D = ctypes.byref(d)
        assert _lib.query("acg_conv2d_s16_supported", D)
        assert bool(_lib.query("acg_conv2d_bwd_data_s16_sums_supported", D)) == unpad
        pk = ops.PackedConv(_dev_t(w), _dev_t(b), Ci, Co)
        xs, dys = enc(_dev_t(x)), enc(_dev_t(dy))
        xv, dyv = n(dec(xs)).astype(np.float64), n(dec(dys)).astype(np.float64)
        kern = {}
        y = torch.full((N, H, W, Co), float("nan"), device="cuda")
        part = torch.full((N, H * W // 128, 2, Co), float("nan"), device="cuda") if (H * W) % 128 == 0 else None
        _lib.call("acg_conv2d_fwd_s16", D, P(xs), P(pk.wf), P(pk.bias), P(y), 0, P(part), 0, st)
        kern["fwd"] = _lib.query("acg_last_kernel").decode()
        if part is not None:
            mean = torch.empty(N * Co, device="cuda"); rstd = torch.empty(N * Co, device="cuda")
            _lib.call("acg_norm_stats_from_partials", P(part), N, H * W, Co, 128, 1e-5, 0, P(mean), P(rstd), st)
        nb_d = _lib.query("acg_conv2d_bwd_data_workspace_bytes", D)
        nb_w = _lib.query("acg_conv2d_bwd_weight_workspace_bytes", D)
        ws = ops.workspace(max(nb_d, nb_w, 1))
        dx = torch.full((N, H, W, Ci), float("nan"), device="cuda")
        _lib.call("acg_conv2d_bwd_data_s16", D, P(dys), P(pk.wb), P(dx), P(ws), nb_d, None, None, None, 0, st)
        kern["dgrad"] = _lib.query("acg_last_kernel").decode()
        dx = n(dx)
        dw = torch.full((Co, Ci, 3, 3), float("nan"), device="cuda"); db = torch.full((Co,), float("nan"), device="cuda")
        _lib.call("acg_conv2d_bwd_weight_s16", D, P(xs), P(dys), P(dw), P(db), Co, Ci, P(ws), nb_w, 0, st)
        kern["wgrad"] = _lib.query("acg_last_kernel").decode()
        torch.cuda.synchronize()
    print("KERNELS", case, kern)
    assert kern["fwd"].startswith("igemm_conv_x3_pre") and kern["dgrad"].startswith("igemm_conv_x3_pre"), kern
    assert kern["wgrad"] == "wgrad_x3_krow_s16", kern
    dev = _ref_device()
    X = torch.tensor(_nchw(xv), dtype=torch.float64, device=dev, requires_grad=True)
    Wt = torch.tensor(w, dtype=torch.float64, device=dev, requires_grad=True)
    B = torch.tensor(b, dtype=torch.float64, device=dev, requires_grad=True)
    yr = F.conv2d(F.pad(X, (1, 1, 1, 1), mode="reflect"), Wt, B)
    yr.backward(torch.tensor(_nchw(dyv), dtype=torch.float64, device=dev))
    yr = yr.detach().cpu().numpy()
    assert rel(_nchw(n(y)), yr) < 2e-5, "y"
    assert rel(_nchw(dx), X.grad.cpu().numpy()) < 2e-5, "dx"
    assert rel(n(dw), Wt.grad.cpu().numpy()) < 1e-4, "dw"
    assert rel(n(db), B.grad.cpu().numpy()) < 1e-4, "db"
    if part is not None:
        mu = n(mean).reshape(N, Co).astype(np.float64); var = 1.0 / n(rstd).reshape(N, Co).astype(np.float64) ** 2 - 1e-5
        mu_r, var_r = yr.mean((2, 3)), yr.var((2, 3))
        assert np.abs(mu - mu_r).max() < 1e-4 * np.abs(mu_r).max() and np.abs(var - var_r).max() < 1e-4 * var_r.max(), "statistics"
    if not unpad:
        return
    dx_r = X.grad.cpu().numpy()
    # the norm sums of the norm in front, ReLU and NONE, shared and per-sample affine parameters
    for variant in ("relu_shared", "relu_per_sample", "none_shared"):
        per_sample = variant == "relu_per_sample"
        act = ops.ACT_NONE if variant == "none_shared" else ops.ACT_RELU
        xn, mean_, rstd_, gamma, beta = _norm_inputs(rs, N, Ci, H, W, per_sample)
        with precision("bf16x3"):
            st = ops._stream()
            dxs = torch.full((N, H, W, Ci), float("nan"), device="cuda")
            psum = torch.full((N, H * W // 128, 2, Ci), float("nan"), device="cuda")
            ns = _lib.NormSumsDesc()
            xn_t, m_t, r_t = _dev_t(_nhwc(xn)), _dev_t(mean_.reshape(-1)), _dev_t(rstd_.reshape(-1))
            g_t, b_t = _dev_t(gamma.reshape(-1)), _dev_t(beta.reshape(-1))
            ns.x, ns.mean, ns.rstd, ns.gamma, ns.beta = P(xn_t), P(m_t), P(r_t), P(g_t), P(b_t)
            ns.gstride, ns.sign_mask, ns.act, ns.part = (Ci if per_sample else 0), None, act, P(psum)
            _lib.call("acg_conv2d_bwd_data_s16_sums", D, P(dys), P(pk.wb), P(dxs), P(ws), nb_d, None, None, ctypes.byref(ns), st)
            k = _lib.query("acg_last_kernel").decode()
            torch.cuda.synchronize()
        assert "SUMS=1" in k and k.startswith("igemm_conv_x3_pre"), k
        dx_k = _nchw(n(dxs))
        assert rel(dx_k, dx_r) < 2e-5, (variant, "dx")
        _sums_check(dx_k, dx_r, n(psum), xn, mean_, rstd_, gamma, beta, act, N, Ci)
    # the data gradient masked by the sign bitmask of a ReLU output (pre-split output)
    sign = rs.normal(0, 1, (N, H, W, Ci)) > 0
    bits = (torch.from_numpy(sign.reshape(-1, 32).astype(np.int64)) << torch.arange(32)).sum(1)
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32).cuda()
    with precision("bf16x3"):
        st = ops._stream()
        dxm = torch.full((N, H, W, Ci), float("nan"), device="cuda")
        _lib.call("acg_conv2d_bwd_data_s16_mask", D, P(dys), P(pk.wb), P(dxm), P(ws), nb_d, P(bits), st)
        k = _lib.query("acg_last_kernel").decode()
        got = n(dec(dxm))
    assert k.startswith("igemm_conv_x3_pre"), k
    assert rel(got, _nhwc(dx_r) * sign) < 3e-5, "masked dx (pre-split output: + 2^-17 storage rounding)"
