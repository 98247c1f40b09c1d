"""GPU tests of the connected components of excursion sets: acg_components, through ops.components and through the C ABI,
against tests/components_ref.py for equality, on the statistics and on the canonical labels (everything is an integer: no
tolerance anywhere), in every layout, at the sizes where tiles and seams appear, in passes, and its refusals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import components_ref as R
import minkowski_ref as K
from guard_util import GUARD, Buf
from field_cases import OFFSET_LAYOUTS as LAYOUTS, offset_operand as _device

pytestmark = pytest.mark.gpu

TH, TW = 32, 64            # the tile of a workgroup (csrc/components.hip CC_TH, CC_TW)
# 1 x 1 and single rows / columns; one cell short of a tile, a tile, one cell past it (a seam each way and a corner); three
# by three tiles with a ragged edge; off the tile grid both ways; the native grid of many tiles
SIZES = ((1, 1), (1, 64), (64, 1), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 1, 3 * TW - 1), (63, 65), (65, 63), (321, 321))
TC = ((1, 1), (2, 3), (31, 4))


@functools.lru_cache(maxsize=None)
def _case(kind, H, W, T, C, rows=2):
    """rows of C fields, their thresholds and, per connectivity, the reference statistics and labels; left unchanged"""
    thr = R.make_thresholds(kind, C, T, seed=T + C)
    x = R.make_fields(kind, rows, C, H, W, thr, seed=T)
    ref = {conn: R.stats(x, thr, conn, labels=True) for conn in (4, 8)}
    for a in (thr, x) + ref[4] + ref[8]:
        a.setflags(write=False)
    return x, thr, ref


def _comp(xd, C, layout, thr, conn, H, W):
    """ops.components into poisoned outputs -> host (rows, C, T, 25) int64 and (rows, C, T, H, W) int32"""
    from dtgan_amd import ops
    T = thr.shape[1]
    out = torch.full((xd.shape[0], C, T, R.COMP_STATS), -7, dtype=torch.int64, device="cuda")
    lab = torch.full((xd.shape[0], C, T, H, W), -7, dtype=torch.int32, device="cuda")
    got = ops.components(xd, C, layout, thr, conn=conn, out=out, labels=lab)
    assert got[0] is out and got[1] is lab
    return out.cpu().numpy(), lab.cpu().numpy()


def _path(layout, Cp, off, H, W):
    load = "c4" if (layout, Cp, off) == ("nhwc", 4, 0) else "strided"
    one_tile = H <= TH and W <= TW
    return ("comp_label<%s> + comp_stats" if one_tile else "comp_label<%s> + comp_merge + comp_root + comp_stats") % load


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("H,W", SIZES)
def test_kernel_equals_the_reference_in_every_layout(H, W, kind):
    from dtgan_amd import _lib
    big = H * W >= 100000
    for T, C in (TC[2:] if big else TC):
        x, thr, ref = _case(kind, H, W, T, C, 1 if big else 2)
        for conn in (4, 8):
            for layout, Cp, off in LAYOUTS:
                got, lab = _comp(_device(x, layout, Cp, off, seed=T), C, layout, thr, conn, H, W)
                assert _lib.query("acg_last_kernel").decode() == _path(layout, Cp, off, H, W)
                assert got.dtype == np.int64 and lab.dtype == np.int32
                assert np.array_equal(got, ref[conn][0]), (kind, H, W, T, C, conn, layout, Cp, off, np.argwhere(got != ref[conn][0])[:5])
                assert np.array_equal(lab, ref[conn][1]), (kind, H, W, T, C, conn, layout, Cp, off, np.argwhere(lab != ref[conn][1])[:5])


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("kind", ("spiral", "comb", "checker", "perc41", "perc59"))
def test_one_large_plane(kind, conn):
    """1024 x 1024, C = T = 1: 512 tiles; the spiral and the comb are one component through all of them"""
    from dtgan_amd import _lib
    H = W = 1024
    thr = np.zeros((1, 1), np.float32)
    x = R.make_fields(kind, 1, 1, H, W, thr)
    ref, rl = R.stats(x, thr, conn, labels=True)
    if kind in ("spiral", "comb") or (kind, conn) == ("checker", 8):
        assert ref[0, 0, 0, 0] == 1 and ref[0, 0, 0, 2] == ref[0, 0, 0, 1] ** 2 > 1 << 36
    for layout, Cp in (("nchw", 0), ("nhwc", 4)):
        got, lab = _comp(_device(x, layout, Cp), 1, layout, thr, conn, H, W)
        assert _lib.query("acg_last_kernel").decode() == _path(layout, Cp, 0, H, W)
        assert np.array_equal(got, ref), (layout, got[0, 0, 0], ref[0, 0, 0])
        assert np.array_equal(lab, rl), (layout, np.argwhere(lab != rl)[:5])


def _abi_call(lib, xd, rows, C, H, W, sx, thr_d, T, conn, out, labels, ws, nbytes):
    from dtgan_amd import ops
    return lib.acg_components(ops._ptr(xd), rows, C, H, W, sx[0], sx[1], sx[2], ops._ptr(thr_d), T, conn, out, labels, ws, nbytes,
                              ops._stream())


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("kind,H,W", (("special", 65, 63), ("perc41", 70, 130), ("perc59", 33, 65)))
def test_passes_guard_words_poison_and_repeatability(kind, H, W, conn):
    """through the C ABI, 7 planes (one field, 7 thresholds: the passes cut through a workgroup's walk over its planes): with a
    workspace of exactly one plane, of three planes and of the query's size the same bits, also from a 0xFF-filled workspace
    and on a second call; out and labels start poisoned and lie, like the workspace, between guard words"""
    from dtgan_amd import _lib
    lib = _lib.load()
    rows, C, T = 1, 1, 7
    x, thr, ref = _case(kind, H, W, T, C, 1)
    thr_d = torch.from_numpy(thr.copy()).cuda()
    plane = (H * W * 8 + 15) // 16 * 16
    need = lib.acg_components_workspace_bytes(rows, C, H, W, T)
    assert need == 7 * plane
    n_out, n_lab = rows * C * T * R.COMP_STATS, rows * C * T * H * W
    seen = []
    for layout, Cp, sx in (("nhwc", 4, (H * W * 4, 4, 1)), ("nhwc", 16, (H * W * 16, 16, 1)), ("nchw", 0, (C * H * W, 1, H * W))):
        xd = _device(x, layout, Cp, seed=3)
        for nbytes in (plane, 3 * plane, need):
            out = Buf.out(GUARD + 2 * n_out, np.uint32)
            lab = Buf.out(GUARD + n_lab, np.uint32)
            ws = Buf(GUARD + nbytes // 4, dtype=np.uint32)         # 0xFFFFFFFF everywhere
            for call in range(2):
                rc = _abi_call(lib, xd, rows, C, H, W, sx, thr_d, T, conn, out.at(GUARD), lab.at(GUARD), ws.at(GUARD), nbytes)
                assert rc == 0, lib.acg_last_error().decode()
                o, l = out.host(), lab.host()                      # checks the words behind the buffers
                assert np.all(o[:GUARD] == 0xFFFFFFFF) and np.all(l[:GUARD] == 0xFFFFFFFF) and np.all(ws.host()[:GUARD] == 0xFFFFFFFF)
                seen.append((o[GUARD:].copy(), l[GUARD:].copy()))
                assert np.array_equal(o[GUARD:].view(np.int64).reshape(ref[conn][0].shape), ref[conn][0]), (layout, Cp, nbytes, call)
                assert np.array_equal(l[GUARD:].view(np.int32).reshape(ref[conn][1].shape), ref[conn][1]), (layout, Cp, nbytes, call)
        # without labels: the same statistics
        out = Buf.out(GUARD + 2 * n_out, np.uint32)
        ws = Buf(GUARD + need // 4, dtype=np.uint32)
        assert _abi_call(lib, xd, rows, C, H, W, sx, thr_d, T, conn, out.at(GUARD), None, ws.at(GUARD), need) == 0
        assert np.array_equal(out.host()[GUARD:], seen[0][0])
    assert all(np.array_equal(s[0], seen[0][0]) and np.array_equal(s[1], seen[0][1]) for s in seen)
    Buf.check_all()


@pytest.mark.parametrize("H,W", ((33, 65), (64, 128)))
def test_the_two_kernels_agree_and_the_holes_are_the_brute_forces(H, W):
    """smooth fields: area == nF of acg_minkowski, and n - euler{conn} of its counts is the number of labelled holes, >= 0"""
    from dtgan_amd import ops
    C, T = 2, 6
    thr = K.make_thresholds(C, T, seed=4)
    x = K.make_fields("smooth", 2, C, H, W, thr, seed=6)
    xd = _device(x, "nchw")
    counts = ops.minkowski(xd, C, "nchw", thr).cpu().numpy()
    euler = K.functionals(counts)
    four, eight = R._STRUCTURE[4], R._STRUCTURE[8]
    from scipy import ndimage
    for conn, bg in ((4, eight), (8, four)):
        got = ops.components(xd, C, "nchw", thr, conn=conn).cpu().numpy()
        assert np.array_equal(got[..., 1], counts[..., 0])
        holes = got[..., 0] - euler["euler%d" % conn]
        assert np.all(holes >= 0) and holes.max() > 0
        for r in range(2):
            for c in range(C):
                for t in range(T):
                    with np.errstate(invalid="ignore"):
                        mask = x[r, c] >= thr[c, t]
                    assert holes[r, c, t] == ndimage.label(~np.pad(mask, 2), structure=bg)[1] - 1, (conn, r, c, t)
        brute = np.stack([[K.functionals_brute(x[r, c], thr[c])["euler%d" % conn] for c in range(C)] for r in range(2)])
        assert np.array_equal(euler["euler%d" % conn], brute)


def test_device_thresholds_and_a_fresh_output():
    """thresholds already on the device are taken as they are; without `out` a new int64 tensor comes back, with labels=True a
    new int32 one too; nothing requires grad"""
    from dtgan_amd import ops
    x, thr, ref = _case("special", 65, 63, 31, 4)
    xd = _device(x, "nhwc", 4).requires_grad_(True)
    got = ops.components(xd, 4, "nhwc", torch.from_numpy(thr.copy()).cuda())
    assert got.dtype == torch.int64 and got.is_cuda and not got.requires_grad and np.array_equal(got.cpu().numpy(), ref[8][0])
    out, lab = ops.components(xd, 2, "nhwc", thr[:2], conn=4, labels=True)      # the first two of four stored channels
    assert lab.dtype == torch.int32 and lab.is_cuda and not lab.requires_grad and not out.requires_grad
    assert np.array_equal(out.cpu().numpy(), ref[4][0][:, :2]) and np.array_equal(lab.cpu().numpy(), ref[4][1][:, :2])
    assert ops.COMP_STATS == R.COMP_STATS and ops.COMP_BINS == R.COMP_BINS


def test_the_call_is_capturable_in_a_graph():
    """launches only: captured once, replayed on new fields, the same bits as the plain call"""
    from dtgan_amd import ops
    x, thr, ref = _case("perc41", 65, 63, 2, 3)
    xd = _device(x, "nhwc", 4)
    thr_d = torch.from_numpy(thr.copy()).cuda()
    out = torch.full((2, 3, 2, R.COMP_STATS), -7, dtype=torch.int64, device="cuda")
    ops.components(xd, 3, "nhwc", thr_d, out=out)                  # the workspace exists before the capture
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        out.fill_(-7)
        with torch.cuda.graph(graph, stream=s):
            ops.components(xd, 3, "nhwc", thr_d, out=out)
    torch.cuda.current_stream().wait_stream(s)
    out.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref[8][0])


def test_kernel_refuses_bad_arguments_before_launching():
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    x = torch.zeros(1 << 16, device="cuda")
    thr_d = torch.zeros(256, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    lab = torch.full((1 << 16,), -7, dtype=torch.int32, device="cuda")
    big = ws.numel()
    plane = 64 * 64 * 8
    assert lib.acg_components_workspace_bytes(2, 1, 64, 64, 3) == 6 * plane
    assert lib.acg_components_workspace_bytes(1, 1, 1, 1, 1) == 16 and lib.acg_components_workspace_bytes(1, 1, 3, 5, 2) == 2 * 128
    # capped at the whole planes inside 256 MiB: the evaluator's group, and one plane of the largest field
    assert lib.acg_components_workspace_bytes(255, 3, 256, 256, 31) == 256 << 20
    assert lib.acg_components_workspace_bytes(64, 1, 1000, 1000, 1) == ((256 << 20) // 8000000) * 8000000
    assert lib.acg_components_workspace_bytes(1, 1, 1024, 1024, 1) == 8 << 20
    for bad in ((0, 1, 8, 8, 1), (1, 0, 8, 8, 1), (1, 1, 0, 8, 1), (1, 1, 8, 1025, 1), (1, 1, 8, 8, 0), (1, 1, 8, 8, 256), (1 << 30, 4, 8, 8, 1)):
        assert lib.acg_components_workspace_bytes(*bad) == 0, bad
    P = (4096, 1, 4096)
    # rows, C, H, W, strides, T, conn, x?, thr?, out?, labels?, workspace offset, bytes, status, a word of the message
    bad = [(2, 1, 64, 64, P, 3, 8, 0, 1, 1, 0, 0, big, -1, "null"), (2, 1, 64, 64, P, 3, 8, 1, 0, 1, 0, 0, big, -1, "null"),
           (2, 1, 64, 64, P, 3, 8, 1, 1, 0, 0, 0, big, -1, "null"), (2, 1, 0, 64, P, 3, 8, 1, 1, 1, 0, 0, big, -1, "H x W"),
           (2, 1, 64, 1025, P, 3, 8, 1, 1, 1, 0, 0, big, -1, "H x W"), (2, 1, 1025, 4, P, 3, 8, 1, 1, 1, 0, 0, big, -1, "H x W"),
           (0, 1, 64, 64, P, 3, 8, 1, 1, 1, 0, 0, big, -1, "rows >= 1"), (2, 0, 64, 64, P, 3, 8, 1, 1, 1, 0, 0, big, -1, "C >= 1"),
           (2, 1, 64, 64, P, 0, 8, 1, 1, 1, 0, 0, big, -1, "thresholds"), (2, 1, 64, 64, P, 256, 8, 1, 1, 1, 0, 0, big, -1, "thresholds"),
           (2, 1, 64, 64, P, 3, 6, 1, 1, 1, 0, 0, big, -1, "connectivity"), (2, 1, 64, 64, P, 3, 0, 1, 1, 1, 0, 0, big, -1, "connectivity"),
           (1 << 30, 4, 8, 8, P, 1, 8, 1, 1, 1, 0, 0, big, -1, "too many planes"),
           (1 << 20, 1, 64, 64, P, 1, 8, 1, 1, 1, 1, 0, big, -1, "labels"),
           (2, 1, 64, 64, (0, 1, 4096), 3, 8, 1, 1, 1, 0, 0, big, -1, "strides"), (2, 1, 64, 64, (4096, 0, 4096), 3, 8, 1, 1, 1, 0, 0, big, -1, "strides"),
           (2, 1, 64, 64, (4096, 1, -1), 3, 8, 1, 1, 1, 0, 0, big, -1, "strides"),
           (2, 1, 64, 64, P, 3, 8, 1, 1, 1, 0, 0, plane - 1, -2, "workspace too small"), (2, 1, 64, 64, P, 3, 8, 1, 1, 1, 0, 8, big - 8, -1, "aligned")]
    for rows, C, H, W, sx, T, conn, has_x, has_thr, has_out, has_lab, off, nbytes, rc_want, word in bad:
        out = torch.full((4096,), -7, dtype=torch.int64, device="cuda")
        rc = _abi_call(lib, x if has_x else None, rows, C, H, W, sx, thr_d if has_thr else None, T, conn, ops._ptr(out) if has_out else None,
                       ops._ptr(lab) if has_lab else None, ctypes.c_void_p(ws.data_ptr() + off), nbytes)
        msg = lib.acg_last_error().decode()
        assert rc == rc_want and msg.startswith("acg_components") and word in msg, (rows, C, H, W, sx, T, conn, rc, msg)
        torch.cuda.synchronize()
        assert torch.all(out == -7) and torch.all(lab == -7)       # nothing was written
    rc = _abi_call(lib, x, 2, 1, 64, 64, P, thr_d, 3, 8, ops._ptr(out), None, None, 0)
    assert rc == -2 and torch.all(out == -7)                       # a missing workspace
    rc = _abi_call(lib, x, 2, 1, 64, 64, P, thr_d, 3, 8, ops._ptr(out), None, ctypes.c_void_p(ws.data_ptr()), plane)
    assert rc == 0, lib.acg_last_error().decode()                  # and the same call with one plane: six passes
    torch.cuda.synchronize()
    got = out[:6 * 25].view(2, 3, 25)                              # zeros >= 0: one component of 4096 cells on the border
    want = torch.zeros(25, dtype=torch.int64)
    want[0], want[1], want[2], want[3], want[4 + 12] = 1, 4096, 4096 * 4096, 1, 1
    assert torch.equal(got.cpu(), want.expand(2, 3, 25)) and torch.all(out[6 * 25:] == -7)
