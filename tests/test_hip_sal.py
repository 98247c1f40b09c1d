"""GPU tests of the SAL moments: acg_sal, through ops.sal and through the C ABI, against tests/sal_ref.py: the integers
(field, obj) for equality, the two double sums within the order of their additions, in every layout, at the sizes where tiles
and seams appear, in passes, from a captured graph, and its refusals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sal_ref as S
from guard_util import GUARD, Buf
from field_cases import offset_operand as _device
from sal_ref import check as _check

pytestmark = pytest.mark.gpu

TH, TW = 32, 64            # the tile of a workgroup (csrc/components.hip CC_TH, CC_TW)
# 1 x 1, a single row and column; one cell short of a tile, a tile, one cell past it; two by two tiles; off the tile grid
# both ways; the native grid of many tiles
SIZES = ((1, 1), (1, 7), (5, 1), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (64, 128), (97, 130), (321, 321))
TC = ((1, 1), (3, 3), (31, 4))
LAYOUTS = (("nchw", 0), ("nhwc", 4), ("nhwc", 16))
KINDS = ("special", "smooth", "constant", "perc59", "corners")


@functools.lru_cache(maxsize=None)
def _case(kind, H, W, T, C, rows=2):
    """rows of C fields, their thresholds and, per connectivity, the reference triple; left unchanged"""
    thr = S.make_thresholds(kind, C, T, seed=T + C)
    x = S.make_fields(kind, rows, C, H, W, thr, seed=T)
    ref = {conn: S.sal(x, thr, conn) for conn in (4, 8)}
    for a in (thr, x) + ref[4] + ref[8]:
        a.setflags(write=False)
    return x, thr, ref


def _sal(xd, C, layout, thr, conn, floor=-1.0):
    """ops.sal into poisoned outputs -> host field, obj, shape"""
    from dtgan_amd import ops
    rows, T = xd.shape[0], thr.shape[1]
    out = (torch.full((rows, C, 3), -7, dtype=torch.int64, device="cuda"), torch.full((rows, C, T, 4), -7, dtype=torch.int64, device="cuda"),
           torch.full((rows, C, T, 2), float("nan"), dtype=torch.float64, device="cuda"))
    got = ops.sal(xd, C, layout, thr, floor=floor, conn=conn, out=out)
    assert all(g is o for g, o in zip(got, out))
    return tuple(o.cpu().numpy() for o in out)


def _path(layout, Cp, H, W):
    load = "c4" if (layout, Cp) == ("nhwc", 4) else "strided"
    one_tile = H <= TH and W <= TW
    return ("sal_field<%s> + sal_label<%s> + sal_finish" if one_tile else "sal_field<%s> + sal_label<%s> + comp_merge + sal_root + sal_finish") % (load, load)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", SIZES)
def test_kernel_equals_the_reference_in_every_layout(H, W, kind):
    from dtgan_amd import _lib, ops
    big = H * W >= 100000
    for T, C in (TC[1:2] if big else TC):
        x, thr, ref = _case(kind, H, W, T, C, 1 if big else 2)
        for conn in (4, 8):
            seen = []
            for layout, Cp in LAYOUTS:
                xd = _device(x, layout, Cp, seed=T)
                got = _sal(xd, C, layout, thr, conn)
                assert _lib.query("acg_last_kernel").decode() == _path(layout, Cp, H, W)
                _check(got, ref[conn], (kind, H, W, T, C, conn, layout, Cp))
                seen.append(got)
            assert all(np.array_equal(a, b) for s in seen[1:] for a, b in zip(s, seen[0]))     # the same bits in every layout
            comp = ops.components(xd, C, layout, thr, conn=conn).cpu().numpy()
            assert np.array_equal(seen[0][1][..., :2], comp[..., :2])


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("kind", ("spiral", "checker"))
def test_one_large_plane(kind, conn):
    """1024 x 1024, C = T = 1: 512 tiles; the spiral is one object through all of them, the checkerboard has the most"""
    from dtgan_amd import _lib
    H = W = 1024
    thr = np.zeros((1, 1), np.float32)
    x = S.make_fields(kind, 1, 1, H, W, thr)
    ref = S.sal(x, thr, conn)
    n = ref[1][0, 0, 0, 0]
    assert n == (1 if kind == "spiral" or conn == 8 else H * W // 2)
    seen = []
    for layout, Cp in (("nchw", 0), ("nhwc", 4)):
        got = _sal(_device(x, layout, Cp), 1, layout, thr, conn)
        assert _lib.query("acg_last_kernel").decode() == _path(layout, Cp, H, W)
        _check(got, ref, (kind, conn, layout))
        seen.append(got)
    assert all(np.array_equal(a, b) for a, b in zip(seen[0], seen[1]))


def test_the_saturated_largest_field():
    """1024 x 1024 with every cell at floor + 16: q = 2^24 everywhere, one object, the largest sums there are (QY < 2^54)"""
    H = W = 1024
    x = np.full((1, 1, H, W), 15.0, np.float32)
    thr = np.zeros((1, 1), np.float32)
    field, obj, shape = _sal(_device(x, "nchw"), 1, "nchw", thr, 4)
    Q, M1 = 1 << 44, (1 << 24) * 1024 * (1023 * 1024 // 2)
    assert field[0, 0].tolist() == [Q, M1, M1] and M1 < 1 << 54
    assert obj[0, 0, 0].tolist() == [1, H * W, Q, Q]
    assert shape[0, 0, 0].tolist() == [float(Q) * (float(Q) / float(1 << 24)), 0.0]
    x[0, 0, 0, 0] = np.inf                                           # +inf saturates too, -inf and NaN weigh nothing and lie outside
    x[0, 0, 5, 5], x[0, 0, 9, 9] = -np.inf, np.nan
    got = _sal(_device(x, "nhwc", 4), 1, "nhwc", thr, 8)
    _check(got, S.sal(x, thr, 8), "specials")
    assert got[1][0, 0, 0].tolist() == [1, H * W - 2, Q - (2 << 24), Q - (2 << 24)]


def test_other_floors_and_edge_thresholds():
    """floor 0, a floor off the binary grid and one above most values; a threshold only +inf reaches, one that every cell but
    NaN and -inf reaches, repeats; a field with no cell above its threshold"""
    H, W = 70, 131
    thr = np.array([[-9.0, -0.25, -0.25, 0.25, 9.0]] * 2, np.float32)
    x = S.make_fields("special", 2, 2, H, W, thr[:, 1:4], seed=4)
    for floor in (0.0, -1.3, 0.4):
        for conn in (4, 8):
            ref = S.sal(x, thr, conn, floor)
            assert np.array_equal(ref[1][:, :, 4, 1], np.isposinf(x).sum((2, 3))) and np.array_equal(ref[1][:, :, 1], ref[1][:, :, 2])
            for layout, Cp in LAYOUTS:
                _check(_sal(_device(x, layout, Cp), 2, layout, thr, conn, floor), ref, (floor, conn, layout, Cp))
    low = np.full((1, 1, H, W), -0.5, np.float32)                    # nothing exceeds: no object, mass in the field all the same
    field, obj, shape = _sal(_device(low, "nchw"), 1, "nchw", thr[:1, 3:4], 8)
    assert field[0, 0, 0] == H * W << 19 and not obj.any() and not shape.any()


def _abi_call(lib, xd, rows, C, H, W, sx, thr_d, T, conn, floor, field, obj, shape, ws, nbytes):
    from dtgan_amd import ops
    return lib.acg_sal(ops._ptr(xd), rows, C, H, W, sx[0], sx[1], sx[2], ops._ptr(thr_d), T, conn, floor, field, obj, shape, ws, nbytes,
                       ops._stream())


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("kind,H,W", (("special", 65, 63), ("perc59", 70, 130), ("smooth", 33, 65)))
def test_passes_guard_words_poison_and_repeatability(kind, H, W, conn):
    """through the C ABI, 7 planes (one field, 7 thresholds: the passes cut through a workgroup's walk over its planes): with a
    workspace of exactly one plane, of three planes and of the query's size the same bits, also from a 0xFF-filled workspace,
    on a second call and in every layout; the outputs start poisoned and lie, like the workspace, between guard words"""
    from dtgan_amd import _lib
    lib = _lib.load()
    rows, C, T = 1, 1, 7
    x, thr, ref = _case(kind, H, W, T, C, 1)
    thr_d = torch.from_numpy(thr.copy()).cuda()
    plane = H * W * 32
    need = lib.acg_sal_workspace_bytes(rows, C, H, W, T)
    assert need == 7 * plane
    seen = []
    for layout, Cp, sx in (("nhwc", 4, (H * W * 4, 4, 1)), ("nhwc", 16, (H * W * 16, 16, 1)), ("nchw", 0, (C * H * W, 1, H * W))):
        xd = _device(x, layout, Cp, seed=3)
        for nbytes in (plane, 3 * plane, need):
            outs = [Buf.out(GUARD + 2 * n, np.uint32) for n in (rows * C * 3, rows * C * T * 4, rows * C * T * 2)]
            ws = Buf(GUARD + nbytes // 4, dtype=np.uint32)         # 0xFFFFFFFF everywhere
            for call in range(2):
                rc = _abi_call(lib, xd, rows, C, H, W, sx, thr_d, T, conn, -1.0, *[o.at(GUARD) for o in outs], ws.at(GUARD), nbytes)
                assert rc == 0, lib.acg_last_error().decode()
                host = [o.host() for o in outs]                    # checks the words behind the buffers
                assert all(np.all(h[:GUARD] == 0xFFFFFFFF) for h in host) and np.all(ws.host()[:GUARD] == 0xFFFFFFFF)
                raw = [h[GUARD:].copy() for h in host]
                seen.append(raw)
                got = tuple(r.view(dt).reshape(a.shape) for r, dt, a in zip(raw, (np.int64, np.int64, np.float64), ref[conn]))
                _check(got, ref[conn], (layout, Cp, nbytes, call))
    assert all(np.array_equal(a, b) for s in seen[1:] for a, b in zip(s, seen[0]))
    Buf.check_all()


def test_device_thresholds_and_fresh_outputs():
    """thresholds already on the device are taken as they are; without `out` new tensors come back; nothing requires grad"""
    from dtgan_amd import ops
    x, thr, ref = _case("special", 97, 130, 31, 4)
    xd = _device(x, "nhwc", 4).requires_grad_(True)
    got = ops.sal(xd, 4, "nhwc", torch.from_numpy(thr.copy()).cuda())
    assert [g.dtype for g in got] == [torch.int64, torch.int64, torch.float64]
    assert all(g.is_cuda and not g.requires_grad for g in got)
    _check(tuple(g.cpu().numpy() for g in got), ref[8], "device thresholds")
    got = ops.sal(xd, 2, "nhwc", thr[:2], conn=4)                   # the first two of four stored channels
    _check(tuple(g.cpu().numpy() for g in got), tuple(a[:, :2] for a in ref[4]), "two of four channels")


def test_the_call_is_capturable_in_a_graph():
    """launches only: captured once, replayed, the same bits as the plain call"""
    from dtgan_amd import ops
    x, thr, ref = _case("perc59", 65, 63, 2, 3)
    xd = _device(x, "nhwc", 4)
    thr_d = torch.from_numpy(thr.copy()).cuda()
    eager = [g.clone() for g in ops.sal(xd, 3, "nhwc", thr_d)]      # the workspace exists before the capture
    out = (torch.empty((2, 3, 3), dtype=torch.int64, device="cuda"), torch.empty((2, 3, 2, 4), dtype=torch.int64, device="cuda"),
           torch.empty((2, 3, 2, 2), dtype=torch.float64, device="cuda"))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            ops.sal(xd, 3, "nhwc", thr_d, out=out)
    torch.cuda.current_stream().wait_stream(s)
    for o in out:
        o.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(o, e) for o, e in zip(out, eager))
    _check(tuple(o.cpu().numpy() for o in out), ref[8], "replay")


def test_kernel_refuses_bad_arguments_before_launching():
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    x = torch.zeros(1 << 16, device="cuda")
    thr_d = torch.zeros(256, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    big = ws.numel()
    plane = 64 * 64 * 32
    assert lib.acg_sal_workspace_bytes(2, 1, 64, 64, 3) == 6 * plane
    P = (4096, 1, 4096)
    inf, nan = float("inf"), float("nan")
    # rows, C, H, W, strides, T, conn, floor, x?, thr?, field?, obj?, shape?, workspace offset, bytes, status, a word of the message
    bad = [(2, 1, 64, 64, P, 3, 8, -1.0, 0, 1, 1, 1, 1, 0, big, -1, "null"), (2, 1, 64, 64, P, 3, 8, -1.0, 1, 0, 1, 1, 1, 0, big, -1, "null"),
           (2, 1, 64, 64, P, 3, 8, -1.0, 1, 1, 0, 1, 1, 0, big, -1, "null"), (2, 1, 64, 64, P, 3, 8, -1.0, 1, 1, 1, 0, 1, 0, big, -1, "null"),
           (2, 1, 64, 64, P, 3, 8, -1.0, 1, 1, 1, 1, 0, 0, big, -1, "null"),
           (2, 1, 0, 64, P, 3, 8, -1.0, 1, 1, 1, 1, 1, 0, big, -1, "H x W"), (2, 1, 64, 1025, P, 3, 8, -1.0, 1, 1, 1, 1, 1, 0, big, -1, "H x W"),
           (2, 1, 1025, 4, P, 3, 8, -1.0, 1, 1, 1, 1, 1, 0, big, -1, "H x W"),
           (0, 1, 64, 64, P, 3, 8, -1.0, 1, 1, 1, 1, 1, 0, big, -1, "rows >= 1"), (2, 0, 64, 64, P, 3, 8, -1.0, 1, 1, 1, 1, 1, 0, big, -1, "C >= 1"),
           (2, 1, 64, 64, P, 0, 8, -1.0, 1, 1, 1, 1, 1, 0, big, -1, "thresholds"), (2, 1, 64, 64, P, 256, 8, -1.0, 1, 1, 1, 1, 1, 0, big, -1, "thresholds"),
           (2, 1, 64, 64, P, 3, 6, -1.0, 1, 1, 1, 1, 1, 0, big, -1, "connectivity"), (2, 1, 64, 64, P, 3, 0, -1.0, 1, 1, 1, 1, 1, 0, big, -1, "connectivity"),
           (2, 1, 64, 64, P, 3, 8, nan, 1, 1, 1, 1, 1, 0, big, -1, "floor"), (2, 1, 64, 64, P, 3, 8, inf, 1, 1, 1, 1, 1, 0, big, -1, "floor"),
           (2, 1, 64, 64, P, 3, 8, -inf, 1, 1, 1, 1, 1, 0, big, -1, "floor"),
           (1 << 30, 4, 8, 8, P, 1, 8, -1.0, 1, 1, 1, 1, 1, 0, big, -1, "too many planes"),
           (2, 1, 64, 64, (0, 1, 4096), 3, 8, -1.0, 1, 1, 1, 1, 1, 0, big, -1, "strides"),
           (2, 1, 64, 64, (4096, 0, 4096), 3, 8, -1.0, 1, 1, 1, 1, 1, 0, big, -1, "strides"),
           (2, 1, 64, 64, (4096, 1, -1), 3, 8, -1.0, 1, 1, 1, 1, 1, 0, big, -1, "strides"),
           (2, 1, 64, 64, P, 3, 8, -1.0, 1, 1, 1, 1, 1, 0, plane - 1, -2, "workspace too small"),
           (2, 1, 64, 64, P, 3, 8, -1.0, 1, 1, 1, 1, 1, 8, big - 8, -1, "aligned")]
    outs = [torch.full((4096,), -7, dtype=torch.int64, device="cuda") for _ in range(2)] + [torch.full((4096,), -7.0, dtype=torch.float64, device="cuda")]
    for rows, C, H, W, sx, T, conn, floor, has_x, has_thr, has_f, has_o, has_s, off, nbytes, rc_want, word in bad:
        ptrs = [ops._ptr(o) if has else None for o, has in zip(outs, (has_f, has_o, has_s))]
        rc = _abi_call(lib, x if has_x else None, rows, C, H, W, sx, thr_d if has_thr else None, T, conn, floor, *ptrs,
                       ctypes.c_void_p(ws.data_ptr() + off), nbytes)
        msg = lib.acg_last_error().decode()
        assert rc == rc_want and msg.startswith("acg_sal") and word in msg, (rows, C, H, W, sx, T, conn, floor, rc, msg)
        torch.cuda.synchronize()
        assert all(torch.all(o == -7) for o in outs)               # nothing was written
    ptrs = [ops._ptr(o) for o in outs]
    rc = _abi_call(lib, x, 2, 1, 64, 64, P, thr_d, 3, 8, -1.0, *ptrs, None, 0)
    assert rc == -2 and all(torch.all(o == -7) for o in outs)      # a missing workspace
    rc = _abi_call(lib, x, 2, 1, 64, 64, P, thr_d, 3, 8, -1.0, *ptrs, ctypes.c_void_p(ws.data_ptr()), plane)
    assert rc == 0, lib.acg_last_error().decode()                  # and the same call with one plane: six passes
    torch.cuda.synchronize()
    q = 1 << 20                                                    # zeros >= 0: one object of 4096 cells, each 1 above the floor
    assert outs[0][:6].view(2, 3).tolist() == [[4096 * q, q * 64 * (63 * 64 // 2), q * 64 * (63 * 64 // 2)]] * 2
    assert outs[1][:24].view(6, 4).tolist() == [[1, 4096, 4096 * q, 4096 * q]] * 6
    assert outs[2][:12].view(6, 2).tolist() == [[float(4096 * q) * 4096.0, 0.0]] * 6
    assert torch.all(outs[0][6:] == -7) and torch.all(outs[1][24:] == -7) and torch.all(outs[2][12:] == -7)
