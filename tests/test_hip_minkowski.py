"""GPU tests of the Minkowski counts: acg_minkowski, through ops.minkowski and through the C ABI, against
tests/minkowski_ref.py for equality (the kernel is integer after the comparison: no tolerance anywhere), in every layout, at
the shapes where its index arithmetic changes, and its refusals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import minkowski_ref as K
from field_cases import OFFSET_LAYOUTS as LAYOUTS, offset_operand as _device
from guard_util import GUARD, Buf

pytestmark = pytest.mark.gpu

BAND = 8                   # lattice rows per workgroup (csrc/minkowski.hip MK_BAND); a field of H rows has H + 1 lattice rows
# 1 x 1 and single rows / columns; off the 64-lane and the 4-byte tile grid both ways; lattices of BAND - 1 .. BAND + 2 rows;
# a row as wide as allowed (the largest LDS tile); the native grid
SIZES = ((1, 1), (1, 64), (64, 1), (63, 65), (65, 63), (17, 129), (BAND - 2, 5), (BAND - 1, 5), (BAND, 5), (BAND + 1, 5), (9, 1024),
         (321, 321))
# (T, C): one threshold, two, the evaluator's default and the most; one channel, three and four
TC = ((1, 1), (2, 3), (31, 4), (255, 3))
@functools.lru_cache(maxsize=None)
def _case(kind, H, W, T, C):
    """two rows of C fields, their thresholds (with repeats from T = 31 on) and the reference counts; left unchanged"""
    thr = K.make_thresholds(C, T, seed=T + C, duplicates=T >= 31)
    x = K.make_fields(kind, 2, C, H, W, thr, seed=T)
    ref = K.counts(x, thr)
    for a in (thr, x, ref):
        a.setflags(write=False)
    return x, thr, ref


def _mink(xd, C, layout, thr):
    """ops.minkowski into a poisoned output -> host int64 (rows, C, T, 5)"""
    from dtgan_amd import ops
    out = torch.full((xd.shape[0], C, thr.shape[1], 5), -7, dtype=torch.int64, device="cuda")
    assert ops.minkowski(xd, C, layout, thr, out=out) is out
    return out.cpu().numpy()


def _path(layout, Cp, off):
    return "mink_hist<%s> + mink_finish" % ("c4" if (layout, Cp, off) == ("nhwc", 4, 0) else "strided")


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("H,W", SIZES)
def test_kernel_equals_the_reference_in_every_layout(H, W, kind):
    from dtgan_amd import _lib
    for T, C in (TC if H * W < 100000 else TC[2:]):
        x, thr, ref = _case(kind, H, W, T, C)
        for layout, Cp, off in LAYOUTS:
            got = _mink(_device(x, layout, Cp, off, seed=T), C, layout, thr)
            assert _lib.query("acg_last_kernel").decode() == _path(layout, Cp, off)
            assert got.dtype == np.int64 and got.shape == (2, C, T, 5)
            assert np.array_equal(got, ref), (kind, H, W, T, C, layout, Cp, off, np.argwhere(got != ref)[:5])
    if kind == "constant":                                         # every pixel on a threshold: a rectangle at and below it
        f = K.functionals(ref)
        assert set(np.unique(f["area"])) <= {0, H * W} and set(np.unique(f["euler8"])) <= {0, 1}


def test_one_large_field():
    """1024 x 1024, one channel, 255 thresholds: 129 bands, the largest counts (2 * 1025 * 1024 edges at the lowest level)"""
    from dtgan_amd import _lib
    thr = K.make_thresholds(1, 255, seed=9, duplicates=True)
    x = K.make_fields("smooth", 1, 1, 1024, 1024, thr, seed=9)
    x[0, 0, :, 512:] = 1.3                                         # half the field above every threshold
    ref = K.counts(x, thr)
    assert ref[0, 0, 0, 1] > 1 << 20 and ref[0, 0, -1, 0] >= 512 * 1024
    for layout, Cp in (("nchw", 0), ("nhwc", 4)):
        got = _mink(_device(x, layout, Cp), 1, layout, thr)
        assert _lib.query("acg_last_kernel").decode() == _path(layout, Cp, 0)
        assert np.array_equal(got, ref), (layout, np.argwhere(got != ref)[:5])


def test_device_thresholds_and_a_fresh_output():
    """thresholds already on the device are taken as they are; without `out` a new int64 tensor comes back; nothing requires grad"""
    from dtgan_amd import ops
    x, thr, ref = _case("special", 17, 129, 31, 4)
    xd = _device(x, "nhwc", 4).requires_grad_(True)
    got = ops.minkowski(xd, 4, "nhwc", torch.from_numpy(thr.copy()).cuda())
    assert got.dtype == torch.int64 and got.is_cuda and not got.requires_grad and np.array_equal(got.cpu().numpy(), ref)
    sub = ops.minkowski(xd, 2, "nhwc", thr[:2])                    # the first two of four stored channels
    assert np.array_equal(sub.cpu().numpy(), ref[:, :2])
    summary = ops.minkowski_summary(got.sum(0).cpu().numpy(), 2 * 17 * 129)
    want = K.functionals(ref.sum(0))
    assert all(np.array_equal(summary[k], want[k].astype(np.float64)) for k in want)


def _abi_call(lib, xd, rows, C, H, W, sx, thr_d, T, out, ws, nbytes):
    from dtgan_amd import ops
    return lib.acg_minkowski(ops._ptr(xd), rows, C, H, W, sx[0], sx[1], sx[2], ops._ptr(thr_d), T, out, ws, nbytes, ops._stream())


@pytest.mark.parametrize("H,W,T", ((5, 7, 2), (65, 63, 31), (64, 64, 255)))
def test_guard_words_poison_and_repeatability(H, W, T):
    """through the C ABI: the output starts poisoned and lies, like the 0xFF-filled workspace, between guard words; two calls
    give the same bits, whatever the first left in the workspace"""
    from dtgan_amd import _lib
    lib = _lib.load()
    rows, C = 2, 3
    x, thr, ref = _case("special", H, W, T, C)
    thr_d = torch.from_numpy(thr.copy()).cuda()
    need = lib.acg_minkowski_workspace_bytes(rows, C, H, W, T)
    assert need % 16 == 0 and need >= rows * C * ((H + 1 + BAND - 1) // BAND) * 5 * T * 4
    n_out = rows * C * T * 5
    for layout, Cp, sx in (("nhwc", 4, (H * W * 4, 4, 1)), ("nhwc", 16, (H * W * 16, 16, 1)), ("nchw", 0, (C * H * W, 1, H * W))):
        xd = _device(x, layout, Cp, seed=3)
        out = Buf.out(GUARD + 2 * n_out, np.uint32)
        ws = Buf(GUARD + need // 4, dtype=np.uint32)               # 0xFFFFFFFF everywhere
        firsts = []
        for call in range(2):
            rc = _abi_call(lib, xd, rows, C, H, W, sx, thr_d, T, out.at(GUARD), ws.at(GUARD), need)
            assert rc == 0, lib.acg_last_error().decode()
            o = out.host()                                         # checks the words behind the buffer
            assert np.all(o[:GUARD] == 0xFFFFFFFF)                 # and these are the words in front of it
            firsts.append(o[GUARD:].copy())
            assert np.array_equal(o[GUARD:].view(np.int64).reshape(ref.shape), ref), (layout, Cp, call)
            assert np.all(ws.host()[:GUARD] == 0xFFFFFFFF)
        assert np.array_equal(firsts[0], firsts[1])
    Buf.check_all()


def test_kernel_refuses_bad_arguments_before_launching():
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    x = torch.zeros(1 << 16, device="cuda")
    thr_d = torch.zeros(256, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    big = ws.numel()
    need = lib.acg_minkowski_workspace_bytes(2, 1, 64, 64, 3)
    assert need == (2 * 9 * 5 * 3 * 4 + 15) // 16 * 16            # two rows of nine bands, rounded up to 16 bytes
    P = (4096, 1, 4096)
    # rows, C, H, W, strides, T, x?, thr?, out?, workspace offset, bytes, status, a word of the message
    bad = [(2, 1, 64, 64, P, 3, 0, 1, 1, 0, big, -1, "null"), (2, 1, 64, 64, P, 3, 1, 0, 1, 0, big, -1, "null"),
           (2, 1, 64, 64, P, 3, 1, 1, 0, 0, big, -1, "null"), (2, 1, 0, 64, P, 3, 1, 1, 1, 0, big, -1, "H x W"),
           (2, 1, 64, 1025, P, 3, 1, 1, 1, 0, big, -1, "H x W"), (2, 1, 1025, 4, P, 3, 1, 1, 1, 0, big, -1, "H x W"),
           (0, 1, 64, 64, P, 3, 1, 1, 1, 0, big, -1, "rows >= 1"), (2, 0, 64, 64, P, 3, 1, 1, 1, 0, big, -1, "C >= 1"),
           (2, 1, 64, 64, P, 0, 1, 1, 1, 0, big, -1, "thresholds"), (2, 1, 64, 64, P, 256, 1, 1, 1, 0, big, -1, "thresholds"),
           (2, 1, 64, 64, P, -1, 1, 1, 1, 0, big, -1, "thresholds"), (1 << 30, 4, 8, 8, P, 1, 1, 1, 1, 0, big, -1, "too many"),
           (1 << 24, 1, 8, 8, P, 255, 1, 1, 1, 0, big, -1, "too many"),
           (2, 1, 64, 64, (0, 1, 4096), 3, 1, 1, 1, 0, big, -1, "strides"), (2, 1, 64, 64, (4096, 0, 4096), 3, 1, 1, 1, 0, big, -1, "strides"),
           (2, 1, 64, 64, (4096, 1, -1), 3, 1, 1, 1, 0, big, -1, "strides"),
           (2, 1, 64, 64, P, 3, 1, 1, 1, 0, need - 1, -2, "workspace too small"), (2, 1, 64, 64, P, 3, 1, 1, 1, 8, need, -1, "aligned")]
    for rows, C, H, W, sx, T, has_x, has_thr, has_out, off, nbytes, rc_want, word in bad:
        out = torch.full((4096,), -7, dtype=torch.int64, device="cuda")
        rc = _abi_call(lib, x if has_x else None, rows, C, H, W, sx, thr_d if has_thr else None, T, ops._ptr(out) if has_out else None,
                       ctypes.c_void_p(ws.data_ptr() + off), nbytes)
        msg = lib.acg_last_error().decode()
        assert rc == rc_want and msg.startswith("acg_minkowski") and word in msg, (rows, C, H, W, sx, T, rc, msg)
        torch.cuda.synchronize()
        assert torch.all(out == -7)                                # nothing was written
    rc = _abi_call(lib, x, 2, 1, 64, 64, P, thr_d, 3, ops._ptr(out), None, 0)
    assert rc == -2 and torch.all(out == -7)                       # a missing workspace
    rc = _abi_call(lib, x, 2, 1, 64, 64, P, thr_d, 3, ops._ptr(out), ctypes.c_void_p(ws.data_ptr()), need)
    assert rc == 0, lib.acg_last_error().decode()                  # and the same call with what it asks for
    torch.cuda.synchronize()
    assert out[:30].view(2, 3, 5)[:, :, 0].eq(4096).all() and torch.all(out[30:] == -7)      # zeros >= 0: every cell in every set
