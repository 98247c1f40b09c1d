"""GPU tests of the one fast-layout rule of the field metrics (csrc/field.h: field_load_mode) through the C ABI of every entry
point that has a 16-byte mode.  An operand that has the shape of a fast layout but lies one float off the 16-byte grid, or
whose row stride is no multiple of 4, must take the scalar path and give the bits of the aligned call; where acg_last_kernel
names the mode it says so.  Values against the references are the business of the entry points' own tests."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from guard_util import Buf

pytestmark = pytest.mark.gpu

ROWS = 2
# (floats past a 16-byte aligned allocation, floats a row lies further from the last than a dense one)
ALIGNED = (0, 0)
FALLBACKS = {"one float off the grid": (1, 0), "odd row stride": (0, 1)}
# entry point, H, W: the sizes at which its kernels change (one workgroup / two passes, two tiles each way, two words per row)
CASES = [("acg_radial_spectrum", 16, 16), ("acg_radial_spectrum_bwd", 16, 16), ("acg_cross_spectrum", 16, 16),
         ("acg_cross_spectrum", 128, 128), ("acg_field_spectrum", 20, 28), ("acg_field_cross_spectrum", 20, 28),
         ("acg_ssim", 27, 43), ("acg_ssim_bwd", 27, 43), ("acg_fss", 16, 70), ("acg_marginal_loss_bwd", 16, 16)]
NAMES_ITS_MODE = ("acg_ssim", "acg_ssim_bwd", "acg_fss", "acg_marginal_loss_bwd")


class Operand(object):
    """vals (rows, C, H, W) on the device in `layout` with Cp stored channels (NHWC: +-50 garbage in the padded ones), its first
    float `offset` floats into a 16-byte aligned allocation and its rows `row_pad` floats further apart than dense ones.
    vals=None: NaN everywhere, a gradient to be written in that geometry"""

    def __init__(self, shape, layout, Cp, offset, row_pad, vals=None, seed=0):
        rows, C, H, W = shape
        if layout == "nhwc":
            self.dense, self.strides = (rows, H, W, Cp), (H * W * Cp + row_pad, Cp, 1)
        else:
            assert Cp == C
            self.dense, self.strides = (rows, C, H, W), (C * H * W + row_pad, 1, H * W)
        self.rows, self.row_len, self.offset = rows, self.strides[0] - row_pad, offset
        host = np.full(offset + rows * self.strides[0] + 4, np.nan, np.float32)
        if vals is not None:
            d = np.ascontiguousarray(vals)
            if layout == "nhwc":
                d = np.random.RandomState(seed).uniform(-50, 50, self.dense).astype(np.float32)
                d[..., :C] = np.moveaxis(vals, 1, 3)
            for r in range(rows):
                self._row(host, r)[:] = d[r].ravel()
        self.t = torch.from_numpy(host).cuda()
        assert self.t.data_ptr() % 16 == 0

    def _row(self, flat, r):
        at = self.offset + r * self.strides[0]
        return flat[at:at + self.row_len]

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + 4 * self.offset)

    def host(self):
        """the rows as a dense array; every float around and between them must still be the NaN it was"""
        torch.cuda.synchronize()
        flat = self.t.cpu().numpy()
        out = np.stack([self._row(flat, r).copy() for r in range(self.rows)]).reshape(self.dense)
        for r in range(self.rows):
            self._row(flat, r)[:] = np.nan
        assert np.all(np.isnan(flat)), "a float outside the operand's rows was written"
        return out


@functools.lru_cache(maxsize=None)
def _values(H, W):
    """a correlated pair (ROWS, 3, H, W), read-only, the same for every placement"""
    rs = np.random.RandomState(1000 * H + W)
    x = rs.standard_normal((ROWS, 3, H, W)).astype(np.float32)
    y = (0.6 * x + 0.8 * rs.standard_normal(x.shape)).astype(np.float32)
    x.setflags(write=False), y.setflags(write=False)
    return x, y


def _workspace(nbytes):
    return Buf.out((nbytes + 3) // 4 + 4, np.uint32)


def run(entry, H, W, layout="nhwc", C=3, Cp=4, offset=0, row_pad=0):
    """the entry point on the seeded values in that placement (of every operand, and of a gradient it writes) ->
    (its outputs as host arrays, what acg_last_kernel names)"""
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    xv, yv = _values(H, W)
    shape = (ROWS, C, H, W)
    x = Operand(shape, layout, Cp, offset, row_pad, xv[:, :C], seed=1)
    y = Operand(shape, layout, Cp, offset, row_pad, yv[:, :C], seed=2)
    gx = Operand(shape, layout, Cp, offset, row_pad)
    rs = np.random.RandomState(7)
    n, st, one = ROWS * C, ops._stream(), Buf.of([0.75])
    if entry in ("acg_radial_spectrum", "acg_radial_spectrum_bwd", "acg_cross_spectrum"):
        assert H == W
        nb = H // 2 + 1
        need = getattr(lib, entry + "_workspace_bytes")(ROWS, C, H)
        ws = _workspace(need)
        if entry == "acg_radial_spectrum":
            out = Buf.out(n * nb)
            rc = lib.acg_radial_spectrum(x.ptr, ROWS, C, H, *x.strides, out.ptr, ws.ptr, need, st)
        elif entry == "acg_cross_spectrum":
            out = Buf.out(n * 3 * nb)
            rc = lib.acg_cross_spectrum(x.ptr, y.ptr, ROWS, 1, C, H, *x.strides, *y.strides, out.ptr, ws.ptr, need, st)
        else:
            g, out = Buf.of(rs.standard_normal((n, nb))), gx
            rc = lib.acg_radial_spectrum_bwd(x.ptr, g.ptr, ROWS, C, Cp, H, *x.strides, gx.ptr, ws.ptr, need, st)
        outs = [out]
    elif entry in ("acg_field_spectrum", "acg_field_cross_spectrum"):
        nb = min(H, W) // 2 + 1
        need = getattr(lib, entry + "_workspace_bytes")(ROWS, C, H, W)
        ws = _workspace(need)
        if entry == "acg_field_spectrum":
            out = Buf.out(n * nb)
            rc = lib.acg_field_spectrum(x.ptr, ROWS, C, H, W, *x.strides, out.ptr, ws.ptr, need, st)
        else:
            out = Buf.out(n * 3 * nb)
            rc = lib.acg_field_cross_spectrum(x.ptr, y.ptr, ROWS, 1, C, H, W, *x.strides, *y.strides, out.ptr, ws.ptr, need, st)
        outs = [out]
    elif entry == "acg_ssim":
        need = lib.acg_ssim_workspace_bytes(ROWS, C, H, W)
        ws, out, maps = _workspace(need), Buf.out(n * 2), Buf.out(3 * n * (H - 10) * (W - 10))
        rc = lib.acg_ssim(x.ptr, y.ptr, ROWS, 1, C, H, W, *x.strides, *y.strides, 2.0, out.ptr, maps.ptr, ws.ptr, need, st)
        outs = [out, maps]
    elif entry == "acg_ssim_bwd":
        maps = Buf.of(rs.standard_normal((3, n, H - 10, W - 10)))
        rc = lib.acg_ssim_bwd(maps.ptr, x.ptr, y.ptr, one.ptr, ROWS, C, Cp, H, W, *x.strides, *y.strides, gx.ptr, st)
        outs = [gx]
    elif entry == "acg_fss":
        thr, win = Buf.of(np.linspace(-0.3, 0.3, C).reshape(C, 1)), (ctypes.c_int * 2)(1, 3)
        need = lib.acg_fss_workspace_bytes(ROWS, 1, C, H, W, 1, 2, 0)
        ws, out = _workspace(need), Buf.out(n * 2 * 3 * 2, np.uint32)             # (rows, C, 1, 2, 3) int64
        rc = lib.acg_fss(x.ptr, y.ptr, ROWS, 1, C, H, W, *x.strides, *y.strides, thr.ptr, 1, win, 2, out.ptr, None, ws.ptr, need, st)
        outs = [out]
    elif entry == "acg_marginal_loss_bwd":
        P = H * W
        d = Buf.of(rs.standard_normal((C, P)))
        rank = Buf.of(np.stack([rs.permutation(P) for _ in range(n)]), np.int32)
        rc = lib.acg_marginal_loss_bwd(d.ptr, rank.ptr, one.ptr, ROWS, C, Cp, H, W, *x.strides, gx.ptr, st)
        outs = [gx]
    else:
        raise ValueError(entry)
    assert rc == 0, (entry, lib.acg_last_error().decode())
    note = _lib.query("acg_last_kernel").decode()
    got = [o.host() for o in outs]
    Buf.check_all()
    return got, note


def _same_bits(got, want):
    return len(got) == len(want) and all(a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
                                         for a, b in zip(got, want))


def _written(outs):
    """no element is the poison it started as: NaN of a float output, all ones of an integer one"""
    return all(not np.any(np.isnan(a) if a.dtype == np.float32 else a.view(np.uint64) == np.uint64(2 ** 64 - 1)) for a in outs)


@pytest.mark.parametrize("entry, H, W", CASES)
def test_a_c4_operand_off_the_grid_or_with_an_odd_row_stride_gives_the_aligned_bits(entry, H, W):
    want, note = run(entry, H, W, "nhwc", 3, 4, *ALIGNED)
    assert _written(want), entry
    if entry in NAMES_ITS_MODE:
        assert "c4" in note, note
    for what, (offset, row_pad) in FALLBACKS.items():
        got, other = run(entry, H, W, "nhwc", 3, 4, offset, row_pad)
        assert _same_bits(got, want), (entry, what, other)
        if entry in NAMES_ITS_MODE:
            assert "c4" not in other and ("strided" in other or "scalar" in other), (what, other)


@pytest.mark.parametrize("entry", ["acg_radial_spectrum", "acg_radial_spectrum_bwd", "acg_cross_spectrum"])
def test_a_planar_operand_off_the_grid_gives_the_aligned_bits(entry):
    want, _ = run(entry, 16, 16, "nchw", 3, 3, *ALIGNED)
    assert _written(want), entry
    for what, (offset, row_pad) in FALLBACKS.items():
        got, _ = run(entry, 16, 16, "nchw", 3, 3, offset, row_pad)
        assert _same_bits(got, want), (entry, what)
