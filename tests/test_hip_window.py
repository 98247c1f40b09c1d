"""csrc/window.hip through the C ABI against tests/window_ref.py: acg_window_gather (a copy: compared bit for bit) and
acg_window_blend (fp64 reference).  Outputs start as NaN and every buffer ends in guard words (tests/guard_util.py); padded
input channels of the tiles hold NaN / 1e30, so a blend that lets them into a real channel fails.

Bars.  The gather and every singly covered pixel of the blend are copies: bits.  A blended pixel is a convex combination of at
most 3 x 3 tile values in [-1, 1]: nine fp32 multiply-adds, a divide and (in the stated form) the two weight roundings stay
under 16 ulp of 1, so 2e-6 absolute.  Two launches on the same input give the same bits (no atomics).

Measured on the MI355X: blended pixels within 1.1e-7 of the reference, gather then blend within 1.2e-7 of the field; 75 tests in
about 2 s."""
import ctypes

import numpy as np
import pytest

import window_ref as R
from guard_util import Buf, rejected

pytestmark = pytest.mark.gpu

BAR = 2e-6
CS = [1, 3, 4, 5]                                        # stored as 4, 4, 4, 16
PLANS = [(8, 8, 8, 2), (9, 13, 8, 0), (9, 13, 8, 4), (21, 30, 8, 3), (40, 17, 16, 8)]


@pytest.fixture(autouse=True)
def _fresh_buffers():
    Buf.live = []
    yield
    Buf.live = []


def _env():
    from dtgan_amd import _lib, ops
    return _lib, _lib.load(), ops._stream()


def _record(p):
    from dtgan_amd import _lib
    rec = _lib.WindowPlan(H=p["H"], W=p["W"], S=p["S"], R=p["R"], ny=len(p["oy"]), nx=len(p["ox"]))
    rec.oy[:len(p["oy"])], rec.ox[:len(p["ox"])] = p["oy"], p["ox"]
    return rec


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _fields(N, C, H, W, seed):
    f = np.random.RandomState(seed).uniform(-1, 1, (N, C, H, W)).astype(np.float32)
    f[0, 0, 0, 0], f[-1, -1, -1, -1] = -0.0, np.float32(np.nan)      # a copy keeps the sign of zero and a NaN's bits
    return f


def _table(N, H, W, S):
    """origins at 0, at the maximum and in between; all four flips at one origin of one field; every field used"""
    my, mx = H - S, W - S
    rows = [(0, 0, 0, 0), (N - 1, my, mx, 0), (1 % N, my // 2, mx // 2, 0), (0, my, 0, 1), (N - 1, 0, mx, 2)]
    rows += [(1 % N, (my + 1) // 2, mx // 3, f) for f in range(4)]
    rows += [(N - 1, 0, 0, 3), (0, my, mx, 3)]
    return rows


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("H,W,S", [(9, 13, 8), (16, 16, 8), (16, 16, 16)])
def test_gather_is_the_reference_bit_for_bit(C, H, W, S):
    _lib, lib, st = _env()
    N, Cp = 3, R.cimg(C)
    f = _fields(N, C, H, W, seed=C * 100 + H)
    table = _table(N, H, W, S)
    want = R.gather(f, table, S)
    assert want.shape == (len(table), S, S, Cp)
    src, tab, out = Buf.of(f), Buf.of(np.array(table, dtype=np.int32), np.int32), Buf.out(want.size)
    _lib.call("acg_window_gather", src.ptr, tab.ptr, out.ptr, N, C, H, W, len(table), S, Cp, st)
    got = out.host(want.shape)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(got[..., C:]), np.zeros_like(_bits(got[..., C:])))      # padding channels: +0
    Buf.check_all()


def test_gather_through_ops_checks_the_table_before_the_upload():
    import torch
    from dtgan_amd import ops
    f = _fields(2, 3, 9, 13, seed=1)
    x = torch.from_numpy(f).cuda()
    table = _table(2, 9, 13, 8)
    got = ops.window_gather(x, table, 8)
    assert tuple(got.shape) == (len(table), 8, 8, 4)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(R.gather(f, table, 8)))
    assert tuple(ops.window_gather(x, table, 8, img=False).shape) == (len(table), 8, 8, 16)
    seen = []
    again = ops.window_gather(x, table, 8, upload=lambda t: seen.append(t) or t.cuda())
    assert torch.equal(again.view(torch.int32), got.view(torch.int32)) and len(seen) == 1       # bits: the fields hold a NaN
    assert seen[0].dtype == torch.int32 and not seen[0].is_cuda and seen[0].tolist() == [list(r) for r in table]
    for bad in [(2, 0, 0, 0), (0, 2, 0, 0), (0, 0, 6, 0), (0, 0, 0, 4), (0, -1, 0, 0)]:
        with pytest.raises(ValueError):
            ops.window_gather(x, table + [bad], 8)
    with pytest.raises(ValueError):
        ops.window_gather(x, table, 10)


def _tiles(p, rows, C, seed):
    Cp = R.cimg(C)
    t = np.random.RandomState(seed).uniform(-1, 1, (rows * len(p["oy"]) * len(p["ox"]), p["S"], p["S"], Cp)).astype(np.float32)
    if Cp > C:
        pad = np.full(t[..., C:].shape, 1e30, dtype=np.float32)
        pad.reshape(-1)[::2] = np.nan
        t[..., C:] = pad
    return t


def _blend(tiles, p, rows, C):
    _lib, lib, st = _env()
    src, out = Buf.of(tiles), Buf.out(rows * C * p["H"] * p["W"])
    rec = _record(p)
    _lib.call("acg_window_blend", src.ptr, ctypes.byref(rec), out.ptr, rows, C, tiles.shape[-1], st)
    first = out.host((rows, C, p["H"], p["W"]))
    again = Buf.out(first.size)
    _lib.call("acg_window_blend", src.ptr, ctypes.byref(rec), again.ptr, rows, C, tiles.shape[-1], st)
    assert np.array_equal(_bits(first), _bits(again.host(first.shape)))                  # reproducible
    Buf.check_all()
    return first


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("case", PLANS)
def test_blend_against_the_reference(case, C, rows):
    from dtgan_amd import ops
    H, W, S, overlap = case
    p = R.plan(H, W, S, overlap)
    made = ops.window_plan(H, W, S, overlap)
    assert (list(made.oy[:made.ny]), list(made.ox[:made.nx]), made.R) == (p["oy"], p["ox"], p["R"])
    tiles = _tiles(p, rows, C, seed=H * 7 + C + rows)
    got = _blend(tiles, p, rows, C)
    want, cover = R.blend(tiles[..., :C], p, rows, C)
    err = np.abs(got.astype(np.float64) - want).max()
    print("blend %s C=%d rows=%d: max abs err %.3g, cover up to %d" % (case, C, rows, err, cover.max()))
    assert cover.max() <= 9 and err <= BAR, err
    # a pixel under exactly one tile is that tile's value, bit for bit
    ky, kx = R.single_source(p)
    ys, xs = np.nonzero(ky >= 0)
    nx = len(p["ox"])
    for r in range(rows):
        t = (r * len(p["oy"]) + ky[ys, xs]) * nx + kx[ys, xs]
        src = tiles[t, ys - np.array(p["oy"])[ky[ys, xs]], xs - np.array(p["ox"])[kx[ys, xs]], :C]      # (pixels, C)
        assert np.array_equal(_bits(got[r][:, ys, xs].T), _bits(src))


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("case", PLANS)
def test_gather_then_blend_returns_the_field(case, C):
    _lib, lib, st = _env()
    H, W, S, overlap = case
    p, rows, Cp = R.plan(H, W, S, overlap), 2, R.cimg(C)
    f = np.random.RandomState(H + C).uniform(-1, 1, (rows, C, H, W)).astype(np.float32)
    table = R.plan_table(p, rows)
    src, tab = Buf.of(f), Buf.of(np.array(table, dtype=np.int32), np.int32)
    tiles, out = Buf.out(len(table) * S * S * Cp), Buf.out(f.size)
    rec = _record(p)
    _lib.call("acg_window_gather", src.ptr, tab.ptr, tiles.ptr, rows, C, H, W, len(table), S, Cp, st)
    _lib.call("acg_window_blend", tiles.ptr, ctypes.byref(rec), out.ptr, rows, C, Cp, st)
    got = out.host(f.shape)
    err = np.abs(got.astype(np.float64) - f).max()
    print("gather+blend %s C=%d: max abs err %.3g" % (case, C, err))
    assert err <= BAR, err
    Buf.check_all()


def test_rejected_records_and_scalars_never_launch():
    _lib, lib, st = _env()
    p = R.plan(21, 30, 8, 3)
    tiles = _tiles(p, 1, 3, seed=0)
    src, out = Buf.of(tiles), Buf.out(3 * 21 * 30)

    def blend(rec, rows=1, C=3, Cp=4, t=src.ptr, o=out.ptr):
        return rejected(lib, "acg_window_blend", t, ctypes.byref(rec), o, rows, C, Cp, st)

    def changed(**kw):
        q = dict(p, oy=list(p["oy"]), ox=list(p["ox"]))
        q.update(kw)
        return _record(q)
    oy, ox = p["oy"], p["ox"]
    assert len(oy) >= 3 and len(ox) >= 3
    assert "ascend" in blend(changed(oy=[oy[0], oy[1], oy[1]] + oy[3:]))               # a repeated origin
    assert "ascend" in blend(changed(ox=ox[:3] + [ox[2] - 1] + ox[4:]))                # a step back
    assert "first origin" in blend(changed(oy=[1] + oy[1:]))
    assert "first origin" in blend(changed(ox=[1] + ox[1:]))
    assert "last origin" in blend(changed(oy=oy[:-1] + [oy[-1] - 1]))
    assert "last origin" in blend(changed(ox=ox[:-1] + [ox[-1] + 1]))
    assert "last origin" in blend(changed(H=22))
    assert "gap" in blend(changed(oy=[0, 21 - 8]))
    assert "gap" in blend(changed(ox=[0, 30 - 8]))
    for n in (0, 65, -1):
        rec = changed()
        rec.ny = n
        assert "windows along y" in blend(rec)
        rec = changed()
        rec.nx = n
        assert "windows along x" in blend(rec)
    for r in (0, 9, -1):
        assert "ramp" in blend(changed(R=r))
    assert "window" in blend(changed(S=0))
    big = _record(dict(H=4097, W=4097, S=4097, R=1, oy=[0], ox=[0]))
    assert "4096" in blend(big)
    assert "rows" in blend(changed(), rows=0)
    assert "too large" in blend(changed(), rows=0x7fffffff)                            # the grid would pass 2^31 blocks
    for C, Cp in ((0, 4), (5, 4), (3, 8), (3, 0), (17, 16)):
        assert "Cp" in blend(changed(), C=C, Cp=Cp)
    assert "null" in blend(changed(), t=None)
    assert "null" in blend(changed(), o=None)
    assert "null" in rejected(lib, "acg_window_blend", src.ptr, None, out.ptr, 1, 3, 4, st)

    f = Buf.of(_fields(2, 3, 9, 13, seed=2))
    tab = Buf.of(np.array([(0, 0, 0, 0)], dtype=np.int32), np.int32)
    win = Buf.out(8 * 8 * 4)

    def gather(N=2, C=3, H=9, W=13, T=1, S=8, Cp=4, a=f.ptr, b=tab.ptr, c=win.ptr):
        return rejected(lib, "acg_window_gather", a, b, c, N, C, H, W, T, S, Cp, st)
    assert "N >= 1" in gather(N=0) and "T >= 1" in gather(T=0)
    assert "S <= H" in gather(S=0) and "S <= H" in gather(S=10) and "S <= H" in gather(S=9, H=9, W=8)
    for C, Cp in ((0, 4), (5, 4), (3, 8), (3, 0), (17, 16)):
        assert "Cp" in gather(C=C, Cp=Cp)
    assert "too large" in gather(H=0x7fffffff, W=0x7fffffff, S=0x7fffffff, T=0x7fffffff, Cp=16)
    assert "null" in gather(a=None) and "null" in gather(b=None) and "null" in gather(c=None)
    assert "aligned" in gather(c=win.at(1)) and "aligned" in gather(b=tab.at(1))
    # nothing was launched: the outputs are still poisoned
    assert np.all(np.isnan(out.host())) and np.all(np.isnan(win.host()))
    Buf.check_all()
