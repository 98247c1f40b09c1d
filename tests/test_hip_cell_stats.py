"""GPU tests of the per-cell statistics: acg_cell_stats through the C ABI against tests/cell_stats_ref.py for EQUALITY on every
plane, the doubles included (the definition fixes each rounding and the order; only the sign and payload of a NaN are left
open), in every layout, at the sizes where the index arithmetic changes, on a non-zero starting state between guard words,
for rows given in one call and in calls of 1 + rest, repeated and replayed from a graph, and every refusal in its order."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cell_stats_ref as R
from field_cases import field_operand
from guard_util import Buf

pytestmark = pytest.mark.gpu

# (layout x, stored channels x (0: planar), floats off the 16-byte grid, the same for y): planar; a pixel's channels in one
# 16-byte load on either side or both; a wide pixel; operands shifted off the grid
LAYOUTS = (("nchw", 0, None, "nchw", 0, None), ("nhwc", 4, 0, "nchw", 0, None), ("nhwc", 4, 0, "nhwc", 4, 0), ("nchw", 0, None, "nhwc", 4, 0),
           ("nhwc", 16, 0, "nhwc", 16, 0), ("nhwc", 4, 1, "nchw", 0, 1), ("nchw", 0, 3, "nhwc", 4, 2))
# (H, W, C, M, T, E, Ny): 255, 256 and 257 cells lie around a workgroup's worth; W = 63 .. 65 and 1 x 67 / 67 x 1 around a wave's
CASES = ((1, 1, 1, 1, 0, 0, 4), (1, 67, 3, 2, 1, 1, 3), (67, 1, 4, 3, 8, 63, 3), (5, 63, 5, 2, 1, 5, 3), (4, 64, 3, 64, 8, 1, 2),
         (3, 65, 3, 3, 1, 63, 3), (16, 16, 3, 2, 1, 3, 3), (15, 17, 4, 1, 8, 0, 3), (1, 257, 1, 3, 0, 7, 3), (9, 1024, 3, 2, 1, 4, 2),
         (321, 321, 1, 2, 1, 3, 2))


@functools.lru_cache(maxsize=None)
def _case(H, W, C, M, T, E, Ny):
    """members, truths, tables, a non-zero starting state (the reference on rows of their own) and the reference after the rows"""
    thr, edges = R.tables(C, T, E, seed=H + W)
    x, y = R.fields(Ny, M, C, H, W, seed=M + 7 * T, thr=thr, edges=edges)
    x0, y0 = R.fields(2, M, C, H, W, seed=99, thr=thr, edges=edges, special=False)
    start = R.accumulate(R.new_state(C, H, W, T, E), x0, y0, M, thr, edges)
    ref = R.accumulate(R.copy_state(start), x, y, M, thr, edges)
    for a in (x, y, thr, edges) + tuple(start.values()) + tuple(ref.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x, y, thr, edges, start, ref


def _strides(t, layout):
    """(row, pixel, channel) strides in floats of a contiguous operand"""
    if layout == "nhwc":
        _, H, W, Cp = t.shape
        return H * W * Cp, Cp, 1
    _, Cs, H, W = t.shape
    return Cs * H * W, 1, H * W


def _operand(a, layout, C, cp, off, seed):
    return field_operand(a, layout, C, max(cp, 8) if (cp and C > 4) else cp, seed=seed, nan=0.2, off=off)


class State(object):
    """a state in guarded device buffers, started from host arrays"""
    WORDS = dict(mom=(np.float64, 2), evt=(np.int64, 2), hist_x=(np.int32, 1), hist_y=(np.int32, 1))

    def __init__(self, start):
        self.start = start
        self.buf = {k: None if start[k] is None else Buf(start[k].size * w, start[k], dt) for k, (dt, w) in self.WORDS.items()}

    def ptr(self, k):
        return None if self.buf[k] is None else self.buf[k].ptr

    def host(self, n, M):
        out = {k: None if b is None else b.host(self.start[k].shape) for k, b in self.buf.items()}      # checks the guard words
        out.update(n=n, M=M)
        return out


def _call(lib, xd, lx, yd, ly, rows, M, C, H, W, thr_d, T, edges_d, E, st, x_from=0):
    from dtgan_amd import ops
    sx, sy = _strides(xd, lx), _strides(yd, ly)
    px = ctypes.c_void_p(xd.data_ptr() + 4 * x_from * M * sx[0])
    py = ctypes.c_void_p(yd.data_ptr() + 4 * x_from * sy[0])
    rc = lib.acg_cell_stats(px, py, rows, M, C, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], ops._ptr(thr_d), T, ops._ptr(edges_d), E,
                            st.ptr("mom"), st.ptr("evt"), st.ptr("hist_x"), st.ptr("hist_y"), ops._stream())
    assert rc == 0, lib.acg_last_error().decode()


def _dev(a):
    return None if a is None else torch.from_numpy(a.copy()).cuda()


@pytest.mark.parametrize("H,W,C,M,T,E,Ny", CASES)
def test_kernel_equals_the_reference_in_every_layout_and_split(H, W, C, M, T, E, Ny):
    from dtgan_amd import _lib
    lib = _lib.load()
    x, y, thr, edges, start, ref = _case(H, W, C, M, T, E, Ny)
    thr_d, edges_d = _dev(thr), _dev(edges)
    first = None
    for i, (lx, cpx, ox, ly, cpy, oy) in enumerate(LAYOUTS if H * W < 20000 else LAYOUTS[:3]):
        if C > 4 and i in (2, 3):                                  # five channels do not fit a 16-byte pixel: covered by the wide one
            continue
        xd, yd = _operand(x, lx, C, cpx, ox, 1), _operand(y, ly, C, cpy, oy, 2)
        st = State(start)
        _call(lib, xd, lx, yd, ly, Ny * M, M, C, H, W, thr_d, T, edges_d, E, st)
        got = st.host(start["n"] + Ny, M)
        for k in ("mom", "evt", "hist_x", "hist_y"):
            assert (got[k] is None and ref[k] is None) or R.same(got[k], ref[k]), (k, lx, cpx, ox, ly, cpy, oy)
        c4 = lambda lay, cp, off: "c4" if (lay == "nhwc" and cp == 4 and C <= 4 and not off) else "strided"
        want = "cell_mom<%s, %s>%s%s" % (c4(lx, cpx, ox), c4(ly, cpy, oy), " + cell_evt" if T else "", " + cell_hist" if E else "")
        assert _lib.query("acg_last_kernel").decode() == want
        if first is None:
            first = got
        else:                                                      # the same bits in every layout, the NaNs' included
            assert all(got[k] is None or got[k].tobytes() == first[k].tobytes() for k in ("mom", "evt", "hist_x", "hist_y"))
        # the rows in calls of 1 truth + the rest: the same bits
        st2 = State(start)
        _call(lib, xd, lx, yd, ly, M, M, C, H, W, thr_d, T, edges_d, E, st2)
        _call(lib, xd, lx, yd, ly, (Ny - 1) * M, M, C, H, W, thr_d, T, edges_d, E, st2, x_from=1)
        split = st2.host(start["n"] + Ny, M)
        assert all(split[k] is None or split[k].tobytes() == got[k].tobytes() for k in ("mom", "evt", "hist_x", "hist_y")), (lx, ly)
    if E:
        assert np.all(first["hist_x"].sum(1) == (start["n"] + Ny) * M) and np.all(first["hist_y"].sum(1) == start["n"] + Ny)
    Buf.check_all()


def test_parts_off_leave_their_buffers_alone_and_match():
    """T = 0 or E = 0 through the op: the moments are those of the full call"""
    from dtgan_amd import ops
    H, W, C, M, T, E, Ny = CASES[6]
    x, y, thr, edges, start, ref = _case(H, W, C, M, T, E, Ny)
    xd, yd = _operand(x, "nhwc", C, 4, 0, 1), _operand(y, "nchw", C, 0, None, 2)
    zero = R.accumulate(R.new_state(C, H, W, T, E), x, y, M, thr, edges)
    for t, e in ((thr, edges), (None, edges), (thr, None), (None, None)):
        s = ops.cell_state(C, H, W, 0 if t is None else T, 0 if e is None else E, "cuda")
        assert ops.cell_stats(xd, yd, C, "nhwc", "nchw", s, thresholds=t, edges=e, x_per_y=M) is s
        assert s["n"] == Ny and s["M"] == M and (s["evt"] is None) == (t is None) and (s["hist_x"] is None) == (e is None)
        for k in ("mom", "evt", "hist_x", "hist_y"):
            assert s[k] is None or R.same(s[k].cpu().numpy(), zero[k]), k


def test_repeatable_and_the_same_bits_replayed_from_a_graph():
    from dtgan_amd import ops
    H, W, C, M, T, E, Ny = 33, 65, 3, 3, 2, 9, 3
    x, y, thr, edges, start, ref = _case(H, W, C, M, T, E, Ny)
    xd, yd = _operand(x, "nhwc", C, 4, 0, 1), _operand(y, "nchw", C, 0, None, 2)
    thr_d, edges_d = _dev(thr), _dev(edges)
    parts = ("mom", "evt", "hist_x", "hist_y")

    def fresh():
        s = ops.cell_state(C, H, W, T, E, "cuda")
        for k in parts:
            s[k].copy_(torch.from_numpy(start[k].copy()))
        s.update(n=start["n"], M=M)
        return s
    s = fresh()
    call = lambda: ops.cell_stats(xd, yd, C, "nhwc", "nchw", s, thresholds=thr_d, edges=edges_d, x_per_y=M)
    call()
    one = {k: s[k].cpu().numpy() for k in parts}
    assert all(R.same(one[k], ref[k]) for k in parts) and s["n"] == ref["n"]
    again = fresh()
    ops.cell_stats(xd, yd, C, "nhwc", "nchw", again, thresholds=thr_d, edges=edges_d, x_per_y=M)
    assert all(again[k].cpu().numpy().tobytes() == one[k].tobytes() for k in parts)
    for k in parts:
        s[k].copy_(torch.from_numpy(start[k].copy()))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    for k in parts:
        s[k].copy_(torch.from_numpy(start[k].copy()))
    graph.replay()
    torch.cuda.synchronize()
    assert all(s[k].cpu().numpy().tobytes() == one[k].tobytes() for k in parts)


def test_kernel_refuses_bad_arguments_in_the_documented_order():
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    x = torch.zeros(1 << 14, device="cuda")
    tab = torch.zeros(64, device="cuda")
    state = torch.full((1 << 18,), -7, dtype=torch.int32, device="cuda")
    MOM, EVT, HX, HY = 0, 327680, 458752, 524288                   # byte offsets: 9 x 4096 doubles, 4 x 4096 int64, 2 x 3 x 4096 int32
    at = lambda byte: ctypes.c_void_p(state.data_ptr() + byte)
    P = (4096, 1, 4096)
    # everything wrong at once; mending the first refusal shows the next: (what to mend, the word of the refusal it mends)
    args = dict(xd=None, yd=None, rows=0, per=0, C=0, H=0, W=1025, sx=(0, 1, 4096), sy=(4096, 1, -1), thr=None, T=9, edges=None, E=64,
                mom=None, evt=None, hx=None, hy=None)
    steps = ((dict(rows=2), "rows >= 1"), (dict(C=1), "C >= 1"), (dict(sx=P), "strides"), (dict(sy=P), "strides"), (dict(per=3), "x_per_y"),
             (dict(per=65, rows=130), "x_per_y"), (dict(per=1, rows=2), "x_per_y"), (dict(xd=x), "null"), (dict(yd=x), "null"),
             (dict(mom=at(MOM + 4)), "null"), (dict(H=64), "H x W"), (dict(W=64), "H x W"), (dict(T=-1), "thresholds"), (dict(T=1), "thresholds"),
             (dict(thr=tab), "thresholds"), (dict(evt=at(EVT + 4)), "thresholds"), (dict(E=-1), "edges"), (dict(E=2), "edges"),
             (dict(edges=tab), "edges"), (dict(hx=at(HX + 2)), "edges"), (dict(hy=at(HY + 1)), "edges"), (dict(mom=at(MOM)), "aligned"),
             (dict(evt=at(EVT)), "aligned"), (dict(hx=at(HX)), "aligned"), (dict(hy=at(HY)), "aligned"))

    def call():
        a = dict(args)
        return lib.acg_cell_stats(ops._ptr(a["xd"]), ops._ptr(a["yd"]), a["rows"], a["per"], a["C"], a["H"], a["W"], a["sx"][0], a["sx"][1],
                                  a["sx"][2], a["sy"][0], a["sy"][1], a["sy"][2], ops._ptr(a["thr"]), a["T"], ops._ptr(a["edges"]), a["E"],
                                  a["mom"], a["evt"], a["hx"], a["hy"], ops._stream())
    for mend, word in steps:
        rc = call()
        msg = lib.acg_last_error().decode()
        assert rc == -1 and msg.startswith("acg_cell_stats") and word in msg, (mend, word, rc, msg)
        args.update(mend)
    torch.cuda.synchronize()
    assert torch.all(state == -7)                                  # nothing was written by any of them
    state.zero_()
    assert call() == 0, lib.acg_last_error().decode()              # and the mended call passes: 64 x 64 x (9 doubles, 4 int64, 2 x 3 bins)
    torch.cuda.synchronize()
    assert state[HX // 4:HX // 4 + 12288].view(3, 4096).sum(0).eq(2).all() and state[HY // 4 + 12288:].eq(0).all()   # 2 rows per cell
    with pytest.raises(_lib.AcgError, match="cell_stats: .*M=2"):
        s = ops.cell_state(1, 8, 8, 0, 0, "cuda")
        s["M"] = 2
        ops.cell_stats(x[:128].view(2, 1, 8, 8), x[:128].view(2, 1, 8, 8), 1, "nchw", "nchw", s)
