"""GPU tests of the reliability tables: acg_reliability against tests/reliability_ref.py for equality (the kernel is integer:
no tolerance anywhere) in every layout, at the sizes where the word and row arithmetic changes, for every slice count of the
members' carry-save sum, between guard words, on a 0xFF-filled workspace, repeated and replayed from a graph, against
ops.fss's ensemble triple at window 1, and every refusal in its documented order."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fss_ref as F
import reliability_ref as R
from field_cases import field_operand as _device
from guard_util import GUARD, Buf

pytestmark = pytest.mark.gpu

LAYOUTS = (("nchw", 0, "nhwc", 4), ("nhwc", 4, "nchw", 0), ("nhwc", 16, "nhwc", 16), ("nchw", 0, "nchw", 0), ("nhwc", 4, "nhwc", 4))
EIGHT = (1, 3, 5, 9, 17, 33, 63, 65)
# (H, W, M, T, windows, kind): the word count changes at W = 64 | 65 and 128 | 129, the row band at H = 1, 2 and above the
# radius; M = 1, 2, 3, 4, 7, 8, 16, 64 take 1, 2, 2, 3, 3, 4, 5, 7 slices; 15 and 65 are wider than the small domains
CASES = ((1, 1, 1, 1, (1, 3), "noise"), (1, 7, 2, 1, (1, 3, 15), "nan"), (7, 1, 3, 8, (1, 3, 65), "ties"), (5, 63, 4, 1, (1, 3, 65), "noise"),
         (2, 64, 7, 1, (1, 3, 65), "nan"), (33, 65, 8, 1, EIGHT, "shifted"), (3, 128, 16, 1, (3,), "noise"), (2, 129, 64, 1, (1, 65), "noise"),
         (9, 1024, 3, 1, (1, 3, 65), "nan"), (33, 31, 2, 8, (65,), "extremes"), (17, 70, 1, 1, (1, 3, 65), "ties"))
LDS_MAX = 64 * 1024 - 1024


@functools.lru_cache(maxsize=None)
def _case(H, W, M, T, win, kind, C=3, groups=2):
    """members (groups M, C, H, W), truths (groups, C, H, W), thresholds (C, T) and the reference tables"""
    x, _, thr3 = F.make_pair(kind, H, W, rows=groups * M, C=C, seed=M)
    y = F.make_pair(kind, H, W, rows=groups, C=C, seed=M + 50)[1]
    thr = thr3[:, :1] if T == 1 else np.concatenate([thr3, thr3[:, :1] + np.float32([-0.5, 0.25, 0.5, 1.0, 2.0])], 1)
    thr = np.ascontiguousarray(thr, dtype=np.float32)
    ref = R.tables(x, y, thr, win, M)
    for a in (x, y, thr, ref):
        a.setflags(write=False)
    return x, y, thr, ref


def _rel(xd, yd, C, lx, ly, thr, win, M):
    """ops.reliability into a poisoned output -> host int64"""
    from dtgan_amd import ops
    out = torch.full((xd.shape[0] // M, C, thr.shape[1], len(win), M + 1, 2), -7, dtype=torch.int64, device="cuda")
    assert ops.reliability(xd, yd, C, lx, ly, thr[:C], win, x_per_y=M, out=out) is out
    return out.cpu().numpy()


def _abi_call(lib, xd, yd, rows, per, C, H, W, sx, sy, thr_d, T, win, table, ws, nbytes):
    from dtgan_amd import ops
    warr = None if win is None else (ctypes.c_int * max(len(win), 1))(*win)
    return lib.acg_reliability(None if xd is None else ops._ptr(xd), None if yd is None else ops._ptr(yd), rows, per, C, H, W,
                               sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], None if thr_d is None else ops._ptr(thr_d), T, warr,
                               0 if win is None else len(win), table, ws, nbytes, ops._stream())


@pytest.mark.parametrize("H,W,M,T,win,kind", CASES)
def test_kernel_equals_the_reference(H, W, M, T, win, kind):
    from dtgan_amd import _lib
    x, y, thr, ref = _case(H, W, M, T, win, kind)
    assert ref.shape == (2, 3, T, len(win), M + 1, 2) and np.all(ref.sum((-2, -1)) == H * W)
    for i, (lx, cpx, ly, cpy) in enumerate(LAYOUTS):
        C = 3 if i < 4 else 1
        got = _rel(_device(x, lx, C, cpx, seed=1), _device(y, ly, C, cpy, seed=2), C, lx, ly, thr, win, M)
        assert got.dtype == np.int64 and np.array_equal(got, ref[:, :C]), (lx, cpx, ly, cpy, np.argwhere(got != ref[:, :C])[:5])
        resident = (M + 1) * H * ((W + 63) // 64) * 8 <= LDS_MAX
        want = "fss_events<%s> + fss_rel<%s>" % ("c4" if cpx == 4 else "strided", "lds" if resident else "global")
        assert _lib.query("acg_last_kernel").decode() == want


@pytest.mark.parametrize("H,W,M,T,win,kind", (CASES[1], CASES[5], CASES[8]))
def test_guard_words_a_poisoned_output_and_a_filled_workspace(H, W, M, T, win, kind):
    """through the C ABI: the table starts as 0xFF.. between guard words, the workspace is 0xFF-filled between guard words, and
    NaN and +-50 garbage in the padded channels of either operand changes nothing"""
    from dtgan_amd import _lib
    lib = _lib.load()
    x, y, thr, ref = _case(H, W, M, T, win, kind)
    C, rows, nw = 3, 2 * M, len(win)
    thr_d = torch.from_numpy(thr.copy()).cuda()
    need = lib.acg_reliability_workspace_bytes(rows, M, C, H, W, T, nw)
    assert need % 16 == 0 and need > 0
    for seed in (0, 1):
        xd = _device(x, "nhwc", C, 4, seed=seed, nan=0.3 * seed)
        yd = _device(y, "nhwc", C, 16, seed=10 + seed, nan=0.3 * seed)
        table, ws = Buf.out(GUARD + 2 * ref.size, np.uint32), Buf(GUARD + need // 4, dtype=np.uint32)
        rc = _abi_call(lib, xd, yd, rows, M, C, H, W, (H * W * 4, 4, 1), (H * W * 16, 16, 1), thr_d, T, win, table.at(GUARD), ws.at(GUARD), need)
        assert rc == 0, lib.acg_last_error().decode()
        o = table.host()                                           # checks the words behind the buffer
        assert np.all(o[:GUARD] == 0xFFFFFFFF)                     # and these are the words in front of it
        assert np.array_equal(o[GUARD:].view(np.int64).reshape(ref.shape), ref), seed
        assert np.all(ws.host()[:GUARD] == 0xFFFFFFFF)
    Buf.check_all()


@pytest.mark.parametrize("H,W,M", ((33, 65, 3), (321, 321, 4)))
def test_repeatable_and_the_same_bits_replayed_from_a_graph(H, W, M):
    """33 x 65 with 3 members lies in LDS; 321 x 321, the native grid, with 4 members (five planes of 15 KiB) is read from the
    workspace"""
    from dtgan_amd import _lib, ops
    win = (1, 17) if H > 100 else (1, 3, 65)
    x, y, thr, ref = _case(H, W, M, 1, win, "shifted", C=1, groups=1)
    xd, yd = _device(x, "nhwc", 1, 4, seed=1), _device(y, "nchw", 1)
    thr_d = torch.from_numpy(thr.copy()).cuda()
    out = torch.full(ref.shape, -7, dtype=torch.int64, device="cuda")
    call = lambda: ops.reliability(xd, yd, 1, "nhwc", "nchw", thr_d, win, x_per_y=M, out=out)
    call()                                                         # the workspace exists before the capture
    resident = (M + 1) * H * ((W + 63) // 64) * 8 <= LDS_MAX
    assert resident == (H < 100) and _lib.query("acg_last_kernel").decode().endswith("fss_rel<%s>" % ("lds" if resident else "global"))
    first = out.cpu().numpy()
    assert np.array_equal(first, ref)
    out.fill_(-7)
    call()
    assert np.array_equal(out.cpu().numpy(), first)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            call()
    torch.cuda.current_stream().wait_stream(s)
    out.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), first)


@pytest.mark.parametrize("M", (1, 2, 3, 4, 7, 8, 16, 64))
def test_window_1_is_the_ensemble_triple_of_ops_fss(M):
    """every slice count: sum k^2 n_k, sum_k table[k][1] and sum_k k table[k][1] are acg_fss's (sum E^2, sum co^2, sum E co)"""
    from dtgan_amd import ops
    H, W = 20, 67
    x, y, thr, ref = _case(H, W, M, 1, (1, 5), "noise", C=1, groups=2)
    xd, yd = _device(x, "nhwc", 1, 4), _device(y, "nchw", 1)
    got = _rel(xd, yd, 1, "nhwc", "nchw", thr, (1, 5), M)
    assert np.array_equal(got, ref)
    _, ens = ops.fss(xd, yd, 1, "nhwc", "nchw", thr, (1,), x_per_y=M, ensemble=True)
    ens = ens.cpu().numpy()[..., 0, :]
    t1, k = got[..., 0, :, :], np.arange(M + 1)
    assert np.array_equal((k * k * t1.sum(-1)).sum(-1), ens[..., 0])
    assert np.array_equal(t1[..., 1].sum(-1), ens[..., 1]) and np.array_equal((k * t1[..., 1]).sum(-1), ens[..., 2])
    assert 0 < ens[..., 1].min() and (M == 1 or got[..., 0, 1:M, :].sum() > 0)                         # the threshold cuts through
    # a table per member (x_per_y = 1, a truth row each) adds up to the ensemble's margins
    per = _rel(xd, yd.repeat_interleave(M, 0), 1, "nhwc", "nchw", thr, (1, 5), 1)
    assert np.array_equal(per.reshape((2, M) + per.shape[1:])[..., 1, :].sum(1), (k[:, None] * got).sum(-2))


def test_all_event_and_no_event_fields():
    H, W, M = 6, 130, 3
    x = np.full((M, 1, H, W), -3.0, np.float32)
    y = np.full((1, 1, H, W), 3.0, np.float32)
    x[1] = np.inf
    x[2, 0, 0, 129] = 0.0                                          # on the threshold: an event, in the last valid bit of a row
    thr, win = np.zeros((1, 1), np.float32), (1, 3, 65)
    got = _rel(_device(x, "nchw", 1), _device(y, "nchw", 1), 1, "nchw", "nchw", thr, win, M)
    assert np.array_equal(got, R.tables(x, y, thr, win, M))
    assert got[0, 0, 0, 0].tolist() == [[0, 0], [0, H * W - 1], [0, 1], [0, 0]]
    assert got[0, 0, 0, 1].tolist() == [[0, 0], [0, H * W - 4], [0, 4], [0, 0]]
    none = _rel(_device(x[:1], "nchw", 1), _device(-y, "nchw", 1), 1, "nchw", "nchw", thr, win, 1)
    assert np.all(none[..., 0, 0] == H * W) and none.sum() == 3 * H * W


def test_kernel_refuses_bad_arguments_in_the_documented_order():
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    x = torch.zeros(1 << 16, device="cuda")
    thr_d = torch.zeros(8, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    table = torch.full((4096,), -7, dtype=torch.int64, device="cuda")
    big, P = ws.numel(), (4096, 1, 4096)
    need = lib.acg_reliability_workspace_bytes(2, 1, 1, 64, 64, 1, 1)
    assert need == 2 * 2 * 64 * 12
    # everything wrong at once; mending the first refusal shows the next: (what to mend, the word of the refusal it mends)
    args = dict(xd=None, yd=None, rows=0, per=0, C=0, H=0, W=1025, sx=(0, 1, 4096), sy=(4096, 1, -1), thr_d=None, T=9, win=(1, 2), nw=0,
                table=None, ws=ctypes.c_void_p(ws.data_ptr() + 8), nbytes=0)
    steps = ((dict(rows=2), "rows >= 1"), (dict(C=1), "C >= 1"), (dict(sx=P), "strides"), (dict(sy=P), "strides"), (dict(per=3), "x_per_y"),
             (dict(per=65, rows=130), "x_per_y"), (dict(per=1, rows=2), "x_per_y"), (dict(xd=x), "null"), (dict(yd=x), "null"), (dict(thr_d=thr_d), "null"),
             (dict(nw=2), "null"), (dict(table=ops._ptr(table)), "null"), (dict(H=64), "H x W"), (dict(W=64), "H x W"),
             (dict(T=0), "thresholds"), (dict(T=1, win=(1, 2, 3, 5, 7, 9, 11, 13, 15), nw=9), "thresholds"), (dict(nw=2), "windows (nw="),
             (dict(win=(1, 67)), "odd"), (dict(win=(-1, 3)), "odd"), (dict(win=(0, 3)), "odd"), (dict(win=(1, 65)), "odd"),
             (dict(nbytes=need - 1), "workspace too small"), (dict(nbytes=need), "workspace too small"), (dict(ws=ctypes.c_void_p(ws.data_ptr())), "aligned"))

    def call():
        a = dict(args)
        win = a["win"][:a["nw"]] if a["nw"] <= len(a["win"]) else a["win"]
        warr = None if a["nw"] == 0 else (ctypes.c_int * len(win))(*win)
        return lib.acg_reliability(None if a["xd"] is None else ops._ptr(a["xd"]), None if a["yd"] is None else ops._ptr(a["yd"]),
                                   a["rows"], a["per"], a["C"], a["H"], a["W"], a["sx"][0], a["sx"][1], a["sx"][2], a["sy"][0], a["sy"][1],
                                   a["sy"][2], None if a["thr_d"] is None else ops._ptr(a["thr_d"]), a["T"], warr, a["nw"], a["table"],
                                   a["ws"], a["nbytes"], ops._stream())
    for mend, word in steps:
        rc = call()
        msg = lib.acg_last_error().decode()
        assert rc == (-2 if word == "workspace too small" else -1) and msg.startswith("acg_reliability") and word in msg, (mend, word, rc, msg)
        args.update(mend)
    torch.cuda.synchronize()
    assert torch.all(table == -7)                                  # nothing was written by any of them
    assert call() == 0, lib.acg_last_error().decode()              # and the mended call passes
    torch.cuda.synchronize()
    nt = 2 * 1 * 1 * 2 * 2 * 2
    assert table[:nt].view(2, 2, 2, 2).sum((-2, -1)).tolist() == [[4096, 4096]] * 2 and torch.all(table[nt:] == -7)
    args.update(ws=None, nbytes=0)
    assert call() == -2                                            # a missing workspace
    with pytest.raises(_lib.AcgError, match="reliability: .*windows"):
        ops.reliability(x[:128].view(2, 1, 8, 8), x[:128].view(2, 1, 8, 8), 1, "nchw", "nchw", np.zeros((1, 1), np.float32), (67,))
