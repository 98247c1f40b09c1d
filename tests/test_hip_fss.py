"""GPU tests of the fractions skill score: acg_fss against tests/fss_ref.py for equality (the kernel is integer: no
tolerance anywhere), model.translate_fss against generate_multi / translate_ensemble and the reference, and
`python -m dtgan_amd.test --metric fss` in a child process."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import fss_ref as F
from eval_cases import checkpoint_model, S as EVAL_S, count_sync_warnings as _count_sync_warnings, experiment, run_test  # noqa: F401  (the fixture)
from field_cases import field_operand as _device
from guard_util import GUARD, Buf
from model_cases import ensemble_inputs as _inputs, ensemble_model as _model

pytestmark = pytest.mark.gpu

# x in every layout crossed with a planar and an NHWC truth: (layout x, stored channels x, layout y, stored channels y)
LAYOUTS = [(lx, cpx, ly, cpy) for lx, cpx in (("nchw", 0), ("nhwc", 4), ("nhwc", 16)) for ly, cpy in (("nchw", 0), ("nhwc", 4))]


@functools.lru_cache(maxsize=None)
def _case(kind, H, W):
    """the pair (2, 3, H, W) each, its thresholds (3, 3), windows and reference triples (2, 3, 3, nw, 3)"""
    x, y, thr = F.make_pair(kind, H, W)
    win = F.case_windows(H, W)
    ref = F.triples(x, y, thr, win)
    ref.setflags(write=False)
    return x, y, thr, win, ref


def _fss(xd, yd, C, lx, ly, thr, win, x_per_y=1, ensemble=False):
    """ops.fss into poisoned outputs -> host int64 (rows, C, T, nw, 3) [, (rows / x_per_y, C, T, nw, 3)]"""
    from dtgan_amd import ops
    rows = xd.shape[0]
    shape = (C, thr.shape[1], len(win), 3)
    out = torch.full((rows,) + shape, -7, dtype=torch.int64, device="cuda")
    if not ensemble:
        assert ops.fss(xd, yd, C, lx, ly, thr[:C], win, x_per_y=x_per_y, out=out) is out
        return out.cpu().numpy()
    ens = torch.full((rows // x_per_y,) + shape, -7, dtype=torch.int64, device="cuda")
    got = ops.fss(xd, yd, C, lx, ly, thr[:C], win, x_per_y=x_per_y, ensemble=True, out=(out, ens))
    assert got[0] is out and got[1] is ens
    return out.cpu().numpy(), ens.cpu().numpy()


@pytest.mark.parametrize("kind", F.KINDS)
@pytest.mark.parametrize("H,W", F.SIZES)
def test_kernel_equals_the_reference(H, W, kind):
    x, y, thr, win, ref = _case(kind, H, W)
    for C in (3, 1):
        for lx, cpx, ly, cpy in (LAYOUTS if C == 3 else LAYOUTS[2:4]):
            got = _fss(_device(x, lx, C, cpx, seed=1), _device(y, ly, C, cpy, seed=2), C, lx, ly, thr, win)
            assert got.dtype == np.int64 and got.shape == (2, C, 3, len(win), 3)
            assert np.array_equal(got, ref[:, :C]), (kind, H, W, C, lx, cpx, ly, cpy, np.argwhere(got != ref[:, :C])[:5])
    if kind == "noise":                                            # the thresholds nothing and everything exceeds
        assert np.all(ref[:, :, 1] == 0) and np.all(ref[:, :, 2, 0] == H * W)
        assert np.all(ref[:, :, 2, -1] == (H * W) ** 3)            # the whole domain from every cell: c = H W everywhere


def test_one_large_field_puts_the_high_word_under_test():
    """1024 x 1024: an all-ones row, whose whole-domain sums are exactly 2^60, and a noise row"""
    from dtgan_amd import _lib
    rs = np.random.RandomState(5)
    x = np.ones((2, 1, 1024, 1024), dtype=np.float32)
    y = np.ones((2, 1, 1024, 1024), dtype=np.float32)
    x[1, 0], y[1, 0] = rs.standard_normal((2, 1024, 1024)).astype(np.float32)
    thr, win = np.array([[0.5]], dtype=np.float32), (1, 33, 2047)
    got = _fss(_device(x, "nchw", 1), _device(y, "nhwc", 1, 4, seed=3), 1, "nchw", "nhwc", thr, win)
    assert _lib.query("acg_last_kernel").decode() == "fss_events<strided> + fss_box<global>"
    assert np.all(got[0, 0, 0, 2] == 1 << 60) and np.all(got[0, 0, 0, 0] == 1 << 20)
    assert np.array_equal(got, F.triples(x, y, thr, win))


def test_members_share_a_truth_through_x_per_y():
    """6 members against 2 truth rows at x_per_y = 3: the call with every truth row repeated, and the ensemble triples"""
    H, W, M = 33, 31, 3
    x, _, thr = F.make_pair("noise", H, W, rows=6, seed=1)
    y = F.make_pair("noise", H, W, rows=2, seed=2)[1]
    win = F.case_windows(H, W)
    xd, yd = _device(x, "nhwc", 3, 4), _device(y, "nchw", 3)
    shared, ens = _fss(xd, yd, 3, "nhwc", "nchw", thr, win, x_per_y=M, ensemble=True)
    repeated = _fss(xd, yd.repeat_interleave(M, 0), 3, "nhwc", "nchw", thr, win)
    assert np.array_equal(shared, repeated) and np.array_equal(shared, F.triples(x, y, thr, win, x_per_y=M))
    assert not np.array_equal(shared[2], shared[3])                # member 3 is the first of the second truth
    assert np.array_equal(ens, F.ens_triples(x, y, thr, win, M))
    # E = sum_m cf_m: the same numbers from the members' count planes, summed before they are squared
    bx, by = F.events(x, thr), F.events(y, thr)
    for k, n in enumerate(win):
        E = F.box_counts(bx, n).reshape((2, M) + bx.shape[1:]).sum(1)
        assert np.array_equal(ens[..., k, :], F.triples_of_counts(E, F.box_counts(by, n))), n
    only = _fss(xd, yd, 3, "nhwc", "nchw", thr, win, x_per_y=M)    # without the ensemble output: the same members
    assert np.array_equal(only, shared)


def test_the_ensemble_output_of_single_members_equals_out():
    x, y, thr, win, ref = _case("noise", 33, 31)
    out, ens = _fss(_device(x, "nchw", 3), _device(y, "nchw", 3), 3, "nchw", "nchw", thr, win, ensemble=True)
    assert np.array_equal(out, ref) and np.array_equal(ens, out)


@pytest.mark.parametrize("H,W", ((16, 16), (65, 130), (256, 256)))
def test_repeatable_and_the_same_bits_in_every_layout(H, W):
    x, y, thr, win, _ = _case("shifted", H, W)
    first = _fss(_device(x, "nchw", 3), _device(y, "nchw", 3), 3, "nchw", "nchw", thr, win)
    for lx, cpx in (("nchw", 0), ("nhwc", 4), ("nhwc", 16)):
        for ly, cpy in (("nchw", 0), ("nhwc", 4), ("nhwc", 16)):
            xd, yd = _device(x, lx, 3, cpx, seed=1), _device(y, ly, 3, cpy, seed=2)
            a, b = _fss(xd, yd, 3, lx, ly, thr, win), _fss(xd, yd, 3, lx, ly, thr, win)
            assert np.array_equal(a, b) and np.array_equal(a, first), (lx, cpx, ly, cpy)


def _abi_call(lib, xd, yd, rows, per, C, H, W, sx, sy, thr_d, T, win, out, ens, ws, nbytes):
    from dtgan_amd import ops
    warr = (ctypes.c_int * len(win))(*win)
    return lib.acg_fss(ops._ptr(xd), ops._ptr(yd), rows, per, C, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], ops._ptr(thr_d), T,
                       warr, len(win), out, ens, ws, nbytes, ops._stream())


@pytest.mark.parametrize("H,W", ((5, 7), (65, 130), (256, 256)))
def test_guard_words_and_padded_channels(H, W):
    """through the C ABI: both outputs start poisoned and lie, like the workspace, between guard words; +-50 and NaN garbage
    in the padded channels of either operand changes nothing"""
    from dtgan_amd import _lib
    lib = _lib.load()
    M, C, T = 2, 3, 3
    x, _, thr = F.make_pair("noise", H, W, rows=4, seed=3)
    y = F.make_pair("nan", H, W, rows=2, seed=4)[1]
    win = F.case_windows(H, W)
    nw = len(win)
    want, want_ens = F.triples(x, y, thr, win, x_per_y=M), F.ens_triples(x, y, thr, win, M)
    thr_d = torch.from_numpy(thr).cuda()
    need = lib.acg_fss_workspace_bytes(4, M, C, H, W, T, nw, 1)
    assert need % 16 == 0 and need > 0
    for seed in (0, 1):
        xd, yd = _device(x, "nhwc", C, 4, seed=seed, nan=0.3 * (seed == 1)), _device(y, "nhwc", C, 16, seed=10 + seed, nan=0.3 * (seed == 1))
        n_out, n_ens = 4 * C * T * nw * 3, 2 * C * T * nw * 3
        out, ens = Buf.out(GUARD + 2 * n_out, np.uint32), Buf.out(GUARD + 2 * n_ens, np.uint32)
        ws = Buf(GUARD + need // 4, dtype=np.uint32)
        rc = _abi_call(lib, xd, yd, 4, M, C, H, W, (H * W * 4, 4, 1), (H * W * 16, 16, 1), thr_d, T, win, out.at(GUARD), ens.at(GUARD),
                       ws.at(GUARD), need)
        assert rc == 0, lib.acg_last_error().decode()
        for buf, n, ref in ((out, n_out, want), (ens, n_ens, want_ens)):
            o = buf.host()                                         # checks the words behind the buffer
            assert np.all(o[:GUARD] == 0xFFFFFFFF)                 # and these are the words in front of it
            assert np.array_equal(o[GUARD:].view(np.int64).reshape(ref.shape), ref), seed
        assert np.all(ws.host()[:GUARD] == 0xFFFFFFFF)
    Buf.check_all()


def _plane_bytes(H, W):
    WW = (W + 63) // 64
    return H * WW * 8 + H * (WW + 1) * 2


LDS_MAX = 64 * 1024 - 512


@pytest.mark.parametrize("H,W", F.SIZES + ((512, 512), (1024, 1024)))
def test_the_path_a_size_takes(H, W):
    """a workgroup's planes (words and row prefixes, (8 WW + 2 (WW + 1)) H bytes each, WW = ceil(W / 64)) go into
    LDS while they fit 64 KiB - 512, through the workspace above: two planes for the members, bit_width(M) + 1 for the
    ensemble; the workspace holds the planes of x, of y and, for an ensemble of M > 1, bit_width(M) slices per truth plane"""
    from dtgan_amd import _lib
    P = _plane_bytes(H, W)
    x = np.zeros((2, 1, H, W), dtype=np.float32)
    thr, win = np.zeros((1, 1), dtype=np.float32), (1, 3)
    path = lambda n: "lds" if n * P <= LDS_MAX else "global"
    _fss(_device(x, "nhwc", 1, 4), _device(x[:1], "nchw", 1), 1, "nhwc", "nchw", thr, win, x_per_y=2, ensemble=True)
    k = _lib.query("acg_last_kernel").decode()
    assert k == "fss_events<c4> + fss_box<%s> + fss_slices + fss_ens<%s>" % (path(2), path(3)), k
    assert (path(2) == "lds") == ((H, W) not in ((512, 512), (1024, 1024)))
    _fss(_device(x, "nchw", 1), _device(x, "nhwc", 1, 16), 1, "nchw", "nhwc", thr, win, ensemble=True)
    k = _lib.query("acg_last_kernel").decode()
    assert k == "fss_events<strided> + fss_box<%s> + fss_ens<%s>" % (path(2), path(2)), k      # M = 1: no slices
    _fss(_device(x, "nchw", 1), _device(x, "nchw", 1), 1, "nchw", "nchw", thr, win)
    assert _lib.query("acg_last_kernel").decode() == "fss_events<strided> + fss_box<%s>" % path(2)
    up = lambda n: (n + 15) // 16 * 16
    WW = (W + 63) // 64
    planes = lambda n: up(n * H * WW * 8) + up(n * H * (WW + 1) * 2)
    need = _lib.query("acg_fss_workspace_bytes", 4, 2, 3, H, W, 3, 6, 1)
    assert need == planes(36) + planes(18) + planes(18 * 2), need
    assert _lib.query("acg_fss_workspace_bytes", 4, 2, 3, H, W, 3, 1, 0) == planes(36) + planes(18)      # whatever the windows
    assert _lib.query("acg_fss_workspace_bytes", 16, 16, 1, H, W, 1, 1, 1) == planes(16) + planes(1) + planes(5)
    assert _lib.query("acg_fss_workspace_bytes", 4, 1, 1, H, W, 1, 1, 1) == 2 * planes(4)             # M = 1: no slices


@pytest.mark.parametrize("H,W,M", ((256, 256, 16), (321, 321, 16), (33, 31, 64)))
def test_an_ensemble_of_many_members(H, W, M):
    """16 members at 256^2 are the evaluator's case: five slices and the truth, 63 KiB, still in LDS; 321^2 is not; 64 members
    need seven slices"""
    from dtgan_amd import _lib
    rs = np.random.RandomState(M)
    x = rs.standard_normal((M, 1, H, W)).astype(np.float32)
    x[0] = 3.0                                                     # and with the threshold everything exceeds every count is M
    y = rs.standard_normal((1, 1, H, W)).astype(np.float32)
    thr, win = np.array([[0.3, -1e30]], dtype=np.float32), (1, 5, 33)
    out, ens = _fss(_device(x, "nhwc", 1, 4), _device(y, "nchw", 1), 1, "nhwc", "nchw", thr, win, x_per_y=M, ensemble=True)
    k = _lib.query("acg_last_kernel").decode()
    ns = M.bit_length()
    assert k.endswith("fss_slices + fss_ens<%s>" % ("lds" if (ns + 1) * _plane_bytes(H, W) <= LDS_MAX else "global")), k
    assert ("ens<lds>" in k) == ((H, W) != (321, 321))
    assert np.array_equal(out, F.triples(x, y, thr, win, x_per_y=M)) and np.array_equal(ens, F.ens_triples(x, y, thr, win, M))


def test_kernel_refuses_bad_arguments_before_launching():
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    x = torch.zeros(4 << 20, device="cuda")
    thr_d = torch.zeros(8, device="cuda")
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    big = ws.numel()
    need = lib.acg_fss_workspace_bytes(2, 1, 1, 64, 64, 1, 1, 0)
    assert need == 2 * 2 * 64 * 12
    assert lib.acg_fss_workspace_bytes(1, 16, 1, 1024, 1024, 1, 1, 1) == 0 and lib.acg_fss_workspace_bytes(16, 16, 1, 1024, 1024, 1, 1, 1) <= big
    # rows, x_per_y, C, H, W, (x strides), (y strides), T, windows, out?, ens?, workspace offset, bytes, status, a word of the message
    P = (4096, 1, 4096)
    bad = [(2, 1, 1, 64, 64, None, None, 1, (2,), 1, 0, 0, big, -1, "odd"), (2, 1, 1, 64, 64, None, None, 1, (1, 0), 1, 0, 0, big, -1, "odd"),
           (2, 1, 1, 64, 64, None, None, 1, (3, -5), 1, 0, 0, big, -1, "odd"), (6, 4, 1, 64, 64, None, None, 1, (1,), 1, 0, 0, big, -1, "x_per_y"),
           (6, 0, 1, 64, 64, None, None, 1, (1,), 1, 0, 0, big, -1, "x_per_y"), (130, 65, 1, 8, 8, None, None, 1, (1,), 1, 0, 0, big, -1, "x_per_y"),
           (2, 1, 1, 64, 64, (4096, 0, 4096), None, 1, (1,), 1, 0, 0, big, -1, "strides"),
           (2, 1, 1, 64, 64, None, (0, 1, 4096), 1, (1,), 1, 0, 0, big, -1, "strides"),
           (2, 1, 1, 64, 64, None, (4096, 1, -1), 1, (1,), 1, 0, 0, big, -1, "strides"),
           (2, 1, 1, 64, 64, None, None, 1, (1,), 0, 0, 0, big, -1, "both NULL"), (2, 1, 1, 0, 64, None, None, 1, (1,), 1, 0, 0, big, -1, "H x W"),
           (2, 1, 1, 64, 1025, None, None, 1, (1,), 1, 0, 0, big, -1, "H x W"), (2, 1, 1, 64, 64, None, None, 9, (1,), 1, 0, 0, big, -1, "thresholds"),
           (2, 1, 1, 64, 64, None, None, 0, (1,), 1, 0, 0, big, -1, "thresholds"), (2, 1, 0, 64, 64, None, None, 1, (1,), 1, 0, 0, big, -1, "C >= 1"),
           (0, 1, 1, 64, 64, None, None, 1, (1,), 1, 0, 0, big, -1, "rows >= 1"),
           (2, 1, 1, 64, 64, None, None, 1, (1,), 1, 0, 0, need - 1, -2, "workspace too small"),
           (2, 1, 1, 64, 64, None, None, 1, (1,), 1, 0, 8, need, -1, "aligned"),
           # 1024^2 with the whole-domain window: 2^60 for single members (accepted below), 2^68 for 16 members' summed counts
           (16, 16, 1, 1024, 1024, None, None, 1, (1, 2047), 1, 1, 0, big, -1, "overflow"),
           (16, 16, 1, 1024, 1024, None, None, 1, (1, 1449), 0, 1, 0, big, -1, "overflow")]
    for rows, per, C, H, W, sx, sy, T, win, has_out, has_ens, off, nbytes, rc_want, word in bad:
        sx, sy = sx or (H * W, 1, H * W), sy or (H * W, 1, H * W)
        out = torch.full((4096,), -7, dtype=torch.int64, device="cuda")
        ens = torch.full((4096,), -7, dtype=torch.int64, device="cuda")
        rc = _abi_call(lib, x, x, rows, per, C, H, W, sx, sy, thr_d, T, win, ops._ptr(out) if has_out else None,
                       ops._ptr(ens) if has_ens else None, ctypes.c_void_p(ws.data_ptr() + off), nbytes)
        msg = lib.acg_last_error().decode()
        assert rc == rc_want and msg.startswith("acg_fss") and word in msg, (rows, per, C, H, W, win, rc, msg)
        torch.cuda.synchronize()
        assert torch.all(out == -7) and torch.all(ens == -7)       # nothing was written
    nine = tuple(range(1, 19, 2))
    rc = _abi_call(lib, x, x, 2, 1, 1, 64, 64, P, P, thr_d, 1, nine, ops._ptr(out), None, ctypes.c_void_p(ws.data_ptr()), big)
    assert rc == -1 and "windows" in lib.acg_last_error().decode()
    rc = _abi_call(lib, x, x, 2, 1, 1, 64, 64, P, P, thr_d, 1, (1,), ops._ptr(out), None, None, 0)
    assert rc == -2 and torch.all(out == -7)                       # a missing workspace
    # the reach of the overflow rule: the members' own triples at 1024^2 are accepted next to the refused ensemble's
    rc = _abi_call(lib, x, x, 1, 1, 1, 1024, 1024, (1 << 20, 1, 1 << 20), (1 << 20, 1, 1 << 20), thr_d, 1, (2047,), ops._ptr(out), None,
                   ctypes.c_void_p(ws.data_ptr()), big)
    assert rc == 0, lib.acg_last_error().decode()
    torch.cuda.synchronize()
    assert out[:3].tolist() == [1 << 60] * 3 and torch.all(out[3:] == -7)            # zeros >= 0: every cell an event
    with pytest.raises(_lib.AcgError, match="overflow"):             # through ops: (4 * 2^20)^2 * 2^20 = 2^64
        ops.fss(x.view(4, 1, 1024, 1024), x[:1 << 20].view(1, 1, 1024, 1024), 1, "nchw", "nchw", np.zeros((1, 1), np.float32), (2047,),
                x_per_y=4, ensemble=True)
    torch.cuda.synchronize()


THR, WIN = F.THR, F.WIN


@pytest.mark.parametrize("S", (64, 48))
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_translate_fss_equals_generate_multi_and_the_reference(prec, S):
    from hip_util import precision
    from dtgan_amd import ops
    N, M = 3, 5
    with precision(prec):
        m = _model()
        A, B, g = _inputs(N, S)
        z = torch.randn(N * M, m.opt.nlatent, 1, 1, device="cuda", generator=g)
        r = m.translate_fss(A, M, B, THR, WIN, z=z)
        assert set(r) == {"members", "ens_prob", "ens_mean"}
        assert r["members"].shape == (N, M, 3, 3, 4, 3) and r["ens_prob"].shape == r["ens_mean"].shape == (N, 3, 3, 4, 3)
        assert all(v.dtype == torch.int64 and not v.requires_grad for v in r.values())
        with torch.no_grad():
            members = m.generate_multi(A, z)
        direct, direct_ens = ops.fss(members, B, 3, "nchw", "nchw", THR, WIN, x_per_y=M, ensemble=True)
        assert torch.equal(r["members"].reshape(N * M, 3, 3, 4, 3), direct) and torch.equal(r["ens_prob"], direct_ens)
        mean = m.translate_ensemble(A, M, z=z, real_B=B)["mean"]
        assert torch.equal(r["ens_mean"], ops.fss(mean, B, 3, "nchw", "nchw", THR, WIN))
        Bh, mh, meanh = B.cpu().numpy(), members.cpu().numpy(), mean.cpu().numpy()
        assert np.array_equal(direct.cpu().numpy(), F.triples(mh, Bh, THR, WIN, x_per_y=M))
        assert np.array_equal(direct_ens.cpu().numpy(), F.ens_triples(mh, Bh, THR, WIN, M))
        assert np.array_equal(r["ens_mean"].cpu().numpy(), F.triples(meanh, Bh, THR, WIN))
        assert 0 < direct[..., 0, 0].sum() < direct[..., 0, 0].numel() * S * S      # the thresholds cut through the members
        one = m.translate_fss(A, M, B, torch.from_numpy(THR).cuda(), WIN, z=z, chunk=M)   # one input per group
        for k in r:
            assert torch.equal(r[k], one[k]), k


def test_translate_fss_refusals():
    m = _model()
    A, B, _ = _inputs(2, 64)
    with pytest.raises(ValueError, match="n_samples"):
        m.translate_fss(A, 65, B, THR, WIN)
    with pytest.raises(ValueError, match="codes"):
        m.translate_fss(A, 2, B, THR, WIN, z=torch.zeros(3, m.opt.nlatent, 1, 1, device="cuda"))
    with pytest.raises(ValueError, match="cannot hold"):
        m.translate_fss(A, 4, B, THR, WIN, chunk=3)
    with pytest.raises(ValueError, match="does not pair"):
        m.translate_fss(A, 2, B[:1], THR, WIN)
    with pytest.raises(ValueError, match="odd"):
        m.translate_fss(A, 2, B, THR, (1, 4))
    with pytest.raises(ValueError, match="thresholds"):
        m.translate_fss(A, 2, B, THR[:2], WIN)


def test_translate_fss_host_syncs_do_not_grow_with_groups():
    m = _model()
    A, B, _ = _inputs(4, 64, seed=7)
    M = 3
    thr = torch.from_numpy(THR).cuda()
    m.translate_fss(A, M, B, thr, WIN)                             # warm-up
    n1 = _count_sync_warnings(lambda: m.translate_fss(A, M, B, thr, WIN))
    n4 = _count_sync_warnings(lambda: m.translate_fss(A, M, B, thr, WIN, chunk=M))
    assert n1 == n4 and n1 <= 1, (n1, n4)


def test_metric_fss(experiment):
    S = EVAL_S
    from dtgan_amd import eval_metrics as EM
    from dtgan_amd.dataloader import load_numpy_data
    num = r"(\d+\.\d{4}|nan)"
    pat = (r"^DEV_FSS_B: %s, TEST_FSS_B: %s, TEST_FSS_PROB_B: %s, TEST_FSS_MEAN_B: %s, TEST_FSS_A: %s, TEST_USEFUL_SCALE_B: %s$"
           % ((num,) * 6))
    runs = []
    for res_dir in ("res_fss", "res_fss_again"):
        out = run_test(experiment, "fss", "--n_samples", "4", "--fss_windows", "3,9,17", "--res_dir", res_dir)
        mt = re.search(pat, out, re.M)
        assert mt, out[-2000:]
        runs.append((mt.groups(), dict(np.load(os.path.join(experiment["expr"], res_dir, "fss.npz")))))
    (line, arr), (line2, arr2) = runs
    assert line == line2 and set(arr) == set(arr2)
    for k in arr:                                                  # two runs, the same file
        assert arr[k].dtype == arr2[k].dtype and np.array_equal(arr[k], arr2[k], equal_nan=True), k
    win, M, C, Tn = (1, 3, 9, 17), 4, 3, 3
    want = {"n_samples", "windows", "thresholds_B", "thresholds_A"}
    want |= {"%s_%s_%s" % (split, q, k) for split in ("dev", "test") for k in EM.FSS_PAIRS
             for q in ("sums", "fss", "bias", "csi", "base_rate", "useful_scale")}
    assert set(arr) == want, set(arr) ^ want
    assert int(arr["n_samples"]) == M and arr["windows"].dtype == np.int64 and tuple(arr["windows"]) == win     # 1 put in front
    trainA, trainB, devA, devB, testA, testB = load_numpy_data(experiment["data"], grid_size=S)
    for name, train in (("thresholds_B", trainB), ("thresholds_A", trainA)):
        q = np.quantile(np.asarray(train).astype(np.float64).transpose(1, 0, 2, 3).reshape(C, -1), [0.5, 0.9, 0.99], axis=1).T
        assert arr[name].dtype == np.float32 and arr[name].shape == (C, Tn) and np.array_equal(arr[name], q.astype(np.float32)), name
    for split, A, B in (("dev", np.asarray(devA), np.asarray(devB)), ("test", np.asarray(testA), np.asarray(testB))):
        for k in EM.FSS_PAIRS:
            g = lambda q: arr["%s_%s_%s" % (split, q, k)]
            sums = g("sums")
            assert sums.shape == (C, Tn, 4, 3) and sums.dtype == np.int64 and np.all(sums >= 0), (split, k)
            assert g("fss").shape == (C, Tn, 4) and g("fss").dtype == np.float64, (split, k)
            for q in ("bias", "csi", "base_rate", "useful_scale"):
                assert g(q).shape == (C, Tn) and g(q).dtype == (np.int64 if q == "useful_scale" else np.float64), (split, k, q)
            members = M if k == "ens_prob_B" else 1
            truth, thr = (A, arr["thresholds_A"]) if k == "fake_A" else (B, arr["thresholds_B"])
            pairs = len(truth) * (M if k == "members_B" else 1)
            ref = F.summary(sums, win, pairs * S * S, members)
            for q in ref:
                assert np.allclose(g(q), ref[q], rtol=1e-12, equal_nan=True), (split, k, q)
            assert np.all(np.isin(g("useful_scale"), (0,) + win))
            # the observed side of the triple is the reference on the paired real field, once per pair; exactly
            oo = F.triples(truth, truth, thr, win).sum(0)[..., 1]
            assert np.array_equal(sums[..., 1], oo * (pairs // len(truth))), (split, k)
    t, w = 2, 2                                                    # the highest threshold, the median listed window (9)
    for i, key in ((0, "dev_fss_members_B"), (1, "test_fss_members_B"), (2, "test_fss_ens_prob_B"), (3, "test_fss_ens_mean_B"),
                   (4, "test_fss_fake_A")):
        v = arr[key][:, t, w]
        assert (line[i] == "nan" and np.all(np.isnan(v))) or abs(float(line[i]) - np.nanmean(v)) < 1e-4, (key, line[i], v)
    assert abs(float(line[5]) - arr["test_useful_scale_members_B"][:, t].mean()) < 1e-4
    # B -> A in process: the reference on predict_A's fields gives the file's sums, exactly
    with checkpoint_model(experiment) as model:
        with torch.no_grad():
            fake_A = model.predict_A(torch.as_tensor(np.asarray(testB)).cuda()).cpu().numpy()
    assert np.array_equal(arr["test_sums_fake_A"], F.triples(fake_A, np.asarray(testA), arr["thresholds_A"], win).sum(0))

