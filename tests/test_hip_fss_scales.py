"""GPU tests of the intensity-scale triples: acg_fss_scales against tests/fss_scales_ref.py for equality (the kernel is
integer: no tolerance anywhere), against ops.fss at level 0, model.translate_fss(scales=True) against generate_multi and the
reference, and `python -m dtgan_amd.test --metric fss --fss_scales 1` in a child process."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import fss_ref as F
import fss_scales_ref as R
from eval_cases import checkpoint_model, S as EVAL_S, count_sync_warnings as _count_sync_warnings, experiment, run_test  # noqa: F401  (the fixture)
from field_cases import PAIR_LAYOUTS as LAYOUTS, field_operand as _device, shifted as _shifted
from fss_ref import THR, WIN
from guard_util import GUARD, Buf
from model_cases import ensemble_inputs as _inputs, ensemble_model as _model

pytestmark = pytest.mark.gpu

@functools.lru_cache(maxsize=None)
def _case(kind, H, W):
    """the pair (2, 3, H, W) each, its thresholds (3, 3) and the reference triples (2, 3, 3, nl, 3)"""
    x, y, thr = F.make_pair(kind, H, W)
    ref = R.triples(x, y, thr)
    ref.setflags(write=False)
    return x, y, thr, ref


def _scales(xd, yd, C, lx, ly, thr, x_per_y=1, ensemble=False):
    """ops.fss_scales into poisoned outputs -> host int64 (rows, C, T, nl, 3) [, (rows / x_per_y, C, T, nl, 3)]"""
    from dtgan_amd import ops
    rows = xd.shape[0]
    H, W = (xd.shape[2], xd.shape[3]) if lx == "nchw" else (xd.shape[1], xd.shape[2])
    shape = (C, thr.shape[1], ops.fss_scale_levels(H, W), 3)
    out = torch.full((rows,) + shape, -7, dtype=torch.int64, device="cuda")
    if not ensemble:
        assert ops.fss_scales(xd, yd, C, lx, ly, thr[:C], x_per_y=x_per_y, out=out) is out
        return out.cpu().numpy()
    ens = torch.full((rows // x_per_y,) + shape, -7, dtype=torch.int64, device="cuda")
    got = ops.fss_scales(xd, yd, C, lx, ly, thr[:C], x_per_y=x_per_y, ensemble=True, out=(out, ens))
    assert got[0] is out and got[1] is ens
    return out.cpu().numpy(), ens.cpu().numpy()


@pytest.mark.parametrize("kind", F.KINDS)
@pytest.mark.parametrize("H,W", R.SIZES)
def test_kernel_equals_the_reference(H, W, kind):
    from dtgan_amd import _lib
    x, y, thr, ref = _case(kind, H, W)
    nl = R.levels(H, W)
    for C in (3, 1):
        for lx, cpx, off, ly, cpy in (LAYOUTS if C == 3 else LAYOUTS[1:2]):
            xd, yd = _shifted(_device(x, lx, C, cpx, seed=1), off), _device(y, ly, C, cpy, seed=2)
            got = _scales(xd, yd, C, lx, ly, thr)
            assert got.dtype == np.int64 and got.shape == (2, C, 3, nl, 3)
            assert np.array_equal(got, ref[:, :C]), (kind, H, W, C, lx, cpx, off, ly, cpy, np.argwhere(got != ref[:, :C])[:5])
            path = _lib.query("acg_last_kernel").decode()
            assert path == "fss_events<%s> + fss_scales" % ("c4" if (lx, cpx, off) == ("nhwc", 4, 0) else "strided"), path
    if kind == "noise":                                            # the thresholds nothing and everything exceeds
        assert np.all(ref[:, :, 1] == 0) and np.all(ref[:, :, 2, 0] == H * W) and np.all(ref[:, :, 2, -1] == (H * W) ** 2)


@pytest.mark.parametrize("H,W", ((1, 1024), (1024, 1024)))
def test_one_pair_at_the_largest_extent(H, W):
    """eleven levels, 16 (x 16) tiles per workgroup, levels 7 .. 10 from the tiles' totals"""
    rs = np.random.RandomState(H)
    x, y = rs.standard_normal((2, 1, 1, H, W)).astype(np.float32)
    thr = np.array([[0.5]], dtype=np.float32)
    got = _scales(_device(x, "nchw", 1), _device(y, "nhwc", 1, 4, seed=3), 1, "nchw", "nhwc", thr)
    assert got.shape == (1, 1, 1, 11, 3) and np.array_equal(got, R.triples(x, y, thr))


@pytest.mark.parametrize("H,W", ((5, 7), (65, 130), (256, 256)))
def test_level_zero_is_the_window_one_triple_of_ops_fss(H, W):
    from dtgan_amd import ops
    x, y, thr, ref = _case("nan", H, W)
    xd, yd = _device(x, "nhwc", 3, 4, seed=1), _device(y, "nchw", 3)
    box = ops.fss(xd, yd, 3, "nhwc", "nchw", thr, (1,))
    got = ops.fss_scales(xd, yd, 3, "nhwc", "nchw", thr)
    assert torch.equal(got[..., 0, :], box[..., 0, :]) and np.array_equal(got.cpu().numpy(), ref)


def test_the_ensemble_output_of_single_members_equals_out():
    x, y, thr, ref = _case("noise", 63, 65)
    out, ens = _scales(_device(x, "nchw", 3), _device(y, "nchw", 3), 3, "nchw", "nchw", thr, ensemble=True)
    assert np.array_equal(out, ref) and np.array_equal(ens, out)


@pytest.mark.parametrize("H,W,M", ((65, 130, 5), (33, 31, 64)))
def test_members_share_a_truth_and_sum_to_the_ensemble(H, W, M):
    from dtgan_amd import _lib
    x, _, thr = F.make_pair("noise", H, W, rows=2 * M, seed=1)
    y = F.make_pair("noise", H, W, rows=2, seed=2)[1]
    x[0] = 3.0                                                     # one member all events: the first truth's counts reach M
    xd, yd = _device(x, "nhwc", 3, 4), _device(y, "nchw", 3)
    out, ens = _scales(xd, yd, 3, "nhwc", "nchw", thr, x_per_y=M, ensemble=True)
    assert _lib.query("acg_last_kernel").decode() == "fss_events<c4> + fss_scales + fss_slices + fss_scales_ens"
    assert np.array_equal(out, R.triples(x, y, thr, x_per_y=M)) and np.array_equal(ens, R.ens_triples(x, y, thr, M))
    assert np.array_equal(_scales(xd, yd, 3, "nhwc", "nchw", thr, x_per_y=M), out)     # without the ensemble output
    assert ens[0, 0, 2, 0, 0] == M * M * H * W                     # the threshold everything exceeds: E = M in every cell


def test_sixty_four_members_of_all_events_reach_the_high_word():
    """M = 64 at 1024^2, every cell an event in every member: E = 64 * 4^l per block, so level l holds
    (2^(32 + 2l), 2^(20 + 2l), 2^(26 + 2l)) and level L = 10 reaches 2^52, the largest value there is"""
    from dtgan_amd import ops
    x = torch.ones((64, 1, 1024, 1024), device="cuda")
    y = torch.ones((1, 1, 1024, 1024), device="cuda")
    out, ens = ops.fss_scales(x, y, 1, "nchw", "nchw", np.array([[0.5]], dtype=np.float32), x_per_y=64, ensemble=True)
    lv = np.arange(11)
    assert np.array_equal(ens.cpu().numpy()[0, 0, 0], np.stack([2 ** (32 + 2 * lv), 2 ** (20 + 2 * lv), 2 ** (26 + 2 * lv)], -1))
    assert ens[0, 0, 0, 10, 0].item() == 1 << 52
    assert np.array_equal(out.cpu().numpy(), np.broadcast_to((2 ** (20 + 2 * lv))[:, None], (64, 1, 1, 11, 3)))


def _abi_call(lib, xd, yd, rows, per, C, H, W, sx, sy, thr_d, T, out, ens, ws, nbytes):
    from dtgan_amd import ops
    return lib.acg_fss_scales(ops._ptr(xd), ops._ptr(yd), rows, per, C, H, W, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], ops._ptr(thr_d),
                              T, out, ens, ws, nbytes, ops._stream())


@pytest.mark.parametrize("H,W", ((5, 7), (65, 130), (256, 256)))
def test_guard_words_and_padded_channels(H, W):
    """through the C ABI: both outputs start poisoned and lie between guard words; the workspace has exactly the queried
    size, starts as 0xFF bytes and lies between guard words too; +-50 and NaN garbage in the padded channels of either
    operand changes nothing"""
    from dtgan_amd import _lib
    lib = _lib.load()
    M, C, T = 2, 3, 3
    x, _, thr = F.make_pair("noise", H, W, rows=4, seed=3)
    y = F.make_pair("nan", H, W, rows=2, seed=4)[1]
    nl = R.levels(H, W)
    want, want_ens = R.triples(x, y, thr, x_per_y=M), R.ens_triples(x, y, thr, M)
    thr_d = torch.from_numpy(thr).cuda()
    need = lib.acg_fss_scales_workspace_bytes(4, M, C, H, W, T, 1)
    assert need % 16 == 0 and need > 0
    for seed in (0, 1):
        xd, yd = _device(x, "nhwc", C, 4, seed=seed, nan=0.3 * (seed == 1)), _device(y, "nhwc", C, 16, seed=10 + seed, nan=0.3 * (seed == 1))
        n_out, n_ens = 4 * C * T * nl * 3, 2 * C * T * nl * 3
        out, ens = Buf.out(GUARD + 2 * n_out, np.uint32), Buf.out(GUARD + 2 * n_ens, np.uint32)
        ws = Buf(GUARD + need // 4, dtype=np.uint32)               # 0xFFFFFFFF everywhere
        rc = _abi_call(lib, xd, yd, 4, M, C, H, W, (H * W * 4, 4, 1), (H * W * 16, 16, 1), thr_d, T, out.at(GUARD), ens.at(GUARD),
                       ws.at(GUARD), need)
        assert rc == 0, lib.acg_last_error().decode()
        for buf, ref in ((out, want), (ens, want_ens)):
            o = buf.host()                                         # checks the words behind the buffer
            assert np.all(o[:GUARD] == 0xFFFFFFFF)                 # and these are the words in front of it
            assert np.array_equal(o[GUARD:].view(np.int64).reshape(ref.shape), ref), seed
        assert np.all(ws.host()[:GUARD] == 0xFFFFFFFF)
    Buf.check_all()


@pytest.mark.parametrize("H,W", ((63, 65), (321, 321)))
def test_repeatable_and_the_same_bits_replayed_from_a_graph(H, W):
    from dtgan_amd import ops
    x, y, thr, ref = _case("shifted", H, W)
    xd, yd = _device(x, "nhwc", 3, 4, seed=1), _device(y[:1], "nchw", 3)      # two members of one truth
    thr_d = torch.from_numpy(thr.copy()).cuda()
    nl = R.levels(H, W)
    out = torch.full((2, 3, 3, nl, 3), -7, dtype=torch.int64, device="cuda")
    ens = torch.full((1, 3, 3, nl, 3), -7, dtype=torch.int64, device="cuda")
    call = lambda: ops.fss_scales(xd, yd, 3, "nhwc", "nchw", thr_d, x_per_y=2, ensemble=True, out=(out, ens))
    call()                                                         # the workspace exists before the capture
    first = out.cpu().numpy(), ens.cpu().numpy()
    call()
    assert np.array_equal(out.cpu().numpy(), first[0]) and np.array_equal(ens.cpu().numpy(), first[1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            call()
    torch.cuda.current_stream().wait_stream(s)
    out.fill_(-7), ens.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), first[0]) and np.array_equal(ens.cpu().numpy(), first[1])
    assert np.array_equal(first[0], R.triples(x, y[:1], thr, x_per_y=2)) and np.array_equal(first[1], R.ens_triples(x, y[:1], thr, 2))


def test_kernel_refuses_bad_arguments_before_launching():
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    x = torch.zeros(1 << 20, device="cuda")
    thr_d = torch.zeros(8, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    big = ws.numel()
    need = lib.acg_fss_scales_workspace_bytes(2, 1, 1, 64, 64, 1, 0)
    assert need == 2 * 2 * 64 * 12
    # rows, x_per_y, C, H, W, (x strides), (y strides), T, out?, ens?, workspace offset, bytes, status, a word of the message
    bad = [(6, 4, 1, 64, 64, None, None, 1, 1, 0, 0, big, -1, "x_per_y"), (6, 0, 1, 64, 64, None, None, 1, 1, 0, 0, big, -1, "x_per_y"),
           (130, 65, 1, 8, 8, None, None, 1, 1, 0, 0, big, -1, "x_per_y"),
           (2, 1, 1, 64, 64, (4096, 0, 4096), None, 1, 1, 0, 0, big, -1, "strides"),
           (2, 1, 1, 64, 64, None, (0, 1, 4096), 1, 1, 0, 0, big, -1, "strides"),
           (2, 1, 1, 64, 64, None, (4096, 1, -1), 1, 1, 0, 0, big, -1, "strides"),
           (2, 1, 1, 64, 64, None, None, 1, 0, 0, 0, big, -1, "both NULL"), (2, 1, 1, 0, 64, None, None, 1, 1, 0, 0, big, -1, "H x W"),
           (2, 1, 1, 64, 1025, None, None, 1, 1, 0, 0, big, -1, "H x W"), (2, 1, 1, 64, 64, None, None, 9, 1, 0, 0, big, -1, "thresholds"),
           (2, 1, 1, 64, 64, None, None, 0, 1, 0, 0, big, -1, "thresholds"), (2, 1, 0, 64, 64, None, None, 1, 1, 0, 0, big, -1, "C >= 1"),
           (0, 1, 1, 64, 64, None, None, 1, 1, 0, 0, big, -1, "rows >= 1"),
           (2, 1, 1, 64, 64, None, None, 1, 1, 1, 0, need - 1, -2, "workspace too small"),
           (2, 1, 1, 64, 64, None, None, 1, 1, 0, 8, need, -1, "aligned"),
           (1 << 22, 1, 1, 1024, 1, None, None, 1, 1, 0, 0, big, -1, "too many planes"),      # 2^32 image rows
           # the order: rows before strides before the pairing before the outputs before the extent before T
           (0, 0, 1, 64, 64, (0, 0, 0), None, 1, 0, 0, 0, big, -1, "rows >= 1"), (2, 3, 1, 64, 64, (0, 1, 1), None, 1, 0, 0, 0, big, -1, "strides"),
           (2, 3, 1, 0, 64, None, None, 9, 0, 0, 0, big, -1, "x_per_y"), (2, 1, 1, 0, 64, None, None, 9, 0, 0, 0, big, -1, "both NULL"),
           (2, 1, 1, 0, 64, None, None, 9, 1, 0, 8, big, -1, "H x W"), (2, 1, 1, 64, 64, None, None, 9, 1, 0, 8, big, -1, "thresholds")]
    for rows, per, C, H, W, sx, sy, T, has_out, has_ens, off, nbytes, rc_want, word in bad:
        plane = max(H * W, 1)                                      # an extent of 0 is refused for itself, not for a stride
        sx, sy = sx or (plane, 1, plane), sy or (plane, 1, plane)
        out = torch.full((4096,), -7, dtype=torch.int64, device="cuda")
        ens = torch.full((4096,), -7, dtype=torch.int64, device="cuda")
        rc = _abi_call(lib, x, x, rows, per, C, H, W, sx, sy, thr_d, T, ops._ptr(out) if has_out else None,
                       ops._ptr(ens) if has_ens else None, ctypes.c_void_p(ws.data_ptr() + off), nbytes)
        msg = lib.acg_last_error().decode()
        assert rc == rc_want and msg.startswith("acg_fss_scales") and word in msg, (rows, per, C, H, W, rc, msg)
        torch.cuda.synchronize()
        assert torch.all(out == -7) and torch.all(ens == -7)       # nothing was written
    P = (4096, 1, 4096)
    rc = _abi_call(lib, x, x, 2, 1, 1, 64, 64, P, P, thr_d, 1, ops._ptr(out), None, None, 0)
    assert rc == -2 and torch.all(out == -7)                       # a missing workspace
    rc = _abi_call(lib, None, x, 2, 1, 1, 64, 64, P, P, thr_d, 1, ops._ptr(out), None, ctypes.c_void_p(ws.data_ptr()), big)
    assert rc == -1 and "null tensor" in lib.acg_last_error().decode()
    rc = _abi_call(lib, x, x, 2, 1, 1, 64, 64, P, P, thr_d, 1, ops._ptr(out), None, ctypes.c_void_p(ws.data_ptr()), need)
    assert rc == 0, lib.acg_last_error().decode()                  # and the call they all fall short of
    torch.cuda.synchronize()
    assert out[:42].view(2, 7, 3)[:, 0].tolist() == [[4096] * 3] * 2 and torch.all(out[42:] == -7)      # zeros >= 0: every cell
    with pytest.raises(_lib.AcgError, match="out"):                  # through ops: an output of ops.fss's shape
        ops.fss_scales(x.view(4, 1, 512, 512), x.view(4, 1, 512, 512), 1, "nchw", "nchw", np.zeros((1, 1), np.float32),
                       out=torch.zeros((4, 1, 1, 1, 3), dtype=torch.int64, device="cuda"))
    with pytest.raises(_lib.AcgError, match="thresholds"):
        ops.fss_scales(x.view(4, 1, 512, 512), x.view(4, 1, 512, 512), 1, "nchw", "nchw", np.zeros((1, 9), np.float32))


@pytest.mark.parametrize("S", (64, 48))
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_translate_fss_scales_equals_generate_multi_and_the_reference(prec, S):
    from hip_util import precision
    from dtgan_amd import ops
    N, M = 3, 5
    nl = R.levels(S, S)
    with precision(prec):
        m = _model()
        A, B, g = _inputs(N, S)
        z = torch.randn(N * M, m.opt.nlatent, 1, 1, device="cuda", generator=g)
        plain = m.translate_fss(A, M, B, THR, WIN, z=z)
        assert set(plain) == {"members", "ens_prob", "ens_mean"}       # the default call is what it was
        r = m.translate_fss(A, M, B, THR, WIN, z=z, scales=True)
        assert set(r) == set(plain) | {"members_scale", "ens_prob_scale", "ens_mean_scale"}
        for k in plain:
            assert torch.equal(r[k], plain[k]), k
        assert r["members_scale"].shape == (N, M, 3, 3, nl, 3) and r["ens_prob_scale"].shape == r["ens_mean_scale"].shape == (N, 3, 3, nl, 3)
        assert all(v.dtype == torch.int64 and not v.requires_grad for v in r.values())
        with torch.no_grad():
            members = m.generate_multi(A, z)
        direct, direct_ens = ops.fss_scales(members, B, 3, "nchw", "nchw", THR, x_per_y=M, ensemble=True)
        assert torch.equal(r["members_scale"].reshape(N * M, 3, 3, nl, 3), direct) and torch.equal(r["ens_prob_scale"], direct_ens)
        mean = m.translate_ensemble(A, M, z=z, real_B=B)["mean"]
        assert torch.equal(r["ens_mean_scale"], ops.fss_scales(mean, B, 3, "nchw", "nchw", THR))
        Bh, mh, meanh = B.cpu().numpy(), members.cpu().numpy(), mean.cpu().numpy()
        assert np.array_equal(direct.cpu().numpy(), R.triples(mh, Bh, THR, x_per_y=M))
        assert np.array_equal(direct_ens.cpu().numpy(), R.ens_triples(mh, Bh, THR, M))
        assert np.array_equal(r["ens_mean_scale"].cpu().numpy(), R.triples(meanh, Bh, THR))
        assert torch.equal(r["members_scale"][..., 0, :], r["members"][..., 0, :])      # level 0 is the window 1
        one = m.translate_fss(A, M, B, torch.from_numpy(THR).cuda(), WIN, z=z, chunk=M, scales=True)   # one input per group
        for k in r:
            assert torch.equal(r[k], one[k]), k


def test_translate_fss_scales_host_syncs_do_not_grow_with_groups():
    m = _model()
    A, B, _ = _inputs(4, 64, seed=7)
    M = 3
    thr = torch.from_numpy(THR).cuda()
    m.translate_fss(A, M, B, thr, WIN, scales=True)                # warm-up
    n0 = _count_sync_warnings(lambda: m.translate_fss(A, M, B, thr, WIN))
    n1 = _count_sync_warnings(lambda: m.translate_fss(A, M, B, thr, WIN, scales=True))
    n4 = _count_sync_warnings(lambda: m.translate_fss(A, M, B, thr, WIN, chunk=M, scales=True))
    assert n0 == n1 == n4 and n1 <= 1, (n0, n1, n4)


def _run(experiment, res_dir, *extra):
    out = run_test(experiment, "fss", "--n_samples", "4", "--fss_windows", "3,9,17", "--res_dir", res_dir, *extra)
    return out, dict(np.load(os.path.join(experiment["expr"], res_dir, "fss.npz")))


def test_metric_fss_with_scales(experiment):
    S = EVAL_S
    from dtgan_amd import eval_metrics as EM
    from dtgan_amd.dataloader import load_numpy_data
    out0, arr0 = _run(experiment, "res_fss_scales_off", "--fss_scales", "0")
    out1, arr1 = _run(experiment, "res_fss_scales_on", "--fss_scales", "1")
    num = r"(-?\d+\.\d{4}|nan)"
    pat = (r"^DEV_ISS_B: %s, TEST_ISS_B: %s, TEST_SKILL_SCALE_B: %s, TEST_SKILL_SCALE_PROB_B: %s, TEST_SKILL_SCALE_MEAN_B: %s, "
           r"TEST_SKILL_SCALE_A: %s$" % ((num,) * 6))
    mt = re.search(pat, out1, re.M)
    assert mt, out1[-2000:]
    assert "ISS" not in out0 and "SKILL_SCALE" not in out0         # with 0: the output and the file of before
    old = {"n_samples", "windows", "thresholds_B", "thresholds_A"}
    old |= {"%s_%s_%s" % (split, q, k) for split in ("dev", "test") for k in EM.FSS_PAIRS
            for q in ("sums", "fss", "bias", "csi", "base_rate", "useful_scale")}
    assert set(arr0) == old, set(arr0) ^ old
    fss_line = lambda o: re.search(r"^DEV_FSS_B: .*$", o, re.M).group(0)
    assert fss_line(out0) == fss_line(out1)
    for k in old:                                                  # the old entries do not move
        assert arr0[k].dtype == arr1[k].dtype and np.array_equal(arr0[k], arr1[k], equal_nan=True), k
    new = {"scales"} | {"%s_%s_%s" % (split, q, k) for split in ("dev", "test") for k in EM.FSS_PAIRS
                        for q in ("scale_sums", "mse_scale", "iss", "en_rel", "mse_random", "skill_scale")}
    assert set(arr1) == old | new, set(arr1) ^ (old | new)
    M, C, Tn, nl = 4, 3, 3, R.levels(S, S)
    assert arr1["scales"].dtype == np.int64 and np.array_equal(arr1["scales"], 2 ** np.arange(nl))
    trainA, trainB, devA, devB, testA, testB = load_numpy_data(experiment["data"], grid_size=S)
    for split, A, B in (("dev", np.asarray(devA), np.asarray(devB)), ("test", np.asarray(testA), np.asarray(testB))):
        for k in EM.FSS_PAIRS:
            g = lambda q: arr1["%s_%s_%s" % (split, q, k)]
            sums = g("scale_sums")
            assert sums.shape == (C, Tn, nl, 3) and sums.dtype == np.int64 and np.all(sums >= 0), (split, k)
            for q in ("mse_scale", "iss", "en_rel"):
                assert g(q).shape == (C, Tn, nl) and g(q).dtype == np.float64, (split, k, q)
            assert g("mse_random").shape == (C, Tn) and g("mse_random").dtype == np.float64
            assert g("skill_scale").shape == (C, Tn) and g("skill_scale").dtype == np.int64 and np.all(np.isin(g("skill_scale"), arr1["scales"]))
            members = M if k == "ens_prob_B" else 1
            truth, thr = (A, arr1["thresholds_A"]) if k == "fake_A" else (B, arr1["thresholds_B"])
            pairs = len(truth) * (M if k == "members_B" else 1)
            cells = pairs * S * S
            n_f = arr1["%s_scale_sums_members_B" % split][..., 0, 0] if k == "ens_prob_B" else None
            ref = R.summary(sums, cells, members, n_f)
            for q, name in (("mse", "mse_scale"), ("iss", "iss"), ("en_rel", "en_rel"), ("mse_random", "mse_random"), ("skill_scale", "skill_scale")):
                assert np.allclose(g(name), ref[q], rtol=1e-12, atol=1e-15, equal_nan=True), (split, k, q)
            # level 0 is the window-1 triple of the same run, and the components add up to the plain MSE of the events
            box = arr1["%s_sums_%s" % (split, k)][..., 0, :].astype(np.float64)
            assert np.array_equal(sums[..., 0, :], arr1["%s_sums_%s" % (split, k)][..., 0, :]), (split, k)
            plain = (box[..., 0] / members ** 2 + box[..., 1] - 2 * box[..., 2] / members) / cells
            assert np.allclose(g("mse_scale").sum(-1), plain, rtol=1e-12, atol=1e-15), (split, k)
            # the observed side is the reference on the paired real field, once per pair; exactly
            assert np.array_equal(sums[..., 1], R.triples(truth, truth, thr).sum(0)[..., 1] * (pairs // len(truth))), (split, k)
    t = 2                                                          # the highest threshold
    line = mt.groups()
    for i, key in ((0, "dev_iss_members_B"), (1, "test_iss_members_B")):
        v = arr1[key][:, t, 0]
        assert (line[i] == "nan" and np.all(np.isnan(v))) or abs(float(line[i]) - np.nanmean(v)) < 1e-4, (key, line[i], v)
    for i, k in enumerate(EM.FSS_PAIRS):
        assert abs(float(line[2 + i]) - arr1["test_skill_scale_" + k][:, t].mean()) < 1e-4, k
    # B -> A in process: the reference on predict_A's fields gives the file's sums, exactly, on both splits
    with checkpoint_model(experiment) as model:
        for split, A, B in (("dev", devA, devB), ("test", testA, testB)):
            with torch.no_grad():
                fake_A = model.predict_A(torch.as_tensor(np.asarray(B)).cuda()).cpu().numpy()
            assert np.array_equal(arr1[split + "_scale_sums_fake_A"], R.triples(fake_A, np.asarray(A), arr1["thresholds_A"]).sum(0)), split

