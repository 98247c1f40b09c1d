"""GPU tests of the paired cross-spectra: acg_cross_spectrum against tests/cross_spectrum_ref.py, model.translate_coherence
against generate_multi / translate_ensemble and the reference, and `python -m dtgan_amd.test --metric coherence` in a child
process."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import cross_spectrum_ref as X
import spectrum_ref as R
from guard_util import GUARD, Buf
from eval_cases import checkpoint_model, S as EVAL_S, count_sync_warnings as _count_sync_warnings, experiment, run_test  # noqa: F401  (the fixture)
from field_cases import LAYOUTS, field_operand as _device
from model_cases import ensemble_inputs as _inputs, ensemble_model as _model
from spectrum_ref import TAU, within as _within

pytestmark = pytest.mark.gpu

SIZES = tuple(S for S, _, _ in X.PAIR_CASES)
# |cxy - ref| <= CTAU (sqrt(pxx_ref Ey) + sqrt(pyy_ref Ex)) + CTAU^2 sqrt(Ex Ey) per bin, Ex, Ey the fields' mean squares: a
# per-cell transform error of tau sqrt(E) S in each field and Cauchy-Schwarz over a ring.  Measured, not chosen:
# torch.fft.fft2 in float32 on the CPU, binned in float64, needs tau = 1.0087e-5 over every bin, pair kind and size of
# X.PAIR_CASES (`python tools/spectrum_bench.py --cpu-cross-tolerance`; the largest is the shifted pair at S = 1024).  The
# constant is 4 x that: a different butterfly order.  pxx and pyy are held to the bound of test_hip_spectrum (that run needed
# 5.3733e-5 for them, inside that test's measured 1.3214e-4).
CTAU = 4 * 1.0087e-5
# x in every layout of the single-field test, crossed with a planar and an NHWC y; the two largest sizes once, one channel
COMBOS = [(S, rows, lx, C, Cp, ly) for S, rows, Cc in X.PAIR_CASES if Cc == 3 for lx, C, Cp in LAYOUTS for ly in ("nchw", "nhwc")]
COMBOS += [(S, rows, "nhwc", 1, 4, "nchw") for S, rows, Cc in X.PAIR_CASES if Cc == 1]


@functools.lru_cache(maxsize=None)
def _case(kind, S):
    """the pair (rows, C, S, S) each, their reference triples (rows, C, 3, nb) and mean squares"""
    rows, C = next((r, c) for s, r, c in X.PAIR_CASES if s == S)
    x, y = X.make_pairs(kind, S, rows=rows, C=C)
    ms = lambda a: np.mean(a.astype(np.float64) ** 2, axis=(-2, -1))
    return x, y, X.cross_spectrum(x, y), ms(x), ms(y)


def _y_device(y, layout, C, Cp, seed=7):
    return _device(y, layout, C, Cp if layout == "nhwc" else C, seed=seed)


def _cross(xd, yd, C, lx, ly, x_per_y=1):
    """ops.cross_spectrum into a NaN-poisoned output -> host (rows, C, 3, nb)"""
    from dtgan_amd import ops
    rows, S = xd.shape[0], xd.shape[2]
    out = torch.full((rows, C, 3, S // 2 + 1), float("nan"), device="cuda")
    assert ops.cross_spectrum(xd, yd, C, lx, ly, x_per_y=x_per_y, out=out) is out
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _cross_within(got, ref, Ex, Ey, what):
    """all three outputs of a call against the reference triples; no bin is excluded"""
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    _within(got[..., 0, :], ref[..., 0, :], Ex, what + " pxx")
    _within(got[..., 1, :], ref[..., 1, :], Ey, what + " pyy")
    d = np.abs(got[..., 2, :].astype(np.float64) - ref[..., 2, :])
    bound = X.cross_bound(ref, Ex, Ey, CTAU)
    print("%s cxy: tau needed %.3e (allowed %.3e)" % (what, X.cross_tolerance_needed(got[..., 2, :], ref, Ex, Ey), CTAU))
    assert np.all(d <= bound), (what, float((d / bound).max()), np.argwhere(d > bound)[:5])


@pytest.mark.parametrize("S,rows,lx,C,Cp,ly", COMBOS)
def test_kernel_matches_reference(S, rows, lx, C, Cp, ly):
    for kind in X.PAIR_KINDS:
        x, y, ref, Ex, Ey = _case(kind, S)
        got = _cross(_device(x, lx, C, Cp), _y_device(y, ly, C, Cp), C, lx, ly)
        assert got.shape == (rows, C, 3, S // 2 + 1)
        _cross_within(got, ref[:, :C], Ex[:, :C], Ey[:, :C], "%s S=%d x %s C=%d Cp=%d y %s" % (kind, S, lx, C, Cp, ly))


@pytest.mark.parametrize("S", SIZES)
def test_exact_cases(S):
    x, _, ref, Ex, _ = _case("same", S)
    C = x.shape[1]
    xd = _device(x, "nchw", C, C)
    same = _cross(xd, xd.clone(), C, "nchw", "nchw")
    _within(same[..., 2, :], ref[..., 0, :], Ex, "same S=%d: cxy against pxx" % S)
    neg = _cross(xd, -xd, C, "nchw", "nchw")
    _within(-neg[..., 2, :], ref[..., 0, :], Ex, "neg S=%d: -cxy against pxx" % S)
    zero = _cross(_device(x, "nhwc", C, 4), torch.zeros_like(xd), C, "nhwc", "nchw")
    _within(zero[..., 0, :], ref[..., 0, :], Ex, "zero y S=%d: pxx" % S)
    assert np.all(zero[..., 1, :] == 0) and np.all(zero[..., 2, :] == 0), np.abs(zero[..., 1:, :]).max()


@pytest.mark.parametrize("S", SIZES)
def test_the_nyquist_column_away_from_fy_0(S):
    """x = (-1)^w cos(2 pi m h / S) against itself and against 0.5 x: the cells (+-m, S/2) of both packed columns.  At
    m = nyquist_row(S) ring S/2 holds P = (S^2 / 2) / count of Pxx, and Pyy and Cxy in the ratios of the amplitudes; one row
    further the cells lie in the dropped corner and every ring of every output stays empty.  Empty: within TAU^2 of the mean
    squares Ex, Ey and, for Cxy, sqrt(Ex Ey)"""
    m, last = R.nyquist_row(S), S // 2
    for mm in (m, m + 1):
        x = R.make_fields("nyquist_column", S, rows=1, C=3, m=mm)
        Ex = _ms(x)
        xd = _device(x, "nchw", 3, 3)
        for a in (1.0, 0.5):
            got = _cross(xd, _y_device(np.float32(a) * x, "nhwc", 3, 4), 3, "nchw", "nhwc")
            for k, (name, scale) in enumerate((("pxx", 1.0), ("pyy", a * a), ("cxy", a))):
                g = got[..., k, :]
                empty = np.delete(g, last, axis=-1) if mm == m else g
                print("nyquist column S=%d m=%d y=%gx %s: bin %d holds %.6e, largest other bin %.3e (allowed %.3e)"
                      % (S, mm, a, name, last, g[..., last].max(), np.abs(empty).max(), TAU ** 2 * scale * Ex.min()))
                assert np.all(np.abs(empty) <= TAU ** 2 * scale * Ex[..., None]), (mm, a, name)
                if mm == m:
                    assert np.allclose(g[..., last], scale * (S * S / 2.) / R.bin_counts(S)[last], rtol=1e-4), (a, name)


@pytest.mark.parametrize("S", (32, 128))
def test_members_share_a_truth_through_x_per_y(S):
    """6 members against 2 truth rows at x_per_y = 3: bit for bit the call with every truth row repeated three times"""
    x = R.make_fields("tanh_red", S, rows=6, C=3)
    y = R.make_fields("red", S, rows=2, C=3, seed=1)
    xd, yd = _device(x, "nhwc", 3, 4), _device(y, "nchw", 3, 3)
    shared = _cross(xd, yd, 3, "nhwc", "nchw", x_per_y=3)
    repeated = _cross(xd, yd.repeat_interleave(3, 0), 3, "nhwc", "nchw")
    assert np.array_equal(shared.view(np.uint32), repeated.view(np.uint32))
    ref = X.cross_spectrum(x, np.repeat(y, 3, axis=0))
    ms = lambda a: np.mean(a.astype(np.float64) ** 2, axis=(-2, -1))
    _cross_within(shared, ref, ms(x), np.repeat(ms(y), 3, axis=0), "x_per_y S=%d" % S)
    assert not np.array_equal(shared[2], shared[3])                # member 3 is the first of the second truth


@pytest.mark.parametrize("S", (16, 64, 128, 256))
def test_repeatable_and_the_same_bits_in_every_layout(S):
    x, y, _, _, _ = _case("lowpass_noise", S)
    first = _cross(_device(x, "nchw", 3, 3), _device(y, "nchw", 3, 3), 3, "nchw", "nchw")
    for lx, Cpx in (("nchw", 3), ("nhwc", 4), ("nhwc", 16)):       # C16: the scalar loads
        for ly, Cpy in (("nchw", 3), ("nhwc", 4), ("nhwc", 16)):
            xd, yd = _device(x, lx, 3, Cpx, seed=1), _device(y, ly, 3, Cpy, seed=2)
            a, b = _cross(xd, yd, 3, lx, ly), _cross(xd, yd, 3, lx, ly)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (lx, Cpx, ly, Cpy)
            assert np.array_equal(a.view(np.uint32), first.view(np.uint32)), (lx, Cpx, ly, Cpy)


@pytest.mark.parametrize("S", (16, 64, 128, 256))
def test_guard_words_and_padded_channels(S):
    """through the C ABI: out starts as NaN, out and the workspace lie between guard words, and +-50 garbage in the padded
    channels of either operand changes no bit"""
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    x, y, _, _, _ = _case("indep", S)
    rows, C, nb = x.shape[0], 3, S // 2 + 1
    plain = _cross(_device(x, "nchw", 3, 3), _device(y, "nchw", 3, 3), 3, "nchw", "nchw")
    need = lib.acg_cross_spectrum_workspace_bytes(rows, C, S)
    for seed in (0, 1):
        xd, yd = _device(x, "nhwc", C, 4, seed=seed), _device(y, "nhwc", C, 16, seed=10 + seed)
        out = Buf.out(GUARD + rows * C * 3 * nb)
        ws = Buf(GUARD + need // 4, dtype=np.uint32)
        rc = lib.acg_cross_spectrum(ops._ptr(xd), ops._ptr(yd), rows, 1, C, S, S * S * 4, 4, 1, S * S * 16, 16, 1, out.at(GUARD),
                                    ws.at(GUARD) if need else None, need, ops._stream())
        assert rc == 0, lib.acg_last_error().decode()
        o = out.host()                                             # checks the words behind out
        assert np.all(np.isnan(o[:GUARD]))                         # and these are the words in front of it
        assert np.all(ws.host()[:GUARD] == 0xFFFFFFFF)
        got = o[GUARD:].reshape(rows, C, 3, nb)
        assert np.array_equal(got.view(np.uint32), plain.view(np.uint32)), seed
    Buf.check_all()


@pytest.mark.parametrize("S", SIZES)
def test_the_path_a_size_takes(S):
    """one workgroup per pair up to S = 64 (one size below the single-field switch), two passes above"""
    from dtgan_amd import _lib
    x, y, _, _, _ = _case("indep", S)
    _cross(_device(x, "nchw", 1, 1), _device(y, "nchw", 1, 1), 1, "nchw", "nchw")
    k = _lib.query("acg_last_kernel").decode()
    assert k == ("cross_spectrum_field<%d>" % S if S <= 64 else "cross_spectrum_rows<%d> + cross_spectrum_cols<%d>" % (S, S)), k
    need = _lib.query("acg_cross_spectrum_workspace_bytes", 3, 3, S)
    assert need == (0 if S <= 64 else 9 * S * S * 8), need         # both half spectra of every pair


def test_kernel_refuses_bad_arguments_before_launching():
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    x = torch.zeros(6 << 14, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    need = lib.acg_cross_spectrum_workspace_bytes(1, 1, 128)
    assert need == 128 * 128 * 8 and need <= ws.numel()
    big = ws.numel()
    # S, rows, x_per_y, C, (x strides), (y strides), workspace offset, bytes, the status and a word of the message
    bad = [(192, 1, 1, 1, None, None, 0, big, -1, "power of two"), (8, 1, 1, 1, None, None, 0, big, -1, "power of two"),
           (2048, 1, 1, 1, None, None, 0, big, -1, "power of two"), (64, 1, 1, 0, None, None, 0, big, -1, "C >= 1"),
           (64, 0, 1, 1, None, None, 0, big, -1, "rows >= 1"), (64, 1, 1, 1, (4096, 0, 4096), None, 0, big, -1, "strides"),
           (64, 1, 1, 1, None, (0, 1, 4096), 0, big, -1, "strides"), (64, 1, 1, 1, None, (4096, 1, -1), 0, big, -1, "strides"),
           (64, 6, 0, 1, None, None, 0, big, -1, "x_per_y"), (64, 6, -2, 1, None, None, 0, big, -1, "x_per_y"),
           (64, 6, 4, 1, None, None, 0, big, -1, "x_per_y"), (128, 1, 1, 1, None, None, 0, need - 1, -2, "workspace too small"),
           (128, 1, 1, 1, None, None, 4, need, -1, "aligned")]
    for S, rows, per, C, sx, sy, off, nbytes, rc_want, word in bad:
        sx, sy = sx or (S * S, 1, S * S), sy or (S * S, 1, S * S)
        out = torch.full((6, 1, 3, 1025), -7.0, device="cuda")
        rc = lib.acg_cross_spectrum(ops._ptr(x), ops._ptr(x), rows, per, C, S, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], ops._ptr(out),
                                    ctypes.c_void_p(ws.data_ptr() + off), nbytes, ops._stream())
        msg = lib.acg_last_error().decode()
        assert rc == rc_want and msg.startswith("acg_cross_spectrum") and word in msg, (S, rows, per, C, rc, msg)
        if word == "power of two":
            assert str(S) in msg, msg                                  # the size and the rule
        torch.cuda.synchronize()
        assert torch.all(out == -7.0)                                  # nothing was written
    rc = lib.acg_cross_spectrum(ops._ptr(x), ops._ptr(x), 1, 1, 1, 128, 1 << 14, 1, 1 << 14, 1 << 14, 1, 1 << 14, ops._ptr(out), None, 0,
                                ops._stream())
    assert rc == -2 and torch.all(out == -7.0)                         # a missing workspace above the switch
    for shape in ((1, 1, 192, 192), (1, 1, 64, 32), (1, 1, 8, 8)):
        with pytest.raises(_lib.AcgError, match="power of two"):
            ops.cross_spectrum(torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda"), 1, "nchw", "nchw")
    with pytest.raises(_lib.AcgError, match="x_per_y"):
        ops.cross_spectrum(torch.zeros(6, 1, 32, 32, device="cuda"), torch.zeros(2, 1, 32, 32, device="cuda"), 1, "nchw", "nchw", x_per_y=4)
    with pytest.raises(_lib.AcgError, match="do not pair"):
        ops.cross_spectrum(torch.zeros(6, 1, 32, 32, device="cuda"), torch.zeros(3, 1, 32, 32, device="cuda"), 1, "nchw", "nchw", x_per_y=3)


def _ms(a):
    return np.mean(a.astype(np.float64) ** 2, axis=(-2, -1))


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_translate_coherence_equals_generate_multi_and_the_reference(prec):
    from hip_util import precision
    from dtgan_amd import ops
    N, M = 3, 5
    with precision(prec):
        m = _model()
        A, B, g = _inputs(N)
        z = torch.randn(N * M, m.opt.nlatent, 1, 1, device="cuda", generator=g)
        r = m.translate_coherence(A, M, B, z=z)
        assert set(r) == {"members", "ens_mean"}
        assert r["members"].shape == (N, M, 3, 3, 33) and r["ens_mean"].shape == (N, 3, 3, 33)
        with torch.no_grad():
            members = m.generate_multi(A, z)
        direct = ops.cross_spectrum(members, B, 3, "nchw", "nchw", x_per_y=M)
        assert torch.equal(r["members"].reshape(N * M, 3, 3, 33), direct)      # the same members, bit for bit
        mean = m.translate_ensemble(A, M, z=z, real_B=B)["mean"]
        assert torch.equal(r["ens_mean"], ops.cross_spectrum(mean, B, 3, "nchw", "nchw"))
        Bh, mh, meanh = B.cpu().numpy(), members.cpu().numpy(), mean.cpu().numpy()
        Bm = np.repeat(Bh, M, axis=0)
        _cross_within(direct.cpu().numpy(), X.cross_spectrum(mh, Bm), _ms(mh), _ms(Bm), "members " + prec)
        _cross_within(r["ens_mean"].cpu().numpy(), X.cross_spectrum(meanh, Bh), _ms(meanh), _ms(Bh), "ens_mean " + prec)
        one = m.translate_coherence(A, M, B, z=z, chunk=M)                      # one input per group
        for k in r:
            assert torch.equal(r[k], one[k]), k
        assert not r["members"].requires_grad and not r["ens_mean"].requires_grad


def test_translate_coherence_refusals():
    from dtgan_amd import _lib
    m = _model()
    A, B, _ = _inputs(2)
    with pytest.raises(ValueError, match="n_samples"):
        m.translate_coherence(A, 65, B)
    with pytest.raises(ValueError, match="codes"):
        m.translate_coherence(A, 2, B, z=torch.zeros(3, m.opt.nlatent, 1, 1, device="cuda"))
    with pytest.raises(ValueError, match="cannot hold"):
        m.translate_coherence(A, 4, B, chunk=3)
    with pytest.raises(ValueError, match="does not pair"):
        m.translate_coherence(A, 2, B[:1])
    with pytest.raises(_lib.AcgError, match="power of two"):
        m.translate_coherence(torch.zeros(1, 3, 48, 48, device="cuda"), 2, torch.zeros(1, 3, 48, 48, device="cuda"))


def test_translate_coherence_host_syncs_do_not_grow_with_groups():
    m = _model()
    A, B, _ = _inputs(4, seed=7)
    M = 3
    m.translate_coherence(A, M, B)                                 # warm-up
    n1 = _count_sync_warnings(lambda: m.translate_coherence(A, M, B))
    n4 = _count_sync_warnings(lambda: m.translate_coherence(A, M, B, chunk=M))
    assert n1 == n4 and n1 <= 1, (n1, n4)


def test_metric_coherence(experiment):
    S = EVAL_S
    from dtgan_amd import eval_metrics as EM
    from dtgan_amd.dataloader import AlignedIterator, load_numpy_data
    pat = (r"^DEV_KEFF_B: (\d+\.\d{4}), TEST_KEFF_B: (\d+\.\d{4}), TEST_KEFF_MEAN_B: (\d+\.\d{4}), TEST_KEFF_A: (\d+\.\d{4}), "
           r"TEST_COH_B: (\d+\.\d{4})$")
    runs = []
    for res_dir in ("res_coherence", "res_coherence_again"):
        out = run_test(experiment, "coherence", "--n_samples", "4", "--res_dir", res_dir)
        mt = re.search(pat, out, re.M)
        assert mt, out[-2000:]
        runs.append((mt.groups(), dict(np.load(os.path.join(experiment["expr"], res_dir, "coherence.npz")))))
    (line, arr), (line2, arr2) = runs
    assert line == line2 and set(arr) == set(arr2)
    for k in arr:                                                  # two runs, the same file
        assert arr[k].dtype == arr2[k].dtype and np.array_equal(arr[k], arr2[k]), k
    nb = S // 2 + 1
    want = {"n_samples", "bin_counts"} | {"%s_%s_%s" % (split, q, k) for split in ("dev", "test") for k in EM.COHERENCE_PAIRS
                                          for q in ("sums", "coh", "r", "perr", "k_eff")}
    assert set(arr) == want, set(arr) ^ want
    assert int(arr["n_samples"]) == 4 and np.array_equal(arr["bin_counts"], R.bin_counts(S))
    _, _, devA, devB, testA, testB = load_numpy_data(experiment["data"], grid_size=S)
    for split, A, B in (("dev", devA, devB), ("test", testA, testB)):
        for k in EM.COHERENCE_PAIRS:
            sums, coh, r = arr["%s_sums_%s" % (split, k)], arr["%s_coh_%s" % (split, k)], arr["%s_r_%s" % (split, k)]
            perr, k_eff = arr["%s_perr_%s" % (split, k)], arr["%s_k_eff_%s" % (split, k)]
            assert sums.shape == (3, 3, nb) and sums.dtype == np.float64 and np.all(np.isfinite(sums)), (split, k)
            assert coh.shape == r.shape == perr.shape == (3, nb) and coh.dtype == np.float64, (split, k)
            assert np.all((coh >= 0) & (coh <= 1)) and np.all(np.abs(r) <= 1), (split, k)
            assert k_eff.shape == (3,) and k_eff.dtype == np.int64 and np.all((k_eff >= 1) & (k_eff <= nb)), (split, k)
            ref = X.summary(sums)
            assert np.allclose(coh, np.minimum(ref["coh"], 1)) and np.array_equal(k_eff, ref["k_eff"]), (split, k)
            # the truth's side of the triple is the reference's spectrum of the paired real field, once per pair
            truth, pairs = (A, len(A)) if k == "fake_A" else (B, len(B) * (4 if k == "members_B" else 1))
            want_pyy, E = R.rapsd(truth).sum(0) * (pairs // len(truth)), _ms(truth).max()
            assert np.all(np.abs(sums[:, 1] - want_pyy) <= pairs * (TAU * np.sqrt(R.rapsd(truth).max(0) * E) + TAU ** 2 * E)), (split, k)
            assert np.allclose(perr * pairs, sums[:, 0] + sums[:, 1] - 2 * sums[:, 2], rtol=1e-12), (split, k)
    assert abs(float(line[1]) - arr["test_k_eff_members_B"].mean()) < 1e-4
    assert abs(float(line[4]) - arr["test_coh_members_B"][:, 1:].mean()) < 1e-4
    # the same numbers in process, from the same seed
    with checkpoint_model(experiment) as model:
        torch.manual_seed(12345)
        EM.eval_coherence(AlignedIterator(devA, devB, batch_size=len(devA)), model, 4)
        test = EM.eval_coherence(AlignedIterator(testA, testB, batch_size=len(testA)), model, 4)
    for k in EM.COHERENCE_PAIRS:
        assert np.allclose(arr["test_sums_" + k], test["sums_" + k], rtol=1e-6), k
        assert np.array_equal(arr["test_k_eff_" + k], test["k_eff_" + k]), k

