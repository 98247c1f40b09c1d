"""GPU tests of the radially averaged power spectra: acg_radial_spectrum against tests/spectrum_ref.py, model.translate_spectrum
against generate_multi / translate_ensemble and the reference, and `python -m dtgan_amd.test --metric spectrum` in a child
process."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import spectrum_ref as R
from eval_cases import checkpoint_model, S as EVAL_S, count_sync_warnings as _count_sync_warnings, experiment, run_test  # noqa: F401  (the fixture)
from field_cases import LAYOUTS, field_operand as _device
from model_cases import ensemble_inputs as _inputs, ensemble_model as _model
from spectrum_ref import within as _within

pytestmark = pytest.mark.gpu

ROWS = 3
TAU = R.TAU                       # the bar of spectrum_ref.within


@functools.lru_cache(maxsize=None)
def _case(kind, S):
    """the fields (ROWS, 3, S, S), their reference spectra and mean squares"""
    x = R.make_fields(kind, S, rows=ROWS, C=3)
    return x, R.rapsd(x), np.mean(x.astype(np.float64) ** 2, axis=(-2, -1))


def _spectrum(xd, C, layout):
    from dtgan_amd import ops
    out = ops.radial_spectrum(xd, C, layout)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("layout,C,Cp", LAYOUTS)
@pytest.mark.parametrize("S", R.FIELD_SIZES)
def test_kernel_matches_reference(S, layout, C, Cp):
    for kind in R.FIELD_KINDS:
        x, ref, E = _case(kind, S)
        got = _spectrum(_device(x, layout, C, Cp), C, layout)
        assert got.shape == (ROWS, C, S // 2 + 1)
        _within(got, ref[:, :C], E[:, :C], "%s S=%d %s C=%d Cp=%d" % (kind, S, layout, C, Cp))


@pytest.mark.parametrize("S", R.FIELD_SIZES)
def test_exact_cases_leak_nothing(S):
    const = np.full((ROWS, 3, S, S), 0.7, dtype=np.float32)
    got = _spectrum(_device(const, "nhwc", 3, 4), 3, "nhwc")
    E = np.float64(np.float32(0.7)) ** 2
    print("constant S=%d: largest bin beyond 0 %.3e (allowed %.3e)" % (S, got[..., 1:].max(), TAU ** 2 * E))
    assert np.all(np.abs(got[..., 1:]) <= TAU ** 2 * E)
    assert np.allclose(got[..., 0], E * S * S, rtol=1e-5)
    wave, ref, Ew = _case("plane_wave", S)
    got = _spectrum(_device(wave, "nchw", 3, 3), 3, "nchw")
    others = np.delete(got, 5, axis=-1)
    print("plane wave S=%d: largest bin beside 5 %.3e (allowed %.3e)" % (S, np.abs(others).max(), TAU ** 2 * Ew.min()))
    assert np.all(np.abs(others) <= TAU ** 2 * Ew[..., None])
    assert np.allclose(got[..., 5], (S * S / 2.) / R.bin_counts(S)[5], rtol=1e-4)


@pytest.mark.parametrize("S", R.FIELD_SIZES)
def test_the_nyquist_column_away_from_fy_0(S):
    """(-1)^w cos(2 pi m h / S): the cells (+-m, S/2) of the packed column.  At m = nyquist_row(S) they are the last of ring
    S/2, one row further they lie in the dropped corner and every ring stays empty"""
    m, last = R.nyquist_row(S), S // 2
    for mm, layout, Cp in ((m, "nhwc", 4), (m + 1, "nchw", 3)):
        x = R.make_fields("nyquist_column", S, rows=1, C=3, m=mm)
        E = np.mean(x.astype(np.float64) ** 2, axis=(-2, -1))
        got = _spectrum(_device(x, layout, 3, Cp), 3, layout)
        empty = np.delete(got, last, axis=-1) if mm == m else got
        print("nyquist column S=%d m=%d: bin %d holds %.6e, largest other bin %.3e (allowed %.3e)"
              % (S, mm, last, got[..., last].max(), np.abs(empty).max(), TAU ** 2 * E.min()))
        assert np.all(np.isfinite(got)) and np.all(np.abs(empty) <= TAU ** 2 * E[..., None])
        if mm == m:
            assert np.allclose(got[..., last], (S * S / 2.) / R.bin_counts(S)[last], rtol=1e-4)


@pytest.mark.parametrize("S", R.FIELD_SIZES)
def test_repeatable_and_the_same_bits_in_both_layouts(S):
    x, _, _ = _case("tanh_red", S)
    nhwc, nchw = _device(x, "nhwc", 3, 4), _device(x, "nchw", 3, 3)
    a, b = _spectrum(nhwc, 3, "nhwc"), _spectrum(nhwc, 3, "nhwc")
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    c = _spectrum(nchw, 3, "nchw")
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
    wide = _spectrum(_device(x, "nhwc", 3, 16, seed=1), 3, "nhwc")          # the scalar loads of a C16 tensor as well
    assert np.array_equal(a.view(np.uint32), wide.view(np.uint32))


@pytest.mark.parametrize("S", R.FIELD_SIZES)
def test_the_path_a_size_takes(S):
    """one workgroup per field up to S = 128, the row and the column pass above"""
    from dtgan_amd import _lib
    x, _, _ = _case("white", S)
    _spectrum(_device(x, "nchw", 1, 1), 1, "nchw")
    k = _lib.query("acg_last_kernel").decode()
    assert k == ("spectrum_field<%d>" % S if S <= 128 else "spectrum_rows<%d> + spectrum_cols<%d>" % (S, S)), k
    assert (_lib.query("acg_radial_spectrum_workspace_bytes", ROWS, 3, S) == 0) == (S <= 128)


def test_kernel_refuses_bad_arguments_before_launching():
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    x = torch.zeros(1 << 16, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    need = lib.acg_radial_spectrum_workspace_bytes(1, 1, 256)
    assert need == 256 * 128 * 8 and need <= ws.numel()
    for S, C, nbytes, rc_want in ((192, 1, ws.numel(), -1), (8, 1, ws.numel(), -1), (2048, 1, ws.numel(), -1), (64, 0, ws.numel(), -1),
                                  (256, 1, need - 1, -2)):
        out = torch.full((1, 1, 1025), -7.0, device="cuda")
        rc = lib.acg_radial_spectrum(ops._ptr(x), 1, C, S, S * S, 1, S * S, ops._ptr(out), ops._ptr(ws), nbytes, ops._stream())
        msg = lib.acg_last_error().decode()
        assert rc == rc_want and msg.startswith("acg_radial_spectrum"), (S, C, rc, msg)
        if rc_want == -1 and C > 0:
            assert str(S) in msg and "power of two" in msg, msg       # the size and the rule
        torch.cuda.synchronize()
        assert torch.all(out == -7.0)                                  # nothing was written
    for shape in ((1, 1, 192, 192), (1, 1, 64, 32), (1, 1, 8, 8)):
        with pytest.raises(_lib.AcgError, match="power of two"):
            ops.radial_spectrum(torch.zeros(shape, device="cuda"), 1, "nchw")


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_translate_spectrum_equals_generate_multi_and_the_reference(prec):
    from hip_util import precision
    from dtgan_amd import ops
    N, M = 3, 5
    with precision(prec):
        m = _model()
        A, B, g = _inputs(N)
        z = torch.randn(N * M, m.opt.nlatent, 1, 1, device="cuda", generator=g)
        r = m.translate_spectrum(A, M, z=z, real_B=B)
        assert set(r) == {"members", "ens_mean", "target"}
        assert r["members"].shape == (N, M, 3, 33) and r["ens_mean"].shape == (N, 3, 33) and r["target"].shape == (N, 3, 33)
        with torch.no_grad():
            members = m.generate_multi(A, z)
        direct = ops.radial_spectrum(members, 3, "nchw")
        assert torch.equal(r["members"].reshape(N * M, 3, 33), direct)         # the same members, bit for bit
        mean = m.translate_ensemble(A, M, z=z, real_B=B)["mean"]
        assert torch.equal(r["ens_mean"], ops.radial_spectrum(mean, 3, "nchw"))
        Bh = B.cpu().numpy()
        _within(r["target"].cpu().numpy(), R.rapsd(Bh), np.mean(Bh.astype(np.float64) ** 2, axis=(-2, -1)), "target " + prec)
        mh = members.cpu().numpy()
        _within(direct.cpu().numpy(), R.rapsd(mh), np.mean(mh.astype(np.float64) ** 2, axis=(-2, -1)), "members " + prec)
        one = m.translate_spectrum(A, M, z=z, real_B=B, chunk=M)                # one input per group
        for k in r:
            assert torch.equal(r[k], one[k]), k
        bare = m.translate_spectrum(A, M, z=z)
        assert set(bare) == {"members", "ens_mean"} and torch.equal(bare["members"], r["members"])


def test_translate_spectrum_refusals():
    from dtgan_amd import _lib
    m = _model()
    A, B, _ = _inputs(2)
    with pytest.raises(ValueError, match="n_samples"):
        m.translate_spectrum(A, 65)
    with pytest.raises(ValueError, match="codes"):
        m.translate_spectrum(A, 2, z=torch.zeros(3, m.opt.nlatent, 1, 1, device="cuda"))
    with pytest.raises(ValueError, match="cannot hold"):
        m.translate_spectrum(A, 4, chunk=3)
    with pytest.raises(_lib.AcgError, match="power of two"):
        m.translate_spectrum(torch.zeros(1, 3, 48, 48, device="cuda"), 2)


def test_cycle_gan_gives_identical_member_spectra():
    N, M = 2, 6
    m = _model("cycle_gan")
    A, _, _ = _inputs(N, seed=5)
    r = m.translate_spectrum(A, M)
    for k in range(M):
        assert torch.equal(r["members"][:, k], r["ens_mean"]), k


def test_translate_spectrum_host_syncs_do_not_grow_with_groups():
    m = _model()
    A, B, _ = _inputs(4, seed=7)
    M = 3
    m.translate_spectrum(A, M, real_B=B)                           # warm-up
    n1 = _count_sync_warnings(lambda: m.translate_spectrum(A, M, real_B=B))
    n4 = _count_sync_warnings(lambda: m.translate_spectrum(A, M, real_B=B, chunk=M))
    assert n1 == n4 and n1 <= 1, (n1, n4)


def test_metric_spectrum(experiment):
    S = EVAL_S
    from dtgan_amd import eval_metrics as EM
    from dtgan_amd.dataloader import AlignedIterator, load_numpy_data
    out = run_test(experiment, "spectrum", "--n_samples", "4", "--res_dir", "res_spectrum")
    pat = r"^DEV_LSD_B: (\d+\.\d{4}), TEST_LSD_B: (\d+\.\d{4}), TEST_LSD_MEAN_B: (\d+\.\d{4}), TEST_LSD_A: (\d+\.\d{4})$"
    mt = re.search(pat, out, re.M)
    assert mt, out[-2000:]
    arr = np.load(os.path.join(experiment["expr"], "res_spectrum", "spectrum.npz"))
    nb = S // 2 + 1
    assert int(arr["n_samples"]) == 4 and np.array_equal(arr["bin_counts"], R.bin_counts(S))
    for split, n in (("dev", 6), ("test", 5)):
        for k in ("psd_real_B", "psd_members_B", "psd_ens_mean_B", "psd_real_A", "psd_fake_A"):
            a = arr["%s_%s" % (split, k)]
            assert a.shape == (3, nb) and a.dtype == np.float64 and np.all(np.isfinite(a)) and np.all(a >= 0), (split, k)
        for k in ("lsd_B", "lsd_mean_B", "lsd_A"):
            a = arr["%s_%s" % (split, k)]
            assert a.shape == () and np.isfinite(a) and a >= 0, (split, k)
        per = arr["%s_lsd_B_per_input" % split]
        assert per.shape == (n,) and np.all(np.isfinite(per))
    assert abs(float(mt.group(2)) - float(arr["test_lsd_B"])) < 1e-4
    # the stored spectra of the real fields are the reference's
    _, _, devA, devB, testA, testB = load_numpy_data(experiment["data"], grid_size=S)
    for key, data in (("test_psd_real_B", testB), ("dev_psd_real_A", devA)):
        ref, E = R.rapsd(data).mean(0), np.mean(data.astype(np.float64) ** 2, axis=(-2, -1)).max()
        assert np.all(np.abs(arr[key] - ref) <= TAU * np.sqrt(ref * E) + TAU ** 2 * E), key
    # the same numbers in process, from the same seed
    with checkpoint_model(experiment) as model:
        torch.manual_seed(12345)
        EM.eval_spectrum(AlignedIterator(devA, devB, batch_size=len(devA)), model, 4)
        test = EM.eval_spectrum(AlignedIterator(testA, testB, batch_size=len(testA)), model, 4)
    assert abs(float(mt.group(2)) - test["lsd_B"]) < 1e-4, (mt.group(2), test["lsd_B"])
    assert np.allclose(arr["test_lsd_B_per_input"], test["lsd_B_per_input"], rtol=1e-6)

