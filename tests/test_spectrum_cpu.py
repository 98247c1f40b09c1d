"""CPU tests of the radially averaged power spectrum's definition (tests/spectrum_ref.py), of the log-spectral distance, of the
evaluator's spectrum option and of the two entry points' declarations."""
import numpy as np
import pytest

import abi
import dtgan_amd  # noqa: F401
from dtgan_amd import options as O
import spectrum_ref as R

SIZES = R.FIELD_SIZES


@pytest.mark.parametrize("S", [16, 64, 256])
def test_a_plane_wave_puts_its_power_into_two_cells_of_bin_5(S):
    h, w = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    x = np.cos(2 * np.pi * (3 * h + 4 * w) / S).astype(np.float32)
    P = R.power_plane(x)
    assert np.allclose(P[3, 4], S * S / 4., rtol=1e-6) and np.allclose(P[S - 3, S - 4], S * S / 4., rtol=1e-6)
    psd, counts = R.rapsd(x), R.bin_counts(S)
    assert np.allclose(psd[5], (S * S / 2.) / counts[5], rtol=1e-6)
    assert np.all(np.delete(psd, 5) < 1e-9 * psd[5])


@pytest.mark.parametrize("S", SIZES)
def test_the_nyquist_column_fills_ring_half_s_up_to_its_last_row_only(S):
    m, nb = R.nyquist_row(S), S // 2 + 1
    assert m * m <= S // 2 < (m + 1) * (m + 1)
    x = R.make_fields("nyquist_column", S, rows=1, C=1)[0, 0]
    P = R.power_plane(x)
    assert np.allclose(P[m, S // 2], S * S / 4., rtol=1e-6) and np.allclose(P[S - m, S // 2], S * S / 4., rtol=1e-6)
    psd = R.rapsd(x)
    assert np.allclose(psd[nb - 1], (S * S / 2.) / R.bin_counts(S)[nb - 1], rtol=1e-6)
    assert np.all(psd[:nb - 1] < 1e-9 * psd[nb - 1])
    beyond = R.rapsd(R.make_fields("nyquist_column", S, rows=1, C=1, m=m + 1)[0, 0])    # the dropped corner: no ring is filled
    assert np.all(beyond < 1e-9 * psd[nb - 1])


def test_a_constant_field_has_only_bin_0():
    S, c = 32, 0.7
    psd = R.rapsd(np.full((S, S), c, dtype=np.float32))
    assert np.allclose(psd[0], np.float64(np.float32(c)) ** 2 * S * S, rtol=1e-12)
    assert np.all(psd[1:] < 1e-20)


@pytest.mark.parametrize("S", [16, 128])
def test_parseval_with_the_dropped_corners(S):
    x = np.random.RandomState(S).uniform(-1, 1, (S, S)).astype(np.float32)
    P, b = R.power_plane(x), R.bin_index(S)
    E = np.mean(x.astype(np.float64) ** 2)
    total = np.sum(R.rapsd(x) * R.bin_counts(S)) + P[b > S // 2].sum()
    assert np.allclose(total, S * S * E, rtol=1e-12)


@pytest.mark.parametrize("S", SIZES)
def test_the_integer_bin_rule_is_the_rounded_root_and_counts_add_up(S):
    f = R.wavenumbers(S)
    s = f[:, None] ** 2 + f[None, :] ** 2
    b = R.bin_index(S)
    assert np.array_equal(b, np.floor(np.sqrt(s.astype(np.float64)) + 0.5).astype(np.int64))
    assert np.all((b * (b - 1) < s) | (s == 0)) and np.all(s <= b * (b + 1))
    counts = R.bin_counts(S)
    assert counts.shape == (S // 2 + 1,) and np.all(counts >= 1) and counts[0] == 1
    assert counts.sum() == S * S - np.count_nonzero(b > S // 2)


def test_log_spectral_distance():
    p = np.random.RandomState(0).uniform(0.1, 10, (3, 17))
    assert np.all(R.lsd(p, p) == 0)
    assert np.allclose(R.lsd(p, 10 * p), 10) and np.allclose(R.lsd(10 * p, p), 10)
    q = p.copy()
    q[:, 0] *= 1e6                                                 # bin 0 takes no part
    assert np.all(R.lsd(p, q) == 0)
    z = np.zeros((1, 5))
    assert np.all(R.lsd(z, z) == 0)                                # both clamped to 1e-30
    t = np.full((1, 5), 1e-20)
    assert np.allclose(R.lsd(t, z), 100)                           # 1e-20 against the clamp 1e-30: ten decades
    assert np.allclose(R.lsd_channels(np.stack([p, 10 * p], 1), np.stack([p, p], 1)), 5)


def test_the_evaluators_distance_is_the_references():
    from dtgan_amd import eval_metrics as EM
    rs = np.random.RandomState(3)
    p, q = rs.uniform(0, 5, (4, 3, 33)), rs.uniform(0, 5, (4, 3, 33))
    p[0, 0, 3] = 0
    assert np.allclose(EM.log_spectral_distance(p, q), R.lsd_channels(p, q), rtol=1e-14)


def test_the_spectrum_metric_parses():
    o = O.TestOptions().parse(["--chk_path", "c", "--dataroot", "d", "--metric", "spectrum"])
    assert o.metric == "spectrum" and o.n_samples == 16
    o = O.TestOptions().parse(["--chk_path", "c", "--dataroot", "d", "--metric", "spectrum", "--n_samples", "4"])
    assert o.n_samples == 4


@pytest.mark.parametrize("S", SIZES)
def test_ops_spectrum_bins_equals_the_reference(S):
    from dtgan_amd import ops
    got = ops.spectrum_bins(S)
    assert got.dtype == np.int64 and np.array_equal(got, R.bin_counts(S))


def test_ops_refuses_unsupported_sizes_on_the_host():
    from dtgan_amd import _lib, ops
    for S in (8, 192, 2048):
        with pytest.raises(_lib.AcgError, match="power of two"):
            ops.spectrum_bins(S)


def test_the_header_declares_both_entries_and_the_binding_matches():
    from dtgan_amd import _lib
    for name in ("acg_radial_spectrum_workspace_bytes", "acg_radial_spectrum"):
        assert len(abi.header_args(name)) == len(_lib.SIGNATURES[name][1]), name
