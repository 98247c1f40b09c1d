"""CPU tests of the whole-field spectra's definition (tests/field_spectrum_ref.py), of the Python that needs no device
(ops.field_spectrum_bins, the --metric field_spectrum option) and of the float32 Bluestein restatement behind the GPU test's
tolerance (tools/field_spectrum_bench.py)."""
import os
import sys

import numpy as np
import pytest

import field_spectrum_ref as F
import spectrum_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((17, 17), (18, 30), (31, 16), (20, 28), (1000, 1024))


@pytest.mark.parametrize("S", (16, 32, 256))
def test_square_bins_are_the_square_rule(S):
    assert np.array_equal(F.bin_index(S, S), R.bin_index(S))
    assert np.array_equal(F.bin_counts(S, S), R.bin_counts(S))


def test_square_spectrum_is_the_square_reference():
    x = R.make_fields("tanh_red", 32, rows=2, C=2)
    assert np.array_equal(F.rapsd(x), R.rapsd(x))


@pytest.mark.parametrize("H,W", SHAPES)
def test_integer_rule_is_the_rounded_radius_and_every_bin_is_populated(H, W):
    """The rule puts the boundary between rings b and b + 1 at r^2 = b (b + 1), i.e. at r = sqrt(b (b + 1)), which lies below
    b + 1/2 by less than 1 / (8 b).  Where r^2 is an integer (H = W) no cell falls in between and the rule IS rounding; on
    an ellipse r^2 is rational and a few cells do.  So: the rule equals its own boundary evaluated in floating point wherever
    that is more than 1e-9 from a tie, and equals r rounded to nearest wherever r is further than 1 / (8 r) + 1e-9 below a
    half-integer, which is all but a sliver of the plane."""
    L = min(H, W)
    fy, fx = F.wavenumbers(H).astype(np.float64), F.wavenumbers(W).astype(np.float64)
    r = L * np.sqrt((fy[:, None] / H) ** 2 + (fx[None, :] / W) ** 2)
    b = F.bin_index(H, W)
    edge = 0.5 + np.sqrt(r * r + 0.25)                               # b (b - 1) < r^2  <=>  b < 1/2 + sqrt(r^2 + 1/4)
    clear = np.abs(edge - np.round(edge)) > 1e-9
    assert np.array_equal(b[clear], (np.ceil(edge) - 1).astype(np.int64)[clear]) and (b[~clear] == np.round(edge)[~clear] - 1).all()
    below = np.floor(r) + 0.5 - r                                    # how far r lies below the next half-integer
    plain = (below < -1e-9) | (below > 1.0 / (8.0 * np.maximum(r, 1.0)) + 1e-9)
    assert plain.mean() > 0.9 and np.array_equal(b[plain], np.floor(r + 0.5).astype(np.int64)[plain])
    if H == W:
        away = np.abs(below) > 1e-9
        assert np.array_equal(b[away], np.floor(r + 0.5).astype(np.int64)[away])
    assert b[0, 0] == 0 and (b.ravel()[1:] >= 1).all()
    counts = F.bin_counts(H, W)
    assert counts.shape == (L // 2 + 1,) and counts[0] == 1 and (counts > 0).all()
    # ring b: b cycles per L pixels along either axis
    for k in range(1, L // 2 + 1):
        assert (b[k, 0] if H == L else b[0, k]) == k


@pytest.mark.parametrize("H,W", SHAPES)
def test_bin_map_of_the_transposed_shape_is_the_transpose(H, W):
    assert np.array_equal(F.bin_index(W, H), F.bin_index(H, W).T)
    assert np.array_equal(F.bin_counts(W, H), F.bin_counts(H, W))


def test_ops_bins_agree_with_the_reference():
    from dtgan_amd import _lib, ops
    for H, W in F.SHAPES:
        assert ops.field_spectrum_bins(H, W) == F.bins(H, W) == len(F.bin_counts(H, W))
    for H, W in ((15, 64), (64, 1025), (8, 8)):
        with pytest.raises(_lib.AcgError, match="16..1024"):
            ops.field_spectrum_bins(H, W)


def test_options_accept_the_metric():
    from dtgan_amd.options import TestOptions
    a = TestOptions().parse(["--chk_path", "x/latest", "--dataroot", "d", "--metric", "field_spectrum", "--n_samples", "3",
                             "--overlap", "5"])
    assert (a.metric, a.n_samples, a.overlap) == ("field_spectrum", 3, 5)
    from dtgan_amd import eval_metrics as EM
    assert "field_spectrum" in EM.WHOLE_FIELD_METRICS and "translate" in EM.WHOLE_FIELD_METRICS


def test_cross_reference_of_a_field_with_itself():
    x = F.make_fields("red", 18, 30, rows=1, C=2)
    t = F.cross_spectrum(x, x)
    assert np.allclose(t[..., 0, :], t[..., 2, :], rtol=1e-12) and np.allclose(t[..., 0, :], F.rapsd(x), rtol=1e-12)


@pytest.mark.parametrize("H,W", [s for s in F.SHAPES if s[0] * s[1] <= F.LARGE])
def test_float32_bluestein_restatement_stays_inside_the_gpu_bound(H, W):
    """the yardstick of the GPU tolerance on the shapes that take a moment on the host; the large ones are the tool's"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import field_spectrum_bench as B
    from field_spectrum_ref import CTAU, TAU
    per, cross = B.restated_tolerances(H, W)
    print("%d x %d: tau %s, cxy %.3e" % (H, W, {k: "%.3e" % v for k, v in per.items()}, cross))
    assert max(per.values()) <= TAU / 4 and cross <= CTAU / 4
    # the restatement is a transform: against numpy's on a field of every parity
    x = F.make_fields("white", H, W, rows=1, C=1)
    got = B.fft2_f32(x).numpy()
    want = np.fft.fft2(x.astype(np.float64))
    assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max()
