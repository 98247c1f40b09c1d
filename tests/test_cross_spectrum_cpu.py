"""CPU tests of the paired cross-spectra: the reference (tests/cross_spectrum_ref.py) against its own identities,
ops.coherence_summary on hand-made triples, the evaluator's coherence option, the host-side refusals of ops.cross_spectrum and
the two entry points' declarations."""
import numpy as np
import pytest
import torch

import abi
import dtgan_amd  # noqa: F401
from dtgan_amd import options as O
import cross_spectrum_ref as X
import spectrum_ref as R

SIZES = (16, 64)


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("kind", X.PAIR_KINDS)
def test_the_reference_obeys_its_identities(kind, S):
    x, y = X.make_pairs(kind, S, rows=2, C=2)
    assert x.shape == y.shape == (2, 2, S, S) and x.dtype == y.dtype == np.float32
    t = X.cross_spectrum(x, y)
    assert t.shape == (2, 2, 3, S // 2 + 1) and t.dtype == np.float64
    pxx, pyy, cxy = t[..., 0, :], t[..., 1, :], t[..., 2, :]
    scale = np.sqrt(pxx * pyy).max()
    # the quadrature part vanishes ring by ring: why it is no output
    assert np.all(np.abs(X.quadrature(x, y)) <= 1e-12 * scale)
    # pxx and pyy are each field's own spectrum
    assert np.allclose(pxx, R.rapsd(x), rtol=1e-13, atol=0) and np.allclose(pyy, R.rapsd(y), rtol=1e-13, atol=0)
    # polarisation: Cxy = (P(x + y) - P(x - y)) / 4, the sum and the difference formed in float64
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    pol = (R.bin_power(R.power_plane(xd + yd)) - R.bin_power(R.power_plane(xd - yd))) / 4.0
    assert np.all(np.abs(cxy - pol) <= 1e-12 * scale)
    # Cauchy-Schwarz over a ring
    assert np.all(cxy * cxy <= pxx * pyy * (1 + 1e-12) + 1e-300)
    # Parseval for the error spectrum, the dropped corners added back
    perr = X.summary(t)["perr"]
    assert np.all(np.abs(perr - R.rapsd(xd - yd)) <= 1e-12 * (pxx + pyy).max())
    corner = R.power_plane(xd - yd)[..., R.bin_index(S) > S // 2].sum(-1)
    total = (perr * R.bin_counts(S)).sum(-1) + corner
    assert np.allclose(total, S * S * np.mean((xd - yd) ** 2, axis=(-2, -1)), rtol=1e-10, atol=1e-12 * S * S)


def test_the_nyquist_pair_loads_the_packed_columns_and_the_dc_pair_bin_0():
    S = 32
    x, y = X.make_pairs("nyquist", S, rows=1, C=1)
    _, _, cxy, _ = X.planes(x[0, 0], y[0, 0])
    assert np.allclose(cxy[0, S // 2], 0.5 * S * S)                                  # (-1)^w against 0.5 (-1)^w: kx = S/2, ky = 0
    assert np.allclose(cxy[3, 0], 0.25 * 0.5 * 0.25 * np.cos(1.0) * S * S)           # the two cosines along h: kx = 0, ky = 3
    t = X.cross_spectrum(x, y)[0, 0]
    assert t[2, S // 2] > 0 and t[2, 3] > 0 and t[1, S // 2] > t[0, S // 2]          # (-1)^h lies in ring S/2 as well
    x, y = X.make_pairs("dc", S, rows=1, C=1)
    t = X.cross_spectrum(x, y)[0, 0]
    assert t[2, 0] < 0 and np.allclose(t[2, 0], -np.sqrt(t[0, 0] * t[1, 0]), rtol=1e-12)   # means 0.7 and -0.4


def _summary(t):
    from dtgan_amd import ops
    return ops.coherence_summary(t)


def test_coherence_summary_on_hand_made_triples():
    nb = 9
    rs = np.random.RandomState(0)
    p = rs.uniform(0.5, 2, nb)
    s = _summary(np.stack([p, p, p]))                              # same
    assert np.all(s["coh"] == 1) and np.all(s["r"] == 1) and np.all(s["perr"] == 0) and s["k_eff"] == nb
    assert s["coh"].dtype == s["r"].dtype == s["perr"].dtype == np.float64 and s["k_eff"].dtype == np.int64
    s = _summary(np.stack([p, p, -p]))                             # neg
    assert np.all(s["coh"] == 1) and np.all(s["r"] == -1) and np.allclose(s["perr"], 4 * p) and s["k_eff"] == nb
    q = rs.uniform(0.5, 2, nb)
    r = np.array([1, .9, .8, .75, .7, .72, .3, .9, .1])            # coh = r^2 first falls below 0.5 at bin 4 (0.49)
    t = np.stack([p, q, r * np.sqrt(p * q)])
    s = _summary(t)
    assert np.allclose(s["r"], r) and np.allclose(s["coh"], r * r) and s["k_eff"] == 4
    assert np.allclose(s["perr"], p + q - 2 * t[2])
    low0 = t.copy()
    low0[2, 0] = 0                                                 # bin 0 takes no part in k_eff
    assert _summary(low0)["k_eff"] == 4
    zero = t.copy()
    zero[1, 2] = 0                                                 # a zero denominator: 0, not NaN, and the first bin below 0.5
    zero[2, 2] = 0
    s = _summary(zero)
    assert s["coh"][2] == 0 and s["r"][2] == 0 and np.all(np.isfinite(s["coh"])) and np.all(np.isfinite(s["r"])) and s["k_eff"] == 2
    s = _summary(np.zeros((3, nb)))
    assert np.all(s["coh"] == 0) and np.all(s["r"] == 0) and s["k_eff"] == 1
    # leading axes, and the sums of pairs rather than the pairs: independent fields pool towards 0
    many = _summary(np.stack([t, np.stack([p, p, p])]))
    assert many["coh"].shape == (2, nb) and np.array_equal(many["k_eff"], [4, nb])
    with pytest.raises(ValueError, match="triples"):
        _summary(np.zeros((4, nb)))


@pytest.mark.parametrize("kind", X.PAIR_KINDS)
def test_coherence_summary_equals_the_reference(kind):
    x, y = X.make_pairs(kind, 32, rows=4, C=2)
    sums = X.cross_spectrum(x, y).sum(0)
    got, ref = _summary(sums), X.summary(sums)
    for k in ("coh", "r", "perr"):
        assert np.allclose(got[k], ref[k], rtol=1e-12, atol=1e-15), k
    assert np.array_equal(got["k_eff"], ref["k_eff"])
    assert np.all((got["coh"] >= 0) & (got["coh"] <= 1)) and np.all(np.abs(got["r"]) <= 1)
    assert np.all((got["k_eff"] >= 1) & (got["k_eff"] <= 17))


def test_pooling_pairs_is_what_tames_the_low_bins():
    """one independent pair reaches a sizeable ring-wise coherence where a ring has few cells; the pooled sums do not"""
    S, n = 32, 64
    rs = np.random.RandomState(4)
    x, y = rs.standard_normal((n, S, S)).astype(np.float32), rs.standard_normal((n, S, S)).astype(np.float32)
    t = X.cross_spectrum(x, y)
    single = X.summary(t)["coh"][:, 1:4].max()
    pooled = X.summary(t.sum(0))["coh"][1:4].max()
    assert single > 0.3 and pooled < 0.1, (single, pooled)


def test_the_coherence_metric_parses_and_fid_does_not():
    o = O.TestOptions().parse(["--chk_path", "c", "--dataroot", "d", "--metric", "coherence"])
    assert o.metric == "coherence" and o.n_samples == 16
    o = O.TestOptions().parse(["--chk_path", "c", "--dataroot", "d", "--metric", "coherence", "--n_samples", "4"])
    assert o.n_samples == 4
    with pytest.raises(SystemExit):
        O.TestOptions().parse(["--chk_path", "c", "--dataroot", "d", "--metric", "fid"])


def test_ops_refuses_on_the_host_before_any_device_call(monkeypatch):
    from dtgan_amd import _lib, ops

    def no_device(*a, **k):
        raise AssertionError("a refusal reached the library")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(_lib, "query", no_device)
    z = lambda *shape: torch.zeros(shape)
    for S in (192, 8, 2048):
        with pytest.raises(_lib.AcgError, match="power of two"):
            ops.cross_spectrum(z(1, 1, S, S), z(1, 1, S, S), 1, "nchw", "nchw")
    with pytest.raises(_lib.AcgError, match="power of two"):
        ops.cross_spectrum(z(1, 1, 64, 32), z(1, 1, 64, 32), 1, "nchw", "nchw")              # not square
    with pytest.raises(_lib.AcgError, match="power of two"):
        ops.cross_spectrum(z(1, 32, 32, 4), z(1, 3, 32, 48), 3, "nhwc", "nchw")              # y not square
    with pytest.raises(_lib.AcgError, match="do not pair"):
        ops.cross_spectrum(z(2, 1, 32, 32), z(2, 1, 64, 64), 1, "nchw", "nchw")              # sizes differ
    with pytest.raises(_lib.AcgError, match="do not pair"):
        ops.cross_spectrum(z(4, 1, 32, 32), z(3, 1, 32, 32), 1, "nchw", "nchw")              # rows differ
    with pytest.raises(_lib.AcgError, match="do not pair"):
        ops.cross_spectrum(z(6, 32, 32, 4), z(3, 3, 32, 32), 3, "nhwc", "nchw", x_per_y=3)   # 6 members need 2 truths
    with pytest.raises(_lib.AcgError, match="channels"):
        ops.cross_spectrum(z(2, 32, 32, 4), z(2, 2, 32, 32), 3, "nhwc", "nchw")              # y lacks the third channel
    for bad in (0, -1, 4):
        with pytest.raises(_lib.AcgError, match="x_per_y"):
            ops.cross_spectrum(z(6, 1, 32, 32), z(6, 1, 32, 32), 1, "nchw", "nchw", x_per_y=bad)
    with pytest.raises(_lib.AcgError, match="layout"):
        ops.cross_spectrum(z(1, 1, 32, 32), z(1, 1, 32, 32), 1, "nchw", "chwn")
    with pytest.raises(_lib.AcgError, match="out"):
        ops.cross_spectrum(z(2, 1, 32, 32), z(2, 1, 32, 32), 1, "nchw", "nchw", out=z(2, 1, 17))
    with pytest.raises(_lib.AcgError, match="ROCm device"):                                   # and a valid call has no CPU path
        ops.cross_spectrum(z(2, 1, 32, 32), z(2, 1, 32, 32), 1, "nchw", "nchw")


def test_the_header_declares_both_entries_and_the_binding_matches():
    from dtgan_amd import _lib
    for name in ("acg_cross_spectrum_workspace_bytes", "acg_cross_spectrum"):
        assert len(abi.header_args(name)) == len(_lib.SIGNATURES[name][1]), name
    lib = _lib.load()
    assert lib.acg_cross_spectrum_workspace_bytes(3, 3, 64) == 0                     # one workgroup per pair up to 64
    assert lib.acg_cross_spectrum_workspace_bytes(3, 3, 128) == 9 * 128 * 128 * 8    # two half spectra per pair above
    assert lib.acg_cross_spectrum_workspace_bytes(1, 1, 192) == 0
