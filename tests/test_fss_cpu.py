"""CPU tests of the fractions skill score: the numpy reference (tests/fss_ref.py) against brute-force window loops and the
float definition, ops.fss_summary, the option parsers, the header and the host-side refusals of ops.fss."""
import numpy as np
import pytest
import torch

import abi
import fss_ref as F
from eval_cases import parse_test

LISTED = (1, 3, 5, 9, 17, 33)


@pytest.mark.parametrize("H,W", ((5, 7), (16, 16), (33, 31)))
def test_the_summed_area_reference_equals_window_loops(H, W):
    b = (np.random.RandomState(H).uniform(size=(H, W)) < 0.3).astype(np.int64)
    e = np.random.RandomState(W).randint(0, 17, (H, W)).astype(np.int64)     # an exceedance-count plane of 16 members
    for n in (1, 3, 5, 9, 33, 65):
        assert np.array_equal(F.box_counts(b, n), F.box_counts_brute(b, n)), n
        assert np.array_equal(F.box_counts(e, n), F.box_counts_brute(e, n)), n
    assert np.array_equal(F.box_counts(b, 1), b)
    assert np.all(F.box_counts(b, 2 * max(H, W) - 1) == b.sum())


def test_the_integer_form_equals_the_float_definition():
    x, y, _ = F.make_pair("shifted", 33, 31, rows=1, C=1)
    x, y = x[0, 0], y[0, 0]
    thr = np.array([[0.5]], dtype=np.float32)
    t = F.triples(x[None, None], y[None, None], thr, LISTED)[0, 0, 0]
    got = F.summary(t, LISTED, x.size)["fss"]
    for k, n in enumerate(LISTED):
        want = F.fss_float(x, y, np.float32(0.5), n)
        assert abs(got[k] - want) <= 1e-12 * abs(want), (n, got[k], want)


def test_identical_fields_score_one_and_distant_events_zero():
    x, _, thr = F.make_pair("noise", 16, 16, rows=2, C=3)
    t = F.triples(x, x, thr, LISTED).sum(0)
    s = F.summary(t, LISTED, 2 * 256)
    assert np.all(s["fss"][:, 0] == 1.0) and np.all(s["fss"][:, 2] == 1.0)          # exactly
    assert np.all(np.isnan(s["fss"][:, 1]))                                           # the threshold nothing exceeds
    assert np.all(s["bias"][:, 0] == 1.0) and np.all(s["csi"][:, 0] == 1.0)
    a, b = np.zeros((1, 1, 33, 31), np.float32), np.zeros((1, 1, 33, 31), np.float32)
    a[0, 0, 2, 3], b[0, 0, 20, 25] = 1, 1                                             # 18 rows and 22 columns apart
    t = F.triples(a, b, np.array([[0.5]], np.float32), (1, 3, 9, 17))[0, 0, 0]
    assert np.all(t[:, 2] == 0) and np.all(F.summary(t, (1, 3, 9, 17), 33 * 31)["fss"] == 0.0)
    assert F.triples(a, b, np.array([[0.5]], np.float32), (37,))[0, 0, 0, 0, 2] > 0   # a window that reaches both


def test_the_shifted_pair_gains_skill_with_the_window():
    x, y, thr = F.make_pair("shifted", 64, 64, rows=2, C=3)
    s = F.summary(F.triples(x, y, thr, LISTED).sum(0), LISTED, 2 * 64 * 64)
    fss = s["fss"][:, 0]
    assert np.all(np.diff(fss, axis=-1) >= 0), fss
    assert np.all(fss[:, 0] < 0.5) and np.all(fss[:, -1] > 0.9), fss                  # displaced by (2, 3): no skill per cell
    assert np.all((s["useful_scale"][:, 0] >= 3) & (s["useful_scale"][:, 0] <= 17)), s["useful_scale"]
    assert np.allclose(s["bias"][:, 0], 1.0)                                          # a periodic shift keeps every event


def test_all_ones_factorises_and_reaches_two_to_the_sixty():
    for H, W, n in ((5, 7, 3), (33, 31, 9), (16, 16, 65)):
        ri = np.minimum(np.arange(H) + n // 2, H - 1) - np.maximum(np.arange(H) - n // 2, 0) + 1
        rj = np.minimum(np.arange(W) + n // 2, W - 1) - np.maximum(np.arange(W) - n // 2, 0) + 1
        c = F.box_counts(np.ones((H, W), np.int64), n)
        assert int((c * c).sum()) == int((ri ** 2).sum()) * int((rj ** 2).sum())
    r = np.full(1024, 1024, dtype=np.int64)                                           # the whole domain from every cell
    assert int((r ** 2).sum()) ** 2 == 1 << 60


def test_fss_summary():
    from dtgan_amd import ops
    x, y, thr = F.make_pair("noise", 33, 31, rows=4, C=2)
    win = (3, 1, 9)                                                                   # 1 need not come first
    t = F.triples(x, y, thr, win).sum(0)
    got, ref = ops.fss_summary(t, win, 4 * 33 * 31), F.summary(t, win, 4 * 33 * 31)
    assert set(got) == {"fss", "bias", "csi", "base_rate", "useful_scale"}
    for k in ref:
        assert got[k].shape == ref[k].shape and np.allclose(got[k], ref[k], rtol=1e-12, equal_nan=True), k
    assert got["fss"].shape == (2, 3, 3) and got["bias"].shape == (2, 3) and got["useful_scale"].dtype == np.int64
    assert np.all(np.isnan(got["fss"][:, 1])) and np.all(np.isnan(got["bias"][:, 1])) and np.all(np.isnan(got["csi"][:, 1]))
    assert np.all(got["base_rate"][:, 1] == 0) and np.all(got["useful_scale"][:, 1] == 0)
    assert np.all(got["fss"][:, 2] == 1.0) and np.all(got["base_rate"][:, 2] == 1.0)  # everything exceeds: 1 >= 0.5 + 1/2
    assert np.all(got["useful_scale"][:, 2] == 1)
    assert set(ops.fss_summary(t[..., 1:, :], (3, 9), 1)) == {"fss"}                  # without the window 1
    # by hand: one threshold, windows (1, 3); forecast 4 events, observed 2, 1 hit, 100 cells
    hand = np.array([[[4, 2, 1], [30, 20, 22]]], dtype=np.int64)
    s = ops.fss_summary(hand, (1, 3), 100)
    assert np.allclose(s["fss"], [[2 / 6, 44 / 50]]) and np.allclose(s["bias"], [2.0]) and np.allclose(s["csi"], [0.2])
    assert np.allclose(s["base_rate"], [0.02]) and np.array_equal(s["useful_scale"], [3])     # 0.88 >= 0.51 > 1/3
    # M members: the ensemble triples of M copies of one member are (M^2 ff, oo, M fo) and score as the member does
    M = 4
    ens = t * np.array([M * M, 1, M], dtype=np.int64)
    sm = ops.fss_summary(ens, win, 4 * 33 * 31, members=M)
    assert np.allclose(sm["fss"], got["fss"], rtol=1e-12, equal_nan=True) and np.allclose(sm["csi"][:, 0], F.summary(ens, win, 1, M)["csi"][:, 0])
    assert np.allclose(sm["bias"], M * got["bias"], equal_nan=True)                   # sum e^2 / M, e = M on an event
    with pytest.raises(ValueError, match="triples"):
        ops.fss_summary(np.zeros((2, 3, 2)), win, 1)
    with pytest.raises(ValueError, match="odd"):
        ops.fss_summary(t, (1, 2, 9), 1)


def _parse(*extra):
    return parse_test("fss", *extra)


def test_the_fss_options():
    o = _parse()
    assert o.metric == "fss" and o.n_samples == 16 and o.fss_quantiles == (0.5, 0.9, 0.99) and o.fss_thresholds is None
    assert o.fss_windows == (1, 3, 5, 9, 17, 33)
    o = _parse("--fss_windows", "9,3,3,17", "--fss_thresholds", "0.5,-1", "--fss_quantiles", "0.25", "--n_samples", "4")
    assert o.fss_windows == (1, 3, 9, 17) and o.fss_thresholds == (0.5, -1.0) and o.fss_quantiles == (0.25,) and o.n_samples == 4
    assert _parse("--fss_windows", "1,3,5,7,9,11,13,15").fss_windows == (1, 3, 5, 7, 9, 11, 13, 15)
    for bad in (("--fss_windows", "2,3"), ("--fss_windows", "0"), ("--fss_windows", "3,5,7,9,11,13,15,17"), ("--fss_windows", "a"),
                ("--fss_quantiles", "1.5"), ("--fss_quantiles", ""), ("--fss_thresholds", "1,2,3,4,5,6,7,8,9"), ("--fss_thresholds", "nan")):
        with pytest.raises(SystemExit):
            _parse(*bad)
    for metric in ("coherence", "mse"):                                               # the others keep parsing
        from dtgan_amd import options as O
        assert O.TestOptions().parse(["--chk_path", "c", "--dataroot", "d", "--metric", metric]).metric == metric


def test_thresholds_are_float64_quantiles_per_channel():
    from dtgan_amd import eval_metrics as EM
    train = np.random.RandomState(1).uniform(0, 3, (6, 2, 8, 8)).astype(np.float32)
    thr = EM.fss_thresholds(train, (0.5, 0.9))
    want = np.stack([np.quantile(train[:, c].astype(np.float64), [0.5, 0.9]) for c in range(2)]).astype(np.float32)
    assert thr.dtype == np.float32 and thr.shape == (2, 2) and np.array_equal(thr, want)
    assert np.array_equal(EM.fss_thresholds(train, (0.5,), (1.0, 2.5)), np.array([[1.0, 2.5], [1.0, 2.5]], np.float32))


def test_the_header_declares_both_entries_and_the_binding_matches():
    from dtgan_amd import _lib
    for name in ("acg_fss_workspace_bytes", "acg_fss"):
        assert len(abi.header_args(name)) == len(_lib.SIGNATURES[name][1]), name
    assert len(_lib.SIGNATURES["acg_fss"][1]) == 22
    lib = _lib.load()
    # per plane and image row ceil(W / 64) words and one more 16-bit prefix; x's planes, then y's, then for an
    # ensemble of M > 1 bit_width(M) slices per truth plane
    assert lib.acg_fss_workspace_bytes(4, 2, 3, 64, 64, 3, 6, 1) == (36 + 18 + 18 * 2) * 64 * (8 + 4)
    assert lib.acg_fss_workspace_bytes(4, 2, 3, 64, 64, 3, 6, 0) == (36 + 18) * 64 * (8 + 4)
    assert lib.acg_fss_workspace_bytes(1, 1, 1, 321, 321, 1, 1, 0) == 2 * (321 * 6 * 8 + 321 * 7 * 2 + 2)     # rounded to 16
    assert lib.acg_fss_workspace_bytes(3, 2, 1, 64, 64, 1, 1, 0) == 0 and lib.acg_fss_workspace_bytes(1, 1, 1, 1025, 4, 1, 1, 0) == 0


def test_ops_refuses_on_the_host_before_any_device_call(monkeypatch):
    from dtgan_amd import _lib, ops

    def no_device(*a, **k):
        raise AssertionError("a refusal reached the library")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(_lib, "query", no_device)
    z = lambda *shape: torch.zeros(shape)
    thr, win = np.zeros((1, 2), np.float32), (1, 3)
    with pytest.raises(_lib.AcgError, match="layout"):
        ops.fss(z(1, 1, 32, 32), z(1, 1, 32, 32), 1, "nchw", "chwn", thr, win)
    with pytest.raises(_lib.AcgError, match="1024"):
        ops.fss(z(1, 1, 4, 1025), z(1, 1, 4, 1025), 1, "nchw", "nchw", thr, win)
    with pytest.raises(_lib.AcgError, match="channels"):
        ops.fss(z(2, 8, 8, 4), z(2, 2, 8, 8), 3, "nhwc", "nchw", np.zeros((3, 1), np.float32), win)
    for bad in (0, -1, 4, 65):
        with pytest.raises(_lib.AcgError, match="x_per_y"):
            ops.fss(z(6, 1, 8, 8), z(6, 1, 8, 8), 1, "nchw", "nchw", thr, win, x_per_y=bad)
    with pytest.raises(_lib.AcgError, match="do not pair"):
        ops.fss(z(2, 1, 8, 8), z(2, 1, 8, 12), 1, "nchw", "nchw", thr, win)
    with pytest.raises(_lib.AcgError, match="do not pair"):
        ops.fss(z(6, 8, 8, 4), z(3, 3, 8, 8), 3, "nhwc", "nchw", np.zeros((3, 1), np.float32), win, x_per_y=3)
    for bad in ((2,), (1, 4), (), (-3,), tuple(range(1, 19, 2)), (3.5,)):
        with pytest.raises(_lib.AcgError, match="windows"):
            ops.fss(z(2, 1, 8, 8), z(2, 1, 8, 8), 1, "nchw", "nchw", thr, bad)
    for bad in (np.zeros((2, 2), np.float32), np.zeros(2, np.float32), np.zeros((1, 9), np.float32), np.zeros((1, 0), np.float32)):
        with pytest.raises(_lib.AcgError, match="thresholds"):
            ops.fss(z(2, 1, 8, 8), z(2, 1, 8, 8), 1, "nchw", "nchw", bad, win)
    with pytest.raises(_lib.AcgError, match="out"):
        ops.fss(z(2, 1, 8, 8), z(2, 1, 8, 8), 1, "nchw", "nchw", thr, win, out=torch.zeros(2, 1, 2, 2, 3))           # not int64
    with pytest.raises(_lib.AcgError, match="ens"):
        ops.fss(z(4, 1, 8, 8), z(2, 1, 8, 8), 1, "nchw", "nchw", thr, win, x_per_y=2, ensemble=True,
                out=(torch.zeros(4, 1, 2, 2, 3, dtype=torch.int64), torch.zeros(4, 1, 2, 2, 3, dtype=torch.int64)))
    with pytest.raises(_lib.AcgError, match="ROCm device"):                                   # and a valid call has no CPU path
        ops.fss(z(2, 1, 8, 8), z(2, 1, 8, 8), 1, "nchw", "nchw", thr, win)
    with pytest.raises(ValueError, match="odd"):
        ops.check_windows((1, 2))
