"""CPU tests of the SAL score: the reference (tests/sal_ref.py) against closed forms, its integers against
tests/components_ref.py and additivity, the fixed-point mass, ops.sal_scores against the reference's plain loops with its
broadcasting and refusals, the option parser (--fss_sal and its four options), the header and the host-side refusals of ops.sal."""
import math
import os

import numpy as np
import pytest
import torch

import abi
import components_ref as R
import minkowski_ref as K
import sal_ref as S
from eval_cases import parse_test

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO = np.zeros((1, 1), np.float32)
H, W = 33, 65


def _gauss(H, W, cy, cx, sigma, peak, base=-1.0):
    y, x = np.mgrid[0:H, 0:W]
    return (base + (peak - base) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2.0 * sigma ** 2))).astype(np.float32)[None]


def test_a_displaced_block_moves_the_centre_and_nothing_else():
    a, b = S.block(H, W, 5, 10, 6, 9, 0.5), S.block(H, W, 9, 30, 6, 9, 0.5)
    for conn in (4, 8):
        s = S.pair_scores(b, a, ZERO, conn)
        assert s["S"].item() == 0 and s["A"].item() == 0 and s["L2"].item() == 0
        assert s["L1"].item() == s["L"].item() == math.sqrt(4 ** 2 + 20 ** 2) / math.sqrt(32 ** 2 + 64 ** 2)
        assert abs(s["L1"].item() - math.hypot(4, 20) / math.hypot(32, 64)) < 1e-15


def test_a_taller_block_has_more_amplitude_and_the_same_structure():
    a = S.block(H, W, 5, 10, 6, 9, 0.5)                              # 1.5 above the floor
    b = S.block(H, W, 5, 10, 6, 9, 1.0)                              # 2.0 above it: 4 / 3 of the height
    s = S.pair_scores(b, a, ZERO)
    assert s["S"].item() == 0 and s["L"].item() == 0 and s["A"].item() == (2.0 - 1.5) / (0.5 * (2.0 + 1.5)) == 2.0 / 7.0


def test_a_plateau_against_a_peak_of_the_same_mass_is_too_flat():
    thr = np.full((1, 1), -0.5, np.float32)
    peak = _gauss(H, W, 16, 32, 4.0, 2.0)                            # 3 above the floor at its top: a mass of about 3 * 2 pi 16 = 301
    flat = S.block(H, W, 10, 20, 13, 25, -0.1)                       # 0.9 above the floor on 325 cells: 292.5
    s = S.pair_scores(flat, peak, thr)
    assert abs(s["A"].item()) < 0.1                                  # comparable mass
    assert s["S"].item() > 1.0 and s["L"].item() == 0.0              # mass over peak: 325 cells against about 95
    assert S.pair_scores(peak, flat, thr)["S"].item() == -s["S"].item()


def test_identical_fields_score_zero():
    thr = K.make_thresholds(2, 3, seed=1)
    x = K.make_fields("smooth", 1, 2, 40, 50, thr, seed=2)[0]
    s = S.pair_scores(x, x, thr)
    for k in ("S", "A", "L1", "L2", "L"):
        ok = ~np.isnan(s[k])
        assert ok.any() and np.all(s[k][ok] == 0), k


def test_the_empty_set_and_the_all_nan_field_follow_the_nan_rules():
    x = S.block(H, W, 5, 10, 6, 9, 0.5)
    thr = np.array([[0.0, 2.0]], np.float32)                         # nothing reaches 2
    f, o, sh = S.sal(x[None], thr, 8)
    assert o[0, 0, 1].tolist() == [0, 0, 0, 0] and sh[0, 0, 1].tolist() == [0.0, 0.0] and f[0, 0, 0] > 0
    s = S.pair_scores(x, x, thr)
    assert s["S"][0, 0] == 0 and np.isnan(s["S"][0, 1]) and np.isnan(s["L2"][0, 1]) and np.isnan(s["L"][0, 1])
    assert s["A"].item() == 0 and s["L1"].item() == 0
    nan = np.full((1, H, W), np.nan, np.float32)
    f, o, sh = S.sal(nan[None], thr, 8)
    assert not f.any() and not o.any() and not sh.any()
    s = S.pair_scores(nan, nan, thr)
    assert all(np.all(np.isnan(v)) for v in s.values())
    s = S.pair_scores(x, nan, thr)                                    # one side without mass: A = 2, no place, no objects
    assert s["A"].item() == 2.0 and np.isnan(s["L1"]).all() and np.isnan(s["S"]).all() and np.isnan(s["L"]).all()
    one = S.scores_one(*(2 * [tuple(a[0] for a in S.sal(np.ones((1, 1, 1, 1), np.float32), ZERO, 8))]), 1, 1)
    assert one["L1"].item() == 0 and one["L2"].item() == 0 and one["S"].item() == 0        # d = 0


def test_a_component_at_the_floor_is_counted_and_weighs_nothing():
    x = np.full((1, 1, 9, 12), -2.0, np.float32)
    x[0, 0, 1:3, 1:4] = -1.0                                         # on the floor and on the threshold: inside, no mass
    x[0, 0, 5:8, 6:10] = 0.0
    thr = np.full((1, 1), -1.0, np.float32)
    f, o, sh = S.sal(x, thr, 8)
    q1 = 1 << 20
    assert o[0, 0, 0].tolist() == [2, 6 + 12, 12 * q1, 12 * q1] and f[0, 0, 0] == 12 * q1
    assert sh[0, 0, 0, 0] == float(12 * q1) * 12.0 and sh[0, 0, 0, 1] == 0.0      # the one object is the field's mass: at its centre
    assert f[0, 0].tolist() == [12 * q1, q1 * 4 * (5 + 6 + 7), q1 * 3 * (6 + 7 + 8 + 9)]


@pytest.mark.parametrize("kind", ("special", "smooth", "perc59", "corners"))
def test_the_integers_are_the_components_and_add_over_halves(kind):
    Hh, Ww = 70, 131
    thr = S.make_thresholds(kind, 2, 4, seed=3)
    x = S.make_fields(kind, 2, 2, Hh, Ww, thr, seed=5)
    for conn in (4, 8):
        f, o, sh = S.sal(x, thr, conn)
        assert f.dtype == o.dtype == np.int64 and sh.dtype == np.float64
        assert np.array_equal(o[..., :2], R.stats(x, thr, conn)[..., :2])
        assert np.all(o[..., 3] <= o[..., 2]) and np.all(o[..., 2] <= f[..., None, 0]) and np.all(sh >= 0)
        # a column outside every set parts the field into disconnected halves: the integers add, the largest object is either's
        cut = x.copy()
        cut[..., 64] = np.nan
        left, right = cut.copy(), cut.copy()
        left[..., 64:], right[..., :64] = np.nan, np.nan
        (fc, oc, _), (fl, ol, _), (fr, orr, _) = (S.sal(v, thr, conn) for v in (cut, left, right))
        assert np.array_equal(fc, fl + fr) and np.array_equal(oc[..., :3], ol[..., :3] + orr[..., :3])
        assert np.array_equal(oc[..., 3], np.maximum(ol[..., 3], orr[..., 3]))


def test_quant_rounds_to_even_clamps_and_takes_the_special_values():
    u = 2.0 ** -20
    x = np.array([-1.0, -1.0 + 0.5 * u, -1.0 + 1.5 * u, -1.0 + 2.5 * u, -1.0 + 0.75 * u, -3.0, 15.0, 15.5, 3e38, np.nan, np.inf, -np.inf,
                  -1.0 - u], np.float32)
    assert S.quant(x).tolist() == [0, 0, 2, 2, 1, 0, 1 << 24, 1 << 24, 1 << 24, 0, 1 << 24, 0, 0]
    assert S.quant(np.float32([0.5, 1.0]), floor=0.0).tolist() == [1 << 19, 1 << 20] and S.quant(x).dtype == np.int64
    assert S.quant(np.float32([3e38]), floor=-3e38).tolist() == [1 << 24]       # the difference overflows: clamped
    big = np.full((1024, 1024), 15.0, np.float32)                    # the largest field, every cell saturated
    Q, QY, QX = S.field_sums(S.quant(big)).tolist()
    assert Q == 1 << 44 and QY == QX == (1 << 24) * 1024 * (1023 * 1024 // 2) < 1 << 54


def test_scores_broadcast_members_against_truth():
    from dtgan_amd import ops
    thr = K.make_thresholds(2, 3, seed=7)
    N, M, Hh, Ww = 3, 4, 24, 31
    xm = K.make_fields("smooth", N * M, 2, Hh, Ww, thr, seed=1)
    xo = K.make_fields("smooth", N, 2, Hh, Ww, thr, seed=2)
    xo[0, 1] = np.nan                                                # a truth without mass
    xm[5, 0] = -2.0                                                  # a member without mass
    f = tuple(a.reshape((N, M) + a.shape[1:]) for a in S.sal(xm, thr, 8))
    o = S.sal(xo, thr, 8)
    got = ops.sal_scores(f, tuple(a[:, None] for a in o), Hh, Ww)
    assert {k: v.shape for k, v in got.items()} == dict(S=(N, M, 2, 3), A=(N, M, 2), L1=(N, M, 2), L2=(N, M, 2, 3), L=(N, M, 2, 3))
    assert all(v.dtype == np.float64 for v in got.values())
    for n in range(N):
        for m in range(M):
            want = S.scores_one(tuple(a[n, m] for a in f), tuple(a[n] for a in o), Hh, Ww)
            for k in want:
                assert np.allclose(got[k][n, m], want[k], rtol=1e-14, atol=1e-15, equal_nan=True), (k, n, m)
                assert np.array_equal(np.isnan(got[k][n, m]), np.isnan(want[k])), (k, n, m)
    assert np.isnan(got["S"][0, :, 1]).all() and np.isnan(got["L1"][0, :, 1]).all() and np.all(got["A"][0, :, 1] == 2.0)
    assert np.isnan(got["S"][1, 1, 0]).all() and got["A"][1, 1, 0] == -2.0
    ok = ~np.isnan(got["S"])
    assert np.all(np.abs(got["S"][ok]) <= 2) and np.all(np.abs(got["A"][~np.isnan(got["A"])]) <= 2)
    assert np.all(got["L"][~np.isnan(got["L"])] >= 0) and np.all(got["L"][~np.isnan(got["L"])] <= 2)
    same = ops.sal_scores(o, o, Hh, Ww)                              # per-input triples against themselves
    assert same["S"].shape == (N, 2, 3) and np.all(same["A"][~np.isnan(same["A"])] == 0) and np.all(same["L"][~np.isnan(same["L"])] == 0)


def test_scores_refuse_mismatched_shapes():
    from dtgan_amd import ops
    z = lambda *s: np.zeros(s)
    good = (z(2, 3, 3), z(2, 3, 5, 4), z(2, 3, 5, 2))
    assert ops.sal_scores(good, good, 8, 8)["L"].shape == (2, 3, 5)
    bad = ((z(2, 3, 2), z(2, 3, 5, 4), z(2, 3, 5, 2)), (z(2, 3, 3), z(2, 3, 5, 3), z(2, 3, 5, 2)), (z(2, 3, 3), z(2, 3, 5, 4), z(2, 3, 5, 3)),
           (z(2, 3, 3), z(2, 4, 5, 4), z(2, 4, 5, 2)), (z(2, 3, 3), z(2, 3, 5, 4), z(2, 3, 6, 2)), (z(3), z(5, 4), z(5, 2)),
           (z(2, 3, 3), z(2, 3, 5, 4)), None)
    for b in bad:
        with pytest.raises(ValueError, match="sal_scores"):
            ops.sal_scores(b, good, 8, 8)
        with pytest.raises(ValueError, match="sal_scores"):
            ops.sal_scores(good, b, 8, 8)
    for other in ((z(3, 3, 3), z(3, 3, 5, 4), z(3, 3, 5, 2)), (z(2, 3, 3), z(2, 3, 6, 4), z(2, 3, 6, 2)), (z(2, 2, 3), z(2, 2, 5, 4), z(2, 2, 5, 2))):
        with pytest.raises(ValueError, match="broadcast"):
            ops.sal_scores(good, other, 8, 8)
    for hw in ((0, 8), (8, 0)):
        with pytest.raises(ValueError, match="H x W"):
            ops.sal_scores(good, good, *hw)


def _parse(*extra):
    return parse_test("fss", *extra)


def test_the_parser_takes_the_switch_and_the_four_options():
    """SAL is an option of its partner fss: the table of metrics and the parser's choices are what they were"""
    from dtgan_amd import eval_metrics as EM, options as O
    o = _parse()
    assert o.fss_sal == 0 and o.sal_quantiles == (0.9,) and o.sal_thresholds is None and o.sal_floor == -1.0 and o.sal_conn == 8
    assert _parse("--fss_sal", "1").fss_sal == 1 and _parse("--fss_sal", "0", "--fss_scales", "1").fss_sal == 0
    assert _parse("--sal_quantiles", "0.99,0.5,0.9").sal_quantiles == (0.5, 0.9, 0.99)
    assert _parse("--sal_thresholds", "0.5,-0.25").sal_thresholds == (-0.25, 0.5)
    assert _parse("--sal_floor", "0").sal_floor == 0.0 and _parse("--sal_floor", "-2.5").sal_floor == -2.5
    assert _parse("--sal_conn", "4").sal_conn == 4 and _parse("--fss_sal", "1", "--ema", "1").ema == 1
    for name, bads in (("--fss_sal", ("2", "-1", "x", "1.0")),
                       ("--sal_quantiles", ("1.5", "-0.1", "", "a", "0,.1,.2,.3,.4,.5,.6,.7,.8", "nan")),
                       ("--sal_thresholds", ("nan", "inf", "x", "", "0,1,2,3,4,5,6,7,8")),
                       ("--sal_floor", ("nan", "inf", "-inf", "x")), ("--sal_conn", ("0", "6", "x", "8.0"))):
        for bad in bads:
            with pytest.raises(SystemExit):
                _parse(name, bad)
    for metric in ("marginal", "fss", "mse", "minkowski"):         # the others keep parsing
        assert O.TestOptions().parse(["--chk_path", "c", "--dataroot", "d", "--metric", metric]).metric == metric
    with pytest.raises(SystemExit):                                  # and there is no metric of that name
        O.TestOptions().parse(["--chk_path", "c", "--dataroot", "d", "--metric", "sal"])
    assert all(w in O.TestOptions.__doc__ for w in ("--fss_sal", "--sal_quantiles", "--sal_thresholds", "--sal_floor", "--sal_conn"))
    assert "sal" not in [m.name for m in EM.METRICS]
    doc = [m.doc for m in EM.METRICS if m.name == "fss"][0]
    assert doc.startswith("  fss ") and "--fss_sal 1" in doc and "Wernli" in doc and "ops.sal_scores" in doc and "sal.npz" in doc
    assert all(w in doc for w in ("--sal_quantiles", "--sal_thresholds", "--sal_floor", "--sal_conn", "model.translate_sal"))
    assert EM.SAL_PAIRS == ("members_B", "ens_mean_B", "fake_A")


def test_the_header_declares_both_entries_and_the_binding_matches():
    from dtgan_amd import _lib
    for name, nargs in (("acg_sal_workspace_bytes", 5), ("acg_sal", 18)):
        assert len(abi.header_args(name)) == len(_lib.SIGNATURES[name][1]) == nargs, name
    for name in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        doc = open(os.path.join(ROOT, name)).read()
        assert "acg_sal" in doc and "--metric fss --fss_sal 1" in doc, name
    assert "ops.sal_scores" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    # whole planes of 32 H W bytes (int32 parents, uint32 peaks, three uint64 sums); at most what fits 256 MiB, at least one
    assert lib.acg_sal_workspace_bytes(2, 3, 64, 64, 31) == 2 * 3 * 31 * 64 * 64 * 32
    assert lib.acg_sal_workspace_bytes(1, 1, 7, 5, 1) == 7 * 5 * 32 and lib.acg_sal_workspace_bytes(1, 2, 1, 1, 3) == 6 * 32
    assert lib.acg_sal_workspace_bytes(255, 3, 256, 256, 31) == 256 << 20
    assert lib.acg_sal_workspace_bytes(64, 1, 1000, 1000, 1) == ((256 << 20) // 32000000) * 32000000
    assert lib.acg_sal_workspace_bytes(1, 1, 1024, 1024, 1) == 32 << 20 and lib.acg_sal_workspace_bytes(3, 1, 1024, 1024, 255) == 256 << 20
    for bad in ((0, 1, 8, 8, 1), (1, 0, 8, 8, 1), (1, 1, 0, 8, 1), (1, 1, 8, 0, 1), (1, 1, 8, 1025, 1), (1, 1, 1025, 8, 1), (1, 1, 8, 8, 0),
                (1, 1, 8, 8, 256), (1 << 30, 4, 8, 8, 1)):
        assert lib.acg_sal_workspace_bytes(*bad) == 0, bad


def test_ops_refuses_on_the_host_before_any_device_call(monkeypatch):
    from dtgan_amd import _lib, ops

    def no_device(*a, **k):
        raise AssertionError("a refusal reached the library")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(_lib, "query", no_device)
    z = lambda *shape: torch.zeros(shape)
    thr = np.zeros((1, 2), np.float32)
    with pytest.raises(_lib.AcgError, match="layout"):
        ops.sal(z(1, 1, 32, 32), 1, "chwn", thr)
    with pytest.raises(_lib.AcgError, match="4-d"):
        ops.sal(z(1, 32, 32), 1, "nchw", thr)
    with pytest.raises(_lib.AcgError, match="1024"):
        ops.sal(z(1, 1, 4, 1025), 1, "nchw", thr)
    with pytest.raises(_lib.AcgError, match="1024"):
        ops.sal(z(1, 1025, 4, 4), 1, "nhwc", thr)
    with pytest.raises(_lib.AcgError, match="channels"):
        ops.sal(z(2, 8, 8, 4), 5, "nhwc", np.zeros((5, 1), np.float32))
    for bad in (0, 6, 16, "8", None):
        with pytest.raises(_lib.AcgError, match="connectivity"):
            ops.sal(z(2, 1, 8, 8), 1, "nchw", thr, conn=bad)
    for bad in (float("nan"), float("inf"), -float("inf"), "0", None, True):
        with pytest.raises(_lib.AcgError, match="floor"):
            ops.sal(z(2, 1, 8, 8), 1, "nchw", thr, floor=bad)
    for bad in (np.zeros((2, 2), np.float32), np.zeros(2, np.float32), np.zeros((1, 256), np.float32), np.zeros((1, 0), np.float32),
                np.array([[1.0, 0.0]]), np.array([[0.0, np.nan]]), np.array([[0.0, np.inf]])):
        with pytest.raises(_lib.AcgError, match="sal: thresholds"):
            ops.sal(z(2, 1, 8, 8), 1, "nchw", bad)
    for bad in (torch.zeros(2, 2), torch.zeros(1, 256), torch.zeros(1, 2, dtype=torch.float64)):      # tensors: shape and type only
        with pytest.raises(_lib.AcgError, match="sal: thresholds"):
            ops.sal(z(2, 1, 8, 8), 1, "nchw", bad)
    i64, f64 = torch.int64, torch.float64
    good = lambda: [torch.zeros(2, 1, 3, dtype=i64), torch.zeros(2, 1, 2, 4, dtype=i64), torch.zeros(2, 1, 2, 2, dtype=f64)]
    for i, name, bads in ((0, "field", (torch.zeros(2, 1, 3), torch.zeros(2, 1, 4, dtype=i64), torch.zeros(2, 1, 6, dtype=i64)[..., ::2])),
                          (1, "obj", (torch.zeros(2, 1, 2, 4, dtype=f64), torch.zeros(2, 1, 3, 4, dtype=i64))),
                          (2, "shape", (torch.zeros(2, 1, 2, 2), torch.zeros(2, 1, 2, 2, dtype=i64), torch.zeros(2, 1, 2, 3, dtype=f64)))):
        for b in bads:
            out = good()
            out[i] = b
            with pytest.raises(_lib.AcgError, match="sal: " + name):
                ops.sal(z(2, 1, 8, 8), 1, "nchw", thr, out=out)
    for bad in (torch.zeros(2, 1, 3, dtype=i64), good()[:2], [good()[0], None, 5]):
        with pytest.raises(_lib.AcgError, match="triple"):
            ops.sal(z(2, 1, 8, 8), 1, "nchw", thr, out=bad)
    with pytest.raises(_lib.AcgError, match="ROCm device"):          # and a valid call has no CPU path
        ops.sal(z(2, 1, 8, 8), 1, "nchw", thr)
    with pytest.raises(_lib.AcgError, match="ROCm device"):
        ops.sal(z(2, 1, 8, 8), 1, "nchw", thr, out=good())
