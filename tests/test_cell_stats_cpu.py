"""No GPU: the NumPy definition of the per-cell statistics (tests/cell_stats_ref.py) against a brute force over cells, its
batch-split invariance, ops.cell_summary against np.corrcoef / np.searchsorted per cell, closed forms, the Brier identity and
every NaN rule, the four --map_* options, plan_ens_maps' refusals and every host-side refusal of ops.cell_stats."""
import argparse

import numpy as np
import pytest
import torch

import cell_stats_ref as R
from eval_cases import parse_test

RTOL = 1e-12


def _state(x, y, M, thr=None, edges=None):
    C, H, W = y.shape[1:]
    return R.accumulate(R.new_state(C, H, W, 0 if thr is None else thr.shape[1], 0 if edges is None else edges.shape[1]), x, y, M, thr, edges)


def test_reference_equals_a_brute_force_over_cells_and_does_not_depend_on_the_split():
    C, H, W, M, Ny = 2, 3, 5, 3, 4
    thr, edges = R.tables(C, 3, 6)
    x, y = R.fields(Ny, M, C, H, W, seed=1, thr=thr, edges=edges)
    s = _state(x, y, M, thr, edges)
    for c in range(C):
        for i in range(H):
            for j in range(W):
                a, e, hx, hy = R.brute_cell(x, y, M, c, i, j, thr, edges)
                assert R.same(a, s["mom"][:, c, i, j].copy()) and np.array_equal(e, s["evt"][c, :, :, i, j])
                assert np.array_equal(hx, s["hist_x"][c, :, i, j]) and np.array_equal(hy, s["hist_y"][c, :, i, j])
    assert np.all(s["hist_x"].sum(1) == Ny * M) and np.all(s["hist_y"].sum(1) == Ny) and s["n"] == Ny and s["M"] == M
    for cut in (1, 2, 3):                                          # the rows in two calls: the same bits
        t = R.accumulate(R.new_state(C, H, W, 3, 6), x[:cut * M], y[:cut], M, thr, edges)
        R.accumulate(t, x[cut * M:], y[cut:], M, thr, edges)
        assert R.same_state(s, t) and all(s[k].tobytes() == t[k].tobytes() for k in ("mom", "evt", "hist_x", "hist_y"))
    # the bin of a value on an edge lies above it, of a NaN in bin 0, a repeated edge counts twice
    e = np.float32([[0.0, 1.0, 1.0, 2.0]])
    v = np.float32([np.nan, -1.0, -0.0, 0.5, 1.0, 2.0, np.inf, -np.inf]).reshape(1, 1, 8)
    assert R.bins(v, e)[0, 0].tolist() == [0, 0, 1, 1, 3, 4, 4, 0]
    assert np.array_equal(R.bins(v, e)[0, 0][1:], np.searchsorted(e[0], v[0, 0, 1:], side="right"))


def test_cell_summary_against_numpy_per_cell():
    from dtgan_amd import ops
    C, H, W, M, Ny = 2, 2, 3, 4, 9
    thr, edges = R.tables(C, 2, 7, seed=3)
    x, y = R.fields(Ny, M, C, H, W, seed=2, special=False)
    levels = (0.25, 0.5, 0.9, 1.0)
    s = _state(x, y, M, thr, edges)
    m = ops.cell_summary(s, thr, edges, levels)
    xm = x.reshape(Ny, M, C, H, W).astype(np.float64)
    yd = y.astype(np.float64)
    close = lambda a, b: np.testing.assert_allclose(a, b, rtol=RTOL, atol=1e-13)
    close(m["mean_x"], xm.mean((0, 1))), close(m["mean_y"], yd.mean(0)), close(m["bias"], xm.mean((0, 1)) - yd.mean(0))
    close(m["std_x"], xm.std((0, 1))), close(m["std_y"], yd.std(0)), close(m["std_ratio"], xm.std((0, 1)) / yd.std(0))
    close(m["rmse"], np.sqrt(((xm - yd[:, None]) ** 2).mean((0, 1)))), close(m["mae"], np.abs(xm - yd[:, None]).mean((0, 1)))
    em = xm.mean(1)
    close(m["rmse_mean"], np.sqrt(((em - yd) ** 2).mean(0)))
    close(m["spread"], np.sqrt(xm.var(1, ddof=1).mean(0)))
    close(m["spread_skill"], np.sqrt((M + 1.0) / M) * m["spread"] / m["rmse_mean"])
    for c in range(C):
        for i in range(H):
            for j in range(W):
                yy = np.repeat(yd[:, c, i, j], M)
                close(m["corr"][c, i, j], np.corrcoef(xm[:, :, c, i, j].reshape(-1), yy)[0, 1])
                close(m["corr_mean"][c, i, j], np.corrcoef(em[:, c, i, j], yd[:, c, i, j])[0, 1])
                xs, ys = np.sort(x[:, c, i, j]), np.sort(y[:, c, i, j])
                cx = np.searchsorted(xs, edges[c], side="left") / float(Ny * M)      # the share of values below the edge
                cy = np.searchsorted(ys, edges[c], side="left") / float(Ny)
                close(m["cdf_x"][c, :, i, j], cx), close(m["cdf_y"][c, :, i, j], cy)
                close(m["ks"][c, i, j], np.abs(cx - cy).max())
                for li, lv in enumerate(levels):                   # the first edge whose CDF reaches the level
                    hit = np.nonzero(cx >= lv)[0]
                    want = edges[c, hit[0]] if hit.size else np.nan
                    assert (np.isnan(want) and np.isnan(m["q_x"][c, li, i, j])) or m["q_x"][c, li, i, j] == want
                    # and it brackets np.quantile from above, to the resolution of the edges
                    if hit.size:
                        assert np.quantile(xs.astype(np.float64), lv, method="inverted_cdf") <= want or cx[hit[0]] == lv
    # the events: frequencies, the Brier identity against a per-cell float64 evaluation, hit rate and CSI
    k = (x.reshape(Ny, M, C, 1, H, W) >= thr[None, None, :, :, None, None]).sum(1).astype(np.float64)
    o = (y[:, :, None] >= thr[None, :, :, None, None]).astype(np.float64)
    close(m["freq_x"], k.mean(0) / M), close(m["freq_y"], o.mean(0)), close(m["brier"], ((k / M - o) ** 2).mean(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        hits, union = (k * o).sum(0), (k + M * o - k * o).sum(0)
        close(m["hit_rate"], np.where(o.sum(0) > 0, hits / (M * o.sum(0)), np.nan))
        close(m["csi"], np.where(union > 0, hits / union, np.nan))
        close(m["freq_bias"], np.where(o.sum(0) > 0, (k.mean(0) / M) / o.mean(0), np.nan))
    assert set(m) == {"mean_x", "mean_y", "bias", "std_x", "std_y", "std_ratio", "corr", "rmse", "mae", "rmse_mean", "corr_mean", "spread",
                      "spread_skill", "freq_x", "freq_y", "freq_bias", "brier", "hit_rate", "csi", "cdf_x", "cdf_y", "ks", "q_x", "q_y"}
    assert all(v.dtype == np.float64 for v in m.values())


def test_closed_forms():
    from dtgan_amd import ops
    C, H, W, Ny = 1, 2, 4, 6
    rs = np.random.RandomState(4)
    y = rs.normal(0, 1, (Ny, C, H, W)).astype(np.float32)
    thr = np.float32([[0.0]])
    # x on the truth, two identical members: no error, correlation 1 (to rounding), a collapsed ensemble's spread exactly 0
    m = ops.cell_summary(_state(np.repeat(y, 2, 0), y, 2, thr), thr)
    assert np.all(m["bias"] == 0) and np.all(m["mae"] == 0) and np.all(m["spread"] == 0)
    # rmse comes from Sxx + M Syy - 2 Sxy, three sums of about N each rounded to 2^-53 relatively: what is left of the
    # cancellation is below sqrt(8 N 2^-53) of the values' size, 1e-7 here
    assert np.all(m["rmse"] < 1e-7) and np.all(m["rmse_mean"] < 1e-7)
    assert np.all(np.isnan(m["spread_skill"][m["rmse_mean"] == 0])) and np.allclose(m["corr"], 1, rtol=0, atol=1e-12) and np.allclose(m["std_ratio"], 1, rtol=0, atol=1e-12)
    assert np.all(m["brier"] == 0) and np.all(m["freq_bias"][m["freq_y"] > 0] == 1) and np.all(m["csi"][m["freq_y"] > 0] == 1)
    # a collapsed ensemble of values whose M Q - S S rounds below zero somewhere is clamped, never NaN
    x3 = np.repeat((y * np.float32(1e3) + np.float32(0.1)).astype(np.float32), 3, 0)
    s3 = _state(x3, y, 3)
    assert np.all(ops.cell_summary(s3)["spread"] == 0) or np.all(np.isfinite(ops.cell_summary(s3)["spread"]))
    assert np.all(ops.cell_summary(dict(s3, mom=np.where(np.arange(9)[:, None, None, None] == 8, -1e-9, s3["mom"])))["spread"] == 0)
    # a constant offset (exact in float32): bias, rmse and mae are the offset, correlation stays 1
    off = ops.cell_summary(_state((y.astype(np.float64) + 0.5).astype(np.float32) * 0 + (np.round(y * 8) / 8 + np.float32(0.5)), np.round(y * 8) / 8, 1))
    assert np.allclose(off["bias"], 0.5, rtol=0, atol=1e-13) and np.allclose(off["rmse"], 0.5, rtol=0, atol=1e-12) and np.all(off["mae"] == 0.5)
    assert np.allclose(off["corr"], 1, rtol=0, atol=1e-12) and np.all(np.isnan(off["spread"])) and np.all(np.isnan(off["spread_skill"]))
    # one member: the ensemble mean is the member
    x1 = rs.normal(0, 1, (Ny, C, H, W)).astype(np.float32)
    one = ops.cell_summary(_state(x1, y, 1))
    assert np.allclose(one["rmse_mean"], one["rmse"], rtol=1e-12) and np.allclose(one["corr_mean"], one["corr"], rtol=1e-10)
    # members that are permutations of each other: the per-truth sums S, Q do not move, nor does anything derived from them
    xa = rs.normal(0, 1, (Ny, 3, C, H, W)).astype(np.float32)
    a, b = _state(xa.reshape(-1, C, H, W), y, 3), _state(xa[:, ::-1].reshape(-1, C, H, W), y, 3)
    pa, pb = ops.cell_summary(a), ops.cell_summary(b)
    assert all(np.allclose(pa[k], pb[k], rtol=1e-12, atol=1e-14) for k in pa)
    # all events, no events
    hi, lo = np.full_like(y, 2.0), np.full_like(y, -2.0)
    ev = ops.cell_summary(_state(np.repeat(hi, 2, 0), hi, 2, thr), thr)
    assert np.all(ev["freq_x"] == 1) and np.all(ev["freq_y"] == 1) and np.all(ev["brier"] == 0) and np.all(ev["hit_rate"] == 1) and np.all(ev["csi"] == 1)
    no = ops.cell_summary(_state(np.repeat(lo, 2, 0), lo, 2, thr), thr)
    assert np.all(no["freq_x"] == 0) and np.all(no["brier"] == 0) and all(np.all(np.isnan(no[k])) for k in ("freq_bias", "hit_rate", "csi"))
    miss = ops.cell_summary(_state(np.repeat(lo, 2, 0), hi, 2, thr), thr)
    assert np.all(miss["brier"] == 1) and np.all(miss["hit_rate"] == 0) and np.all(miss["csi"] == 0) and np.all(miss["freq_bias"] == 0)


def test_nan_rules_of_cell_summary():
    from dtgan_amd import ops
    y = np.zeros((3, 1, 1, 2), np.float32)
    y[:, 0, 0, 1] = (1, 2, 3)
    x = np.repeat(y, 2, 0) + np.float32(1)
    x[:, 0, 0, 0] = 1.0
    edges = np.float32([[0.5, 10.0]])
    m = ops.cell_summary(_state(x, y, 2, None, edges), None, edges, (0.5, 1.0))
    assert np.isnan(m["corr"][0, 0, 0]) and np.isnan(m["std_ratio"][0, 0, 0]) and np.isnan(m["corr_mean"][0, 0, 0])      # zero variances: NaN, not inf
    assert np.isfinite(m["corr"][0, 0, 1]) and abs(m["std_ratio"][0, 0, 1] - 1) < 1e-12
    assert m["q_x"][0, :, 0, 0].tolist() == [10.0, 10.0] and m["q_y"][0, 0, 0, 0] == 0.5         # the first edge whose CDF reaches the level
    none = ops.cell_summary(_state(x + 100, y, 2, None, edges), None, edges, (0.5,))
    assert np.all(np.isnan(none["q_x"])) and np.all(none["cdf_x"] == 0)                        # no edge reaches it
    empty = ops.cell_summary(R.new_state(1, 1, 2, 1, 1), np.zeros((1, 1), np.float32), np.zeros((1, 1), np.float32), (0.5,))
    assert all(np.all(np.isnan(v)) for v in empty.values())                                    # n = 0
    bad = _state(x, y, 2)
    bad["mom"][0, 0, 0, 0] = np.nan
    assert np.isnan(ops.cell_summary(bad)["bias"][0, 0, 0]) and np.isfinite(ops.cell_summary(bad)["bias"][0, 0, 1])
    assert not any(np.isinf(v).any() for v in m.values())
    for wrong in (dict(mom=np.zeros((8, 1, 1, 2))), dict(evt=np.zeros((1, 1, 3, 1, 2), np.int64)), dict(hist_x=np.zeros((1, 2, 1, 2), np.int32))):
        with pytest.raises(ValueError, match="cell_summary"):
            ops.cell_summary(dict(R.new_state(1, 1, 2, 1, 2), n=1, M=1, **wrong), np.zeros((1, 1)), np.zeros((1, 2)))


def test_options_and_their_refusals():
    opt = parse_test("ensemble")
    assert (opt.ens_maps, opt.map_quantiles, opt.map_thresholds, opt.map_bins, opt.map_levels) == (0, (0.9, 0.99), None, 32, (0.5, 0.95, 0.99))
    opt = parse_test("ensemble", "--ens_maps", "1", "--map_quantiles", "0.99,0.5", "--map_thresholds", "3,-1.5", "--map_bins", "0", "--map_levels", "0,1")
    assert (opt.ens_maps, opt.map_quantiles, opt.map_thresholds, opt.map_bins, opt.map_levels) == (1, (0.5, 0.99), (-1.5, 3.0), 0, (0.0, 1.0))
    assert parse_test("ensemble", "--map_quantiles", "none").map_quantiles == () and parse_test("ensemble", "--map_bins", "64").map_bins == 64
    for bad in (("--ens_maps", "2"), ("--map_quantiles", "1.5"), ("--map_quantiles", ",".join(["0.5"] * 9)), ("--map_quantiles", "x"),
                ("--map_thresholds", "nan"), ("--map_thresholds", "inf"), ("--map_thresholds", ",".join(["1"] * 9)), ("--map_bins", "1"),
                ("--map_bins", "65"), ("--map_bins", "-2"), ("--map_levels", "1.01"), ("--map_levels", ",".join(["0.5"] * 17))):
        with pytest.raises(SystemExit):
            parse_test("ensemble", *bad)


def test_plan_ens_maps_and_its_refusals():
    from dtgan_amd import eval_metrics as EM, ops
    rs = np.random.RandomState(0)
    small = [rs.normal(0, 1, (n, 2, 4, 5)).astype(np.float32) for n in (6, 6, 3, 3, 2, 2)]
    opt = argparse.Namespace(map_quantiles=(0.5, 0.9), map_thresholds=None, map_bins=4, map_levels=(0.5,), n_samples=3)
    p = EM.plan_ens_maps(opt, small)
    assert np.array_equal(p["thresholds_B"], EM.fss_thresholds(small[1], (0.5, 0.9))) and np.array_equal(p["thresholds_A"], EM.fss_thresholds(small[0], (0.5, 0.9)))
    assert np.array_equal(p["edges_B"], EM.marginal_edges(small[1], 4)) and p["edges_A"].shape == (2, 3) and p["levels"] == (0.5,)
    opt.map_thresholds, opt.map_bins = (1.0, 2.0, 3.0), 0
    p = EM.plan_ens_maps(opt, small)
    assert p["thresholds_A"].tolist() == [[1.0, 2.0, 3.0]] * 2 and p["edges_B"] is None and p["edges_A"] is None
    opt.map_thresholds, opt.map_quantiles = None, ()
    assert EM.plan_ens_maps(opt, small)["thresholds_B"] is None
    assert ops.cell_state_bytes(3, 321, 321, 2, 31) == 3 * 321 * 321 * (72 + 64 + 256)
    # a whole-split state above 2 GiB is refused before any data is touched: the size and the options that shrink it
    class Shape(object):                                           # arrays the plan only asks for their shape and length
        def __init__(self, *shape):
            self.shape = shape

        def __len__(self):
            return self.shape[0]
    big = list(small[:2]) + [Shape(4, 2, 1024, 1024)] * 4
    opt = argparse.Namespace(map_quantiles=(0.5,) * 8, map_thresholds=None, map_bins=64, map_levels=(0.5,), n_samples=3)
    with pytest.raises(ValueError, match=r"--ens_maps: .*3523215360 bytes \(3\.28 GiB\).*--map_bins.*--map_quantiles"):
        EM.plan_ens_maps(opt, big)
    opt.map_bins = 0
    assert EM.plan_ens_maps(opt, big)["edges_B"] is None           # 1.25 GiB passes
    with pytest.raises(ValueError, match="int32 histogram"):
        EM.plan_ens_maps(argparse.Namespace(map_quantiles=(), map_thresholds=None, map_bins=0, map_levels=(), n_samples=64),
                         list(small[:2]) + [Shape(1 << 26, 1, 2, 2)] * 4)


def test_host_side_refusals_of_cell_stats_name_it():
    from dtgan_amd import _lib, ops
    x, y = torch.zeros(4, 2, 3, 5), torch.zeros(2, 2, 3, 5)
    thr, edges = np.zeros((2, 1), np.float32), np.float32([[0, 1], [0, 1]])
    s = ops.cell_state(2, 3, 5, 1, 2, "cpu")
    assert s["mom"].shape == (9, 2, 3, 5) and s["evt"].shape == (2, 1, 4, 3, 5) and s["hist_x"].shape == (2, 3, 3, 5) and (s["n"], s["M"]) == (0, 0)
    assert s["mom"].dtype == torch.float64 and s["evt"].dtype == torch.int64 and s["hist_y"].dtype == torch.int32
    bare = ops.cell_state(2, 3, 5, 0, 0, "cpu")
    assert bare["evt"] is None and bare["hist_x"] is None and bare["hist_y"] is None
    for bad in ((0, 3, 5, 0, 0), (1, 0, 5, 0, 0), (1, 3, 1025, 0, 0), (1, 3, 5, 9, 0), (1, 3, 5, 0, 64), (1, 3, 5, -1, 0)):
        with pytest.raises(ValueError, match="cell_state"):
            ops.cell_state(*bad, device="cpu")
    call = lambda **kw: ops.cell_stats(*[kw.pop(k, d) for k, d in (("x", x), ("y", y), ("C", 2), ("lx", "nchw"), ("ly", "nchw"), ("state", s))],
                                       **dict(dict(thresholds=thr, edges=edges, x_per_y=2), **kw))
    cases = ((dict(x=x[0]), "4-d"), (dict(lx="chwn"), "layout"), (dict(C=3), "stored channels"), (dict(x_per_y=3), "x_per_y"), (dict(x_per_y=65), "x_per_y"),
             (dict(x_per_y=1), "do not pair"), (dict(y=torch.zeros(2, 2, 3, 6)), "do not pair"), (dict(x=torch.zeros(2, 2, 1025, 1), y=torch.zeros(1, 2, 1025, 1)), "H x W"),
             (dict(state=None), "dict"), (dict(state={"mom": s["mom"]}), "dict"), (dict(thresholds=None), r"state\['evt'\] is present"),
             (dict(edges=None), r"state\['hist_x'\] is present"), (dict(state=bare), r"state\['evt'\] is absent"), (dict(thresholds=np.zeros((2, 2), np.float32)), r"state\['evt'\]"),
             (dict(edges=np.zeros((2, 3), np.float32)), r"state\['hist_x'\]"), (dict(thresholds=np.zeros((3, 1), np.float32)), "thresholds must be"),
             (dict(thresholds=np.zeros((2, 9), np.float32)), "thresholds must be"), (dict(edges=np.zeros((2, 64), np.float32)), "edges must be"),
             (dict(edges=np.float32([[1, 0], [0, 1]])), "non-decreasing"), (dict(edges=np.float32([[0, np.nan], [0, 1]])), "finite"),
             (dict(state=dict(s, mom=s["mom"].float())), r"state\['mom'\]"), (dict(state=dict(s, hist_y=s["hist_y"][:, :, :, :4])), r"state\['hist_y'\]"),
             (dict(state=dict(s, evt=s["evt"].numpy())), r"state\['evt'\]"), (dict(state=dict(s, M=3)), "M=3"))
    for kw, word in cases:
        with pytest.raises(_lib.AcgError, match="cell_stats: .*" + word):
            call(**kw)
    with pytest.raises(_lib.AcgError, match="ROCm device"):        # and what has passed them all reaches the device check
        call()
    assert (s["n"], s["M"]) == (0, 0) and not s["mom"].any()
