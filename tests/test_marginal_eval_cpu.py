"""CPU tests of the marginal evaluator's definition (tests/marginal_eval_ref.py against numpy.quantile, scipy's Wasserstein
distance, numpy.searchsorted and closed forms), of marginal_edges and ops.marginal_summary, of the new entry point's
declaration and of the --metric marginal options."""
import os

import numpy as np
import pytest

import abi
import dtgan_amd  # noqa: F401
from dtgan_amd import ops
from dtgan_amd import options as O
from dtgan_amd import eval_metrics as EM
import marginal_eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--chk_path", "e/latest", "--dataroot", "d", "--metric", "marginal"]


def _sorted(kind, H, W, rows=2, C=2, seed=0):
    x = R.make_fields(kind, H, W, rows, C, seed)
    return x, R.sorted_values(x.reshape(rows, C, H * W))


@pytest.mark.parametrize("H, W", R.CPU_SHAPES)
def test_the_quantiles_are_numpys_linear_ones_within_one_float32_ulp(H, W):
    for kind in R.FIELD_KINDS:
        x, s = _sorted(kind, H, W)
        q = R.quantiles(s, R.LEVELS16)
        assert q.dtype == np.float32 and q.shape == (2, 2, 16)
        want = np.quantile(x.reshape(2, 2, -1).astype(np.float64), np.asarray(R.LEVELS16, dtype=np.float64), axis=-1,
                           method="linear")
        want = np.moveaxis(want, 0, -1).astype(np.float32)
        assert R.ulp_distance(q, want).max() <= 1, (kind, H, W)
        assert np.array_equal(q[..., 0], s[..., 0]) and np.array_equal(q[..., 1], s[..., -1])     # level 0: min, level 1: max


@pytest.mark.parametrize("H, W", [(1, 1), (11, 13), (64, 64), (91, 91)])
def test_w1_is_scipys_wasserstein_distance(H, W):
    stats = pytest.importorskip("scipy.stats")
    for i, kind in enumerate(R.FIELD_KINDS):
        x, sx = _sorted(kind, H, W, seed=1)
        y, sy = _sorted(R.FIELD_KINDS[(i + 2) % len(R.FIELD_KINDS)], H, W, seed=2)
        w = R.wasserstein(sx, sy)
        for r in range(2):
            for c in range(2):
                ref = stats.wasserstein_distance(x[r, c].ravel().astype(np.float64), y[r, c].ravel().astype(np.float64))
                assert abs(w[r, c, 0] - ref) <= 1e-12, (kind, H, W)


def test_a_shift_gives_its_size_and_equal_fields_give_exactly_zero():
    for kind in R.FIELD_KINDS:
        x, sx = _sorted(kind, 17, 13)
        assert np.all(R.wasserstein(sx, sx) == 0.0)
        for shift in (0.5, -0.25):
            y = (x + np.float32(shift)).astype(np.float32)                    # 0.5 ulp of a value below 2: 2^-24 each
            w = R.wasserstein(R.sorted_values(y.reshape(2, 2, -1)), sx)
            assert np.all(np.abs(w[..., 0] - abs(shift)) <= 2.0 ** -24), kind
            assert np.all(np.abs(w[..., 1] - shift * shift) <= 2 * abs(shift) * 2.0 ** -24 + 2.0 ** -48), kind


def test_members_share_a_truth_row_by_row():
    x, sx = _sorted("uniform", 8, 8, rows=6)
    y, sy = _sorted("tanh_normal", 8, 8, rows=2)
    w = R.wasserstein(sx, sy, x_per_y=3)
    for r in range(6):
        assert np.array_equal(w[r], R.wasserstein(sx[r:r + 1], sy[r // 3:r // 3 + 1])[0])


@pytest.mark.parametrize("kind", R.FIELD_KINDS)
def test_the_counts_are_searchsorted_and_complement_the_fss_events(kind):
    x, s = _sorted(kind, 11, 13)
    edges = R.make_edges(s, 256)
    b = R.below(s, edges)
    assert b.dtype == np.int32 and b.shape == (2, 2, 256)
    flat = x.reshape(2, 2, -1)
    for r in range(2):
        for c in range(2):
            for e in range(256):
                assert b[r, c, e] == int((flat[r, c] < edges[c, e]).sum())
                assert flat.shape[-1] - b[r, c, e] == int((flat[r, c] >= edges[c, e]).sum())
    # integers add: the members' counts are the counts of the concatenated members
    pooled = np.sort(np.concatenate([s[0], s[1]], axis=-1)[None], axis=-1)
    assert np.array_equal(b.sum(0, dtype=np.int64), R.below(pooled, edges)[0])


def test_scores_holds_only_what_was_asked_for():
    x = R.make_fields("masked", 9, 7, 4, 3)
    y = R.make_fields("uniform", 9, 7, 2, 3)
    s = R.sorted_values(x.reshape(4, 3, -1))
    e = R.make_edges(s, 1)
    full = R.scores(x, y, R.LEVELS1, e, x_per_y=2)
    assert full["w"].shape == (4, 3, 2) and full["q"].shape == (4, 3, 1) and full["below"].shape == (4, 3, 1)
    assert sorted(R.scores(x, None, R.LEVELS1, None)) == ["q"] and sorted(R.scores(x, y, (), None, 2)) == ["w"]
    assert sorted(R.scores(x, None, (), e)) == ["below"]


def test_marginal_edges_are_the_training_quantiles_per_channel():
    train = np.concatenate([R.make_fields("masked", 16, 16, 5, 2), R.make_fields("uniform", 16, 16, 4, 2, seed=3)])
    for bins in (2, 10, 100, 257):
        e = EM.marginal_edges(train, bins)
        assert e.dtype == np.float32 and e.shape == (2, bins - 1)
        for c in range(2):
            want = np.quantile(train[:, c].astype(np.float64).ravel(), np.arange(1, bins) / float(bins))
            assert np.array_equal(e[c], want.astype(np.float32))
        assert np.all(np.diff(e, axis=1) >= 0)
    assert np.any(np.diff(EM.marginal_edges(train, 100), axis=1) == 0)               # the mass at 0 repeats an edge
    for bins in (1, 258):
        with pytest.raises(ValueError):
            EM.marginal_edges(train, bins)


def test_marginal_summary_on_hand_made_counts():
    below = np.array([[0, 5, 10, 20], [20, 20, 0, 10]], dtype=np.int64)
    real = np.array([[0, 10, 10, 40], [40, 0, 0, 20]], dtype=np.int64)
    s = ops.marginal_summary(below, 20, real, 40)
    assert s["cdf"].dtype == np.float64 and s["cdf"].shape == (2, 4) and s["ks"].shape == (2,)
    assert np.array_equal(s["cdf"], [[0, 0.25, 0.5, 1.0], [1.0, 1.0, 0, 0.5]])
    assert np.array_equal(s["cdf_real"], [[0, 0.25, 0.25, 1.0], [1.0, 0, 0, 0.5]])
    assert np.array_equal(s["ks"], [0.25, 1.0])
    same = ops.marginal_summary(real, 40, real, 40)
    assert np.all(same["ks"] == 0.0) and np.array_equal(same["cdf"], same["cdf_real"])
    assert np.array_equal(ops.marginal_summary(np.zeros((3, 0)), 1, np.zeros((3, 0)), 1)["ks"], np.zeros(3))
    with pytest.raises(ValueError):
        ops.marginal_summary(below, 20, real[:, :3], 40)
    with pytest.raises(ValueError):
        ops.marginal_summary(below, 0, real, 40)


def test_check_levels_and_the_limits():
    assert ops.MARG_MAX_LEVELS == 16 and ops.MARG_MAX_EDGES == 256
    assert ops.check_levels([1, 0, 0.5]) == (1.0, 0.0, 0.5) and ops.check_levels(()) == ()
    assert len(ops.check_levels(R.LEVELS16)) == 16
    for bad in ((1.5,), (-0.1,), (float("nan"),), tuple([0.5] * 17)):
        with pytest.raises(ValueError):
            ops.check_levels(bad)


def test_the_header_declares_the_entry_and_the_binding_matches():
    from dtgan_amd import _lib
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert abi.declarations()["acg_marginal_scores"][0] == "int"
    assert len(abi.header_args("acg_marginal_scores")) == len(_lib.SIGNATURES["acg_marginal_scores"][1]) == 14
    assert "acg_marginal_scores" in doc


def test_the_parser_takes_the_metric_with_its_defaults():
    o = O.TestOptions().parse(BASE)
    assert o.metric == "marginal" and o.n_samples == 16 and o.marg_bins == 100
    assert o.marg_levels == (0.0, 0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 0.999, 1.0)
    o = O.TestOptions().parse(BASE + ["--marg_levels", "1,0,0.5", "--marg_bins", "257"])
    assert o.marg_levels == (1.0, 0.0, 0.5) and o.marg_bins == 257
    assert len(O.TestOptions().parse(BASE + ["--marg_levels", ",".join(["0.5"] * 16)]).marg_levels) == 16
    assert O.TestOptions().parse(BASE + ["--marg_bins", "2"]).marg_bins == 2


@pytest.mark.parametrize("extra", [["--marg_levels", ",".join(["0.5"] * 17)], ["--marg_levels", "0.5,1.5"], ["--marg_levels", ""],
                                   ["--marg_bins", "1"], ["--marg_bins", "258"],
                                   ["--fss_quantiles", ",".join(["0.5"] * 9)], ["--quantiles", ",".join(["0.5"] * 9)]])
def test_the_parser_refuses(extra, capsys):
    with pytest.raises(SystemExit):
        O.TestOptions().parse(BASE + extra)
    assert extra[0] in capsys.readouterr().err
    assert len(O.TestOptions().parse(BASE + ["--fss_quantiles", ",".join(["0.5"] * 8)]).fss_quantiles) == 8
