"""CPU tests of the ensemble statistics' definitions (tests/ensemble_ref.py) and of the evaluator's ensemble options."""
import numpy as np
import pytest

import dtgan_amd  # noqa: F401
from ensemble_ref import e2_pairs, e2_sorted, ensemble_stats, quantile_linear
from eval_cases import parse_test


def _parse(*extra, metric="ensemble"):
    return parse_test(metric, *extra)


@pytest.mark.parametrize("M", [1, 2, 3, 7, 16, 33, 64])
def test_sorted_e2_equals_the_double_sum_ties_included(M):
    rs = np.random.RandomState(M)
    x = rs.uniform(-1, 1, (50, M))
    x[:10] = np.round(x[:10] * 2) / 2                            # ties
    x[10:15] = 1.0                                               # all members equal (saturated tanh)
    x[15:20, : M // 2] = -1.0
    assert np.allclose(e2_sorted(x), e2_pairs(x), rtol=1e-12, atol=1e-12)
    assert np.all(e2_sorted(x[10:15]) == 0)


def test_quantiles_follow_numpys_linear_rule():
    rs = np.random.RandomState(1)
    x = rs.randn(20, 9)
    for q in (0.0, 0.05, 0.5, 0.9, 1.0):
        assert np.allclose(quantile_linear(x, q), np.quantile(x, q, axis=-1), rtol=0, atol=1e-12)


def test_reference_scores_of_a_degenerate_ensemble():
    """every member equal: std 0, CRPS = |x - y|, every cell in one rank bin (the middle one when tied with the target)"""
    rs = np.random.RandomState(2)
    one = rs.uniform(-1, 1, (2, 1, 3, 4, 5))
    x = np.repeat(one, 6, axis=1)
    y = rs.uniform(-1, 1, (2, 3, 4, 5))
    y[0, 0, 0, :] = x[0, 0, 0, 0, :]
    r = ensemble_stats(x, y, (0.1, 0.9))
    assert np.allclose(r["std"], 0, atol=1e-15)
    assert np.allclose(r["crps_map"], np.abs(one[:, 0] - y))
    assert r["rank_hist"].sum() == y.size
    assert set(np.nonzero(r["rank_hist"].sum(0))[0]) <= {0, 3, 6}
    assert r["rank_hist"][0, 3] == 5


def test_ensemble_options_defaults_and_refusals():
    o = _parse()
    assert o.metric == "ensemble" and o.n_samples == 16 and o.quantiles == (0.05, 0.5, 0.95)
    assert _parse("--n_samples", "64", "--quantiles", "0,1").n_samples == 64
    assert _parse("--quantiles", "0,0.25,0.5,0.5,1").quantiles == (0.0, 0.25, 0.5, 0.5, 1.0)
    for bad in (["--n_samples", "0"], ["--n_samples", "65"], ["--quantiles", "0.9,0.1"], ["--quantiles", "-0.1,0.5"],
                ["--quantiles", "0.5,1.5"], ["--quantiles", ",".join(["0.5"] * 9)], ["--quantiles", "a,b"]):
        with pytest.raises(SystemExit):
            _parse(*bad)


def test_existing_metrics_still_parse_with_their_defaults():
    for metric in ("bpp", "mse", "visual", "noise_sens", "mvgauss"):
        o = _parse(metric=metric)
        assert o.metric == metric and (o.res_dir, o.train_logvar, o.ubo_steps, o.gpu_ids) == ("test_res", 1, 500, "0")


def test_quantile_level_checks_of_the_host_op():
    from dtgan_amd import ops
    assert ops.check_quantiles([0, 0.5, 1]) == (0.0, 0.5, 1.0)
    for bad in ([], [0.5] * 9, [0.6, 0.4], [1.1]):
        with pytest.raises(ValueError):
            ops.check_quantiles(bad)
