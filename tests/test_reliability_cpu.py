"""CPU tests of the reliability tables: the reference (tests/reliability_ref.py) against a brute force over cells and against
scipy's maximum filter, its sums and its window-1 tie to tests/fss_ref.py, ops.reliability_summary against closed forms, the
Murphy identity, the per-cell evaluation (within reliability_ref.SUMMARY_TOL) and a brute-force Mann-Whitney count, the option
parser (--fss_rel, --rel_windows), the docs and the host-side refusals of ops.reliability."""
import os

import numpy as np
import pytest
import torch

import fss_ref as F
import reliability_ref as R
from eval_cases import parse_test

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOATS = tuple(k for k in R.SUMMARY_KEYS if k not in ("n",))


def _summary(table):
    from dtgan_amd import ops
    return ops.reliability_summary(table)


@pytest.mark.parametrize("H,W,M", ((1, 1, 1), (1, 7, 2), (7, 1, 3), (5, 7, 2), (9, 12, 4)))
def test_reference_equals_a_brute_force_over_cells(H, W, M):
    x, _, thr = F.make_pair("nan", H, W, rows=2 * M, C=2, seed=M)
    y = F.make_pair("ties", H, W, rows=2, C=2, seed=M + 1)[1]
    win = (1, 3, 5, 2 * max(H, W) - 1)
    ref = R.tables(x, y, thr, win, M)
    assert ref.shape == (2, 2, 3, 4, M + 1, 2) and ref.dtype == np.int64
    assert np.array_equal(ref, R.tables_brute(x, y, thr, win, M))


@pytest.mark.parametrize("kind", F.KINDS)
def test_reference_equals_scipys_maximum_filter(kind):
    from scipy.ndimage import maximum_filter
    H, W, M = 33, 70, 3
    x, y, thr = F.make_pair(kind, H, W, rows=2 * M, C=2, seed=3)
    y = y[:2]
    bx, by = F.events(x, thr), F.events(y, thr)
    for n in (1, 3, 9, 65, 2 * max(H, W) - 1):
        size = (1,) * (bx.ndim - 2) + (n, n)
        dx, dy = maximum_filter(bx, size=size, mode="constant", cval=0), maximum_filter(by, size=size, mode="constant", cval=0)
        assert np.array_equal(R.dilate(bx, n), dx) and np.array_equal(R.dilate(by, n), dy), n
        assert np.array_equal(R.dilate(bx, n), (F.box_counts(bx, n) > 0).astype(np.int64)), n      # acg_fss's count is positive
        k = dx.reshape((2, M) + dx.shape[1:]).sum(1)
        assert np.array_equal(R.tables(x, y, thr, (n,), M)[..., 0, :, :], R.table_of_planes(k, dy, M)), n


def test_every_block_sums_to_the_cells_and_window_1_is_fss_refs_ensemble_triple():
    H, W, M = 20, 67, 5
    x, _, thr = F.make_pair("noise", H, W, rows=2 * M, seed=5)
    y = F.make_pair("shifted", H, W, rows=2, seed=6)[1]
    win = (1, 5, 17, 2 * W - 1)
    t = R.tables(x, y, thr, win, M)
    assert np.all(t.sum((-2, -1)) == H * W) and t.min() >= 0
    k = np.arange(M + 1)
    ens = F.ens_triples(x, y, thr, (1,), M)[..., 0, :]
    n = t[..., 0, :, :].sum(-1)
    assert np.array_equal((k * k * n).sum(-1), ens[..., 0])
    assert np.array_equal(t[..., 0, :, 1].sum(-1), ens[..., 1])
    assert np.array_equal((k * t[..., 0, :, 1]).sum(-1), ens[..., 2])
    # the whole domain: every cell has the same pair; the threshold nothing exceeds puts all cells at k = 0, o = 0
    whole = t[..., 3, :, :]
    assert np.all((whole == H * W).sum((-2, -1)) == 1)
    assert np.all(t[:, :, 1, :, 0, 0] == H * W) and np.all(t[:, :, 2, :, M, 1] == H * W)
    # M = 1: the 2 x 2 contingency table of the events
    one = R.tables(x[:2], y, thr, (1,), 1)[..., 0, :, :]
    bx, by = F.events(x[:2], thr), F.events(y, thr)
    for a in (0, 1):
        for b in (0, 1):
            assert np.array_equal(one[..., a, b], ((bx == a) & (by == b)).sum((-2, -1)))


def test_closed_forms():
    M, cells = 4, 1000
    perfect = np.zeros((M + 1, 2), np.int64)
    perfect[0, 0], perfect[M, 1] = 700, 300
    s = _summary(perfect)
    assert s["brier"] == 0 and s["reliability"] == 0 and s["auc"] == 1 and s["bss"] == 1 and s["base_rate"] == 0.3
    assert abs(s["resolution"] - s["uncertainty"]) < 1e-15 and s["brier_fair"] == 0      # 0.21 to a few of its 2.8e-17 ulps
    assert np.array_equal(s["n"], [700, 0, 0, 0, 300]) and s["n"].dtype == np.int64 and np.array_equal(s["prob"], np.arange(5) / 4.0)
    assert np.array_equal(s["obs_freq"], [0, np.nan, np.nan, np.nan, 1], equal_nan=True)
    assert np.array_equal(s["roc_hit"], [0, 1, 1, 1, 1, 1]) and np.array_equal(s["roc_false"], [0, 0, 0, 0, 0, 1])
    same = np.zeros((M + 1, 2), np.int64)                          # the same forecast everywhere: 2 of 4 members
    same[2] = (600, 400)
    s = _summary(same)
    assert s["resolution"] == 0 and s["auc"] == 0.5 and s["brier"] == 0.25
    assert abs(s["reliability"] - 0.01) < 1e-15 and abs(s["uncertainty"] - 0.24) < 1e-15
    none = np.zeros((2, 3, M + 1, 2), np.int64)                    # no event on either side
    none[..., 0, 0] = cells
    s = _summary(none)
    assert s["brier"].shape == (2, 3) and np.all(s["brier"] == 0) and np.all(s["uncertainty"] == 0) and np.all(s["base_rate"] == 0)
    assert np.all(np.isnan(s["bss"])) and np.all(np.isnan(s["auc"])) and np.all(np.isnan(s["roc_hit"])) and np.all(np.isnan(s["obs_freq"][..., 1:]))
    assert np.all(s["roc_false"][..., :-1] == 0) and np.all(s["roc_false"][..., -1] == 1) and s["roc_hit"].shape == (2, 3, M + 2)
    every = np.zeros((M + 1, 2), np.int64)                         # events everywhere on both sides
    every[M, 1] = cells
    s = _summary(every)
    assert s["brier"] == 0 and np.isnan(s["bss"]) and np.isnan(s["auc"]) and np.all(np.isnan(s["roc_false"])) and s["base_rate"] == 1
    single = _summary(np.array([[50, 10], [20, 20]]))              # M = 1: a contingency table
    assert np.isnan(single["brier_fair"]) and single["brier"] == 0.3 and np.array_equal(single["prob"], [0.0, 1.0])
    assert np.array_equal(single["roc_hit"], [0, 20 / 30.0, 1]) and np.array_equal(single["roc_false"], [0, 20 / 70.0, 1])
    # a window wider than the domain: one pair for all cells, whatever the fields hold
    x = np.full((3, 1, 6, 9), -1.0, np.float32)
    y = np.full((1, 1, 6, 9), -1.0, np.float32)
    x[1, 0, 5, 8], y[0, 0, 0, 0] = 1.0, 1.0
    t = R.tables(x, y, np.zeros((1, 1), np.float32), (17, 65), 3)
    assert np.all(t[0, 0, 0, :, 1, 1] == 54) and np.all(t.sum((-2, -1)) == 54)
    for bad in (np.zeros((3,)), np.zeros((4, 3)), np.zeros((1, 2)), np.zeros(())):
        with pytest.raises(ValueError, match="reliability_summary"):
            _summary(bad)


@pytest.mark.parametrize("H,W,M,seed", R.SUMMARY_CASES)
def test_summary_equals_the_per_cell_evaluation(H, W, M, seed):
    k, o = R.summary_case(H, W, M, seed)
    table = R.table_of_planes(k.reshape(H, W), o.reshape(H, W), M)
    got, want = _summary(table), R.summary_cells(k, o, M)
    assert set(got) == set(want) == set(R.SUMMARY_KEYS)
    assert np.array_equal(got["n"], want["n"]) and got["n"].dtype == np.int64
    worst = 0.0
    for key in FLOATS:
        a, b = np.asarray(got[key], np.float64), np.asarray(want[key], np.float64)
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), key
        if np.isfinite(a).any():
            worst = max(worst, float(np.nanmax(np.abs(a - b))))
    print("reliability_summary against the per-cell evaluation at %s: largest error %.3g" % ((H, W, M), worst))
    assert worst <= R.SUMMARY_TOL
    # the Murphy identity, and the fair score against the per-cell formula
    if not np.isnan(got["brier"]):
        assert abs(got["brier"] - (got["reliability"] - got["resolution"] + got["uncertainty"])) <= R.SUMMARY_TOL
    if M > 1:
        cellwise = np.mean((k / float(M) - o) ** 2 - k * (M - k) / (float(M) * M * (M - 1)))
        assert abs(got["brier_fair"] - cellwise) <= R.SUMMARY_TOL and got["brier_fair"] <= got["brier"]
    # the trapezoid area is the Mann-Whitney count over all pairs of cells
    mw = R.auc_mann_whitney(k, o)
    assert np.isnan(mw) and np.isnan(got["auc"]) or abs(got["auc"] - mw) <= R.SUMMARY_TOL
    assert np.isnan(got["auc"]) or (np.all(np.diff(got["roc_hit"]) >= 0) and np.all(np.diff(got["roc_false"]) >= 0))


def test_summary_broadcasts_over_leading_axes():
    tabs = np.stack([R.table_of_planes(*(a.reshape(16, 16) for a in R.summary_case(16, 16, 3, s)), M=3) for s in range(6)]).reshape(2, 3, 4, 2)
    s = _summary(tabs)
    for i in range(2):
        for j in range(3):
            one = _summary(tabs[i, j])
            for key in R.SUMMARY_KEYS:
                assert np.array_equal(np.asarray(s[key])[i, j] if key != "prob" else s[key], one[key], equal_nan=True), key
    summed = _summary(tabs.sum((0, 1)))                              # tables add over pairs; scores do not
    assert summed["n"].sum() == 6 * 256


def _parse(*extra):
    return parse_test("fss", *extra)


def test_the_parser_takes_the_switch_and_its_windows():
    from dtgan_amd import eval_metrics as EM, options as O, test as T
    o = _parse()
    assert o.fss_rel == 0 and o.rel_windows == (1, 5, 17) and o.fss_sal == 0 and o.fss_scales == 0
    assert _parse("--fss_rel", "1").fss_rel == 1 and _parse("--fss_rel", "0", "--fss_sal", "1").fss_rel == 0
    assert _parse("--rel_windows", "3").rel_windows == (3,) and _parse("--rel_windows", "65,1,9").rel_windows == (65, 1, 9)
    assert _parse("--rel_windows", "1,3,5,7,9,11,13,15").rel_windows == (1, 3, 5, 7, 9, 11, 13, 15)
    for name, bads in (("--fss_rel", ("2", "-1", "x", "1.0")),
                       ("--rel_windows", ("2", "0", "-3", "67", "1,4", "", "x", "1.5", "1,3,5,7,9,11,13,15,17"))):
        for bad in bads:
            with pytest.raises(SystemExit):
                _parse(name, bad)
    assert all(w in O.TestOptions.__doc__ for w in ("--fss_rel", "--rel_windows"))
    assert "reliability" not in [m.name for m in EM.METRICS]
    doc = [m.doc for m in EM.METRICS if m.name == "fss"][0]
    assert doc.startswith("  fss ") and "(new)" in doc and not doc.endswith("\n") and doc in T.__doc__
    assert all(w in doc for w in ("--fss_rel 1", "--rel_windows", "ops.reliability", "ops.reliability_summary", "reliability.npz", "Murphy 1973",
                                  "Ferro 2014", "Schwartz & Sobash 2017", "model.translate_fss(reliability=", "acgan_verif.h"))
    assert EM.REL_PAIRS == ("ens_prob_B", "members_B", "ens_mean_B", "fake_A")


def test_check_rel_windows():
    from dtgan_amd import ops
    assert ops.check_rel_windows((1, 5, 17)) == (1, 5, 17) and ops.check_rel_windows([65]) == (65,) and ops.REL_MAX_WINDOW == 65
    for bad in ((), (2,), (0,), (-1,), (67,), (1, 129), (1.5,), tuple(range(1, 19, 2))):
        with pytest.raises(ValueError):
            ops.check_rel_windows(bad)


def test_the_docs_name_the_second_header():
    for name in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        doc = open(os.path.join(ROOT, name)).read()
        assert "acg_reliability" in doc and "--metric fss --fss_rel 1" in doc, name
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(w in integration for w in ("include/acgan_verif.h", "acg_verif_version", "ACG_VERIF_VERSION", "ops.reliability_summary"))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 20." in design and "fss_rel" in design and "Schwartz" in design
    header = open(os.path.join(ROOT, "include", "acgan_verif.h")).read()
    assert all(w in header for w in ("Murphy 1973", "Ferro 2014", "Schwartz & Sobash 2017", "tests/reliability_ref.py"))
    assert "test_hip_reliability.py" in open(os.path.join(ROOT, "README.md")).read()


def test_ops_refuses_on_the_host_before_any_device_call(monkeypatch):
    from dtgan_amd import _lib, ops

    def no_device(*a, **k):
        raise AssertionError("a refusal reached the library")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(_lib, "query", no_device)
    z = lambda *shape: torch.zeros(shape)
    thr = np.zeros((1, 2), np.float32)
    rel = lambda x, y, *a, **k: ops.reliability(x, y, 1, "nchw", "nchw", *a, **k)
    with pytest.raises(_lib.AcgError, match="reliability: need a 4-d"):
        ops.reliability(z(1, 1, 8, 8), z(1, 1, 8, 8), 1, "chwn", "nchw", thr, (1,))
    with pytest.raises(_lib.AcgError, match="reliability: need a 4-d"):
        rel(z(1, 8, 8), z(1, 1, 8, 8), thr, (1,))
    with pytest.raises(_lib.AcgError, match="1024"):
        rel(z(1, 1, 4, 1025), z(1, 1, 4, 1025), thr, (1,))
    with pytest.raises(_lib.AcgError, match="channels"):
        ops.reliability(z(2, 8, 8, 4), z(2, 8, 8, 4), 5, "nhwc", "nhwc", np.zeros((5, 1), np.float32), (1,))
    for per in (0, 3, 65, -1):
        with pytest.raises(_lib.AcgError, match="reliability: x_per_y"):
            rel(z(4, 1, 8, 8), z(4, 1, 8, 8), thr, (1,), x_per_y=per)
    with pytest.raises(_lib.AcgError, match="do not pair"):
        rel(z(4, 1, 8, 8), z(4, 1, 8, 8), thr, (1,), x_per_y=2)
    with pytest.raises(_lib.AcgError, match="do not pair"):
        rel(z(4, 1, 8, 8), z(2, 1, 8, 9), thr, (1,), x_per_y=2)
    for bad in ((), (2,), (0,), (1, 67), (1.5,), tuple(range(1, 19, 2))):
        with pytest.raises(_lib.AcgError, match="reliability: .*windows"):
            rel(z(2, 1, 8, 8), z(2, 1, 8, 8), thr, bad)
    for bad in (np.zeros((2, 2), np.float32), np.zeros(2, np.float32), np.zeros((1, 9), np.float32), np.zeros((1, 0), np.float32),
                torch.zeros(2, 2), torch.zeros(1, 2, dtype=torch.float64)):
        with pytest.raises(_lib.AcgError, match="reliability: thresholds"):
            rel(z(2, 1, 8, 8), z(2, 1, 8, 8), bad, (1,))
    i64 = torch.int64
    for bad in (torch.zeros(1, 1, 2, 1, 3, 2), torch.zeros(2, 1, 2, 1, 3, 2, dtype=i64), torch.zeros(1, 1, 2, 1, 2, 2, dtype=i64),
                torch.zeros(1, 1, 2, 1, 3, 4, dtype=i64)[..., ::2], torch.zeros(1, 1, 2, 2, 3, 2, dtype=i64)):
        with pytest.raises(_lib.AcgError, match="reliability: out"):
            rel(z(2, 1, 8, 8), z(1, 1, 8, 8), thr, (3,), x_per_y=2, out=bad)
    with pytest.raises(_lib.AcgError, match="ROCm device"):          # and a valid call has no CPU path
        rel(z(2, 1, 8, 8), z(1, 1, 8, 8), thr, (3,), x_per_y=2)
    with pytest.raises(_lib.AcgError, match="ROCm device"):
        rel(z(2, 1, 8, 8), z(1, 1, 8, 8), thr, (3,), x_per_y=2, out=torch.zeros(1, 1, 2, 1, 3, 2, dtype=i64))
