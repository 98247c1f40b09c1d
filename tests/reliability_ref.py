"""The definition of the reliability tables that acg_reliability computes, in numpy int64, the per-cell float64 evaluation
of the scores ops.reliability_summary derives from them, and the cases the tests share.  No reference project states it.

Events are fss_ref's: b = [x >= thr[c][t]], NaN is no event.  For an odd window n the neighbourhood event of a field is
b^n(i, j) = 1 iff any cell |i' - i| <= n/2, |j' - j| <= n/2 inside the domain is an event (the neighbourhood maximum of
Schwartz & Sobash 2017; equivalently fss_ref.box_counts > 0); n = 1 is the cell itself.  With M members per truth,
k(i, j) = sum_m b_m^n(i, j), o(i, j) = b^n of the truth, and table[k][o] is the number of cells with that pair: every
(M + 1, 2) table sums to H W.  From the tables (Murphy 1973; Ferro 2014) follow the Brier score of the forecast probability
k / M, its reliability - resolution + uncertainty decomposition (exact: the forecast takes M + 1 values, nothing is binned),
the fair Brier score and the ROC of the thresholds k >= j."""
import numpy as np

import fss_ref as F

# the largest |ops.reliability_summary - summary_cells| over the cases of tests/test_reliability_cpu.py (SUMMARY_CASES, every
# entry, measured there: the test prints it) was 1.11e-16, half an ulp of 1; the bar is 4 x that
SUMMARY_TOL = 4 * 1.11e-16

# (H, W, M, seed) of the summary comparison
SUMMARY_CASES = ((1, 1, 1, 0), (5, 7, 1, 1), (5, 7, 2, 2), (16, 16, 3, 3), (33, 31, 4, 4), (9, 70, 7, 5), (24, 24, 16, 6), (12, 12, 64, 7))
SUMMARY_KEYS = ("n", "prob", "obs_freq", "base_rate", "brier", "reliability", "resolution", "uncertainty", "bss", "brier_fair",
                "roc_hit", "roc_false", "auc")


def dilate(b, n):
    """the neighbourhood events of integer planes b (..., H, W) in {0, 1}: the OR over the offsets of the window, cells outside
    the domain contributing nothing; along the rows first, then down the columns (a square window's OR separates)"""
    H, W = b.shape[-2:]
    r = n // 2
    rows = np.zeros_like(b)
    for dj in range(-min(r, W - 1), min(r, W - 1) + 1):
        rows[..., max(dj, 0):W + min(dj, 0)] |= b[..., max(-dj, 0):W + min(-dj, 0)]
    out = np.zeros_like(b)
    for di in range(-min(r, H - 1), min(r, H - 1) + 1):
        out[..., max(di, 0):H + min(di, 0), :] |= rows[..., max(-di, 0):H + min(-di, 0), :]
    return out


def dilate_brute(b, n):
    """the same by loops over the cells (2-d b)"""
    H, W = b.shape
    r = n // 2
    out = np.zeros((H, W), dtype=np.int64)
    for i in range(H):
        for j in range(W):
            out[i, j] = int(b[max(i - r, 0):i + r + 1, max(j - r, 0):j + r + 1].any())
    return out


def planes(x, y, thr, n, x_per_y=1):
    """x (rows, C, H, W), y (rows / M, C, H, W), thr (C, T) -> k, o (rows / M, C, T, H, W) int64 at window n"""
    bx, by = dilate(F.events(x, thr), n), dilate(F.events(y, thr), n)
    return bx.reshape((by.shape[0], x_per_y) + bx.shape[1:]).sum(1), by


def table_of_planes(k, o, M):
    """(..., H, W) planes -> (..., M + 1, 2) int64"""
    lead = k.shape[:-2]
    idx = (k * 2 + o).reshape(lead + (-1,))
    flat = idx.reshape(-1, idx.shape[-1])
    t = np.stack([np.bincount(row, minlength=2 * (M + 1)) for row in flat]).astype(np.int64)
    return t.reshape(lead + (M + 1, 2))


def tables(x, y, thr, windows, x_per_y=1):
    """-> (rows / x_per_y, C, T, nw, M + 1, 2) int64"""
    return np.stack([table_of_planes(*planes(x, y, thr, n, x_per_y), M=x_per_y) for n in windows], -3)


def tables_brute(x, y, thr, windows, x_per_y=1):
    """the same by loops over fields and cells"""
    x, y, thr = np.asarray(x, np.float32), np.asarray(y, np.float32), np.asarray(thr, np.float32)
    rows, C, H, W = x.shape
    M, T = x_per_y, thr.shape[1]
    out = np.zeros((rows // M, C, T, len(windows), M + 1, 2), dtype=np.int64)
    for g in range(rows // M):
        for c in range(C):
            for t in range(T):
                for w, n in enumerate(windows):
                    with np.errstate(invalid="ignore"):
                        o = dilate_brute(y[g, c] >= thr[c, t], n)
                        k = sum(dilate_brute(x[g * M + m, c] >= thr[c, t], n) for m in range(M))
                    for i in range(H):
                        for j in range(W):
                            out[g, c, t, w, k[i, j], o[i, j]] += 1
    return out


def summary_cells(k, o, M):
    """the scores cell by cell in float64: k (cells,) in 0..M, o (cells,) in {0, 1} -> dict with ops.reliability_summary's keys"""
    k, o = np.asarray(k).reshape(-1).astype(np.int64), np.asarray(o).reshape(-1).astype(np.int64)
    cells = k.size
    p, of = k / float(M), o.astype(np.float64)
    n = np.bincount(k, minlength=M + 1).astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        obs = np.array([of[k == v].mean() if n[v] else np.nan for v in range(M + 1)])
        base = of.mean()
        brier = ((p - of) ** 2).mean()
        rel = ((p - obs[k]) ** 2).sum() / cells
        res = ((obs[k] - base) ** 2).sum() / cells
        unc = base * (1.0 - base)
        bss = 1.0 - brier / unc if unc > 0 else np.nan
        fair = ((p - of) ** 2 - k * (M - k) / (float(M) * M * (M - 1))).mean() if M > 1 else np.nan
        n1, n0 = int(o.sum()), int(cells - o.sum())
        js = range(M + 1, -1, -1)
        hit = np.array([(k[o == 1] >= j).mean() if n1 else np.nan for j in js])
        false = np.array([(k[o == 0] >= j).mean() if n0 else np.nan for j in js])
        auc = auc_mann_whitney(k, o)
    return dict(n=n, prob=np.arange(M + 1) / float(M), obs_freq=obs, base_rate=base, brier=brier, reliability=rel, resolution=res,
                uncertainty=unc, bss=bss, brier_fair=fair, roc_hit=hit, roc_false=false, auc=auc)


def auc_mann_whitney(k, o):
    """the probability that a cell with the event has more members in it than one without, ties counting half: a count over
    all pairs (cells with, cells without); NaN where either class is empty"""
    k, o = np.asarray(k).reshape(-1), np.asarray(o).reshape(-1)
    a, b = k[o == 1], k[o == 0]
    if not a.size or not b.size:
        return np.nan
    wins = sum(int((v > b).sum()) for v in a)
    ties = sum(int((v == b).sum()) for v in a)
    return (wins + 0.5 * ties) / (float(a.size) * b.size)


def summary_case(H, W, M, seed):
    """-> k, o (H W,) of one smooth truth and M displaced, perturbed members at a threshold a fifth of the cells exceed"""
    rs = np.random.RandomState(100 + seed)
    y = F.smooth_field(H, W, seed=seed, passes=2 if min(H, W) > 2 else 0)
    x = np.stack([np.roll(y, (m % 3 - 1, m % 2), (0, 1)) + 0.6 * rs.standard_normal((H, W)).astype(np.float32) for m in range(M)])
    thr = np.array([[np.quantile(y, 0.8)]], dtype=np.float32)
    k, o = planes(x[:, None], y[None, None], thr, 3 if min(H, W) > 2 else 1, x_per_y=M)
    return k.reshape(-1), o.reshape(-1)
