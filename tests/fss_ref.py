"""The definition of the fractions-skill-score triples (Roberts & Lean 2008) that acg_fss computes, in numpy int64, and the
fields and cases its tests share.  No reference project states it.

For a field x of H x W cells, a threshold t and an odd window n: the event plane is b = [x >= t] (NaN is no event), the count
plane c(i, j) = sum of b over the cells |i' - i| <= n/2, |j' - j| <= n/2 inside the domain (cells outside count 0; the
fraction c / n^2 is never formed).  For a forecast x and truth y the triple is (sum cf^2, sum co^2, sum cf co) over the cells.
For M members sharing a truth, E = sum_m cf_m and the ensemble triple is (sum E^2, sum co^2, sum E co)."""
import numpy as np

# (H, W) of the equality test; 256 and 321 are the evaluator's and the native grid, 65 x 130 has two and three words per row
SIZES = ((1, 1), (5, 7), (16, 16), (33, 31), (64, 64), (65, 130), (256, 256), (321, 321))
WINDOWS = (1, 3, 9, 33, 65)
KINDS = ("noise", "shifted", "ties", "nan", "extremes")
# thresholds (C, T) and windows of the model-level tests (translate_fss on the fields of a tiny generator, in [-1, 1])
THR = np.array([[-0.1, 0.0, 0.2], [-0.2, 0.05, 0.3], [0.0, 0.1, 0.5]], dtype=np.float32)
WIN = (1, 3, 9, 33)


def events(x, thr):
    """x (..., C, H, W), thr (C, T) -> (..., C, T, H, W) int64 in {0, 1}; NaN compares false"""
    x = np.asarray(x, dtype=np.float32)
    thr = np.asarray(thr, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (x[..., :, None, :, :] >= thr[:, :, None, None]).astype(np.int64)


def box_counts(b, n):
    """the window counts of integer planes b (..., H, W) by a summed-area table, int64"""
    H, W = b.shape[-2:]
    r = n // 2
    sat = np.zeros(b.shape[:-2] + (H + 1, W + 1), dtype=np.int64)
    sat[..., 1:, 1:] = b.cumsum(-2).cumsum(-1)
    i0, i1 = np.clip(np.arange(H) - r, 0, H), np.clip(np.arange(H) + r + 1, 0, H)
    j0, j1 = np.clip(np.arange(W) - r, 0, W), np.clip(np.arange(W) + r + 1, 0, W)
    return (sat[..., i1[:, None], j1[None, :]] - sat[..., i0[:, None], j1[None, :]] - sat[..., i1[:, None], j0[None, :]]
            + sat[..., i0[:, None], j0[None, :]])


def box_counts_brute(b, n):
    """the same by loops over the window's cells (2-d b)"""
    H, W = b.shape
    r = n // 2
    c = np.zeros((H, W), dtype=np.int64)
    for i in range(H):
        for j in range(W):
            c[i, j] = b[max(i - r, 0):i + r + 1, max(j - r, 0):j + r + 1].sum()
    return c


def triples_of_counts(cf, co):
    """(..., H, W) count planes -> (..., 3) int64"""
    return np.stack([(cf * cf).sum((-2, -1)), (co * co).sum((-2, -1)), (cf * co).sum((-2, -1))], -1)


def triples(x, y, thr, windows, x_per_y=1):
    """x (rows, C, H, W), y (rows / x_per_y, C, H, W), thr (C, T) -> (rows, C, T, nw, 3) int64"""
    bx, by = events(x, thr), np.repeat(events(y, thr), x_per_y, axis=0)
    return np.stack([triples_of_counts(box_counts(bx, n), box_counts(by, n)) for n in windows], -2)


def ens_triples(x, y, thr, windows, x_per_y):
    """the triples of the summed event planes e = sum_m b_m of every truth's members -> (rows / x_per_y, C, T, nw, 3) int64"""
    bx, by = events(x, thr), events(y, thr)
    e = bx.reshape((by.shape[0], x_per_y) + bx.shape[1:]).sum(1)
    return np.stack([triples_of_counts(box_counts(e, n), box_counts(by, n)) for n in windows], -2)


def summary(sums, windows, cells, members=1):
    """(..., T, nw, 3) summed triples -> dict(fss (..., T, nw); with 1 among the windows bias, csi, base_rate (..., T) and
    useful_scale (..., T) int64), in float64.  members = M: FSS_prob = 2 M sum E co / (sum E^2 + M^2 sum co^2), and the n = 1
    forecast count and hits are divided by M"""
    t = np.asarray(sums).astype(np.float64)
    M = float(members)
    ff, oo, fo = t[..., 0], t[..., 1], t[..., 2]
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        den = ff + M * M * oo
        out["fss"] = np.where(den > 0, 2 * M * fo / den, np.nan)
        if 1 in windows:
            k = list(windows).index(1)
            f, o, h = ff[..., k] / M, oo[..., k], fo[..., k] / M
            out["bias"] = np.where(o > 0, f / o, np.nan)
            out["csi"] = np.where(f + o - h > 0, h / (f + o - h), np.nan)
            out["base_rate"] = o / cells
            scale = np.zeros(out["bias"].shape, dtype=np.int64)
            for n in sorted(windows, reverse=True):
                ok = out["fss"][..., list(windows).index(n)] >= 0.5 + out["base_rate"] / 2
                scale = np.where(ok, n, scale)
            out["useful_scale"] = scale
    return out


def fss_float(x, y, t, n):
    """the float definition for one pair of 2-d fields: 1 - sum (Pf - Po)^2 / (sum Pf^2 + sum Po^2), P = c / n^2"""
    pf = box_counts((x >= t).astype(np.int64), n) / float(n * n)
    po = box_counts((y >= t).astype(np.int64), n) / float(n * n)
    return 1.0 - ((pf - po) ** 2).sum() / ((pf ** 2).sum() + (po ** 2).sum())


def smooth_field(H, W, seed=0, passes=3):
    """white noise box-filtered a few times with periodic wrap and scaled to unit variance: features a few cells wide"""
    x = np.random.RandomState(seed).standard_normal((H, W))
    for _ in range(passes):
        x = sum(np.roll(np.roll(x, di, 0), dj, 1) for di in (-1, 0, 1) for dj in (-1, 0, 1)) / 9.0
    return (x / max(x.std(), 1e-12)).astype(np.float32)


def make_pair(kind, H, W, rows=2, C=3, seed=0):
    """-> x, y (rows, C, H, W) float32 and thr (C, 3) float32.  Every threshold set holds one nothing exceeds (or, for `ties`,
    one met exactly by many cells) and one everything exceeds."""
    rs = np.random.RandomState(seed + 17 * H + W)
    lo_hi = lambda mid: np.tile(np.array([mid, 1e30, -1e30], dtype=np.float32), (C, 1))
    if kind == "noise":
        x, y = rs.standard_normal((2, rows, C, H, W)).astype(np.float32)
        thr = lo_hi(0.5)
        thr[:, 0] += np.arange(C, dtype=np.float32) * 0.25         # the channels differ
    elif kind == "shifted":
        y = np.stack([[smooth_field(H, W, seed=seed + 10 * r + c) for c in range(C)] for r in range(rows)])
        x = np.roll(np.roll(y, 2, -2), 3, -1)                      # the truth displaced by (2, 3) cells
        thr = lo_hi(1.0)
    elif kind == "ties":
        x, y = rs.randint(-2, 3, (2, rows, C, H, W)).astype(np.float32) * 0.5
        thr = lo_hi(0.5)                                           # a quarter of the cells sit exactly on it
        thr[:, 1] = 1.0                                            # the largest value present: met, never exceeded
    elif kind == "nan":
        x, y = rs.standard_normal((2, rows, C, H, W)).astype(np.float32)
        x[rs.uniform(size=x.shape) < 0.1] = np.nan
        y[rs.uniform(size=y.shape) < 0.05] = np.nan
        x[:, :, 0, 0] = np.inf
        thr = lo_hi(0.0)
    elif kind == "extremes":
        x = np.full((rows, C, H, W), -3.0, dtype=np.float32)       # all below against all above, in turn
        y = np.full((rows, C, H, W), 3.0, dtype=np.float32)
        x[1::2], y[1::2] = 3.0, -3.0
        thr = lo_hi(0.0)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x), np.ascontiguousarray(y), thr


def case_windows(H, W):
    """the listed windows and one that covers the whole domain from every cell"""
    return WINDOWS + (2 * max(H, W) - 1,)
