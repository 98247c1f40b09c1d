"""Float64 NumPy restatement of the ensemble statistics (acg_ensemble_stats, model.translate_ensemble): the reference the
kernel and the model API are checked against."""
import numpy as np


def e2_sorted(xs):
    """E2 = (1/M^2) sum_ij |x_i - x_j| in its sorted form (2/M^2) sum_i (2i - M - 1) x_(i), members on the last axis"""
    x = np.sort(np.asarray(xs, dtype=np.float64), axis=-1)
    M = x.shape[-1]
    coef = 2.0 * np.arange(1, M + 1) - M - 1
    return 2.0 / M ** 2 * (x * coef).sum(-1)


def e2_pairs(xs):
    """the same by the double sum"""
    x = np.asarray(xs, dtype=np.float64)
    return np.abs(x[..., :, None] - x[..., None, :]).sum((-1, -2)) / x.shape[-1] ** 2


def quantile_linear(xs, q):
    """numpy's default (linear) rule: h = (M - 1) q, x_floor(h) + (h - floor(h)) (x_ceil(h) - x_floor(h))"""
    x = np.sort(np.asarray(xs, dtype=np.float64), axis=-1)
    M = x.shape[-1]
    h = (M - 1) * float(q)
    lo, hi = int(np.floor(h)), int(np.ceil(h))
    return x[..., lo] + (h - lo) * (x[..., hi] - x[..., lo])


def ensemble_stats(members, target, quantiles):
    """members (N, M, C, H, W), target (N, C, H, W) or None -> dict of float64 / int64 arrays: mean, std (N, C, H, W),
    quantiles (N, nq, C, H, W) and, with a target, crps_map (N, C, H, W), sums (N, 6), rank_hist (N, M + 1) and the derived
    per-input crps, crps_fair, mse_mean, spread, coverage"""
    x = np.asarray(members, dtype=np.float64)
    N, M = x.shape[:2]
    xm = np.moveaxis(x, 1, -1)                                   # (N, C, H, W, M)
    out = dict(mean=xm.mean(-1), std=xm.std(-1, ddof=1) if M > 1 else np.zeros(xm.shape[:-1]),
               quantiles=np.stack([quantile_linear(xm, q) for q in quantiles], 1))
    if target is None:
        return out
    y = np.asarray(target, dtype=np.float64)
    e1 = np.abs(xm - y[..., None]).mean(-1)
    e2 = e2_sorted(xm)
    out["crps_map"] = e1 - e2 / 2
    qlo, qhi = out["quantiles"][:, 0], out["quantiles"][:, -1]
    cells = float(np.prod(y.shape[1:]))
    flat = lambda a: a.reshape(N, -1)
    sums = np.stack([flat(e1).sum(1), flat(e2).sum(1), flat((out["mean"] - y) ** 2).sum(1), flat(out["std"] ** 2).sum(1),
                     flat((qlo <= y) & (y <= qhi)).sum(1).astype(np.float64), np.full(N, cells)], 1)
    out["sums"] = sums
    rank = (xm < y[..., None]).sum(-1) + (xm == y[..., None]).sum(-1) // 2
    out["rank_hist"] = np.stack([np.bincount(flat(rank)[n], minlength=M + 1) for n in range(N)])
    out["crps"] = (sums[:, 0] - sums[:, 1] / 2) / cells
    out["crps_fair"] = (sums[:, 0] - sums[:, 1] * M / (2 * (M - 1))) / cells if M > 1 else np.full(N, np.nan)
    out["mse_mean"] = sums[:, 2] / cells
    out["spread"] = np.sqrt(sums[:, 3] / cells)
    out["coverage"] = sums[:, 4] / cells
    return out
