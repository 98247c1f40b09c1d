"""The definition of the fractions-skill-score training loss that acg_fss_loss_fwd / acg_fss_loss_bwd and ops.fss_loss compute,
in fp64 numpy, its analytic gradient, a float32 restatement that sets the bars of the device tests, and the cases the tests
share.  No reference project states it (Roberts & Lean 2008; Ebert-Uphoff et al. 2021; Lagerquist & Ebert-Uphoff 2022).

x (N, C, H, W) forecasts, y the paired truths, thr (C, T), nw odd windows n, a temperature tau > 0:
  p = 1 / (1 + exp(-(x - thr[c][t]) / tau)), q the same of y (on the device: fp32 in exactly this form with 1 / tau a float,
      saturating to exactly 0 and 1; NaN is not masked);
  cf(i, j) = sum of p over the cells |i' - i| <= n/2, |j' - j| <= n/2 inside the domain (cells outside count 0, / n^2 is never
      formed: fss_ref.box_counts on real planes), co of q;
  num[n, c, t, w] = sum over cells (cf - co)^2, den = sum over cells (cf^2 + co^2);
  Num = sum_n num, Den = sum_n den (pooled over the batch before dividing, as ops.fss_summary pools a split),
  R = Num / Den = 1 - FSS, 0 where Den == 0 exactly; loss = mean of R over C, T, nw.
Gradient (B_n, the window sum, is symmetric; the inner plane lives on the domain's cells only):
  a = 2 (1 - R) / Den, b = 2 / Den (0 where Den == 0),
  d loss / d x(q) = 1 / (C T nw) sum_t p_t (1 - p_t) / tau sum_w B_n(a cf - b co)(q);  y gets none."""
import numpy as np

import fss_ref

MAX_WINDOW = 65
TILE = 32                                # the kernels' tile extent: sizes around it are among the cases


def box_sum(b, n, dtype=np.float64, order="sequential"):
    """the window sums of real planes b (..., H, W) in `dtype`: n terms along the row, then n terms down the column, cells
    outside the domain 0; order 'sequential' adds the terms in ascending order, 'pairwise' by a balanced tree"""
    r = n // 2
    out = np.asarray(b, dtype=dtype)
    for axis in (-1, -2):
        L = out.shape[axis]
        pad = [(0, 0)] * out.ndim
        pad[axis] = (r, r)
        padded = np.pad(out, pad)
        terms = [np.take(padded, np.arange(k, k + L), axis=axis) for k in range(n)]
        if order == "sequential":
            acc = np.zeros_like(out)
            for t in terms:
                acc = acc + t
        elif order == "pairwise":
            while len(terms) > 1:
                terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
            acc = terms[0]
        else:
            raise ValueError(order)
        out = acc.astype(dtype)
    return out


def soft_events(x, thr, tau):
    """x (..., C, H, W), thr (C, T) -> (..., C, T, H, W) fp64"""
    x, thr = np.asarray(x, dtype=np.float64), np.asarray(thr, dtype=np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-(x[..., :, None, :, :] - thr[:, :, None, None]) / float(tau)))


def soft_events32(x, thr, tau):
    """the same in float32, in the device's form: 1 / (1 + exp(-(x - thr) inv_tau)) with inv_tau = float32(1 / tau)"""
    x, thr = np.asarray(x, dtype=np.float32), np.asarray(thr, dtype=np.float32)
    inv_tau, one = np.float32(1.0 / float(tau)), np.float32(1.0)
    with np.errstate(over="ignore", under="ignore"):
        return one / (one + np.exp(-(x[..., :, None, :, :] - thr[:, :, None, None]) * inv_tau))


def pool(num, den):
    """(N, C, T, nw) -> Num, Den, R (C, T, nw) and the loss"""
    Num, Den = num.sum(0), den.sum(0)
    some = Den != 0
    R = np.where(some, Num / np.where(some, Den, 1.0), 0.0)
    return Num, Den, R, R.mean()


def coefficients(R, Den):
    """a, b (C, T, nw), with the 1 / (C T nw) of the mean"""
    some = Den != 0
    inv = np.where(some, 1.0 / np.where(some, Den, 1.0), 0.0) / R.size
    return 2.0 * (1.0 - R) * inv, 2.0 * inv


def parts(x, y, thr, windows, tau):
    """-> num, den (N, C, T, nw) fp64"""
    p, q = soft_events(x, thr, tau), soft_events(y, thr, tau)
    num, den = [], []
    for n in windows:
        cf, co = box_sum(p, n), box_sum(q, n)
        num.append(((cf - co) ** 2).sum((-2, -1)))
        den.append((cf ** 2 + co ** 2).sum((-2, -1)))
    return np.stack(num, -1), np.stack(den, -1)


def loss(x, y, thr, windows, tau):
    """-> dict(loss, R, Num, Den, num, den)"""
    num, den = parts(x, y, thr, windows, tau)
    Num, Den, R, l = pool(num, den)
    return dict(loss=l, R=R, Num=Num, Den=Den, num=num, den=den)


def grad(x, y, thr, windows, tau):
    """the analytic d loss / d x (N, C, H, W) fp64"""
    p, q = soft_events(x, thr, tau), soft_events(y, thr, tau)
    f = loss(x, y, thr, windows, tau)
    a, b = coefficients(f["R"], f["Den"])
    s = np.zeros_like(p)
    for w, n in enumerate(windows):
        aw, bw = a[None, :, :, w, None, None], b[None, :, :, w, None, None]
        s += box_sum(aw * box_sum(p, n) - bw * box_sum(q, n), n)
    return (p * (1.0 - p) / float(tau) * s).sum(2)


def parts32(x, y, thr, windows, tau, order="sequential"):
    """the float32 restatement of the forward: fp32 events, fp32 window sums in `order`, double sums over cells"""
    p, q = soft_events32(x, thr, tau), soft_events32(y, thr, tau)
    num, den = [], []
    for n in windows:
        cf = box_sum(p, n, np.float32, order).astype(np.float64)
        co = box_sum(q, n, np.float32, order).astype(np.float64)
        num.append(((cf - co) ** 2).sum((-2, -1)))
        den.append((cf ** 2 + co ** 2).sum((-2, -1)))
    return np.stack(num, -1), np.stack(den, -1)


def grad32(x, y, thr, windows, tau, order="sequential"):
    """the float32 restatement of the backward, on the coefficients of its own forward: u = float32(a p - b q) combined in
    double, fp32 window sums of u and of B_n u, the windows and then the thresholds added in float32"""
    p, q = soft_events32(x, thr, tau), soft_events32(y, thr, tau)
    _, Den, R, _ = pool(*parts32(x, y, thr, windows, tau, order))
    a, b = coefficients(R, Den)
    inv_tau, one = np.float32(1.0 / float(tau)), np.float32(1.0)
    s = np.zeros_like(p)
    for w, n in enumerate(windows):
        aw, bw = a[None, :, :, w, None, None], b[None, :, :, w, None, None]
        u = (aw * p.astype(np.float64) - bw * q.astype(np.float64)).astype(np.float32)
        s = s + box_sum(box_sum(u, n, np.float32, order), n, np.float32, order)
    out = np.zeros(np.asarray(x).shape, dtype=np.float32)
    for t in range(p.shape[2]):
        out = out + p[:, :, t] * (one - p[:, :, t]) * inv_tau * s[:, :, t]
    return out


def make_case(H, W, rows, C, T, kind="noise", seed=0):
    """x, y (rows, C, H, W) float32 of fss_ref.make_pair and thr (C, T) float32 spread over the values, the channels differing"""
    x, y, _ = fss_ref.make_pair(kind, H, W, rows=rows, C=C, seed=seed)
    thr = (np.linspace(-0.5, 1.5, T, dtype=np.float64)[None, :] if T > 1 else np.full((1, 1), 0.5)) + 0.125 * np.arange(C)[:, None]
    return x, y, thr.astype(np.float32)


def harden(x, thr, margin):
    """x with every value closer than margin to one of its channel's thresholds moved to 2 margin above that threshold
    (repeated, since thresholds closer than 3 margin to each other chain); asserts that none is left"""
    x = np.array(x, dtype=np.float32)
    for _ in range(thr.shape[1] + 1):
        for c in range(thr.shape[0]):
            for t in thr[c]:
                near = np.abs(x[:, c].astype(np.float64) - float(t)) < margin * 1.0001
                x[:, c][near] = np.float32(float(t) + 2.0 * margin)
    assert all((np.abs(x[:, c].astype(np.float64) - float(t)) >= margin).all() for c in range(thr.shape[0]) for t in thr[c])
    return x


# (H, W, rows, C, T, windows, tau, kind) of the device tests and of the float32 bars: the sizes at which the index arithmetic
# changes (one cell, one row, a window wider than the domain, the tile extent and its neighbours, 321 x 321 with more tiles
# than the fold's wave has lanes, a 1024-wide plane of a few rows), T and nw at 1 and 8, rows from 1
CASES = (
    (1, 1, 1, 1, 1, (1,), 0.25, "noise"),
    (1, 7, 2, 3, 2, (3, 9), 0.25, "noise"),
    (5, 7, 2, 3, 2, (9,), 0.25, "noise"),
    (33, 31, 2, 3, 1, (33, 65), 0.25, "noise"),
    (31, 33, 1, 1, 8, (5,), 0.25, "shifted"),
    (TILE, TILE, 3, 1, 2, (1, 3, 9), 0.05, "ties"),
    (TILE - 1, TILE - 1, 1, 3, 2, (17,), 0.25, "shifted"),
    (TILE + 1, TILE + 1, 1, 3, 2, (1, 3, 5, 7, 9, 11, 13, 15), 0.25, "noise"),
    (64, 64, 2, 3, 2, (3, 9, 17), 0.05, "shifted"),
    (65, 130, 1, 3, 2, (3, 9, 33), 0.25, "noise"),
    (321, 321, 1, 1, 2, (3, 17, 65), 0.25, "shifted"),
    (3, 1024, 1, 1, 1, (9, 65), 0.25, "noise"),
)


def measure_bars(cases=CASES, orders=("sequential", "pairwise")):
    """the float32 restatement against the fp64 definition -> {order: (forward, gradient)}: the largest |num32 - num| / den and
    |den32 - den| / den over the cases, and the largest |grad32 - grad| / max |grad| (this is how FWD_MEASURED and GRAD_MEASURED
    below were obtained)"""
    res = {}
    for order in orders:
        fwd = bwd = 0.0
        for (H, W, rows, C, T, windows, tau, kind) in cases:
            x, y, thr = make_case(H, W, rows, C, T, kind)
            num, den = parts(x, y, thr, windows, tau)
            num32, den32 = parts32(x, y, thr, windows, tau, order)
            ok = den > 0
            fwd = max(fwd, (np.abs(num32 - num)[ok] / den[ok]).max(), (np.abs(den32 - den)[ok] / den[ok]).max())
            g = grad(x, y, thr, windows, tau)
            if np.abs(g).max() > 0:
                bwd = max(bwd, np.abs(grad32(x, y, thr, windows, tau, order) - g).max() / np.abs(g).max())
        res[order] = (float(fwd), float(bwd))
    return res


# measure_bars() on CASES: {order: (forward relative to den, gradient relative to the largest |gradient| of the case)}
FWD_MEASURED = {"sequential": 2.61e-07, "pairwise": 2.09e-07}
GRAD_MEASURED = {"sequential": 4.50e-07, "pairwise": 2.97e-07}
# the device's bars: 4 x the worse of the two orders; the factor covers the device's expf and its own summation order
FWD_BAR = 4.0 * max(FWD_MEASURED.values())
GRAD_BAR = 4.0 * max(GRAD_MEASURED.values())
