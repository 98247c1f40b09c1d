"""The definition of the intensity-scale triples (Casati et al. 2004; Casati 2010) that acg_fss_scales computes, in numpy
int64, beside fss_ref.py whose events and fields it shares.  No reference project states it.

For a field of H x W cells: L = ceil(log2(max(H, W))), nl = L + 1.  Level l = 0 .. L cuts the plane into blocks of 2^l x 2^l
cells anchored at cell (0, 0); blocks at the right and bottom edge are cut by the domain, which equals zero-padding the event
planes to 2^L x 2^L.  With bf, bo the events [x >= t], [y >= t] (NaN is no event) of forecast and truth in a block, the triple
of level l is (sum bf^2, sum bo^2, sum bf bo) over its blocks.  For M members sharing a truth the ensemble triple is
(sum E^2, sum bo^2, sum E bo), E the block count of the summed member planes.  Level 0 is (n_f, n_o, hits) (the window-1
triple of fss_ref.triples), level L is (n_f^2, n_o^2, n_f n_o).

summary() turns triples summed over a set of pairs into the Haar component energies of the error field: with D_l = ff_l / M^2
+ oo_l - 2 fo_l / M (the sum over the blocks of level l of the squared block sums of the error), the component "mean over 2^j
blocks minus mean over 2^(j+1) blocks" has the energy (4 D_j - D_{j+1}) / 4^(j+1) per canvas, and the mean term D_L / 4^L;
haar_mse() states the same by an explicit decomposition in float64."""
import numpy as np

import fss_ref as F

# (H, W) of the equality test: one cell, single rows and columns, both sides of the 64-cell word and tile, several tiles per
# side, the evaluator's 256 and the native 321
SIZES = ((1, 1), (1, 7), (5, 1), (2, 2), (63, 65), (64, 64), (65, 64), (64, 128), (129, 1), (100, 37), (256, 256), (321, 321))


def levels(H, W):
    """nl = L + 1, L = ceil(log2(max(H, W)))"""
    return int(max(H, W) - 1).bit_length() + 1


def block_counts(b, l):
    """integer planes b (..., H, W) -> the sums over the blocks of 2^l x 2^l cells anchored at (0, 0), int64"""
    s = 1 << l
    H, W = b.shape[-2:]
    return np.add.reduceat(np.add.reduceat(b.astype(np.int64), np.arange(0, H, s), -2), np.arange(0, W, s), -1)


def triples_of_planes(bx, by):
    """(..., H, W) event (or exceedance-count) planes -> (..., nl, 3) int64"""
    nl = levels(*bx.shape[-2:])
    return np.stack([F.triples_of_counts(block_counts(bx, l), block_counts(by, l)) for l in range(nl)], -2)


def triples(x, y, thr, x_per_y=1):
    """x (rows, C, H, W), y (rows / x_per_y, C, H, W), thr (C, T) -> (rows, C, T, nl, 3) int64"""
    return triples_of_planes(F.events(x, thr), np.repeat(F.events(y, thr), x_per_y, axis=0))


def ens_triples(x, y, thr, x_per_y):
    """the triples of the summed event planes of every truth's members -> (rows / x_per_y, C, T, nl, 3) int64"""
    bx, by = F.events(x, thr), F.events(y, thr)
    return triples_of_planes(bx.reshape((by.shape[0], x_per_y) + bx.shape[1:]).sum(1), by)


def component_energies(s, cells):
    """s (..., nl): the summed squared block sums of a field per level -> the energies of its Haar components per cell"""
    L = s.shape[-1] - 1
    num = np.concatenate([4 * s[..., :-1] - s[..., 1:], 4 * s[..., -1:]], -1)
    return num.astype(np.float64) / 4.0 ** np.arange(1, L + 2) / float(cells)


def summary(sums, cells, members=1, forecast_events=None):
    """(..., T, nl, 3) summed triples -> dict(mse, iss, en_rel (..., T, nl); mse_random (..., T); skill_scale (..., T) int64).
    members = M > 1: the triples are an ensemble's, and forecast_events (..., T) gives the members' events n_f"""
    t = np.asarray(sums).astype(np.int64)
    M = int(members)
    L = t.shape[-2] - 1
    ff, oo, fo = t[..., 0], t[..., 1], t[..., 2]
    if M == 1:
        D = ff + oo - 2 * fo                                       # int64: 4 D_j - D_{j+1} is exact
        n_f = ff[..., 0]
    else:
        D = ff / float(M * M) + oo - 2.0 * fo / M
        n_f = np.asarray(forecast_events)
    out = dict(mse=component_energies(D, cells))
    e_f, e_o = n_f / float(M * cells), oo[..., 0] / float(cells)
    out["mse_random"] = ff[..., 0] / float(M * M * cells) - 2 * e_f * e_o + e_o
    en_f, en_o = component_energies(ff / float(M * M), cells), component_energies(oo, cells)
    with np.errstate(divide="ignore", invalid="ignore"):
        rnd = out["mse_random"][..., None]
        out["iss"] = np.where(rnd != 0, 1.0 - out["mse"] * (L + 1) / rnd, np.nan)
        out["en_rel"] = np.where(en_f + en_o != 0, (en_f - en_o) / (en_f + en_o), np.nan)
    scale = np.full(out["mse_random"].shape, 1 << L, dtype=np.int64)
    for idx in np.ndindex(scale.shape):
        for j in range(L - 1, -1, -1):                             # down from the largest mother scale while skill stays
            if not out["iss"][idx][j] > 0:
                break
            scale[idx] = 1 << j
    out["skill_scale"] = scale
    return out


def haar_mse(e):
    """the explicit decomposition of one error field e (H, W) float64: zero-pad to 2^L x 2^L, m_j = the means over the 2^j
    blocks, and per j < L the sum over the canvas of (m_j - m_{j+1} spread over its four children)^2, then of m_L^2 -> (nl,)
    sums of squares (divide by the real cells for the MSE per cell)"""
    H, W = e.shape
    L = levels(H, W) - 1
    n = 1 << L
    canvas = np.zeros((n, n), dtype=np.float64)
    canvas[:H, :W] = e
    means = [canvas.reshape(n >> j, 1 << j, n >> j, 1 << j).mean((1, 3)) for j in range(L + 1)]
    parts = [((means[j] - np.kron(means[j + 1], np.ones((2, 2)))) ** 2).sum() * 4.0 ** j for j in range(L)]
    return np.array(parts + [(means[L] ** 2).sum() * 4.0 ** L])
