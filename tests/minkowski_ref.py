"""The definition of the counts behind the Minkowski functionals of excursion sets that acg_minkowski computes, in numpy
int64, a brute-force companion that works threshold by threshold with scipy.ndimage.label, and the fields and thresholds its
tests share.  No reference project states it.

For a field x of H x W cells and non-decreasing thresholds thr[0 .. T - 1]: the level of a pixel is L = #{t : thr[t] <= x}
(NaN: 0; x == thr counts), the excursion set at threshold t is {L >= t + 1}, and the field stands in a ring of level-0 cells.
F: the levels of the pixels; Emax / Emin: the max / min of the two pixels on either side of each of the H (W + 1) + (H + 1) W
unit edges; Vmax / Vmin: the max / min of the four pixels around each of the (H + 1) (W + 1) vertices.  n_X[t] = #{elements
of X with level >= t + 1}, and the counts are (nF, nE1, nE2, nV1, nV4) = (n_F, n_Emax, n_Emin, n_Vmax, n_Vmin).  Then
area = nF, perimeter = nE1 - nE2, euler8 = nV1 - nE1 + nF, euler4 = nF - nE2 + nV4."""
import numpy as np

KINDS = ("smooth", "constant", "special")


def levels(x, thr):
    """x (..., C, H, W) float32, thr (C, T) float32 non-decreasing -> (..., C, H, W) int64 in 0 .. T; NaN has level 0"""
    x = np.asarray(x, dtype=np.float32)
    thr = np.asarray(thr, dtype=np.float32)
    L = np.empty(x.shape, dtype=np.int64)
    for c in range(thr.shape[0]):
        L[..., c, :, :] = np.searchsorted(thr[c], x[..., c, :, :], side="right")
    L[np.isnan(x)] = 0                                             # searchsorted sorts NaN behind everything
    return L


def _suffix(lv, T):
    """lv (..., n) levels in 0 .. T -> (..., T): the number of elements with level >= t + 1"""
    lead = lv.shape[:-1]
    flat = lv.reshape(-1, lv.shape[-1])
    hist = np.stack([np.bincount(r, minlength=T + 1) for r in flat]).astype(np.int64)
    return hist[:, ::-1].cumsum(1)[:, ::-1][:, 1:].reshape(lead + (T,))


def counts(x, thr):
    """x (rows, C, H, W), thr (C, T) -> (rows, C, T, 5) int64: (nF, nE1, nE2, nV1, nV4)"""
    T = np.asarray(thr).shape[1]
    L = levels(x, thr)
    P = np.pad(L, [(0, 0)] * (L.ndim - 2) + [(1, 1), (1, 1)])      # the ring of level-0 cells
    lead = L.shape[:-2]
    ev = (P[..., 1:-1, :-1], P[..., 1:-1, 1:])                     # the H (W + 1) vertical edges: left and right pixel
    eh = (P[..., :-1, 1:-1], P[..., 1:, 1:-1])                     # the (H + 1) W horizontal edges: upper and lower pixel
    v = (P[..., :-1, :-1], P[..., :-1, 1:], P[..., 1:, :-1], P[..., 1:, 1:])
    flat = lambda a: a.reshape(lead + (-1,))
    both = lambda op: np.concatenate([flat(op(*ev)), flat(op(*eh))], -1)
    four = lambda op: flat(op(op(v[0], v[1]), op(v[2], v[3])))
    sets = (flat(L), both(np.maximum), both(np.minimum), four(np.maximum), four(np.minimum))
    return np.stack([_suffix(s, T) for s in sets], -1)


def functionals(n):
    """(..., 5) counts -> dict of int64 arrays (...): area, perimeter, euler4, euler8"""
    n = np.asarray(n, dtype=np.int64)
    nF, nE1, nE2, nV1, nV4 = (n[..., k] for k in range(5))
    return dict(area=nF, perimeter=nE1 - nE2, euler4=nF - nE2 + nV4, euler8=nV1 - nE1 + nF)


def _euler(mask, fg_structure, bg_structure):
    """foreground components minus holes: the holes are the background components of the doubly padded complement, less the
    one that reaches the outside"""
    from scipy import ndimage
    n_fg = ndimage.label(mask, structure=fg_structure)[1]
    n_bg = ndimage.label(~np.pad(mask, 2), structure=bg_structure)[1]
    return n_fg - (n_bg - 1)


def functionals_brute(x, thr):
    """one field x (H, W) and its thresholds thr (T,) -> dict of int64 arrays (T,): per threshold the mask [x >= thr[t]] (NaN
    compares false), its area, its perimeter from the explicit edge differences of the padded mask, and the Euler numbers
    from labelled components and holes: euler8 with 8-connected foreground and 4-connected background, euler4 the other way"""
    x = np.asarray(x, dtype=np.float32)
    thr = np.asarray(thr, dtype=np.float32)
    four = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)
    eight = np.ones((3, 3), dtype=bool)
    res = {k: np.zeros(thr.shape[0], dtype=np.int64) for k in ("area", "perimeter", "euler4", "euler8")}
    for t, v in enumerate(thr):
        with np.errstate(invalid="ignore"):
            mask = x >= v
        p = np.pad(mask, 1).astype(np.int64)
        res["area"][t] = mask.sum()
        res["perimeter"][t] = np.abs(np.diff(p, axis=0)).sum() + np.abs(np.diff(p, axis=1)).sum()
        res["euler8"][t] = _euler(mask, eight, four)
        res["euler4"][t] = _euler(mask, four, eight)
    return res


def _box_smooth(a, n):
    """n passes of a 3 x 3 box mean with wrap-around: noise with a correlation length, so components and holes exist"""
    for _ in range(n):
        a = sum(np.roll(np.roll(a, dy, -2), dx, -1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
    return a


def make_thresholds(C, T, seed=0, duplicates=False, lo=-1.0, hi=1.0):
    """(C, T) float32, per channel non-decreasing inside [lo, hi]; duplicates: every third threshold repeats its neighbour"""
    rs = np.random.RandomState(1000 + seed)
    thr = np.sort(rs.uniform(lo, hi, (C, T)), axis=1).astype(np.float32)
    if duplicates and T > 1:
        n = thr[:, 1::3].shape[1]
        thr[:, 1::3] = thr[:, 0::3][:, :n]
    return thr


def make_fields(kind, rows, C, H, W, thr, seed=0):
    """(rows, C, H, W) float32 fields for the thresholds thr (C, T):
      smooth    smoothed noise scaled to cross all thresholds;
      constant  one value per (row, channel), taken from the thresholds themselves (the bin every lane hits at once);
      special   smoothed noise with NaN, +-inf, values exactly on thresholds, and values just beside them"""
    rs = np.random.RandomState(seed + 7 * H + W)
    thr = np.asarray(thr, dtype=np.float32)
    T = thr.shape[1]
    x = _box_smooth(rs.standard_normal((rows, C, H, W)), 2)
    x = (x / max(np.abs(x).max(), 1e-6)).astype(np.float32) * 1.2
    if kind == "smooth":
        return x
    if kind == "constant":
        for r in range(rows):
            for c in range(C):
                x[r, c] = thr[c, (r * 5 + c) % T]
        return x
    assert kind == "special", kind
    pick = rs.uniform(size=x.shape)
    onthr = thr[np.arange(C)[None, :, None, None], rs.randint(0, T, x.shape)]
    x = np.where(pick < 0.25, onthr, x)
    x = np.where((pick >= 0.25) & (pick < 0.30), np.nextafter(onthr, np.float32(-np.inf)), x)
    x = np.where((pick >= 0.30) & (pick < 0.35), np.nextafter(onthr, np.float32(np.inf)), x)
    x = np.where((pick >= 0.35) & (pick < 0.45), np.nan, x)
    x = np.where((pick >= 0.45) & (pick < 0.50), np.inf, x)
    x = np.where((pick >= 0.50) & (pick < 0.55), -np.inf, x)
    return x.astype(np.float32)
