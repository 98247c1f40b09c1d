"""The definition of what acg_components computes, with scipy.ndimage.label, and the fields its tests share.  No reference
project states it.

A plane is one (field row, channel c, threshold t); its set is the mask minkowski_ref.levels(x, thr) >= t + 1, that is
[x >= thr[c][t]] with NaN outside and x == thr inside.  Its components under 4-connectivity (the cross structure) or
8-connectivity (the full 3 x 3 structure) give COMP_STATS = 25 int64 values: n, the number of components; area, the cells in
the set; sum_sq, the sum of the components' squared areas; n_border, the components with a cell in the first or last row or
column; hist[b], b = 0 .. 20, the components with floor(log2(area)) == b.  The canonical label of a cell is 0 outside the set
and 1 + the row-major index of the first cell of its component inside."""
import functools

import numpy as np

import minkowski_ref as K

COMP_STATS, COMP_BINS = 25, 21
TH, TW = 32, 64            # the kernel's tile (csrc/components.hip CC_TH, CC_TW): where `corners` puts its pairs
BINARY = ("full", "empty", "checker", "rings", "diag", "spiral", "comb", "perc41", "perc59", "corners")
KINDS = K.KINDS + BINARY
_STRUCTURE = {4: np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool), 8: np.ones((3, 3), dtype=bool)}


def plane(mask, conn, labels=False):
    """one boolean mask (H, W) -> its 25 int64 values [, its canonical labels (H, W) int32]"""
    from scipy import ndimage
    H, W = mask.shape
    lab, n = ndimage.label(mask, structure=_STRUCTURE[conn])
    out = np.zeros(COMP_STATS, dtype=np.int64)
    if n:
        areas = np.bincount(lab.ravel(), minlength=n + 1)[1:].astype(np.int64)
        edge = np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))
        out[0], out[1], out[2], out[3] = n, areas.sum(), (areas * areas).sum(), np.count_nonzero(edge)
        out[4:] = np.bincount(np.floor(np.log2(areas)).astype(np.int64), minlength=COMP_BINS)
    if not labels:
        return out
    first = np.full(n + 1, H * W, dtype=np.int64)
    np.minimum.at(first, lab.ravel(), np.arange(H * W))
    return out, np.where(lab > 0, first[lab] + 1, 0).astype(np.int32)


def stats(x, thr, conn, labels=False):
    """x (rows, C, H, W), thr (C, T) -> (rows, C, T, 25) int64 [, (rows, C, T, H, W) int32 canonical labels]"""
    x = np.asarray(x, dtype=np.float32)
    rows, C, H, W = x.shape
    T = np.asarray(thr).shape[1]
    L = K.levels(x, thr)
    out = np.zeros((rows, C, T, COMP_STATS), dtype=np.int64)
    lab = np.zeros((rows, C, T, H, W), dtype=np.int32) if labels else None
    for r in range(rows):
        for c in range(C):
            for t in range(T):
                res = plane(L[r, c] >= t + 1, conn, labels)
                if labels:
                    out[r, c, t], lab[r, c, t] = res
                else:
                    out[r, c, t] = res
    return (out, lab) if labels else out


def _spiral(H, W):
    """a one-cell-wide arm from the top left corner inwards, clockwise, one cell of gap between its turns"""
    a = np.zeros((H, W), dtype=bool)
    y = x = 0
    dy, dx = 0, 1
    a[0, 0] = True
    inside = lambda i, j: 0 <= i < H and 0 <= j < W
    while True:
        for _ in range(2):
            ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(ny, nx) and not a[ny, nx] and not (inside(fy, fx) and a[fy, fx]):
                break
            dy, dx = dx, -dy                                       # turn right
        else:
            return a
        y, x = ny, nx
        a[y, x] = True


@functools.lru_cache(maxsize=None)
def mask(kind, H, W, seed=0):
    """the boolean mask (H, W) of a binary kind; read-only"""
    y, x = np.mgrid[0:H, 0:W]
    if kind == "full":
        m = np.ones((H, W), dtype=bool)
    elif kind == "empty":
        m = np.zeros((H, W), dtype=bool)
    elif kind == "checker":
        m = (y + x) % 2 == 0
    elif kind == "rings":                                          # square rings at every second distance from the border
        m = np.minimum(np.minimum(y, x), np.minimum(H - 1 - y, W - 1 - x)) % 2 == 0
    elif kind == "diag":
        m = (y + x) % 3 == 0
    elif kind == "spiral":
        m = _spiral(H, W)
    elif kind == "comb":
        m = (x % 2 == 0) | (y == H - 1)
    elif kind in ("perc41", "perc59"):
        m = np.random.RandomState(41 + seed + 3 * H + W).uniform(size=(H, W)) < (0.41 if kind == "perc41" else 0.59)
    else:
        assert kind == "corners", kind
        m = np.zeros((H, W), dtype=bool)
        for i, r0 in enumerate(range(TH, H, TH)):
            for j, c0 in enumerate(range(TW, W, TW)):
                if (i + j) % 2 == 0:
                    m[r0 - 1, c0 - 1] = m[r0, c0] = True           # the main diagonal across the corner
                else:
                    m[r0 - 1, c0] = m[r0, c0 - 1] = True           # the other one
    m.setflags(write=False)
    return m


def make_thresholds(kind, C, T, seed=0):
    """(C, T) float32: minkowski_ref.make_thresholds (repeats from T = 31 on) for its kinds; for the binary kinds, whose fields
    are +-1, the values -2 (every cell), 0 (the mask) and 2 (no cell) in turn, sorted"""
    if kind in K.KINDS:
        return K.make_thresholds(C, T, seed=seed, duplicates=T >= 31)
    return np.tile(np.sort(np.array([0.0, -2.0, 2.0], dtype=np.float32)[np.arange(T) % 3])[None], (C, 1))


def make_fields(kind, rows, C, H, W, thr, seed=0):
    """(rows, C, H, W) float32: minkowski_ref.make_fields for its kinds, else +1 on the kind's mask and -1 off it (the noise
    kinds draw a mask per field)"""
    if kind in K.KINDS:
        return K.make_fields(kind, rows, C, H, W, thr, seed=seed)
    x = np.empty((rows, C, H, W), dtype=np.float32)
    for r in range(rows):
        for c in range(C):
            x[r, c] = np.where(mask(kind, H, W, seed + 7 * (r * C + c) if kind.startswith("perc") else 0), 1.0, -1.0)
    return x
