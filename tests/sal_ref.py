"""The definition of what acg_sal and ops.sal_scores compute: the SAL score of Wernli et al. (2008), structure, amplitude and
location of the objects of a field, in numpy with scipy.ndimage.label, and the fields its tests share.  No reference project
states it.

A plane is one (field row, channel c, threshold t); its set is [x >= thr[c][t]] with NaN outside and x == thr inside, its
objects are the components of the set under 4-connectivity (the cross structure) or 8-connectivity (the full 3 x 3 structure),
in the order of their first cells.  The mass of a cell is the fixed-point integer q = clamp(rint((x - floor) 2^20), 0, 2^24),
computed in float32 with every operation rounded on its own (NaN: 0, -inf: 0, +inf: 2^24), so that every sum of masses is an
exact int64 (H, W <= 1024: below 2^54).
  field (3,)  Q, QY, QX = sum of q, q h, q w over all H W cells (h the row, w the column);
  obj (4,)    n, the objects; area, the cells in the set; Robj = sum_n R_n; Rmax = max_n R_n (0 without an object), with
              R_n, Y_n, X_n = sum of q, q h, q w and P_n = max q over the cells of object n;
  shape (2,)  in float64, every integer converted first, over the objects with R_n > 0, summed in their order:
              SV = sum_n R_n (R_n / P_n) and SR = sum_n R_n sqrt((Y_n / R_n - QY / Q)^2 + (X_n / R_n - QX / Q)^2); 0.0 without one.
The scores of a pair (forecast f, observation o), with d = sqrt((H - 1)^2 + (W - 1)^2):
  A = (Q_f - Q_o) / (0.5 (Q_f + Q_o)), NaN when Q_f + Q_o = 0;   L1 = |c_f - c_o| / d with c = (QY / Q, QX / Q), NaN when either
  Q is 0, 0 when d = 0;   V = SV / Robj, S = (V_f - V_o) / (0.5 (V_f + V_o));   r = SR / Robj, L2 = 2 |r_f - r_o| / d;
  L = L1 + L2;   S, L2 and L are NaN when either side has Robj = 0.
Closed forms (tests/test_sal_cpu.py): a displaced block has S = A = L2 = 0 and L1 = the displacement over d; a block whose
height above the floor is scaled by 4/3 has S = L = 0 and A = 2/7; a plateau against a narrow peak of the same mass has S > 1."""
import functools

import numpy as np

import components_ref as R
import minkowski_ref as K

QBITS, QMAX = 20, 1 << 24
BINARY = ("spiral", "checker", "corners", "perc59", "rings")
KINDS = K.KINDS + BINARY


def quant(x, floor=-1.0):
    """float32 values -> their int64 masses"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.rint((x - np.float32(floor)) * np.float32(1 << QBITS))   # float32 throughout; rint rounds ties to even
    assert s.dtype == np.float32
    s = np.where(np.isnan(s), np.float32(0), s)
    return np.clip(s, np.float32(0), np.float32(QMAX)).astype(np.int64)


def field_sums(q):
    """q (H, W) int64 -> (3,) int64: Q, QY, QX"""
    H, W = q.shape
    h, w = np.arange(H, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    return np.array([q.sum(), (q * h).sum(), (q * w).sum()], dtype=np.int64)


def plane(mask, q, conn, fsum):
    """one boolean mask (H, W), the masses (H, W) and the field's (Q, QY, QX) -> obj (4,) int64, shape (2,) float64"""
    from scipy import ndimage
    H, W = mask.shape
    lab, n = ndimage.label(mask, structure=R._STRUCTURE[conn])
    obj, shape = np.zeros(4, dtype=np.int64), np.zeros(2, dtype=np.float64)
    if not n:
        return obj, shape
    first = np.full(n + 1, H * W, dtype=np.int64)
    np.minimum.at(first, lab.ravel(), np.arange(H * W))
    order = np.argsort(first[1:], kind="stable")                   # the objects by their first cells (scipy's order already)
    inside = lab.ravel() > 0
    idx = lab.ravel()[inside] - 1
    qq = q.ravel()[inside]
    hh, ww = np.divmod(np.flatnonzero(inside).astype(np.int64), W)
    Rn, Yn, Xn, Pn = (np.zeros(n, dtype=np.int64) for _ in range(4))
    np.add.at(Rn, idx, qq)
    np.add.at(Yn, idx, qq * hh)
    np.add.at(Xn, idx, qq * ww)
    np.maximum.at(Pn, idx, qq)
    Rn, Yn, Xn, Pn = Rn[order], Yn[order], Xn[order], Pn[order]
    obj[:] = n, inside.sum(), Rn.sum(), Rn.max()
    live = Rn > 0
    if live.any():
        Rd, Yd, Xd, Pd = (a[live].astype(np.float64) for a in (Rn, Yn, Xn, Pn))
        Q, QY, QX = (np.float64(v) for v in fsum)
        dy, dx = Yd / Rd - QY / Q, Xd / Rd - QX / Q
        shape[0] = np.cumsum(Rd * (Rd / Pd))[-1]                   # cumsum: one after the other
        shape[1] = np.cumsum(Rd * np.sqrt(dy * dy + dx * dx))[-1]
    return obj, shape


def sal(x, thr, conn, floor=-1.0):
    """x (rows, C, H, W), thr (C, T) -> field (rows, C, 3) int64, obj (rows, C, T, 4) int64, shape (rows, C, T, 2) float64"""
    x = np.asarray(x, dtype=np.float32)
    thr = np.asarray(thr, dtype=np.float32)
    rows, C, H, W = x.shape
    T = thr.shape[1]
    field = np.zeros((rows, C, 3), dtype=np.int64)
    obj = np.zeros((rows, C, T, 4), dtype=np.int64)
    shape = np.zeros((rows, C, T, 2), dtype=np.float64)
    for r in range(rows):
        for c in range(C):
            q = quant(x[r, c], floor)
            field[r, c] = field_sums(q)
            for t in range(T):
                if t and thr[c, t] == thr[c, t - 1]:
                    obj[r, c, t], shape[r, c, t] = obj[r, c, t - 1], shape[r, c, t - 1]
                    continue
                with np.errstate(invalid="ignore"):
                    mask = x[r, c] >= thr[c, t]
                obj[r, c, t], shape[r, c, t] = plane(mask, q, conn, field[r, c])
    return field, obj, shape


def scores_one(f, o, H, W):
    """two triples of ONE field each: field (C, 3), obj (C, T, 4), shape (C, T, 2) -> dict of float64 arrays S (C, T), A (C,),
    L1 (C,), L2 (C, T), L (C, T); plain loops, python floats"""
    import math
    nan = float("nan")
    C, T = f[1].shape[0], f[1].shape[1]
    d = math.sqrt((H - 1) ** 2 + (W - 1) ** 2)
    res = dict(S=np.full((C, T), nan), A=np.full(C, nan), L1=np.full(C, nan), L2=np.full((C, T), nan), L=np.full((C, T), nan))
    for c in range(C):
        qf, qo = int(f[0][c, 0]), int(o[0][c, 0])
        if qf + qo:
            res["A"][c] = (float(qf) - float(qo)) / (0.5 * (float(qf) + float(qo)))
        if qf and qo:
            cf = [float(f[0][c, k]) / float(qf) for k in (1, 2)]
            co = [float(o[0][c, k]) / float(qo) for k in (1, 2)]
            res["L1"][c] = math.sqrt((cf[0] - co[0]) ** 2 + (cf[1] - co[1]) ** 2) / d if d > 0 else 0.0
        for t in range(T):
            rf, ro = float(f[1][c, t, 2]), float(o[1][c, t, 2])
            if rf == 0 or ro == 0:
                continue
            vf, vo = float(f[2][c, t, 0]) / rf, float(o[2][c, t, 0]) / ro
            res["S"][c, t] = (vf - vo) / (0.5 * (vf + vo))
            res["L2"][c, t] = 2.0 * abs(float(f[2][c, t, 1]) / rf - float(o[2][c, t, 1]) / ro) / d if d > 0 else 0.0
            res["L"][c, t] = res["L1"][c] + res["L2"][c, t]
    return res


def pair_scores(xf, xo, thr, conn=8, floor=-1.0):
    """two single fields (C, H, W) -> scores_one of their triples"""
    H, W = xf.shape[-2:]
    f, o = (tuple(a[0] for a in sal(x[None], thr, conn, floor)) for x in (xf, xo))
    return scores_one(f, o, H, W)


def block(H, W, r0, c0, h, w, height, base=-1.0):
    """(1, H, W) float32: `height` on the h x w block at (r0, c0), `base` elsewhere"""
    x = np.full((1, H, W), base, dtype=np.float32)
    x[0, r0:r0 + h, c0:c0 + w] = height
    return x


def make_thresholds(kind, C, T, seed=0):
    """(C, T) float32: components_ref.make_thresholds (-2, 0, 2 in turn for the binary kinds, whose fields lie in (-1.5, 1])"""
    return R.make_thresholds(kind if kind in K.KINDS else "full", C, T, seed=seed)


@functools.lru_cache(maxsize=None)
def _weights(H, W, seed):
    u = np.random.RandomState(90 + seed + 5 * H + W).uniform(size=(2, H, W)).astype(np.float32)
    u.setflags(write=False)
    return u


def make_fields(kind, rows, C, H, W, thr, seed=0):
    """(rows, C, H, W) float32: minkowski_ref.make_fields for its kinds; for a binary kind values in [0.25, 1] on the kind's mask
    of components_ref and in (-1.5, -0.5] off it (some below the floor -1), so that the objects at threshold 0 are the mask's
    with unequal masses"""
    if kind in K.KINDS:
        return K.make_fields(kind, rows, C, H, W, thr, seed=seed)
    x = np.empty((rows, C, H, W), dtype=np.float32)
    for r in range(rows):
        for c in range(C):
            s = seed + 7 * (r * C + c)
            u = _weights(H, W, s)
            x[r, c] = np.where(R.mask(kind, H, W, s if kind.startswith("perc") else 0), 0.25 + 0.75 * u[0], -0.5 - u[1])
    return x


def check(got, ref, what):
    """field and obj equal; shape within (n + 8) 2^-52 of the reference, relatively: the terms are non-negative and built from
    equal integers, the sums differ in the order of n - 1 additions; exactly 0.0 where the reference is"""
    assert got[0].dtype == got[1].dtype == np.int64 and got[2].dtype == np.float64
    assert np.array_equal(got[0], ref[0]), (what, np.argwhere(got[0] != ref[0])[:5])
    assert np.array_equal(got[1], ref[1]), (what, np.argwhere(got[1] != ref[1])[:5])
    bar = (ref[1][..., :1] + 8) * 2.0 ** -52 * ref[2]
    err = np.abs(got[2] - ref[2])
    assert np.all(err <= bar), (what, np.argwhere(~(err <= bar))[:5], err.max())
    assert np.all(got[2][ref[2] == 0] == 0)
