"""The definition of the per-cell statistics of acg_cell_stats (include/acgan_cell.h) in NumPy: a loop over the truth rows n and
the members m, vectorised over the cells, one NumPy operation per line of the definition, so that every double is rounded
where the kernel rounds it and the result can be compared for equality.  Also the inputs the tests share."""
import numpy as np

MOMENTS = ("Sx", "Sxx", "Sy", "Syy", "Sxy", "Sad", "SS", "SSy", "Sw")


def new_state(C, H, W, T, E):
    return dict(mom=np.zeros((9, C, H, W), np.float64), evt=np.zeros((C, T, 4, H, W), np.int64) if T else None,
                hist_x=np.zeros((C, E + 1, H, W), np.int32) if E else None, hist_y=np.zeros((C, E + 1, H, W), np.int32) if E else None,
                n=0, M=0)


def copy_state(s):
    return {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in s.items()}


def bins(v, edges):
    """v (C, H, W) float32, edges (C, E) float32 -> #{e : edges[c][e] <= v}; a NaN compares false: bin 0"""
    return (edges[:, :, None, None] <= v[:, None]).sum(1)


def accumulate(state, x, y, M, thr=None, edges=None):
    """adds x (Ny M, C, H, W) float32 against y (Ny, C, H, W) float32 to the state, in place -> the state"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    Ny = y.shape[0]
    assert x.shape[0] == Ny * M and x.shape[1:] == y.shape[1:] and state["M"] in (0, M)
    Sx, Sxx, Sy, Syy, Sxy, Sad, SS, SSy, Sw = state["mom"]          # views: updated in place
    Md = np.float64(M)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(Ny):
            yv = y[n].astype(np.float64)
            Sy += yv
            Syy += yv * yv
            S = np.zeros_like(yv)
            Q = np.zeros_like(yv)
            for m in range(M):
                xv = x[n * M + m].astype(np.float64)
                Sx += xv
                Sxx += xv * xv
                Sxy += xv * yv
                Sad += np.abs(xv - yv)
                S += xv
                Q += xv * xv
            u = S * S
            SS += u
            SSy += S * yv
            t = Md * Q
            v = t - u
            Sw += v
            if thr is not None:
                k = (x[n * M:(n + 1) * M][:, :, None] >= thr[None, :, :, None, None]).sum(0).astype(np.int64)   # (C, T, H, W), float32
                o = (y[n][:, None] >= thr[:, :, None, None]).astype(np.int64)
                state["evt"] += np.stack([k, o, k * o, k * k], 2)
            if edges is not None:
                E = edges.shape[1]
                by = bins(y[n], edges)
                for b in range(E + 1):
                    state["hist_y"][:, b] += (by == b)
                for m in range(M):
                    bx = bins(x[n * M + m], edges)
                    for b in range(E + 1):
                        state["hist_x"][:, b] += (bx == b)
    state["n"] += Ny
    state["M"] = M
    return state


def brute_cell(x, y, M, c, i, j, thr=None, edges=None):
    """one cell by Python scalars (float is an IEEE double) -> (the nine sums, evt (T, 4), hist_x, hist_y)"""
    a = [0.0] * 9
    T, E = (0 if thr is None else thr.shape[1]), (0 if edges is None else edges.shape[1])
    evt = np.zeros((T, 4), np.int64)
    hx, hy = np.zeros(E + 1, np.int64), np.zeros(E + 1, np.int64)
    for n in range(y.shape[0]):
        yf = y[n, c, i, j]
        yv = float(yf)
        a[2] += yv
        a[3] += yv * yv
        S = Q = 0.0
        k = np.zeros(T, np.int64)
        for m in range(M):
            xf = x[n * M + m, c, i, j]
            xv = float(xf)
            a[0] += xv
            a[1] += xv * xv
            a[4] += xv * yv
            a[5] += abs(xv - yv)
            S += xv
            Q += xv * xv
            for t in range(T):
                k[t] += bool(xf >= thr[c, t])
            if E:
                hx[sum(bool(e <= xf) for e in edges[c])] += 1
        a[6] += S * S
        a[7] += S * yv
        a[8] += M * Q - S * S
        for t in range(T):
            o = int(yf >= thr[c, t])
            evt[t] += (k[t], o, k[t] * o, k[t] * k[t])
        if E:
            hy[sum(bool(e <= yf) for e in edges[c])] += 1
    return np.array(a), evt, hx, hy


def same(a, b):
    """equality of two arrays with NaNs in the same places (the sign and payload of a NaN are not part of the definition:
    inf - inf is -NaN on one machine and +NaN on another); everything else bit for bit, -0.0 apart from 0.0"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    bits = a.view(np.int64 if a.dtype == np.float64 else np.int32) == b.view(np.int64 if b.dtype == np.float64 else np.int32)
    return bool(np.array_equal(na, nb) and np.all(bits | na))


def same_state(a, b):
    return all((a[k] is None and b[k] is None) or same(a[k], b[k]) for k in ("mom", "evt", "hist_x", "hist_y")) \
        and a["n"] == b["n"] and a["M"] == b["M"]


def tables(C, T, E, seed=0):
    """thresholds (C, T) and ascending edges (C, E) float32 (None for 0); edges repeat a value where E >= 4"""
    rs = np.random.RandomState(1000 + seed)
    thr = np.sort(rs.uniform(-1.0, 1.5, (C, T)).astype(np.float32), 1) if T else None
    edges = np.sort(rs.uniform(-2.0, 2.0, (C, E)).astype(np.float32), 1) if E else None
    if E >= 4:
        edges[:, 2] = edges[:, 1]
    return thr, edges


def fields(Ny, M, C, H, W, seed=0, thr=None, edges=None, special=True):
    """members (Ny M, C, H, W) and truths (Ny, C, H, W) float32: correlated noise (no subnormals); with `special`, cells that
    hold values on a threshold and on an edge, +-0, and (for H W >= 8) one NaN, one +inf and one -inf cell in x and in y"""
    rs = np.random.RandomState(seed)
    y = rs.normal(0.0, 1.0, (Ny, C, H, W)).astype(np.float32)
    x = (np.repeat(y, M, 0) * np.float32(0.6) + rs.normal(0.2, 0.8, (Ny * M, C, H, W))).astype(np.float32)
    if special:
        fx, fy = x.reshape(Ny * M, C, H * W), y.reshape(Ny, C, H * W)
        pick = lambda: rs.randint(H * W)
        for c in range(C):
            if thr is not None:
                fx[rs.randint(Ny * M), c, pick()] = thr[c, -1]
                fy[rs.randint(Ny), c, pick()] = thr[c, 0]
            if edges is not None:
                fx[rs.randint(Ny * M), c, pick()] = edges[c, 0]
                fx[rs.randint(Ny * M), c, pick()] = edges[c, -1]
                fy[rs.randint(Ny), c, pick()] = edges[c, edges.shape[1] // 2]
            fx[0, c, pick()] = -0.0
            fy[0, c, pick()] = 0.0
        if H * W >= 8:
            cells = rs.permutation(H * W)[:6]
            fx[rs.randint(Ny * M), 0, cells[0]] = np.nan
            fx[rs.randint(Ny * M), 0, cells[1]] = np.inf
            fx[rs.randint(Ny * M), C - 1, cells[2]] = -np.inf
            fy[rs.randint(Ny), 0, cells[3]] = np.nan
            fy[rs.randint(Ny), C - 1, cells[4]] = np.inf
            fy[rs.randint(Ny), 0, cells[5]] = -np.inf
    assert not np.any((np.abs(x) < np.finfo(np.float32).tiny) & (x != 0)) and not np.any((np.abs(y) < np.finfo(np.float32).tiny) & (y != 0))
    return x, y
