"""fp64 NumPy statement of the window plan, the window cut and the seam blend (ops.window_plan, acg_window_gather,
acg_window_blend), written from their specification, loops and all — not from the kernels.

plan     per axis one window if the extent equals S, else n = ceil((extent - overlap) / (S - overlap)) windows with origins
         round(k (extent - S) / (n - 1)), k = 0 .. n-1; R = max(overlap, 1)
gather   window t of table row (src, oy, ox, flip): out[t, i, j, c] = fields[src, c, oy + i', ox + j'], i' = S-1-i if
         flip & 2 else i, j' = S-1-j if flip & 1 else j; channels C .. Cp-1 zero
blend    tile (ky, kx) of canvas r sits at row (r ny + ky) nx + kx with its origin at (oy[ky], ox[kx]); tile pixel (i, j)
         weighs w(i) w(j), w(i) = min(i + 1, S - i, R) / R; a canvas pixel is sum(w v) / sum(w) over the covering tiles
"""
import math

import numpy as np


def plan_axis(extent, S, overlap):
    if extent < S:
        raise ValueError("extent %d below the window %d" % (extent, S))
    if not 0 <= overlap <= S // 2:
        raise ValueError("overlap %d outside 0..%d" % (overlap, S // 2))
    if extent == S:
        return [0]
    n = int(math.ceil((extent - overlap) / float(S - overlap)))
    return [int(round(k * (extent - S) / float(n - 1))) for k in range(n)]


def plan(H, W, S, overlap):
    return dict(H=H, W=W, S=S, R=max(overlap, 1), oy=plan_axis(H, S, overlap), ox=plan_axis(W, S, overlap))


def cimg(C):
    return 4 if C <= 4 else (C + 15) // 16 * 16


def gather(fields, table, S, Cp=None):
    """fields (N, C, H, W), table rows (src, oy, ox, flip) -> (T, S, S, Cp), the dtype of fields (a copy, bit for bit)"""
    fields = np.asarray(fields)
    N, C, H, W = fields.shape
    Cp = cimg(C) if Cp is None else Cp
    out = np.zeros((len(table), S, S, Cp), fields.dtype)
    for t, (src, oy, ox, flip) in enumerate(table):
        assert 0 <= src < N and 0 <= oy <= H - S and 0 <= ox <= W - S and 0 <= flip <= 3, (src, oy, ox, flip)
        for i in range(S):
            y = oy + (S - 1 - i if flip & 2 else i)
            for j in range(S):
                x = ox + (S - 1 - j if flip & 1 else j)
                out[t, i, j, :C] = fields[src, :, y, x]
    return out


def weight(S, R):
    return np.array([min(i + 1, S - i, R) / float(R) for i in range(S)], dtype=np.float64)


def plan_table(p, rows):
    """the table that cuts every window of plan p out of `rows` fields, in the order the blend takes the tiles back"""
    return [(r, oy, ox, 0) for r in range(rows) for oy in p["oy"] for ox in p["ox"]]


def blend(tiles, p, rows, C):
    """tiles (rows ny nx, S, S, Cp) -> (canvas (rows, C, H, W) float64, cover (H, W) int: the tiles over every pixel)"""
    H, W, S, R, oy, ox = p["H"], p["W"], p["S"], p["R"], p["oy"], p["ox"]
    ny, nx = len(oy), len(ox)
    tiles = np.asarray(tiles, dtype=np.float64)
    assert tiles.shape[:3] == (rows * ny * nx, S, S)
    w = weight(S, R)
    w2 = w[:, None] * w[None, :]
    num = np.zeros((rows, C, H, W))
    den = np.zeros((H, W))
    cover = np.zeros((H, W), dtype=np.int64)
    for ky in range(ny):
        for kx in range(nx):
            ys, xs = slice(oy[ky], oy[ky] + S), slice(ox[kx], ox[kx] + S)
            den[ys, xs] += w2
            cover[ys, xs] += 1
            for r in range(rows):
                v = tiles[(r * ny + ky) * nx + kx, :, :, :C].transpose(2, 0, 1)
                num[r, :, ys, xs] += w2[None] * v
    assert cover.min() >= 1 and den.min() > 0
    return num / den[None, None], cover


def single_source(p):
    """per canvas pixel covered by exactly one tile: (ky, kx) of that tile, -1 elsewhere -> two (H, W) int arrays"""
    H, W, S, oy, ox = p["H"], p["W"], p["S"], p["oy"], p["ox"]
    cy = [[k for k, o in enumerate(oy) if o <= y < o + S] for y in range(H)]
    cx = [[k for k, o in enumerate(ox) if o <= x < o + S] for x in range(W)]
    ky = np.full((H, W), -1)
    kx = np.full((H, W), -1)
    for y in range(H):
        for x in range(W):
            if len(cy[y]) == 1 and len(cx[x]) == 1:
                ky[y, x], kx[y, x] = cy[y][0], cx[x][0]
    return ky, kx
