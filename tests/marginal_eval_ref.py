"""The definition of the marginal evaluator (acg_marginal_scores, ops.sorted_scores, ops.marginal_scores, --metric marginal)
in float64 NumPy, and the cases its tests use.

For a field x of P pixels with sorted values s_x (after + 0.0: a -0.0 sorts and leaves as +0.0) and its paired truth y:
  w1    = mean_k |s_x[k] - s_y[k]|, w2sq = mean_k (s_x[k] - s_y[k])^2, differences and sums in float64: for samples of equal
          size the 1-Wasserstein and the squared 2-Wasserstein distance of the two empirical distributions;
  q(level): pos = level (P - 1), lo = floor(pos), hi = min(lo + 1, P - 1), s[lo] + (pos - lo) (s[hi] - s[lo]) in float64,
          rounded once to float32: numpy.quantile(..., method="linear");
  below(edge) = #{p : x[p] < edge}: numpy.searchsorted(s_x, edge, side="left"); P - below = #{p : x[p] >= edge}."""
import numpy as np

from marginal_ref import FIELD_KINDS, make_fields  # noqa: F401  (the tests take their fields from there)

MAX_LEVELS, MAX_EDGES = 16, 256
# 16 levels: both ends (the clamp hi = P - 1 at level 1), 1/3 (no exact position in any P > 1), the evaluator's defaults
LEVELS16 = (0.0, 1.0, 1.0 / 3.0, 0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99, 0.999, 0.9999, 2.0 / 3.0, 1e-7)
LEVELS1 = (1.0 / 3.0,)
# (H, W) of the CPU checks of the definition
CPU_SHAPES = ((1, 1), (1, 2), (11, 13), (64, 64), (91, 91), (129, 127))


def sorted_values(x):
    """x (..., P) -> the same dtype, every field ascending, -0.0 as +0.0"""
    return np.sort(x + x.dtype.type(0.0), axis=-1)


def wasserstein(sx, sy, x_per_y=1):
    """sx (rows, C, P), sy (rows / x_per_y, C, P), both sorted -> (rows, C, 2) float64: w1, w2sq"""
    d = sx.astype(np.float64) - np.repeat(sy.astype(np.float64), x_per_y, axis=0)
    return np.stack([np.abs(d).mean(-1), (d * d).mean(-1)], axis=-1)


def quantiles(sx, levels):
    """sx (rows, C, P) sorted -> (rows, C, L) float32"""
    P = sx.shape[-1]
    s = sx.astype(np.float64)
    out = np.empty(sx.shape[:-1] + (len(levels),), dtype=np.float32)
    for i, level in enumerate(levels):
        pos = np.float64(level) * np.float64(P - 1)
        lo = int(np.floor(pos))
        hi = min(lo + 1, P - 1)
        frac = pos - np.float64(lo)
        out[..., i] = (s[..., lo] + frac * (s[..., hi] - s[..., lo])).astype(np.float32)
    return out


def below(sx, edges):
    """sx (rows, C, P) sorted, edges (C, E) float32 -> (rows, C, E) int32"""
    rows, C, _ = sx.shape
    out = np.empty((rows, C, edges.shape[1]), dtype=np.int32)
    for r in range(rows):
        for c in range(C):
            out[r, c] = np.searchsorted(sx[r, c], edges[c], side="left")
    return out


def scores(x, y, levels, edges, x_per_y=1):
    """x (rows, C, H, W), y (rows / x_per_y, C, H, W) or None, float32 -> dict(w, q, below) as ops.marginal_scores gives them"""
    sx = sorted_values(x.reshape(x.shape[0], x.shape[1], -1))
    res = {}
    if y is not None:
        res["w"] = wasserstein(sx, sorted_values(y.reshape(y.shape[0], y.shape[1], -1)), x_per_y)
    if len(levels):
        res["q"] = quantiles(sx, levels)
    if edges is not None and edges.shape[1]:
        res["below"] = below(sx, edges)
    return res


def make_edges(sx, E, seed=0):
    """(C, E) float32 edges for sorted fields sx (rows, C, P), in no order: exact data values, one below the minimum and one
    above the maximum, -inf and +inf, both zeros (-0.0 against fields that hold zeros), repeats, the rest uniform in the range"""
    rows, C, P = sx.shape
    rs = np.random.RandomState(seed + 31 * E + P)
    lo, hi = np.float32(sx.min()), np.float32(sx.max())
    e = rs.uniform(min(lo, -1.0), max(hi, 1.0), (C, E)).astype(np.float32)
    if E == 1:
        e[:, 0] = sx[0, :, P // 2]                                 # an exact data value
        return e
    special = [np.float32(-np.inf), np.float32(np.inf), np.float32(-0.0), np.float32(0.0), np.nextafter(lo, np.float32(-np.inf)),
               np.nextafter(hi, np.float32(np.inf)), lo, hi]
    for c in range(C):
        vals = special + [sx[rs.randint(rows), c, rs.randint(P)] for _ in range(24)]
        vals = vals + vals[:8]                                     # repeats
        at = rs.permutation(E)[:len(vals)]
        e[c, at] = np.asarray(vals[:len(at)], dtype=np.float32)
    return e


def ulp_distance(a, b):
    """float32 arrays (finite, after + 0.0) -> the distance of every pair in units in the last place, int64"""
    def key(v):
        i = np.ascontiguousarray(v + np.float32(0.0), dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


# The C-ABI cases: (P, rows, C, x_per_y or 0 for no truth, L, E).  P: one wave and its edges (63, 64, 65), a group of four and
# its remainders (1, 2, 143), one trip of the 1024 threads and more (4096, 8192), just above the sort's one-launch size (8281 =
# 91 x 91), 16383 = 129 x 127, and 103041 = 321 x 321 once.  rows C in {1, 21}, x_per_y in {1, 3} and no truth, L in {0, 1, 16},
# E in {0, 1, 256}; every value of each appears with small and large fields.
ABI_CASES = (
    (1, 1, 1, 1, 16, 256), (1, 7, 3, 0, 1, 1), (2, 1, 1, 1, 16, 0), (2, 21, 1, 3, 0, 256),
    (63, 1, 1, 1, 1, 256), (63, 7, 3, 0, 16, 1), (64, 7, 3, 1, 16, 256), (64, 1, 1, 0, 0, 1),
    (65, 21, 1, 3, 16, 1), (65, 1, 1, 1, 0, 0), (143, 3, 7, 3, 16, 256), (143, 1, 1, 0, 16, 0),
    (4096, 7, 3, 1, 16, 256), (4096, 1, 1, 1, 0, 0), (8192, 1, 1, 1, 1, 1), (8192, 7, 3, 0, 16, 256),
    (8281, 21, 1, 3, 16, 256), (8281, 1, 1, 1, 16, 1), (16383, 7, 3, 1, 1, 256), (16383, 1, 1, 0, 16, 256),
    (103041, 1, 1, 1, 16, 256),
)
# the kinds a case draws its fields from (x, then y), in turn
ABI_KINDS = (("uniform", "tanh_normal"), ("masked", "uniform"), ("signed_zeros", "masked"), ("constant", "ascending"),
             ("descending", "tanh_normal"), ("tanh_normal", "tanh_normal"), ("ascending", "signed_zeros"))


def abi_case_fields(i):
    """case i of ABI_CASES -> (sx (rows, C, P), sy (rows / x_per_y, C, P) or None) float32, sorted on the host"""
    P, rows, C, per, L, E = ABI_CASES[i]
    kx, ky = ABI_KINDS[i % len(ABI_KINDS)]
    sx = sorted_values(make_fields(kx, 1, P, rows, C, seed=10 + i).reshape(rows, C, P))
    sy = None
    if per:
        sy = sorted_values(make_fields(ky, 1, P, rows // per, C, seed=50 + i).reshape(rows // per, C, P))
    return sx, sy
