"""The definition of the marginal loss (ops.field_sort, ops.marginal_loss) in float64 NumPy, and the fields its tests use.

Order inside one field of P = H W pixels: pixel p = h W + w comes before pixel q iff x[p] < x[q] as floats, or x[p] == x[q]
and p < q (-0.0 and +0.0 tie): numpy.argsort(kind="stable") of the field after + 0.0.
  s[r, c, k]     the k-th smallest value of field (r, c)
  rank[r, c, p]  the position of pixel p in that order
  Q_x[c, k] = mean_r s_x[r, c, k] (and Q_y), d = Q_x - Q_y, loss = mean_{c, k} d^2,
  d loss / d x[r, c, p] = 2 d[c, rank_x[r, c, p]] / (C P Rx)."""
import numpy as np

FIELD_KINDS = ("uniform", "tanh_normal", "masked", "constant", "signed_zeros", "descending", "ascending")


def make_fields(kind, H, W, rows=3, C=3, seed=0):
    """(rows, C, H, W) float32 fields in [-1, 1]"""
    rs = np.random.RandomState(seed + 7919 * FIELD_KINDS.index(kind))
    shape, P = (rows, C, H, W), H * W
    if kind == "uniform":
        x = rs.uniform(-1, 1, shape)
    elif kind == "tanh_normal":                                    # saturates: exact +-1 ties
        x = np.tanh(rs.standard_normal(shape).astype(np.float32) * np.float32(4))
    elif kind == "masked":                                         # 40 % of the pixels exactly equal (a zero-filled NaN mask)
        x = rs.uniform(-1, 1, shape)
        x[rs.uniform(size=shape) < 0.4] = 0.0
    elif kind == "constant":
        x = np.full(shape, 0.25)
    elif kind == "signed_zeros":
        x = np.where(rs.uniform(size=shape) < 0.5, -0.0, 0.0)
        x = np.where(rs.uniform(size=shape) < 0.2, rs.uniform(-1, 1, shape), x)
    elif kind in ("descending", "ascending"):
        ramp = np.linspace(-1, 1, P) if P > 1 else np.zeros(1)
        if kind == "descending":
            ramp = ramp[::-1]
        x = np.broadcast_to(ramp.reshape(H, W), shape) * (1 + np.arange(rows * C).reshape(rows, C, 1, 1)) / (rows * C)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32)


def sort_fields(x):
    """x (rows, C, H, W) -> (sorted (rows, C, P) in the dtype of x, rank (rows, C, P) int32).  A -0.0 leaves as +0.0."""
    rows, C, H, W = x.shape
    f = x.reshape(rows, C, H * W) + x.dtype.type(0.0)
    order = np.argsort(f, axis=-1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(H * W), order.shape), axis=-1)
    return np.take_along_axis(f, order, axis=-1), rank.astype(np.int32)


def quantile_difference(x, y):
    """d (C, P) float64 = Q_x - Q_y"""
    sx, _ = sort_fields(x.astype(np.float64))
    sy, _ = sort_fields(y.astype(np.float64))
    return sx.mean(0) - sy.mean(0)


def marginal_loss(x, y):
    d = quantile_difference(x, y)
    return float(np.mean(d * d))


def marginal_loss_and_grad(x, y):
    """-> (loss, d loss / d x (rows, C, H, W), d (C, P)), all float64"""
    rows, C, H, W = x.shape
    _, rank = sort_fields(x.astype(np.float64))
    d = quantile_difference(x, y)
    g = 2.0 * np.take_along_axis(np.broadcast_to(d, rank.shape), rank.astype(np.int64), axis=-1) / (C * H * W * rows)
    return float(np.mean(d * d)), g.reshape(x.shape), d


# (H, W, rows of x, rows of y) of the loss tests: padded and unpadded fields on the single-launch path and on the launch chain,
# unequal row counts once, and the field size and batch of the training-step tests
LOSS_CASES = ((16, 16, 3, 3), (17, 13, 3, 3), (90, 90, 3, 3), (96, 96, 3, 2), (160, 200, 3, 3), (64, 64, 4, 4))


def loss_batches(H, W, rows_x=3, rows_y=3, C=3):
    """a uniform batch against a saturating one: a loss of order 1e-2, not a difference of near-equal numbers"""
    return make_fields("uniform", H, W, rows_x, C, seed=1), make_fields("tanh_normal", H, W, rows_y, C, seed=2)
