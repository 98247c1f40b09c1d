"""Float64 NumPy statement of the CRPS training loss (ops.crps_loss, acg_crps_fwd / acg_crps_bwd): the reference the kernels,
the op and the paired step are checked against.

For one cell (input n, channel c, pixel p) with members x_1 .. x_M and truth y:
    e1 = (1/M) sum_i |x_i - y|,   e2 = sum_{i<j} |x_i - x_j|,   s = e1 - w e2,
    w  = alpha / (M (M - 1)) + (1 - alpha) / M^2   (M >= 2; 0 for M = 1).
alpha = 1 is the fair CRPS (Ferro 2014), alpha = 0 the ensemble CRPS E1 - E2 / 2 with E2 = (1/M^2) sum_ij |x_i - x_j|, values
between them the almost fair score (Lang et al. 2024).  The loss is the mean of s over N inputs, C channels and H W pixels.
The gradient uses sign(0) = 0:
    d loss / d x_i = g (sign(x_i - y) / M - w sum_{j != i} sign(x_i - x_j)) / (N C H W),
evaluated as g (coef_y sy - coef_pair sp) with the two coefficients 1 / (M N C H W) and w / (N C H W) in double and the
integer sign sums sy, sp: the expression the kernel evaluates, term by term."""
import numpy as np


def weight(M, alpha):
    M = int(M)
    return 0.0 if M == 1 else float(alpha) / (M * (M - 1)) + (1.0 - float(alpha)) / (M * M)


def _cells(x, y, M):
    """x (N M, C, H, W), member m of input n at row n M + m, y (N, C, H, W) -> (N, M, C, H, W), (N, 1, C, H, W) float64"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    N = y.shape[0]
    assert x.shape[0] == N * M and x.shape[1:] == y.shape[1:], (x.shape, y.shape, M)
    return x.reshape((N, M) + y.shape[1:]), y[:, None]


def cell_terms(x, y, M):
    """-> e1, e2 per cell, (N, C, H, W) each"""
    xm, yb = _cells(x, y, M)
    e1 = np.abs(xm - yb).sum(1) / M
    e2 = np.zeros_like(e1)
    for i in range(M):
        for j in range(i + 1, M):
            e2 += np.abs(xm[:, i] - xm[:, j])
    return e1, e2


def sums(x, y, M):
    """what acg_crps_fwd writes: (N, C, 2), the sums over the pixels of e1 and of e2"""
    e1, e2 = cell_terms(x, y, M)
    return np.stack([e1.sum((-2, -1)), e2.sum((-2, -1))], -1)


def score_map(x, y, M, alpha):
    e1, e2 = cell_terms(x, y, M)
    return e1 - weight(M, alpha) * e2


def loss(x, y, M, alpha):
    return float(score_map(x, y, M, alpha).mean())


def parts(x, y, M, alpha):
    """(loss, e1, pair): pair = the mean over cells of the mean |x_i - x_j| over i != j, 0 for M = 1"""
    e1, e2 = cell_terms(x, y, M)
    pair = float((2.0 * e2 / (M * (M - 1))).mean()) if M > 1 else 0.0
    return float((e1 - weight(M, alpha) * e2).mean()), float(e1.mean()), pair


def grad(x, y, M, alpha, g=1.0):
    """d loss / d x, (N M, C, H, W) float64; g the upstream gradient"""
    xm, yb = _cells(x, y, M)
    cells = int(np.prod(yb.shape))
    coef_y, coef_pair = 1.0 / (M * cells), weight(M, alpha) / cells
    sy = np.sign(xm - yb)
    sp = np.zeros_like(xm)
    for i in range(M):
        for j in range(M):
            if j != i:
                sp[:, i] += np.sign(xm[:, i] - xm[:, j])
    d = float(g) * (coef_y * sy - coef_pair * sp)
    return d.reshape(np.asarray(x).shape)
