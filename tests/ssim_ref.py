"""The definition of the project's structural similarity (ops.ssim, ops.ssim_loss, csrc/ssim.hip) in direct NumPy, float64
unless a dtype is given, and the case lists the CPU and GPU tests share.

Wang et al. 2004 with a Gaussian window over 'valid' positions: w the separable 11 x 11 Gaussian, sigma = 1.5, each axis
normalised to sum 1.  For fields x, y of H x W and every window position p of the (H - 10) x (W - 10) valid region (the window
covers pixels p .. p + 10 on both axes):
    mu_x = sum w x, mu_y = sum w y, s_x = sum w x^2 - mu_x^2, s_y = sum w y^2 - mu_y^2, s_xy = sum w x y - mu_x mu_y,
    A1 = 2 mu_x mu_y + C1, A2 = 2 s_xy + C2, B1 = mu_x^2 + mu_y^2 + C1, B2 = s_x + s_y + C2,
    C1 = (0.01 L)^2, C2 = (0.03 L)^2, L = data_range (2: fields live in [-1, 1]),
    S(p) = A1 A2 / (B1 B2), cs(p) = A2 / B2; no clamping of the variances.
Per (row, channel): the mean of S and the mean of cs over the valid region.  Row r of x pairs with row r / x_per_y of y.
loss = 1 - the mean over rows and channels of the mean S.  With c = 2 A1 / (B1 B2) = dS/dE[xy], b = -S / B2 = dS/dE[x^2] and
a = 2 mu_y A2 / (B1 B2) - 2 mu_x S / B1 - c mu_y - 2 b mu_x (the total derivative in mu_x),
    d loss / d x(q) = -g / (rows C (H - 10) (W - 10)) ((w * a)(q) + 2 x(q) (w * b)(q) + y(q) (w * c)(q)),
* the FULL correlation of a valid-region map (zero outside) with the symmetric window, H x W."""
import numpy as np

K, SIGMA = 11, 1.5
TILE_W, TILE_H = 32, 16            # the shipped tile of csrc/ssim.hip (SS_TW x SS_TH): window positions forward, pixels backward

# The worst errors of the SAME separable formula in NumPy float32 (textbook E[x^2] - mu^2, no pivot) against float64 over
# CASES, measured by tests/test_ssim_ref_cpu.py::test_fp32_bars_over_the_gpu_case_lists, which also checks these numbers:
FP32_VALUE_ERR = 6.0130e-05        # |mean S - mean S64| and |mean cs - mean cs64|, absolute (a near-flat case)
FP32_GRAD_ERR = 1.7730e-04         # max |grad - grad64| over a field / max |grad64| over that field (a near-flat case)
# The bars of the kernels are 4 x those: a different summation order of the same 11- and 121-term sums.
VALUE_TOL = 4 * FP32_VALUE_ERR     # 4 x 6.0130e-05
GRAD_TOL = 4 * FP32_GRAD_ERR       # 4 x 1.7730e-04


def window(dtype=np.float64):
    k = np.arange(K, dtype=np.float64) - K // 2
    w = np.exp(-k * k / (2.0 * SIGMA * SIGMA))
    return (w / w.sum()).astype(dtype)


def _valid(m, w):
    """(..., H, W) -> (..., H - 10, W - 10): the horizontal 11-tap pass, then the vertical one, in m's dtype"""
    H, W = m.shape[-2:]
    h = np.zeros(m.shape[:-1] + (W - K + 1,), m.dtype)
    for k in range(K):
        h = h + w[k] * m[..., :, k:k + W - K + 1]
    v = np.zeros(m.shape[:-2] + (H - K + 1, W - K + 1), m.dtype)
    for k in range(K):
        v = v + w[k] * h[..., k:k + H - K + 1, :]
    return v


def _full(m, w):
    """(..., Hv, Wv) -> (..., Hv + 10, Wv + 10): the full correlation with the window, the map zero outside"""
    pad = [(0, 0)] * (m.ndim - 2) + [(K - 1, K - 1), (K - 1, K - 1)]
    return _valid(np.pad(m, pad), w)


def _pair(x, y, x_per_y, dtype):
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    assert x.ndim == 4 and y.ndim == 4 and x.shape[0] == y.shape[0] * x_per_y and x.shape[1:] == y.shape[1:], (x.shape, y.shape)
    return x, np.repeat(y, x_per_y, axis=0)


def maps(x, y, x_per_y=1, data_range=2.0, dtype=np.float64):
    """-> dict of (rows, C, H - 10, W - 10) maps in dtype: S, cs and the derivatives a, b, c"""
    x, y = _pair(x, y, x_per_y, dtype)
    w = window(dtype)
    two = dtype(2.0)
    c1, c2 = dtype((0.01 * data_range) ** 2), dtype((0.03 * data_range) ** 2)
    mx, my = _valid(x, w), _valid(y, w)
    vx, vy, cov = _valid(x * x, w) - mx * mx, _valid(y * y, w) - my * my, _valid(x * y, w) - mx * my
    A1, A2, B1, B2 = two * mx * my + c1, two * cov + c2, mx * mx + my * my + c1, vx + vy + c2
    S = A1 * A2 / (B1 * B2)
    c = two * A1 / (B1 * B2)
    b = -S / B2
    a = two * my * A2 / (B1 * B2) - two * mx * S / B1 - c * my - two * b * mx
    return dict(S=S, cs=A2 / B2, a=a, b=b, c=c)


def ssim(x, y, x_per_y=1, data_range=2.0, dtype=np.float64):
    """-> (rows, C, 2) float64: the means of S and cs over the valid region (of maps in dtype, the means in float64)"""
    m = maps(x, y, x_per_y, data_range, dtype)
    return np.stack([m["S"].astype(np.float64).mean((-2, -1)), m["cs"].astype(np.float64).mean((-2, -1))], axis=-1)


def ssim_loss(x, y, data_range=2.0):
    return 1.0 - ssim(x, y, 1, data_range)[..., 0].mean()


def ssim_and_grad(x, y, g=1.0, data_range=2.0, dtype=np.float64):
    """-> (ssim(x, y) (rows, C, 2) float64, the loss float64, d loss / d x (rows, C, H, W) in dtype by the analytic formula of
    the header) from one evaluation of the maps"""
    m = maps(x, y, 1, data_range, dtype)
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    w = window(dtype)
    rows, C, H, W = x.shape
    coef = dtype(-g / (rows * C * (H - K + 1) * (W - K + 1)))
    grad = coef * (_full(m["a"], w) + dtype(2.0) * x * _full(m["b"], w) + y * _full(m["c"], w))
    val = np.stack([m["S"].astype(np.float64).mean((-2, -1)), m["cs"].astype(np.float64).mean((-2, -1))], axis=-1)
    return val, 1.0 - val[..., 0].mean(), grad


def ssim_loss_and_grad(x, y, g=1.0, data_range=2.0, dtype=np.float64):
    """-> (loss float64, d loss / d x (rows, C, H, W) in dtype)"""
    return ssim_and_grad(x, y, g, data_range, dtype)[1:]


def field_grad_error(got, want):
    """the worst, over the (row, channel) fields, of max |got - want| / max |want|"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want).max((-2, -1))
    return float((err / np.abs(want).max((-2, -1))).max())


# ------------------------------------------------------------------------------------------------------------- the cases
KINDS = ("uniform", "smooth_noise", "near_flat", "step")


def make_pair(kind, H, W, rows=3, C=3, seed=0):
    """-> x, y (rows, C, H, W) float32 inside [-1, 1]
    uniform       independent U(-1, 1) noise;
    smooth_noise  a smooth field (low-order sinusoids) as y, x = y + 5 % noise;
    near_flat     y = 0.9 + 1e-3 noise, x = y + 1e-3 noise: E[x^2] - mu^2 cancels in float32;
    step          y a field of -1 with a 10 x 10 block at 0.5 (clipped to the field), x the block moved by (2, 3) + 1 % noise"""
    rs = np.random.RandomState(1000 * seed + 17 * H + W + {"uniform": 0, "smooth_noise": 1, "near_flat": 2, "step": 3}[kind])
    shape = (rows, C, H, W)
    if kind == "uniform":
        x, y = rs.uniform(-1, 1, shape), rs.uniform(-1, 1, shape)
    elif kind == "smooth_noise":
        i, j = np.arange(H)[:, None] / float(H), np.arange(W)[None, :] / float(W)
        ph = rs.uniform(0, 2 * np.pi, (rows, C, 1, 1, 3))
        y = 0.45 * np.sin(2 * np.pi * i + ph[..., 0]) * np.cos(4 * np.pi * j + ph[..., 1]) + 0.35 * np.sin(6 * np.pi * (i + j) + ph[..., 2])
        x = y + 0.05 * rs.standard_normal(shape)
    elif kind == "near_flat":
        y = 0.9 + 1e-3 * rs.standard_normal(shape)
        x = y + 1e-3 * rs.standard_normal(shape)
    elif kind == "step":
        y = np.full(shape, -1.0)
        x = np.full(shape, -1.0)
        y[..., H // 3:H // 3 + 10, W // 3:W // 3 + 10] = 0.5
        x[..., H // 3 + 2:H // 3 + 12, W // 3 + 3:W // 3 + 13] = 0.5
        x = x + 0.01 * np.abs(rs.standard_normal(shape))
    else:
        raise ValueError(kind)
    return np.clip(x, -1, 1).astype(np.float32), np.clip(y, -1, 1).astype(np.float32)


# (H, W) and the edge each exercises
SHAPES = [
    (11, 11),                                  # one window position
    (12, 17),                                  # two rows of seven positions
    (21, 21),                                  # the first size at which a pixel (the centre) lies in all 121 windows
    (11, 64), (64, 11),                        # one row / one column of positions, more than one tile across / down
    (TILE_H + 9, TILE_W + 10),                 # one position short of a full tile down, exactly one tile across
    (TILE_H + 10, TILE_W + 11),                # exactly one tile down, one position into the second tile across
    (TILE_H + 11, TILE_W + 9),                 # one position into the second tile down, one short across
    (2 * TILE_H + 10, 2 * TILE_W + 11),        # two full tiles down, a third tile across holding one column
    (43, 37),                                  # odd sizes, two tiles down
    (64, 64),                                  # the training tests' size
]
LARGE_SHAPES = [
    (321, 321),                                # many tiles, ragged edges on both axes; one row
    (1024, 1024),                              # the upper limit: 32 x 64 tiles; one row, one channel
]
# (kind, H, W, rows, C): what the GPU tests run and the fp32 bars are measured over
CASES = [(kind, H, W, 3, 3) for H, W in SHAPES for kind in KINDS] + \
        [(kind, 321, 321, 1, 3) for kind in ("smooth_noise", "near_flat")] + \
        [("smooth_noise", 1024, 1024, 1, 1)]
