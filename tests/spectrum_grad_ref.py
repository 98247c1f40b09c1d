"""Float64 NumPy restatement of the data gradient of the radially averaged power spectrum (acg_radial_spectrum_bwd,
ops.RadialSpectrum) and of ops.spectral_loss with its input gradient; the spectrum itself is tests/spectrum_ref.py's.

For a cotangent g[b] of psd[b], b = 0 .. S/2:  d sum_b g[b] psd[b] / dx = 2 Re ifft2(w fft2(x)), w[ky, kx] = g[bin] / count[bin]
for bin <= S/2, else 0 (psd[b] = sum over the ring of F conj(F) / (S^2 count[b]); d/dx of F conj(F) is 2 Re(conj(F) dF/dx), and
sum_k w_k conj(F_k) exp(-i k x) is real for a radial w: S^2 ifft2(w F))."""
import numpy as np

import spectrum_ref as R

COTANGENT_KINDS = ("normal", "count_uniform", "bin_0", "bin_1", "bin_last")


def cell_weights(S, g):
    """(..., S/2 + 1) cotangents -> (..., S, S) float64: g[bin] / count[bin] per cell, 0 in the dropped corners"""
    g = np.asarray(g, dtype=np.float64)
    b = R.bin_index(S)
    per_bin = g / R.bin_counts(S)
    return np.where(b <= S // 2, per_bin[..., np.minimum(b, S // 2)], 0.0)


def rapsd_vjp(x, g):
    """(..., S, S) fields, (..., S/2 + 1) cotangents -> (..., S, S) float64: the gradient of sum(g * rapsd(x)) in x"""
    x = np.asarray(x, dtype=np.float64)
    F = np.fft.fft2(x, axes=(-2, -1))
    return 2.0 * np.fft.ifft2(cell_weights(x.shape[-1], g) * F, axes=(-2, -1)).real


def cotangents(kind, S, shape, seed=0):
    """shape + (S/2 + 1,) float32 cotangents, seeded by (kind, S, seed): N(0, 1) per bin; count[b] U(-1, 1) (every cell weight
    O(1)); a single bin (0, 1 or S/2) set to 1.5"""
    nb = S // 2 + 1
    rs = np.random.RandomState(5000 + 100 * COTANGENT_KINDS.index(kind) + 13 * S + seed)
    if kind == "normal":
        g = rs.standard_normal(shape + (nb,))
    elif kind == "count_uniform":
        g = R.bin_counts(S) * rs.uniform(-1, 1, shape + (nb,))
    else:
        g = np.zeros(shape + (nb,))
        g[..., {"bin_0": 0, "bin_1": 1, "bin_last": nb - 1}[kind]] = 1.5
    return np.ascontiguousarray(g, dtype=np.float32)


def vjp_error(gx, ref, g, x):
    """max |gx - ref| / (2 max_b |g[b] / count[b]| rms(x)) per field -> (...,): the denominator bounds rms(ref) (Parseval:
    |w F| <= max|w| |F| cell by cell), so the measure keeps its meaning where ref is tiny or concentrated"""
    S = x.shape[-1]
    wmax = np.abs(np.asarray(g, dtype=np.float64) / R.bin_counts(S)).max(axis=-1)
    rms = np.sqrt(np.mean(np.asarray(x, dtype=np.float64) ** 2, axis=(-2, -1)))
    return np.abs(np.asarray(gx, dtype=np.float64) - ref).max(axis=(-2, -1)) / (2.0 * wmax * rms)


def spectral_loss(x, y, eps=1e-6):
    """x (rows, C, S, S), y (rows', C, S, S) -> float64: the mean over channels and bins 1 .. S/2 of
    (ln(p + eps) - ln(q + eps))^2, p / q the means over the rows of the spectra of x / y"""
    return spectral_loss_and_grad(x, y, eps)[0]


def spectral_loss_and_grad(x, y, eps=1e-6):
    """-> (loss, d loss / d x (rows, C, S, S), the cotangent every row's spectrum receives (C, S/2 + 1)), all float64"""
    p, q = R.rapsd(x).mean(axis=0), R.rapsd(y).mean(axis=0)
    d = np.log(p[:, 1:] + eps) - np.log(q[:, 1:] + eps)
    loss = float(np.mean(d * d))
    g = np.zeros_like(p)
    g[:, 1:] = 2.0 * d / (p[:, 1:] + eps) / d.size / x.shape[0]
    return loss, rapsd_vjp(x, np.broadcast_to(g, (x.shape[0],) + g.shape)), g


LOSS_KINDS = ("white", "red", "tanh_red")
LOSS_SIZES = (64, 256)


def loss_batches(kind, S, rows=4, C=3):
    """the batches ops.spectral_loss is tested on: x of the kind, y a red field of another seed (unpaired, one row more)"""
    return R.make_fields(kind, S, rows=rows, C=C, seed=2), R.make_fields("red", S, rows=rows + 1, C=C, seed=3)
