"""Float64 NumPy restatement of the paired cross-spectra (acg_cross_spectrum, model.translate_coherence) and of the quantities
the evaluator derives from them: the reference the kernel and `--metric coherence` are tested against.

For paired real fields x, y, S x S: X = fft2(x), Y = fft2(y) (unnormalised, no taper, no mean removal); per cell
Pxx = |X|^2 / S^2, Pyy = |Y|^2 / S^2, Cxy = Re(X conj Y) / S^2.  The rings are spectrum_ref.bin_index's (bins 0 .. S/2, corners
dropped); pxx[b], pyy[b], cxy[b] are the means over the ring's cells.  The quadrature part Im(X conj Y) sums to 0 over every
ring (the ring is closed under k -> -k and the twin cell holds the conjugate product), so it is no output.

From triples summed over a set of pairs: coherence coh[b] = (sum cxy)^2 / (sum pxx sum pyy) (0 where the denominator is 0),
signed correlation r[b] = sum cxy / sqrt(sum pxx sum pyy), error spectrum perr = pxx + pyy - 2 cxy (the radial spectrum of
x - y), effective resolution k_eff: the smallest b >= 1 with coh[b] < 0.5, S/2 + 1 if there is none."""
import numpy as np

import spectrum_ref as R

PAIR_KINDS = ("same", "neg", "indep", "shift", "lowpass_noise", "nyquist", "dc", "scaled")
# (S, rows, C) of the accuracy test and of the tolerance measurement behind it: one workgroup per pair up to 64, the first
# two-pass size 128, every size above it; the large ones once
PAIR_CASES = ((16, 3, 3), (32, 3, 3), (64, 3, 3), (128, 3, 3), (256, 3, 3), (512, 1, 1), (1024, 1, 1))


def planes(x, y):
    """(..., S, S) fields -> the float64 planes (Pxx, Pyy, Cxy, Qxy), Qxy = Im(X conj Y) / S^2"""
    x, y = np.asarray(x), np.asarray(y)
    S = x.shape[-1]
    X = np.fft.fft2(x.astype(np.float64), axes=(-2, -1))
    Y = np.fft.fft2(y.astype(np.float64), axes=(-2, -1))
    XY = X * np.conj(Y)
    n = float(S * S)
    return (X.real ** 2 + X.imag ** 2) / n, (Y.real ** 2 + Y.imag ** 2) / n, XY.real / n, XY.imag / n


def cross_spectrum(x, y):
    """(..., S, S) paired fields -> (..., 3, S/2 + 1) float64: the ring means pxx, pyy, cxy"""
    pxx, pyy, cxy, _ = planes(x, y)
    return np.stack([R.bin_power(pxx), R.bin_power(pyy), R.bin_power(cxy)], axis=-2)


def quadrature(x, y):
    """(..., S/2 + 1) float64: the ring means of Im(X conj Y) / S^2 (identically 0 for real fields)"""
    return R.bin_power(planes(x, y)[3])


def summary(sums):
    """(..., 3, nb) summed triples -> dict(coh, r, perr (..., nb), k_eff (...) int64)"""
    t = np.asarray(sums, dtype=np.float64)
    pxx, pyy, cxy = t[..., 0, :], t[..., 1, :], t[..., 2, :]
    den = pxx * pyy
    coh, r = np.zeros_like(den), np.zeros_like(den)
    ok = den > 0
    coh[ok] = cxy[ok] ** 2 / den[ok]
    r[ok] = cxy[ok] / np.sqrt(den[ok])
    nb = t.shape[-1]
    k_eff = np.full(t.shape[:-2], nb, dtype=np.int64)
    for i in np.ndindex(*t.shape[:-2]):
        low = np.nonzero(coh[i][1:] < 0.5)[0]
        if low.size:
            k_eff[i] = low[0] + 1
    return dict(coh=coh, r=r, perr=pxx + pyy - 2.0 * cxy, k_eff=k_eff)


def make_pairs(kind, S, rows=3, C=3, seed=0):
    """(x, y), each (rows, C, S, S) float32, seeded by (kind, S, seed) through spectrum_ref.make_fields:
      same           x = tanh_red, y = x
      neg            y = -x
      indep          y = a red field of another seed
      shift          y = x rolled by (3, 5)
      lowpass_noise  y = x filtered by exp(-(k / (S/8))^2) + 0.05 white
      nyquist        x = (-1)^w + 0.25 cos(2 pi 3 h / S), y = 0.5 (-1)^w + (-1)^h + 0.5 cos(2 pi 3 h / S + 1): energy on the
                     self-twin cells and on the packed columns kx = 0 and kx = S/2
      dc             x = dc_noise, y = -0.4 + 0.5 (x - 0.7): bin 0 with opposite signs
      scaled         y = 1e-3 red"""
    if kind == "nyquist":
        h, w = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
        sw, sh = 1.0 - 2.0 * (w % 2), 1.0 - 2.0 * (h % 2)
        x = sw + 0.25 * np.cos(2 * np.pi * 3 * h / S)
        y = 0.5 * sw + sh + 0.5 * np.cos(2 * np.pi * 3 * h / S + 1.0)
        x, y = np.broadcast_to(x, (rows, C, S, S)), np.broadcast_to(y, (rows, C, S, S))
    elif kind == "dc":
        x = R.make_fields("dc_noise", S, rows, C, seed).astype(np.float64)
        y = -0.4 + 0.5 * (x - 0.7)
    else:
        x = R.make_fields("tanh_red", S, rows, C, seed).astype(np.float64)
        if kind == "same":
            y = x
        elif kind == "neg":
            y = -x
        elif kind == "indep":
            y = R.make_fields("red", S, rows, C, seed + 1)
        elif kind == "shift":
            y = np.roll(x, (3, 5), axis=(-2, -1))
        elif kind == "lowpass_noise":
            f = R.wavenumbers(S).astype(np.float64)
            k = np.sqrt(f[:, None] ** 2 + f[None, :] ** 2)
            rs = np.random.RandomState(31 * S + seed + 5)
            y = np.fft.ifft2(np.fft.fft2(x) * np.exp(-(k / (S / 8.0)) ** 2)).real + 0.05 * rs.uniform(-1, 1, x.shape)
        elif kind == "scaled":
            y = 1e-3 * R.make_fields("red", S, rows, C, seed + 1).astype(np.float64)
        else:
            raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)


def cross_tolerance_needed(cxy, ref, Ex, Ey):
    """the smallest tau with |cxy - ref_cxy| <= tau (sqrt(pxx_ref Ey) + sqrt(pyy_ref Ex)) + tau^2 sqrt(Ex Ey) in every bin;
    ref (..., 3, nb) the reference triples, Ex, Ey (...) the fields' mean squares.  The bound follows from a per-cell transform
    error of tau sqrt(E) S in each field and Cauchy-Schwarz over a ring."""
    d = np.abs(np.asarray(cxy, dtype=np.float64) - ref[..., 2, :])
    Ex = np.broadcast_to(np.asarray(Ex, dtype=np.float64)[..., None], d.shape)
    Ey = np.broadcast_to(np.asarray(Ey, dtype=np.float64)[..., None], d.shape)
    a, b = np.sqrt(Ex * Ey), np.sqrt(ref[..., 0, :] * Ey) + np.sqrt(ref[..., 1, :] * Ex)
    root = b + np.sqrt(b * b + 4.0 * a * d)
    tau = 2.0 * d / np.where(root > 0, root, 1.0)                  # the stable root of a tau^2 + b tau - d = 0
    return float(np.max(np.where(d > 0, tau, 0.0)))


def cross_bound(ref, Ex, Ey, tau):
    """the allowed |cxy - ref_cxy| per bin, (..., nb)"""
    Ex, Ey = np.asarray(Ex, dtype=np.float64)[..., None], np.asarray(Ey, dtype=np.float64)[..., None]
    return tau * (np.sqrt(ref[..., 0, :] * Ey) + np.sqrt(ref[..., 1, :] * Ex)) + tau ** 2 * np.sqrt(Ex * Ey)
