"""Float64 NumPy restatement of the radially averaged power spectrum (acg_radial_spectrum, model.translate_spectrum) and of the
log-spectral distance: the reference the kernel and the evaluator's numbers are tested against.

For a real field x[h, w], S x S: F = fft2(x) (unnormalised, no taper, no mean removal), P = |F|^2 / S^2.  With signed integer
wavenumbers fy = ky if ky < S/2 else ky - S (fx alike) and s = fx^2 + fy^2, the bin of a cell is 0 for s = 0, else the largest
integer b with b (b - 1) < s: sqrt(s) rounded to the nearest integer, in integers.  Bins 0 .. S/2; the corners beyond are
dropped; psd[b] is the mean of P over the cells of bin b."""
import numpy as np


def wavenumbers(S):
    f = np.arange(S, dtype=np.int64)
    return np.where(f < S // 2, f, f - S)


def bin_index(S):
    """(S, S) int64: the bin of every cell [ky, kx] by the integer rule (a search, no floating point)"""
    f = wavenumbers(S)
    s = f[:, None] ** 2 + f[None, :] ** 2
    b = np.arange(1, 2 * S, dtype=np.int64)
    idx = np.searchsorted(b * (b - 1), s.ravel(), side="left")      # the number of b >= 1 with b (b - 1) < s
    return idx.reshape(S, S)


def bin_counts(S):
    """(S/2 + 1,) int64 cells per bin"""
    b = bin_index(S).ravel()
    return np.bincount(b[b <= S // 2], minlength=S // 2 + 1).astype(np.int64)


def bin_power(P):
    """(..., S, S) power planes -> (..., S/2 + 1) float64 bin means"""
    P = np.asarray(P, dtype=np.float64)
    S = P.shape[-1]
    assert P.shape[-2] == S
    nb = S // 2 + 1
    b = bin_index(S).ravel()
    keep = b < nb
    flat = P.reshape(-1, S * S)
    sums = np.zeros((flat.shape[0], nb), dtype=np.float64)
    for i in range(flat.shape[0]):
        np.add.at(sums[i], b[keep], flat[i, keep])
    return (sums / bin_counts(S)).reshape(P.shape[:-2] + (nb,))


def power_plane(x):
    """(..., S, S) float32 fields -> P in float64"""
    x = np.asarray(x)
    S = x.shape[-1]
    F = np.fft.fft2(x.astype(np.float64), axes=(-2, -1))
    return (F.real ** 2 + F.imag ** 2) / float(S * S)


def rapsd(x):
    """(..., S, S) fields -> (..., S/2 + 1) float64 radially averaged power spectra"""
    return bin_power(power_plane(x))


def lsd(p, q):
    """log-spectral distance in dB over bins 1 .. S/2 of (..., nb) spectra -> (...,) float64"""
    p = np.maximum(np.asarray(p, dtype=np.float64)[..., 1:], 1e-30)
    q = np.maximum(np.asarray(q, dtype=np.float64)[..., 1:], 1e-30)
    return np.sqrt(np.mean((10.0 * np.log10(p / q)) ** 2, axis=-1))


def lsd_channels(p, q):
    """(..., C, nb) spectra -> (...,): the mean of the per-channel distances"""
    return lsd(p, q).mean(axis=-1)


FIELD_KINDS = ("white", "red", "tanh_red", "plane_wave", "dc_noise")
FIELD_SIZES = (16, 32, 64, 128, 256, 512, 1024)


def _red(rs, shape):
    """power ~ k^-3 (amplitude ~ k^-1.5, no mean), every field scaled to max |x| = 1"""
    S = shape[-1]
    f = wavenumbers(S).astype(np.float64)
    k = np.sqrt(f[:, None] ** 2 + f[None, :] ** 2)
    amp = np.where(k > 0, np.maximum(k, 1.0) ** -1.5, 0.0)
    x = np.fft.ifft2(np.fft.fft2(rs.standard_normal(shape)) * amp).real
    return x / np.abs(x).max(axis=(-2, -1), keepdims=True)


def nyquist_row(S):
    """the last row m of the column kx = S/2 that ring S/2 still holds: (S/2)^2 + m^2 <= (S/2) (S/2 + 1), m = floor(sqrt(S/2))"""
    return int(np.floor(np.sqrt(S // 2)))


def make_fields(kind, S, rows=3, C=3, seed=0, m=None):
    """(rows, C, S, S) float32 test fields, seeded by (kind, S, seed): U(-1, 1) white noise; a red field; tanh(3 red) (what a
    generator head emits); the plane wave cos(2 pi (3 h + 4 w) / S); the constant 0.7 plus 1e-3 noise.  Beside FIELD_KINDS, the
    exact kind nyquist_column: (-1)^w cos(2 pi m h / S), all of its power S^2 / 4 each in the cells (ky = +-m, kx = S/2); m
    defaults to nyquist_row(S), one row further the cells lie in the dropped corner"""
    shape = (rows, C, S, S)
    if kind == "nyquist_column":
        h, w = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
        x = (1.0 - 2.0 * (w % 2)) * np.cos(2 * np.pi * (nyquist_row(S) if m is None else m) * h / S)
        return np.ascontiguousarray(np.broadcast_to(x, shape), dtype=np.float32)
    rs = np.random.RandomState(1000 * FIELD_KINDS.index(kind) + 7 * S + seed)
    if kind == "white":
        x = rs.uniform(-1, 1, shape)
    elif kind == "red":
        x = _red(rs, shape)
    elif kind == "tanh_red":
        x = np.tanh(3.0 * _red(rs, shape))
    elif kind == "plane_wave":
        h, w = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
        x = np.broadcast_to(np.cos(2 * np.pi * (3 * h + 4 * w) / S), shape)
    elif kind == "dc_noise":
        x = 0.7 + 1e-3 * rs.standard_normal(shape)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32)


def tolerance_needed(psd, ref, E):
    """the smallest tau with |psd - ref| <= tau sqrt(ref E) + tau^2 E in every bin (E: the field's mean square, broadcast over
    bins): the positive root of E tau^2 + sqrt(ref E) tau - |psd - ref| = 0"""
    d = np.abs(np.asarray(psd, dtype=np.float64) - ref)
    E = np.broadcast_to(np.asarray(E, dtype=np.float64)[..., None], d.shape)
    b = np.sqrt(ref * E)
    tau = 2.0 * d / (b + np.sqrt(b * b + 4.0 * E * d))               # the stable form of (-b + sqrt(b^2 + 4 E d)) / 2E
    return float(np.max(np.where(d > 0, tau, 0.0)))


# The kernel tests' bar: |psd - ref| <= TAU sqrt(ref E) + TAU^2 E per bin, E the field's mean square.  Measured, not chosen:
# torch.fft.fft2 in float32 on the CPU, binned in float64, needs tau = 1.3214e-4 over every bin, input and size above (`python
# tools/spectrum_bench.py --cpu-tolerance`; the largest is the constant-plus-noise field at S = 1024, whose DC coefficient of
# 0.7 S^2 is rounded to fp32: 2^-24 S).  The constant is 4 x that: a different butterfly order.
TAU = 4 * 1.3214e-4


def within(psd, ref, E, what, tau=TAU):
    """asserts that bar on finite spectra and prints the tau the comparison needed beside it"""
    d = np.abs(psd.astype(np.float64) - ref)
    bound = tau * np.sqrt(ref * E[..., None]) + tau ** 2 * E[..., None]
    print("%s: tau needed %.3e (allowed %.3e)" % (what, tolerance_needed(psd, ref, E), tau))
    assert np.all(np.isfinite(psd)) and np.all(d <= bound), (what, float((d / bound).max()), np.argwhere(d > bound)[:5])
