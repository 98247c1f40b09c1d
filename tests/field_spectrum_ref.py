"""Float64 NumPy restatement of the whole-field spectra (acg_field_spectrum, acg_field_cross_spectrum,
model.translate_field_spectrum): the reference the kernels and `--metric field_spectrum` are tested against.

For a real field x[h, w], H x W with 16 <= H, W <= 1024, any integers: F = fft2(x) (unnormalised, no taper, no mean removal),
P = |F|^2 / (H W).  Signed wavenumbers fy = ky if 2 ky < H else ky - H, fx alike with W (for even N, k = N/2 maps to -N/2, as
spectrum_ref.wavenumbers does).  L = min(H, W).  The ring radius of a cell is L sqrt((fy/H)^2 + (fx/W)^2) rounded to the nearest
integer, in integers: the bin is 0 for fy = fx = 0, otherwise the largest b with
b (b - 1) H^2 W^2 < L^2 (fy^2 W^2 + fx^2 H^2); both sides stay below 2^60 for extents up to 1024.  Bins 0 .. L // 2; the cells
beyond are dropped; psd[b] is the mean of P over the cells of bin b.  (The boundary between rings b and b + 1 is
r^2 = b (b + 1): for the integer r^2 of a square field that is rounding exactly; for the rational r^2 of an ellipse it lies below
b + 1/2 by less than 1 / (8 b).)  Ring b is "b cycles per L pixels" along either axis, and
every bin is populated: the cell (b, 0) on the shorter axis has radius exactly b.  For H = W = S the rule is
spectrum_ref.bin_index's, term for term.

The cross form follows cross_spectrum_ref: per ring the means of Pxx, Pyy and Cxy = Re(X conj Y) / (H W)."""
import numpy as np

import spectrum_ref as R

FIELD_KINDS = R.FIELD_KINDS
# the shapes of the GPU accuracy test and of the tolerance measurement behind it (tools/field_spectrum_bench.py), each with the
# edge it walks
SHAPES = ((16, 16),        # both axes direct; forwarded to the square kernels
          (16, 32), (32, 16),   # both axes direct, but no square: the other side of the forwarding rule
          (17, 17),        # odd prime, M = 64, no Nyquist column, an unpaired last row
          (18, 30),        # even lengths that are no powers of two: a Nyquist on both axes
          (31, 16), (16, 31),   # one Bluestein axis and one direct axis, in both orders
          (20, 28),        # the driver test's shape
          (33, 65),        # 2 N - 1 = 65: the first M = 128; and M = 256
          (127, 129),      # either side of a power of two
          (321, 321),      # the README's field
          (1023, 513),     # M = 2048 on both axes: the largest padding
          (1000, 1024), (1024, 1000))   # the largest extents; one direct axis of 1024
LARGE = 321 * 321          # above: one layout per kind in the GPU test


def wavenumbers(N):
    f = np.arange(N, dtype=np.int64)
    return np.where(2 * f < N, f, f - N)


def bins(H, W):
    return min(H, W) // 2 + 1


def bin_index(H, W):
    """(H, W) int64: the bin of every cell [ky, kx] by the integer rule (a search, no floating point)"""
    L = min(H, W)
    fy, fx = wavenumbers(H), wavenumbers(W)
    s = L * L * (fy[:, None] ** 2 * (W * W) + fx[None, :] ** 2 * (H * H))
    b = np.arange(1, 2 * max(H, W) + 2, dtype=np.int64)
    idx = np.searchsorted(b * (b - 1) * (H * H * W * W), s.ravel(), side="left")   # the number of b >= 1 with b (b - 1) H^2 W^2 < s
    return idx.reshape(H, W)


def bin_counts(H, W):
    b = bin_index(H, W).ravel()
    nb = bins(H, W)
    return np.bincount(b[b < nb], minlength=nb).astype(np.int64)


def bin_power(P):
    """(..., H, W) planes -> (..., nb) float64 bin means"""
    P = np.asarray(P, dtype=np.float64)
    H, W = P.shape[-2:]
    nb = bins(H, W)
    b = bin_index(H, W).ravel()
    keep = b < nb
    flat = P.reshape(-1, H * W)
    sums = np.zeros((flat.shape[0], nb), dtype=np.float64)
    for i in range(flat.shape[0]):
        sums[i] = np.bincount(b[keep], weights=flat[i, keep], minlength=nb)
    return (sums / bin_counts(H, W)).reshape(P.shape[:-2] + (nb,))


def power_plane(x):
    x = np.asarray(x)
    H, W = x.shape[-2:]
    F = np.fft.fft2(x.astype(np.float64), axes=(-2, -1))
    return (F.real ** 2 + F.imag ** 2) / float(H * W)


def rapsd(x):
    """(..., H, W) fields -> (..., nb) float64 ring-averaged power spectra"""
    return bin_power(power_plane(x))


def cross_spectrum(x, y):
    """(..., H, W) paired fields -> (..., 3, nb) float64: the ring means pxx, pyy, cxy"""
    x, y = np.asarray(x), np.asarray(y)
    H, W = x.shape[-2:]
    X = np.fft.fft2(x.astype(np.float64), axes=(-2, -1))
    Y = np.fft.fft2(y.astype(np.float64), axes=(-2, -1))
    n = float(H * W)
    return np.stack([bin_power((X.real ** 2 + X.imag ** 2) / n), bin_power((Y.real ** 2 + Y.imag ** 2) / n),
                     bin_power((X * np.conj(Y)).real / n)], axis=-2)


def _red(rs, shape):
    """power ~ k^-3 in cycles per L pixels (no mean), every field scaled to max |x| = 1"""
    H, W = shape[-2:]
    L = min(H, W)
    k = L * np.sqrt((wavenumbers(H)[:, None] / float(H)) ** 2 + (wavenumbers(W)[None, :] / float(W)) ** 2)
    amp = np.where(k > 0, np.maximum(k, 1.0) ** -1.5, 0.0)
    x = np.fft.ifft2(np.fft.fft2(rs.standard_normal(shape)) * amp).real
    return x / np.abs(x).max(axis=(-2, -1), keepdims=True)


def make_fields(kind, H, W, rows=2, C=3, seed=0):
    """(rows, C, H, W) float32 test fields, seeded by (kind, H, W, seed): spectrum_ref.make_fields' kinds on H x W; the plane
    wave is cos(2 pi (3 h / H + 4 w / W))"""
    shape = (rows, C, H, W)
    rs = np.random.RandomState(1000 * FIELD_KINDS.index(kind) + 7 * H + 13 * W + seed)
    if kind == "white":
        x = rs.uniform(-1, 1, shape)
    elif kind == "red":
        x = _red(rs, shape)
    elif kind == "tanh_red":
        x = np.tanh(3.0 * _red(rs, shape))
    elif kind == "plane_wave":
        h, w = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        x = np.broadcast_to(np.cos(2 * np.pi * (3.0 * h / H + 4.0 * w / W)), shape)
    elif kind == "dc_noise":
        x = 0.7 + 1e-3 * rs.standard_normal(shape)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32)


def make_pair(H, W, rows=2, C=3, seed=0):
    """a prediction and a truth that share their large scales: x = tanh_red, y = 0.8 x rolled by (1, 2) + a faint red field"""
    x = make_fields("tanh_red", H, W, rows, C, seed)
    y = 0.8 * np.roll(x, (1, 2), axis=(-2, -1)) + 0.05 * make_fields("red", H, W, rows, C, seed + 1)
    return x, np.ascontiguousarray(y, dtype=np.float32)


# The bars of the whole-field kernels.  |psd - ref| <= TAU sqrt(ref E) + TAU^2 E per bin, E the field's mean square.  Measured,
# not chosen: the float32 Bluestein restatement on torch.fft of complex64 on the CPU, binned in float64, needs tau = 3.1424e-4
# over every bin, kind and shape of SHAPES (`python tools/field_spectrum_bench.py --cpu-tolerance`; the largest is the
# constant-plus-noise field at 1023 x 513, M = 2048 on both axes: the DC coefficient of 0.7 H W goes through two padded
# transforms and back).  The constant is 4 x that: a different butterfly order, as spectrum_ref.TAU.
TAU = 4 * 3.1424e-4
# |cxy - ref| <= CTAU (sqrt(pxx_ref Ey) + sqrt(pyy_ref Ex)) + CTAU^2 sqrt(Ex Ey) per bin (cross_spectrum_ref.cross_bound): the
# same run needs 3.7226e-5 for the co-spectrum of make_pair over those shapes (the largest at 1023 x 513); 4 x that.
CTAU = 4 * 3.7226e-5
