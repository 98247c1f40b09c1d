#!/usr/bin/env python3
"""Whole-field spectra (ops.field_spectrum, ops.field_cross_spectrum): what they cost beside the power-of-two kernels, and the
tolerance of their accuracy test.

Default mode (needs a GPU): milliseconds per call of both ops on 48 planar fields (16 rows x 3 channels) of 321 x 321 and
1000 x 1024, beside ops.radial_spectrum on 48 fields of the next power of two (512, 1024), with device events after a warm-up
call; the fields' own bytes over the time, and the ratio to the power-of-two kernel stated as it is: Bluestein runs two
transforms of 2-4 x the length per axis.  One JSON line per shape.

    python tools/field_spectrum_bench.py [--reps 10] [--shapes 321x321,1000x1024]

--cpu-tolerance needs no GPU: a float32 restatement of the kernels' transform on torch.fft of complex64 on the CPU - per axis
the direct transform for a power of two, else Bluestein's chirp-z on transforms of the power of two M >= 2 N - 1 with the
kernels' chirp rule (n^2 reduced mod 2 N in integers, evaluated in float64, rounded once) - binned in float64 by
tests/field_spectrum_ref.py, against the float64 np.fft.fft2 spectra on every shape and field kind of
tests/test_hip_field_spectrum.py.  Prints per shape and overall the smallest tau with |psd - ref| <= tau sqrt(ref E) + tau^2 E
in every bin (spectrum_ref.tolerance_needed), and the same for the co-spectrum of field_spectrum_ref.make_pair under
cross_spectrum_ref's bound.  An independent fp32 computation of the same algorithm, not the kernel; the test's constants are
4 x the overall values.

    python tools/field_spectrum_bench.py --cpu-tolerance
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def padded(N):
    """the length of the transforms that carry a transform of length N"""
    if N & (N - 1) == 0:
        return N
    M = 1
    while M < 2 * N - 1:
        M <<= 1
    return M


def chirp(N):
    """c[n] = exp(-i pi n^2 / N) as complex64, the argument reduced mod 2 N in integers"""
    import numpy as np
    n = np.arange(N, dtype=np.int64)
    return np.exp(-1j * np.pi * ((n * n) % (2 * N)) / N).astype(np.complex64)


def dft_f32(a):
    """the transform along the last axis of a complex64 tensor as the kernels form it, in float32 on the CPU"""
    import torch
    N = a.shape[-1]
    M = padded(N)
    if M == N:
        return torch.fft.fft(a)
    c = torch.from_numpy(chirp(N))
    b = torch.zeros(M, dtype=torch.complex64)
    b[:N] = c.conj()
    b[M - N + 1:] = c[1:].conj().flip(0)
    u = torch.zeros(a.shape[:-1] + (M,), dtype=torch.complex64)
    u[..., :N] = a * c
    return torch.fft.ifft(torch.fft.fft(u) * torch.fft.fft(b))[..., :N] * c


def fft2_f32(x):
    """fft2 of (..., H, W) float32 fields: rows, then columns -> complex64 tensor"""
    import torch
    F = dft_f32(torch.from_numpy(x).to(torch.complex64))
    return dft_f32(F.transpose(-1, -2).contiguous()).transpose(-1, -2)


def restated_tolerances(H, W, rows=2, C=3):
    """-> ({kind: tau of the spectrum}, tau of the co-spectrum of make_pair) of the float32 restatement at H x W"""
    import numpy as np
    import cross_spectrum_ref as X
    import field_spectrum_ref as F
    import spectrum_ref as R
    n = float(H * W)
    per = {}
    for kind in F.FIELD_KINDS:
        x = F.make_fields(kind, H, W, rows, C)
        T = fft2_f32(x)
        P = (T.real.double() ** 2 + T.imag.double() ** 2).numpy() / n
        per[kind] = R.tolerance_needed(F.bin_power(P), F.rapsd(x), np.mean(x.astype(np.float64) ** 2, axis=(-2, -1)))
    x, y = F.make_pair(H, W, rows, C)
    Tx, Ty = fft2_f32(x), fft2_f32(y)
    cxy = (Tx.real.double() * Ty.real.double() + Tx.imag.double() * Ty.imag.double()).numpy() / n
    Ex, Ey = np.mean(x.astype(np.float64) ** 2, axis=(-2, -1)), np.mean(y.astype(np.float64) ** 2, axis=(-2, -1))
    return per, X.cross_tolerance_needed(F.bin_power(cxy), F.cross_spectrum(x, y), Ex, Ey)


def cpu_tolerance():
    import field_spectrum_ref as F
    worst = worst_c = 0.0
    for H, W in F.SHAPES:
        per, cross = restated_tolerances(H, W)
        worst, worst_c = max(worst, max(per.values())), max(worst_c, cross)
        print(json.dumps(dict(tool="field_spectrum_bench", mode="cpu-tolerance", H=H, W=W, M_rows=padded(W), M_cols=padded(H),
                              tau={k: float("%.3e" % v) for k, v in per.items()}, tau_cxy=float("%.3e" % cross))), flush=True)
    print(json.dumps(dict(tool="field_spectrum_bench", mode="cpu-tolerance", tau_overall=float("%.4e" % worst),
                          test_constant_4x=float("%.4e" % (4 * worst)), tau_cxy_overall=float("%.4e" % worst_c),
                          cross_constant_4x=float("%.4e" % (4 * worst_c)))), flush=True)


def bench(a):
    import torch
    import dtgan_amd  # noqa: F401
    from dtgan_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("field_spectrum_bench needs a GPU (or --cpu-tolerance)")
    gen = torch.Generator(device="cuda").manual_seed(1)
    rows, C = 16, 3

    def timed(fn):
        fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.reps + 1)]
        ev[0].record()
        for i in range(a.reps):
            fn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(a.reps))
        return ms[len(ms) // 2]

    for shape in a.shapes.split(","):
        H, W = (int(v) for v in shape.split("x"))
        P = 1
        while P < max(H, W):
            P <<= 1
        x = torch.rand(rows, C, H, W, device="cuda", generator=gen) * 2 - 1
        y = torch.rand(rows, C, H, W, device="cuda", generator=gen) * 2 - 1
        xp = torch.rand(rows, C, P, P, device="cuda", generator=gen) * 2 - 1
        with torch.no_grad():
            f_ms = timed(lambda: ops.field_spectrum(x, C, "nchw"))
            kernel = _lib.query("acg_last_kernel").decode()
            c_ms = timed(lambda: ops.field_cross_spectrum(x, y, C, "nchw", "nchw"))
            p_ms = timed(lambda: ops.radial_spectrum(xp, C, "nchw"))
            p_kernel = _lib.query("acg_last_kernel").decode()
        nbytes = x.numel() * 4
        print(json.dumps(dict(tool="field_spectrum_bench", H=H, W=W, fields=rows * C, reps=a.reps, kernel=kernel,
                              field_spectrum_ms=round(f_ms, 3), field_spectrum_GBps=round(nbytes / (f_ms * 1e-3) / 1e9, 2),
                              field_cross_spectrum_ms=round(c_ms, 3),
                              field_cross_spectrum_GBps=round(2 * nbytes / (c_ms * 1e-3) / 1e9, 2),
                              pow2=P, pow2_kernel=p_kernel, radial_spectrum_pow2_ms=round(p_ms, 3),
                              radial_spectrum_pow2_GBps=round(xp.numel() * 4 / (p_ms * 1e-3) / 1e9, 2),
                              field_over_pow2=round(f_ms / p_ms, 2))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-tolerance", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="321x321,1000x1024")
    a = ap.parse_args()
    if a.cpu_tolerance:
        return cpu_tolerance()
    return bench(a)


if __name__ == "__main__":
    main()
