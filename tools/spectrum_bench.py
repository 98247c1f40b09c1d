#!/usr/bin/env python3
"""Milliseconds of the radially averaged power spectra of an A -> B ensemble (model.translate_spectrum's two halves) at the
geometries a user runs it, and the tolerance of the kernel's accuracy test.

  256 x 256 x 3, 512 x 512 x 1 and 64 x 64 x 3, N = 200 inputs, M = 16 samples, the bench model (ngf 32, 9 residual blocks)

For each case: the generator forwards of every group and the acg_radial_spectrum launches on their members, each timed with
device events around the same groups translate_spectrum forms (after a warm-up run), and the spectrum kernels' time over the
HBM floor of the traffic the design implies at 8 TB/s: the members read once, padded channels included, plus the half-spectrum
workspace written and read once above S = 128.  One JSON line per case.

    python tools/spectrum_bench.py [--reps 3] [--precision bf16x3] [--cases 256x3:16,512x1:16,64x3:16]

--cpu-tolerance needs no GPU: torch.fft.fft2 in float32 on the CPU, binned in float64 by tests/spectrum_ref.py, against the
float64 reference on exactly the inputs and sizes of tests/test_hip_spectrum.py; prints per size and overall the smallest tau
with |psd - ref| <= tau sqrt(ref E) + tau^2 E in every bin.  The test's constant is 4 x the overall value.

    python tools/spectrum_bench.py --cpu-tolerance
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 8e12


def cpu_tolerance():
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import spectrum_ref as R
    worst = 0.0
    for S in R.FIELD_SIZES:
        per = {}
        for kind in R.FIELD_KINDS:
            x = R.make_fields(kind, S)
            F = torch.fft.fft2(torch.from_numpy(x))                     # complex64 on the CPU
            P = (F.real.double() ** 2 + F.imag.double() ** 2).numpy() / float(S * S)
            E = np.mean(x.astype(np.float64) ** 2, axis=(-2, -1))
            per[kind] = R.tolerance_needed(R.bin_power(P), R.rapsd(x), E)
        worst = max(worst, max(per.values()))
        print(json.dumps(dict(tool="spectrum_bench", mode="cpu-tolerance", S=S, tau={k: float("%.3e" % v) for k, v in per.items()})),
              flush=True)
    print(json.dumps(dict(tool="spectrum_bench", mode="cpu-tolerance", tau_overall=float("%.4e" % worst),
                          test_constant_4x=float("%.4e" % (4 * worst)))), flush=True)


def spectrum_bytes(rows, S, C, Cp):
    read = rows * S * S * Cp * 4                                        # the members, padded channels included
    half = rows * C * S * (S // 2) * 8 if S > 128 else 0                # the packed half spectrum, written and read once
    return read + 2 * half + rows * C * (S // 2 + 1) * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-tolerance", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--cases", default="256x3:16,512x1:16,64x3:16")
    a = ap.parse_args()
    if a.cpu_tolerance:
        return cpu_tolerance()
    import torch
    import dtgan_amd  # noqa: F401
    from dtgan_amd import _lib, ops
    from dtgan_amd.model import AugmentedCycleGAN, ensemble_chunk
    from dtgan_amd.modules import _starts_with_conv, as_latent
    if not torch.cuda.is_available():
        raise SystemExit("spectrum_bench needs a GPU (or --cpu-tolerance)")
    ops.set_precision(a.precision)
    for case in a.cases.split(","):
        geo, M = case.split(":")
        S, C = (int(v) for v in geo.split("x"))
        M, N = int(M), a.N
        torch.manual_seed(0)
        opt = argparse.Namespace(input_nc=C, output_nc=C, ngf=32, nef=32, ndf=64, nlatent=16, lr=2e-4, beta1=0.5, max_gnorm=500.0,
                                 lambda_A=1.0, lambda_B=1.0, lambda_z_B=0.025, lambda_sup_A=0.1, lambda_sup_B=0.1, stoch_enc=False,
                                 z_gan=1, enc_A_B=1, no_lsgan=False, norm="instance", use_dropout=False, which_model_netG="resnet",
                                 which_model_netD="basic", gpu_ids=[0], monitor_gnorm=True, niter_decay=25, expr_dir="/tmp",
                                 n_blocks=9)
        model = AugmentedCycleGAN(opt, testing=True)
        G = model.netG_A_B
        G.eval()
        gen = torch.Generator(device="cuda").manual_seed(1)
        A = torch.rand(N, C, S, S, device="cuda", generator=gen) * 2 - 1
        z = torch.randn(N * M, 16, device="cuda", generator=gen)
        per = ensemble_chunk(32, S, S) // M
        psd = torch.empty((N * M, C, S // 2 + 1), device="cuda")

        def run():
            ev = []
            with torch.no_grad():
                for g0 in range(0, N, per):
                    n = min(per, N - g0)
                    a_ = A[g0:g0 + n]
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                    e[0].record()
                    x = ops.ToNHWC.apply(a_.unsqueeze(1).expand(n, M, C, S, S).reshape(n * M, C, S, S), _starts_with_conv(G.model))
                    members = G.forward_nhwc(x, as_latent(z[g0 * M:(g0 + n) * M]))
                    e[1].record()
                    ops.radial_spectrum(members, C, "nhwc", out=psd[g0 * M:(g0 + n) * M])
                    e[2].record()
                    ev.append(e)
                    cp = members.shape[-1]
            torch.cuda.synchronize()
            return sum(e[0].elapsed_time(e[1]) for e in ev), sum(e[1].elapsed_time(e[2]) for e in ev), cp

        run()
        gen_ms, spec_ms = [], []
        for _ in range(a.reps):
            g_ms, s_ms, Cp = run()
            gen_ms.append(g_ms)
            spec_ms.append(s_ms)
        nb = spectrum_bytes(N * M, S, C, Cp)
        s_med = sorted(spec_ms)[len(spec_ms) // 2]
        print(json.dumps(dict(tool="spectrum_bench", S=S, C=C, Cp=Cp, N=N, M=M, group_inputs=per, precision=a.precision,
                              kernel=_lib.query("acg_last_kernel").decode(),
                              generator_ms=[round(v, 2) for v in gen_ms], spectrum_ms=[round(v, 3) for v in spec_ms],
                              spectrum_share=round(s_med / sorted(gen_ms)[len(gen_ms) // 2], 4), spectrum_bytes=nb,
                              spectrum_GBps=round(nb / (s_med * 1e-3) / 1e9, 1),
                              spectrum_x_hbm_floor=round(s_med * 1e-3 / (nb / HBM), 2))), flush=True)
        del model, psd, A, z
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
