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

--cpu-grad-tolerance, the same for the data gradient (tests/test_hip_spectrum_grad.py): 2 Re ifft2(w fft2(x)) with torch.fft
in float32 on the CPU against tests/spectrum_grad_ref.py in float64 over that test's sizes, fields and cotangents; the error
of a field is max |gx - ref| / (2 max_b |g[b] / count[b]| rms(x)).  Then ops.spectral_loss's value and input gradient
formed in float32 the same way (ring sums in float64, as the kernel forms them; torch's autograd) on that test's batches.
The test's constants are 4 x the overall values.

    python tools/spectrum_bench.py --cpu-grad-tolerance

--backward: microseconds per field of acg_radial_spectrum_bwd beside the forward's at 128 x 128 x 3 x 32, 256 x 256 x 3 x 32
and 512 x 512 x 1 x 32 (C4 NHWC, what the training step hands it), each over the HBM floor of one read of x and one write of
gx (padded channels included).  One JSON line per case.

    python tools/spectrum_bench.py --backward [--reps 20] [--bwd-cases 128x3:32,256x3:32,512x1:32]

--cpu-cross-tolerance, the same for the paired cross-spectra (tests/test_hip_cross_spectrum.py): Re(X conj Y) / S^2 from
torch.fft.fft2 in float32 on the CPU, binned in float64, against tests/cross_spectrum_ref.py over that test's pair kinds and
sizes; prints the smallest tau with |cxy - ref| <= tau (sqrt(pxx Ey) + sqrt(pyy Ex)) + tau^2 sqrt(Ex Ey) in every bin, and
beside it what pxx and pyy need under --cpu-tolerance's bound.  The test's constant is 4 x the overall value.

    python tools/spectrum_bench.py --cpu-cross-tolerance

--cross: microseconds per pair of acg_cross_spectrum beside the polarisation route to the same three spectra (x + y and x - y
materialised, acg_radial_spectrum on x, y and both: Cxy = (P(x+y) - P(x-y)) / 4), in one process with device events, at
64 x 64 x 3, 256 x 256 x 3 and 512 x 512 x 1, x C4 NHWC (what the generator emits) against a planar y.  One JSON line per case.

    python tools/spectrum_bench.py --cross [--reps 20] [--cross-cases 64x3:64,256x3:32,512x1:32]
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


def cpu_grad_tolerance(loss_only=False):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import spectrum_grad_ref as G
    import spectrum_ref as R
    worst = 0.0
    for S in (() if loss_only else R.FIELD_SIZES):
        per = {}
        for kind in R.FIELD_KINDS:
            x = R.make_fields(kind, S)
            F = torch.fft.fft2(torch.from_numpy(x))                     # complex64 on the CPU
            for ck in G.COTANGENT_KINDS:
                g = G.cotangents(ck, S, x.shape[:2])
                w = torch.from_numpy(G.cell_weights(S, g).astype(np.float32))
                gx = 2.0 * torch.fft.ifft2(w * F).real
                err = float(G.vjp_error(gx.numpy(), G.rapsd_vjp(x, g), g, x).max())
                per[kind] = max(per.get(kind, 0.0), err)
        worst = max(worst, max(per.values()))
        print(json.dumps(dict(tool="spectrum_bench", mode="cpu-grad-tolerance", S=S,
                              err={k: float("%.3e" % v) for k, v in per.items()})), flush=True)
    if not loss_only:
        print(json.dumps(dict(tool="spectrum_bench", mode="cpu-grad-tolerance", err_overall=float("%.4e" % worst),
                              test_constant_4x=float("%.4e" % (4 * worst)))), flush=True)
    # the loss itself in float32 (transform, power, logs; the ring sums in float64 as the forward kernel forms them) with
    # torch's autograd behind it, on the batches of the test of ops.spectral_loss
    worst_v = worst_g = 0.0
    for S in G.LOSS_SIZES:
        for kind in G.LOSS_KINDS:
            x, y = G.loss_batches(kind, S)
            ref, dref, g = G.spectral_loss_and_grad(x, y)
            b = torch.from_numpy(R.bin_index(S).ravel())
            keep, cnt = b <= S // 2, torch.from_numpy(R.bin_counts(S)).double()

            def mean_psd(t):
                F = torch.fft.fft2(t)
                P = ((F.real ** 2 + F.imag ** 2) / float(S * S)).reshape(t.shape[:2] + (S * S,))
                sums = torch.zeros(t.shape[:2] + (S // 2 + 1,), dtype=torch.float64).index_add(-1, b[keep], P.double()[..., keep])
                return (sums / cnt).float().mean(0)
            xt = torch.from_numpy(x).requires_grad_()
            d = torch.log(mean_psd(xt)[:, 1:] + 1e-6) - torch.log(mean_psd(torch.from_numpy(y))[:, 1:] + 1e-6)
            loss = (d * d).mean()
            loss.backward()
            ev = abs(float(loss.detach()) - ref) / ref
            eg = float(G.vjp_error(xt.grad.numpy(), dref, np.broadcast_to(g, (x.shape[0],) + g.shape), x).max())
            worst_v, worst_g = max(worst_v, ev), max(worst_g, eg)
            print(json.dumps(dict(tool="spectrum_bench", mode="cpu-grad-tolerance", loss=kind, S=S, value=float("%.6g" % ref),
                                  value_rel_err=float("%.3e" % ev), grad_err=float("%.3e" % eg))), flush=True)
    print(json.dumps(dict(tool="spectrum_bench", mode="cpu-grad-tolerance", loss_value_rel_err_overall=float("%.4e" % worst_v),
                          loss_grad_err_overall=float("%.4e" % worst_g), value_constant_4x=float("%.4e" % (4 * worst_v)),
                          grad_constant_4x=float("%.4e" % (4 * worst_g)))), flush=True)


def cpu_cross_tolerance():
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cross_spectrum_ref as X
    import spectrum_ref as R
    worst = worst_p = 0.0
    for S, rows, C in X.PAIR_CASES:
        per, per_p = {}, {}
        for kind in X.PAIR_KINDS:
            x, y = X.make_pairs(kind, S, rows, C)
            Fx, Fy = torch.fft.fft2(torch.from_numpy(x)), torch.fft.fft2(torch.from_numpy(y))     # complex64 on the CPU
            cxy = (Fx.real.double() * Fy.real.double() + Fx.imag.double() * Fy.imag.double()).numpy() / float(S * S)
            pxx = (Fx.real.double() ** 2 + Fx.imag.double() ** 2).numpy() / float(S * S)
            pyy = (Fy.real.double() ** 2 + Fy.imag.double() ** 2).numpy() / float(S * S)
            ref = X.cross_spectrum(x, y)
            Ex, Ey = np.mean(x.astype(np.float64) ** 2, axis=(-2, -1)), np.mean(y.astype(np.float64) ** 2, axis=(-2, -1))
            per[kind] = X.cross_tolerance_needed(R.bin_power(cxy), ref, Ex, Ey)
            per_p[kind] = max(R.tolerance_needed(R.bin_power(pxx), ref[..., 0, :], Ex),
                              R.tolerance_needed(R.bin_power(pyy), ref[..., 1, :], Ey))
        worst, worst_p = max(worst, max(per.values())), max(worst_p, max(per_p.values()))
        print(json.dumps(dict(tool="spectrum_bench", mode="cpu-cross-tolerance", S=S, rows=rows, C=C,
                              tau_cxy={k: float("%.3e" % v) for k, v in per.items()},
                              tau_pxx_pyy={k: float("%.3e" % v) for k, v in per_p.items()})), flush=True)
    print(json.dumps(dict(tool="spectrum_bench", mode="cpu-cross-tolerance", tau_cxy_overall=float("%.4e" % worst),
                          test_constant_4x=float("%.4e" % (4 * worst)), tau_pxx_pyy_overall=float("%.4e" % worst_p))), flush=True)


def cross_bench(a):
    import torch
    import dtgan_amd  # noqa: F401
    from dtgan_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("spectrum_bench needs a GPU (or one of the --cpu-* modes)")
    gen = torch.Generator(device="cuda").manual_seed(1)
    for case in a.cross_cases.split(","):
        geo, rows = case.split(":")
        S, C = (int(v) for v in geo.split("x"))
        rows, Cp = int(rows), 4
        x = torch.rand(rows, S, S, Cp, device="cuda", generator=gen) * 2 - 1
        y = torch.rand(rows, C, S, S, device="cuda", generator=gen) * 2 - 1

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

        def polarisation():
            xp = x[..., :C].permute(0, 3, 1, 2)
            s, d = (xp + y).contiguous(), (xp - y).contiguous()
            pxx, pyy = ops.radial_spectrum(x, C, "nhwc"), ops.radial_spectrum(y, C, "nchw")
            ps, pd = ops.radial_spectrum(s, C, "nchw"), ops.radial_spectrum(d, C, "nchw")
            return torch.stack([pxx, pyy, (ps - pd) * 0.25], 2)
        with torch.no_grad():
            fused_ms = timed(lambda: ops.cross_spectrum(x, y, C, "nhwc", "nchw"))
            kernel = _lib.query("acg_last_kernel").decode()
            pol_ms = timed(polarisation)
            diff = float((ops.cross_spectrum(x, y, C, "nhwc", "nchw") - polarisation()).abs().max())
        pairs = rows * C
        print(json.dumps(dict(tool="spectrum_bench", mode="cross", S=S, C=C, Cp=Cp, rows=rows, reps=a.reps, kernel=kernel,
                              fused_us_per_pair=round(fused_ms * 1e3 / pairs, 2), polarisation_us_per_pair=round(pol_ms * 1e3 / pairs, 2),
                              polarisation_over_fused=round(pol_ms / fused_ms, 2), max_abs_difference=float("%.3e" % diff))), flush=True)


def backward_bench(a):
    import torch
    import dtgan_amd  # noqa: F401
    from dtgan_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("spectrum_bench needs a GPU (or --cpu-tolerance / --cpu-grad-tolerance)")
    gen = torch.Generator(device="cuda").manual_seed(1)
    for case in a.bwd_cases.split(","):
        geo, rows = case.split(":")
        S, C = (int(v) for v in geo.split("x"))
        rows, Cp = int(rows), 4
        x = torch.rand(rows, S, S, Cp, device="cuda", generator=gen) * 2 - 1
        g = torch.randn(rows, C, S // 2 + 1, device="cuda", generator=gen)

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
        with torch.no_grad():
            fwd_ms = timed(lambda: ops.radial_spectrum(x, C, "nhwc"))
            fwd_kernel = _lib.query("acg_last_kernel").decode()
            bwd_ms = timed(lambda: ops.radial_spectrum_bwd(x, g, C, "nhwc"))
        fields, floor_s = rows * C, 2 * x.numel() * 4 / HBM
        print(json.dumps(dict(tool="spectrum_bench", mode="backward", S=S, C=C, Cp=Cp, rows=rows, reps=a.reps,
                              fwd_kernel=fwd_kernel, bwd_kernel=_lib.query("acg_last_kernel").decode(),
                              fwd_us_per_field=round(fwd_ms * 1e3 / fields, 2), bwd_us_per_field=round(bwd_ms * 1e3 / fields, 2),
                              bwd_over_fwd=round(bwd_ms / fwd_ms, 2), hbm_floor_us_per_field=round(floor_s * 1e6 / fields, 3),
                              bwd_x_hbm_floor=round(bwd_ms * 1e-3 / floor_s, 1))), flush=True)


def spectrum_bytes(rows, S, C, Cp):
    read = rows * S * S * Cp * 4                                        # the members, padded channels included
    half = rows * C * S * (S // 2) * 8 if S > 128 else 0                # the packed half spectrum, written and read once
    return read + 2 * half + rows * C * (S // 2 + 1) * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-tolerance", action="store_true")
    ap.add_argument("--cpu-grad-tolerance", action="store_true")
    ap.add_argument("--cpu-cross-tolerance", action="store_true")
    ap.add_argument("--backward", action="store_true")
    ap.add_argument("--cross", action="store_true")
    ap.add_argument("--cross-cases", default="64x3:64,256x3:32,512x1:32")
    ap.add_argument("--bwd-cases", default="128x3:32,256x3:32,512x1:32")
    ap.add_argument("--reps", type=int, default=None, help="default 3, with --backward or --cross 20")
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--cases", default="256x3:16,512x1:16,64x3:16")
    a = ap.parse_args()
    if a.cpu_tolerance:
        return cpu_tolerance()
    if a.cpu_grad_tolerance:
        return cpu_grad_tolerance()
    if a.cpu_cross_tolerance:
        return cpu_cross_tolerance()
    if a.reps is None:
        a.reps = 20 if a.backward or a.cross else 3
    if a.backward:
        return backward_bench(a)
    if a.cross:
        return cross_bench(a)
    import torch
    import dtgan_amd  # noqa: F401
    from dtgan_amd import _lib, ops
    from dtgan_amd.model import AugmentedCycleGAN, ensemble_chunk, eval_state
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
        gen = torch.Generator(device="cuda").manual_seed(1)
        A = torch.rand(N, C, S, S, device="cuda", generator=gen) * 2 - 1
        z = torch.randn(N * M, 16, device="cuda", generator=gen)
        per = ensemble_chunk(32, S, S) // M
        psd = torch.empty((N * M, C, S // 2 + 1), device="cuda")

        def stamp():
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            return e

        def run():
            ev = []
            with eval_state(G), torch.no_grad():
                e0 = stamp()                                       # the generator half: the step that advances the model's loop
                for g0, n, members in model.ensemble_groups(A, z, M, per):
                    e1 = stamp()
                    ops.radial_spectrum(members, C, "nhwc", out=psd[g0 * M:(g0 + n) * M])
                    e2 = stamp()
                    ev.append((e0, e1, e2))
                    e0, cp = e2, members.shape[-1]
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
