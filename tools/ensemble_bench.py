#!/usr/bin/env python3
"""Milliseconds of an A -> B ensemble (model.translate_ensemble's two halves) at the geometries a user runs it:

  256 x 256 x 3 and 512 x 512 x 1, N = 200 inputs, M = 16 and 64 samples, the bench model (ngf 32, 9 residual blocks)

For each case: the generator forwards of every group (the steps of model.ensemble_groups, the loop translate_ensemble runs)
and the acg_ensemble_stats launches, each timed with device events, and the stats kernel's bytes (members and target read,
maps written) over its time as GB/s and as a fraction of 8 TB/s.  One JSON line per case.

A case whose M samples of one input do not fit one generator pass (512 x 512 with M = 64: 63 images) is reported as skipped.

    python tools/ensemble_bench.py [--reps 3] [--precision bf16x3] [--cases 256x3:16,256x3:64,512x1:16,512x1:64]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 8e12
QS = (0.05, 0.5, 0.95)


def stats_bytes(N, M, H, W, C, Cp, nq):
    read = (N * M + N) * H * W * Cp * 4                       # members and target rows, padded channels included
    written = N * C * H * W * 4 * (3 + nq)                    # mean, std, crps_map, quantiles
    return read + written


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--cases", default="256x3:16,256x3:64,512x1:16,512x1:64")
    a = ap.parse_args()
    import torch
    import dtgan_amd  # noqa: F401
    from dtgan_amd import ops
    from dtgan_amd.model import AugmentedCycleGAN, ensemble_chunk, eval_state
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_bench needs a GPU")
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
        B = torch.rand(N, C, S, S, device="cuda", generator=gen) * 2 - 1
        z = torch.randn(N * M, 16, device="cuda", generator=gen)
        per = ensemble_chunk(32, S, S) // M
        if per < 1:
            print(json.dumps(dict(tool="ensemble_bench", S=S, C=C, N=N, M=M, skipped="a generator pass holds %d images at %d x %d, "
                                  "fewer than one input's %d samples" % (ensemble_chunk(32, S, S), S, S, M))), flush=True)
            continue
        out = ops.ensemble_outputs(N, M, C, S, S, len(QS), True, A.device)

        def stamp():
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            return e

        def run():
            ev = []
            with eval_state(G), torch.no_grad():
                e0 = stamp()                                       # the generator half: the step that advances the model's loop
                for g0, n, members in model.ensemble_groups(A, z, M, per):
                    tgt = ops.ToNHWC.apply(B[g0:g0 + n], members.shape[-1] == ops.cimg(C))
                    e1 = stamp()
                    ops.ensemble_stats(members, tgt, M, C, QS, out={k: v[g0:g0 + n] for k, v in out.items()})
                    e2 = stamp()
                    ev.append((e0, e1, e2))
                    e0, cp = e2, members.shape[-1]
            torch.cuda.synchronize()
            return sum(e[0].elapsed_time(e[1]) for e in ev), sum(e[1].elapsed_time(e[2]) for e in ev), cp

        run()
        gen_ms, stats_ms = [], []
        for _ in range(a.reps):
            g_ms, s_ms, Cp = run()
            gen_ms.append(g_ms)
            stats_ms.append(s_ms)
        nb = stats_bytes(N, M, S, S, C, Cp, len(QS))
        s_med = sorted(stats_ms)[len(stats_ms) // 2]
        print(json.dumps(dict(tool="ensemble_bench", S=S, C=C, N=N, M=M, group_inputs=per, precision=a.precision,
                              generator_ms=[round(v, 2) for v in gen_ms], stats_ms=[round(v, 3) for v in stats_ms],
                              stats_share=round(s_med / sorted(gen_ms)[len(gen_ms) // 2], 4), stats_bytes=nb,
                              stats_GBps=round(nb / (s_med * 1e-3) / 1e9, 1), stats_frac_of_8TBps=round(nb / (s_med * 1e-3) / HBM, 3),
                              stats_x_hbm_floor=round(s_med * 1e-3 / (nb / HBM), 2))), flush=True)
        del model, out, A, B, z
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
