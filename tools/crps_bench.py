#!/usr/bin/env python3
"""Milliseconds of the CRPS launches (csrc/crps.hip) beside the L1 pair on the same tensors, and of the paired step with the
term on beside the paired step with it off:

  x: N M fields of S x S x 3 as C4 NHWC image tensors (member m of input n at row n M + m), y: the N truths

Timed with device events in one process, warm, the candidates interleaved inside every repetition, at the batch shape
(--N 32 --S 256) and at 64 x 64:
  crps_fwd        acg_crps_fwd, both launches (x once, y once)
  crps_bwd        acg_crps_bwd (x once, y once, dx once)
  l1_fwd, l1_bwd  acg_l1_fwd / acg_l1_bwd on x against the truths repeated to x's rows: the baseline, the same bytes of x and dx
                  (L1 reads a truth per member where the CRPS kernels read it once per input; the bytes of each are listed)
  sup, sup_crps_M one AugmentedCycleGAN.supervised_train_instance (eager) of the default model and of the same model with
                  --lambda_crps_B 0.5 --crps_members M, M = 2, 4, 8, same inputs, alternating, at a batch of --step-N 16
Each kernel's bytes (from shapes) over its median time as GB/s.  One JSON line.

    python tools/crps_bench.py [--reps 7] [--inner 200] [--precision bf16x3] [--members 4] [--no-step]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=200, help="launches of a kernel per timed window (tens of microseconds each)")
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--N", type=int, default=32)
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--members", type=int, default=4, help="members per input of the timed launches")
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--step-N", type=int, default=16, help="batch of the timed paired steps (8 members of 32 inputs at 256 x 256 are "
                                                            "more images than one generator pass holds: model.ensemble_chunk)")
    ap.add_argument("--no-step", action="store_true", help="time the launches only")
    a = ap.parse_args()
    import torch
    import dtgan_amd  # noqa: F401
    from dtgan_amd import _lib, ops
    from dtgan_amd.model import AugmentedCycleGAN
    if not torch.cuda.is_available():
        raise SystemExit("crps_bench needs a GPU")
    ops.set_precision(a.precision)
    N, C, M = a.N, 3, a.members
    Cp = ops.cimg(C)
    gen = torch.Generator(device="cuda").manual_seed(1)
    one = torch.ones(1, device="cuda")
    st = ops._stream()
    P = ops._ptr
    rws, rnb = ops._red_ws()
    runs, nbytes = {}, {}
    keep = []
    for S in sorted({a.S, 64}, reverse=True):
        y = torch.zeros(N, S, S, Cp, device="cuda")
        y[..., :C] = torch.tanh(torch.randn(N, S, S, C, device="cuda", generator=gen))
        x = y.repeat_interleave(M, 0)
        x[..., :C] = (x[..., :C] + 0.1 * torch.randn(N * M, S, S, C, device="cuda", generator=gen)).clamp(-1, 1)
        yrep = y.repeat_interleave(M, 0).contiguous()
        out = torch.empty(N, C, 2, dtype=torch.float64, device="cuda")
        dx = torch.empty_like(x)
        l1 = torch.empty((), device="cuda")
        need = _lib.query("acg_crps_workspace_bytes", N * M, M, C, S, S)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        keep.append((x, y, yrep, out, dx, l1, ws))
        sx = (S * S * Cp, Cp, 1)
        cells = N * C * S * S
        cy, cp = ctypes.c_double(1.0 / (M * cells)), ctypes.c_double(ops.crps_weight(M, 0.95) / cells)
        tag = "_%d" % S

        def make(x=x, y=y, yrep=yrep, out=out, dx=dx, l1=l1, ws=ws, need=need, sx=sx, cy=cy, cp=cp, S=S):
            return dict(
                crps_fwd=lambda: _lib.call("acg_crps_fwd", P(x), P(y), N * M, M, C, S, S, sx[0], sx[1], sx[2], sx[0], sx[1], sx[2], P(out),
                                           P(ws), need, st),
                crps_bwd=lambda: _lib.call("acg_crps_bwd", P(x), P(y), P(one), N * M, M, C, Cp, S, S, sx[0], sx[1], sx[2], sx[0], sx[1],
                                           sx[2], cy, cp, P(dx), st),
                l1_fwd=lambda: _lib.call("acg_l1_fwd", P(x), P(yrep), N * M * S * S, C, Cp, P(l1), P(rws), rnb, st),
                l1_bwd=lambda: _lib.call("acg_l1_bwd", P(x), P(yrep), N * M * S * S, C, Cp, P(one), P(dx), None, st))
        for k, fn in make().items():
            runs[k + tag] = fn
        image, truth = N * M * S * S * Cp * 4, N * S * S * Cp * 4
        nbytes.update({"crps_fwd" + tag: image + truth, "crps_bwd" + tag: 2 * image + truth, "l1_fwd" + tag: 2 * image,
                       "l1_bwd" + tag: 3 * image})

    def timed(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / k

    steps = {}
    if not a.no_step:
        Ns, S = a.step_N, a.S

        def model(**kw):
            torch.manual_seed(0)
            opt = argparse.Namespace(input_nc=C, output_nc=C, ngf=32, nef=32, ndf=64, nlatent=16, lr=2e-4, beta1=0.5, max_gnorm=500.0,
                                     lambda_A=1.0, lambda_B=1.0, lambda_z_B=0.025, lambda_sup_A=0.1, lambda_sup_B=0.1, stoch_enc=False,
                                     z_gan=1, enc_A_B=1, no_lsgan=False, norm="instance", use_dropout=False,
                                     which_model_netG="resnet", which_model_netD="basic", gpu_ids=[0], monitor_gnorm=True,
                                     niter_decay=25, expr_dir="/tmp", n_blocks=a.blocks, grid_size=S, **kw)
            return AugmentedCycleGAN(opt, testing=True)
        A = torch.rand(Ns, C, S, S, device="cuda", generator=gen) * 2 - 1
        B = torch.rand(Ns, C, S, S, device="cuda", generator=gen) * 2 - 1
        z = torch.randn(Ns, 16, 1, 1, device="cuda", generator=gen)
        models = [("sup", model())] + [("sup_crps_%d" % m, model(lambda_crps_B=0.5, crps_members=m, crps_alpha=0.95)) for m in (2, 4, 8)]
        for name, m in models:
            steps[name] = (lambda m: lambda: m.supervised_train_instance(A, B, z))(m)
    ms = {k: [] for k in list(runs) + list(steps)}
    for fn in runs.values():                                     # warm every shape
        timed(fn, 2)
    for fn in steps.values():
        timed(fn, 2)
    for _ in range(a.reps):                                      # interleaved: every repetition times every candidate
        for k, fn in runs.items():
            ms[k].append(timed(fn, a.inner))
        for k, fn in steps.items():
            ms[k].append(timed(fn, 1))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    res = dict(tool="crps_bench", N=N, M=M, C=C, Cp=Cp, S=a.S, precision=a.precision, reps=a.reps, inner=a.inner)
    for k in runs:
        res[k + "_ms"] = [round(v, 4) for v in ms[k]]
        res[k + "_bytes"] = nbytes[k]
        res[k + "_GBps"] = round(nbytes[k] / (med[k] * 1e-3) / 1e9, 1)
    for k in steps:
        res[k + "_ms"] = [round(v, 2) for v in ms[k]]
    if steps:
        res["blocks"], res["step_N"] = a.blocks, a.step_N
        for k in steps:
            if k != "sup":
                res[k + "_over_sup"] = round(med[k] / med["sup"], 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
