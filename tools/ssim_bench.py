#!/usr/bin/env python3
"""Milliseconds of the structural-similarity launches (csrc/ssim.hip) at the training geometry, beside their traffic floor and
the step they join:

  N = 32 fields of 256 x 256 x 3 as C4 NHWC image tensors (x and y: 33.6 MB each)

Timed with device events in one process, warm, the candidates interleaved inside every repetition:
  ssim_fwd       acg_ssim without the derivative maps (what ops.ssim and a weight-0 monitor launch), both launches
  ssim_fwd_maps  acg_ssim storing the maps a, b, c (3 x 32 x 3 x 246 x 246 floats: 69.7 MB written)
  ssim_bwd       acg_ssim_bwd: the maps through the window once more, the combine with x and y, one gradient written
  l1_fwd, l1_bwd acg_l1_fwd / acg_l1_bwd on the same tensors: the traffic floor (x and y read once, one gradient written)
  step, step_ssim  one AugmentedCycleGAN.train_instance (eager) of the default model and of the same model with
                 --lambda_ssim_A 0.5 --lambda_ssim_B 0.5, same inputs, alternating
Each kernel's bytes (from shapes) over its median time as GB/s.  One JSON line.

    python tools/ssim_bench.py [--reps 7] [--inner 10] [--precision bf16x3] [--no-step]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10, help="launches of a kernel per timed window")
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--N", type=int, default=32)
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--no-step", action="store_true", help="time the launches only")
    a = ap.parse_args()
    import torch
    import dtgan_amd  # noqa: F401
    from dtgan_amd import _lib, ops
    from dtgan_amd.model import AugmentedCycleGAN
    if not torch.cuda.is_available():
        raise SystemExit("ssim_bench needs a GPU")
    ops.set_precision(a.precision)
    N, C, S = a.N, 3, a.S
    Cp = ops.cimg(C)
    Sv = S - ops.SSIM_WINDOW + 1
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.zeros(N, S, S, Cp, device="cuda")
    y = torch.zeros(N, S, S, Cp, device="cuda")
    y[..., :C] = torch.tanh(torch.randn(N, S, S, C, device="cuda", generator=gen))
    x[..., :C] = (y[..., :C] + 0.1 * torch.randn(N, S, S, C, device="cuda", generator=gen)).clamp(-1, 1)
    out = torch.empty(N, C, 2, device="cuda")
    maps = torch.empty(3, N, C, Sv, Sv, device="cuda")
    gx = torch.empty_like(x)
    one = torch.ones(1, device="cuda")
    l1 = torch.empty((), device="cuda")
    need = _lib.query("acg_ssim_workspace_bytes", N, C, S, S)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rws, rnb = ops._red_ws()
    st = ops._stream()
    P = ops._ptr
    sx = (S * S * Cp, Cp, 1)

    def fwd(m):
        return lambda: _lib.call("acg_ssim", P(x), P(y), N, 1, C, S, S, sx[0], sx[1], sx[2], sx[0], sx[1], sx[2], 2.0, P(out), P(m), P(ws),
                                 need, st)
    runs = dict(
        ssim_fwd=fwd(None), ssim_fwd_maps=fwd(maps),
        ssim_bwd=lambda: _lib.call("acg_ssim_bwd", P(maps), P(x), P(y), P(one), N, C, Cp, S, S, sx[0], sx[1], sx[2], sx[0], sx[1], sx[2],
                                   P(gx), st),
        l1_fwd=lambda: _lib.call("acg_l1_fwd", P(x), P(y), N * S * S, C, Cp, P(l1), P(rws), rnb, st),
        l1_bwd=lambda: _lib.call("acg_l1_bwd", P(x), P(y), N * S * S, C, Cp, P(one), P(gx), None, st))
    image, mapb = N * S * S * Cp * 4, 3 * N * C * Sv * Sv * 4
    nbytes = dict(ssim_fwd=2 * image, ssim_fwd_maps=2 * image + mapb, ssim_bwd=mapb + 3 * image, l1_fwd=2 * image, l1_bwd=3 * image)

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
        def model(**kw):
            torch.manual_seed(0)
            opt = argparse.Namespace(input_nc=C, output_nc=C, ngf=32, nef=32, ndf=64, nlatent=16, lr=2e-4, beta1=0.5, max_gnorm=500.0,
                                     lambda_A=1.0, lambda_B=1.0, lambda_z_B=0.025, lambda_sup_A=0.1, lambda_sup_B=0.1, stoch_enc=False,
                                     z_gan=1, enc_A_B=1, no_lsgan=False, norm="instance", use_dropout=False,
                                     which_model_netG="resnet", which_model_netD="basic", gpu_ids=[0], monitor_gnorm=True,
                                     niter_decay=25, expr_dir="/tmp", n_blocks=a.blocks, grid_size=S, **kw)
            return AugmentedCycleGAN(opt, testing=True)
        A = torch.rand(N, C, S, S, device="cuda", generator=gen) * 2 - 1
        B = torch.rand(N, C, S, S, device="cuda", generator=gen) * 2 - 1
        z = torch.randn(N, 16, 1, 1, device="cuda", generator=gen)
        for name, m in (("step", model()), ("step_ssim", model(lambda_ssim_A=0.5, lambda_ssim_B=0.5))):
            steps[name] = (lambda m: lambda: m.train_instance(A, B, z))(m)
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
    res = dict(tool="ssim_bench", N=N, C=C, Cp=Cp, S=S, precision=a.precision, reps=a.reps, inner=a.inner)
    for k in runs:
        res[k + "_ms"] = [round(v, 4) for v in ms[k]]
        res[k + "_bytes"] = nbytes[k]
        res[k + "_GBps"] = round(nbytes[k] / (med[k] * 1e-3) / 1e9, 1)
    for k in steps:
        res[k + "_ms"] = [round(v, 2) for v in ms[k]]
    if steps:
        res["blocks"] = a.blocks
        res["step_ssim_over_step"] = round(med["step_ssim"] / med["step"], 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
