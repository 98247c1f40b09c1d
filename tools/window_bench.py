#!/usr/bin/env python3
"""Milliseconds of the two window kernels (csrc/window.hip) at the geometry they were written for, beside what they frame:

  N = 32 fields of 321 x 321 x 3, windows of 256 with overlap 64: 4 windows per field, 128 tiles (C4: 134 MB)

Timed with device events in one process, warm, the candidates interleaved inside every repetition:
  gather      acg_window_gather: 128 windows cut from the 32 fields
  blend       acg_window_blend: the 128 tiles back onto 32 canvases
  to_nhwc     acg_nchw_to_nhwc16 on 128 x 3 x 256 x 256, the same 134 MB on the NHWC side (the project's own layout kernel)
  generator   netG_A_B.forward_nhwc on the 128 tiles (ngf 32, 9 residual blocks): the pass the two kernels frame
Each kernel's bytes (from shapes: every field plane once and every tile once for the gather; every tile and every canvas
plane once for the blend; NCHW in plus NHWC out for the layout kernel) over its median time as GB/s.  One JSON line.

    python tools/window_bench.py [--reps 7] [--inner 10] [--precision bf16x3]
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
    ap.add_argument("--HW", type=int, default=321)
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--overlap", type=int, default=64)
    a = ap.parse_args()
    import torch
    import dtgan_amd  # noqa: F401
    from dtgan_amd import _lib, ops
    from dtgan_amd.model import AugmentedCycleGAN, eval_state
    if not torch.cuda.is_available():
        raise SystemExit("window_bench needs a GPU")
    ops.set_precision(a.precision)
    N, C, H, W, S = a.N, 3, a.HW, a.HW, a.S
    plan = ops.window_plan(H, W, S, a.overlap)
    T = plan.ny * plan.nx
    Cp = ops.cimg(C)
    torch.manual_seed(0)
    opt = argparse.Namespace(input_nc=C, output_nc=C, ngf=32, nef=32, ndf=64, nlatent=16, lr=2e-4, beta1=0.5, max_gnorm=500.0,
                             lambda_A=1.0, lambda_B=1.0, lambda_z_B=0.025, lambda_sup_A=0.1, lambda_sup_B=0.1, stoch_enc=False,
                             z_gan=1, enc_A_B=1, no_lsgan=False, norm="instance", use_dropout=False, which_model_netG="resnet",
                             which_model_netD="basic", gpu_ids=[0], monitor_gnorm=True, niter_decay=25, expr_dir="/tmp",
                             n_blocks=9, grid_size=S)
    G = AugmentedCycleGAN(opt, testing=True).netG_A_B
    gen = torch.Generator(device="cuda").manual_seed(1)
    fields = torch.rand(N, C, H, W, device="cuda", generator=gen) * 2 - 1
    z = torch.randn(N * T, 16, device="cuda", generator=gen)
    rows = [(n, oy, ox, 0) for n in range(N) for oy in plan.oy[:plan.ny] for ox in plan.ox[:plan.nx]]
    tab = ops.check_window_table(rows, N, H, W, S).cuda()
    tiles = torch.empty((N * T, S, S, Cp), device="cuda")
    canvas = torch.empty((N, C, H, W), device="cuda")
    nchw = torch.rand(N * T, C, S, S, device="cuda", generator=gen)
    nhwc = torch.empty((N * T, S, S, Cp), device="cuda")
    st = ops._stream()
    runs = dict(
        gather=lambda: _lib.call("acg_window_gather", ops._ptr(fields), ops._ptr(tab), ops._ptr(tiles), N, C, H, W, N * T, S, Cp, st),
        blend=lambda: ops.window_blend(tiles, plan, N, C, out=canvas),
        to_nhwc=lambda: _lib.call("acg_nchw_to_nhwc16", ops._ptr(nchw), ops._ptr(nhwc), N * T, C, S, S, Cp, st))
    tile_bytes = N * T * S * S * Cp * 4
    nbytes = dict(gather=N * C * H * W * 4 + tile_bytes, blend=tile_bytes + N * C * H * W * 4, to_nhwc=N * T * C * S * S * 4 + tile_bytes)

    def timed(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / k

    ms = {k: [] for k in list(runs) + ["generator"]}
    with eval_state(G), torch.no_grad():
        gen_pass = lambda: G.forward_nhwc(tiles, z)
        for fn in list(runs.values()) + [gen_pass]:              # warm every shape
            timed(fn, 2)
        for _ in range(a.reps):                                  # interleaved: every repetition times all four
            for k, fn in runs.items():
                ms[k].append(timed(fn, a.inner))
            ms["generator"].append(timed(gen_pass, 1))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    out = dict(tool="window_bench", N=N, C=C, H=H, W=W, S=S, overlap=a.overlap, windows=N * T, precision=a.precision,
               reps=a.reps, inner=a.inner)
    for k in runs:
        out[k + "_ms"] = [round(v, 4) for v in ms[k]]
        out[k + "_bytes"] = nbytes[k]
        out[k + "_GBps"] = round(nbytes[k] / (med[k] * 1e-3) / 1e9, 1)
    out["generator_ms"] = [round(v, 2) for v in ms["generator"]]
    out["pair_share_of_generator"] = round((med["gather"] + med["blend"]) / med["generator"], 5)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
