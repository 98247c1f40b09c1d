#!/usr/bin/env python3
"""The cost of the marginal loss (--lambda_marg_A / --lambda_marg_B).

Default: milliseconds per training step with the loss on (both weights positive) against the default step, in one process on
one GPU: the bench model (256 x 256 x 3, batch 32, ngf 32, 9 residual blocks, bf16x3), the step replayed as a captured graph,
each variant timed with device events over --steps steps after --warmup, the two variants alternating --rounds times.

--sort: microseconds per acg_field_sort call (ranks included) at 128^2 x 3 x 32, 256^2 x 3 x 32 and 512^2 x 1 x 16 (NHWC image
layout; 512^2: planar), the median of --rounds timings of --steps calls each, beside the traffic floor of the launch chain:
every launch reads and writes each 8-byte word once, words x 16 B x launches, at --tbps TB/s.

--cpu-tolerance needs no GPU: the loss in float32 with torch on the CPU (sort, mean over the rows, mean of the squares)
against the float64 reference on the batches of tests/marginal_ref.LOSS_CASES; the relative error it needs is the figure
behind LOSS_VALUE_TOL of tests/test_hip_marginal.py (4 x the largest).

    python tools/marginal_step_cost.py [--steps 10] [--warmup 4] [--rounds 2] [--size 256] [--batch 32]
    python tools/marginal_step_cost.py --sort [--steps 20] [--rounds 5]
    python tools/marginal_step_cost.py --cpu-tolerance
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cpu_tolerance():
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import marginal_ref as R
    worst = 0.0
    for H, W, rx, ry in R.LOSS_CASES:
        x, y = R.loss_batches(H, W, rx, ry)
        ref = R.marginal_loss(x, y)
        qx = torch.sort(torch.from_numpy(x).reshape(rx, 3, H * W), dim=-1).values.mean(0)
        qy = torch.sort(torch.from_numpy(y).reshape(ry, 3, H * W), dim=-1).values.mean(0)
        got = float(((qx - qy) ** 2).mean())
        err = abs(got - ref) / ref
        worst = max(worst, err)
        print(json.dumps(dict(tool="marginal_step_cost", mode="cpu-tolerance", H=H, W=W, rows_x=rx, rows_y=ry, loss64=ref, loss32=got,
                              relative_error=float("%.4e" % err))), flush=True)
    print(json.dumps(dict(tool="marginal_step_cost", mode="cpu-tolerance", relative_error_overall=float("%.4e" % worst),
                          numpy=np.__version__, torch=torch.__version__)), flush=True)


def sort_cost(a):
    import statistics
    import torch
    import dtgan_amd  # noqa: F401
    from dtgan_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("marginal_step_cost --sort needs a GPU")
    gen = torch.Generator(device="cuda").manual_seed(1)
    for S, C, N, layout in ((128, 3, 32, "nhwc"), (256, 3, 32, "nhwc"), (512, 1, 16, "nchw")):
        shape = (N, S, S, ops.cimg(C)) if layout == "nhwc" else (N, C, S, S)
        x = torch.rand(shape, device="cuda", generator=gen) * 2 - 1
        for _ in range(a.warmup):
            ops.field_sort(x, C, layout)
        path = _lib.query("acg_last_kernel").decode()
        us = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.steps):
                ops.field_sort(x, C, layout)
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / a.steps)
        ppad = 1 << (S * S - 1).bit_length()
        m = max(ppad // 8192, 1).bit_length() - 1
        launches = 1 + sum((s + 1) // 2 + 1 for s in range(1, m + 1))
        words = N * C * ppad
        floor_us = words * 16 * launches / (a.tbps * 1e12) * 1e6
        print(json.dumps(dict(tool="marginal_step_cost", mode="sort", size=S, C=C, rows=N, layout=layout, path=path, launches=launches,
                              words=words, us_per_call=round(statistics.median(us), 1), us_all=[round(u, 1) for u in us],
                              traffic_floor_us=round(floor_us, 1), floor_tbps=a.tbps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--sort", action="store_true")
    ap.add_argument("--tbps", type=float, default=4.0, help="--sort: the bandwidth of the traffic floor, TB/s")
    ap.add_argument("--cpu-tolerance", action="store_true")
    a = ap.parse_args()
    if a.cpu_tolerance:
        return cpu_tolerance()
    if a.sort:
        return sort_cost(a)
    import torch
    import dtgan_amd  # noqa: F401
    from dtgan_amd import ops
    from dtgan_amd.model import AugmentedCycleGAN
    if not torch.cuda.is_available():
        raise SystemExit("marginal_step_cost needs a GPU (or --cpu-tolerance)")
    ops.set_precision("bf16x3")
    S, N = a.size, a.batch
    gen = torch.Generator(device="cuda").manual_seed(1)
    A = torch.rand(N, 3, S, S, device="cuda", generator=gen) * 2 - 1
    B = torch.rand(N, 3, S, S, device="cuda", generator=gen) * 2 - 1
    z = torch.randn(N, 16, 1, 1, device="cuda", generator=gen)

    def build(lam):
        torch.manual_seed(0)
        opt = argparse.Namespace(input_nc=3, output_nc=3, ngf=32, nef=32, ndf=64, nlatent=16, lr=2e-4, beta1=0.5, max_gnorm=500.0,
                                 lambda_A=1.0, lambda_B=1.0, lambda_z_B=0.025, lambda_sup_A=0.1, lambda_sup_B=0.1, stoch_enc=False,
                                 z_gan=1, enc_A_B=1, no_lsgan=False, norm="instance", use_dropout=False, which_model_netG="resnet",
                                 which_model_netD="basic", gpu_ids=[0], monitor_gnorm=True, niter_decay=25, expr_dir="/tmp",
                                 n_blocks=a.blocks, lambda_marg_A=lam, lambda_marg_B=lam)
        m = AugmentedCycleGAN(opt, testing=True)
        m.enable_step_graph()
        for _ in range(a.warmup):
            m.train_instance(A, B, z)
        return m

    def timed(m):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.steps):
            losses = m.train_instance(A, B, z)[0]
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps, losses
    models = {"off": build(0.0), "on": build(0.1)}
    ms = {k: [] for k in models}
    for _ in range(a.rounds):
        for k, m in models.items():
            t, losses = timed(m)
            ms[k].append(round(t, 3))
            keys = len(losses)
    off, on = min(ms["off"]), min(ms["on"])
    print(json.dumps(dict(tool="marginal_step_cost", size=S, batch=N, blocks=a.blocks, steps=a.steps, ms_per_step=ms,
                          best_off=off, best_on=on, added_ms=round(on - off, 3), added_percent=round(100 * (on - off) / off, 2),
                          loss_keys_on=keys)), flush=True)


if __name__ == "__main__":
    main()
