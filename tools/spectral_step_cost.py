#!/usr/bin/env python3
"""Milliseconds per training step with the spectral loss on (both weights positive) against the default step, in one process on
one GPU: the bench model (256 x 256 x 3, batch 32, ngf 32, 9 residual blocks, bf16x3), the step replayed as a captured graph,
each variant timed with device events over --steps steps after --warmup, the two variants alternating --rounds times.

    python tools/spectral_step_cost.py [--steps 10] [--warmup 4] [--rounds 2] [--size 256] [--batch 32]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=9)
    a = ap.parse_args()
    import torch
    import dtgan_amd  # noqa: F401
    from dtgan_amd import ops
    from dtgan_amd.model import AugmentedCycleGAN
    if not torch.cuda.is_available():
        raise SystemExit("spectral_step_cost needs a GPU")
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
                                 n_blocks=a.blocks, lambda_spec_A=lam, lambda_spec_B=lam)
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
    print(json.dumps(dict(tool="spectral_step_cost", size=S, batch=N, blocks=a.blocks, steps=a.steps, ms_per_step=ms,
                          best_off=off, best_on=on, added_ms=round(on - off, 3), added_percent=round(100 * (on - off) / off, 2),
                          loss_keys_on=keys)), flush=True)


if __name__ == "__main__":
    main()
