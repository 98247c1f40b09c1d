#!/usr/bin/env python3
"""Milliseconds per iterate of the variational bound (evaluate.variational_ubo: the generator forward and backward to the
latent, the likelihood, KLD and RMSprop tail) at the two geometries that run it:

  a  test.py's own:                         64 x 64 x 3, N = 200, ngf 32, 3 residual blocks
  b  train.py's per-epoch evaluation at bench geometry: 256 x 256 x 3, N = 100, ngf 32, 9 residual blocks

Only the public evaluate.variational_ubo and the model are used, so the script measures any checkout, an older one
included: --tree <checkout> (default: the one this script belongs to).  Each repetition times a call of K iterates and one
of K0 iterates with device events (each ending in a synchronise); (T(K) - T(K0)) / (K - K0) removes the per-batch set-up (encoder, conversions, the final read).
Prints one JSON line.

    python tools/bound_iter_bench.py --geometry a [--tree DIR] [--iters 40] [--iters0 5] [--reps 3] [--precision bf16x3]
"""
import argparse
import json
import os
import sys
import time

GEOMETRIES = {"a": dict(S=64, N=200, n_blocks=3), "b": dict(S=256, N=100, n_blocks=9)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", choices=sorted(GEOMETRIES), default="a")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--iters0", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5, help="iterates of the untimed first call")
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout whose dtgan_amd is measured (default: this one)")
    a = ap.parse_args()
    if a.iters <= a.iters0 or a.iters0 < 1:
        ap.error("need 1 <= --iters0 < --iters")
    root = os.path.abspath(a.tree)
    if not os.path.isfile(os.path.join(root, "dtgan_amd.py")):
        ap.error("--tree %s holds no dtgan_amd.py" % root)
    sys.path.insert(0, root)
    import torch
    import dtgan_amd  # noqa: F401
    if os.path.dirname(os.path.abspath(dtgan_amd.__file__)) != os.path.join(root, "domain-transfer-gan_amd"):
        raise SystemExit("dtgan_amd was imported from %s, not from --tree %s" % (dtgan_amd.__file__, root))
    from dtgan_amd import ops
    from dtgan_amd.evaluate import variational_ubo
    from dtgan_amd.model import AugmentedCycleGAN

    if not torch.cuda.is_available():
        raise SystemExit("bound_iter_bench needs a GPU")
    g = GEOMETRIES[a.geometry]
    ops.set_precision(a.precision)
    torch.manual_seed(0)
    opt = argparse.Namespace(input_nc=3, output_nc=3, ngf=32, nef=32, ndf=64, nlatent=16, lr=2e-4, beta1=0.5, max_gnorm=500.0,
                             lambda_A=1.0, lambda_B=1.0, lambda_z_B=0.025, lambda_sup_A=0.1, lambda_sup_B=0.1, stoch_enc=False,
                             z_gan=1, enc_A_B=1, no_lsgan=False, norm="instance", use_dropout=False, which_model_netG="resnet",
                             which_model_netD="basic", gpu_ids=[0], monitor_gnorm=True, niter_decay=25, expr_dir="/tmp",
                             n_blocks=g["n_blocks"])
    model = AugmentedCycleGAN(opt, testing=True)
    gen = torch.Generator(device="cuda").manual_seed(1)
    A = torch.rand(g["N"], 3, g["S"], g["S"], device="cuda", generator=gen) * 2 - 1
    B = torch.rand(g["N"], 3, g["S"], g["S"], device="cuda", generator=gen) * 2 - 1

    def timed(k):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = variational_ubo(model, A, B, k)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    t0 = time.time()
    timed(a.warmup)
    per_iter, last = [], None
    for _ in range(a.reps):
        tk, last = timed(a.iters)
        tk0, _ = timed(a.iters0)
        per_iter.append((tk - tk0) / (a.iters - a.iters0))
    per_iter.sort()
    print(json.dumps(dict(tool="bound_iter_bench", tree=root, geometry=a.geometry, S=g["S"], N=g["N"], n_blocks=g["n_blocks"],
                          precision=a.precision, iters=a.iters, iters0=a.iters0, ms_per_iter=per_iter,
                          ms_per_iter_median=per_iter[len(per_iter) // 2], last_ubo_kld_bpp=list(last),
                          wall_s=round(time.time() - t0, 1))))


if __name__ == "__main__":
    main()
