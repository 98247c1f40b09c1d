#!/usr/bin/env python3
"""Milliseconds of the fractions-skill-score triples of an A -> B ensemble (ops.fss as model.translate_fss calls it) beside
the torch composition of the same scores, in one process with device events.

  32 inputs x 16 members x 3 channels at 256 x 256, members C4 NHWC (what the generator emits) against a planar truth, the
  evaluator's default windows 1,3,5,9,17,33 and three thresholds per channel (the 0.5, 0.9 and 0.99 quantiles of the truth)

HIP: one acg_fss call with x_per_y = 16 and the ensemble triples (events, box, slices, ens kernels).  torch, on the same
members held as planar NCHW: per threshold the comparison as float32, per window F.avg_pool2d with zero padding (the
fractions), the three products summed per field, and the same on the members' mean event plane for the ensemble.  Its float
sums depend on the pooling order; the integer triples do not.  The two are compared as FSS values.  One JSON line.

Beside it the intensity-scale triples of the same events (ops.fss_scales, what --fss_scales 1 adds per group: events, scales,
slices and the ensemble's scales kernels) on the same tensors, as scales_ms in that line, and a second JSON line for one
1024 x 1024 pair of one channel and one threshold, the largest field either call takes: fss_ms at the same windows and
scales_ms.  Both calls begin with the same events pass; a kernel trace of this tool splits their times by kernel.

    python tools/fss_bench.py [--reps 10] [--case 256x3:32x16] [--windows 1,3,5,9,17,33]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--case", default="256x3:32x16", help="SxC:NxM")
    ap.add_argument("--windows", default="1,3,5,9,17,33")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import dtgan_amd  # noqa: F401
    from dtgan_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("fss_bench needs a GPU")
    geo, nm = a.case.split(":")
    S, C = (int(v) for v in geo.split("x"))
    N, M = (int(v) for v in nm.split("x"))
    win = tuple(int(v) for v in a.windows.split(","))
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(N * M, S, S, 4, device="cuda", generator=gen) * 2 - 1
    y = torch.rand(N, C, S, S, device="cuda", generator=gen) * 2 - 1
    thr = torch.quantile(y.transpose(0, 1).reshape(C, -1)[:, ::7], torch.tensor([0.5, 0.9, 0.99], device="cuda"), dim=1).t().contiguous()
    T = thr.size(1)
    xp = x[..., :C].permute(0, 3, 1, 2).contiguous()               # the members as a torch pipeline holds them: planar NCHW

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

    def hip():
        return ops.fss(x, y, C, "nhwc", "nchw", thr, win, x_per_y=M, ensemble=True)

    def hip_scales():
        return ops.fss_scales(x, y, C, "nhwc", "nchw", thr, x_per_y=M, ensemble=True)

    def composed():
        """-> member triples (N M, C, T, nw, 3) and ensemble triples (N, C, T, nw, 3) of FRACTIONS, float32"""
        mem, ens = [], []
        for t in range(T):
            level = thr[:, t].view(1, C, 1, 1)
            bx, by = (xp >= level).float(), (y >= level).float()
            be = bx.view(N, M, C, S, S).mean(1)
            mw, ew = [], []
            for n in win:
                pf, po, pe = (F.avg_pool2d(b, n, stride=1, padding=n // 2) for b in (bx, by, be))
                pom = po.repeat_interleave(M, 0)
                mw.append(torch.stack([(pf * pf).sum((2, 3)), (pom * pom).sum((2, 3)), (pf * pom).sum((2, 3))], -1))
                ew.append(torch.stack([(pe * pe).sum((2, 3)), (po * po).sum((2, 3)), (pe * po).sum((2, 3))], -1))
            mem.append(torch.stack(mw, 2))
            ens.append(torch.stack(ew, 2))
        return torch.stack(mem, 2), torch.stack(ens, 2)

    with torch.no_grad():
        hip_ms = timed(hip)
        kernel = _lib.query("acg_last_kernel").decode()
        scales_ms = timed(hip_scales)
        scales_kernel = _lib.query("acg_last_kernel").decode()
        torch_ms = timed(composed)
        (o, e), (om, em) = hip(), composed()
        fss = lambda t: 2 * t[..., 2].sum(0).double() / (t[..., 0].sum(0).double() + t[..., 1].sum(0).double())
        fss_prob = 2 * M * e[..., 2].sum(0).double() / (e[..., 0].sum(0).double() + M * M * e[..., 1].sum(0).double())
        diff = float(torch.nan_to_num(fss(o) - fss(om)).abs().max())
        diff_prob = float(torch.nan_to_num(fss_prob - fss(em)).abs().max())
    print(json.dumps(dict(tool="fss_bench", S=S, C=C, N=N, M=M, T=T, windows=list(win), reps=a.reps, kernel=kernel,
                          hip_ms=round(hip_ms, 3), scales_ms=round(scales_ms, 3), scales_kernel=scales_kernel, torch_ms=round(torch_ms, 3), torch_over_hip=round(torch_ms / hip_ms, 2),
                          workspace_MiB=round(_lib.query("acg_fss_workspace_bytes", N * M, M, C, S, S, T, len(win), 1) / 2 ** 20, 1),
                          max_fss_difference=float("%.3e" % diff), max_fss_prob_difference=float("%.3e" % diff_prob))), flush=True)
    big = torch.rand(2, 1, 1024, 1024, device="cuda", generator=gen) * 2 - 1
    half = torch.zeros(1, 1, device="cuda")
    with torch.no_grad():
        pair_ms = timed(lambda: ops.fss(big[:1], big[1:], 1, "nchw", "nchw", half, win))
        pair_kernel = _lib.query("acg_last_kernel").decode()
        pair_scales_ms = timed(lambda: ops.fss_scales(big[:1], big[1:], 1, "nchw", "nchw", half))
    print(json.dumps(dict(tool="fss_bench", S=1024, C=1, N=1, M=1, T=1, windows=list(win), reps=a.reps, kernel=pair_kernel,
                          fss_ms=round(pair_ms, 3), scales_ms=round(pair_scales_ms, 3),
                          scales_kernel=_lib.query("acg_last_kernel").decode())), flush=True)


if __name__ == "__main__":
    main()
