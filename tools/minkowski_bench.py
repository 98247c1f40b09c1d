#!/usr/bin/env python3
"""Microseconds of the Minkowski counts (csrc/minkowski.hip: acg_minkowski, its two launches) beside their traffic floor and
beside a plain torch statement of the same counts, on 256 x 256 x 3 fields:

  batch  32 fields as a C4 NHWC image tensor (mink_hist<c4>): a training batch, and equally the evaluator's group of 2 inputs
         x 16 members
  mean   what follows per group: the ensemble mean's 2 x 3 planar fields (mink_hist<strided>)

at T = 31 thresholds (--mink_bins 32) and T = 255 (the most), on two kinds of field:

  spread    uniform values against their own quantiles as thresholds: every level equally likely, neighbours differ
  constant  one value everywhere: every lane of every wave adds to the same bin of each histogram, the worst case for
            contention without the aggregation of equal neighbours

Timed with device events in one process, warm, the candidates interleaved inside every repetition:
  mink_<kind>_T<T>        acg_minkowski on the batch
  mean_<kind>_T<T>        acg_minkowski on the ensemble mean's fields
  l1_fwd                  acg_l1_fwd on the two halves of the batch: the streaming floor (every value read once)
  torch_spread_T31        bucketize, pad, max / min of shifted views, bincount and a reversed cumsum on the batch
Ratios to the floor are of the medians.  The kernel's counts are compared with the torch statement's before anything is timed.
One JSON line.

    python tools/minkowski_bench.py [--reps 7] [--inner 10]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_counts(x, thr):
    """x (rows, C, H, W), thr (C, T) on the device -> (rows, C, T, 5) int64: the definition in plain torch"""
    import torch
    rows, C, H, W = x.shape
    T = thr.size(1)
    L = torch.stack([torch.bucketize(x[:, c], thr[c], right=True) for c in range(C)], 1)
    P = torch.nn.functional.pad(L, (1, 1, 1, 1))
    a, b, c, d = P[..., :-1, :-1], P[..., :-1, 1:], P[..., 1:, :-1], P[..., 1:, 1:]
    flat = lambda t: t.reshape(rows * C, -1)
    sets = (flat(L),
            torch.cat([flat(torch.maximum(P[..., 1:-1, :-1], P[..., 1:-1, 1:])), flat(torch.maximum(P[..., :-1, 1:-1], P[..., 1:, 1:-1]))], 1),
            torch.cat([flat(torch.minimum(P[..., 1:-1, :-1], P[..., 1:-1, 1:])), flat(torch.minimum(P[..., :-1, 1:-1], P[..., 1:, 1:-1]))], 1),
            flat(torch.maximum(torch.maximum(a, b), torch.maximum(c, d))), flat(torch.minimum(torch.minimum(a, b), torch.minimum(c, d))))
    base = (torch.arange(rows * C, device=x.device) * (T + 1))[:, None]
    out = []
    for s in sets:
        hist = torch.bincount((s + base).reshape(-1), minlength=rows * C * (T + 1)).view(rows * C, T + 1)
        out.append(hist.flip(1).cumsum(1).flip(1)[:, 1:])
    return torch.stack(out, -1).view(rows, C, T, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10, help="calls of an entry point per timed window")
    ap.add_argument("--N", type=int, default=32)
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--M", type=int, default=16)
    a = ap.parse_args()
    import torch
    import dtgan_amd  # noqa: F401
    from dtgan_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("minkowski_bench needs a GPU")
    N, C, S, M = a.N, 3, a.S, a.M
    if N % M or N % 2:
        raise SystemExit("--N must be even and a multiple of --M")
    Cp, n = ops.cimg(C), N // M
    gen = torch.Generator(device="cuda").manual_seed(1)
    fields = dict(spread=torch.zeros(N, S, S, Cp, device="cuda"), constant=torch.full((N, S, S, Cp), 0.3, device="cuda"))
    fields["spread"][..., :C] = torch.rand(N, S, S, C, device="cuda", generator=gen) * 2 - 1
    means = {k: v[:n, ..., :C].permute(0, 3, 1, 2).contiguous() for k, v in fields.items()}
    # uniform values on [-1, 1]: the quantiles k / (T + 1) are evenly spaced; the constant 0.3 lies between two of them
    thr = {T: (torch.arange(1, T + 1, device="cuda", dtype=torch.float32) / (T + 1) * 2 - 1).repeat(C, 1).contiguous() for T in (31, 255)}
    st, Pt = ops._stream(), ops._ptr
    nhwc, nchw = (S * S * Cp, Cp, 1), (C * S * S, 1, S * S)
    need = max(_lib.query("acg_minkowski_workspace_bytes", N, C, S, S, T) for T in thr)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty(N, C, 255, 5, device="cuda", dtype=torch.int64)
    rws, rnb = ops._red_ws()
    l1 = torch.empty((), device="cuda")

    def mink(x, rows, strides, T):
        nb = _lib.query("acg_minkowski_workspace_bytes", rows, C, S, S, T)
        return lambda: _lib.call("acg_minkowski", Pt(x), rows, C, S, S, strides[0], strides[1], strides[2], Pt(thr[T]), T, Pt(out), Pt(ws),
                                 nb, st)
    runs, paths = {}, {}
    for kind in fields:
        for T in thr:
            runs["mink_%s_T%d" % (kind, T)] = mink(fields[kind], N, nhwc, T)
            runs["mean_%s_T%d" % (kind, T)] = mink(means[kind], n, nchw, T)
    half = fields["spread"][:N // 2], fields["spread"][N // 2:]
    runs["l1_fwd"] = lambda: _lib.call("acg_l1_fwd", Pt(half[0]), Pt(half[1]), N // 2 * S * S, C, Cp, Pt(l1), Pt(rws), rnb, st)
    planar = {k: v[..., :C].permute(0, 3, 1, 2).contiguous() for k, v in fields.items()}
    runs["torch_spread_T31"] = lambda: torch_counts(planar["spread"], thr[31])
    for kind in fields:                                            # the kernel against the torch statement, before any timing
        for T in thr:
            runs["mink_%s_T%d" % (kind, T)]()
            paths["mink_%s_T%d" % (kind, T)] = _lib.query("acg_last_kernel").decode()
            got = out.view(-1)[:N * C * T * 5].view(N, C, T, 5).clone()
            if not torch.equal(got, torch_counts(planar[kind], thr[T])):
                raise SystemExit("acg_minkowski and the torch statement disagree (%s, T=%d)" % (kind, T))

    def timed(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / k * 1e3

    us = {k: [] for k in runs}
    for fn in runs.values():                                       # warm every shape
        timed(fn, 2)
    for _ in range(a.reps):                                        # interleaved: every repetition times every candidate
        for k, fn in runs.items():
            us[k].append(timed(fn, a.inner))
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    img = N * S * S * Cp * 4
    res = dict(tool="minkowski_bench", N=N, C=C, Cp=Cp, S=S, M=M, reps=a.reps, inner=a.inner, batch_bytes=img, paths=paths)
    for k in runs:
        res[k + "_us"] = [round(v, 1) for v in us[k]]
    res["l1_fwd_GBps"] = round(img / (med["l1_fwd"] * 1e-6) / 1e9, 1)
    for k in runs:
        if k.startswith("mink_"):
            res[k + "_GBps"] = round(img / (med[k] * 1e-6) / 1e9, 1)
            res[k + "_over_l1"] = round(med[k] / med["l1_fwd"], 2)
    for T in thr:
        res["constant_over_spread_T%d" % T] = round(med["mink_constant_T%d" % T] / med["mink_spread_T%d" % T], 2)
    res["torch_over_mink_spread_T31"] = round(med["torch_spread_T31"] / med["mink_spread_T31"], 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
