#!/usr/bin/env python3
"""Microseconds of the marginal evaluator's launches (csrc/marginal.hip: acg_field_sort, acg_marginal_scores) beside their
traffic floor, at two geometries of 256 x 256 x 3 fields as C4 NHWC image tensors:

  batch  32 fields against 32 paired truths (x_per_y = 1)
  group  the evaluator's group: 2 inputs x 16 members against 2 truths (x_per_y = 16), and what follows it per group: the
         ensemble mean's 2 x 3 fields (planar) against the same truths, and the truths alone

Timed with device events in one process, warm, the candidates interleaved inside every repetition:
  sort_x, sort_y       the acg_field_sort launches of the two operands, without ranks (8 launches each at 2^16 pixels)
  scores               acg_marginal_scores on the sorted fields: w, 10 levels, 99 edges
  l1_fwd               acg_l1_fwd on the same two tensors: the streaming floor (x and y read once)
  group_sort_members, group_sort_truth, group_scores    the same for the group
  mean_sort, mean_scores   the ensemble-mean call: 6 fields of 2^16 pixels, one workgroup each
  truth_scores         the truths alone (no distance)
Each launch's bytes (from shapes) over its median time as GB/s.  One JSON line.

    python tools/marginal_eval_bench.py [--reps 7] [--inner 10]
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
    ap.add_argument("--inner", type=int, default=10, help="calls of an entry point per timed window")
    ap.add_argument("--N", type=int, default=32)
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--M", type=int, default=16)
    a = ap.parse_args()
    import torch
    import dtgan_amd  # noqa: F401
    from dtgan_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("marginal_eval_bench needs a GPU")
    N, C, S, M = a.N, 3, a.S, a.M
    if N % M:
        raise SystemExit("--N must be a multiple of --M")
    Cp, P, n = ops.cimg(C), S * S, N // M
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.zeros(N, S, S, Cp, device="cuda")
    y = torch.zeros(N, S, S, Cp, device="cuda")
    y[..., :C] = torch.tanh(torch.randn(N, S, S, C, device="cuda", generator=gen))
    x[..., :C] = (y[..., :C] + 0.1 * torch.randn(N, S, S, C, device="cuda", generator=gen)).clamp(-1, 1)
    mean = torch.rand(n, C, S, S, device="cuda", generator=gen) * 2 - 1
    levels = (0.0, 0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 0.999, 1.0)
    L, E = len(levels), 99
    lv = (ctypes.c_double * L)(*levels)
    edges = torch.linspace(-1, 1, C * E, device="cuda").view(C, E).contiguous()
    st, Pt = ops._stream(), ops._ptr
    nhwc, nchw = (S * S * Cp, Cp, 1), (C * S * S, 1, S * S)
    need = _lib.query("acg_field_sort_workspace_bytes", N, C, S, S)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    rws, rnb = ops._red_ws()
    l1 = torch.empty((), device="cuda")

    def srt(rows):
        return torch.empty(rows, C, P, device="cuda")
    sx, sy, sm = srt(N), srt(N), srt(n)
    w = torch.empty(N, C, 2, device="cuda", dtype=torch.float64)
    q = torch.empty(N, C, L, device="cuda")
    below = torch.empty(N, C, E, device="cuda", dtype=torch.int32)

    def sort(src, rows, strides, dst):
        nb = _lib.query("acg_field_sort_workspace_bytes", rows, C, S, S)
        return lambda: _lib.call("acg_field_sort", Pt(src), rows, C, S, S, strides[0], strides[1], strides[2], Pt(dst), None,
                                 Pt(ws) if nb else None, nb, st)

    def scores(a_, b_, rows, per):
        return lambda: _lib.call("acg_marginal_scores", Pt(a_), Pt(b_), rows, per, C, P, lv, L, Pt(edges), E,
                                 Pt(w) if b_ is not None else None, Pt(q), Pt(below), st)
    runs = dict(
        sort_x=sort(x, N, nhwc, sx), sort_y=sort(y, N, nhwc, sy), scores=scores(sx, sy, N, 1),
        l1_fwd=lambda: _lib.call("acg_l1_fwd", Pt(x), Pt(y), N * S * S, C, Cp, Pt(l1), Pt(rws), rnb, st),
        group_sort_members=sort(x, N, nhwc, sx), group_sort_truth=sort(y, n, nhwc, sy), group_scores=scores(sx, sy, N, M),
        mean_sort=sort(mean, n, nchw, sm), mean_scores=scores(sm, sy, n, 1), truth_scores=scores(sy, None, n, 1))
    Ppad = 1 << (P - 1).bit_length()
    m = max(Ppad // 8192, 1).bit_length() - 1
    launches = 1 + sum((s + 1) // 2 + 1 for s in range(1, m + 1))

    def sort_bytes(rows, image):
        """the operand read once and the sorted fields written once; with a launch chain, the 8-byte words written by the first
        launch, read and written by every one between and read by the last"""
        words = 8 * rows * C * Ppad
        return image + 4 * rows * C * P + (0 if launches == 1 else words * 2 * (launches - 1))
    img = lambda rows: rows * S * S * Cp * 4
    plane = lambda rows: rows * C * P * 4
    nbytes = dict(sort_x=sort_bytes(N, img(N)), sort_y=sort_bytes(N, img(N)), scores=2 * plane(N), l1_fwd=2 * img(N),
                  group_sort_members=sort_bytes(N, img(N)), group_sort_truth=sort_bytes(n, img(n)), group_scores=2 * plane(N),
                  mean_sort=sort_bytes(n, plane(n)), mean_scores=2 * plane(n), truth_scores=plane(n))

    def timed(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / k * 1e3

    us = {k: [] for k in runs}
    for fn in (runs["sort_x"], runs["sort_y"], runs["group_sort_truth"], runs["mean_sort"]):   # the sorted operands exist
        timed(fn, 1)
    for fn in runs.values():                                     # warm every shape
        timed(fn, 2)
    for _ in range(a.reps):                                      # interleaved: every repetition times every candidate
        for k, fn in runs.items():
            us[k].append(timed(fn, a.inner))
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    res = dict(tool="marginal_eval_bench", N=N, C=C, Cp=Cp, S=S, M=M, levels=L, edges=E, sort_launches=launches, reps=a.reps,
               inner=a.inner)
    for k in runs:
        res[k + "_us"] = [round(v, 1) for v in us[k]]
        res[k + "_bytes"] = nbytes[k]
        res[k + "_GBps"] = round(nbytes[k] / (med[k] * 1e-6) / 1e9, 1)
    res["scores_over_sorts"] = round(med["scores"] / (med["sort_x"] + med["sort_y"]), 4)
    res["scores_over_l1"] = round(med["scores"] / med["l1_fwd"], 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
