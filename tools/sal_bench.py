#!/usr/bin/env python3
"""Microseconds of the SAL moments (csrc/components.hip: acg_sal, one launch per call and four per pass) beside
acg_components on the same tensors: what the mass, the peak and the centre of mass per object, the whole-field sums and the
finishing pass in double cost over the labelling they stand on.  Two shapes:

  group  the evaluator's group: 32 fields (2 inputs x 16 members) of 256 x 256 x 3 as a C4 NHWC image tensor, T = 1 threshold
         (--sal_quantiles 0.9): 96 planes
  plane  one 1024 x 1024 plane (C = T = 1, planar): 512 tiles; one workgroup finishes it

on two kinds of field:

  spread    box-smoothed noise cut at its 0.9 quantile: objects of every size, the evaluator's case
  constant  every cell 0.5 against the threshold 0: ONE object through every tile, every LDS atomic of a tile on one root

under 8-connectivity (--conn).  Device times: device events, warm, the candidates interleaved inside every repetition.  The
kernel's n and area are compared with acg_components' before anything is reported.  There is no target: the numbers are
recorded (the SAL section).  One JSON line.

    python tools/sal_bench.py [--reps 5] [--inner 3] [--conn 8]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3, help="calls of an entry point per timed window")
    ap.add_argument("--N", type=int, default=32)
    ap.add_argument("--conn", type=int, default=8, choices=[4, 8])
    a = ap.parse_args()
    import numpy as np
    import torch
    import dtgan_amd  # noqa: F401
    from dtgan_amd import _lib, ops
    import minkowski_ref as K
    if not torch.cuda.is_available():
        raise SystemExit("sal_bench needs a GPU")
    st, Pt = ops._stream(), ops._ptr

    def fields(kind, rows, C, S):
        if kind == "constant":
            return np.full((rows, C, S, S), 0.5, np.float32), np.zeros((C, 1), np.float32)
        x = K._box_smooth(np.random.RandomState(1).standard_normal((rows, C, S, S)), 3)
        x = (x / np.abs(x).max()).astype(np.float32)
        return x, np.quantile(x.transpose(1, 0, 2, 3).reshape(C, -1).astype(np.float64), 0.9, axis=1)[:, None].astype(np.float32)

    shapes = dict(group=(a.N, 3, 256, 1), plane=(1, 1, 1024, 1))
    runs, paths, passes = {}, {}, {}
    keep = []
    for shape, (rows, C, S, T) in shapes.items():
        need_c = _lib.query("acg_components_workspace_bytes", rows, C, S, S, T)
        need_s = _lib.query("acg_sal_workspace_bytes", rows, C, S, S, T)
        passes[shape] = -(-rows * C * T * S * S * 32 // need_s)
        ws_c = torch.empty(need_c, dtype=torch.uint8, device="cuda")
        ws_s = torch.empty(need_s, dtype=torch.uint8, device="cuda")
        out_c = torch.empty(rows, C, T, ops.COMP_STATS, device="cuda", dtype=torch.int64)
        out_s = (torch.empty(rows, C, 3, device="cuda", dtype=torch.int64), torch.empty(rows, C, T, 4, device="cuda", dtype=torch.int64),
                 torch.empty(rows, C, T, 2, device="cuda", dtype=torch.float64))
        for kind in ("spread", "constant"):
            x, thr = fields(kind, rows, C, S)
            thr_d = torch.from_numpy(thr).cuda()
            if shape == "group":                                   # a C4 NHWC image tensor, as the generator hands its members over
                xd = torch.zeros(rows, S, S, ops.cimg(C), device="cuda")
                xd[..., :C] = torch.from_numpy(np.moveaxis(x, 1, 3)).cuda()
                sx = (S * S * xd.size(3), xd.size(3), 1)
            else:
                xd = torch.from_numpy(x).cuda()
                sx = (C * S * S, 1, S * S)
            keep.append((xd, thr_d))
            key = "%s_%s" % (shape, kind)

            def comp(xd=xd, thr_d=thr_d, sx=sx, rows=rows, C=C, S=S, T=T, out_c=out_c, ws_c=ws_c, need_c=need_c):
                _lib.call("acg_components", Pt(xd), rows, C, S, S, sx[0], sx[1], sx[2], Pt(thr_d), T, a.conn, Pt(out_c), None, Pt(ws_c),
                          need_c, st)

            def sal(xd=xd, thr_d=thr_d, sx=sx, rows=rows, C=C, S=S, T=T, out_s=out_s, ws_s=ws_s, need_s=need_s):
                _lib.call("acg_sal", Pt(xd), rows, C, S, S, sx[0], sx[1], sx[2], Pt(thr_d), T, a.conn, -1.0, Pt(out_s[0]), Pt(out_s[1]),
                          Pt(out_s[2]), Pt(ws_s), need_s, st)
            runs["comp_" + key], runs["sal_" + key] = comp, sal
            sal()
            paths["sal_" + key] = _lib.query("acg_last_kernel").decode()
            comp()
            if not torch.equal(out_s[1][..., :2], out_c[..., :2]):
                raise SystemExit("acg_sal and acg_components disagree (%s)" % key)

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
        timed(fn, 1)
    for _ in range(a.reps):                                        # interleaved: every repetition times every candidate
        for k, fn in runs.items():
            us[k].append(timed(fn, a.inner))
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    res = dict(tool="sal_bench", N=a.N, conn=a.conn, reps=a.reps, inner=a.inner, shapes={k: list(v) for k, v in shapes.items()},
               passes=passes, paths=paths)
    for k in runs:
        res[k + "_us"] = [round(v, 1) for v in us[k]]
    for key in sorted(k[4:] for k in runs if k.startswith("sal_")):
        res["sal_over_comp_%s" % key] = round(med["sal_" + key] / med["comp_" + key], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
