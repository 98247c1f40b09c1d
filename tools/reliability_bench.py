#!/usr/bin/env python3
"""Microseconds of the reliability tables (csrc/fss.hip: acg_reliability, fss_events twice and one fss_rel launch) beside
acg_fss with its ensemble output on the same tensors and the same windows: what the neighbourhood events and the table cost
next to the window counts they share their event planes with.  Two shapes:

  group  the evaluator's group: 32 fields (2 inputs x 16 members) of 256 x 256 x 3 as a C4 NHWC image tensor against 2 planar
         truths, T = 3 thresholds, windows 1, 5, 17 (--rel_windows' default); 17 planes do not fit LDS: fss_rel<global>
  plane  one 1024 x 1024 plane with 16 members (C = T = 1, planar), windows 1, 17, 65

and, for the evaluator's other two calls, the group's members one by one (x_per_y = 1, a truth row each: fss_rel<lds>).
Fields: box-smoothed noise, thresholds at its 0.5, 0.9 and 0.99 quantiles.  Device times: device events, warm, the candidates
interleaved inside every repetition.  The table's window-1 margins are compared with acg_fss's ensemble triple before anything
is reported.  There is no target: the numbers are recorded (the reliability section).  One JSON line.

    python tools/reliability_bench.py [--reps 5] [--inner 3]
"""
import argparse
import ctypes
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
    a = ap.parse_args()
    import numpy as np
    import torch
    import dtgan_amd  # noqa: F401
    from dtgan_amd import _lib, ops
    import minkowski_ref as K
    if not torch.cuda.is_available():
        raise SystemExit("reliability_bench needs a GPU")
    st, Pt = ops._stream(), ops._ptr

    def fields(rows, C, S, seed):
        x = K._box_smooth(np.random.RandomState(seed).standard_normal((rows, C, S, S)), 3)
        return (x / np.abs(x).max()).astype(np.float32)

    # name -> (rows of x, x_per_y, C, S, T, windows, x as a C4 NHWC tensor)
    shapes = dict(group=(32, 16, 3, 256, 3, (1, 5, 17), True), group_members=(32, 1, 3, 256, 3, (1, 5, 17), True),
                  plane=(16, 16, 1, 1024, 1, (1, 17, 65), False))
    runs, paths, keep = {}, {}, []
    for shape, (rows, M, C, S, T, win, c4) in shapes.items():
        x, y = fields(rows, C, S, 1), fields(rows // M, C, S, 2)
        thr = np.quantile(y.transpose(1, 0, 2, 3).reshape(C, -1).astype(np.float64), (0.5, 0.9, 0.99)[:T], axis=1).T.astype(np.float32)
        thr_d, yd = torch.from_numpy(np.ascontiguousarray(thr)).cuda(), torch.from_numpy(y).cuda()
        if c4:                                                     # as the generator hands its members over
            xd = torch.zeros(rows, S, S, ops.cimg(C), device="cuda")
            xd[..., :C] = torch.from_numpy(np.moveaxis(x, 1, 3)).cuda()
            sx = (S * S * xd.size(3), xd.size(3), 1)
        else:
            xd = torch.from_numpy(x).cuda()
            sx = (C * S * S, 1, S * S)
        sy, nw = (C * S * S, 1, S * S), len(win)
        warr = (ctypes.c_int * nw)(*win)
        need_f = _lib.query("acg_fss_workspace_bytes", rows, M, C, S, S, T, nw, 1)
        need_r = _lib.query("acg_reliability_workspace_bytes", rows, M, C, S, S, T, nw)
        ws_f = torch.empty(need_f, dtype=torch.uint8, device="cuda")
        ws_r = torch.empty(need_r, dtype=torch.uint8, device="cuda")
        out = torch.empty(rows, C, T, nw, 3, device="cuda", dtype=torch.int64)
        ens = torch.empty(rows // M, C, T, nw, 3, device="cuda", dtype=torch.int64)
        table = torch.empty(rows // M, C, T, nw, M + 1, 2, device="cuda", dtype=torch.int64)
        keep.append((xd, yd, thr_d, warr, ws_f, ws_r))

        def fss(xd=xd, yd=yd, rows=rows, M=M, C=C, S=S, sx=sx, sy=sy, thr_d=thr_d, T=T, warr=warr, nw=nw, out=out, ens=ens, ws=ws_f, need=need_f):
            _lib.call("acg_fss", Pt(xd), Pt(yd), rows, M, C, S, S, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], Pt(thr_d), T, warr, nw,
                      Pt(out), Pt(ens), Pt(ws), need, st)

        def rel(xd=xd, yd=yd, rows=rows, M=M, C=C, S=S, sx=sx, sy=sy, thr_d=thr_d, T=T, warr=warr, nw=nw, table=table, ws=ws_r, need=need_r):
            _lib.call("acg_reliability", Pt(xd), Pt(yd), rows, M, C, S, S, sx[0], sx[1], sx[2], sy[0], sy[1], sy[2], Pt(thr_d), T, warr,
                      nw, Pt(table), Pt(ws), need, st)
        runs["fss_" + shape], runs["rel_" + shape] = fss, rel
        fss()
        paths["fss_" + shape] = _lib.query("acg_last_kernel").decode()
        rel()
        paths["rel_" + shape] = _lib.query("acg_last_kernel").decode()
        t1, e1 = table[..., 0, :, :].cpu().numpy(), ens[..., 0, :].cpu().numpy()
        k = np.arange(M + 1)
        same = (np.array_equal((k * k * t1.sum(-1)).sum(-1), e1[..., 0]) and np.array_equal(t1[..., 1].sum(-1), e1[..., 1])
                and np.array_equal((k * t1[..., 1]).sum(-1), e1[..., 2]) and np.all(table.cpu().numpy().sum((-2, -1)) == S * S))
        if not same:
            raise SystemExit("acg_reliability and acg_fss disagree at window 1 (%s)" % shape)

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
    res = dict(tool="reliability_bench", reps=a.reps, inner=a.inner, shapes={k: list(v[:5]) + [list(v[5])] for k, v in shapes.items()},
               paths=paths)
    for k in runs:
        res[k + "_us"] = [round(v, 1) for v in us[k]]
    for shape in shapes:
        res["rel_over_fss_" + shape] = round(med["rel_" + shape] / med["fss_" + shape], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
