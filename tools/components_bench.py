#!/usr/bin/env python3
"""Microseconds of the connected components of excursion sets (csrc/components.hip: acg_components, four launches per pass)
beside acg_minkowski on the same operand and beside the host path it replaces - the device->host copy of the fields, then
scipy.ndimage.label and numpy.bincount plane by plane - at two shapes:

  group  the evaluator's group: 32 fields (2 inputs x 16 members) of 256 x 256 x 3 as a C4 NHWC image tensor, T = 31
         thresholds: 2976 planes, in passes of the 512 planes that 256 MiB hold
  plane  one 1024 x 1024 plane (C = T = 1, planar): 512 tiles, what the merge across seams costs when nothing else hides it

on three kinds of field:

  smooth  box-smoothed noise against evenly spaced thresholds: blobs of every size, the evaluator's case
  spiral  a one-cell arm with one-cell gaps, +-1 against thresholds 0: ONE component through every tile, the longest chases
  perc41  iid noise at p = 0.41, +-1 against thresholds 0: ragged clusters near the 8-connected percolation point

under 8-connectivity (--conn).  Device times: device events, warm, the candidates interleaved inside every repetition.  The
host path is timed once per case with the wall clock (it takes seconds).  The kernel's n and area are compared with the host
path's before anything is reported.  One JSON line.

    python tools/components_bench.py [--reps 5] [--inner 3] [--conn 8]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_path(x_dev, thr, conn):
    """x (rows, C, H, W) on the device, thr (C, T) on the host -> (seconds, (rows, C, T, 2) int64 n and area): the copy, then
    label and bincount per plane"""
    import numpy as np
    from scipy import ndimage
    structure = np.ones((3, 3), bool) if conn == 8 else ndimage.generate_binary_structure(2, 1)
    t0 = time.perf_counter()
    x = x_dev.cpu().numpy()
    rows, C = x.shape[:2]
    out = np.zeros((rows, C, thr.shape[1], 2), np.int64)
    for r in range(rows):
        for c in range(C):
            for t in range(thr.shape[1]):
                lab, n = ndimage.label(x[r, c] >= thr[c, t], structure=structure)
                areas = np.bincount(lab.ravel(), minlength=n + 1)[1:]
                out[r, c, t] = n, areas.sum()
    return time.perf_counter() - t0, out


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
    import components_ref as R
    import minkowski_ref as K
    if not torch.cuda.is_available():
        raise SystemExit("components_bench needs a GPU")
    st, Pt = ops._stream(), ops._ptr

    def fields(kind, rows, C, S):
        if kind == "smooth":
            x = K._box_smooth(np.random.RandomState(1).standard_normal((rows, C, S, S)), 3)
            return (x / np.abs(x).max()).astype(np.float32)
        return R.make_fields(kind, rows, C, S, S, None, seed=1)

    shapes = dict(group=(a.N, 3, 256, 31), plane=(1, 1, 1024, 1))
    runs, host, paths, passes = {}, {}, {}, {}
    keep = []
    for shape, (rows, C, S, T) in shapes.items():
        need_m = _lib.query("acg_minkowski_workspace_bytes", rows, C, S, S, T)
        need_c = _lib.query("acg_components_workspace_bytes", rows, C, S, S, T)
        passes[shape] = -(-rows * C * T * S * S * 8 // need_c)
        ws_m = torch.empty(need_m, dtype=torch.uint8, device="cuda")
        ws_c = torch.empty(need_c, dtype=torch.uint8, device="cuda")
        out_m = torch.empty(rows, C, T, 5, device="cuda", dtype=torch.int64)
        out_c = torch.empty(rows, C, T, ops.COMP_STATS, device="cuda", dtype=torch.int64)
        for kind in ("smooth", "spiral", "perc41"):
            x = fields(kind, rows, C, S)
            # evenly spaced thresholds inside the smooth fields' range; the binary kinds are cut at 0 by every threshold
            thr = np.tile((np.linspace(-0.5, 0.5, T) if kind == "smooth" else np.zeros(T)).astype(np.float32)[None], (C, 1))
            thr_d = torch.from_numpy(thr).cuda()
            if shape == "group":                                   # a C4 NHWC image tensor, as the generator hands its members over
                xd = torch.zeros(rows, S, S, ops.cimg(C), device="cuda")
                xd[..., :C] = torch.from_numpy(np.moveaxis(x, 1, 3)).cuda()
                sx = (S * S * xd.size(3), xd.size(3), 1)
            else:
                xd = torch.from_numpy(x).cuda()
                sx = (C * S * S, 1, S * S)
            planar = torch.from_numpy(x).cuda()
            keep.append((xd, thr_d, planar))
            key = "%s_%s" % (shape, kind)

            def comp(xd=xd, thr_d=thr_d, sx=sx, rows=rows, C=C, S=S, T=T, out_c=out_c, ws_c=ws_c, need_c=need_c):
                _lib.call("acg_components", Pt(xd), rows, C, S, S, sx[0], sx[1], sx[2], Pt(thr_d), T, a.conn, Pt(out_c), None, Pt(ws_c),
                          need_c, st)

            def mink(xd=xd, thr_d=thr_d, sx=sx, rows=rows, C=C, S=S, T=T, out_m=out_m, ws_m=ws_m, need_m=need_m):
                _lib.call("acg_minkowski", Pt(xd), rows, C, S, S, sx[0], sx[1], sx[2], Pt(thr_d), T, Pt(out_m), Pt(ws_m), need_m, st)
            runs["comp_" + key], runs["mink_" + key] = comp, mink
            comp()
            paths["comp_" + key] = _lib.query("acg_last_kernel").decode()
            got = out_c.cpu().numpy()
            secs, want = host_path(planar, thr, a.conn)
            if not np.array_equal(got[..., :2], want):
                raise SystemExit("acg_components and the host path disagree (%s)" % key)
            host[key] = secs

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
    res = dict(tool="components_bench", N=a.N, conn=a.conn, reps=a.reps, inner=a.inner, shapes={k: list(v) for k, v in shapes.items()},
               passes=passes, paths=paths)
    for k in runs:
        res[k + "_us"] = [round(v, 1) for v in us[k]]
    for key, secs in host.items():
        res["host_%s_us" % key] = round(secs * 1e6, 1)
        res["host_over_comp_%s" % key] = round(secs * 1e6 / med["comp_" + key], 1)
        res["comp_over_mink_%s" % key] = round(med["comp_" + key] / med["mink_" + key], 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
