#!/usr/bin/env python3
"""Microseconds of the per-cell statistics (csrc/cell_stats.hip: acg_cell_stats, cell_mom and, with the parts on, cell_evt and
two cell_hist launches) beside acg_ensemble_stats on the same tensors and beside acg_l1_fwd, the streaming floor the other
benches use (two tensors of the members' size read once).  Two shapes:

  group  the evaluator's group: 240 fields (15 inputs x 16 members, what one generator pass holds) of 256 x 256 x 3 as C4 NHWC
         image tensors against 15 NHWC truths
  plane  one 1024 x 1024 x 1 group of 16 members, NHWC as the generator hands it over

each with the parts off (moments alone), with T = 2 thresholds, with E = 31 edges (--map_bins 32), and with both.  The state
lives in (9 8 + 32 T + 8 (E + 1)) bytes per cell and channel and is read and written once per launch.  Fields: correlated
noise.  Device times: device events, warm, the candidates interleaved inside every repetition.  The histogram columns are
checked to sum to the rows before anything is reported.  There is no target: the numbers are recorded: per
variant the time, its multiple of acg_ensemble_stats's and its time per input byte as a multiple of acg_l1_fwd's.  One JSON
line.

    python tools/cell_stats_bench.py [--reps 5] [--inner 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
QS = (0.05, 0.5, 0.95)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3, help="calls of an entry point per timed window")
    a = ap.parse_args()
    import torch
    import dtgan_amd  # noqa: F401
    from dtgan_amd import _lib, ops
    if not torch.cuda.is_available():
        raise SystemExit("cell_stats_bench needs a GPU")
    st, Pt = ops._stream(), ops._ptr
    gen = torch.Generator(device="cuda").manual_seed(1)
    # name -> (rows of x, x_per_y, C, S)
    shapes = dict(group=(240, 16, 3, 256), plane=(16, 16, 1, 1024))
    variants = dict(mom=(0, 0), evt=(2, 0), hist=(0, 31), all=(2, 31))
    runs, paths, nbytes, keep = {}, {}, {}, []
    for shape, (rows, M, C, S) in shapes.items():
        Cp, Ny = ops.cimg(C), rows // M
        y = torch.zeros(Ny, S, S, Cp, device="cuda")
        y[..., :C] = torch.randn(Ny, S, S, C, device="cuda", generator=gen)
        x = torch.zeros(rows, S, S, Cp, device="cuda")
        x[..., :C] = 0.6 * y[..., :C].repeat_interleave(M, 0) + 0.8 * torch.randn(rows, S, S, C, device="cuda", generator=gen)
        x2 = x.flip(0).contiguous()
        thr = torch.tensor([[0.5, 1.5]] * C, device="cuda")
        edges = torch.linspace(-2, 2, 31, device="cuda").repeat(C, 1).contiguous()
        out = ops.ensemble_outputs(Ny, M, C, S, S, len(QS), True, x.device)
        rws, rnb = ops._red_ws()
        l1 = torch.empty((), device="cuda")
        keep.append((x, x2, y, thr, edges, out, l1))
        img = lambda n: n * S * S * Cp * 4
        runs["ens_" + shape] = lambda x=x, y=y, M=M, C=C, out=out: ops.ensemble_stats(x, y, M, C, QS, out=out)
        runs["l1_" + shape] = lambda x=x, x2=x2, rows=rows, S=S, C=C, Cp=Cp: _lib.call("acg_l1_fwd", Pt(x), Pt(x2), rows * S * S, C, Cp, Pt(l1),
                                                                                       Pt(rws), rnb, st)
        nbytes["l1_" + shape] = 2 * img(rows)
        for name, (T, E) in variants.items():
            state = ops.cell_state(C, S, S, T, E, "cuda")
            passes = 1 + (T > 0) + (E > 0)                             # launches that each read the members
            nbytes["cell_%s_%s" % (name, shape)] = passes * img(rows) + passes * img(Ny)
            key = "cell_%s_%s" % (name, shape)
            runs[key] = lambda x=x, y=y, C=C, M=M, state=state, T=T, E=E, thr=thr, edges=edges: ops.cell_stats(
                x, y, C, "nhwc", "nhwc", state, thresholds=thr[:, :T] if T else None, edges=edges if E else None, x_per_y=M)
            runs[key]()
            paths[key] = _lib.query("acg_last_kernel").decode()
            if E and not (bool((state["hist_x"].sum(1) == rows).all()) and bool((state["hist_y"].sum(1) == Ny).all())):
                raise SystemExit("the histogram columns of %s do not sum to the rows" % key)

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
    res = dict(tool="cell_stats_bench", reps=a.reps, inner=a.inner, shapes={k: list(v) for k, v in shapes.items()},
               variants={k: list(v) for k, v in variants.items()}, paths=paths)
    for k in runs:
        res[k + "_us"] = [round(v, 1) for v in us[k]]
    for shape in shapes:
        per_byte = med["l1_" + shape] / nbytes["l1_" + shape]
        res["l1_GBps_" + shape] = round(nbytes["l1_" + shape] / med["l1_" + shape] / 1e3, 1)
        for name in variants:
            k = "cell_%s_%s" % (name, shape)
            res[k + "_over_ens"] = round(med[k] / med["ens_" + shape], 2)
            res[k + "_over_floor"] = round(med[k] / nbytes[k] / per_byte, 2)         # per byte its launches read, against l1's
            res[k + "_over_one_read"] = round(med[k] / ((nbytes["l1_" + shape] / 2) * per_byte), 2)   # against the members read once
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
