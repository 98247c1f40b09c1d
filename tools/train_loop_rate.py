#!/usr/bin/env python3
"""Images/s of the TRAINING LOOP (dtgan_amd.train.Trainer.train_epoch on --synthetic data), not of bench.py's timed step:
per size, one child process per procedure — eager, --step_graph, --step_graph --defer_scalars — each under its own
`timeout -k 10`; the first child that fails ends the run.  A child trains one epoch untimed (the eager warm-up steps and the
capture), then times the next epoch from a synchronised device to a synchronised device: the steady-state steps.  Logging
and PNG dumps are off (print / display frequencies beyond the epoch), as in a long run between two log lines.
    python tools/train_loop_rate.py [--sizes 64,256] [--limit 900]
Sizes: 64 -> 64x64x3, batch 4 (launch-bound); 256 -> configs[2]: 256x256x3, batch 32.  9 residual blocks, bf16x3."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {64: dict(batch=4, n=800), 256: dict(batch=32, n=320)}
MODES = [("eager", []), ("step_graph", ["--step_graph"]), ("step_graph+defer_scalars", ["--step_graph", "--defer_scalars"])]


def child(a):
    sys.path.insert(0, ROOT)
    import torch

    import dtgan_amd  # noqa: F401
    from dtgan_amd.train import Trainer
    c = SIZES[a.size]
    with tempfile.TemporaryDirectory() as d:
        argv = ["--name", "rate", "--checkpoints_dir", d, "--synthetic", str(c["n"]), "--grid_size", str(a.size),
                "--batchSize", str(c["batch"]), "--n_blocks", "9", "--print_freq", "1000000000",
                "--display_freq", "1000000000", "--seed", "1"] + a.flags
        tr = Trainer(argv)
        tr.tick = time.time()
        tr.train_epoch(1)                                  # warm-up: lazily built state, the eager steps, the capture
        torch.cuda.synchronize()
        steps0 = tr.total_steps
        t0 = time.perf_counter()
        tr.train_epoch(2)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    images = tr.total_steps - steps0
    print(json.dumps(dict(size=a.size, batch=c["batch"], mode=a.mode, steps=images // c["batch"], seconds=round(dt, 4),
                          ms_per_step=round(1e3 * dt * c["batch"] / images, 3), images_per_s=round(images / dt, 2))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256")
    ap.add_argument("--limit", type=int, default=900, help="seconds per child process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--size", type=int, help=argparse.SUPPRESS)
    ap.add_argument("--mode", help=argparse.SUPPRESS)
    a, flags = ap.parse_known_args()
    if a.child:
        a.flags = flags
        return child(a)
    rows = []
    for size in (int(s) for s in a.sizes.split(",")):
        for mode, mflags in MODES:
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--size", str(size),
                   "--mode", mode] + mflags
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.stderr.write("\n%s at %d: exit status %d; stopping here\n" % (mode, size, r.returncode))
                return r.returncode
            rows.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
            print(json.dumps(rows[-1]), flush=True)
    print("\n%-6s %-26s %7s %12s %10s" % ("size", "procedure", "steps", "ms/step", "images/s"))
    for r in rows:
        print("%-6s %-26s %7d %12.2f %10.1f" % ("%dx%d" % (r["size"], r["batch"]), r["mode"], r["steps"], r["ms_per_step"],
                                               r["images_per_s"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
