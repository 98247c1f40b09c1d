#!/usr/bin/env python3
"""rocprofv3 kernel_trace.csv of a training run with --ema_decay -> the time of every ema_multi_kernel launch beside the
adam_multi_kernel launch in front of it (FusedAdam.clip_and_step issues the two on the same flat buffers), per launch shape,
with the bytes each moves (12 B per element for the average: p and e read, e written; 32 B for Adam: p, g, m, v read and
written) and the rate that implies.
    python tools/ema_kernel_cost.py <kernel_trace.csv> <out.md> <elements of each launch shape, in the order of their blocks>
e.g. for AugmentedCycleGAN: the elements of G_B_A, then of G_A_B + E_B (printed by tools/ema_kernel_cost.py --elements)."""
import collections
import csv
import os
import statistics
import sys


def elements():
    """the padded parameter counts of the averaged launches at configs[2] geometry (no GPU needed: shapes only)"""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import dtgan_amd  # noqa: F401
    from dtgan_amd import networks as N
    count = lambda net: sum((p.numel() + 3) // 4 * 4 for p in net.parameters())
    g_ab, g_ba, e_b = N.define_stochastic_G(16, 3, 3, 32, n_blocks=9), N.define_G(3, 3, 32, n_blocks=9), N.define_E(16, 6, 32, "batch")
    print("G_B_A %d; G_A_B %d + E_B %d = %d" % (count(g_ba), count(g_ab), count(e_b), count(g_ab) + count(e_b)))


def main():
    if sys.argv[1] == "--elements":
        return elements()
    src, out, counts = sys.argv[1], sys.argv[2], [int(v) for v in sys.argv[3:]]
    rows = sorted(csv.DictReader(open(src)), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    grid = lambda r: int(r["Grid_Size_X"])
    pairs, last_adam = collections.defaultdict(list), None
    for r in rows:
        if "adam_multi_kernel" in r["Kernel_Name"]:
            last_adam = r
        elif "ema_multi_kernel" in r["Kernel_Name"]:
            assert last_adam is not None, "an ema_multi_kernel launch without an adam_multi_kernel launch in front of it"
            pairs[grid(r)].append((us(r), us(last_adam)))
            last_adam = None
    assert pairs, "no ema_multi_kernel launch in %s" % src
    with open(out, "w") as f:
        f.write("# ema_multi_kernel beside the adam_multi_kernel launch on the same groups, from %s (tools/ema_kernel_cost.py)\n\n" % src)
        f.write("| ema grid (threads) | launches | elements | ema median us | ema min us | ema GB/s (12 B/el) | adam median us | adam min us | "
                "adam GB/s (32 B/el) | ema / adam |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for i, g in enumerate(sorted(pairs)):
            e, a = [p[0] for p in pairs[g]], [p[1] for p in pairs[g]]
            me, ma = statistics.median(e), statistics.median(a)
            n = counts[i] if i < len(counts) else None
            rate = lambda bytes_per, t: ("%.0f" % (n * bytes_per / t / 1e3)) if n else "-"
            f.write("| %d | %d | %s | %.1f | %.1f | %s | %.1f | %.1f | %s | %.2f |\n"
                    % (g, len(e), n if n else "-", me, min(e), rate(12, me), ma, min(a), rate(32, ma), me / ma))
    print(open(out).read())


if __name__ == "__main__":
    main()
