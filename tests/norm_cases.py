"""Case lists of tests/test_hip_norm_matrix.py (no GPU, no torch: tests/test_norm_ref_cpu.py imports the same lists to
check the generator's margin and to measure the fp32 bars on them).

A case is a dict: G, P, C, act, res, mask (store / read the sign bitmask), fmt (acg_norm_apply: bit 0 residual pre-split,
bit 1 y pre-split), gs ("0" shared parameters, "C" per group, "3C" per group as a column block of a (G, 3C) matrix),
mode (0 biased, 1 unbiased, 2 eval-mode BatchNorm), msrc (backward's source of the activation mask: 0 reads y, 1 recomputes
it from x, 2 reads the bitmask), dres, dx_s16, nparam (None = C), accumulate, running, nreal, large_mean, seed."""
import norm_ref as R

EW_RUN = 1024      # float4 per workgroup of the apply passes (EW_UNROLL * 256)
FIN_CH, FIN_KQ = 32, 8


def plan(G, P, C, rows_per_chunk=R.NORM_ROWS):
    """where the index arithmetic of csrc/norm.hip stands for this shape"""
    C4 = C // 4
    nch = -(-P // rows_per_chunk)
    return dict(inv=int(256 % C4 == 0), rows_par=256 // C4, idle=256 - (256 // C4) * C4, nchunks=nch,
                final="eq" if P == nch * rows_per_chunk else "chan", wgs=-(-(P * C4) // EW_RUN), f4=P * C4,
                finblocks=-(-C // FIN_CH))


def shape_id(G, P, C):
    p = plan(G, P, C)
    return "G%d_P%d_C%d-inv%d_rp%d_idle%d_nch%d_%s_f4x%d_wg%d_fin%d" % (G, P, C, p["inv"], p["rows_par"], p["idle"], p["nchunks"],
                                                                       p["final"], p["f4"], p["wgs"], p["finblocks"])


# (P, C): every edge of "where the index arithmetic turns over", each run with G = 1 and with G >= 2
_PC = [
    # one run of 1024 float4 per workgroup: P*C/4 = 1023 / 1024 / 1025 / 2047 / 2048 / 2049; C = 4: rows_par = 256;
    # NORM_ROWS: P on both sides of 4 and 8 chunks; nchunks 8 (equal) and 9 (Chan)
    (1023, 4), (1024, 4), (1025, 4), (2047, 4), (2048, 4), (2049, 4),
    # NORM_ROWS on both sides of one and two chunks, inv true (16, 32) and false (24, 48); FIN_CH: C = 16 is half a block,
    # C = 48 a block and a half; 256 x 16: exactly one workgroup run
    (255, 16), (256, 16), (257, 16), (511, 24), (512, 32), (513, 48),
    # FIN_KQ = 8 lanes over the chunks: nchunks 7 (equal), 8 (Chan, last chunk one row), 17 equal and 17 Chan
    (1792, 16), (1793, 80), (4352, 16), (4100, 144),
    # inv false with idle threads: C = 24 -> 42 rows + 4 idle, C = 1020 -> 1 row + 1 idle; 272, 144, 80
    (300, 272), (70, 1020), (257, 1020), (43, 24),
    # the unrolled trip of norm_bwd_partial (4 * rows_par rows) against its tail: rows_par = 1, 2, 4, 8 with 256 = 4 * 64
    (9, 1024), (33, 512), (40, 256), (130, 128), (64, 64),
    # tiny P
    (1, 16), (2, 16), (3, 128),
]
SHAPES = [(G, P, C) for (P, C) in _PC for G in (1, 2 if P * C > 100000 else 3)]

_DEF = dict(act=R.ACT_NONE, res=False, mask=False, fmt=0, gs="0", mode=0, msrc=0, dres=False, dx_s16=False, nparam=None,
            accumulate=0, running=False, nreal=None, large_mean=False, seed=0)


def case(G, P, C, **kw):
    c = dict(_DEF, G=G, P=P, C=C)
    c.update(kw)
    return c


def mask_ok(c):
    return (c["P"] * (c["C"] // 4)) % 8 == 0


def valid(c):
    """what the ABI accepts (include/acgan_hip.h); the rejected combinations have their own test"""
    a = c["act"]
    if c["mask"] and not (c["res"] and a in (R.ACT_RELU, R.ACT_LRELU) and mask_ok(c)):
        return False
    if c["fmt"] and not (a == R.ACT_RELU and c["C"] % 8 == 0 and (c["fmt"] == 2 or c["res"])):
        return False
    if a != R.ACT_NONE and c["msrc"] == 1 and c["res"]:
        return False   # the mask can be recomputed from x only when nothing was added before the activation
    if (c["msrc"] == 2) != bool(c["mask"]):
        return False
    if c["dx_s16"] and not (a == R.ACT_RELU and not c["dres"] and c["C"] % 8 == 0 and c["msrc"] in (1, 2)):
        return False
    if c["accumulate"] and c["gs"] != "0":
        return False
    if (c["running"] or c["mode"] == 2) and c["G"] != 1:
        return False
    if c["running"] and c["mode"] == 2:
        return False
    if c["mode"] == 1 and c["P"] < 2:
        return False
    if c["mode"] == 2 and a != R.ACT_NONE and not c["res"]:
        return False   # a padded channel's pre-activation would be beta alone (make_case)
    if c["large_mean"] and a != R.ACT_NONE:
        return False
    return True


def case_id(c):
    s = shape_id(c["G"], c["P"], c["C"]) + "-" + R.ACT_NAMES[c["act"]]
    s += ("+res" if c["res"] else "") + ("+mask" if c["mask"] else "") + ("-fmt%d" % c["fmt"] if c["fmt"] else "")
    s += "-gs%s-var%d-msrc%d" % (c["gs"], c["mode"], c["msrc"])
    s += ("+dres" if c["dres"] else "") + ("+dxs16" if c["dx_s16"] else "")
    s += ("-np%d" % c["nparam"] if c["nparam"] is not None else "") + ("+acc" if c["accumulate"] else "")
    s += ("+running" if c["running"] else "") + ("-nreal%d" % c["nreal"] if c["nreal"] is not None else "")
    s += ("-mean50" if c["large_mean"] else "") + "-s%d" % c["seed"]
    return s


def _shape_cases():
    """every shape twice: the block-output norm (ReLU + residual, bitmask where the layout allows it, dres, shared
    parameters) and a plain one (no activation, per-group parameters, unbiased variance where P >= 2)"""
    out = []
    for i, (G, P, C) in enumerate(SHAPES):
        a = case(G, P, C, act=R.ACT_RELU, res=True, dres=True, seed=i)
        if mask_ok(a):
            a.update(mask=True, msrc=2)
        out.append(a)
        out.append(case(G, P, C, gs="C", mode=1 if P >= 2 else 0, seed=i))
        out.append(case(G, P, C, act=R.ACT_LRELU, msrc=1, seed=i))
    return out


# the reduced list of the variant crosses: inv 1 / 0, bitmask layout possible (256x16, 300x24, 40x256) or not, C % 8 != 0
REDUCED = [(2, 256, 16), (3, 513, 48), (1, 300, 24), (2, 70, 1020), (1, 2049, 4), (2, 40, 256)]


def _fwd_cases():
    out = []
    for si, (G, P, C) in enumerate(REDUCED):
        sd = 100 + si
        for act in (R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU, R.ACT_TANH):
            for res in (False, True):
                out.append(case(G, P, C, act=act, res=res, msrc=0 if res or act == R.ACT_NONE else 1, seed=sd))
        for act in (R.ACT_RELU, R.ACT_LRELU):
            out.append(case(G, P, C, act=act, res=True, mask=True, msrc=2, seed=sd))
        for fmt, res, mask in ((1, True, False), (1, True, True), (2, False, False), (2, True, False), (2, True, True),
                               (3, True, False), (3, True, True)):
            out.append(case(G, P, C, act=R.ACT_RELU, res=res, mask=mask, fmt=fmt, msrc=2 if mask else (0 if res else 1), seed=sd))
        for gs in ("C", "3C"):
            out.append(case(G, P, C, act=R.ACT_RELU, gs=gs, msrc=1, seed=sd))
            out.append(case(G, P, C, act=R.ACT_LRELU, res=True, gs=gs, seed=sd))
        out.append(case(G, P, C, act=R.ACT_RELU, mode=1, msrc=1, seed=sd))
        out.append(case(1, P, C, mode=2, nreal=C - 3, seed=sd))
        out.append(case(1, P, C, act=R.ACT_RELU, res=True, mode=2, nreal=C - 1, seed=sd))
        out.append(case(1, P, C, running=True, mode=1, seed=sd))
        out.append(case(1, P, C, act=R.ACT_RELU, running=True, msrc=1, seed=sd))
        out.append(case(G, P, C, large_mean=True, seed=sd))
    return [c for c in out if valid(c)]


def _bwd_cases():
    out = []
    for si, (G, P, C) in enumerate(REDUCED):
        sd = 200 + si
        for act in (R.ACT_RELU, R.ACT_LRELU):
            for msrc in (0, 1, 2):
                for dres in (False, True):
                    res = msrc != 1
                    out.append(case(G, P, C, act=act, res=res, mask=msrc == 2, msrc=msrc, dres=dres, seed=sd))
        for dres in (False, True):
            out.append(case(G, P, C, dres=dres, res=dres, seed=sd))
        for msrc in (1, 2):
            out.append(case(G, P, C, act=R.ACT_RELU, res=msrc == 2, mask=msrc == 2, msrc=msrc, dx_s16=True, seed=sd))
            out.append(case(G, P, C, act=R.ACT_RELU, res=msrc == 2, mask=msrc == 2, msrc=msrc, dx_s16=True, gs="C", seed=sd))
        for mode in (0, 1, 2):
            out.append(case(1 if mode == 2 else G, P, C, act=R.ACT_RELU, res=True, mode=mode, dres=True, seed=sd))
            out.append(case(1 if mode == 2 else G, P, C, mode=mode, seed=sd))
        for npar in (C - 3, 1):
            for acc in (0, 1):
                out.append(case(G, P, C, act=R.ACT_RELU, msrc=1, nparam=npar, accumulate=acc, seed=sd))
        out.append(case(G, P, C, act=R.ACT_LRELU, res=True, gs="C", dres=True, seed=sd))
        out.append(case(G, P, C, act=R.ACT_RELU, gs="3C", msrc=1, seed=sd))
    return [c for c in out if valid(c)]


def _unique(cases, seen):
    out = []
    for c in cases:
        if case_id(c) not in seen:
            seen.add(case_id(c))
            out.append(c)
    return out


_seen = set()
SHAPE_CASES = _unique([c for c in _shape_cases() if valid(c)], _seen)
FWD_CASES = _unique(_fwd_cases(), _seen)
BWD_CASES = _unique(_bwd_cases(), _seen)
# acg_norm_stats_from_partials: (G, P, C, rows_per_chunk) — P a multiple of it and not, a short last chunk, 1 / 7 / 8 / 9 / 17
# chunks over the 8 lanes
PARTIAL_STATS = [(G, P, C, rpc) for G in (1, 3) for (P, C, rpc) in
                 [(128, 16, 128), (896, 48, 128), (1024, 16, 128), (1025, 24, 128), (2176, 32, 128), (2100, 80, 128),
                  (96, 16, 96), (768, 48, 96), (800, 1020, 96), (1633, 64, 96), (97, 4, 96)]]
# acg_norm_bwd_partials: (G, P, C, nchunks of the supplied partials != ceil(P / 256)), without and with an activation
PARTIAL_BWD = [(1, 256, 16, 2), (3, 513, 48, 5), (2, 300, 24, 9), (2, 1024, 64, 8), (1, 1793, 80, 17), (2, 70, 1020, 3)]
assert all(nch != -(-P // R.NORM_ROWS) for _, P, _, nch in PARTIAL_BWD)
PARTIAL_BWD_CASES = [(nch, case(G, P, C, act=act, msrc=1 if act else 0, seed=300))
                     for (G, P, C, nch) in PARTIAL_BWD for act in (R.ACT_NONE, R.ACT_RELU)]
# SyncBN: this rank holds P of Ptot = 2 P pixels; the case is the whole batch (1, 2 P, C)
SYNCBN = [(256, 16), (513, 48), (300, 24), (1025, 4), (70, 1020)]
SYNCBN_CASES = [case(1, 2 * P, C, act=act, res=act != R.ACT_NONE, mode=unbiased, dres=True, seed=400)
                for act in (R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU) for unbiased in (0, 1) for (P, C) in SYNCBN]


def inputs(c):
    return R.make_case(c["G"], c["P"], c["C"], act=c["act"], res=c["res"], group_affine=c["gs"] != "0", mode=c["mode"],
                       seed=c["seed"], large_mean=c["large_mean"], res_s16=bool(c["fmt"] & 1), nreal=c["nreal"])


def references_full(c, d):
    """fp64 reference (forward, backward), the fp32 restatement of both on the same inputs, its error and the bar per output"""
    kw = dict(mean=d["mean"], var=d["var"]) if c["mode"] == 2 else {}
    shared = c["gs"] == "0"
    f64 = R.forward(d["x"], d["gamma"], d["beta"], d["res"], c["act"], d["eps"], c["mode"], **kw)
    f32 = R.forward32(d["x"], d["gamma"], d["beta"], d["res"], c["act"], d["eps"], c["mode"], y_s16=bool(c["fmt"] & 2), **kw)
    cpu = {k: R.rel(f32[k], f64[k]) for k in ("y", "mean", "rstd")}
    b64 = b32 = None
    if c["act"] != R.ACT_TANH:
        b64 = R.backward(d["dy"], f64, d["gamma"], c["act"], c["mode"], shared)
        b32 = R.backward32(d["dy"], f32, d["gamma"], c["act"], c["mode"], shared, dx_s16=c["dx_s16"])
        cpu.update({k: R.rel(b32[k], b64[k]) for k in ("dx", "dres", "dgamma", "dbeta", "S1", "S2")})
    if c["running"]:
        rm0, rv0 = running_init(c["C"])
        r64 = R.running_update(rm0, rv0, d["x"], 0.1)
        m32, _, s32 = R.stats32(d["x"], 1)
        P = c["P"]
        r32 = (0.9 * rm0 + 0.1 * m32[0], 0.9 * rv0 + 0.1 * s32[0] / max(P - 1, 1))
        f64["run_mean"], f64["run_var"] = r64
        cpu["run_mean"], cpu["run_var"] = R.rel(r32[0], r64[0]), R.rel(r32[1], r64[1])
    return f64, b64, f32, b32, cpu, {k: R.bar(k, v) for k, v in cpu.items()}


def references(c, d):
    f64, b64, _, _, cpu, bars = references_full(c, d)
    return f64, b64, cpu, bars


def syncbn_references(c, d):
    """a SYNCBN case: references of the whole batch, and per rank (half of the pixels) the fp64 sums (2, C) = (S1, S2) that
    acg_norm_bwd_sums must return.  cpu / bars "S1", "S2" are those of the halves: what plain fp32 sums need (the per-rank
    sums are that rank's dbeta / dgamma: the project's 1e-4)."""
    import numpy as np
    f64, b64, f32, b32, cpu, bars = references_full(c, d)
    P = c["P"] // 2
    halves, e1, e2 = [], 0.0, 0.0
    for h in (slice(0, P), slice(P, 2 * P)):
        ref = np.stack([b64["gy"][0, h].sum(axis=0), (b64["gy"][0, h] * f64["xhat"][0, h]).sum(axis=0)])
        s1, s2 = R.sums32(b32["gy"][:, h], f32["xhat"][:, h])
        e1, e2 = max(e1, R.rel(s1[0], ref[0])), max(e2, R.rel(s2[0], ref[1]))
        halves.append((h, ref))
    cpu["S1"], cpu["S2"] = e1, e2
    bars["S1"], bars["S2"] = R.bar("S1", e1), R.bar("S2", e2)
    return f64, b64, halves, cpu, bars


def running_init(C):
    import numpy as np
    return (np.linspace(-0.5, 0.5, C).astype(np.float32), np.linspace(0.5, 2.0, C).astype(np.float32))
