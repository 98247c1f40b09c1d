"""fp64 numpy reference of the normalisation kernels (csrc/norm.hip), the bit / byte layouts they share with the
convolutions, an fp32 restatement of the same formulas (what plain fp32 arithmetic needs against fp64: the source of every
bar that is not one of the project's own), and the seeded input generator of tests/test_hip_norm_matrix.py.

A tensor is [G groups][P pixels][C channels] (InstanceNorm: G = N, P = H*W; BatchNorm: G = 1, P = N*H*W).
    xhat = (x - mean) / sqrt(var + eps)      y = act(xhat * gamma + beta [+ res])
var is the biased (mode 0) or unbiased (mode 1) variance of the group, or given from outside (mode 2, BatchNorm eval).
gamma / beta are shared (C,) or per group (G, C).  No GPU, no torch."""
import numpy as np

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3
ACT_NAMES = {ACT_NONE: "none", ACT_RELU: "relu", ACT_LRELU: "lrelu", ACT_TANH: "tanh"}
LRELU_SLOPE = 0.2
MARGIN = 1e-4          # every pre-activation of an activation case keeps this distance from the kink (see make_case)
NORM_ROWS = 256        # pixels per chunk of the kernels' reduction passes


def act_fwd(pre, act):
    if act == ACT_RELU:
        return np.where(pre > 0, pre, 0 * pre)
    if act == ACT_LRELU:
        return np.where(pre > 0, pre, pre.dtype.type(LRELU_SLOPE) * pre)
    if act == ACT_TANH:
        return np.tanh(pre)
    return pre


def act_grad(pre, act):
    one = pre.dtype.type(1)
    if act == ACT_RELU:
        return np.where(pre > 0, one, 0 * one)
    if act == ACT_LRELU:
        return np.where(pre > 0, one, pre.dtype.type(LRELU_SLOPE))
    if act == ACT_TANH:
        return one - np.tanh(pre) ** 2
    return np.ones_like(pre)


def _gc(v, G):
    """shared (C,) or per-group (G, C) parameters -> (G, 1, C)"""
    v = np.asarray(v)
    return (np.broadcast_to(v, (G, v.shape[-1])) if v.ndim == 1 else v)[:, None, :]


def stats(x, mode):
    """mean and variance (G, C) of x (G, P, C): mode 0 biased, 1 unbiased"""
    x = np.asarray(x, np.float64)
    P = x.shape[1]
    mean = x.mean(axis=1)
    m2 = ((x - mean[:, None, :]) ** 2).sum(axis=1)
    return mean, m2 / (P - 1 if mode == 1 else P)


def forward(x, gamma, beta, res=None, act=ACT_NONE, eps=1e-5, mode=0, mean=None, var=None):
    """fp64 forward.  mode 2: mean / var (G, C) are given.  Returns dict(mean, var, rstd, xhat, pre, y)."""
    x = np.asarray(x, np.float64)
    G = x.shape[0]
    if mode != 2:
        mean, var = stats(x, mode)
    mean, var = np.asarray(mean, np.float64).reshape(G, -1), np.asarray(var, np.float64).reshape(G, -1)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (x - mean[:, None, :]) * rstd[:, None, :]
    pre = xhat * _gc(np.asarray(gamma, np.float64), G) + _gc(np.asarray(beta, np.float64), G)
    if res is not None:
        pre = pre + np.asarray(res, np.float64)
    return dict(mean=mean, var=var, rstd=rstd, xhat=xhat, pre=pre, y=act_fwd(pre, act))


def backward(dy, fw, gamma, act=ACT_NONE, mode=0, shared=True, Ptot=None, sums=None):
    """fp64 backward, written out.  gy = dy * act'(pre); S1 = sum_p gy, S2 = sum_p gy * xhat (G, C);
        dx = gamma * rstd * (gy - S1 / P - xhat * S2 / D),  D = P (mode 0) or P - 1 (mode 1);   mode 2: dx = gamma * rstd * gy
    dres = gy; dbeta = S1, dgamma = S2 (summed over the groups when the parameters are shared).
    Ptot / sums (S1, S2): the SyncBN form, the statistics and the sums cover Ptot pixels of which this tensor holds P."""
    dy = np.asarray(dy, np.float64)
    G, P, C = dy.shape
    gy = dy * act_grad(fw["pre"], act)
    S1, S2 = gy.sum(axis=1), (gy * fw["xhat"]).sum(axis=1)
    a, b = (S1, S2) if sums is None else (np.asarray(sums[0], np.float64), np.asarray(sums[1], np.float64))
    n = P if Ptot is None else Ptot
    gr = _gc(np.asarray(gamma, np.float64), G) * fw["rstd"][:, None, :]
    if mode == 2:
        dx = gr * gy
    else:
        dx = gr * (gy - a[:, None, :] / n - fw["xhat"] * b[:, None, :] / (n - 1 if mode == 1 else n))
    dgamma, dbeta = (S2.sum(axis=0), S1.sum(axis=0)) if shared else (S2, S1)
    return dict(gy=gy, S1=S1, S2=S2, dx=dx, dres=gy, dgamma=dgamma, dbeta=dbeta)


def running_update(run_mean, run_var, x, momentum):
    """BatchNorm (G == 1) momentum update: the running variance takes the unbiased estimate"""
    mean, var = stats(x, 1 if np.asarray(x).shape[1] > 1 else 0)
    return ((1 - momentum) * np.asarray(run_mean, np.float64) + momentum * mean[0],
            (1 - momentum) * np.asarray(run_var, np.float64) + momentum * var[0])


def chan_merge_partials(part_mean, part_m2, rows):
    """fp64 merge of per-chunk (mean, M2) partials (nch, ..., C) with `rows` (nch,) rows each -> mean, M2"""
    rows = np.asarray(rows, np.float64)
    pm, p2 = np.asarray(part_mean, np.float64), np.asarray(part_m2, np.float64)
    w = rows.reshape((-1,) + (1,) * (pm.ndim - 1))
    mean = (pm * w).sum(axis=0) / rows.sum()
    return mean, (p2 + w * (pm - mean) ** 2).sum(axis=0)


# ---------------------------------------------------------------- bit and byte layouts
def pack_bits(flags):
    """one bit per element in flat order: bit e % 32 of (uint32) word e / 32"""
    f = np.asarray(flags).reshape(-1).astype(np.uint64)
    assert f.size % 32 == 0
    return (f.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def unpack_bits(words, n):
    w = np.asarray(words).view(np.uint32).reshape(-1, 1)
    return ((w >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)[:n].astype(bool)


def _bf16_rne(v32):
    """fp32 -> the upper 16 bits, round to nearest even (finite inputs)"""
    u = np.asarray(v32, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def _bf16_to_f32(h16):
    return (np.asarray(h16, np.uint16).astype(np.uint32) << 16).view(np.float32)


def s16_encode(v):
    """fp32 (n,), n % 8 == 0 -> the pre-split bytes (uint8, 4 n): per 8 consecutive elements 16 bytes of bf16 hi
    (= bf16(v)) then 16 bytes of bf16 lo (= bf16(v - hi)), little endian, element order kept"""
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 8)
    hi = _bf16_rne(v)
    lo = _bf16_rne(v - _bf16_to_f32(hi))
    return np.concatenate([hi, lo], axis=1).astype("<u2").view(np.uint8).reshape(-1)


def s16_decode(raw):
    """the inverse: bytes -> fp64 values hi + lo"""
    h = np.ascontiguousarray(raw).view(np.uint8).reshape(-1).view("<u2").reshape(-1, 16)
    return (_bf16_to_f32(h[:, :8].copy()).astype(np.float64) + _bf16_to_f32(h[:, 8:].copy()).astype(np.float64)).reshape(-1)


def s16_round(v):
    """what a value becomes when it is stored pre-split (fp32 in, fp32 out: hi + lo is exact in fp32)"""
    return s16_decode(s16_encode(np.asarray(v, np.float32).reshape(-1))).astype(np.float32).reshape(np.shape(v))


# ---------------------------------------------------------------- the same formulas in plain fp32
def _chan32(na, ma, sa, nb, mb, sb):
    f = np.float32
    n = f(na + nb)
    d = mb - ma
    return n, ma + d * f(nb / n), sa + sb + d * d * f(na * nb / n)


def stats32(x, mode, rows_per_chunk=NORM_ROWS):
    """fp32 statistics in the kernels' order: per thread plain sums over the rows r0 + rl + k * rows_par of a chunk, then
    (mean, M2) merged over the threads of a chunk and over the chunks with Chan's update.  Returns mean, var, M2 (fp32)."""
    f = np.float32
    x = np.asarray(x, f)
    G, P, C = x.shape
    rows_par = max(1, 256 // (C // 4))
    N, M, S = f(0), np.zeros((G, C), f), np.zeros((G, C), f)
    for r0 in range(0, P, rows_per_chunk):
        ch = x[:, r0:min(P, r0 + rows_per_chunk)]
        n, m, s = f(0), np.zeros((G, C), f), np.zeros((G, C), f)
        for rl in range(min(rows_par, ch.shape[1])):
            t = ch[:, rl::rows_par]
            s1, s2 = np.zeros((G, C), f), np.zeros((G, C), f)
            for k in range(t.shape[1]):
                s1 = s1 + t[:, k]
                s2 = s2 + t[:, k] * t[:, k]
            cnt = f(t.shape[1])
            mean = s1 / cnt
            n, m, s = _chan32(n, m, s, cnt, mean, np.maximum(s2 - s1 * mean, f(0)))
        N, M, S = _chan32(N, M, S, n, m, s)
    return M, S / f(P - 1 if mode == 1 else P), S


def forward32(x, gamma, beta, res=None, act=ACT_NONE, eps=1e-5, mode=0, mean=None, var=None, y_s16=False):
    f = np.float32
    x = np.asarray(x, f)
    G = x.shape[0]
    if mode != 2:
        mean, var, _ = stats32(x, mode)
    mean, var = np.asarray(mean, f).reshape(G, -1), np.asarray(var, f).reshape(G, -1)
    rstd = (f(1) / np.sqrt(var + f(eps))).astype(f)
    xhat = (x - mean[:, None, :]) * rstd[:, None, :]
    pre = xhat * _gc(np.asarray(gamma, f), G) + _gc(np.asarray(beta, f), G)
    if res is not None:
        pre = pre + np.asarray(res, f)
    y = act_fwd(pre, act).astype(f)
    return dict(mean=mean, var=var, rstd=rstd, xhat=xhat, pre=pre, y=s16_round(y) if y_s16 else y)


def sums32(gy, xhat):
    """S1 = sum_p gy, S2 = sum_p gy * xhat (G, C): plain fp32 sums, chunk of 256 pixels after chunk"""
    f = np.float32
    G, P, C = gy.shape
    S1, S2 = np.zeros((G, C), f), np.zeros((G, C), f)
    for r0 in range(0, P, NORM_ROWS):
        S1 = S1 + gy[:, r0:r0 + NORM_ROWS].sum(axis=1, dtype=f)
        S2 = S2 + (gy[:, r0:r0 + NORM_ROWS] * xhat[:, r0:r0 + NORM_ROWS]).sum(axis=1, dtype=f)
    return S1, S2


def backward32(dy, fw, gamma, act=ACT_NONE, mode=0, shared=True, Ptot=None, sums=None, dx_s16=False):
    f = np.float32
    dy = np.asarray(dy, f)
    G, P, C = dy.shape
    gy = (dy * act_grad(fw["pre"], act).astype(f)).astype(f)
    S1, S2 = sums32(gy, fw["xhat"])
    a, b = (S1, S2) if sums is None else (np.asarray(sums[0], f), np.asarray(sums[1], f))
    n = P if Ptot is None else Ptot
    gr = _gc(np.asarray(gamma, f), G) * fw["rstd"][:, None, :]
    if mode == 2:
        dx = gr * gy
    else:
        dx = gr * (gy - a[:, None, :] * f(1.0 / n) - fw["xhat"] * (b[:, None, :] * f(1.0 / (n - 1 if mode == 1 else n))))
    dgamma, dbeta = (S2.sum(axis=0, dtype=f), S1.sum(axis=0, dtype=f)) if shared else (S2, S1)
    dx = dx.astype(f)
    return dict(gy=gy, S1=S1, S2=S2, dx=s16_round(dx) if dx_s16 else dx, dres=gy, dgamma=dgamma, dbeta=dbeta)


def rel(a, b):
    """max-abs error over max-abs value (tests/hip_util.rel)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


# the project's bars (tests/test_hip_ops.py): activations 2e-5, gradients and statistics 1e-4, running statistics 1e-5
PROJECT_BAR = dict(y=2e-5, dx=1e-4, dres=1e-4, dgamma=1e-4, dbeta=1e-4, mean=1e-4, rstd=1e-4, S1=1e-4, S2=1e-4,
                   run_mean=1e-5, run_var=1e-5)


def bar(name, cpu_err):
    """the project's bar, or — where plain fp32 arithmetic on the same inputs does not meet it — 4x what that needs"""
    p = PROJECT_BAR[name]
    return p if cpu_err <= p else 4.0 * cpu_err


# ---------------------------------------------------------------- inputs
def make_case(G, P, C, act=ACT_NONE, res=False, group_affine=False, mode=0, seed=0, large_mean=False, res_s16=False,
              eps=1e-5, nreal=None):
    """Seeded fp32 inputs (x, res, gamma, beta, dy[, run_mean, run_var]) of one case.

    fp32 and fp64 can disagree about the sign of a pre-activation that is nearly zero, and one flipped element changes
    S1 / S2 and through them every dx of its channel.  With an activation, every pre-activation — evaluated in fp64 on
    the inputs as rounded to fp32 (and to S16 where the residual is stored pre-split) — therefore keeps |pre| >= MARGIN:
    offending residual elements are moved, or without a residual the offending x elements are nudged until the
    (shifted) statistics leave none, or the case is reseeded.  No element is left out of any comparison.
    Unit-scale inputs; large_mean (mean 50, std 1) is for act = none only.  mode 2 adds running statistics whose first
    `nreal` channels are real (the others: mean 0, var 0, x = 0 as padded channels hold)."""
    assert not (large_mean and act != ACT_NONE)
    f = np.float32
    for attempt in range(50):
        rs = np.random.RandomState((seed * 1000003 + G * 7919 + P * 31 + C + attempt * 104729) % (2 ** 31))
        x = rs.normal(50.0 if large_mean else 0.3, 1.0, (G, P, C)).astype(f)
        shp = (G, C) if group_affine else (C,)
        gamma = (rs.normal(1.0, 0.3, shp)).astype(f)
        beta = rs.normal(0.0, 0.3, shp).astype(f)
        dy = rs.normal(0, 1, (G, P, C)).astype(f)
        r = rs.normal(0, 1, (G, P, C)).astype(f) if res else None
        if r is not None and res_s16:
            r = s16_round(r)
        kw = {}
        if mode == 2:
            nreal = C if nreal is None else nreal
            rm, rv = rs.normal(0.3, 0.2, C).astype(f), rs.uniform(0.5, 1.5, C).astype(f)
            rm[nreal:] = 0
            rv[nreal:] = 0
            x[..., nreal:] = 0
            kw = dict(mean=rm[None], var=rv[None])
        out = dict(x=x, res=r, gamma=gamma, beta=beta, dy=dy, eps=eps, mode=mode, act=act, **kw)
        if act == ACT_NONE:
            return out
        for it in range(40):
            pre = forward(x, gamma, beta, r, act, eps, mode, **kw)["pre"]
            bad = np.abs(pre) < MARGIN
            if not bad.any():
                check_margin(out)
                return out
            if r is not None:   # pre moves by exactly the step (statistics do not depend on the residual)
                step = np.where(pre >= 0, 0.0625, -0.0625).astype(f)
                r[bad] = (r[bad] + step[bad]).astype(f)
                if res_s16:
                    r[:] = s16_round(r)
            elif mode == 2 and nreal < C:
                break           # a padded channel's pre-activation is beta alone: reseed
            else:
                away = np.where(pre >= 0, 1.0, -1.0) * np.sign(np.broadcast_to(_gc(gamma, G), pre.shape))
                x[bad] += (0.03125 * away[bad]).astype(f)
        # tiny P: the nudges may not settle -> another seed
    raise AssertionError("no margin for G=%d P=%d C=%d act=%d" % (G, P, C, act))


def check_margin(case):
    """asserts the generator's promise on a finished case (fp64, on the rounded inputs); returns the smallest |pre|"""
    kw = dict(mean=case["mean"], var=case["var"]) if case["mode"] == 2 else {}
    pre = forward(case["x"], case["gamma"], case["beta"], case["res"], case["act"], case["eps"], case["mode"], **kw)["pre"]
    for k in ("x", "gamma", "beta", "dy"):
        assert case[k].dtype == np.float32
    lo = float(np.abs(pre).min())
    if case["act"] != ACT_NONE:
        assert lo >= MARGIN, lo
    return lo
