"""NumPy reference of DiscriminatorLatent's dense chain (networks.py:396-433), written from the definition of its layers and
not from csrc/latent_mlp.hip: three stages Linear -> BatchNorm1d in train mode -> LeakyReLU(0.2), then a Linear(H -> 1) head
with an optional sigmoid.  fp64 by default; `dtype=np.float32` restates the same arithmetic in fp32 (the conditioning guard
of tests/test_latent_mlp_ref_cpu.py).

Parameters come as the 14 arrays of ops.LatentMLPFn, in its order: w[0..3] ([out][in], the head [1][H]), b[0..3], gamma[0..2],
beta[0..2]; buffers as running_mean[0..2] + running_var[0..2].

BatchNorm1d (train): mean and the BIASED variance of the batch normalise; the running buffers move by `momentum` towards the
mean and the UNBIASED variance.  torch refuses a batch of one; this reference takes the library's convention there (include/
acgan_hip.h): the biased variance is 0, and the running variance is updated with 0."""
import zlib

import numpy as np

SLOPE = 0.2
NPARAM = 14


def lrelu(v):
    return np.where(v > 0, v, SLOPE * v)


def batch_stats(a, eps):
    """(mean, rstd) over the batch axis, rstd from the biased variance"""
    mean = a.mean(axis=0)
    var = ((a - mean) ** 2).mean(axis=0)
    return mean, 1.0 / np.sqrt(var + a.dtype.type(eps))


def activate(a, mean, rstd, gamma, beta):
    """LeakyReLU of the normalised, scaled and shifted pre-norm activation"""
    return lrelu((a - mean) * rstd * gamma + beta)


def stage(x, w, b, gamma, beta, eps):
    """one Linear / BatchNorm1d(train) / LeakyReLU stage: x [N][K], w [H][K] -> (a, mean, rstd, h): the pre-norm activation, the
    batch statistics and the stage's output"""
    a = x @ w.T + b
    mean, rstd = batch_stats(a, eps)
    return a, mean, rstd, activate(a, mean, rstd, gamma, beta)


def head(h, w, b, sigmoid):
    y = h @ w.reshape(-1) + b.reshape(-1)[0]
    return 1.0 / (1.0 + np.exp(-y)) if sigmoid else y


def running_update(run_mean, run_var, a, momentum):
    N = a.shape[0]
    mean = a.mean(axis=0)
    unbiased = ((a - mean) ** 2).sum(axis=0) / (N - 1) if N > 1 else np.zeros_like(mean)
    m = a.dtype.type(momentum)
    return (1 - m) * run_mean + m * mean, (1 - m) * run_var + m * unbiased


class Result(object):
    """a [3][N][H]; stats [3][2][H] (mean, rstd); out [N]; dz [N][I]; grads: the 14 parameter gradients; run_mean / run_var: the
    new running buffers, [3][H] each"""
    pass


def step(z, params, buffers, dout, eps, momentum, sigmoid, dtype=np.float64):
    """forward and backward of one training-mode call.  z [N][I], dout [N] (the gradient of the output column)."""
    z = np.asarray(z, dtype)
    dout = np.asarray(dout, dtype).reshape(-1)
    P = [np.asarray(p, dtype) for p in params]
    B = [np.asarray(b, dtype) for b in buffers]
    w, b, gamma, beta = P[0:4], P[4:8], P[8:11], P[11:14]
    N = z.shape[0]
    r = Result()
    hs, a_s, means, rstds = [z], [], [], []
    r.run_mean, r.run_var = [], []
    for l in range(3):
        a, mean, rstd, h = stage(hs[-1], w[l], b[l], gamma[l], beta[l], eps)
        a_s.append(a), means.append(mean), rstds.append(rstd), hs.append(h)
        rm, rv = running_update(B[l], B[3 + l], a, momentum)
        r.run_mean.append(rm), r.run_var.append(rv)
    r.a = np.stack(a_s)
    r.stats = np.stack([np.stack([m, s]) for m, s in zip(means, rstds)])
    r.run_mean, r.run_var = np.stack(r.run_mean), np.stack(r.run_var)
    r.out = head(hs[3], w[3], b[3], sigmoid)

    # backward, the chain rule layer by layer
    d = dout * r.out * (1 - r.out) if sigmoid else dout          # gradient of the head's pre-activation
    dw, db, dgamma, dbeta = [None] * 4, [None] * 4, [None] * 3, [None] * 3
    dw[3] = (d @ hs[3]).reshape(1, -1)
    db[3] = d.sum().reshape(1)
    g = np.outer(d, w[3].reshape(-1))                            # gradient of h3
    for l in (2, 1, 0):
        xh = (a_s[l] - means[l]) * rstds[l]
        pre = xh * gamma[l] + beta[l]
        dpre = g * np.where(pre > 0, 1.0, SLOPE).astype(dtype)
        dbeta[l] = dpre.sum(axis=0)
        dgamma[l] = (dpre * xh).sum(axis=0)
        dxh = dpre * gamma[l]
        # batch normalisation with the biased variance: xh = (a - mean(a)) * rstd(a)
        da = rstds[l] * (dxh - dxh.mean(axis=0) - xh * (dxh * xh).mean(axis=0))
        dw[l] = da.T @ hs[l]
        db[l] = da.sum(axis=0)
        g = da @ w[l]
    r.dz = g
    r.grads = dw + db + dgamma + dbeta
    assert len(r.grads) == NPARAM and all(x.shape == p.shape for x, p in zip(r.grads, P)) and N == r.out.shape[0]
    return r


# ================================================================ the kernel tests' cases, launch plan and bars
EPS, MOMENTUM = 1e-5, 0.1
BAR = 2e-5                      # activations, statistics, running buffers, output, dz; gradients on the scale of gmax
BAR_OWN, OWN_FROM = 1e-4, 0.05  # gradient tensors whose own maximum is at least OWN_FROM * gmax, on their own scale
BAR_ACC = 1e-6                  # accumulate = 1 against g0 + (accumulate = 0), on the scale of gmax
ACT_NONE, ACT_SIGMOID = 0, 4

J_INSTANCES = (1, 2, 4, 8, 16)
MLP_JMAX = 16
LDS_BUDGET = 160 * 1024 - 1024
LDS_DEFAULT = 64 * 1024


# ---------------------------------------------------------------- the launch plan, restated
def lds_bytes(N, H):
    """(forward, backward) dynamic LDS: [N][H + 1] activations, [H][H + 1] weights, two fold buffers of 256; the backward
    adds the linear layer's input and da, [N][H + 1] each"""
    fwd = N * (H + 1) + H * (H + 1) + 2 * 256
    return 4 * fwd, 4 * (fwd + 2 * N * (H + 1))


def supported(N, I, H):
    return (N > 0 and I > 0 and 16 <= H <= 256 and I <= H and 256 % H == 0 and N * H <= 256 * MLP_JMAX
            and lds_bytes(N, H)[1] <= LDS_BUDGET)


def plan(N, I, H):
    need = -(-N * H // 256)
    J = min(j for j in J_INSTANCES if j >= need)
    nstep = 256 // H
    fwd, bwd = lds_bytes(N, H)
    nk_first, nk = -(-I // nstep), H // nstep                  # columns per thread of the weight-gradient block, K = I and K = H
    return dict(J=J, need=need, full=(N * H == 256 * J), nstep=nstep, idle=max(0, 256 - N * H),
                kb_first=-(-nk_first // MLP_JMAX), kb=-(-nk // MLP_JMAX), lds_fwd=fwd, lds_bwd=bwd, head_uneven=(N % 4 != 0))


# ---------------------------------------------------------------- cases
# (N, I, H): the smallest shapes that reach each branch; (64,16,16) and (32,8,64) fill the J = 4 and J = 8 tiles completely
_SHAPES = [(4, 4, 16), (16, 16, 16), (17, 5, 16), (37, 16, 16), (70, 16, 16), (129, 1, 16), (256, 16, 16), (64, 16, 16),
           (5, 8, 32), (24, 32, 32), (72, 3, 32),
           (4, 16, 64), (6, 64, 64), (12, 16, 64), (20, 1, 64), (37, 16, 64), (32, 8, 64), (64, 16, 64),
           (4, 16, 128), (7, 128, 128), (19, 100, 128), (32, 16, 128)]
CASES = [(N, I, H, i % 3 == 1) for i, (N, I, H) in enumerate(_SHAPES)]           # value-checked; a third with the sigmoid head
STAGE_ONLY = [(N, 16, H, H == 64) for H in (16, 64, 128) for N in (1, 2, 3)]     # teacher-forced checks only
CONTRACT = [c for c in CASES if c[:3] in ((17, 5, 16), (72, 3, 32), (64, 16, 64), (7, 128, 128))]
EXTRA = (0, 3)                                                                   # ldz - I
MODULE_CASES = [(32, 16, 64), (7, 4, 16), (12, 16, 128)]


def module_key(N, nlatent, ndf):
    return "module %d %d %d" % (N, nlatent, ndf)


def cid(c):
    N, I, H, sig = c
    p = plan(N, I, H)
    return "n%di%dh%d-J%d%s-ns%d-kb%d-lds%df%db%s" % (N, I, H, p["J"], "f" if p["full"] else "m", p["nstep"], p["kb"],
                                                       -(-p["lds_fwd"] // 1024), -(-p["lds_bwd"] // 1024), "-sig" if sig else "")


class Draw(object):
    pass


def draw(c, key=None):
    """weights ~ N(0, 1 / sqrt(fan_in)), gamma ~ N(1, 0.3), beta, biases ~ N(0, 0.3), z ~ N(0, 1.5): float32 values"""
    N, I, H, sig = c
    rs = np.random.RandomState(zlib.crc32((key or cid(c)).encode()))
    f = np.float32
    d = Draw()
    d.z = rs.normal(0, 1.5, (N, I)).astype(f)
    fan = [I, H, H, H]
    w = [rs.normal(0, fan[l] ** -0.5, ((H if l < 3 else 1), fan[l])).astype(f) for l in range(4)]
    b = [rs.normal(0, 0.3, (H if l < 3 else 1,)).astype(f) for l in range(4)]
    gamma = [rs.normal(1, 0.3, H).astype(f) for _ in range(3)]
    beta = [rs.normal(0, 0.3, H).astype(f) for _ in range(3)]
    d.params = w + b + gamma + beta
    d.buffers = [rs.normal(0, 0.5, H).astype(f) for _ in range(3)] + [rs.uniform(0.5, 1.5, H).astype(f) for _ in range(3)]
    d.dout = rs.normal(0, 1, N).astype(f)
    return d


_REF = {}


def reference(c):
    """the fp64 result of a case, computed once"""
    k = cid(c)
    if k not in _REF:
        d = draw(c)
        _REF[k] = step(d.z, d.params, d.buffers, d.dout, EPS, MOMENTUM, c[3])
    return _REF[k]


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-300))


def value_errors(k, r):
    """{quantity: error on the scale its bar is stated in} of a result k (attributes as latent_mlp_ref.Result, any float
    type) against the fp64 result r.  'grad': the worst gradient tensor on the scale of gmax; 'grad_own': the worst of the
    tensors whose own maximum is at least OWN_FROM * gmax, on their own scale."""
    e = {}
    e["a_save"] = max(relerr(k.a[l], r.a[l]) for l in range(3))
    e["mean"] = max(relerr(k.stats[l][0], r.stats[l][0]) for l in range(3))
    e["rstd"] = max(relerr(k.stats[l][1], r.stats[l][1]) for l in range(3))
    e["run_mean"] = max(relerr(k.run_mean[l], r.run_mean[l]) for l in range(3))
    e["run_var"] = max(relerr(k.run_var[l], r.run_var[l]) for l in range(3))
    e["out"] = relerr(k.out, r.out)
    e["dz"] = relerr(k.dz, r.dz)
    gmax = max(float(np.max(np.abs(g))) for g in r.grads)
    e["grad"] = max(float(np.max(np.abs(np.asarray(a, np.float64) - b))) for a, b in zip(k.grads, r.grads)) / gmax
    e["grad_own"] = max(relerr(a, b) for a, b in zip(k.grads, r.grads) if np.max(np.abs(b)) >= OWN_FROM * gmax)
    return e


BARS = dict(a_save=BAR, mean=BAR, rstd=BAR, run_mean=BAR, run_var=BAR, out=BAR, dz=BAR, grad=BAR, grad_own=BAR_OWN)


def assert_values(k, r, what):
    e = value_errors(k, r)
    print("MEASURED %s %s" % (what, " ".join("%s=%.3g" % kv for kv in sorted(e.items()))))
    for q, v in e.items():
        assert v < BARS[q] or (q == "grad" and v <= BARS[q]), (what, q, v, BARS[q])
