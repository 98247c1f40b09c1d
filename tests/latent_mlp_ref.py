"""NumPy reference of DiscriminatorLatent's dense chain (networks.py:396-433), written from the definition of its layers and
not from csrc/latent_mlp.hip: three stages Linear -> BatchNorm1d in train mode -> LeakyReLU(0.2), then a Linear(H -> 1) head
with an optional sigmoid.  fp64 by default; `dtype=np.float32` restates the same arithmetic in fp32 (the conditioning guard
of tests/test_latent_mlp_ref_cpu.py).

Parameters come as the 14 arrays of ops.LatentMLPFn, in its order: w[0..3] ([out][in], the head [1][H]), b[0..3], gamma[0..2],
beta[0..2]; buffers as running_mean[0..2] + running_var[0..2].

BatchNorm1d (train): mean and the BIASED variance of the batch normalise; the running buffers move by `momentum` towards the
mean and the UNBIASED variance.  torch refuses a batch of one; this reference takes the library's convention there (include/
acgan_hip.h): the biased variance is 0, and the running variance is updated with 0."""
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
