"""float64 reference of the averaged weights (acg_ema_multi): e += (1 - d_t) (p - e), d_t = min(decay, (1 + t) / (10 + t)), t the
1-based number of the optimiser step just taken.  The schedule is formed in float64 from the float32 `decay` the kernel
receives."""
import numpy as np

ULP = 2.0 ** -24


def decay_at(decay, t):
    """d_t in float64; `decay` is rounded to float32 first, as the C ABI passes it"""
    t = int(t)
    assert t >= 1
    return min(float(np.float32(decay)), (1.0 + t) / (10.0 + t))


def crossing(decay):
    """the first step from which d_t == decay"""
    t = 1
    while (1.0 + t) / (10.0 + t) < float(np.float32(decay)):
        t += 1
    return t


def ema_step(e, p, decay, t):
    """one update in float64 -> the new average (inputs untouched)"""
    e, p = np.asarray(e, np.float64), np.asarray(p, np.float64)
    return e + (1.0 - decay_at(decay, t)) * (p - e)


def ema_run(ps, decay, steps, e0=None):
    """the averages after each of `steps` (1-based step numbers) applied in sequence to the parameter snapshots `ps`, starting
    from e0 (default: the first snapshot) -> list of float64 arrays"""
    e = np.asarray(ps[0] if e0 is None else e0, np.float64)
    out = []
    for p, t in zip(ps, steps):
        e = ema_step(e, p, decay, t)
        out.append(e)
    return out


def bound(K, M):
    """max |e - e64| allowed after K sequential float32 steps on values of magnitude <= M: each step has at most four float32
    roundings (d_t, p - e, the product, the sum), each of relative size 2^-24 on a quantity <= 2 M (1 - d_t) or <= M, and the
    recurrence does not amplify (d_t <= 1); 8 is twice that sum"""
    return 8.0 * K * ULP * M
