"""csrc/latent_mlp.hip (DiscriminatorLatent as one 256-thread workgroup per direction) through the C ABI against the fp64
reference of tests/latent_mlp_ref.py, at the (N, I, H) where its launch plan turns over.  A test id spells the plan:
    n17i5h16-J2m-ns16-kb1-lds3f5b[-sig]
J: the register-tile template instance (1, 2, 4, 8, 16 >= ceil(N H / 256)), "f" when all 256 J slots hold an element, "m" when
some are masked by n < N; ns = 256 / H: samples per trip of the thread map; kb: passes of the weight-gradient block's loop over
MLP_JMAX columns (4 at H = 128); lds: KB of dynamic LDS forward / backward (above 64 the launch raises the function's limit
first); sig: the sigmoid head.  plan() restates that arithmetic; tests/test_latent_mlp_ref_cpu.py asserts which branches the
case list reaches, checks the reference against torch in fp64, and guards the conditioning of every value-checked case.

Inputs are seeded by zlib.crc32 of the id.  Every case runs with ldz = I and ldz = I + 3 (the extra columns of z hold NaN and
1e30; those of dz must stay untouched).  Outputs start as NaN and every buffer ends in guard words (tests/guard_util.py).

Bars, none of them fitted to this kernel: 2e-5 of the largest value for activations, statistics, running buffers, output and
dz (the bar for y of test_hip_ops / test_hip_fastpath_fuzz); every parameter gradient within 2e-5 of the largest gradient
entry of all 14 tensors (the Linear biases in front of a BatchNorm have analytically zero gradients, tests/test_hip_bce.py),
and those whose own maximum reaches 0.05 of it within 1e-4 of their own maximum (the project's dw / db bar).  End-to-end values
are compared from N = 4 (BatchNorm over two or three samples is ill-conditioned in fp32 whatever computes it); the
teacher-forced stage checks feed each stage the kernel's own saved activations and statistics and hold at every N.

Measured on the MI355X, worst case over the case list (each on the scale of its bar): a_save 5.8e-7, mean 3.3e-7, rstd 3.0e-6,
running mean 1.2e-7, running variance 1.7e-7, output 1.0e-6, dz 2.9e-6, gradients 1.8e-6 of gmax and 8.5e-6 of their own
maximum (bar 1e-4); the worst are (4,16,128) and (20,1,64).  Teacher-forced stages 4.8e-7.  Module level: output 6.2e-7, input
gradient 4.4e-7, gradients 5.9e-7 of gmax, running buffers 1.8e-7.  The float32 restatement of the reference on the CPU:
output 8.3e-7, dz 1.3e-6, gradients 3.0e-6 of gmax and 2.5e-5 of their own maximum.  A batch of one: the fused kernel and the
layer chain both return, with the same values.

134 tests, 3.6 s on one MI355X (one process).
"""
import ctypes
import zlib

import numpy as np
import pytest

import latent_mlp_ref as R
from guard_util import Buf, rejected
from latent_mlp_ref import (ACT_NONE, ACT_SIGMOID, BAR, BAR_ACC, CASES, CONTRACT, EPS, EXTRA, MODULE_CASES, MOMENTUM, STAGE_ONLY,
                            assert_values, cid, draw, module_key, reference, relerr, supported)

gpu = pytest.mark.gpu


# ---------------------------------------------------------------- the C ABI
@pytest.fixture(autouse=True)
def _fresh_buffers():
    Buf.live = []
    yield
    Buf.live = []


def _env():
    from dtgan_amd import _lib, ops
    return _lib, _lib.load(), ops._stream()


def _addr(b):
    return None if b is None else b.t.data_ptr()


def _garbage(shape):
    a = np.full(shape, 1e30, np.float32)
    a.reshape(-1)[::2] = np.nan
    return a


def run(c, extra=0, accumulate=0, null=(), dz=True, run_null=(), g0=None, pass_out=True, backward=True):
    """one forward and one backward call -> latent_mlp_ref.Result-like object of float32 arrays, plus out4 [N][4], dz_full
    [N][ldz] and the running buffers as they are after the call.  null: indices (LatentMLPFn order) of gradient pointers
    passed as NULL; run_null: layers whose running-buffer pointers are NULL; g0: initial contents of the gradient buffers
    (NaN if None)."""
    _lib, lib, st = _env()
    N, I, H, sig = c
    d = draw(c)
    ldz = I + extra
    zf = _garbage((N, ldz))
    zf[:, :I] = d.z
    zb = Buf.of(zf)
    pb = [Buf.of(p) for p in d.params]
    rb = [Buf.of(b) for b in d.buffers]
    pp = _lib.LatentMlpParams()
    for l in range(4):
        pp.w[l], pp.b[l] = _addr(pb[l]), _addr(pb[4 + l])
    for l in range(3):
        pp.gamma[l], pp.beta[l] = _addr(pb[8 + l]), _addr(pb[11 + l])
        if l not in run_null:
            pp.run_mean[l], pp.run_var[l] = _addr(rb[l]), _addr(rb[3 + l])
    pp.head_act = ACT_SIGMOID if sig else ACT_NONE
    a_save, stats, out = Buf.out(3 * N * H), Buf.out(6 * H), Buf.out(4 * N)
    rc = lib.acg_latent_mlp_fwd(ctypes.byref(pp), zb.ptr, ldz, N, I, H, EPS, MOMENTUM, a_save.ptr, stats.ptr, out.ptr, st)
    assert rc == 0, lib.acg_last_error().decode()
    k = R.Result()
    k.a, k.stats, k.out4 = a_save.host((3, N, H)), stats.host((3, 2, H)), out.host((N, 4))
    k.out = k.out4[:, 0]
    k.run_mean = np.stack([rb[l].host() for l in range(3)])
    k.run_var = np.stack([rb[3 + l].host() for l in range(3)])
    if backward:
        gb = [None if i in null else (Buf.out(p.size) if g0 is None else Buf.of(g0[i])) for i, p in enumerate(d.params)]
        gg = _lib.LatentMlpGrads()
        for l in range(4):
            gg.dw[l], gg.db[l] = _addr(gb[l]), _addr(gb[4 + l])
        for l in range(3):
            gg.dgamma[l], gg.dbeta[l] = _addr(gb[8 + l]), _addr(gb[11 + l])
        do = np.full((N, 4), 1e30, np.float32)                      # only column 0 of the output gradient means anything
        do[:, 0] = d.dout
        dob = Buf.of(do)
        dzb = Buf.out(N * ldz) if dz else None
        rc = lib.acg_latent_mlp_bwd(ctypes.byref(pp), ctypes.byref(gg), zb.ptr, ldz, N, I, H, a_save.ptr, stats.ptr,
                                    out.ptr if pass_out else None, dob.ptr, dzb.ptr if dz else None, accumulate, st)
        assert rc == 0, lib.acg_last_error().decode()
        k.grads = [None if g is None else g.host(p.shape) for g, p in zip(gb, d.params)]
        k.dz_full = dzb.host((N, ldz)) if dz else None
        k.dz = k.dz_full[:, :I] if dz else None
        # the backward leaves what the forward wrote alone
        assert np.array_equal(a_save.host().view(np.uint32), k.a.reshape(-1).view(np.uint32))
    Buf.check_all()
    return k


_RUN = {}


def plain(c, extra):
    """the plain call of a case (accumulate = 0, nothing NULL), run once per (case, ldz)"""
    key = (cid(c), extra)
    if key not in _RUN:
        _RUN[key] = run(c, extra)
    return _RUN[key]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---------------------------------------------------------------- values against fp64
@gpu
@pytest.mark.parametrize("extra", EXTRA, ids=lambda e: "ldz+%d" % e)
@pytest.mark.parametrize("c", CASES, ids=cid)
def test_values_against_fp64(c, extra):
    """every forward and backward output at N >= 4"""
    N, I, H, sig = c
    k, r = plain(c, extra), reference(c)
    assert np.all(k.out4[:, 1:] == 0) and not np.any(np.signbit(k.out4[:, 1:]))
    for x in [k.a, k.stats, k.out4, k.run_mean, k.run_var, k.dz] + k.grads:
        assert np.all(np.isfinite(x))
    if extra:
        assert np.all(np.isnan(k.dz_full[:, I:]))                   # columns >= I are the caller's (ops.LatentMLPFn zero-fills)
    assert_values(k, r, "%s ldz+%d" % (cid(c), extra))


@gpu
@pytest.mark.parametrize("extra", EXTRA, ids=lambda e: "ldz+%d" % e)
@pytest.mark.parametrize("c", CASES + STAGE_ONLY, ids=cid)
def test_teacher_forced_stages(c, extra):
    """each stage on its own, fed what the kernel itself saved: well conditioned at every N, N = 1, 2 and 3 included.  Layer l's
    statistics are those of a_save[l]; a_save[l + 1] is the Linear of the LeakyReLU of a_save[l] normalised with the saved
    statistics; the output is the head of the same; the running buffers moved by the statistics of a_save[l]."""
    N, I, H, sig = c
    k, d = plain(c, extra), draw(c)
    P = [np.asarray(p, np.float64) for p in d.params]
    e = {}
    for l in range(3):
        a = np.asarray(k.a[l], np.float64)
        mean, rstd = R.batch_stats(a, EPS)
        e["mean%d" % l], e["rstd%d" % l] = relerr(k.stats[l][0], mean), relerr(k.stats[l][1], rstd)
        rm, rv = R.running_update(np.asarray(d.buffers[l], np.float64), np.asarray(d.buffers[3 + l], np.float64), a, MOMENTUM)
        e["run_mean%d" % l], e["run_var%d" % l] = relerr(k.run_mean[l], rm), relerr(k.run_var[l], rv)
        h = R.activate(a, np.asarray(k.stats[l][0], np.float64), np.asarray(k.stats[l][1], np.float64), P[8 + l], P[11 + l])
        if l < 2:
            e["a%d" % (l + 1)] = relerr(k.a[l + 1], R.stage(h, P[l + 1], P[5 + l], P[9 + l], P[12 + l], EPS)[0])
        else:
            e["out"] = relerr(k.out, R.head(h, P[3], P[7], sig))
    e["a0"] = relerr(k.a[0], R.stage(np.asarray(d.z, np.float64), P[0], P[4], P[8], P[11], EPS)[0])
    if N == 1:   # the library's definition of a batch of one: rstd = eps^-1/2, so the stage's output is lrelu(beta)
        for l in range(3):
            assert relerr(k.stats[l][1], np.full(H, EPS ** -0.5)) < BAR and same_bits(k.stats[l][0], k.a[l][0])
    print("MEASURED-STAGE %s ldz+%d worst=%.3g" % (cid(c), extra, max(e.values())))
    for q, v in e.items():
        assert v < BAR, (q, v)
    assert np.all(k.out4[:, 1:] == 0)


# ---------------------------------------------------------------- contract
@gpu
@pytest.mark.parametrize("c", CONTRACT, ids=cid)
def test_accumulate_adds_to_known_values(c):
    """accumulate = 1 over g0 gives g0 + gradient; accumulate = 0 overwrites NaN"""
    r = reference(c)
    gmax = max(float(np.max(np.abs(g))) for g in r.grads)
    rs = np.random.RandomState(zlib.crc32(("g0 " + cid(c)).encode()))
    g0 = [(rs.uniform(-1, 1, g.shape) * gmax).astype(np.float32) for g in r.grads]
    k0, k1 = plain(c, 3), run(c, 3, accumulate=1, g0=g0)
    for i in range(R.NPARAM):
        assert np.all(np.isfinite(k0.grads[i]))
        err = float(np.max(np.abs(k1.grads[i].astype(np.float64) - (g0[i].astype(np.float64) + k0.grads[i])))) / gmax
        assert err < BAR_ACC, (i, err)
    assert same_bits(k0.dz_full, k1.dz_full)


@gpu
@pytest.mark.parametrize("c", CONTRACT, ids=cid)
def test_null_outputs_change_nothing_else(c):
    """dz = NULL, then an arbitrary half of the gradient pointers NULL: what remains is bit-identical to the full call"""
    full = plain(c, 3)
    k = run(c, 3, dz=False)
    assert all(same_bits(a, b) for a, b in zip(k.grads, full.grads))
    rs = np.random.RandomState(zlib.crc32(("null " + cid(c)).encode()))
    null = set(int(i) for i in rs.permutation(R.NPARAM)[:R.NPARAM // 2])
    k = run(c, 3, null=null)
    assert same_bits(k.dz, full.dz) and np.all(np.isnan(k.dz_full[:, c[1]:]))
    for i in range(R.NPARAM):
        assert (k.grads[i] is None) == (i in null)
        if i not in null:
            assert same_bits(k.grads[i], full.grads[i]), i
    k = run(c, 3, null=set(range(R.NPARAM)) - null)
    for i in null:
        assert same_bits(k.grads[i], full.grads[i]), i


@gpu
@pytest.mark.parametrize("c", CONTRACT, ids=cid)
def test_null_running_buffers(c):
    """run_mean = run_var = NULL: the forward's outputs are bit-identical and no running buffer is written; with one layer's
    pointers NULL the other two layers' buffers move as before"""
    full, d = plain(c, 3), draw(c)
    k = run(c, 3, run_null=(0, 1, 2), backward=False)
    assert same_bits(k.a, full.a) and same_bits(k.stats, full.stats) and same_bits(k.out4, full.out4)
    for l in range(3):
        assert same_bits(k.run_mean[l], d.buffers[l]) and same_bits(k.run_var[l], d.buffers[3 + l])
    k = run(c, 3, run_null=(1,), backward=False)
    assert same_bits(k.a, full.a) and same_bits(k.stats, full.stats) and same_bits(k.out4, full.out4)
    assert same_bits(k.run_mean[1], d.buffers[1]) and same_bits(k.run_var[1], d.buffers[4])
    for l in (0, 2):
        assert same_bits(k.run_mean[l], full.run_mean[l]) and same_bits(k.run_var[l], full.run_var[l])


@gpu
@pytest.mark.parametrize("c", CONTRACT, ids=cid)
def test_two_calls_give_the_same_bits(c):
    """no atomics anywhere: a difference between two identical calls is a race"""
    a, b = plain(c, 3), run(c, 3)
    for x, y in zip([a.a, a.stats, a.out4, a.run_mean, a.run_var, a.dz_full] + a.grads,
                    [b.a, b.stats, b.out4, b.run_mean, b.run_var, b.dz_full] + b.grads):
        assert same_bits(x, y)


@gpu
@pytest.mark.parametrize("c", CONTRACT, ids=cid)
def test_the_head_and_the_forward_output(c):
    """a sigmoid head's backward needs the forward's output and is refused without it (its values with it are checked
    against the fp64 gradient of sigmoid(head) by test_values_against_fp64); a linear head never reads it"""
    _lib, lib, st = _env()
    N, I, H, sig = c
    if not sig:
        k, full = run(c, 3, pass_out=False), plain(c, 3)
        assert same_bits(k.dz, full.dz) and all(same_bits(a, b) for a, b in zip(k.grads, full.grads))
        return
    d = draw(c)
    pb = [Buf.of(p) for p in d.params]
    pp, gg = _lib.LatentMlpParams(), _lib.LatentMlpGrads()
    for l in range(4):
        pp.w[l], pp.b[l] = _addr(pb[l]), _addr(pb[4 + l])
    for l in range(3):
        pp.gamma[l], pp.beta[l] = _addr(pb[8 + l]), _addr(pb[11 + l])
    pp.head_act = ACT_SIGMOID
    zb, a_save, stats, dout, dz = Buf.of(d.z), Buf.out(3 * N * H), Buf.out(6 * H), Buf.of(np.zeros((N, 4))), Buf.out(N * I)
    msg = rejected(lib, "acg_latent_mlp_bwd", ctypes.byref(pp), ctypes.byref(gg), zb.ptr, I, N, I, H, a_save.ptr, stats.ptr, None,
                   dout.ptr, dz.ptr, 0, st)
    assert "sigmoid" in msg, msg
    pp.head_act = 3                                                   # tanh: not a head this kernel has
    out = Buf.out(4 * N)
    msg = rejected(lib, "acg_latent_mlp_fwd", ctypes.byref(pp), zb.ptr, I, N, I, H, EPS, MOMENTUM, a_save.ptr, stats.ptr, out.ptr, st)
    assert "head activation" in msg, msg
    assert np.all(np.isnan(dz.host())) and np.all(np.isnan(out.host())) and np.all(np.isnan(a_save.host()))
    Buf.check_all()


# ---------------------------------------------------------------- predicate
@gpu
def test_predicate_matches_its_restatement_and_refusals_do_not_launch():
    """acg_latent_mlp_supported over a grid, H = 256 refused for every N (its weight rows alone exceed the LDS budget), and
    every refused (N, I, H) returns the error code from both entry points with the outputs untouched"""
    _lib, lib, st = _env()
    pp, gg = _lib.LatentMlpParams(), _lib.LatentMlpGrads()
    some = Buf.of(np.zeros(64))
    for l in range(4):
        pp.w[l], pp.b[l] = _addr(some), _addr(some)
    for l in range(3):
        pp.gamma[l], pp.beta[l] = _addr(some), _addr(some)
    outs = [Buf.out(64) for _ in range(4)]
    refused = 0
    for H in (8, 16, 24, 32, 48, 64, 128, 256, 512):
        for I in sorted(set((1, 8, 16, H, H + 1))):
            for N in range(1, 301):
                want = supported(N, I, H)
                assert bool(lib.acg_latent_mlp_supported(N, I, H)) == want, (N, I, H)
                assert not (want and H == 256)
                if want:
                    continue
                refused += 1
                msg = rejected(lib, "acg_latent_mlp_fwd", ctypes.byref(pp), some.ptr, I, N, I, H, EPS, MOMENTUM, outs[0].ptr,
                               outs[1].ptr, outs[2].ptr, st)
                assert "outside the fused kernel" in msg, msg
                msg = rejected(lib, "acg_latent_mlp_bwd", ctypes.byref(pp), ctypes.byref(gg), some.ptr, I, N, I, H, outs[0].ptr,
                               outs[1].ptr, outs[2].ptr, some.ptr, outs[3].ptr, 0, st)
                assert "outside the fused kernel" in msg, msg
    assert refused > 1000
    for N, I, H in ((0, 16, 64), (-1, 16, 64), (4, 0, 64), (4, 16, 0)):
        assert not lib.acg_latent_mlp_supported(N, I, H)
    assert all(np.all(np.isnan(o.host())) for o in outs)
    Buf.check_all()


# ---------------------------------------------------------------- the module
def _build_net(c, key, flat):
    import torch
    from dtgan_amd import networks
    from dtgan_amd.model import FlatNet
    N, I, H, sig = c
    d = draw(c, key)
    net = networks.DiscriminatorLatent(I, H, use_sigmoid=sig).cuda()
    mods = list(net.model._modules.values())
    lins, bns = mods[0:10:3], mods[1:9:3]
    order = [m.weight for m in lins] + [m.bias for m in lins] + [b.weight for b in bns] + [b.bias for b in bns]
    with torch.no_grad():
        for p, v in zip(order, d.params):
            p.copy_(torch.from_numpy(v))
        for l, b in enumerate(bns):
            b.running_mean.copy_(torch.from_numpy(d.buffers[l]))
            b.running_var.copy_(torch.from_numpy(d.buffers[3 + l]))
    networks.mark_dirty(net)
    fn = FlatNet(net) if flat else None
    return net, order, bns, d, fn


@gpu
@pytest.mark.parametrize("flat", [False, True], ids=["autograd", "flatnet"])
@pytest.mark.parametrize("N,nlatent,ndf", MODULE_CASES)
def test_module_two_steps_against_fp64(N, nlatent, ndf, flat):
    """networks.DiscriminatorLatent.forward_dense on an (N, cpad(nlatent)) input, as the encoder feeds it, two steps in a row:
    output, input gradient, parameter gradients (autograd tensors, or added into a FlatNet's .grad by the kernel), running
    buffers and num_batches_tracked"""
    import torch
    from dtgan_amd import ops
    c = (N, nlatent, ndf, False)
    net, order, bns, d, fn = _build_net(c, module_key(N, nlatent, ndf), flat)
    ldz = ops.cpad(nlatent)
    zf = np.full((N, ldz), 1e30, np.float32)
    zf[:, :nlatent] = d.z
    zt = torch.from_numpy(zf).cuda().requires_grad_(True)
    do = np.zeros((N, 4), np.float32)
    do[:, 0] = d.dout
    calls, orig = [], ops._lib.call
    ops._lib.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    bufs = d.buffers
    try:
        for step in (1, 2):
            y = net.forward_dense(zt)
            y.backward(torch.from_numpy(do).cuda())
            r = R.step(d.z, d.params, bufs, d.dout, EPS, MOMENTUM, False)
            bufs = list(r.run_mean) + list(r.run_var)
            k = R.Result()
            k.a, k.stats = r.a, r.stats                              # not visible at module level
            yh = y.detach().cpu().numpy()
            assert yh.shape == (N, 4) and np.all(yh[:, 1:] == 0)
            k.out = yh[:, 0]
            zg = zt.grad.cpu().numpy()
            assert np.all(zg[:, nlatent:] == 0)
            k.dz = zg[:, :nlatent] / step
            k.grads = [p.grad.cpu().numpy() / step for p in order]
            k.run_mean = np.stack([b.running_mean.cpu().numpy() for b in bns])
            k.run_var = np.stack([b.running_var.cpu().numpy() for b in bns])
            assert_values(k, r, "module n%di%dh%d %s step%d" % (N, nlatent, ndf, "flatnet" if flat else "autograd", step))
            assert all(int(b.num_batches_tracked) == step for b in bns)
    finally:
        ops._lib.call = orig
    assert calls.count("acg_latent_mlp_fwd") == 2 and calls.count("acg_latent_mlp_bwd") == 2
    assert "acg_linear_fwd" not in calls
    assert bns[0].eps == EPS and bns[0].momentum == MOMENTUM


@gpu
def test_a_batch_of_one_is_the_same_fused_and_layer_by_layer():
    """torch refuses BatchNorm over one sample; this library defines it (rstd = eps^-1/2, running variance updated with 0).
    The fused kernel and the layer chain it replaces must agree on that: both raise, or both give the same values."""
    import torch
    from dtgan_amd import ops
    c = (1, 16, 64, False)
    res = {}
    for fused in (True, False):
        ops.LATENT_MLP = fused
        try:
            net, order, bns, d, fn = _build_net(c, "one", False)
            zt = torch.from_numpy(d.z).cuda().requires_grad_(True)
            try:
                y = net(zt)
                y.backward(torch.from_numpy(d.dout.reshape(1, 1)).cuda())
                torch.cuda.synchronize()
                res[fused] = [y.detach().cpu().numpy(), zt.grad.cpu().numpy()] + [b.running_mean.cpu().numpy() for b in bns] + \
                             [b.running_var.cpu().numpy() for b in bns] + [p.grad.cpu().numpy() for p in order]
            except (RuntimeError, ValueError) as e:
                res[fused] = e
        finally:
            ops.LATENT_MLP = True
    print("N=1: fused %s, layer chain %s" % tuple("raised" if isinstance(res[f], Exception) else "returned" for f in (True, False)))
    if isinstance(res[True], Exception) or isinstance(res[False], Exception):
        assert isinstance(res[True], Exception) and isinstance(res[False], Exception), res
        return
    gmax = max(float(np.max(np.abs(g))) for g in res[False][8:])
    for i, (a, b) in enumerate(zip(res[True], res[False])):
        assert np.all(np.isfinite(a)) and a.shape == b.shape
        if i != 1 and i < 8:
            assert relerr(a, b) < BAR, (i, relerr(a, b))
        else:   # (the input gradient of a batch of one is analytically zero, like most of the parameter gradients)
            assert float(np.max(np.abs(a.astype(np.float64) - b))) <= BAR * gmax, i
