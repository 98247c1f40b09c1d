"""The full-resolution layers of the generators on operands of 2 to 4 GiB, against float64.

Every convolution launcher refuses an operand of 4 GiB or more and forms byte offsets in 32 bits on that promise, and
model.ensemble_chunk sizes a generator pass so that its widest full-resolution tensor (2 * ngf channels) stays one image under
that limit.  These tests put the 64-channel tensor of an ngf-32 generator on both sides of byte 2^31 and right under 2^32 and
run every layer of networks._generator_layers that reads or writes it (modules.Conv2d / ConvTranspose2d / InstanceNorm /
CondInstanceNorm through forward_nhwc / forward_act, as the layer plan calls them), in both parity arithmetics:

    conv 3x3 s1 p1 32 -> 64 (writes it), (Cond)InstanceNorm(64) + ReLU, conv 3x3 s2 p1 64 -> 128 (reads it),
    ConvTranspose2d 128 -> 64 k3 s2 p1 op1 (writes it), conv 3x3 s1 p1 64 -> 32 (reads it);
    forward, data gradient, weight and bias gradient (norms: train forward + dx, parameter gradients, eval-state forward).

Sizes N x H x W of the 64-channel tensor: 129 x 256 x 256 (2^31 + 2^24 bytes: the first image past the signed limit),
255 x 256 x 256 (2^32 - 2^24: ensemble_chunk(32, 256, 256) itself) and 131 x 250 x 262 (2.20e9 bytes: W no multiple of 128, H * W
no multiple of the 128-pixel tile, so the fall-back tiles cross image boundaries past 2 GiB and the row pipeline must not run).

Data.  The N images are the 12 distinct images s * base_k, base_k three seeded normal images (k = i mod 3) and
s = 2^((i mod 4) - 1), exact in fp32 and under the bf16 hi / lo split.  The period 12 divides neither 128 nor 256 (and 3 divides
neither), so an offset that wraps by 2^31 or 2^32 bytes - 128 or 256 images of 2^24 bytes - reads or writes an image of another
class.  The tensors are built on the device by indexing; the float64 reference (F.conv2d / F.conv_transpose2d / the norm
formulas of test_hip_fuzz) is computed for the 12 distinct images only and ALL N images are compared against their class's
reference on the device, 12 images at a time; three scalars come back (max error, max |reference|, worst image).  Outputs and
data gradients are written into memory that held NaN (a NaN-filled block of the output's size is handed back to the caching
allocator right before the call, and the test asserts that the output took it): one NaN left anywhere fails the test.
Weight / bias / norm-parameter gradients take a dy that is random and distinct in every image; their reference uses
linearity: with S_c the float64 sum of dy_i over the images of class c, the gradient is that of the 12 images (x_c, S_c).

Bars: 2e-5 of max-abs on y and dx, 2e-4 on the norm's dx (those of test_hip_fastpath_fuzz / test_hip_fuzz, both arithmetics).
Summed gradients (dw, db, norm parameters; up to 1.7e7 pixels per sum): the larger of 1e-4 and 4 x the error measured for the
same layer at 127 x 256 x 256, where every byte offset is below 2^31 (BASE_127 below; the sum is at most twice as long and an
addressing error shows at 1 / N > 4e-3).  The kernel each case must run on is spelled in its id and asserted from
acg_last_kernel; the norm kernels do not depend on the convolution arithmetic and run once.

The gradient that reaches a norm + ReLU is set to zero where the float64 pre-activation lies within EDGE = 1e-5 of the ReLU's
kink (under 1e-3 of the elements): there the fp32 and the float64 mask may differ, and one flipped element moves a sum over
1.7e7 pixels by 1e-4 to 1e-3 of its size (measured on CondInstanceNorm at 127 images before this was done: 1.7e-3; after: 3e-7).

The end-to-end tests run an ngf-32, one-block CINResnetGenerator on one group of 255 images (85 inputs x 3 samples, the default
chunk) and on groups of 51.  test_translate_ensemble_at_the_default_chunk wants every output equal, as test_hip_ensemble does at
ngf 8 (it found the batch-dependent statistics of the row pipeline: see its docstring);
test_translate_ensemble_at_the_default_chunk_has_no_misplaced_image holds the same outputs to 1e-3, so that a failure of the
first tells rounding from a misplaced image.

Measured on one MI355X, worst case of all sizes: y 5.2e-6 and convolution dx 5.3e-6 (bar 2e-5), norm dx 2.1e-7 (bar 2e-4); dw 8.3e-6,
db 2.0e-6, norm parameters 4.8e-7 against their bars of 1e-4 (4 x the 127-image figures of BASE_127, at most 2.6e-5, is below the
project's 1e-4 everywhere).  End to end: every output equal.  Peak device
memory 16.6 GiB (the norm backward at 255 images: x, y, dy, dx of 4 GiB each); the 92 tests take 25 s, no case above 1.1 s.
"""
import gc
import zlib

import pytest
import torch
import torch.nn.functional as F

from conv_cases import (BASE_127, C_LARGE, EDGE, KERNELS, LARGE_CONV_CASES as CONV_CASES, LARGE_NORM_CASES as NORM_CASES,  # noqa: E402
                        LAYERS, NGF, NLATENT, PERIOD, SIZES, _ref_device, conv_id, expected_kernel, image_class, layer_shapes, norm_id)
from model_cases import tiny_model  # noqa: E402

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------------
# device-side helpers

def _free():
    gc.collect()
    torch.cuda.empty_cache()


def _gen(*key):
    return torch.Generator(device="cuda").manual_seed(zlib.crc32(repr(key).encode()))


def _periodic(base, N):
    """(3, ...) base images -> the N images s * base_k of image_class, built by indexing on the device"""
    idx = torch.arange(N, device="cuda")
    x = base[idx % 3]
    x.mul_(torch.exp2((idx % 4).float() - 1).view(N, *([1] * (base.dim() - 1))))
    return x


def _periodic_normal(shape, *key):
    return _periodic(torch.randn((3,) + tuple(shape[1:]), device="cuda", generator=_gen(*key)), shape[0])


def _poison(shape):
    """hand a NaN-filled block of `shape` floats back to the (otherwise empty) caching allocator -> its address: the next
    allocation of that size takes it"""
    torch.cuda.synchronize()
    _free()
    t = torch.full(tuple(shape), float("nan"), device="cuda")
    p = t.data_ptr()
    del t
    return p


def _workspace():
    from dtgan_amd import ops
    ops.workspace(1 << 28)   # grown once: no launch of this file allocates scratch between _poison and its output


def _class_sums(dy):
    """S_c = sum of dy_i over the images i of class c, in float64: (12, ...)"""
    S = torch.zeros((PERIOD,) + tuple(dy.shape[1:]), dtype=torch.float64, device="cuda")
    for i0 in range(0, dy.shape[0], PERIOD):
        n = min(PERIOD, dy.shape[0] - i0)
        S[:n] += dy[i0:i0 + n]
    return S


def _compare_all(got, ref12, bar, what):
    """every image of `got` (N, ...) against its class's float64 reference (12, ...): three scalars are read back"""
    N = got.shape[0]
    assert tuple(got.shape[1:]) == tuple(ref12.shape[1:]), (what, got.shape, ref12.shape)
    err = torch.empty(N, dtype=torch.float64, device="cuda")
    for i0 in range(0, N, PERIOD):
        n = min(PERIOD, N - i0)
        err[i0:i0 + n] = (got[i0:i0 + n].double() - ref12[:n]).abs_().flatten(1).amax(1)
    nan = torch.isnan(err)
    worst = torch.where(nan.any(), nan.float().argmax(), err.argmax())
    e, i, scale = float(err.max()), int(worst), float(ref12.abs().max())
    print("MEASURED %s: max error %.3e of max-abs %.3e = %.3e (bar %.0e), worst image %d of %d" % (what, e, scale, e / scale, bar, i, N))
    assert e == e, "%s: image %d still holds NaN (never written)" % (what, i)
    assert e < bar * scale, "%s: error %.3e of max-abs %.3e at image %d (class %s)" % (what, e, scale, i, image_class(i))


def _rel(a, b):
    return float((a.double() - b).abs().max() / (b.abs().max() + 1e-300))


# ---------------------------------------------------------------------------------------------------------------------
# convolutions

def _conv_module(layer):
    """the layer with seeded parameters, its packed weights built (call inside hip_util.precision)"""
    from dtgan_amd import modules as M
    Ci, Co, stride, tr, _ = LAYERS[layer]
    if tr:
        m = M.ConvTranspose2d(Ci, Co, 3, stride=2, padding=1, output_padding=1, bias=True).cuda()
    else:
        m = M.Conv2d(Ci, Co, 3, stride=stride, padding=1, bias=True).cuda()
    g = _gen(layer, "parameters")
    with torch.no_grad():
        m.weight.copy_(torch.randn(m.weight.shape, device="cuda", generator=g) * (1.5 / (9 * Ci) ** 0.5))
        m.bias.copy_(torch.randn(m.bias.shape, device="cuda", generator=g) * 0.5)
    m.packed()
    return m


def _conv_ref(layer, m, x12, g12, want):
    """float64 on the 12 distinct images (NHWC in, NHWC out): y, or with the output gradient g12 the gradients in `want`"""
    Ci, Co, stride, tr, _ = LAYERS[layer]
    dev = _ref_device()
    X = x12.permute(0, 3, 1, 2).double().to(dev).requires_grad_(True)
    Wt, B = (p.detach().double().to(dev).requires_grad_(True) for p in (m.weight, m.bias))
    if tr:
        y = F.conv_transpose2d(X, Wt, B, stride=2, padding=1, output_padding=1)
    else:
        y = F.conv2d(X, Wt, B, stride=stride, padding=1)
    if g12 is None:
        return y.detach().permute(0, 2, 3, 1).contiguous().cuda()
    y.backward(g12.permute(0, 3, 1, 2).double().to(dev))
    out = {"dx": X.grad.permute(0, 2, 3, 1).contiguous().cuda(), "dw": Wt.grad.cuda(), "db": B.grad.cuda()}
    return [out[k] for k in want]


def _check_kernel(layer, what, size, prec, kernels):
    name = expected_kernel(layer, what, size, prec)
    assert kernels, (layer, what, "no launch recorded")
    k = kernels[-1]
    assert KERNELS[name] in k, (layer, what, "expected", KERNELS[name], "ran", kernels)
    if name == "bf16tile":
        assert "RP=1" not in k, k
    if size[2] % 128:
        assert not any(KERNELS["rows"] in q for q in kernels), ("the row pipeline ran at W = %d" % size[2], kernels)


def run_conv(layer, what, size, prec):
    """one pass of one layer at one size.  fwd / dgrad: every image is compared inside (asserts); wgrad: -> {"dw": rel, "db": rel}"""
    from hip_util import Spy, precision
    x_shape, y_shape = layer_shapes(layer, size)
    tr = LAYERS[layer][3]
    pre = "acg_conv_transpose2d_" if tr else "acg_conv2d_"
    _workspace()
    with precision(prec):
        m = _conv_module(layer)
        x = _periodic_normal(x_shape, layer, size, "x")
        if what == "fwd":
            p = _poison(y_shape)
            with torch.no_grad(), Spy() as spy:
                y = m.forward_nhwc(x)
            assert y.data_ptr() == p and tuple(y.shape) == y_shape, "the output did not take the NaN-filled block"
            _check_kernel(layer, what, size, prec, spy.kernels(pre + "fwd"))
            _compare_all(y, _conv_ref(layer, m, x[:PERIOD], None, ()), 2e-5, "y")
            return None
        if what == "dgrad":
            for q in m.parameters():
                q.requires_grad_(False)
            x.requires_grad_(True)
            y = m.forward_nhwc(x)
            dy = _periodic_normal(y_shape, layer, size, "dy")
            p = _poison(x_shape)
            with Spy() as spy:
                dx, = torch.autograd.grad(y, [x], dy)
            assert dx.data_ptr() == p and tuple(dx.shape) == x_shape, "dx did not take the NaN-filled block"
            _check_kernel(layer, what, size, prec, spy.kernels(pre + "bwd_data"))
            del y
            ref, = _conv_ref(layer, m, x.detach()[:PERIOD], dy[:PERIOD], ("dx",))
            _compare_all(dx, ref, 2e-5, "dx")
            return None
        y = m.forward_nhwc(x)
        dy = torch.randn(y_shape, device="cuda", generator=_gen(layer, size, "random dy"))
        with Spy() as spy:
            dw, db = torch.autograd.grad(y, [m.weight, m.bias], dy)
        _check_kernel(layer, what, size, prec, spy.kernels(pre + "bwd_weight"))
        del y
        dw_r, db_r = _conv_ref(layer, m, x[:PERIOD], _class_sums(dy), ("dw", "db"))
        assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
        return {"dw": _rel(dw, dw_r), "db": _rel(db, db_r)}


def summed_bar(key, name):
    """the bar of a summed gradient: the larger of the project's 1e-4 and 4 x the error measured at 127 x 256 x 256"""
    return max(1e-4, 4.0 * BASE_127[key][name])


@pytest.mark.parametrize("case", CONV_CASES, ids=conv_id)
def test_convolution_against_fp64(case):
    layer, what, size, prec = case
    if size == SIZES[1]:
        from dtgan_amd.model import ensemble_chunk
        assert ensemble_chunk(NGF, size[1], size[2]) == size[0]
    try:
        got = run_conv(layer, what, size, prec)
        if what == "wgrad":
            for name, e in got.items():
                bar = summed_bar((layer, prec), name)
                print("MEASURED %s: %.3e (bar %.1e)" % (name, e, bar))
            for name, e in got.items():
                assert e < summed_bar((layer, prec), name), (name, e, summed_bar((layer, prec), name))
    finally:
        _free()
    print("PEAK %.2f GiB" % (torch.cuda.max_memory_allocated() / 2.0 ** 30))


# ---------------------------------------------------------------------------------------------------------------------
# norms (+ ReLU, as the layer plan runs them on the large tensor)

def _norm_module(kind):
    from dtgan_amd import modules as M
    g = _gen(kind, "parameters")
    C = C_LARGE
    if kind == "in":
        m = M.InstanceNorm(C).cuda()
        with torch.no_grad():
            m.scale.copy_(1 + 0.3 * torch.randn(C, device="cuda", generator=g))
            m.shift.copy_(0.3 * torch.randn(C, device="cuda", generator=g))
        return m, None
    m = M.CondInstanceNorm(C, NLATENT).cuda()
    with torch.no_grad():
        for seq, mean in ((m.scale_conv, 1.0), (m.shift_conv, 0.2)):
            seq[0].weight.copy_(0.3 * torch.randn(seq[0].weight.shape, device="cuda", generator=g))
            seq[0].bias.copy_(mean + 0.3 * torch.randn(C, device="cuda", generator=g))
    z12 = torch.randn((PERIOD, NLATENT), device="cuda", generator=g)
    return m, z12


def _norm_params(kind, m):
    if kind == "in":
        return [("dscale", m.scale), ("dshift", m.shift)]
    return [("dscale_w", m.scale_conv[0].weight), ("dscale_b", m.scale_conv[0].bias),
            ("dshift_w", m.shift_conv[0].weight), ("dshift_b", m.shift_conv[0].bias)]


def _norm_ref(kind, m, z12, x12, g12):
    """the norm formulas of test_hip_fuzz (InstanceNorm: biased variance; CondInstanceNorm: unbiased, scale / shift =
    ReLU(1x1 conv(z))) + ReLU, float64, NHWC, on the 12 distinct images -> (y, [|pre-activation| > EDGE]), or with g12
    (dx, parameter gradients)"""
    X = x12.double().requires_grad_(True)
    P = [q.detach().double().requires_grad_(True) for _, q in _norm_params(kind, m)]
    mu = X.mean(dim=(1, 2), keepdim=True)
    if kind == "in":
        var = ((X - mu) ** 2).mean(dim=(1, 2), keepdim=True)
        sc, sh = P[0].view(1, 1, 1, -1), P[1].view(1, 1, 1, -1)
    else:
        var = X.var(dim=(1, 2), keepdim=True, unbiased=True)
        Z = z12.double()
        sc = torch.relu(Z @ P[0].view(C_LARGE, NLATENT).t() + P[1]).view(PERIOD, 1, 1, -1)
        sh = torch.relu(Z @ P[2].view(C_LARGE, NLATENT).t() + P[3]).view(PERIOD, 1, 1, -1)
    pre = (X - mu) / torch.sqrt(var + 1e-5) * sc + sh
    y = torch.relu(pre)
    if g12 is None:
        pre = pre.detach()   # (exactly 0: a channel whose scale and shift the ReLU of CondInstanceNorm clamped; no gradient on either side)
        return y.detach(), (pre.abs() > EDGE) | (pre == 0)
    y.backward(g12.double())
    return X.grad, [q.grad for q in P]


def _mask_edges(dy, live12):
    """zero dy where the ReLU in front of it sits within EDGE of its kink (per class: the images of a class are identical)"""
    for i0 in range(0, dy.shape[0], PERIOD):
        n = min(PERIOD, dy.shape[0] - i0)
        dy[i0:i0 + n] *= live12[:n]
    return dy


def _norm_forward(kind, m, x, z12):
    from dtgan_amd import ops
    if kind == "in":
        return m.forward_act(x, ops.ACT_RELU)
    idx = torch.arange(x.shape[0], device="cuda") % PERIOD
    return m.forward_act(x, z12[idx].contiguous(), ops.ACT_RELU)


def run_norm(kind, what, size):
    """eval_fwd / train_fwd_dx: every image is compared inside (asserts); train_params: -> {name: rel}"""
    from hip_util import Spy
    from dtgan_amd.model import eval_state
    shape = size + (C_LARGE,)
    _workspace()
    m, z12 = _norm_module(kind)
    x = _periodic_normal(shape, kind, size, "x")
    x.mul_(1.2).add_(0.3)
    if what == "eval_fwd":
        p = _poison(shape)
        with eval_state(m), torch.no_grad(), Spy() as spy:
            y = _norm_forward(kind, m, x, z12)
        assert y.data_ptr() == p, "the output did not take the NaN-filled block"
        assert {"acg_norm_stats", "acg_norm_apply"} <= spy.entries(), spy.entries()
        _compare_all(y, _norm_ref(kind, m, z12, x[:PERIOD], None)[0], 2e-5, "y")
        return None
    m.train()
    if what == "train_fwd_dx":
        x.requires_grad_(True)
        p = _poison(shape)
        with Spy() as spy:
            y = _norm_forward(kind, m, x, z12)
        assert y.data_ptr() == p, "the output did not take the NaN-filled block"
        assert {"acg_norm_stats", "acg_norm_apply"} <= spy.entries(), spy.entries()
        y_r, live = _norm_ref(kind, m, z12, x.detach()[:PERIOD], None)
        _compare_all(y.detach(), y_r, 2e-5, "y")
        del y_r
        dy = _mask_edges(_periodic_normal(shape, kind, size, "dy"), live)
        p = _poison(shape)
        with Spy() as spy:
            dx, = torch.autograd.grad(y, [x], dy)
        assert dx.data_ptr() == p, "dx did not take the NaN-filled block"
        assert "acg_norm_bwd" in spy.entries(), spy.entries()
        del y
        dx_r, _ = _norm_ref(kind, m, z12, x.detach()[:PERIOD], dy[:PERIOD])
        _compare_all(dx, dx_r, 2e-4, "dx")
        return None
    y = _norm_forward(kind, m, x, z12)
    live = _norm_ref(kind, m, z12, x[:PERIOD], None)[1]
    assert float(live.float().mean()) > 1 - 1e-3
    dy = _mask_edges(torch.randn(shape, device="cuda", generator=_gen(kind, size, "random dy")), live)
    del live
    names, params = zip(*_norm_params(kind, m))
    with Spy() as spy:
        grads = torch.autograd.grad(y, list(params), dy)
    assert "acg_norm_bwd" in spy.entries(), spy.entries()
    del y
    _, refs = _norm_ref(kind, m, z12, x[:PERIOD], _class_sums(dy))
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    return {n: _rel(g, r) for n, g, r in zip(names, grads, refs)}


@pytest.mark.parametrize("case", NORM_CASES, ids=norm_id)
def test_norm_against_fp64(case):
    kind, what, size = case
    try:
        got = run_norm(kind, what, size)
        if what == "train_params":
            for name, e in got.items():
                print("MEASURED %s: %.3e (bar %.1e)" % (name, e, summed_bar((kind, "norm"), name)))
            for name, e in got.items():
                assert e < summed_bar((kind, "norm"), name), (name, e, summed_bar((kind, "norm"), name))
    finally:
        _free()
    print("PEAK %.2f GiB" % (torch.cuda.max_memory_allocated() / 2.0 ** 30))


# ---------------------------------------------------------------------------------------------------------------------
# end to end at the default chunk

E2E_INPUTS, E2E_M, E2E_S = 85, 3, 256


@pytest.fixture(scope="module")
def ensemble_runs():
    """85 inputs x 3 samples at 256 x 256 through an ngf-32, one-block CINResnetGenerator (built as test_hip_ensemble builds its
    own): translate_ensemble with the default chunk and with chunk=51 -> (outputs, outputs, images per generator pass of each)"""
    m = tiny_model(ngf=NGF, n_blocks=1)
    g = _gen("end to end")
    A = torch.rand(E2E_INPUTS, 3, E2E_S, E2E_S, device="cuda", generator=g) * 2 - 1
    B = torch.rand(E2E_INPUTS, 3, E2E_S, E2E_S, device="cuda", generator=g) * 2 - 1
    z = torch.randn(E2E_INPUTS * E2E_M, m.opt.nlatent, 1, 1, device="cuda", generator=g)
    G = m.netG_A_B
    groups, real = [], G.forward_nhwc

    def counted(x, zz):
        groups.append(x.shape[0])
        return real(x, zz)
    G.forward_nhwc = counted
    try:
        one = m.translate_ensemble(A, E2E_M, z=z, real_B=B)
        n_one = list(groups)
        del groups[:]
        many = m.translate_ensemble(A, E2E_M, z=z, real_B=B, chunk=51)
        n_many = list(groups)
    finally:
        del G.forward_nhwc
    del m, A, B, z
    _free()
    print("PEAK %.2f GiB" % (torch.cuda.max_memory_allocated() / 2.0 ** 30))
    yield one, many, n_one, n_many
    del one, many
    _free()


def test_translate_ensemble_at_the_default_chunk(ensemble_runs):
    """the default chunk makes ONE group of 255 images (the 64-channel tensors of the stem and the tail are 2^32 - 2^24 bytes),
    chunk=51 five groups of 0.85 GB tensors; every output equal (torch.equal; allclose for crps_fair: test_hip_ensemble's
    standard for grouped against one input per group).

    This test found that a generator pass was not bit-identical across group sizes: the row pipeline (conv_rows_x3, the stem's
    32 -> 64 convolution) hands the norm behind it the JOINT statistics of the R rows a workgroup owns, and R follows the batch
    (256 rows per workgroup at 255 images, 86 at 51), so the outputs differed by rounding from the second stage on (4.3e-5 of
    max-abs 1.0; test_hip_ensemble's own comparison runs at ngf 8, where that kernel does not run).  A forward under
    torch.no_grad() now leaves those statistics to the norm's own pass (acg_conv2d_fwd_stats_per_tile, ops.Conv2dFn)."""
    from dtgan_amd.model import ensemble_chunk
    one, many, n_one, n_many = ensemble_runs
    assert ensemble_chunk(NGF, E2E_S, E2E_S) == E2E_INPUTS * E2E_M == SIZES[1][0]
    assert n_one == [E2E_INPUTS * E2E_M] and n_many == [51] * 5, (n_one, n_many)
    assert set(one) == set(many)
    for k in one:
        print("MEASURED %s: max |difference| %.3e" % (k, float((one[k].double() - many[k].double()).abs().max())))
    for k in one:
        assert torch.equal(one[k], many[k]) or (k == "crps_fair" and torch.allclose(one[k], many[k])), k


def test_translate_ensemble_at_the_default_chunk_has_no_misplaced_image(ensemble_runs):
    """the same two calls held to a bar that rounding passes and a misplaced image cannot: per input, the maps (mean, std,
    quantiles, crps_map; translations lie in [-1, 1]) within 1e-3, the bf16x3 parity bar on activations (hip_util); the scores
    within 1e-3 relative; the rank histogram, a count over C * H * W cells that a member crossing the target by rounding can
    move, within 1e-3 of the cells.  A byte offset that wraps in the one group of 255 puts another input's translation, zeros or
    nothing (NaN is refused) into inputs 43 .. 84: differences of the order of the values themselves."""
    one, many, n_one, n_many = ensemble_runs
    assert n_one == [E2E_INPUTS * E2E_M] and n_many == [51] * 5, (n_one, n_many)
    cells = 3 * E2E_S * E2E_S
    for k in sorted(one):
        a, b = one[k].double(), many[k].double()
        assert a.shape == b.shape and a.shape[0] == E2E_INPUTS, k
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), k
        d = (a - b).abs().reshape(E2E_INPUTS, -1)
        if k == "rank_hist":
            err, bar = d.sum(1), 1e-3 * cells
        elif a.dim() >= 4:
            err, bar = d.amax(1), 1e-3
        else:
            err, bar = d.amax(1) / b.abs().reshape(E2E_INPUTS, -1).amax(1).clamp_min(1e-30), 1e-3
        worst = int(err.argmax())
        print("MEASURED %s: worst input %d, %.3e (bar %.1e)" % (k, worst, float(err[worst]), bar))
        assert float(err[worst]) < bar, (k, "input", worst, float(err[worst]), bar)
