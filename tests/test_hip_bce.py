"""GPU: --no_lsgan (vanilla GAN) on the HIP path — the sigmoid epilogue of the discriminator heads, the fused latent
discriminator's sigmoid head, the binary cross-entropy loss kernels, and the models' training step against fixtures taken
from the reference's own sigmoid-headed networks with a float-target BCE (tools/make_goldens.py make_bce_goldens).

Semantics (model.criterion_GAN_bce): p = sigmoid(head(x)); loss = F.binary_cross_entropy(p, full_like(p, t)), t in {0., 1.};
the sigmoid and the loss are two autograd steps, as in the reference composite."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from golden_util import load, names  # noqa: E402
from model_cases import REC_TOL, STEP_TOL, build_model, check_digests, make_opt  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST_HEAD_KERNELS = ("igemm_conv_f32", "igemm_conv_bf16", "conv_patch16_x3", "conv_patchn_x3", "thin_out_conv")


# ---------------------------------------------------------------- loss kernels
def _probs(npix, Cp, seed):
    """probabilities from logits spread to +-40 (exact 0 / 1 among them: the -100 clamp and the 1e-12 floor), garbage in the
    pad lanes"""
    rs = np.random.RandomState(seed)
    logits = rs.uniform(-40.0, 40.0, (npix,)).astype(np.float32)
    p = torch.sigmoid(torch.from_numpy(logits)).numpy()
    p[:4] = [0.0, 1.0, 0.0, 1.0]
    full = rs.uniform(-3.0, 3.0, (npix, Cp)).astype(np.float32)
    full[::7, 1:] = np.nan
    full[:, 0] = p
    return full


@pytest.mark.parametrize("Cp", [4, 16])
@pytest.mark.parametrize("target", [0.0, 1.0])
def test_bce_const_kernels_match_torch_in_float64(Cp, target):
    from dtgan_amd import ops
    npix = 5000
    full = _probs(npix, Cp, 3 + Cp)
    p = torch.from_numpy(full).cuda().requires_grad_(True)
    loss = ops.BceConst.apply(p, 1, target)
    loss.backward(torch.tensor(1.7, device="cuda"))
    p64 = torch.from_numpy(full[:, :1].astype(np.float64)).requires_grad_(True)
    ref = F.binary_cross_entropy(p64, torch.full_like(p64, target))
    (ref * 1.7).backward()
    assert abs(float(loss) - float(ref)) <= 2e-6 * abs(float(ref)), (float(loss), float(ref))
    g = p.grad.cpu().numpy()
    assert np.all(g[:, 1:] == 0.0)                     # pad lanes ignored
    gr = p64.grad.numpy()[:, 0]
    assert np.allclose(g[:, 0], gr, rtol=2e-5, atol=1e-6 * np.max(np.abs(gr)))
    # deterministic: the same partial-sum tree every time
    again = [float(ops.BceConst.apply(p.detach(), 1, target)) for _ in range(2)]
    assert again[0] == again[1] == float(loss)


# ---------------------------------------------------------------- head convolutions at the bench geometry
def _pair(which, ndf):
    from dtgan_amd import networks as N
    from dtgan_amd.modules import mark_dirty
    mk = N.define_D_A if which == "A" else N.define_D_B
    torch.manual_seed(5)
    plain = mk(3, ndf, "basic", "instance", gpu_ids=[0])
    sig = mk(3, ndf, "basic", "instance", use_sigmoid=True, gpu_ids=[0])
    with torch.no_grad():
        for (k, a), (k2, b) in zip(plain.state_dict().items(), sig.state_dict().items()):
            assert k == k2
            b.copy_(a)
    mark_dirty(sig)
    return plain, sig


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("which,ndf", [("A", 32), ("B", 64)])
def test_sigmoid_heads_at_bench_geometry(which, ndf, prec):
    """configs[2]: N = 32, 256 x 256 x 3 (D_A ndf 32, D_B ndf 64, as the models build them)"""
    from hip_util import precision, Spy, l2rel
    from dtgan_amd import ops
    from dtgan_amd.model import criterion_GAN_bce
    with precision(prec):
        plain, sig = _pair(which, ndf)
        x = torch.from_numpy(np.random.RandomState(7).uniform(-1, 1, (32, 3, 256, 256)).astype(np.float32)).cuda()
        x1, x2 = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        with Spy() as spy:
            p = sig(x1)
        head = spy.kernels("acg_conv2d_fwd")[-1]
        assert head.startswith(FAST_HEAD_KERNELS), head
        logits = plain(x2)
        ref = torch.sigmoid(logits)
        err = float((p - ref).abs().max() / ref.abs().max())
        assert err <= (1e-6 if prec == "f32" else 1e-5), err
        # stored pad channels of the internal map are exactly zero (sigmoid(0) = 0.5 must not leak)
        with torch.no_grad():
            y = sig.forward_nhwc(ops.ToNHWC.apply(x, True))
        assert y.shape[-1] > 1 and bool((y[..., 1:] == 0).all())
        # input gradient of the BCE loss against torch autograd on sigmoid(net_lsgan(x))
        criterion_GAN_bce(p, True).backward()
        F.binary_cross_entropy(ref, torch.ones_like(ref)).backward()
        assert l2rel(x1.grad.cpu().numpy(), x2.grad.cpu().numpy()) < (1e-5 if prec == "f32" else 1e-4)


@pytest.mark.parametrize("impl", ["direct", "mfma"])
def test_sigmoid_head_pad_channels_zero_small(impl):
    """the thin VALU kernel (f32, <= 64 gathered channels) and the direct cross-check kernel write 0 in the pad channels"""
    from hip_util import precision
    from dtgan_amd import ops
    ops.set_conv_impl(impl)
    try:
        with precision("f32"):
            plain, sig = _pair("B", 8)
            x = torch.from_numpy(np.random.RandomState(9).uniform(-1, 1, (2, 3, 40, 40)).astype(np.float32)).cuda()
            with torch.no_grad():
                y = sig.forward_nhwc(ops.ToNHWC.apply(x, True))
                assert bool((y[..., 1:] == 0).all())
                ref = torch.sigmoid(plain(x))
                assert float((sig(x) - ref).abs().max()) <= 1e-6
    finally:
        ops.set_conv_impl("mfma")


# ---------------------------------------------------------------- latent discriminator
@pytest.mark.parametrize("fused", [True, False])
def test_latent_discriminator_sigmoid_head(fused):
    from hip_util import l2rel
    from dtgan_amd import networks as N, ops
    from dtgan_amd.modules import mark_dirty
    torch.manual_seed(3)
    plain = N.define_LAT_D(16, 64, gpu_ids=[0])
    sig = N.define_LAT_D(16, 64, use_sigmoid=True, gpu_ids=[0])
    sig.load_state_dict(plain.state_dict())
    mark_dirty(sig)
    z = torch.randn(32, 16, device="cuda") * 2.0
    z1, z2 = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
    before = ops.LATENT_MLP
    ops.LATENT_MLP = fused
    try:
        assert ops.latent_mlp_supported(32, 16, 64) == fused
        raw = sig.forward_dense(z1)
        p, pref = raw[:, :1], torch.sigmoid(plain(z2))
        assert bool((raw[:, 1:] == 0).all())
        assert float((p - pref).abs().max()) <= 1e-6
        F.binary_cross_entropy(p, torch.zeros_like(p)).backward()
        F.binary_cross_entropy(pref, torch.zeros_like(pref)).backward()
    finally:
        ops.LATENT_MLP = before
    assert l2rel(z1.grad.cpu().numpy(), z2.grad.cpu().numpy()) < 1e-5
    grads = [(k, a.grad.cpu().numpy(), b.grad.cpu().numpy()) for (k, a), (_, b) in zip(sig.named_parameters(), plain.named_parameters())]
    gmax = max(float(np.max(np.abs(g))) for _, _, g in grads)
    for k, a, b in grads:   # (+ a floor: the Linear biases in front of a BatchNorm have analytically zero gradients)
        assert np.linalg.norm(a - b) <= 1e-5 * np.linalg.norm(b) + 1e-6 * gmax * np.sqrt(b.size), k


# ---------------------------------------------------------------- reference goldens, network level
def _build_bce_net(meta):
    from dtgan_amd import networks as N
    c, n = meta["cfg"], meta["net"]
    if n == "netD_B":
        return N.define_D_B(c["input_nc"], c["ndf"], "basic", "instance", use_sigmoid=True, gpu_ids=[0])
    if n == "netD_A":
        return N.define_D_A(c["input_nc"], c["ndf"], "basic", "instance", use_sigmoid=True, gpu_ids=[0])
    if n == "netD_z_B":
        return N.define_LAT_D(c["nlatent"], c["ndf"], use_sigmoid=True, gpu_ids=[0])
    raise KeyError(n)


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", names("bce_net"))
def test_bce_net_matches_reference_golden(name, prec):
    from hip_util import precision, t, n, rel, l2rel, load_recipe
    arr, meta = load(name)
    with precision(prec):
        net = load_recipe(_build_bce_net(meta), meta["net"], meta["seed"], meta["flavour"])
        net.train()
        x = t(arr["in0"], grad=True)
        out = net.forward(x)
        assert tuple(out.shape) == arr["out0"].shape
        assert rel(n(out), arr["out0"]) < 1e-3
        (out * t(arr["R0"])).sum().backward()
        assert l2rel(n(x.grad), arr["gin0"]) < 1e-3
        got = np.concatenate([n(p.grad).ravel() for p in dict(net.named_parameters()).values()])
        ref = np.concatenate([arr["grad/" + k].ravel() for k in dict(net.named_parameters())])
        assert l2rel(got, ref) < 5e-3
        for k, b in net.named_buffers():
            if "buf/" + k in arr and not k.endswith("num_batches_tracked"):
                assert rel(n(b), arr["buf/" + k]) < 1e-3, k


# ---------------------------------------------------------------- reference goldens, training step
# On the deliberately ill-conditioned 'rich' flavour the latent-conditioned scale / shift layers of G_A_B (modules.py:111-118)
# are not a pin in either precision under the BCE objective: the REFERENCE's own step-0 gradient digests of those tensors
# move by up to 0.9 % when its weights are perturbed by 2e-7 relative (measured on the CPU with tools/make_goldens.py's
# step_case), above the f32 digest tolerance.  They are skipped by name on 'rich'; every other tensor keeps test_hip_step's
# tolerances, and the 'init' fixture pins them.
BCE_RICH_SKIP = (("netG_A_B", "shift_conv"), ("netG_A_B", "scale_conv"))


def _bce_check_digests(m, arr, pre, prec, flavour):
    """test_hip_step's digest check with BCE_RICH_SKIP on 'rich' in both precisions"""
    check_digests(m, arr, pre, prec, flavour, skip=BCE_RICH_SKIP if flavour == "rich" else ())


# After the first Adam update of the 'init' fixture the latent encoder's gradient norm is the most sensitive quantity of the
# step: the reference's own gnorm_E_B at step 1 moves by 0.8 % when its weights are perturbed by 2e-7 relative (a ~4e4
# amplification, measured on the CPU with make_goldens' step_case).  The exact-fp32 path holds test_hip_step's 6e-2; bf16x3
# (2^-17 operand rounding) lands 14 % off there, so in bf16x3 the step-1 gradient norms of that fixture get 0.2.
BCE_X3_INIT_STEP1_GNORM_TOL = 0.2


def _check_bce_steps(name, prec):
    """train_instance against a bce_step fixture, at test_hip_step's tolerances (STEP_TOL, REC_TOL, digests).  The fixtures
    store no inputs (oracle.recipe.inputs regenerates them from the seed; their digests are checked) and the images of the
    first meta["vis_samples"][k] samples of step k; losses, gradient norms and digests cover the whole batch."""
    from golden_util import digest
    from hip_util import t, n, rel
    from oracle import recipe
    arr, meta = load(name)
    m = build_model(meta)
    o = m.opt
    pre = {nn_: {k: p.detach().cpu().numpy().copy() for k, p in net.named_parameters()} for nn_, net in m._net_dict().items()}
    for st in range(meta["steps"]):
        A, B, z = recipe.inputs(meta["seed"] + st, meta["N"], o.input_nc, o.output_nc, meta["S"], o.nlatent)
        assert np.array_equal(digest(A), arr["s%d/real_A_digest" % st]) and np.array_equal(digest(B), arr["s%d/real_B_digest" % st])
        assert np.array_equal(z, arr["s%d/prior_z_B" % st])
        losses, visuals, gnorms = m.train_instance(t(A), t(B), t(z))
        assert list(losses.keys()) == meta["loss_keys"] and list(gnorms.keys()) == meta["gnorm_keys"]
        lt, gt, vt = STEP_TOL[prec][0 if st == 0 else 1]
        if prec == "bf16x3" and meta["flavour"] == "init" and st > 0:
            gt = BCE_X3_INIT_STEP1_GNORM_TOL
        got, ref = np.array(list(losses.values())), arr["s%d/losses" % st]
        assert np.allclose(got, ref, rtol=lt, atol=2e-6), (st, dict(zip(meta["loss_keys"], zip(got, ref))))
        gg, gr = np.array(list(gnorms.values())), arr["s%d/gnorms" % st]
        assert np.allclose(gg, gr, rtol=gt, atol=1e-6), (st, dict(zip(meta["gnorm_keys"], zip(gg, gr))))
        k = meta["vis_samples"][st]
        rt = REC_TOL[(prec, meta["flavour"])][0 if st == 0 else 1]
        for key, tol in (("fake_B", vt), ("fake_A", vt), ("rec_A", rt), ("rec_B", rt)):
            ref = arr["s%d/%s" % (st, key)]
            assert ref.shape[0] == k
            assert rel(n(visuals[key])[:k], ref) < tol, (key, st)
        assert np.array_equal(n(visuals["real_A"]), A) and np.array_equal(n(visuals["real_B"]), B)
        if st == 0:
            _bce_check_digests(m, arr, pre, prec, meta["flavour"])
    if meta["aug"]:   # BatchNorm running buffers after the last step
        for nname in ("netE_B", "netD_z_B"):
            for key, b in m._net_dict()[nname].named_buffers():
                ref = arr["final/buf/%s/%s" % (nname, key)]
                if key.endswith("num_batches_tracked"):
                    assert int(b) == int(ref), (nname, key)
                else:
                    assert rel(n(b), ref) < (2e-3 if prec == "f32" else 5e-3), (nname, key)


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", names("bce_step"))
def test_bce_train_instance_matches_reference_golden(name, prec):
    from hip_util import precision
    with precision(prec):
        _check_bce_steps(name, prec)


# ---------------------------------------------------------------- public API
def _opt(**kw):
    return make_opt(**dict(dict(input_nc=3, output_nc=3, ngf=8, nef=8, ndf=8, nlatent=4, no_lsgan=True), **kw))


def test_public_criterion_on_a_no_lsgan_model():
    from hip_util import l2rel
    from dtgan_amd import model as M
    m = M.AugmentedCycleGAN(_opt(), testing=True)
    assert m.criterionGAN is M.criterion_GAN_bce
    x = torch.from_numpy(np.random.RandomState(4).uniform(-1, 1, (3, 3, 64, 64)).astype(np.float32)).cuda()
    x1, x2 = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    p = m.netD_A(x1)
    assert bool(((p > 0) & (p < 1)).all())
    loss = m.criterionGAN(p, True)
    assert abs(float(loss) - float(M.criterion_GAN_bce(p.detach(), True))) == 0.0
    p64 = p.detach().double()
    assert abs(float(loss) - float(F.binary_cross_entropy(p64, torch.ones_like(p64)))) < 1e-6 * abs(float(loss)) + 1e-7
    loss.backward()
    p2 = m.netD_A(x2)
    F.binary_cross_entropy(p2, torch.ones_like(p2)).backward()
    assert torch.isfinite(x1.grad).all() and l2rel(x1.grad.cpu().numpy(), x2.grad.cpu().numpy()) < 1e-5
    with pytest.raises(NotImplementedError):
        M.criterion_GAN(p.detach(), True, use_sigmoid=True)
    pz = m.netD_z_B(torch.randn(4, 4, device="cuda"))
    assert pz.shape == (4, 1) and bool(((pz > 0) & (pz < 1)).all())
    assert float(m.criterionGAN(pz, False)) > 0.0


# ---------------------------------------------------------------- graph replay (fresh child process: it captures a graph)
_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np, torch
import dtgan_amd
from dtgan_amd import model as M
from hip_util import load_recipe
from model_cases import make_opt
from oracle import recipe
res = {}
for graph in (False, True):
    opt = make_opt(input_nc=3, output_nc=3, ngf=8, nef=8, ndf=8, nlatent=4, no_lsgan=True)
    m = M.AugmentedCycleGAN(opt, testing=True)
    for k, net in m._net_dict().items():
        load_recipe(net, k, 0, "init")
    if graph:
        m.enable_step_graph()
    out = []
    for st in range(5):
        A, B, z = (torch.from_numpy(a).cuda() for a in recipe.inputs(st, 4, 3, 3, 64, 4))
        losses, _, gn = m.train_instance(A, B, z)
        out.append([float(v) for v in losses.values()] + [float(v) for v in gn.values()])
    torch.cuda.synchronize()
    dig = [float(p.detach().double().abs().sum()) for net in m._net_dict().values() for p in net.parameters()]
    res["graph" if graph else "eager"] = dict(vals=out, digest=dig, replayed=bool(graph and m._step_graph.graph is not None))
print("RESULT " + json.dumps(res))
"""


def test_no_lsgan_step_graph_replay_equals_eager():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(line) == 1, r.stdout[-2000:]
    res = json.loads(line[0][7:])
    e, g = res["eager"], res["graph"]
    assert g["replayed"] and not e["replayed"]   # steps 3..5 were replays of the captured graph
    a, b = np.array(e["vals"]), np.array(g["vals"])
    assert np.all(np.isfinite(a)) and a.shape == b.shape
    assert np.allclose(a, b, rtol=1e-5, atol=1e-7), np.max(np.abs(a - b))
    assert np.allclose(e["digest"], g["digest"], rtol=1e-6, atol=0.0)
