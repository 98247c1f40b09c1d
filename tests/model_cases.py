"""Models, inputs, parsed options and child processes of the step-level tests: the option record and the seeded models, the
tiny three-channel model of the loss tests with its inputs, one body for the captured-and-deferred checks of the optional
losses, and the runners of the loss worker and of `python -m dtgan_amd.train`."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

from golden_util import digest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
S = 64                                  # the grid of the loss tests' steps
BASE_KEYS = {True: ['D_A', 'G_A', 'Cyc_A', 'Cyc_z_B', 'KLD_z_B', 'D_B', 'G_B', 'Cyc_B', 'D_z_B', 'P_t_A', 'P_f_A', 'P_t_B', 'P_f_B'],
             False: ['D_A', 'G_A', 'Cyc_A', 'D_B', 'G_B', 'Cyc_B', 'P_t_A', 'P_f_A', 'P_t_B', 'P_f_B']}
# the paired step's scalars and gradient norms
SUP_KEYS = ['S_A', 'S_B', 'KLD_z_B', 'D_z_B']
SUP_GNORMS = ['gnorm_G_A_B', 'gnorm_G_B_A', 'gnorm_E_B', 'gnorm_D_z_B']


def make_opt(**kw):
    d = dict(input_nc=3, output_nc=3, ngf=32, nef=32, ndf=64, nlatent=16, lr=2e-4, beta1=0.5, max_gnorm=500.0,
             lambda_A=1.0, lambda_B=1.0, lambda_z_B=0.025, lambda_sup_A=0.1, lambda_sup_B=0.1, stoch_enc=False, z_gan=1,
             enc_A_B=1, no_lsgan=False, norm="instance", use_dropout=False, which_model_netG="resnet",
             which_model_netD="basic", gpu_ids=[0], monitor_gnorm=True, niter_decay=25, expr_dir="/tmp", n_blocks=3)
    d.update(kw)
    return argparse.Namespace(**d)


def build_model(meta):
    from hip_util import load_recipe
    from dtgan_amd import model as M
    opt = make_opt(**meta["opt"])
    m = M.AugmentedCycleGAN(opt, testing=True) if meta["aug"] else M.StochCycleGAN(opt, testing=True)
    for k, net in m._net_dict().items():
        load_recipe(net, k, meta["seed"], meta["flavour"])
    return m


STEP_TOL = {  # precision -> ((loss, gnorm, image) at step 0, the same after Adam updates)
    "f32": ((2e-4, 1e-3, 1e-4), (1e-2, 6e-2, 5e-3)),
    "bf16x3": ((1e-3, 3e-3, 1e-3), (2e-2, 6e-2, 2e-2)),
}


# cycle reconstructions rec_A / rec_B (model.py:467, 493) chain two generators: (step 0, later steps) per precision and
# fixture flavour.  'init' = the reference's own initialisation statistics (what training starts from): the north-star
# 1e-3 bar holds in bf16x3.  'rich' = O(1) InstanceNorm gains everywhere, deliberately ill-conditioned
# (tools/conditioning_probe.py: the EXACT-fp32 path itself moves rec_* by 4e-4..9e-4 under a 4e-6 input perturbation):
# bf16x3 lands at 1.8-7.9e-4 on the reference goldens (0.7-1.4e-3 in the 6-block oracle case, allowed 2e-3 there).  After an Adam update the fp32 oracle itself is 1.9e-2 from the
# reference on 'rich' (tests/test_oracle_golden.py).
# (after the first Adam update the exact-fp32 HIP path sits 8e-3 and bf16x3 2.5e-2 from the reference on the 'init' stoch_enc fixture: Adam turns
# summation-order noise on ~zero gradients into +-lr moves, and rec_* passes them through two generators)
# Round 6: the measured step-0 errors are recorded every run (ACG_REC_ERR_LOG; profiles/r06_rec_errors.txt) — 'rich' in bf16x3
# lands at 1.8e-4 .. 7.9e-4, so the reference goldens are all held to the north-star 1e-3 at step 0 now (the 3e-3 allowance
# of rounds 2-5 is 2e-3 now in the build's own 6-block oracle case below, which measures 7.3e-4 / 7.6e-4).
REC_TOL = {("f32", "init"): (2e-4, 2e-2), ("f32", "rich"): (3e-4, 4e-2),
           ("bf16x3", "init"): (1e-3, 4e-2), ("bf16x3", "rich"): (1e-3, 6e-2)}


# What the fixtures hold beyond losses and images (tools/make_goldens.py:292-304, taken from the reference after
# `optimizer.step()`, model.py:447-452, 510-515): per-tensor digests of .grad and of the applied update (post - pre), and
# the BatchNorm buffers after the last step.  (grad, update) tolerances on the abs-sum / L2 digests, step 0 only — later
# steps are chaotic per tensor (tests/test_oracle_golden.py).  bf16x3 gradients are norm-wise quantities: a ReLU mask that
# flips under the 2^-17 operand rounding changes single entries discretely (tools/conditioning_probe.py).
# Measured worst over the five fixtures: f32 inside (3e-3, 5e-3); bf16x3 on the 'init' flavour (the reference's own
# initialisation statistics) 1.2e-2 on one CondInstanceNorm shift-conv weight of the full-width config-1 fixture (a sum over
# ReLU-gated per-sample shifts), all other tensors < 1e-2.  On the deliberately ill-conditioned 'rich' flavour some bf16x3
# digests are not a pin: switching the InstanceNorm statistics between two equally accurate fp32 methods (both 1e-7 from fp64,
# test_conv_epilogue_statistics_equal_the_statistics_pass) moves the forward by 3e-5 and the CondInstanceNorm shift / scale
# convolution gradients by up to 17 % there (measured with the statistics A/B switches of DESIGN_LOG.md §5).  Those tensors get a bound of their own in bf16x3 on
# 'rich' (RICH_X3_BOUND; the f32 mode pins them at DIGEST_TOL on the same fixtures); every other tensor is held to the bf16x3
# tolerance.
DIGEST_TOL = {"f32": (3e-3, 5e-3), "bf16x3": (2e-2, 2e-2)}
# (network, parameter name) -> relative bound on both the gradient and the update digests: the latent-conditioned SHIFT layers
# (modules.py:111-118: ReLU(1x1 conv(z)), a sum over ReLU-gated per-sample shifts) of the two full-resolution CondInstanceNorms
# of G_A_B whose planes are largest — the only tensors of the 'rich' fixtures outside the bf16x3 tolerance (all others
# <= 2e-2).  Each bound is about twice the worst digest error measured over the two 'rich' fixtures (step_aug_small_s64,
# step_stoch_small_s64; printed as `digest_err` every run): model.2 weight 8.1e-3 / 6.6e-2, bias 5.1e-3 / 0.16; model.14
# bias 1.0e-3 / 3.3e-2.  model.14's weight (9.4e-4 / 8.2e-3) is held to DIGEST_TOL.
RICH_X3_BOUND = {("netG_A_B", "model.2.shift_conv.0.weight"): 0.13, ("netG_A_B", "model.2.shift_conv.0.bias"): 0.32,
                 ("netG_A_B", "model.14.shift_conv.0.bias"): 0.07}
# The --norm batch --use_dropout fixture: BatchNorm gains are ~N(1, 0.02) at initialisation (networks.py:19-21) where the
# InstanceNorm gains are ~N(0, 0.02), so G_B_A is a high-gain network there although the flavour is 'init', and D_A ends in
# BatchNorms over 4 samples x (2x2 | 1x1) maps.  tools/step_grad_conditioning.py: the EXACT-fp32 path moves G_B_A's gradients
# by 2e-4 .. 8e-3 (discretely: one LeakyReLU / ReLU unit on the other side) when its inputs are perturbed by 4e-6, G_A_B's by
# 2e-5; bf16x3 lands 8e-2 off on the head bias (a sum over all pixels of the image gradient), 2-4e-2 on two more tensors
# whose digests stay inside the tolerance.  That one tensor gets a bound of its own in bf16x3, about twice its measured digest
# error (8.0e-2); f32 pins it at DIGEST_TOL on the same fixture.
BN_DROPOUT_X3_BOUND = {("netG_B_A", "model.19.bias"): 0.16}
# Networks whose .grad after the step is comparable: the reference lets loss_G.backward() pile the (unused) G-phase
# gradients on top of the discriminators' D-phase .grad (model.py:509, no zero_grad for them); the HIP path skips those
# weight gradients, so the discriminators are pinned by their UPDATE digests (which only see the D-phase gradient).
GRAD_NETS = ("netG_A_B", "netG_B_A", "netE_B")


def check_digests(m, arr, pre, prec, flavour="init", bn_dropout=False, skip=()):
    """`skip`: (network, substring) pairs left out of the check (test_hip_bce's BCE_RICH_SKIP)"""
    gt, ut = DIGEST_TOL[prec]
    bounds = {}
    if prec == "bf16x3" and flavour == "rich":
        bounds.update(RICH_X3_BOUND)
    if prec == "bf16x3" and bn_dropout:
        bounds.update(BN_DROPOUT_X3_BOUND)
    bad, seen, skipped, bounded = [], 0, [], []
    for nname, net in m._net_dict().items():
        params = dict(net.named_parameters())
        grads = {k: (p.grad.detach().cpu().numpy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32))
                 for k, p in params.items()}
        gmax = max([float(np.max(np.abs(g))) for g in grads.values()] + [0.0])
        for k, p in params.items():
            key = "s0/grad/%s/%s" % (nname, k)
            assert key in arr, key
            g = grads[k]
            is_skip = any(nname == sn and sub in k for sn, sub in skip)
            own = [b for (sn, sub), b in bounds.items() if nname == sn and sub in k]
            gt_k, ut_k = (own[0], own[0]) if own else (gt, ut)
            if nname in GRAD_NETS:
                dg, rg = digest(g), arr[key]
                floor = 3e-5 * gmax * np.array([g.size, np.sqrt(g.size)])    # summation noise on analytically-zero gradients
                e = float(np.max(np.abs(dg[1:3] - rg[1:3]) / (np.abs(rg[1:3]) + 1e-30)))
                if own and not is_skip:
                    bounded.append(("grad", nname, k, e, own[0]))
                if not np.all(np.abs(dg[1:3] - rg[1:3]) <= gt_k * np.abs(rg[1:3]) + floor):
                    (skipped if is_skip else bad).append(("grad", nname, k, e))
                seen += 0 if is_skip else 1
            d = digest(p.detach().cpu().numpy().astype(np.float64) - pre[nname][k].astype(np.float64))
            r = arr["s0/upd/%s/%s" % (nname, k)]
            # Adam's g / (|g| + eps) amplifies rounding noise on ~zero gradients to O(lr): well-conditioned tensors only (for
            # the discriminators the criterion uses this side's D-phase gradient, which is what their update was made from)
            if np.min(np.abs(g)) > 1e-5 * gmax and np.min(np.abs(g)) > 1e-6:
                e = float(max(abs(d[1] - r[1]) / (r[1] + 1e-30), abs(d[2] - r[2]) / (r[2] + 1e-30)))
                if own and not is_skip:
                    bounded.append(("upd", nname, k, e, own[0]))
                if not (abs(d[1] - r[1]) <= ut_k * r[1] + 1e-12 and abs(d[2] - r[2]) <= ut_k * r[2] + 1e-12):
                    (skipped if is_skip else bad).append(("upd", nname, k, e))
                seen += 0 if is_skip else 1
    if skipped:
        print("digests outside the tolerance on tensors skipped by name (%s, %s):" % (prec, flavour), skipped)
    for kind, nname, k, e, b in bounded:   # the measurement beside the tensor's own bound, every run
        print("digest_err prec=%s flavour=%s %s %s/%s=%.3e allowed=%.1e" % (prec, flavour, kind, nname, k, e, b))
    assert seen > 50 and not bad, (len(bad), bad)


def tiny_model(aug=True, **kw):
    """three channels, width 8, four latents, the 'rich' recipe of seed 0"""
    from hip_util import load_recipe
    from dtgan_amd import model as M
    d = dict(input_nc=3, output_nc=3, ngf=8, nef=8, ndf=8, nlatent=4)
    d.update(kw)
    opt = make_opt(**d)
    m = (M.AugmentedCycleGAN if aug else M.StochCycleGAN)(opt, testing=True)
    for k, net in m._net_dict().items():
        load_recipe(net, k, 0, "rich")
    return m


def step_model(aug=True, **kw):
    """the model of the loss tests' steps: tiny_model with two blocks"""
    return tiny_model(aug=aug, n_blocks=2, **kw)


def step_inputs(seed=3, N=4, S=S, nl=4):
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.rand(N, 3, S, S, device="cuda", generator=g) * 2 - 1
    B = torch.tanh(torch.randn(N, 3, S, S, device="cuda", generator=g))
    return A, B, torch.randn(N, nl, 1, 1, device="cuda", generator=g)


def ensemble_model(kind="aug"):
    """the model of the ensemble translators' tests: tiny_model, or ('cycle_gan') its family without a latent code"""
    m = tiny_model(aug=kind == "aug")
    if kind == "cycle_gan":
        m.ignore_noise = True
    return m


def ensemble_inputs(N, S=S, seed=3):
    """A, B and the generator that drew them (for the codes that follow)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.rand(N, 3, S, S, device="cuda", generator=g) * 2 - 1
    B = torch.rand(N, 3, S, S, device="cuda", generator=g) * 2 - 1
    return A, B, g


def flat(m):
    """a copy of every network's flat parameters"""
    return {k: getattr(m, k).p.clone() for k in ("f_G_A_B", "f_G_B_A", "f_D_A", "f_D_B") + (("f_D_z_B", "f_E_B") if hasattr(m, "f_E_B") else ())}


def parse_train(tmp_path, *extra):
    from dtgan_amd import options as O
    return O.TrainOptions().parse(argv=["--name", "exp", "--checkpoints_dir", str(tmp_path), "--synthetic", "8", "--gpu_ids", "-1"]
                                  + list(extra))


def check_captured_and_deferred(step, options, keys, recapture, off, off_keys, aug=True, steps=4):
    """`step` ('train_instance' or 'supervised_train_instance') of three step_model(aug, **options): eager, captured, and
    captured with deferred scalars.  Two eager warm-up calls, the capture and its replay: the first replayed step runs the eager
    step's kernels on the eager step's numbers, so everything it reports equals the eager model's bit for bit (later steps carry
    the ulp of the device-side bias correction, test_hip_step.py); the deferred scalars are the synchronous graph's; one capture;
    each (option, new value) of `recapture` captures again with the terms (the keys beyond `off_keys`) finite; with `off` set
    the step names `off_keys` again."""
    from dtgan_amd import model as M
    paired = step == "supervised_train_instance"
    scalars = (lambda r: (r,)) if paired else (lambda r: (r[0], r[2]))          # what a step reports beside its images
    graph = (lambda: gr._sup_step_graph) if paired else (lambda: gr._step_graph)
    terms = [k for k in keys if k not in off_keys]
    ref, gr, lazy = step_model(aug, **options), step_model(aug, **options), step_model(aug, **options)
    gr.enable_step_graph(); lazy.enable_step_graph(defer_scalars=True)
    g = torch.Generator(device="cuda").manual_seed(11)
    prev = None
    for st in range(steps):
        A = torch.rand(4, 3, S, S, device="cuda", generator=g) * 2 - 1
        B = torch.rand(4, 3, S, S, device="cuda", generator=g) * 2 - 1
        z = torch.randn(4, 4, 1, 1, device="cuda", generator=g)
        rr, rg = getattr(ref, step)(A, B, z), getattr(gr, step)(A, B, z)
        out = getattr(lazy, step)(A, B, z)
        sr, sg = scalars(rr), scalars(rg)
        assert list(sg[0].keys()) == keys == list(sr[0].keys())
        if prev is not None:
            assert scalars(prev[0].result()) == prev[1]
            prev = None
        if isinstance(out, M.DeferredStep):
            prev = (out, sg)
        else:
            assert st < 2 and scalars(out)[0] == sg[0]
        print("step %d aug=%d: largest difference graph - eager %.3e" % (st, aug, max(abs(sr[0][k] - sg[0][k]) for k in sr[0])))
        if st <= 2:
            assert sg == sr, (st, sg, sr)
            if not paired:
                for k in rr[1]:
                    assert torch.equal(rr[1][k], rg[1][k]), (st, k)
        else:
            for k in sr[0]:
                assert abs(sr[0][k] - sg[0][k]) <= 2e-3 * max(1.0, abs(sr[0][k])), (st, k, sr[0][k], sg[0][k])
    assert prev is not None and scalars(prev[0].result())[0] == prev[1][0]
    assert graph().captures == 1
    for name, value in recapture:
        before = graph().captures
        setattr(gr.opt, name, value)
        v = scalars(getattr(gr, step)(A, B, z))[0]
        assert graph().captures == before + 1 and all(np.isfinite(v[k]) for k in terms), name
    for name, value in off.items():
        setattr(gr.opt, name, value)
    assert list(scalars(getattr(gr, step)(A, B, z))[0].keys()) == off_keys


def run_loss_worker(tmp_path, name, step, options, **env):
    """loss_dp_worker.py in a child process -> the arrays it saved"""
    out = str(tmp_path / (name + ".npz"))
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "ACGAN_DIST_FORCE")}
    e.update(env)
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(HERE, "loss_dp_worker.py"), out, step,
                        json.dumps(options)], env=e, capture_output=True, text=True, timeout=660)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return np.load(out)


def forced_pair(tmp_path, step, options, port):
    """the worker alone, and with one rank and every collective of the exchange forced"""
    plain = run_loss_worker(tmp_path, "plain", step, options)
    forced = run_loss_worker(tmp_path, "forced", step, options, ACGAN_DIST_FORCE="1", ACGAN_DP_BACKEND="nccl", RANK="0",
                             LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                             HSA_ENABLE_IPC_MODE_LEGACY="0")
    assert int(plain["forced"]) == 0 and int(forced["forced"]) == 1
    return plain, forced


def run_module(module, *args, limit=600):
    """`python -m dtgan_amd.<module> args` from the repository root under a time limit -> its output; fails with its tail"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "dtgan_amd." + module] + [str(a) for a in args]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=limit + 60)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-4000:]
    return out
