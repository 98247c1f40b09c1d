"""GPU tests of the structural-similarity loss in training and of the offline metric: the unpaired step of both families with
--lambda_ssim_A / --lambda_ssim_B (eager, captured and deferred), the paired step, model.translate_ssim, `--metric ssim` in
process on a saved tiny checkpoint and `python -m dtgan_amd.train --lambda_ssim_B` in a child process."""
import os
import re

import numpy as np
import pytest
import torch

import ssim_ref as R
from eval_cases import make_experiment
from model_cases import BASE_KEYS, S, check_captured_and_deferred, flat as _flat, run_module, step_inputs as _inputs, step_model as _model
from ssim_ref import VALUE_TOL

pytestmark = pytest.mark.gpu

SSIM = ["Ssim_A", "Ssim_B"]


@pytest.mark.parametrize("aug", [True, False])
def test_step_reports_the_reference_losses_and_the_term_enters_loss_G_only(aug, monkeypatch):
    from dtgan_amd import ops
    maps_seen = []
    real_call = ops._ssim_call
    monkeypatch.setattr(ops, "_ssim_call", lambda *a: (maps_seen.append(a[-1] is not None), real_call(*a))[1])
    A, B, z = _inputs()
    off, on_B, on_A = _model(aug), _model(aug, lambda_ssim_B=0.5), _model(aug, lambda_ssim_A=0.5, lambda_ssim_B=0.0)
    l0, v0, g0 = off.train_instance(A, B, z)
    assert list(l0.keys()) == BASE_KEYS[aug] and maps_seen == []               # the default step: today's dict, no new launch
    for m, with_maps in ((on_B, [False, True]), (on_A, [True, False])):
        del maps_seen[:]
        l, v, gn = m.train_instance(A, B, z)
        assert maps_seen == with_maps                                           # the weight-0 partner: a monitor without gradient
        assert list(l.keys()) == BASE_KEYS[aug] + SSIM and list(gn.keys()) == list(g0.keys())
        for k in BASE_KEYS[aug]:                                                # the forward passes do not see the new term
            assert l[k] == l0[k], (k, l[k], l0[k])
        for k in v0:
            assert torch.equal(v[k], v0[k]), k
        h = {k: t.cpu().numpy() for k, t in v.items()}
        for name, rec, real in (("Ssim_A", "rec_A", "real_A"), ("Ssim_B", "rec_B", "real_B")):
            ref = R.ssim_loss(h[rec], h[real])
            err = abs(l[name] - ref)
            print("%s aug=%d: %.7f (reference %.7f, error %.3e, allowed %.3e)" % (name, aug, l[name], ref, err, VALUE_TOL))
            assert np.isfinite(l[name]) and err <= VALUE_TOL, (name, l[name], ref)
    p0, pB, pA = _flat(off), _flat(on_B), _flat(on_A)
    for k in p0:
        if k.startswith("f_D"):                                                 # the term enters loss_G only
            assert torch.equal(p0[k], pB[k]) and torch.equal(p0[k], pA[k]), k
    for k in ("f_G_A_B", "f_G_B_A"):                                            # a reconstruction went through both generators
        assert not torch.equal(p0[k], pB[k]) and not torch.equal(p0[k], pA[k]), k


@pytest.mark.parametrize("aug", [True, False])
def test_every_family_names_its_scalars_in_order(aug):
    A, B, z = _inputs()
    l, _, _ = _model(aug, lambda_spec_A=0.25, lambda_marg_B=0.5, lambda_ssim_A=0.1).train_instance(A, B, z)
    assert list(l.keys()) == BASE_KEYS[aug] + ["Spec_A", "Spec_B", "Marg_A", "Marg_B"] + SSIM
    assert all(np.isfinite(l[k]) for k in l)
    l, _, _ = _model(aug, lambda_marg_A=0.25, lambda_ssim_B=0.1).train_instance(A, B, z)
    assert list(l.keys()) == BASE_KEYS[aug] + ["Marg_A", "Marg_B"] + SSIM


@pytest.mark.parametrize("aug", [True, False])
def test_captured_and_deferred_steps_with_the_loss_on(aug):
    """a change of either weight re-captures; both off: the 13 (10) keys again"""
    check_captured_and_deferred("train_instance", dict(lambda_ssim_A=0.25, lambda_ssim_B=0.5), BASE_KEYS[aug] + SSIM,
                                (("lambda_ssim_B", 0.125), ("lambda_ssim_A", 0.0)), dict(lambda_ssim_B=0.0), BASE_KEYS[aug], aug=aug)


def test_the_paired_step_names_the_terms_and_keeps_its_gradient_norms():
    A, B, z = _inputs()
    off, on = _model(True), _model(True, lambda_ssim_A=0.3, lambda_ssim_B=0.2)
    v0, v1 = off.supervised_train_instance(A, B, z), on.supervised_train_instance(A, B, z)
    gnorms = ['gnorm_G_A_B', 'gnorm_G_B_A', 'gnorm_E_B', 'gnorm_D_z_B']
    assert list(v0.keys()) == ['S_A', 'S_B', 'KLD_z_B', 'D_z_B'] + gnorms
    assert list(v1.keys()) == ['S_A', 'S_B', 'KLD_z_B', 'D_z_B', 'S_ssim_A', 'S_ssim_B'] + gnorms
    for k in ('S_A', 'S_B', 'KLD_z_B', 'D_z_B'):                                # computed before either update
        assert v1[k] == v0[k], k
    assert 0.0 <= v1['S_ssim_A'] <= 2.0 and 0.0 <= v1['S_ssim_B'] <= 2.0          # a loss as it is, not its square root
    for m, v in ((off, v0), (on, v1)):
        for k, flat in zip(gnorms, (m.f_G_A_B, m.f_G_B_A, m.f_E_B, m.f_D_z_B)):
            want = float(torch.sqrt((flat.gv.double() ** 2).sum()))              # the network's own gradient, clipped to max_gnorm
            assert np.isfinite(v[k]) and want > 0 and abs(min(v[k], 500.0) - want) <= 1e-4 * want, (k, v[k], want)
    assert v1['gnorm_G_A_B'] != v0['gnorm_G_A_B'] and v1['gnorm_G_B_A'] != v0['gnorm_G_B_A']   # the terms reached the generators
    assert v1['gnorm_D_z_B'] == v0['gnorm_D_z_B']


def test_translate_ssim():
    from dtgan_amd import ops
    from dtgan_amd.model import eval_state, plan_ensemble
    m = _model(True)
    A, B, _ = _inputs(N=3)
    g = torch.Generator(device="cuda").manual_seed(5)
    z = torch.randn(6, 4, 1, 1, device="cuda", generator=g)
    r = m.translate_ssim(A, 2, B, z=z, chunk=4)                                 # two groups: 2 inputs, then 1
    assert set(r) == {"members", "ens_mean"}
    assert r["members"].shape == (3, 2, 3, 2) and r["ens_mean"].shape == (3, 3, 2) and r["members"].dtype == torch.float32
    assert torch.isfinite(r["members"]).all() and torch.isfinite(r["ens_mean"]).all()
    assert r["members"].abs().max() <= 1 and r["ens_mean"].abs().max() <= 1
    M_, N, C, H, W, zz, per = plan_ensemble("test", m.opt, A, 2, z, B, 4, need_B=True)
    assert per == 2
    with eval_state(m.netG_A_B), torch.no_grad():
        for g0, n, members in m.ensemble_groups(A, zz, 2, per):
            own = ops.ssim(members, B[g0:g0 + n].contiguous(), 3, "nhwc", "nchw", x_per_y=2)
            assert torch.equal(own.view(n, 2, 3, 2), r["members"][g0:g0 + n])
            host = R.ssim(ops.ToNCHW.apply(members, 3).cpu().numpy(), B[g0:g0 + n].cpu().numpy(), x_per_y=2)
            assert np.abs(own.cpu().numpy() - host).max() <= VALUE_TOL
    again = m.translate_ssim(A, 2, B, z=z)                                      # one group: the same bits
    assert torch.equal(again["members"], r["members"]) and torch.equal(again["ens_mean"], r["ens_mean"])
    one = m.translate_ssim(A, 1, B, z=z[:3])
    assert one["members"].shape == (3, 1, 3, 2) and torch.equal(one["members"][:, 0], one["ens_mean"])   # M = 1: the member itself
    with pytest.raises(ValueError, match="translate_ssim"):
        m.translate_ssim(A, 2, B[:2], z=z)


@pytest.fixture(scope="module")
def experiment(tmp_path_factory):
    """a synthetic .npz split (10 train -> 5 dev + 5 train, 3 test) and the checkpoint <expr_dir>/latest of a seeded tiny model"""
    return make_experiment(tmp_path_factory.mktemp("ssim_metric"), S, 10, 3)


def test_metric_ssim_writes_its_file(experiment, capsys):
    from dtgan_amd import eval_metrics as EM, ops, test as T
    prec = ops.get_precision()
    try:
        T.test_model(["--chk_path", experiment["chk"], "--dataroot", experiment["data"], "--metric", "ssim", "--n_samples", "2",
                      "--res_dir", "res_ssim"])
    finally:
        ops.set_precision(prec)
    out = capsys.readouterr().out
    assert re.search(r"DEV_SSIM_B: -?\d\.\d{4}, TEST_SSIM_B: -?\d\.\d{4}, TEST_CS_B: ", out) and "TEST_SSIM_A: " in out, out[-2000:]
    a = dict(np.load(os.path.join(experiment["expr"], "res_ssim", "ssim.npz")))
    want = {"n_samples"}
    for split, n in (("dev", None), ("test", 3)):
        for k in EM.SSIM_PAIRS:
            for q in ("ssim", "cs"):
                mean, per = a["%s_%s_%s" % (split, q, k)], a["%s_%s_%s_per_input" % (split, q, k)]
                want |= {"%s_%s_%s" % (split, q, k), "%s_%s_%s_per_input" % (split, q, k)}
                n_in = per.shape[0] if n is None else n
                assert mean.shape == (3,) and per.shape == (n_in, 3) and mean.dtype == np.float64 and per.dtype == np.float64
                assert np.isfinite(mean).all() and np.isfinite(per).all() and np.abs(per).max() <= 1 and np.abs(mean).max() <= 1
                assert np.allclose(per.mean(0), mean, rtol=0, atol=1e-12)
    assert EM.SSIM_PAIRS == ('members_B', 'ens_mean_B', 'fake_A') and set(a) == want and int(a["n_samples"]) == 2


def test_train_driver_with_the_ssim_loss(tmp_path):
    out = run_module("train", "--name", "ssim", "--checkpoints_dir", tmp_path,
                     "--synthetic", "8", "--grid_size", "64", "--batchSize", "4", "--ngf", "8", "--nef", "8", "--ndf", "8", "--nlatent", "4",
                     "--niter", "1", "--niter_decay", "0", "--eval_steps", "1", "--num_multi", "2", "--lambda_ssim_B", "0.1",
                     "--print_freq", "4", "--display_freq", "8", "--seed", "1")
    d = os.path.join(str(tmp_path), "ssim")
    log = open(os.path.join(d, "results.txt")).read()
    lines = [ln for ln in log.splitlines() if re.search(r"\) D_A: ", ln)]          # the loss lines (not the gnorm_D_A ones)
    assert lines and all(re.search(r"P_f_B: \S+ Ssim_A: \d+\.\d{3} Ssim_B: \d+\.\d{3} $", ln) for ln in lines), lines
    assert "lambda_ssim_B: 0.1" in open(os.path.join(d, "opt.txt")).read().splitlines()
    assert re.search(r"Ssim_A: \d+\.\d{3}", out) and re.search(r"Ssim_B: \d+\.\d{3}", out)   # the print line as well
