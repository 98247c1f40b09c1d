"""GPU tests of the CRPS term of the paired step (--lambda_crps_B): eager, captured and deferred, under the forced one-rank
exchange, and `python -m dtgan_amd.train --supervised --lambda_crps_B` in a child process."""
import os
import re

import numpy as np
import pytest
import torch

import crps_ref as R
from model_cases import (SUP_GNORMS as GNORMS, SUP_KEYS as BASE, S, check_captured_and_deferred, flat as _flat, forced_pair, run_module,
                         step_inputs as _inputs, step_model as _model)

pytestmark = pytest.mark.gpu

CRPS = ['S_crps_B', 'S_pair_B']
WORKER = dict(lambda_crps_B=0.1, crps_members=3, crps_alpha=0.95)      # the options of the forced-exchange worker


def _spy(monkeypatch):
    from dtgan_amd import ops
    calls = []
    real = ops._crps_call
    monkeypatch.setattr(ops, "_crps_call", lambda *a: (calls.append(a[5]), real(*a))[1])
    return calls


def test_the_default_paired_step_is_todays(monkeypatch):
    calls = _spy(monkeypatch)
    A, B, z = _inputs()
    v = _model(True).supervised_train_instance(A, B, z)
    assert list(v.keys()) == BASE + GNORMS and calls == []
    v = _model(True, lambda_crps_B=0.0, crps_members=3, crps_alpha=0.5).supervised_train_instance(A, B, z)
    assert list(v.keys()) == BASE + GNORMS and calls == []


def test_the_term_reaches_G_A_B_alone_and_reports_the_reference_score(monkeypatch):
    from dtgan_amd import ops
    calls = _spy(monkeypatch)
    A, B, z = _inputs()
    Me, alpha, bs = 3, 0.95, 4
    off, on, before = _model(True), _model(True, lambda_crps_B=0.5, crps_members=Me), _model(True)
    p_on, p_before = _flat(on), _flat(before)
    assert all(torch.equal(p_on[k], p_before[k]) for k in p_on)    # `before`: a copy of the weights taken before the step
    v0, v1 = off.supervised_train_instance(A, B, z), on.supervised_train_instance(A, B, z)
    assert calls == [Me]
    assert list(v0.keys()) == BASE + GNORMS and list(v1.keys()) == BASE + CRPS + GNORMS
    for k in BASE + ['gnorm_G_B_A', 'gnorm_E_B', 'gnorm_D_z_B']:  # neither the encoder nor G_B_A nor D_z_B is on the term's path
        assert v1[k] == v0[k], (k, v1[k], v0[k])
    assert v1['gnorm_G_A_B'] != v0['gnorm_G_A_B']
    for m, v in ((off, v0), (on, v1)):
        for k, flat in zip(GNORMS, (m.f_G_A_B, m.f_G_B_A, m.f_E_B, m.f_D_z_B)):
            want = float(torch.sqrt((flat.gv.double() ** 2).sum()))              # the network's own gradient, clipped to max_gnorm
            assert np.isfinite(v[k]) and want > 0 and abs(min(v[k], 500.0) - want) <= 1e-4 * want, (k, v[k], want)
    p0, p1 = _flat(off), _flat(on)
    for k in p0:
        assert torch.equal(p0[k], p1[k]) == (k != "f_G_A_B"), k
    # the members again, from the weights before the step and the codes prior_z_B[(n + m) % bs]
    with torch.no_grad():
        a = ops.ToNHWC.apply(A, True)
        rep = a.unsqueeze(1).expand(bs, Me, S, S, a.shape[-1]).reshape(bs * Me, S, S, a.shape[-1])
        zz = z.reshape(bs, -1)
        codes = torch.stack([zz[(n + m) % bs] for n in range(bs) for m in range(Me)])
        members = ops.ToNCHW.apply(before.netG_A_B.forward_nhwc(rep, codes), 3).cpu().numpy()
    assert members.shape == (bs * Me, 3, S, S)
    loss, e1, pair = R.parts(members, B.cpu().numpy(), Me, alpha)
    e2 = pair * Me * (Me - 1) / 2
    # the kernel's bound: float32 scalars of double sums that are within T 2^-52 of the reference: one rounding each
    for name, got, want, scale in (("S_crps_B", v1["S_crps_B"], loss, e1 + R.weight(Me, alpha) * e2), ("S_pair_B", v1["S_pair_B"], pair, pair)):
        print("%s: %.9f (reference %.9f, error %.3e, allowed %.3e)" % (name, got, want, abs(got - want), 2.0 ** -23 * scale))
        assert abs(got - want) <= 2.0 ** -23 * scale, (name, got, want)
    assert 0 < v1["S_crps_B"] < e1 and v1["S_pair_B"] > 0          # below the members' mean absolute error: the codes spread them


def test_more_members_than_the_batch_means_the_batch(monkeypatch):
    calls = _spy(monkeypatch)
    A, B, z = _inputs()
    v8 = _model(True, lambda_crps_B=0.5, crps_members=8).supervised_train_instance(A, B, z)
    v4 = _model(True, lambda_crps_B=0.5, crps_members=4).supervised_train_instance(A, B, z)
    assert calls == [4, 4] and v8 == v4 and list(v8.keys()) == BASE + CRPS + GNORMS


def test_a_member_pass_larger_than_one_generator_pass_is_refused_before_a_launch(monkeypatch):
    from dtgan_amd import model as M
    calls = _spy(monkeypatch)
    A, B, z = _inputs()
    m = _model(True, lambda_crps_B=0.5, crps_members=3)
    monkeypatch.setattr(M, "ensemble_chunk", lambda ngf, H, W: 11)              # 4 inputs x 3 members do not fit
    with pytest.raises(ValueError, match="4 inputs x 3 members"):
        m.supervised_train_instance(A, B, z)
    m.opt.crps_members = 17
    with pytest.raises(ValueError, match="crps_members"):
        m.supervised_train_instance(A, B, z)
    assert calls == []


def test_the_names_come_in_order_with_the_ssim_pair():
    A, B, z = _inputs()
    v = _model(True, lambda_ssim_A=0.3, lambda_crps_B=0.5, crps_members=2).supervised_train_instance(A, B, z)
    assert list(v.keys()) == BASE + ['S_ssim_A', 'S_ssim_B'] + CRPS + GNORMS and all(np.isfinite(x) for x in v.values())


def test_captured_and_deferred_paired_steps_with_the_term_on():
    """two eager warm-up calls, the capture and its replay: the first replayed step equals the eager model's bit for bit; the
    deferred scalars are the synchronous graph's; one capture, and a change of each of the three options captures again"""
    check_captured_and_deferred("supervised_train_instance", dict(lambda_crps_B=0.5, crps_members=3, crps_alpha=0.95), BASE + CRPS + GNORMS,
                                (("lambda_crps_B", 0.125), ("crps_members", 2), ("crps_alpha", 0.5)), dict(lambda_crps_B=0.0), BASE + GNORMS)


def test_the_forced_one_rank_exchange_reports_the_same_scalars(tmp_path):
    """S_crps_B / S_pair_B ride in the rank-averaged sums of the encoder's gradient tail: with one rank and every collective
    forced the paired step's scalars are the plain step's, compared as test_hip_marginal.py compares the unpaired step's: step
    0 but for the tail's float64 average of one value, 1e-6; step 1 follows an Adam update"""
    plain, forced = forced_pair(tmp_path, "supervised_train_instance", WORKER, "29577")
    assert list(plain["s0/names"]) == BASE + CRPS + GNORMS == list(forced["s0/names"])
    print("step 0 largest relative difference %.3e" % np.max(np.abs(forced["s0/values"] - plain["s0/values"]) / np.abs(plain["s0/values"])))
    assert np.allclose(forced["s0/values"], plain["s0/values"], rtol=1e-6, atol=1e-9), (forced["s0/values"], plain["s0/values"])
    assert np.allclose(forced["s1/values"], plain["s1/values"], rtol=3e-3, atol=1e-6), (forced["s1/values"], plain["s1/values"])


def test_train_driver_with_the_crps_term(tmp_path):
    """--sup_frac 0.5: four of the eight synthetic pairs form the paired batch (the default tenth of eight is none)"""
    out = run_module("train", "--name", "crps", "--checkpoints_dir", tmp_path,
                     "--synthetic", "8", "--grid_size", "64", "--batchSize", "4", "--supervised", "--lambda_crps_B", "0.1", "--sup_frac", "0.5",
                     "--ngf", "8", "--nef", "8", "--ndf", "8", "--nlatent", "4", "--niter", "1", "--niter_decay", "0", "--eval_steps", "1",
                     "--num_multi", "2", "--print_freq", "4", "--display_freq", "8", "--seed", "1")
    d = os.path.join(str(tmp_path), "crps")
    log = open(os.path.join(d, "results.txt")).read()
    lines = [ln for ln in log.splitlines() if "S_crps_B: " in ln]
    assert lines and all(re.search(r"S_A: \S+ S_B: \S+ KLD_z_B: \S+ D_z_B: \S+ S_crps_B: \d+\.\d{3} S_pair_B: \d+\.\d{3} ", ln) for ln in lines), lines
    assert "lambda_crps_B: 0.1" in open(os.path.join(d, "opt.txt")).read().splitlines()
    assert re.search(r"S_crps_B: \d+\.\d{3}", out) and re.search(r"S_pair_B: \d+\.\d{3}", out)   # the print line as well
