"""GPU tests of the fss term of the paired step (--lambda_fss_A / --lambda_fss_B): eager, captured and deferred, under the
forced one-rank exchange, and `python -m dtgan_amd.train --supervised --lambda_fss_B` in a child process."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

import fss_loss_ref as R
from model_cases import (SUP_GNORMS as GNORMS, SUP_KEYS as BASE, check_captured_and_deferred, flat as _flat, forced_pair, run_module,
                         step_inputs as _inputs, step_model as _model)

pytestmark = pytest.mark.gpu

FSS = ['S_fss_A', 'S_fss_B']
THR = [[0.0, 0.5], [0.1, 0.6], [-0.1, 0.4]]
WINDOWS, TAU = (3, 9, 17), 0.05
ON = dict(fss_loss_windows=WINDOWS, fss_tau=TAU, fss_loss_thr_A=THR, fss_loss_thr_B=THR)
# the options of the forced-exchange worker
WORKER = dict(lambda_fss_A=0.2, lambda_fss_B=0.1, fss_loss_windows=(3, 9), fss_tau=0.05, fss_loss_thr_A=[[0.0, 0.5]] * 3,
              fss_loss_thr_B=[[0.0, 0.5]] * 3)


def _spy(monkeypatch):
    from dtgan_amd import _lib
    calls = []
    real = _lib.call

    def call(name, *a):
        if name.startswith("acg_fss_loss"):
            calls.append(name)
        return real(name, *a)
    monkeypatch.setattr(_lib, "call", call)
    return calls


def test_the_default_paired_step_is_todays(monkeypatch):
    calls = _spy(monkeypatch)
    A, B, z = _inputs()
    v = _model(True).supervised_train_instance(A, B, z)
    assert list(v.keys()) == BASE + GNORMS and calls == []
    v = _model(True, lambda_fss_A=0.0, lambda_fss_B=0.0, **ON).supervised_train_instance(A, B, z)
    assert list(v.keys()) == BASE + GNORMS and calls == []


def test_a_weight_without_thresholds_names_the_options(monkeypatch):
    calls = _spy(monkeypatch)
    A, B, z = _inputs()
    with pytest.raises(ValueError, match="fss_loss_thr_A and fss_loss_thr_B"):
        _model(True, lambda_fss_B=0.5).supervised_train_instance(A, B, z)
    assert calls == []


def test_the_term_on_B_reaches_G_A_B_and_the_encoder_and_reports_the_reference_score(monkeypatch):
    from dtgan_amd import ops
    calls = _spy(monkeypatch)
    A, B, z = _inputs()
    off, on, before = _model(True), _model(True, lambda_fss_B=0.5, **ON), _model(True)
    v0, v1 = off.supervised_train_instance(A, B, z), on.supervised_train_instance(A, B, z)
    # the A side is a monitor without gradient: two forwards, one backward
    assert calls == ["acg_fss_loss_fwd", "acg_fss_loss_fwd", "acg_fss_loss_bwd"]
    assert list(v0.keys()) == BASE + GNORMS and list(v1.keys()) == BASE + FSS + GNORMS
    for k in BASE + ['gnorm_G_B_A', 'gnorm_D_z_B']:                # neither G_B_A nor D_z_B is on the term's path
        assert v1[k] == v0[k], (k, v1[k], v0[k])
    assert v1['gnorm_G_A_B'] != v0['gnorm_G_A_B'] and v1['gnorm_E_B'] != v0['gnorm_E_B']
    p0, p1 = _flat(off), _flat(on)
    for k in p0:
        assert torch.equal(p0[k], p1[k]) == (k not in ("f_G_A_B", "f_E_B")), k
    # the predictions again, from the weights before the step
    with torch.no_grad():
        a, b = ops.ToNHWC.apply(A, True), ops.ToNHWC.apply(B, True)
        pred_B = ops.ToNCHW.apply(before.netG_A_B.forward_nhwc(a, before._encode(a, b)[0]), 3).cpu().numpy()
        pred_A = ops.ToNCHW.apply(before.netG_B_A.forward_nhwc(b), 3).cpu().numpy()
    thr = np.array(THR, dtype=np.float32)
    for name, pred, real in (("S_fss_B", pred_B, B), ("S_fss_A", pred_A, A)):
        want = R.loss(pred, real.cpu().numpy(), thr, WINDOWS, TAU)["loss"]
        allowed = 2.001 * R.FWD_BAR + 2.0 ** -23 * want           # the forward's bar on R, and the scalar's float roundings
        print("%s: %.9f (reference %.9f, error %.3e, allowed %.3e)" % (name, v1[name], want, abs(v1[name] - want), allowed))
        assert abs(v1[name] - want) <= allowed and 0 < v1[name] < 1, (name, v1[name], want)


def test_the_term_on_A_alone_moves_G_B_A_alone(monkeypatch):
    calls = _spy(monkeypatch)
    A, B, z = _inputs()
    off, on = _model(True), _model(True, lambda_fss_A=0.5, **ON)
    v0, v1 = off.supervised_train_instance(A, B, z), on.supervised_train_instance(A, B, z)
    assert calls == ["acg_fss_loss_fwd", "acg_fss_loss_fwd", "acg_fss_loss_bwd"] and list(v1.keys()) == BASE + FSS + GNORMS
    for k in BASE + ['gnorm_G_A_B', 'gnorm_E_B', 'gnorm_D_z_B']:
        assert v1[k] == v0[k], (k, v1[k], v0[k])
    assert v1['gnorm_G_B_A'] != v0['gnorm_G_B_A']
    p0, p1 = _flat(off), _flat(on)
    for k in p0:
        assert torch.equal(p0[k], p1[k]) == (k != "f_G_B_A"), k


def test_the_names_come_in_order_with_the_ssim_and_crps_pairs():
    A, B, z = _inputs()
    v = _model(True, lambda_ssim_A=0.3, lambda_crps_B=0.5, crps_members=2, lambda_fss_A=0.1, lambda_fss_B=0.2,
               **ON).supervised_train_instance(A, B, z)
    assert list(v.keys()) == BASE + ['S_ssim_A', 'S_ssim_B', 'S_crps_B', 'S_pair_B'] + FSS + GNORMS
    assert all(np.isfinite(x) for x in v.values())


def test_captured_and_deferred_paired_steps_with_the_term_on():
    """two eager warm-up calls, the capture and its replay: the first replayed step equals the eager model's bit for bit; the
    deferred scalars are the synchronous graph's; one capture, and a change of each option captures again"""
    check_captured_and_deferred("supervised_train_instance", dict(lambda_fss_A=0.25, lambda_fss_B=0.5, **ON), BASE + FSS + GNORMS,
                                (("lambda_fss_B", 0.125), ("fss_tau", 0.1), ("fss_loss_windows", [3, 5]), ("fss_loss_thr_B", [[0.2, 0.3]] * 3)),
                                dict(lambda_fss_A=0.0, lambda_fss_B=0.0), BASE + GNORMS)


def test_the_forced_one_rank_exchange_reports_the_same_scalars(tmp_path):
    """S_fss_A / S_fss_B ride in the rank-averaged sums of the encoder's gradient tail: with one rank and every collective
    forced the paired step's scalars are the plain step's, compared as test_hip_crps_step.py compares them: step 0 but for
    the tail's float64 average of one value, 1e-6; step 1 follows an Adam update"""
    plain, forced = forced_pair(tmp_path, "supervised_train_instance", WORKER, "29578")
    assert list(plain["s0/names"]) == BASE + FSS + GNORMS == list(forced["s0/names"])
    print("step 0 largest relative difference %.3e" % np.max(np.abs(forced["s0/values"] - plain["s0/values"]) / np.abs(plain["s0/values"])))
    assert np.allclose(forced["s0/values"], plain["s0/values"], rtol=1e-6, atol=1e-9), (forced["s0/values"], plain["s0/values"])
    assert np.allclose(forced["s1/values"], plain["s1/values"], rtol=3e-3, atol=1e-6), (forced["s1/values"], plain["s1/values"])


def test_train_driver_with_the_fss_term(tmp_path):
    """--sup_frac 0.5: four of the eight synthetic pairs form the paired batch (the default tenth of eight is none)"""
    out = run_module("train", "--name", "fss", "--checkpoints_dir", tmp_path,
                     "--synthetic", "8", "--grid_size", "64", "--batchSize", "4", "--supervised", "--lambda_fss_B", "0.5", "--sup_frac", "0.5",
                     "--ngf", "8", "--nef", "8", "--ndf", "8", "--nlatent", "4", "--niter", "1", "--niter_decay", "0", "--eval_steps", "1",
                     "--num_multi", "2", "--print_freq", "4", "--display_freq", "8", "--seed", "1")
    d = os.path.join(str(tmp_path), "fss")
    log = open(os.path.join(d, "results.txt")).read()
    for side in "AB":                                              # U(-1, 1): the 0.9 and 0.99 quantiles, per channel
        m = re.search(r"fss loss thresholds %s \(quantiles \(0\.9, 0\.99\)\): channel 0: (\S+), (\S+); channel 1: " % side, log)
        assert m and 0.7 < float(m.group(1)) < 0.9 and 0.95 < float(m.group(2)) < 1.0, log[:2000]
    lines = [ln for ln in log.splitlines() if "S_fss_B: " in ln]
    assert lines and all(re.search(r"S_A: \S+ S_B: \S+ KLD_z_B: \S+ D_z_B: \S+ S_fss_A: \d+\.\d{3} S_fss_B: \d+\.\d{3} ", ln) for ln in lines), lines
    assert "lambda_fss_B: 0.5" in open(os.path.join(d, "opt.txt")).read().splitlines()
    saved = pickle.load(open(os.path.join(d, "opt.pkl"), "rb"))
    assert np.array(saved["fss_loss_thr_B"]).shape == (3, 2) and np.array(saved["fss_loss_thr_A"]).shape == (3, 2)
    assert re.search(r"S_fss_A: \d+\.\d{3}", out) and re.search(r"S_fss_B: \d+\.\d{3}", out)   # the print line as well
