"""GPU tests of the CRPS term of the paired step (--lambda_crps_B): eager, captured and deferred, under the forced one-rank
exchange, and `python -m dtgan_amd.train --supervised --lambda_crps_B` in a child process."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import crps_ref as R
from test_hip_ssim_step import S, _flat, _inputs, _model

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BASE = ['S_A', 'S_B', 'KLD_z_B', 'D_z_B']
GNORMS = ['gnorm_G_A_B', 'gnorm_G_B_A', 'gnorm_E_B', 'gnorm_D_z_B']
CRPS = ['S_crps_B', 'S_pair_B']


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
    from dtgan_amd import model as M
    kw = dict(lambda_crps_B=0.5, crps_members=3, crps_alpha=0.95)
    ref, gr, lazy = _model(True, **kw), _model(True, **kw), _model(True, **kw)
    gr.enable_step_graph(); lazy.enable_step_graph(defer_scalars=True)
    g = torch.Generator(device="cuda").manual_seed(11)
    prev = None
    for step in range(4):
        A = torch.rand(4, 3, S, S, device="cuda", generator=g) * 2 - 1
        B = torch.rand(4, 3, S, S, device="cuda", generator=g) * 2 - 1
        z = torch.randn(4, 4, 1, 1, device="cuda", generator=g)
        vr, vg = ref.supervised_train_instance(A, B, z), gr.supervised_train_instance(A, B, z)
        out = lazy.supervised_train_instance(A, B, z)
        assert list(vg.keys()) == BASE + CRPS + GNORMS == list(vr.keys())
        if prev is not None:
            assert prev[0].result() == prev[1]
            prev = None
        if isinstance(out, M.DeferredStep):
            prev = (out, vg)
        else:
            assert step < 2 and out == vg
        if step <= 2:
            assert vg == vr, (step, vg, vr)
        else:
            for k in vr:
                assert abs(vr[k] - vg[k]) <= 2e-3 * max(1.0, abs(vr[k])), (step, k, vr[k], vg[k])
    assert prev is not None and prev[0].result() == prev[1]
    assert gr._sup_step_graph.captures == 1
    for name, value in (("lambda_crps_B", 0.125), ("crps_members", 2), ("crps_alpha", 0.5)):
        before = gr._sup_step_graph.captures
        setattr(gr.opt, name, value)
        v = gr.supervised_train_instance(A, B, z)
        assert gr._sup_step_graph.captures == before + 1 and np.isfinite(v["S_crps_B"]) and np.isfinite(v["S_pair_B"]), name
    gr.opt.lambda_crps_B = 0.0                                                  # off: the eight keys again
    assert list(gr.supervised_train_instance(A, B, z).keys()) == BASE + GNORMS


def _worker(tmp_path, name, **extra_env):
    out = str(tmp_path / (name + ".npz"))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "ACGAN_DIST_FORCE")}
    env.update(extra_env)
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(HERE, "crps_dp_worker.py"), out], env=env,
                       capture_output=True, text=True, timeout=660)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return np.load(out)


def test_the_forced_one_rank_exchange_reports_the_same_scalars(tmp_path):
    """S_crps_B / S_pair_B ride in the rank-averaged sums of the encoder's gradient tail: with one rank and every collective
    forced the paired step's scalars are the plain step's, compared as test_hip_marginal.py compares the unpaired step's: step
    0 but for the tail's float64 average of one value, 1e-6; step 1 follows an Adam update"""
    plain = _worker(tmp_path, "plain")
    forced = _worker(tmp_path, "forced", ACGAN_DIST_FORCE="1", ACGAN_DP_BACKEND="nccl", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1",
                     MASTER_ADDR="127.0.0.1", MASTER_PORT="29577", HSA_ENABLE_IPC_MODE_LEGACY="0")
    assert int(plain["forced"]) == 0 and int(forced["forced"]) == 1
    assert list(plain["s0/names"]) == BASE + CRPS + GNORMS == list(forced["s0/names"])
    print("step 0 largest relative difference %.3e" % np.max(np.abs(forced["s0/values"] - plain["s0/values"]) / np.abs(plain["s0/values"])))
    assert np.allclose(forced["s0/values"], plain["s0/values"], rtol=1e-6, atol=1e-9), (forced["s0/values"], plain["s0/values"])
    assert np.allclose(forced["s1/values"], plain["s1/values"], rtol=3e-3, atol=1e-6), (forced["s1/values"], plain["s1/values"])


def test_train_driver_with_the_crps_term(tmp_path):
    """--sup_frac 0.5: four of the eight synthetic pairs form the paired batch (the default tenth of eight is none)"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "dtgan_amd.train", "--name", "crps", "--checkpoints_dir", str(tmp_path),
           "--synthetic", "8", "--grid_size", "64", "--batchSize", "4", "--supervised", "--lambda_crps_B", "0.1", "--sup_frac", "0.5",
           "--ngf", "8", "--nef", "8", "--ndf", "8", "--nlatent", "4", "--niter", "1", "--niter_decay", "0", "--eval_steps", "1",
           "--num_multi", "2", "--print_freq", "4", "--display_freq", "8", "--seed", "1"]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=660)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-4000:]
    d = os.path.join(str(tmp_path), "crps")
    log = open(os.path.join(d, "results.txt")).read()
    lines = [ln for ln in log.splitlines() if "S_crps_B: " in ln]
    assert lines and all(re.search(r"S_A: \S+ S_B: \S+ KLD_z_B: \S+ D_z_B: \S+ S_crps_B: \d+\.\d{3} S_pair_B: \d+\.\d{3} ", ln) for ln in lines), lines
    assert "lambda_crps_B: 0.1" in open(os.path.join(d, "opt.txt")).read().splitlines()
    assert re.search(r"S_crps_B: \d+\.\d{3}", out) and re.search(r"S_pair_B: \d+\.\d{3}", out)   # the print line as well
