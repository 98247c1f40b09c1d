"""GPU tests of the spectral training loss: acg_radial_spectrum_bwd against tests/spectrum_grad_ref.py, ops.RadialSpectrum /
ops.spectral_loss against the same, the training step with --lambda_spec_A / --lambda_spec_B (eager, captured, deferred and
under the forced one-rank exchange) and `python -m dtgan_amd.train --lambda_spec_B` in a child process."""
import os
import re

import numpy as np
import pytest
import torch

import spectrum_grad_ref as G
import spectrum_ref as R
from eval_cases import write_dataset
from field_cases import LAYOUTS, field_operand as _device, strides, valid as _valid
from guard_util import Buf
from model_cases import BASE_KEYS, check_captured_and_deferred, flat as _flat, forced_pair, run_module, step_inputs as _inputs, step_model as _model

pytestmark = pytest.mark.gpu

ROWS = 3
# max |gx - ref| / (2 max_b |g[b] / count[b]| rms(x)) per field.  Measured, not chosen: 2 Re ifft2(w fft2(x)) with torch.fft in
# float32 on the CPU needs 8.1906e-7 over every size, field and cotangent below (`python tools/spectrum_bench.py
# --cpu-grad-tolerance`; the largest is the tanh(red) field at S = 1024).  The constant is 4 x that: a different butterfly order.
GRAD_TOL = 4 * 8.1906e-7
# ops.spectral_loss on the batches of spectrum_grad_ref.loss_batches, the same command: the float32 pipeline (ring sums in
# float64) with torch's autograd needs 1.7881e-7 of the value (relative) and 6.404e-7 of the gradient (the measure above, w
# from the reference's cotangent); 4 x each.
LOSS_VALUE_TOL = 4 * 1.7881e-7
LOSS_GRAD_TOL = 4 * 6.404e-7


def _bwd(xd, g, C, layout, ws=None):
    """acg_radial_spectrum_bwd through the C ABI into a NaN-poisoned, guarded buffer -> gx as x is laid out (host)"""
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    S = xd.shape[2]
    rows, Cp = xd.shape[0], (xd.shape[3] if layout == "nhwc" else C)
    st = strides(layout, C, Cp, S, S)
    gd = torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).cuda()
    out = Buf.out(xd.numel())
    need = lib.acg_radial_spectrum_bwd_workspace_bytes(rows, C, S)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda") if ws is None else ws
    rc = lib.acg_radial_spectrum_bwd(ops._ptr(xd), ops._ptr(gd), rows, C, Cp, S, st[0], st[1], st[2], out.ptr, ops._ptr(ws), need,
                                     ops._stream())
    assert rc == 0, lib.acg_last_error().decode()
    return out.host(tuple(xd.shape))


@pytest.mark.parametrize("S", R.FIELD_SIZES)
def test_kernel_matches_reference(S):
    worst = 0.0
    for kind in R.FIELD_KINDS:
        x = R.make_fields(kind, S, rows=ROWS, C=3)
        dev = {(lay, C, Cp): _device(x, lay, C, Cp) for lay, C, Cp in LAYOUTS}
        for ck in G.COTANGENT_KINDS:
            g = G.cotangents(ck, S, (ROWS, 3))
            ref = G.rapsd_vjp(x, g)
            for (lay, C, Cp), xd in dev.items():
                gx = _bwd(xd, g[:, :C], C, lay)
                assert np.all(np.isfinite(gx)), (kind, ck, lay, C, Cp)
                if lay == "nhwc":
                    assert np.all(gx[..., C:] == 0), (kind, ck, C, Cp)         # padded channels: exactly 0, whatever x holds there
                err = G.vjp_error(_valid(gx, lay, C), ref[:, :C], g[:, :C], x[:, :C]).max()
                worst = max(worst, err)
                print("%s %s S=%d %s C=%d Cp=%d: error %.3e (allowed %.3e)" % (kind, ck, S, lay, C, Cp, err, GRAD_TOL))
                assert err <= GRAD_TOL, (kind, ck, S, lay, C, Cp, err)
    Buf.check_all()
    print("S=%d: worst error %.3e (allowed %.3e)" % (S, worst, GRAD_TOL))


@pytest.mark.parametrize("S", R.FIELD_SIZES)
def test_a_zero_cotangent_gives_exactly_zero(S):
    x = R.make_fields("white", S, rows=ROWS, C=3)
    for lay, C, Cp in (("nhwc", 3, 4), ("nchw", 3, 3)):
        gx = _bwd(_device(x, lay, C, Cp), np.zeros((ROWS, C, S // 2 + 1), np.float32), C, lay)
        assert np.all(gx == 0), (S, lay)
    Buf.check_all()


@pytest.mark.parametrize("S", R.FIELD_SIZES)
def test_repeatable_and_the_same_bits_in_both_layouts(S):
    x = R.make_fields("tanh_red", S, rows=ROWS, C=3)
    g = G.cotangents("normal", S, (ROWS, 3))
    nhwc = _device(x, "nhwc", 3, 4)
    a, b = _valid(_bwd(nhwc, g, 3, "nhwc"), "nhwc", 3), _valid(_bwd(nhwc, g, 3, "nhwc"), "nhwc", 3)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    c = _bwd(_device(x, "nchw", 3, 3), g, 3, "nchw")
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
    wide = _valid(_bwd(_device(x, "nhwc", 3, 16, seed=1), g, 3, "nhwc"), "nhwc", 3)
    assert np.array_equal(a.view(np.uint32), wide.view(np.uint32))
    Buf.check_all()


@pytest.mark.parametrize("S", R.FIELD_SIZES)
def test_the_path_a_size_takes(S):
    from dtgan_amd import _lib
    x = R.make_fields("white", S, rows=1, C=1)
    _bwd(_device(x, "nchw", 1, 1), G.cotangents("normal", S, (1, 1)), 1, "nchw")
    k = _lib.query("acg_last_kernel").decode()
    want = "spectrum_bwd_field<%d>" % S if S <= 128 else "spectrum_rows<%d> + spectrum_bwd_cols<%d> + spectrum_bwd_rows<%d>" % (S, S, S)
    assert k == want, k
    head = (4 * (S // 2 + 1) + 15) // 16 * 16                       # the ring counts
    half = 0 if S <= 128 else ROWS * 3 * S * (S // 2) * 8
    assert _lib.query("acg_radial_spectrum_bwd_workspace_bytes", ROWS, 3, S) == head + half
    assert half == _lib.query("acg_radial_spectrum_workspace_bytes", ROWS, 3, S)


def test_kernel_refuses_bad_arguments_before_launching():
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    x = torch.zeros(1 << 16, device="cuda")
    g = torch.zeros(1 << 11, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    need = lib.acg_radial_spectrum_bwd_workspace_bytes(1, 1, 256)
    assert need == 528 + 256 * 128 * 8 and need <= ws.numel()
    n64 = lib.acg_radial_spectrum_bwd_workspace_bytes(1, 1, 64)
    assert n64 == 144
    out = torch.full((1 << 16,), -7.0, device="cuda")
    P = ops._ptr
    cases = (  # S, C, Cp, row stride, x, g, gx, workspace, bytes, rc, what the message names
        (192, 1, 1, 192 * 192, x, g, out, ws, ws.numel(), -1, "power of two"), (8, 1, 1, 64, x, g, out, ws, ws.numel(), -1, "power of two"),
        (2048, 1, 1, 1 << 22, x, g, out, ws, ws.numel(), -1, "power of two"), (64, 0, 1, 4096, x, g, out, ws, ws.numel(), -1, "C >= 1"),
        (64, 2, 1, 8192, x, g, out, ws, ws.numel(), -1, "stored channels"), (64, 1, 1, 0, x, g, out, ws, ws.numel(), -1, "strides"),
        (64, 1, 1, 4096, None, g, out, ws, ws.numel(), -1, "null"), (64, 1, 1, 4096, x, None, out, ws, ws.numel(), -1, "null"),
        (64, 1, 1, 4096, x, g, None, ws, ws.numel(), -1, "null"), (64, 1, 1, 4096, x, g, x, ws, ws.numel(), -1, "alias"),
        (256, 1, 1, 65536, x, g, out, ws, need - 1, -2, "workspace"), (64, 1, 1, 4096, x, g, out, ws, n64 - 1, -2, "workspace"),
        (64, 1, 1, 4096, x, g, out, None, 0, -2, "workspace"))
    for S, C, Cp, rs, xa, ga, oa, wa, nbytes, rc_want, word in cases:
        rc = lib.acg_radial_spectrum_bwd(P(xa), P(ga), 1, C, Cp, S, rs, 1, S * S, P(oa), P(wa), nbytes, ops._stream())
        msg = lib.acg_last_error().decode()
        assert rc == rc_want and msg.startswith("acg_radial_spectrum_bwd") and word in msg, (S, C, Cp, rc, msg)
        if word == "power of two":
            assert str(S) in msg, msg
        torch.cuda.synchronize()
        assert torch.all(out == -7.0) and torch.all(x == 0)          # nothing was written
    assert lib.acg_radial_spectrum_bwd_workspace_bytes(1, 1, 192) == 0
    for shape in ((1, 1, 192, 192), (1, 1, 64, 32), (1, 1, 8, 8)):
        with pytest.raises(_lib.AcgError, match="power of two"):
            ops.radial_spectrum(torch.zeros(shape, device="cuda", requires_grad=True), 1, "nchw")
        with pytest.raises(_lib.AcgError, match="power of two"):
            ops.spectral_loss(torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda"), 1, "nchw")
    with pytest.raises(_lib.AcgError, match="cotangent"):
        ops.radial_spectrum_bwd(torch.zeros(1, 1, 64, 64, device="cuda"), torch.zeros(1, 1, 32, device="cuda"), 1, "nchw")


# ---------------------------------------------------------------------------------------------------------------- ops
def test_radial_spectrum_is_differentiable_and_keeps_its_bits():
    from dtgan_amd import ops
    S = 128
    x = R.make_fields("tanh_red", S, rows=2, C=3)
    g = G.cotangents("normal", S, (2, 3))
    for lay, C, Cp in (("nhwc", 3, 4), ("nchw", 3, 3)):
        xd = _device(x, lay, C, Cp)
        plain = ops.radial_spectrum(xd, C, lay)
        assert not plain.requires_grad
        xg = xd.clone().requires_grad_()
        psd = ops.radial_spectrum(xg, C, lay)
        assert psd.requires_grad and torch.equal(psd.detach(), plain)           # the same launch, the same bits
        with torch.no_grad():
            assert not ops.radial_spectrum(xg, C, lay).requires_grad
        out = torch.empty_like(plain)
        assert ops.radial_spectrum(xg, C, lay, out=out) is out and not out.requires_grad and torch.equal(out, plain)
        (psd * torch.from_numpy(g).cuda()).sum().backward()
        gx = xg.grad.cpu().numpy()
        assert gx.shape == tuple(xd.shape)
        err = G.vjp_error(_valid(gx, lay, C), G.rapsd_vjp(x, g), g, x).max()
        assert err <= GRAD_TOL, (lay, err)
        if lay == "nhwc":
            assert np.all(gx[..., C:] == 0)


def _loss_on_device(x, y, lay, Cp):
    from dtgan_amd import ops
    C = x.shape[1]
    xd = _device(x, lay, C, Cp).requires_grad_()
    loss = ops.spectral_loss(xd, _device(y, lay, C, Cp, seed=4), C, lay)
    assert loss.shape == () and loss.is_cuda
    loss.backward()
    return float(loss.detach()), _valid(xd.grad.cpu().numpy(), lay, C), xd.grad


@pytest.mark.parametrize("S", G.LOSS_SIZES)
@pytest.mark.parametrize("kind", G.LOSS_KINDS)
def test_spectral_loss_and_its_gradient_match_the_reference(kind, S):
    x, y = G.loss_batches(kind, S)
    ref, dref, g = G.spectral_loss_and_grad(x, y)
    gb = np.broadcast_to(g, (x.shape[0],) + g.shape)
    for lay, Cp in (("nhwc", 4), ("nchw", 3)):
        val, dx, raw = _loss_on_device(x, y, lay, Cp)
        ev, eg = abs(val - ref) / ref, G.vjp_error(dx, dref, gb, x).max()
        print("%s S=%d %s: loss %.6g (reference %.6g, relative error %.3e, allowed %.3e); gradient error %.3e (allowed %.3e)"
              % (kind, S, lay, val, ref, ev, LOSS_VALUE_TOL, eg, LOSS_GRAD_TOL))
        assert ev <= LOSS_VALUE_TOL and eg <= LOSS_GRAD_TOL, (kind, S, lay, ev, eg)
        if lay == "nhwc":
            assert torch.all(raw[..., 3:] == 0)
    from dtgan_amd import ops
    same = _device(x, "nchw", 3, 3)
    assert float(ops.spectral_loss(same, same, 3, "nchw")) == 0.0


# --------------------------------------------------------------------------------------------------------------- step
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("aug", [True, False])
def test_step_reports_the_reference_losses_and_the_term_enters_loss_G_only(aug, prec):
    from hip_util import precision
    with precision(prec):
        A, B, z = _inputs()
        off, on_B, on_A = _model(aug), _model(aug, lambda_spec_B=0.5), _model(aug, lambda_spec_A=0.5, lambda_spec_B=0.0)
        l0, v0, g0 = off.train_instance(A, B, z)
        assert list(l0.keys()) == BASE_KEYS[aug]                                # the default step: today's dict
        for m in (on_B, on_A):
            l, v, gn = m.train_instance(A, B, z)
            assert list(l.keys()) == BASE_KEYS[aug] + ["Spec_A", "Spec_B"] and list(gn.keys()) == list(g0.keys())
            for k in BASE_KEYS[aug]:                                            # the first pass does not see the new term
                assert l[k] == l0[k], (k, l[k], l0[k])
            for k in v0:
                assert torch.equal(v[k], v0[k]), k
            h = {k: t.cpu().numpy() for k, t in v.items()}
            for name, fake, real in (("Spec_A", "fake_A", "real_A"), ("Spec_B", "fake_B", "real_B")):
                ref = G.spectral_loss(h[fake], h[real])
                err = abs(l[name] - ref) / ref
                print("%s %s aug=%d: %.6g (reference %.6g, relative error %.3e, allowed %.3e)" % (name, prec, aug, l[name], ref, err,
                                                                                                 LOSS_VALUE_TOL))
                assert np.isfinite(l[name]) and err <= LOSS_VALUE_TOL, (name, l[name], ref)
        p0, pB, pA = _flat(off), _flat(on_B), _flat(on_A)
        for k in p0:
            if k.startswith("f_D"):                                             # the term enters loss_G only
                assert torch.equal(p0[k], pB[k]) and torch.equal(p0[k], pA[k]), k
        assert not torch.equal(p0["f_G_A_B"], pB["f_G_A_B"])
        assert torch.equal(p0["f_G_B_A"], pB["f_G_B_A"])                        # fake_B does not depend on G_B_A
        assert not torch.equal(p0["f_G_B_A"], pA["f_G_B_A"])


@pytest.mark.parametrize("aug", [True, False])
def test_captured_and_deferred_steps_with_the_loss_on(aug):
    """two eager warm-up calls, the capture and its replay: the first replayed step runs the eager step's kernels on the eager
    step's numbers, so everything it reports equals the eager model's bit for bit (later steps carry the ulp of the device-side
    bias correction, test_hip_step.py); the deferred scalars are the synchronous graph's; a change of either weight re-captures"""
    check_captured_and_deferred("train_instance", dict(lambda_spec_A=0.25, lambda_spec_B=0.5), BASE_KEYS[aug] + ["Spec_A", "Spec_B"],
                                (("lambda_spec_B", 0.125), ("lambda_spec_A", 0.0)), dict(lambda_spec_B=0.0), BASE_KEYS[aug], aug=aug, steps=5)


def test_the_forced_one_rank_exchange_reports_the_same_scalars(tmp_path):
    """Spec_A / Spec_B ride in the rank-averaged sums of the gradient tail: with one rank and every collective forced
    (test_hip_dp.test_rccl_backend_one_rank_group) the step's scalars are the plain step's.  Step 0 is the same arithmetic on
    the same numbers but for the tail's float64 average of one value: 1e-6 (8 ulp of fp32); step 1 follows an Adam update."""
    plain, forced = forced_pair(tmp_path, "train_instance", dict(lambda_spec_A=0.05, lambda_spec_B=0.1), "29571")
    assert list(plain["s0/names"][-2:]) == ["Spec_A", "Spec_B"] and list(forced["s0/names"]) == list(plain["s0/names"])
    print("step 0 largest relative difference %.3e" % np.max(np.abs(forced["s0/losses"] - plain["s0/losses"]) / np.abs(plain["s0/losses"])))
    for k in ("s0/losses", "s0/gnorms"):
        assert np.allclose(forced[k], plain[k], rtol=1e-6, atol=1e-9), (k, forced[k], plain[k])
    for k in ("s1/losses", "s1/gnorms"):
        assert np.allclose(forced[k], plain[k], rtol=3e-3, atol=1e-6), (k, forced[k], plain[k])


# ------------------------------------------------------------------------------------------------------------- driver
def test_train_driver_with_the_spectral_loss_and_the_evaluator_on_its_checkpoint(tmp_path):
    S = 64
    data = tmp_path / "data"
    write_dataset(data, (S, S), 12, 5)
    out = run_module("train", "--name", "spec", "--checkpoints_dir", tmp_path,
                     "--synthetic", "16", "--grid_size", S, "--batchSize", "4", "--ngf", "8", "--nef", "8", "--ndf", "8", "--nlatent", "4",
                     "--niter", "1", "--niter_decay", "0", "--print_freq", "8", "--display_freq", "16", "--save_epoch_freq", "1",
                     "--eval_steps", "2", "--num_multi", "2", "--seed", "1", "--lambda_spec_B", "0.1", limit=900)
    d = os.path.join(str(tmp_path), "spec")
    log = open(os.path.join(d, "results.txt")).read()
    lines = [ln for ln in log.splitlines() if re.search(r"\) D_A: ", ln)]          # the loss lines (not the gnorm_D_A ones)
    assert lines and all(re.search(r"P_f_B: \S+ Spec_A: \d+\.\d{3} Spec_B: \d+\.\d{3} $", ln) for ln in lines), lines
    assert "lambda_spec_B: 0.1" in open(os.path.join(d, "opt.txt")).read().splitlines()
    assert re.search(r"Spec_B: \d+\.\d{3}", out)                               # the print line as well
    out = run_module("test", "--chk_path", os.path.join(d, "latest"), "--dataroot", data, "--metric", "spectrum", "--n_samples", "2",
                     "--res_dir", "res_spectrum")
    assert re.search(r"TEST_LSD_B: \d+\.\d{4}", out), out[-2000:]
    assert os.path.exists(os.path.join(d, "res_spectrum", "spectrum.npz"))
