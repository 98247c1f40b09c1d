"""CPU tests of the structural similarity's definition (tests/ssim_ref.py against float64 torch autograd of a conv2d statement
and against closed forms), of the float32 error the GPU bars are derived from, of the new entry points' declarations, of the
--lambda_ssim_A / --lambda_ssim_B options, of --metric ssim and of the names a step gives its optional loss scalars."""
import argparse
import os
import pickle
import re

import numpy as np
import pytest
import torch

import abi
import dtgan_amd  # noqa: F401
from dtgan_amd import options as O
import ssim_ref as R
from model_cases import parse_train as _parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("acg_ssim_workspace_bytes", "acg_ssim", "acg_ssim_bwd")


def _torch_ssim(x, y, data_range=2.0):
    """the definition stated with conv2d on the full 2-d window -> (S map, cs map), float64 tensors"""
    w = torch.from_numpy(R.window())
    w2 = (w[:, None] * w[None, :])[None, None]
    rows, C, H, W = x.shape
    conv = lambda t: torch.nn.functional.conv2d(t.reshape(rows * C, 1, H, W), w2).reshape(rows, C, H - 10, W - 10)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = conv(x), conv(y)
    vx, vy, cov = conv(x * x) - mx * mx, conv(y * y) - my * my, conv(x * y) - mx * my
    A2, B2 = 2 * cov + c2, vx + vy + c2
    return (2 * mx * my + c1) * A2 / ((mx * mx + my * my + c1) * B2), A2 / B2


@pytest.mark.parametrize("kind, H, W", [("uniform", 21, 21), ("smooth_noise", 43, 37), ("near_flat", 27, 41), ("step", 42, 75),
                                        ("uniform", 11, 11)])
def test_the_reference_and_its_gradient_are_autograds(kind, H, W):
    x, y = (t.astype(np.float64) for t in R.make_pair(kind, H, W, rows=2, C=2, seed=3))
    xt = torch.from_numpy(x).requires_grad_()
    S, cs = _torch_ssim(xt, torch.from_numpy(y))
    lt = 1.0 - S.mean((-2, -1)).mean()
    (lt * 0.25).backward()
    got = R.ssim(x, y)
    assert np.allclose(got[..., 0], S.detach().mean((-2, -1)).numpy(), rtol=0, atol=1e-13)
    assert np.allclose(got[..., 1], cs.detach().mean((-2, -1)).numpy(), rtol=0, atol=1e-13)
    loss, grad = R.ssim_loss_and_grad(x, y, g=0.25)
    assert abs(loss - float(lt.detach())) <= 1e-13 and loss == R.ssim_loss(x, y)
    err = np.abs(grad - xt.grad.numpy()).max() / np.abs(xt.grad.numpy()).max()
    print("%s %dx%d: gradient against autograd, relative error %.3e" % (kind, H, W, err))
    assert err <= 1e-12


def test_identities():
    x, y = R.make_pair("smooth_noise", 27, 41, rows=2, C=2)
    same = R.ssim(x, x)
    assert np.allclose(same, 1.0, rtol=0, atol=1e-12)                            # SSIM(x, x) = 1 and cs = 1
    assert np.allclose(R.ssim(x, y), R.ssim(y, x), rtol=0, atol=1e-14)            # symmetric in (x, y)
    c1 = (0.01 * 2.0) ** 2
    for a, b in ((0.5, -0.25), (0.9, 0.9), (-1.0, 1.0), (0.0, 0.3)):              # constant fields: no variance, cs = 1
        got = R.ssim(np.full((1, 1, 13, 15), a), np.full((1, 1, 13, 15), b))
        assert np.allclose(got[..., 0], (2 * a * b + c1) / (a * a + b * b + c1), rtol=0, atol=1e-12), (a, b, got)
        assert np.allclose(got[..., 1], 1.0, rtol=0, atol=1e-9)
    for L in (1.0, 2.0, 255.0):                                                   # one window: the direct 121-term sums
        x, y = (t.astype(np.float64) for t in R.make_pair("uniform", 11, 11, rows=1, C=1, seed=5))
        w = R.window()
        w2 = w[:, None] * w[None, :]
        assert abs(w2.sum() - 1.0) < 1e-15 and np.array_equal(w, w[::-1])
        mx, my = (w2 * x[0, 0]).sum(), (w2 * y[0, 0]).sum()
        vx, vy, cov = (w2 * x[0, 0] ** 2).sum() - mx * mx, (w2 * y[0, 0] ** 2).sum() - my * my, (w2 * x[0, 0] * y[0, 0]).sum() - mx * my
        k1, k2 = (0.01 * L) ** 2, (0.03 * L) ** 2
        want = ((2 * mx * my + k1) * (2 * cov + k2) / ((mx * mx + my * my + k1) * (vx + vy + k2)), (2 * cov + k2) / (vx + vy + k2))
        got = R.ssim(x, y, data_range=L)
        assert got.shape == (1, 1, 2) and np.allclose(got[0, 0], want, rtol=0, atol=1e-13), (L, got, want)


def test_pairing():
    x, y = R.make_pair("uniform", 17, 19, rows=6, C=2)
    got = R.ssim(x, y[:2], x_per_y=3)
    for r in range(6):
        assert np.array_equal(got[r], R.ssim(x[r:r + 1], y[r // 3:r // 3 + 1])[0])
    with pytest.raises(AssertionError):
        R.ssim(x, y[:4], x_per_y=3)


def test_fp32_bars_over_the_gpu_case_lists():
    """What the GPU tests' tolerances are 4 x of: the same separable formula in NumPy float32 (textbook moments) against
    float64, over exactly ssim_ref.CASES.  The near-flat field off zero and the step are in the list: the bar is honest about the
    cancellation in E[x^2] - mu^2."""
    kinds = {c[0] for c in R.CASES}
    assert {"near_flat", "step"} <= kinds and ("near_flat", 64, 64, 3, 3) in R.CASES
    worst_v, worst_g, table = 0.0, 0.0, {}
    for kind, H, W, rows, C in R.CASES:
        x, y = R.make_pair(kind, H, W, rows, C)
        v32, _, g32 = R.ssim_and_grad(x, y, dtype=np.float32)
        v64, _, g64 = R.ssim_and_grad(x, y)
        ev = float(np.abs(v32 - v64).max())
        eg = R.field_grad_error(g32, g64)
        table[kind] = tuple(max(a, b) for a, b in zip(table.get(kind, (0.0, 0.0)), (ev, eg)))
        worst_v, worst_g = max(worst_v, ev), max(worst_g, eg)
    for kind, (ev, eg) in sorted(table.items()):
        print("%-13s fp32 against fp64: mean S / cs %.3e, gradient (relative to the field's largest) %.3e" % (kind, ev, eg))
    print("worst: value %.4e (ssim_ref.FP32_VALUE_ERR %.4e), gradient %.4e (ssim_ref.FP32_GRAD_ERR %.4e)"
          % (worst_v, R.FP32_VALUE_ERR, worst_g, R.FP32_GRAD_ERR))
    # the recorded numbers are the measured ones (elementwise float32 arithmetic: the same on every host)
    assert worst_v <= R.FP32_VALUE_ERR <= 1.05 * worst_v
    assert worst_g <= R.FP32_GRAD_ERR <= 1.05 * worst_g


def test_scipy_agrees_where_it_is_installed():
    ndimage = pytest.importorskip("scipy.ndimage")
    x, y = (t.astype(np.float64) for t in R.make_pair("smooth_noise", 43, 37, rows=1, C=1))
    w = R.window()
    f = lambda m: ndimage.correlate1d(ndimage.correlate1d(m, w, axis=0, mode="constant"), w, axis=1, mode="constant")[5:-5, 5:-5]
    mx, my = f(x[0, 0]), f(y[0, 0])
    c1, c2 = 0.02 ** 2, 0.06 ** 2
    A2, B2 = 2 * (f(x[0, 0] * y[0, 0]) - mx * my) + c2, f(x[0, 0] ** 2) - mx ** 2 + f(y[0, 0] ** 2) - my ** 2 + c2
    S = (2 * mx * my + c1) * A2 / ((mx ** 2 + my ** 2 + c1) * B2)
    assert np.allclose(R.ssim(x, y)[0, 0], (S.mean(), (A2 / B2).mean()), rtol=0, atol=1e-13)


def test_the_header_declares_the_entries_and_the_binding_matches():
    from dtgan_amd import _lib
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert len(abi.header_args(name)) == len(_lib.SIGNATURES[name][1]), name
        assert name in doc, name
    mk = open(os.path.join(ROOT, "domain-transfer-gan_amd", "csrc", "Makefile")).read()
    assert "ssim.hip" in mk
    src = open(os.path.join(ROOT, "domain-transfer-gan_amd", "csrc", "ssim.hip")).read()
    assert re.search(r"SS_TW = %d, SS_TH = %d\b" % (R.TILE_W, R.TILE_H), src)       # the tile the case lists are built around


def test_the_options_default_to_zero_and_are_written(tmp_path):
    opt = _parse(tmp_path)
    assert opt.lambda_ssim_A == 0.0 and opt.lambda_ssim_B == 0.0
    txt = open(os.path.join(opt.expr_dir, "opt.txt")).read().splitlines()
    assert "lambda_ssim_A: 0.0" in txt and "lambda_ssim_B: 0.0" in txt
    opt = _parse(tmp_path, "--grid_size", "100", "--lambda_ssim_B", "0.25")
    assert opt.lambda_ssim_A == 0.0 and opt.lambda_ssim_B == 0.25
    assert pickle.load(open(os.path.join(opt.expr_dir, "opt.pkl"), "rb"))["lambda_ssim_B"] == 0.25


def test_the_parser_refuses_a_negative_weight_and_a_grid_outside_the_window(tmp_path, capsys):
    for flag in ("--lambda_ssim_A", "--lambda_ssim_B"):
        with pytest.raises(SystemExit):
            _parse(tmp_path, flag, "-0.1")
        assert "negative" in capsys.readouterr().err
        for size in ("8", "2048"):
            with pytest.raises(SystemExit):
                _parse(tmp_path, "--grid_size", size, flag, "0.1")
            err = capsys.readouterr().err
            assert size in err and "1024" in err and "11" in err, err
        assert _parse(tmp_path, "--grid_size", "1024", flag, "0.1").grid_size == 1024
        assert _parse(tmp_path, "--grid_size", "11", flag, "0.1").grid_size == 11
    assert _parse(tmp_path, "--grid_size", "8").grid_size == 8                  # the default weights leave every size alone


def test_the_test_options_accept_the_metric():
    opt = O.TestOptions().parse(["--chk_path", "x/latest", "--dataroot", "d", "--metric", "ssim", "--n_samples", "3", "--ema", "1"])
    assert opt.metric == "ssim" and opt.n_samples == 3 and opt.ema == 1
    with pytest.raises(SystemExit):
        O.TestOptions().parse(["--chk_path", "x/latest", "--dataroot", "d", "--metric", "msssim"])


def test_options_written_before_the_loss_existed_mean_zero():
    from dtgan_amd import losses
    ssim = losses.BY_STEM["ssim"]
    old = argparse.Namespace(lambda_A=1.0, lambda_fss_A=0.0)
    assert ssim.weights(old) == (0.0, 0.0) and not ssim.on(old)
    new = argparse.Namespace(lambda_ssim_A=0.5, lambda_ssim_B=0.0)
    assert ssim.weights(new) == (0.5, 0.0) and ssim.on(new)
    off = argparse.Namespace(opt=old)                                            # both weights 0: nothing is touched, in either step
    assert losses.add_terms(off, losses.UNPAIRED, None, None, None, None, fake=(None, None), rec=(None, None)) == (None, [], [])
    assert losses.add_terms(off, losses.PAIRED, None, None, None, None, pred=(None, None)) == (None, [], [])
    key = losses.key_options()                                                   # what StepGraph._key takes: test_losses_cpu.py
    assert ssim.options() == ["lambda_ssim_A", "lambda_ssim_B"] and "lambda_ssim_A" in key and "lambda_ssim_B" in key


def test_the_optional_loss_names_for_every_combination_of_the_five_families_in_both_steps():
    import itertools
    from dtgan_amd import losses
    unpaired = {"spec": ["Spec_A", "Spec_B"], "marg": ["Marg_A", "Marg_B"], "ssim": ["Ssim_A", "Ssim_B"]}
    paired = {"ssim": ["S_ssim_A", "S_ssim_B"], "crps": ["S_crps_B", "S_pair_B"], "fss": ["S_fss_A", "S_fss_B"]}
    stems = ("spec", "marg", "ssim", "crps", "fss")
    assert tuple(f.stem for f in losses.FAMILIES) == stems
    for on in itertools.product((False, True), repeat=5):
        # one positive weight turns a family on, whichever side it is; the B side, since crps has no other
        opt = argparse.Namespace(**dict(("lambda_%s_B" % s, 0.5) for s, o in zip(stems, on) if o))
        assert losses.names(opt, losses.UNPAIRED) == [n for s, o in zip(stems, on) if o for n in unpaired.get(s, [])], on
        assert losses.names(opt, losses.PAIRED) == [n for s, o in zip(stems, on) if o for n in paired.get(s, [])], on
    assert losses.names(argparse.Namespace(lambda_fss_A=0.5, lambda_spec_A=1.0, lambda_crps_A=1.0), losses.PAIRED) == paired["fss"]
