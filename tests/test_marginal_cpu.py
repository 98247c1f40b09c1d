"""CPU tests of the marginal loss's definition (tests/marginal_ref.py against float64 torch.sort autograd and against NumPy's
stable argsort), of the new entry points' declarations, of the --lambda_marg_A / --lambda_marg_B options and of the names a
step gives its optional loss scalars."""
import argparse
import os
import pickle

import numpy as np
import pytest
import torch

import abi
import dtgan_amd  # noqa: F401
import marginal_ref as R
from model_cases import parse_train as _parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("acg_field_sort_workspace_bytes", "acg_field_sort", "acg_marginal_loss_workspace_bytes", "acg_marginal_loss_fwd",
           "acg_marginal_loss_bwd")


@pytest.mark.parametrize("H, W, rows_y", [(16, 16, 3), (17, 13, 2), (1, 1, 3), (5, 64, 4)])
def test_the_loss_and_its_gradient_are_autograds_on_tie_free_fields(H, W, rows_y):
    x = R.make_fields("uniform", H, W, rows=3, C=2, seed=1).astype(np.float64)
    y = R.make_fields("uniform", H, W, rows=rows_y, C=2, seed=2).astype(np.float64) * 0.5
    loss, dx, d = R.marginal_loss_and_grad(x, y)
    xt = torch.from_numpy(x).requires_grad_()
    qx = torch.sort(xt.reshape(3, 2, H * W), dim=-1).values.mean(0)
    qy = torch.sort(torch.from_numpy(y).reshape(rows_y, 2, H * W), dim=-1).values.mean(0)
    lt = ((qx - qy) ** 2).mean()
    lt.backward()
    assert loss > 0 and abs(loss - float(lt.detach())) <= 1e-13 * loss
    assert np.allclose(d, (qx - qy).detach().numpy(), rtol=0, atol=1e-15)
    assert np.allclose(dx, xt.grad.numpy(), rtol=1e-13, atol=1e-18)
    assert R.marginal_loss(x, y) == loss


@pytest.mark.parametrize("kind", R.FIELD_KINDS)
def test_the_tie_rule_is_numpys_stable_argsort(kind):
    x = R.make_fields(kind, 17, 13, rows=2, C=2)
    s, rank = R.sort_fields(x)
    assert s.dtype == np.float32 and rank.dtype == np.int32
    for r in range(2):
        for c in range(2):
            f = x[r, c].ravel() + np.float32(0.0)
            order = np.argsort(f, kind="stable")
            assert np.array_equal(s[r, c].view(np.uint32), f[order].view(np.uint32))
            assert np.array_equal(rank[r, c][order], np.arange(f.size))
            assert np.array_equal(np.sort(rank[r, c]), np.arange(f.size))         # a permutation
            ties = f[order][1:] == f[order][:-1]
            assert np.all(order[1:][ties] > order[:-1][ties])                   # equal values keep their pixel order
            assert not np.any(np.signbit(s[r, c][s[r, c] == 0]))                # the two zeros tie and leave as +0.0
    if kind in ("tanh_normal", "masked", "constant", "signed_zeros"):
        assert np.any(s[..., 1:] == s[..., :-1])                                # the kind does make ties


def test_identical_batches_give_exactly_zero():
    for kind in R.FIELD_KINDS:
        x = R.make_fields(kind, 16, 16)
        loss, dx, d = R.marginal_loss_and_grad(x, x)
        assert loss == 0.0 and np.all(dx == 0) and np.all(d == 0)


def test_the_header_declares_the_entries_and_the_binding_matches():
    from dtgan_amd import _lib
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert len(abi.header_args(name)) == len(_lib.SIGNATURES[name][1]), name
        assert name in doc, name
    mk = open(os.path.join(ROOT, "domain-transfer-gan_amd", "csrc", "Makefile")).read()
    assert "marginal.hip" in mk


def test_the_options_default_to_zero_and_are_written(tmp_path):
    opt = _parse(tmp_path)
    assert opt.lambda_marg_A == 0.0 and opt.lambda_marg_B == 0.0
    txt = open(os.path.join(opt.expr_dir, "opt.txt")).read().splitlines()
    assert "lambda_marg_A: 0.0" in txt and "lambda_marg_B: 0.0" in txt
    opt = _parse(tmp_path, "--grid_size", "100", "--lambda_marg_B", "0.25")      # no power of two is asked for
    assert opt.lambda_marg_A == 0.0 and opt.lambda_marg_B == 0.25
    assert "lambda_marg_B: 0.25" in open(os.path.join(opt.expr_dir, "opt.txt")).read().splitlines()
    assert pickle.load(open(os.path.join(opt.expr_dir, "opt.pkl"), "rb"))["lambda_marg_B"] == 0.25


def test_the_parser_refuses_a_negative_weight_and_a_grid_beyond_the_sort(tmp_path, capsys):
    for flag in ("--lambda_marg_A", "--lambda_marg_B"):
        with pytest.raises(SystemExit):
            _parse(tmp_path, flag, "-0.1")
        assert "negative" in capsys.readouterr().err
        with pytest.raises(SystemExit):
            _parse(tmp_path, "--grid_size", "2048", flag, "0.1")
        err = capsys.readouterr().err
        assert "2048" in err and "1024" in err, err
        assert _parse(tmp_path, "--grid_size", "1024", flag, "0.1").grid_size == 1024
    assert _parse(tmp_path, "--grid_size", "2048").grid_size == 2048            # the default weights leave every size alone


def test_options_written_before_the_loss_existed_mean_zero():
    from dtgan_amd import losses
    marg = losses.BY_STEM["marg"]
    old = argparse.Namespace(lambda_A=1.0, lambda_ssim_A=0.0)
    assert marg.weights(old) == (0.0, 0.0) and not marg.on(old)
    new = argparse.Namespace(lambda_marg_A=0.5, lambda_marg_B=0.0)
    assert marg.weights(new) == (0.5, 0.0) and marg.on(new)
    off = argparse.Namespace(opt=old)
    assert losses.add_terms(off, losses.UNPAIRED, None, None, None, None, fake=(None, None), rec=(None, None)) == (None, [], [])
    key = losses.key_options()            # (both weights 0: nothing is touched)  what StepGraph._key takes: test_losses_cpu.py
    assert marg.options() == ["lambda_marg_A", "lambda_marg_B"] and "lambda_marg_A" in key and "lambda_marg_B" in key


def test_the_optional_loss_names_for_every_combination_of_the_two_families():
    from dtgan_amd import losses

    def names(spec, marg):
        return losses.names(argparse.Namespace(lambda_spec_B=float(spec), lambda_marg_A=float(marg)), losses.UNPAIRED)
    assert names(False, False) == []
    assert names(True, False) == ["Spec_A", "Spec_B"]
    assert names(False, True) == ["Marg_A", "Marg_B"]
    assert names(True, True) == ["Spec_A", "Spec_B", "Marg_A", "Marg_B"]
