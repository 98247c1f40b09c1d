"""CPU tests of the spectral loss's definition (tests/spectrum_grad_ref.py against float64 autograd of the definition), of the
two new entry points' declarations and of the --lambda_spec_A / --lambda_spec_B options."""
import argparse
import os
import pickle

import numpy as np
import pytest
import torch

import abi
import dtgan_amd  # noqa: F401
import spectrum_grad_ref as G
import spectrum_ref as R
from model_cases import parse_train as _parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# float64 round-off: the transforms carry ~log2(S^2) roundings of 1.1e-16 relative to the largest term; measured 2e-16 at most
ROUND_OFF = 1e-13


def _torch_rapsd(x):
    """float64 autograd form of the definition: torch.fft.fft2, |F|^2 / S^2, ring means by the reference's bin index"""
    S = x.shape[-1]
    F = torch.fft.fft2(x)
    P = (F.real ** 2 + F.imag ** 2) / float(S * S)
    b = torch.from_numpy(R.bin_index(S).ravel())
    keep = b <= S // 2
    sums = torch.zeros(x.shape[:-2] + (S // 2 + 1,), dtype=torch.float64)
    sums = sums.index_add(-1, b[keep], P.reshape(x.shape[:-2] + (S * S,))[..., keep])
    return sums / torch.from_numpy(R.bin_counts(S)).double()


@pytest.mark.parametrize("S", [16, 32, 64])
def test_the_vjp_is_autograds(S):
    for kind in R.FIELD_KINDS:
        x = R.make_fields(kind, S, rows=2, C=2).astype(np.float64)
        for ck in G.COTANGENT_KINDS:
            g = G.cotangents(ck, S, (2, 2)).astype(np.float64)
            xt = torch.from_numpy(x).requires_grad_()
            psd = _torch_rapsd(xt)
            assert np.allclose(psd.detach().numpy(), R.rapsd(x), rtol=1e-12, atol=1e-14)
            (psd * torch.from_numpy(g)).sum().backward()
            err = G.vjp_error(G.rapsd_vjp(x, g), xt.grad.numpy(), g, x).max()
            assert err <= ROUND_OFF, (S, kind, ck, err)


@pytest.mark.parametrize("S", [16, 32, 64])
def test_the_loss_and_its_gradient_are_autograds(S):
    x = R.make_fields("tanh_red", S, rows=3, C=2).astype(np.float64)
    y = R.make_fields("red", S, rows=4, C=2, seed=1).astype(np.float64)
    loss, dx, g = G.spectral_loss_and_grad(x, y)
    xt = torch.from_numpy(x).requires_grad_()
    p, q = _torch_rapsd(xt).mean(0), _torch_rapsd(torch.from_numpy(y)).mean(0)
    lt = ((torch.log(p[:, 1:] + 1e-6) - torch.log(q[:, 1:] + 1e-6)) ** 2).mean()
    lt.backward()
    assert loss > 0 and abs(loss - float(lt.detach())) <= 1e-12 * loss
    gb = np.broadcast_to(g, (3,) + g.shape)
    assert G.vjp_error(dx, xt.grad.numpy(), gb, x).max() <= ROUND_OFF
    assert np.all(g[:, 0] == 0)                                     # bin 0 takes no part
    assert G.spectral_loss(x, x) == 0.0 and np.all(G.spectral_loss_and_grad(x, x)[1] == 0)


def test_the_vjp_of_a_single_ring_is_the_ring_filtered_field():
    """g = count[b] e_b makes w the ring's indicator: the gradient is twice the field band-passed to that ring"""
    S = 32
    x = R.make_fields("white", S, rows=1, C=1)[0, 0].astype(np.float64)
    total = np.zeros_like(x)
    for b in range(S // 2 + 1):
        g = np.zeros(S // 2 + 1)
        g[b] = R.bin_counts(S)[b]
        total += G.rapsd_vjp(x, g)
    corners = np.fft.ifft2(np.where(R.bin_index(S) > S // 2, np.fft.fft2(x), 0)).real
    assert np.allclose(total, 2 * (x - corners), atol=1e-13)


def test_the_header_declares_the_gradient_entries_and_the_binding_matches():
    from dtgan_amd import _lib
    for name in ("acg_radial_spectrum_bwd_workspace_bytes", "acg_radial_spectrum_bwd"):
        assert len(abi.header_args(name)) == len(_lib.SIGNATURES[name][1]), name
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "acg_radial_spectrum_bwd_workspace_bytes" in doc


def test_the_options_default_to_zero_and_are_written(tmp_path):
    opt = _parse(tmp_path)
    assert opt.lambda_spec_A == 0.0 and opt.lambda_spec_B == 0.0
    txt = open(os.path.join(opt.expr_dir, "opt.txt")).read().splitlines()
    assert "lambda_spec_A: 0.0" in txt and "lambda_spec_B: 0.0" in txt
    opt = _parse(tmp_path, "--grid_size", "64", "--lambda_spec_B", "0.25")
    assert opt.lambda_spec_A == 0.0 and opt.lambda_spec_B == 0.25
    assert "lambda_spec_B: 0.25" in open(os.path.join(opt.expr_dir, "opt.txt")).read().splitlines()
    assert pickle.load(open(os.path.join(opt.expr_dir, "opt.pkl"), "rb"))["lambda_spec_B"] == 0.25


@pytest.mark.parametrize("size", [48, 8, 2048, 100])
def test_a_positive_weight_refuses_an_unsupported_grid_size(tmp_path, size, capsys):
    for flag in ("--lambda_spec_A", "--lambda_spec_B"):
        with pytest.raises(SystemExit):
            _parse(tmp_path, "--grid_size", str(size), flag, "0.1")
        err = capsys.readouterr().err
        assert str(size) in err and "power of two" in err, err
    assert _parse(tmp_path, "--grid_size", str(size)).grid_size == size      # the default weights leave every size alone


def test_options_written_before_the_loss_existed_mean_zero():
    """the model reads both weights with a default: an opt.pkl without them (train.py --continue_train, test.py) builds"""
    from dtgan_amd import losses
    spec = losses.BY_STEM["spec"]
    old = argparse.Namespace(lambda_A=1.0)
    assert spec.weights(old) == (0.0, 0.0) and not spec.on(old)
    new = argparse.Namespace(lambda_spec_A=0.5, lambda_spec_B=0.0)
    assert spec.weights(new) == (0.5, 0.0) and spec.on(new)
    key = losses.key_options()                                                   # what StepGraph._key takes: test_losses_cpu.py
    assert spec.options() == ["lambda_spec_A", "lambda_spec_B"] and "lambda_spec_A" in key and "lambda_spec_B" in key
