"""GPU tests of the offline evaluator's pieces against fixtures the reference produced (tools/make_goldens.py walks test.py's
algorithms with the reference's own model and helpers, its random draws fixed): train_logvar, the MVGauss baseline and the
noise sensitivity, in f32 and bf16x3 where a generator is involved."""
import argparse

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eval_draws import driver_draws  # noqa: E402
from golden_util import load  # noqa: E402
from model_cases import tiny_model as _model  # noqa: E402


class _FixedNormal(object):
    """torch.Tensor.normal_(mean, std) on a tensor of `shape` writes mean + std * draws[k] for its k-th such call (the
    make_goldens.FixedNormal of the fixture, on the device)"""

    def __init__(self, shape, draws):
        self.shape, self.draws, self.k = tuple(shape), torch.from_numpy(draws).cuda(), 0

    def __enter__(self):
        self.orig = torch.Tensor.normal_
        me = self

        def normal_(t, mean=0., std=1., *a, **kw):
            if tuple(t.shape) != me.shape:
                return me.orig(t, mean, std, *a, **kw)
            t.copy_(me.draws[me.k] * std + mean)
            me.k += 1
            return t
        torch.Tensor.normal_ = normal_
        return self

    def __exit__(self, *a):
        torch.Tensor.normal_ = self.orig


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_train_logvar_matches_reference_golden(prec):
    """test.py:156-196: per-batch (ubo, kld, bpp) and the trained logvar_B.  RMSprop's first step moves every pixel by about
    lr / sqrt(1 - alpha) * sign(g): a pixel whose batch gradient is within rounding of 0 may step the other way, so logvar_B
    is compared pixel for pixel in f32 and by the share of matching pixels under bf16x3."""
    from hip_util import t, precision
    from dtgan_amd import test as T
    from dtgan_amd.dataloader import AlignedIterator
    arr, meta = load("trainlogvar_aug_small_s64")
    N, S, nb = meta["N"], meta["S"], meta["batches"]
    d = driver_draws("trainlogvar", meta["seed"], N, S, meta["opt"]["nlatent"], nb)
    with precision(prec):
        m = _model(**meta["opt"])
        trace = []
        lv = T.train_logvar(AlignedIterator(d["B"], d["B"], batch_size=N), m, dequant_seq=[t(x) for x in d["dequant"]],
                            eps_seq=[t(e) for e in d["eps"]], trace=trace, verbose=False)
    tol = 1e-4 if prec == "f32" else 1e-3
    assert np.allclose(np.array(trace), arr["trace"], rtol=tol), (trace, arr["trace"])
    got, ref = lv.detach().cpu().numpy(), arr["logvar_B"]
    close = np.isclose(got, ref, rtol=0, atol=1e-4 if prec == "f32" else 1e-3)
    if prec == "f32":
        assert close.all(), np.abs(got - ref).max()
    else:
        assert close.mean() > 0.995, close.mean()


def test_mvgauss_baseline_matches_reference_golden():
    """test.py:109-141: mean and variance over three training batches, bpp over three dequantised test batches"""
    from hip_util import t
    from dtgan_amd import test as T
    from dtgan_amd.dataloader import AlignedIterator
    arr, meta = load("mvgauss_s64")
    N, S, nb = meta["N"], meta["S"], meta["batches"]
    d = driver_draws("mvgauss", meta["seed"], N, S, 4, nb)
    mean, var = T.train_MVGauss_B(AlignedIterator(d["B"], d["B"], batch_size=N))
    assert np.allclose(mean.cpu().numpy(), arr["mean"], rtol=1e-5, atol=1e-6)
    assert np.allclose(var.cpu().numpy(), arr["var"], rtol=1e-4, atol=1e-7)
    bpp = T.eval_bpp_MVGauss_B(AlignedIterator(d["B_test"], d["B_test"], batch_size=N), mean, torch.log(var + 1e-5),
                               dequant_seq=[t(x) for x in d["dequant"]])
    assert abs(bpp - float(arr["bpp"])) < 1e-5 * abs(float(arr["bpp"])), (bpp, float(arr["bpp"]))


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_noise_sensitivity_matches_reference_golden(prec, tmp_path):
    """test.py:97-107 through model.generate_noisy_cycle with the perturbation of fake_A fixed: the k-th normal_(0, std / 127.5)
    on fake_A's shape is std / 127.5 times the fixture's k-th standard normal draw, as in the reference's run.  The eight
    levels differ by 1e-5..1e-3 from one another; a wrong noise scale, normaliser or draw order moves them far more."""
    from hip_util import t, precision
    from dtgan_amd import test as T
    arr, meta = load("noisesens_aug_small_s64")
    N, S = meta["N"], meta["S"]
    d = driver_draws("noisesens", meta["seed"], N, S, meta["opt"]["nlatent"])
    with precision(prec):
        m = _model(**meta["opt"])
        with _FixedNormal((N, 3, S, S), d["noise"]) as fx:
            res = T.sensitivity_to_edge_noise(argparse.Namespace(res_dir=str(tmp_path)), m, t(d["B"]))
        assert fx.k == 8
    ref = arr["noise_sens"]
    assert np.array_equal(np.load(str(tmp_path / "noise_sens.npy")), res)
    assert np.allclose(res, ref, rtol=0, atol=1e-5 if prec == "f32" else 5e-5), np.abs(res - ref).max()
    if prec == "f32":    # the noise's own effect, row k minus the noiseless row 0, is pinned too
        assert np.allclose(res[1:] - res[:1], ref[1:] - ref[:1], rtol=0, atol=1e-5)
