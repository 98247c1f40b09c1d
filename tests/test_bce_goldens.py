"""CPU: the --no_lsgan (vanilla GAN) fixtures written by tools/make_goldens.py (make_bce_goldens) from the reference's own
sigmoid-headed networks, and the public criterion semantics that need no GPU.

The fixtures carry kinds of their own ("bce_net", "bce_step"): tests/test_hip_step.py, test_hip_nets.py and
test_oracle_golden.py collect "step" / "net" fixtures and run them against the LSGAN-only oracle.  Every criterion call
of a step fixture recorded its prediction (the sigmoid probabilities the reference's discriminator returned), its target
and its value, so the recorded losses can be re-derived here in float64."""
import numpy as np
import pytest

from golden_util import load, names

BCE_NETS = ["bce_D_A_s64", "bce_D_B_s40", "bce_D_z_B_n4"]
BCE_STEPS = ["bce_step_aug_small_s64", "bce_step_aug_small_s64_1step", "bce_step_aug_small_s64_init",
             "bce_step_stoch_small_s64"]


def bce64(p, t):
    """torch.nn.functional.binary_cross_entropy (mean) in float64: both logarithms clamped at -100"""
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore"):
        lp, lq = np.maximum(np.log(p), -100.0), np.maximum(np.log1p(-p), -100.0)
    return float(np.mean(-(t * lp + (1.0 - t) * lq)))


def test_bce_fixtures_exist_with_kinds_of_their_own():
    assert sorted(names("bce_net")) == sorted(BCE_NETS)
    assert sorted(names("bce_step")) == sorted(BCE_STEPS)
    for name in BCE_NETS + BCE_STEPS:
        _, meta = load(name)
        assert meta["kind"] not in ("step", "net"), name
    for name in BCE_STEPS:
        _, meta = load(name)
        assert meta["opt"]["no_lsgan"] is True and len(meta["loss_keys"]) == (13 if meta["aug"] else 10)
    assert any(load(n)[1]["flavour"] == "init" for n in BCE_STEPS)
    assert any(not load(n)[1]["aug"] for n in BCE_STEPS)
    assert sorted(load(n)[1]["steps"] for n in BCE_STEPS if load(n)[1]["aug"]) == [1, 2, 2]


@pytest.mark.parametrize("name", BCE_NETS)
def test_bce_net_fixture_outputs_are_probabilities(name):
    arr, meta = load(name)
    assert meta["cfg"]["use_sigmoid"] is True
    out = arr["out0"]
    assert out.shape[1] == 1 and np.all(out > 0.0) and np.all(out < 1.0)


@pytest.mark.parametrize("name", BCE_STEPS)
def test_bce_step_losses_are_the_bce_of_the_recorded_predictions(name):
    arr, meta = load(name)
    aug = meta["aug"]
    for st in range(meta["steps"]):
        targets, values = arr["s%d/gan_target" % st], arr["s%d/gan_values" % st]
        assert len(values) == (9 if aug else 6)
        preds = [arr["s%d/gan_pred/%d" % (st, i)] for i in range(len(values))]
        for i, (p, t) in enumerate(zip(preds, targets)):
            assert np.all((p >= 0.0) & (p <= 1.0)), (st, i)
            assert abs(bce64(p, t) - values[i]) <= 1e-5 * abs(values[i]) + 1e-7, (st, i, bce64(p, t), values[i])
        # criterion call order (model.py:139-171 / 423-464): D fake, D true per discriminator, then the generator terms
        expect_t = [0, 1, 0, 1, 0, 1, 1, 1, 1] if aug else [0, 1, 0, 1, 1, 1]
        assert list(targets) == expect_t[:len(values)]
        losses = dict(zip(meta["loss_keys"], arr["s%d/losses" % st]))
        g = [bce64(p, t) for p, t in zip(preds, targets)]
        tol = lambda a, b: abs(a - b) <= 1e-5 * abs(b) + 1e-7  # noqa: E731
        assert tol(0.5 * (g[0] + g[1]), losses["D_A"]) and tol(0.5 * (g[2] + g[3]), losses["D_B"])
        assert tol(g[6 if aug else 4], losses["G_A"]) and tol(g[7 if aug else 5], losses["G_B"])
        if aug:
            assert tol(0.5 * (g[4] + g[5]), losses["D_z_B"])
        # the monitors are means of the discriminator outputs, i.e. of probabilities
        assert tol(float(np.mean(preds[1], dtype=np.float64)), losses["P_t_A"])
        assert tol(float(np.mean(preds[3], dtype=np.float64)), losses["P_t_B"])


def test_criterion_gan_keeps_the_reference_branch_and_bce_is_separate():
    import torch
    import dtgan_amd  # noqa: F401
    from dtgan_amd import model as M
    with pytest.raises(NotImplementedError):
        M.criterion_GAN(torch.full((2, 1), 0.5), True, use_sigmoid=True)
    assert callable(M.criterion_GAN_bce)


def test_sigmoid_is_a_fusable_activation():
    import torch.nn as nn
    import dtgan_amd  # noqa: F401
    from dtgan_amd import _lib, modules
    assert _lib.ACT_SIGMOID == 4
    assert modules._act_of(nn.Sigmoid()) == _lib.ACT_SIGMOID


@pytest.mark.parametrize("name", BCE_STEPS)
def test_bce_step_inputs_regenerate_from_the_recipe(name):
    """the step fixtures store no images of their inputs: oracle.recipe.inputs(seed + step, ...) regenerates the batch the
    reference trained on, pinned by the stored digests; the stored output images cover the first vis_samples[k] samples"""
    from golden_util import digest
    from oracle import recipe
    arr, meta = load(name)
    o = meta["opt"]
    for st in range(meta["steps"]):
        A, B, z = recipe.inputs(meta["seed"] + st, meta["N"], o["input_nc"], o["output_nc"], meta["S"], o["nlatent"])
        assert np.array_equal(digest(A), arr["s%d/real_A_digest" % st])
        assert np.array_equal(digest(B), arr["s%d/real_B_digest" % st])
        assert np.array_equal(z, arr["s%d/prior_z_B" % st])
        for k in ("fake_B", "rec_B", "fake_A", "rec_A"):
            assert arr["s%d/%s" % (st, k)].shape[0] == meta["vis_samples"][st] >= 1
