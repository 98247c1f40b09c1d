"""GPU tests of the table of optional losses (dtgan_amd.losses) in the steps: every family of a step on at once reports its
scalars in the documented order, each family's scalars are those of a step with that family alone, and the step captures.
The grid is the smallest the step tests' model takes (its encoder and D_A end in a 4 x 4 valid convolution behind four
stride-2 stages: 64), the batch 2."""
import numpy as np
import pytest

from model_cases import BASE_KEYS, S, SUP_GNORMS as PAIRED_GNORMS, SUP_KEYS as PAIRED_BASE, step_inputs as _inputs, step_model as _model

pytestmark = pytest.mark.gpu

THR = [[0.0, 0.5], [0.1, 0.6], [-0.1, 0.4]]
UNPAIRED = [("spec", ["Spec_A", "Spec_B"], dict(lambda_spec_A=0.25, lambda_spec_B=0.5)),
            ("marg", ["Marg_A", "Marg_B"], dict(lambda_marg_A=0.5, lambda_marg_B=0.25)),
            ("ssim", ["Ssim_A", "Ssim_B"], dict(lambda_ssim_A=0.25, lambda_ssim_B=0.5))]
PAIRED = [("ssim", ["S_ssim_A", "S_ssim_B"], dict(lambda_ssim_A=0.25, lambda_ssim_B=0.5)),
          ("crps", ["S_crps_B", "S_pair_B"], dict(lambda_crps_B=0.5, crps_members=2)),
          ("fss", ["S_fss_A", "S_fss_B"], dict(lambda_fss_A=0.25, lambda_fss_B=0.5, fss_loss_windows=(3, 9, 17), fss_tau=0.05,
                                               fss_loss_thr_A=THR, fss_loss_thr_B=THR))]


def _check(families, step, graph, losses_of, head, tail):
    """families: (stem, names, options) in the step's order; step: the model's method; losses_of: the scalars of its result"""
    assert S == 64
    A, B, z = _inputs(N=2)
    everything = dict(kv for _, _, kw in families for kv in kw.items())
    both = losses_of(getattr(_model(True, **everything), step)(A, B, z))
    assert list(both.keys()) == head + [n for _, names, _ in families for n in names] + tail
    assert all(np.isfinite(v) for v in both.values())
    for stem, names, kw in families:
        alone = losses_of(getattr(_model(True, **kw), step)(A, B, z))
        assert list(alone.keys()) == head + names + tail
        for n in names:
            print("%s %s: %s alone, %s with the others" % (stem, n, float(alone[n]).hex(), float(both[n]).hex()))
        for n in names:           # formed from the same forward outputs before any generator step, by deterministic kernels
            assert alone[n] == both[n], (stem, n, alone[n], both[n])
    m = _model(True, **everything)
    m.enable_step_graph()
    for call in range(4):        # two eager warm-up calls, the capture with its first replay, one more replay
        v = losses_of(getattr(m, step)(A, B, z))
        assert list(v.keys()) == list(both.keys()) and all(np.isfinite(x) for x in v.values()), call
        if call == 0:
            assert v == both
    assert getattr(m, graph).captures == 1 and getattr(m, graph).calls == 4


def test_the_unpaired_step_with_spec_marg_and_ssim_on():
    _check(UNPAIRED, "train_instance", "_step_graph", lambda out: out[0], BASE_KEYS[True], [])


def test_the_paired_step_with_ssim_crps_and_fss_on():
    _check(PAIRED, "supervised_train_instance", "_sup_step_graph", lambda vals: vals, PAIRED_BASE, PAIRED_GNORMS)
