"""GPU tests of `python -m dtgan_amd.test`: every --metric on a tiny .npz dataset and a seeded checkpoint, each in a fresh
child process under its own time limit."""
import os
import re

import numpy as np
import pytest

from eval_cases import checkpoint_model, S, experiment, png_shape as _png_shape, run_test  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def _run(exp, metric, timeout=600):
    out = run_test(exp, metric, "--ubo_steps", "3", "--res_dir", "res_" + metric, timeout=timeout)
    return out, os.path.join(exp["expr"], "res_" + metric)


def test_metric_bpp(experiment):
    out, res = _run(experiment, "bpp")
    assert "training logvar_B on training data..." in out
    assert re.search(r"^UBO: -?\d+\.\d{4}, KLD: -?\d+\.\d{4}, BPP: -?\d+\.\d{4}$", out, re.M)
    iters = re.findall(r"^\[(\d+)\] UBO: -?\d+\.\d{4}, KLD: -?\d+\.\d{4}, BPP: -?\d+\.\d{4}, L1: \d+\.\d{4}$", out, re.M)
    assert iters == ["0", "1", "2"], out[-2000:]                     # one test batch of 5, three iterates, in order
    m = re.search(r"^TEST_BPP_B: (-?\d+\.\d{4}), TIME: (\d+\.\d{4})$", out, re.M)
    assert m and np.isfinite(float(m.group(1)))
    assert _png_shape(os.path.join(res, "test_pred_B_0.png"))[1] == 2 + 3 * (S + 2)


def test_metric_mse_equals_eval_mse_A(experiment):
    from dtgan_amd.dataloader import AlignedIterator, load_numpy_data
    from dtgan_amd.evaluate import eval_mse_A
    out, _ = _run(experiment, "mse")
    m = re.search(r"^DEV_MSE_A: (\d+\.\d{4}), TEST_MSE_A: (\d+\.\d{4})$", out, re.M)
    assert m, out[-2000:]
    with checkpoint_model(experiment) as model:
        _, _, devA, devB, testA, testB = load_numpy_data(experiment["data"], grid_size=S)
        dev = eval_mse_A(AlignedIterator(devA, devB, batch_size=len(devA)), model)
        test = eval_mse_A(AlignedIterator(testA, testB, batch_size=len(testA)), model)
    assert abs(float(m.group(1)) - dev) < 1e-4 and abs(float(m.group(2)) - test) < 1e-4, (m.groups(), dev, test)


def test_metric_visual_writes_every_grid(experiment):
    _, res = _run(experiment, "visual")
    for name, cols in (("cycle", 6), ("multi", 6), ("cycle_B_multi", 7), ("multi_cycle", 9), ("inf", 6)):
        h, w = _png_shape(os.path.join(res, "%s_0.png" % name))       # 6 dev samples: one batch
        assert w == 2 + cols * (S + 2), name


def test_metric_noise_sens(experiment):
    _, res = _run(experiment, "noise_sens")
    r = np.load(os.path.join(res, "noise_sens.npy"))
    assert r.shape == (8, 5) and np.isfinite(r).all() and (r >= 0).all()


def test_metric_mvgauss(experiment):
    out, _ = _run(experiment, "mvgauss")
    m = re.search(r"^MVGauss BPP: (-?\d+\.\d{4})$", out, re.M)
    assert m and np.isfinite(float(m.group(1)))
