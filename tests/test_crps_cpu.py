"""CPU tests of the CRPS training loss: the numpy reference (tests/crps_ref.py) against tests/ensemble_ref.py and against
closed forms, its analytic gradient against fp64 autograd, ops.crps_weight, the option parser, the header, the binding and
the documents, and the refusals of ops.crps_loss that need no device."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

import abi
import crps_ref as R
import ensemble_ref as E
from model_cases import parse_train as _parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fields(M, N=2, C=2, H=5, W=7, seed=0, grid=None):
    rs = np.random.RandomState(seed + 17 * M)
    x, y = rs.standard_normal((N * M, C, H, W)), rs.standard_normal((N, C, H, W))
    if grid:                                                       # values on a coarse grid: members tie, with y too
        x, y = np.round(x * grid) / grid, np.round(y * grid) / grid
    return x.astype(np.float32), y.astype(np.float32)


@pytest.mark.parametrize("M", (2, 3, 4, 16))
def test_alpha_zero_and_one_are_the_evaluators_crps_and_its_fair_form_per_cell(M):
    x, y = _fields(M)
    st = E.ensemble_stats(x.reshape((2, M) + x.shape[1:]), y, (0.5,))
    assert np.allclose(R.score_map(x, y, M, 0.0), st["crps_map"], rtol=0, atol=1e-14)
    xm = np.moveaxis(x.reshape((2, M) + x.shape[1:]).astype(np.float64), 1, -1)
    e1 = np.abs(xm - y.astype(np.float64)[..., None]).mean(-1)
    fair = e1 - E.e2_pairs(xm) * M / (2.0 * (M - 1))
    assert np.allclose(R.score_map(x, y, M, 1.0), fair, rtol=0, atol=1e-14)
    cells = float(np.prod(y.shape[1:]))
    per_input = R.score_map(x, y, M, 1.0).reshape(2, -1).sum(1) / cells
    assert np.allclose(per_input, st["crps_fair"], rtol=1e-13) and np.allclose(
        R.score_map(x, y, M, 0.0).reshape(2, -1).sum(1) / cells, st["crps"], rtol=1e-13)
    mid = R.loss(x, y, M, 0.95)                                    # between the two, linear in alpha
    assert abs(mid - (0.95 * R.loss(x, y, M, 1.0) + 0.05 * R.loss(x, y, M, 0.0))) <= 1e-14
    s = R.sums(x, y, M)
    assert s.shape == (2, 2, 2) and abs((s[..., 0].sum() - R.weight(M, 0.95) * s[..., 1].sum()) / (2 * cells) - mid) <= 1e-14


def test_one_member_is_the_mean_absolute_error():
    x, y = _fields(1)
    for alpha in (0.0, 0.5, 1.0):
        assert R.weight(1, alpha) == 0.0
        assert R.loss(x, y, 1, alpha) == np.abs(x.astype(np.float64) - y).mean()
        assert np.array_equal(R.grad(x, y, 1, alpha), np.sign(x.astype(np.float64) - y) / x.size)
    assert R.parts(x, y, 1, 0.95)[2] == 0.0 and np.all(R.sums(x, y, 1)[..., 1] == 0.0)


@pytest.mark.parametrize("M", (2, 5))
def test_permuting_the_members_changes_nothing(M):
    x, y = _fields(M, grid=4)
    perm = np.random.RandomState(3).permutation(M)
    xp = x.reshape((2, M) + x.shape[1:])[:, perm].reshape(x.shape)
    assert abs(R.loss(x, y, M, 0.95) - R.loss(xp, y, M, 0.95)) <= 1e-15
    g, gp = R.grad(x, y, M, 0.95), R.grad(xp, y, M, 0.95)
    assert np.array_equal(g.reshape((2, M) + x.shape[1:])[:, perm].reshape(x.shape), gp)   # integer sign sums: exact


@pytest.mark.parametrize("M", (1, 2, 7))
def test_members_on_the_truth_score_zero_with_a_zero_gradient(M):
    _, y = _fields(M)
    x = np.repeat(y, M, axis=0)
    assert R.loss(x, y, M, 0.95) == 0.0 and R.parts(x, y, M, 0.95) == (0.0, 0.0, 0.0)
    assert np.all(R.grad(x, y, M, 0.95) == 0.0)                    # sign(0) = 0


@pytest.mark.parametrize("M,alpha", ((1, 0.95), (2, 1.0), (3, 0.95), (4, 0.0), (16, 0.95)))
def test_the_analytic_gradient_equals_fp64_autograd_of_the_same_expression(M, alpha):
    x, y = _fields(M, grid=2)
    assert np.any(x.reshape((2, M) + x.shape[1:])[:, 0] == y) and (M == 1 or np.any(x[0] == x[1]))   # ties of both kinds
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yt = torch.tensor(y, dtype=torch.float64)
    xm = xt.reshape((2, M) + x.shape[1:])
    e1 = (xm - yt[:, None]).abs().sum(1) / M
    e2 = sum((xm[:, i] - xm[:, j]).abs() for i in range(M) for j in range(i + 1, M)) if M > 1 else 0.0
    loss = (e1 - R.weight(M, alpha) * e2).mean()
    assert abs(loss.item() - R.loss(x, y, M, alpha)) <= 1e-15
    (loss * 0.375).backward()                                      # torch.abs propagates sign(0) = 0
    assert np.allclose(xt.grad.numpy(), R.grad(x, y, M, alpha, 0.375), rtol=1e-13, atol=1e-18)


def test_crps_weight():
    from dtgan_amd import ops
    assert ops.crps_weight(1, 0.3) == 0.0
    for M in (2, 3, 4, 16):
        assert ops.crps_weight(M, 1.0) == 1.0 / (M * (M - 1)) and ops.crps_weight(M, 0.0) == 1.0 / (M * M)
        for alpha in (0.25, 0.95):
            assert ops.crps_weight(M, alpha) == R.weight(M, alpha) == alpha / (M * (M - 1)) + (1 - alpha) / (M * M)
    assert abs(ops.crps_weight(4, 0.95) - (0.95 / 12 + 0.05 / 16)) <= 1e-17
    for bad in ((0, 0.5), (17, 0.5), (2, -0.1), (2, 1.5), (2, float("nan"))):
        with pytest.raises(ValueError):
            ops.crps_weight(*bad)
    assert ops.CRPS_MAX_M == 16 and ops.CRPS_MAX_HW == 1024


def test_the_options_default_to_off_and_are_written(tmp_path):
    opt = _parse(tmp_path)
    assert opt.lambda_crps_B == 0.0 and opt.crps_members == 4 and opt.crps_alpha == 0.95
    assert not hasattr(opt, "lambda_crps_A")
    opt = _parse(tmp_path, "--supervised", "--lambda_crps_B", "0.25", "--crps_members", "16", "--crps_alpha", "1", "--batchSize", "8")
    assert (opt.lambda_crps_B, opt.crps_members, opt.crps_alpha) == (0.25, 16, 1.0)
    assert "lambda_crps_B: 0.25" in open(os.path.join(opt.expr_dir, "opt.txt")).read().splitlines()
    saved = pickle.load(open(os.path.join(opt.expr_dir, "opt.pkl"), "rb"))
    assert saved["lambda_crps_B"] == 0.25 and saved["crps_members"] == 16
    assert _parse(tmp_path, "--supervised", "--lambda_crps_B", "1", "--crps_members", "2", "--crps_alpha", "0").crps_members == 2
    assert _parse(tmp_path, "--supervised", "--lambda_crps_B", "1", "--grid_size", "1024", "--batchSize", "3").grid_size == 1024
    assert _parse(tmp_path, "--grid_size", "2048", "--norm", "batch", "--model", "cycle_gan").lambda_crps_B == 0.0   # off: nothing to refuse
    assert _parse(tmp_path, "--supervised", "--lambda_crps_B", "1", "--batchSize", "63").batchSize == 63      # 252 images fit one pass
    assert _parse(tmp_path, "--batchSize", "64", "--crps_members", "16").crps_members == 16                   # off again


def test_the_parser_refuses_what_the_term_cannot_take(tmp_path, capsys):
    from dtgan_amd import options as O
    on = ("--supervised", "--lambda_crps_B", "0.1")
    for extra, word in ((("--lambda_crps_B", "-0.1"), "negative"), (on + ("--crps_members", "1"), "2..16"),
                        (on + ("--crps_members", "17"), "2..16"), (("--crps_members", "0"), "2..16"),
                        (on + ("--crps_alpha", "-0.01"), "[0, 1]"), (("--crps_alpha", "1.01"), "[0, 1]"),
                        (("--lambda_crps_B", "0.1"), "--supervised"), (on + ("--model", "cycle_gan"), "paired step"),
                        (on + ("--model", "stoch_cycle_gan"), "paired step"), (on + ("--norm", "batch"), "--norm instance"),
                        (on + ("--grid_size", "1025"), "1024"), (on + ("--grid_size", "2048"), "1024"),
                        (on + ("--batchSize", "32", "--crps_members", "8"), "256 images, more than the 255"),
                        (on + ("--batchSize", "64"), "256 images")):
        with pytest.raises(SystemExit):
            _parse(tmp_path, *extra)
        err = capsys.readouterr().err
        assert word in err and "crps" in err, (extra, err)
    p = O.TrainOptions()
    p.initialize()
    text = p.parser.format_help()
    assert "lambda_crps_A" in text and "deterministic" in text     # why there is no B -> A weight


def test_the_header_the_binding_and_the_documents_agree():
    from dtgan_amd import _lib, ops
    for name, nargs in (("acg_crps_workspace_bytes", 5), ("acg_crps_fwd", 17), ("acg_crps_bwd", 19)):
        assert len(abi.header_args(name)) == len(_lib.SIGNATURES[name][1]) == nargs, name
    doubles = [i for i, k in enumerate(abi.header_args("acg_crps_bwd")) if k == "double"]
    assert doubles == [i for i, t in enumerate(_lib.SIGNATURES["acg_crps_bwd"][1]) if t is _lib.ctypes.c_double] == [15, 16]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("`acg_crps_fwd`", "`acg_crps_bwd`", "acg_crps_workspace_bytes", "ops.crps_loss", "--lambda_crps_B"):
        assert word in doc, word
    assert "--lambda_crps_B" in open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 16\. ", design, re.M) and "acg_crps_fwd" in design and "tools/crps_bench.py" in design
    mk = open(os.path.join(ROOT, "domain-transfer-gan_amd", "csrc", "Makefile")).read()
    assert "crps.hip" in mk
    assert "acg_crps_fwd" in ops.crps_loss.__doc__ and "acg_crps_bwd" in ops.CrpsLoss.__doc__
    lib = _lib.load()
    for args, want in (((12, 3, 3, 64, 64), 16 * 4 * 3 * 4), ((16, 16, 1, 1024, 1024), 16 * 1024), ((2, 1, 5, 1, 1), 16 * 2 * 5),
                       ((4, 2, 3, 33, 31), 16 * 2 * 3)):
        assert lib.acg_crps_workspace_bytes(*args) == want, args
    for args in ((0, 1, 1, 8, 8), (3, 2, 1, 8, 8), (2, 1, 0, 8, 8), (2, 1, 1, 8, 1025), (2, 1, 1, 0, 8), (17, 17, 1, 8, 8), (2, 0, 1, 8, 8)):
        assert lib.acg_crps_workspace_bytes(*args) == 0, args


def test_every_host_side_refusal_comes_before_a_device_is_needed(monkeypatch):
    from dtgan_amd import _lib, ops

    def no_device(*a, **k):
        raise AssertionError("a refusal that needs no device reached the library")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(_lib, "query", no_device)
    z = lambda *shape: torch.zeros(shape)
    x, y = z(6, 3, 8, 8), z(2, 3, 8, 8)
    for alpha in (-0.1, 1.1, float("nan")):
        with pytest.raises(_lib.AcgError, match="crps_loss: alpha"):
            ops.crps_loss(x, y, 3, "nchw", "nchw", 3, alpha=alpha)
    for members in (0, 17, 4):                                     # outside 1..16, and not dividing the six rows
        with pytest.raises(_lib.AcgError, match="crps_loss: x_per_y"):
            ops.crps_loss(x if members != 17 else z(34, 3, 8, 8), y, 3, "nchw", "nchw", members)
    with pytest.raises(_lib.AcgError, match="do not pair"):
        ops.crps_loss(x, z(3, 3, 8, 8), 3, "nchw", "nchw", 3)
    with pytest.raises(_lib.AcgError, match="do not pair"):
        ops.crps_loss(x, z(2, 3, 8, 9), 3, "nchw", "nchw", 3)
    with pytest.raises(_lib.AcgError, match="layout"):
        ops.crps_loss(x, y, 3, "chwn", "nchw", 3)
    with pytest.raises(_lib.AcgError, match="layout"):
        ops.crps_loss(x, y, 3, "nchw", "hwc", 3)
    with pytest.raises(_lib.AcgError, match="4-d"):
        ops.crps_loss(z(6, 8, 8), y, 3, "nchw", "nchw", 3)
    with pytest.raises(_lib.AcgError, match="channels"):
        ops.crps_loss(x, y, 4, "nchw", "nchw", 3)
    with pytest.raises(_lib.AcgError, match="channels"):
        ops.crps_loss(z(6, 8, 8, 4), z(2, 8, 8, 4), 0, "nhwc", "nhwc", 3)
    with pytest.raises(_lib.AcgError, match="1024"):
        ops.crps_loss(z(2, 1, 2, 1025), z(2, 1, 2, 1025), 1, "nchw", "nchw", 1)
    with pytest.raises(_lib.AcgError, match="1024"):
        ops.crps_loss(z(2, 1025, 2, 4), z(2, 1025, 2, 4), 1, "nhwc", "nhwc", 1)
    with pytest.raises(_lib.AcgError, match="no CPU path"):       # what is left is _check: the tensors are on the host
        ops.crps_loss(x, y, 3, "nchw", "nchw", 3)
