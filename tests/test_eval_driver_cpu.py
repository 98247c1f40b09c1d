"""CPU tests of the offline evaluator's host side (dtgan_amd.test): parse_opt_file on the files TrainOptions.parse writes,
TestOptions, and the metadata of the evaluator's fixtures."""
import math
import os

import numpy as np
import pytest

import dtgan_amd  # noqa: F401
from dtgan_amd import options as O
from dtgan_amd import eval_metrics as EM, test as T
from golden_util import load


def _train_opt(tmp_path):
    return O.TrainOptions().parse(argv=["--name", "exp", "--checkpoints_dir", str(tmp_path), "--synthetic", "8", "--gpu_ids",
                                         "-1", "--stoch_enc", "--lr", "0.0005", "--niter", "7"])


def test_parse_opt_file_round_trips_opt_txt_and_pkl(tmp_path):
    opt = _train_opt(tmp_path)
    pkl = T.parse_opt_file(os.path.join(opt.expr_dir, "opt.pkl"))
    assert pkl == vars(opt) or pkl == {k: v for k, v in vars(opt).items() if k in pkl}
    txt = T.parse_opt_file(os.path.join(opt.expr_dir, "opt.txt"))
    assert set(txt) == set(pkl)
    # the reference's parse_val rules: None, bools, ints, floats with a '.', strings
    assert txt["seed"] is None and txt["dataroot"] is None
    assert txt["stoch_enc"] is True and txt["no_lsgan"] is False
    assert txt["niter"] == 7 and isinstance(txt["niter"], int)
    assert txt["lr"] == 0.0005 and isinstance(txt["lr"], float)
    assert txt["max_gnorm"] == 500.0 and isinstance(txt["max_gnorm"], float)
    assert txt["model"] == "aug_cycle_gan" and txt["precision"] == "bf16x3"
    for k, v in pkl.items():
        if isinstance(v, (bool, int, float)) or v is None:
            assert txt[k] == v, k


def test_parse_val_rules():
    assert T.parse_val("inf") == float("inf")
    assert T.parse_val("None") is None and T.parse_val("True") is True and T.parse_val("False") is False
    assert T.parse_val("3") == 3 and isinstance(T.parse_val("3"), int)
    assert T.parse_val("1e-3") == 1e-3 and isinstance(T.parse_val("1e-3"), float)
    assert T.parse_val("2.0") == 2.0 and isinstance(T.parse_val("2.0"), float)
    assert T.parse_val("./checkpoints/") == "./checkpoints/"


def test_parse_opt_file_keeps_colons_in_values(tmp_path):
    p = tmp_path / "opt.txt"
    p.write_text("------------ Options -------------\ndataroot: C:/data\nngf: 8\n-------------- End ----------------\n")
    assert T.parse_opt_file(str(p)) == {"dataroot": "C:/data", "ngf": 8}


def test_test_options_defaults_and_new_choices():
    o = O.TestOptions().parse(["--chk_path", "e/latest", "--dataroot", "d", "--metric", "bpp"])
    assert (o.res_dir, o.train_logvar, o.ubo_steps, o.gpu_ids) == ("test_res", 1, 500, "0")
    for metric in ("bpp", "mse", "visual", "noise_sens", "mvgauss"):
        assert O.TestOptions().parse(["--chk_path", "c", "--dataroot", "d", "--metric", metric]).metric == metric
    with pytest.raises(SystemExit):
        O.TestOptions().parse(["--chk_path", "c", "--dataroot", "d", "--metric", "fid"])
    assert O.TestOptions().parse(["--chk_path", "c", "--dataroot", "d", "--metric", "mse", "--ubo_steps", "3"]).ubo_steps == 3


@pytest.mark.parametrize("name,aug,stoch_enc,l1", [("eval_aug_small_s64_stoch_enc", True, True, False),
                                                   ("eval_stoch_small_s64", False, False, False),
                                                   ("eval_aug_small_s64_l1", True, False, True)])
def test_evaluator_fixtures_metadata_and_inputs(name, aug, stoch_enc, l1):
    from oracle import recipe
    arr, meta = load(name)
    assert meta["kind"] == "eval" and meta["aug"] == aug and meta["compute_l1"] == l1
    assert bool(meta["opt"].get("stoch_enc", False)) == stoch_enc
    N, S, steps, nl = meta["N"], meta["S"], meta["steps"], meta["opt"]["nlatent"]
    assert arr["eps"].shape == (steps + 1, N, 1, nl) and arr["dequant"].shape == (N, 3, S, S)
    assert arr["trace"].shape == (steps, 4 if l1 else 3) and np.isfinite(arr["trace"]).all()
    A, B, _ = recipe.inputs(meta["seed"] + 50, N, 3, 3, S, nl)                 # the inputs are regenerated from their seed
    assert np.array_equal(arr["real_A"], A) and np.array_equal(arr["real_B"], B)
    npx = 3 * S * S
    assert np.allclose(arr["trace"][:, 2], arr["trace"][:, 0] / (npx * math.log(2)), rtol=1e-12)
    assert (arr["dequant"] >= 0).all() and (arr["dequant"] <= 1 / 127.5).all()


@pytest.mark.parametrize("name", ["eval_aug_small_s64_stoch_enc", "eval_stoch_small_s64", "eval_aug_small_s64_l1",
                                  "trainlogvar_aug_small_s64", "mvgauss_s64", "noisesens_aug_small_s64"])
def test_evaluator_fixture_digests(name):
    """every recorded array matches its digest, and the draws the driver fixtures were made with are the ones
    tests/eval_draws.py regenerates from the fixture's seed"""
    from eval_draws import driver_draws
    from golden_util import digest
    arr, meta = load(name)
    recorded = [k[len("digest/"):] for k in arr if k.startswith("digest/")]
    assert recorded
    kind = meta["kind"]
    draws = None if kind == "eval" else driver_draws(kind, meta["seed"], meta["N"], meta["S"], meta.get("opt", {}).get("nlatent", 4),
                                                     meta.get("batches", 1))
    for k in recorded:
        src = arr[k] if k in arr else draws[k]
        assert np.array_equal(digest(src), arr["digest/" + k]), k
    if kind == "trainlogvar":
        assert arr["trace"].shape == (meta["batches"], 3) and arr["logvar_B"].shape == (1, 3, meta["S"], meta["S"])
    if kind == "mvgauss":
        assert np.isclose(float(arr["bpp"]), arr["bpp_batches"].mean(), rtol=1e-12)
    if kind == "noisesens":
        assert arr["noise_sens"].shape == (8, meta["N"])


@pytest.mark.parametrize("dtype", ["float32", "int64"])
def test_read_back_returns_every_tensor_with_its_shape(dtype):
    import torch
    g = torch.Generator().manual_seed(11)
    shapes = [(3, 2, 5), (), (7,), (2, 1, 3, 3), (1,)]
    ts = [(torch.randn(s, generator=g) * 100).to(getattr(torch, dtype)) for s in shapes]
    got = EM._read_back(ts)
    assert len(got) == len(ts)
    for a, t in zip(got, ts):
        assert a.shape == tuple(t.shape) and a.dtype == np.dtype(dtype) and np.array_equal(a, t.numpy())
    (only,) = EM._read_back(iter(ts[:1]))                           # any iterable, a single tensor included
    assert np.array_equal(only, ts[0].numpy())


def _plan_opt():
    import argparse
    return argparse.Namespace(output_nc=3, nlatent=4, ngf=8)


def test_plan_ensemble_on_cpu_tensors():
    import torch
    from dtgan_amd.model import ensemble_chunk, plan_ensemble
    opt = _plan_opt()
    A, B = torch.zeros(3, 3, 64, 64), torch.zeros(3, 3, 64, 64)
    M, N, C, H, W, z, per = plan_ensemble("translate_x", opt, A, 4, real_B=B, chunk=9)
    assert (M, N, C, H, W, per) == (4, 3, 3, 64, 64, 9 // 4) and tuple(z.shape) == (N * M, 4, 1, 1)
    assert plan_ensemble("translate_x", opt, A, 4)[-1] == ensemble_chunk(8, 64, 64) // 4      # the default chunk
    given = torch.ones(12, 4, 1, 1)
    assert plan_ensemble("translate_x", opt, A, 4, z=given)[5] is given
    torch.manual_seed(5)                                           # the draw: one normal_ of the whole block of codes
    drawn = plan_ensemble("translate_x", opt, A, 4)[5]
    torch.manual_seed(5)
    assert torch.equal(drawn, A.new_empty((12, 4, 1, 1)).normal_(0, 1))


def test_plan_ensemble_refusals_on_cpu_tensors():
    import torch
    from dtgan_amd import ops
    from dtgan_amd.model import plan_ensemble
    opt = _plan_opt()
    A, B = torch.zeros(2, 3, 64, 64), torch.zeros(2, 3, 64, 64)
    with pytest.raises(ValueError, match=r"^translate_x: n_samples must lie in 1\.\.64 \(got 65\)$"):
        plan_ensemble("translate_x", opt, A, 65)
    with pytest.raises(ValueError, match=r"^translate_x: z holds 3 codes for 2 inputs x 2 samples$"):
        plan_ensemble("translate_x", opt, A, 2, z=torch.zeros(3, 4, 1, 1))
    with pytest.raises(ValueError, match=r"^translate_x: a group of 3 images cannot hold one input's 4 samples$"):
        plan_ensemble("translate_x", opt, A, 4, chunk=3)
    pair = r"^translate_x: real_B \(1, 3, 64, 64\) does not pair with real_A \(2, 3, 64, 64\)$"
    for need_B in (False, True):
        with pytest.raises(ValueError, match=pair):
            plan_ensemble("translate_x", opt, A, 2, real_B=B[:1], need_B=need_B)
    with pytest.raises(ValueError, match="does not pair"):
        plan_ensemble("translate_x", opt, A, 2, real_B=B[0], need_B=True)
    with pytest.raises(ValueError, match="sorted"):               # translate_ensemble's fifth refusal, next to its plan
        ops.check_quantiles((0.9, 0.1))
