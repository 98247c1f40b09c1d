"""CPU tests of the averaged weights' host side: the schedule and the fixed point of tests/ema_ref.py, the --ema_decay /
--ema_eval / --ema options, the declarations of the two entry points, and that nothing changes with the averaging off."""
import argparse
import inspect
import os
import pickle

import numpy as np
import pytest
import torch

import abi
import dtgan_amd  # noqa: F401
from dtgan_amd import _lib, networks as N, options as O
import ema_ref as E
from model_cases import parse_train as _parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("decay", [0.5, 0.9, 0.99, 0.999])
def test_schedule_is_the_warm_up_below_the_crossing_and_the_decay_from_it_on(decay):
    d32 = float(np.float32(decay))
    x = E.crossing(decay)
    assert x >= 1 and (decay != 0.5 or x == 8)                     # (1 + 8) / (10 + 8) = 0.5
    for t in range(1, x):
        assert E.decay_at(decay, t) == (1.0 + t) / (10.0 + t) < d32, t
    for t in (x, x + 1, 10 * x, 100000, 2 ** 31 - 1):
        assert E.decay_at(decay, t) == d32, t
    assert E.decay_at(decay, 1) == 2.0 / 11.0
    with pytest.raises(AssertionError):
        E.decay_at(decay, 0)


def test_a_constant_parameter_sequence_is_a_fixed_point():
    p = np.random.RandomState(0).uniform(-1, 1, 257).astype(np.float32)
    for decay in (0.5, 0.999):
        out = E.ema_run([p] * 12, decay, range(1, 13))
        assert len(out) == 12 and all(np.array_equal(e, p.astype(np.float64)) for e in out)
    # and a moving one follows the recurrence: two steps by hand
    q = -p
    e1 = p + (1 - 2.0 / 11.0) * (q.astype(np.float64) - p)
    e2 = e1 + (1 - 3.0 / 12.0) * (p - e1)
    got = E.ema_run([q, p], 0.999, [1, 2], e0=p)
    assert np.array_equal(got[0], e1) and np.array_equal(got[1], e2)
    assert E.bound(3, 1.0) == 24 * 2.0 ** -24


def test_training_options_default_off_and_are_written(tmp_path):
    opt = _parse(tmp_path)
    assert opt.ema_decay == 0.0 and opt.ema_eval == 1
    txt = open(os.path.join(opt.expr_dir, "opt.txt")).read().splitlines()
    assert "ema_decay: 0.0" in txt and "ema_eval: 1" in txt
    opt = _parse(tmp_path, "--ema_decay", "0.999", "--ema_eval", "0")
    assert opt.ema_decay == 0.999 and opt.ema_eval == 0
    saved = pickle.load(open(os.path.join(opt.expr_dir, "opt.pkl"), "rb"))
    assert saved["ema_decay"] == 0.999 and saved["ema_eval"] == 0


@pytest.mark.parametrize("bad", [["--ema_decay", "1"], ["--ema_decay", "1.5"], ["--ema_decay", "-0.1"], ["--ema_decay", "nan"],
                                 ["--ema_eval", "2"]])
def test_training_options_out_of_range_are_parser_errors(tmp_path, bad, capsys):
    with pytest.raises(SystemExit):
        _parse(tmp_path, *bad)
    assert bad[0] in capsys.readouterr().err


def test_evaluator_option(capsys):
    base = ["--chk_path", "x/latest", "--dataroot", "d", "--metric", "mse"]
    assert O.TestOptions().parse(base).ema == 0
    assert O.TestOptions().parse(base + ["--ema", "1"]).ema == 1
    with pytest.raises(SystemExit):
        O.TestOptions().parse(base + ["--ema", "2"])
    assert "--ema" in capsys.readouterr().err


def test_flat_buffers_and_optimiser_are_unchanged_with_the_averaging_off():
    """tests/test_host_logic.py builds these on the CPU: no `ema` buffer unless asked for, the optimiser's state dict as it was"""
    from dtgan_amd.model import FlatNet, FusedAdam
    net = N.define_LAT_D(4, 8)
    f = FlatNet(net)
    assert not hasattr(f, "ema")
    opt = FusedAdam([f], 1e-3, (0.5, 0.999))
    assert opt.ema_decay == 0.0
    sd = opt.state_dict()
    ref = torch.optim.Adam(net.parameters(), lr=1e-3, betas=(0.5, 0.999)).state_dict()
    assert sd["param_groups"][0]["params"] == ref["param_groups"][0]["params"]
    assert set(sd) == {"state", "param_groups"} and set(sd["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq"}
    keys = list(net.state_dict().keys())
    f.p[0] = 2.0
    f.enable_ema()                                              # a copy of p, n floats; the network's state dict keeps its keys
    assert f.ema.shape == f.p.shape and torch.equal(f.ema, f.p) and f.ema.data_ptr() != f.p.data_ptr()
    assert list(net.state_dict().keys()) == keys and set(opt.state_dict()) == {"state", "param_groups"}


def test_options_written_before_the_averaging_existed_mean_off():
    from dtgan_amd import model as M
    stub = argparse.Namespace(opt=argparse.Namespace(lr=1.0))
    M._Base._setup_ema(stub)                                    # returns before it touches a network
    assert M._Base._ema == () and not hasattr(stub, "_ema") and M._Base._ema_active is False
    with pytest.raises(ValueError):
        M._Base._setup_ema(argparse.Namespace(opt=argparse.Namespace(ema_decay=1.0)))
    assert '"ema_decay"' in inspect.getsource(M.StepGraph._key)
    assert M.AugmentedCycleGAN.EMA_NETS == ("netG_A_B", "netG_B_A", "netE_B") and M.StochCycleGAN.EMA_NETS == ("netG_A_B", "netG_B_A")
    for cls in (M.AugmentedCycleGAN, M.StochCycleGAN):
        assert list(inspect.signature(cls.load).parameters) == ["self", "chk_path", "use_ema"]
        assert inspect.signature(cls.load).parameters["use_ema"].default is False


def test_the_entry_points_are_declared_bound_and_documented():
    assert abi.defines()["ACG_EMA_MAX_GROUPS"] == 8 and _lib.EMA_MAX_GROUPS == 8
    for name in ("acg_ema_multi", "acg_swap_multi"):
        assert abi.declarations()[name][0] == "int" and len(abi.header_args(name)) == len(_lib.SIGNATURES[name][1]), name
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read(), name
    assert [f[0] for f in _lib.EmaGroup._fields_] == ["p", "e", "n"]
    import ctypes
    assert ctypes.sizeof(_lib.EmaGroup) == 24
    lib = _lib.load()
    assert lib.acg_ema_multi is not None and lib.acg_swap_multi is not None
