"""GPU tests of `python -m dtgan_amd.test`: every --metric on a tiny .npz dataset and a seeded checkpoint, each in a fresh
child process under its own time limit."""
import os
import re
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 64                  # the encoder's 4x4 stride-2 stack needs 64 x 64


@pytest.fixture(scope="module")
def experiment(tmp_path_factory):
    """a .npz dataset (12 train -> 6 dev + 6 train, 5 test) and checkpoint <expr_dir>/latest of a seeded small model"""
    from dtgan_amd import options as O
    from dtgan_amd.model import AugmentedCycleGAN
    root = tmp_path_factory.mktemp("eval_driver")
    data = root / "data"
    data.mkdir()
    rs = np.random.RandomState(0)
    for split, n in (("train", 12), ("test", 5)):
        for dom in "AB":
            np.savez(str(data / ("%s%s.npz" % (split, dom))), data=rs.uniform(0, 3, (n, S, S, 3)).astype(np.float32))
    opt = O.TrainOptions().parse(argv=["--name", "exp", "--checkpoints_dir", str(root), "--dataroot", str(data), "--grid_size",
                                       str(S), "--ngf", "8", "--nef", "8", "--ndf", "8", "--nlatent", "4", "--n_blocks", "2",
                                       "--seed", "3"])
    torch.manual_seed(3)
    m = AugmentedCycleGAN(opt)
    m.save("latest")
    return dict(chk=os.path.join(opt.expr_dir, "latest"), data=str(data), expr=opt.expr_dir)


def _run(exp, metric, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "dtgan_amd.test", "--chk_path", exp["chk"], "--dataroot", exp["data"], "--metric", metric,
           "--ubo_steps", "3", "--res_dir", "res_" + metric]
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-4000:]
    return out, os.path.join(exp["expr"], "res_" + metric)


def _png_shape(path):
    """decode a PNG written by train.write_png (8-bit RGB, filter 0 rows) -> (h, w)"""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, h, w = 8, b"", 0, 0
    while pos < len(raw):
        (ln,), tag = struct.unpack(">I", raw[pos:pos + 4]), raw[pos + 4:pos + 8]
        body = raw[pos + 8:pos + 8 + ln]
        if tag == b"IHDR":
            w, h = struct.unpack(">II", body[:8])
        elif tag == b"IDAT":
            idat += body
        pos += 12 + ln
    assert len(zlib.decompress(idat)) == h * (1 + 3 * w)
    return h, w


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
    from dtgan_amd import ops
    from dtgan_amd import test as T
    from dtgan_amd.dataloader import AlignedIterator, load_numpy_data
    from dtgan_amd.evaluate import eval_mse_A
    out, _ = _run(experiment, "mse")
    m = re.search(r"^DEV_MSE_A: (\d+\.\d{4}), TEST_MSE_A: (\d+\.\d{4})$", out, re.M)
    assert m, out[-2000:]
    import argparse
    opt = argparse.Namespace(**T.parse_opt_file(os.path.join(experiment["expr"], "opt.pkl")))
    opt.gpu_ids = [0]
    prec = ops.get_precision()
    ops.set_precision(opt.precision)
    try:
        model, _ = T._build(opt)
        model.load(experiment["chk"])
        _, _, devA, devB, testA, testB = load_numpy_data(experiment["data"], grid_size=S)
        dev = eval_mse_A(AlignedIterator(devA, devB, batch_size=len(devA)), model)
        test = eval_mse_A(AlignedIterator(testA, testB, batch_size=len(testA)), model)
    finally:
        ops.set_precision(prec)
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
