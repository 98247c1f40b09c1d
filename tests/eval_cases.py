"""What the evaluator-driver tests share: a tiny .npz split with the checkpoint of a seeded model, the parsed test options, the
`python -m dtgan_amd.test` child process, and two small probes (a PNG's extents, host synchronisations of a call)."""
import argparse
import contextlib
import os
import struct
import subprocess
import sys
import warnings
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 64                  # the grid of the shared experiment: the encoder's 4x4 stride-2 stack needs 64 x 64


def write_dataset(root, hw, n_train, n_test, same=False, seed=0, field=None):
    """{train,test}{A,B}.npz of (n, H, W, 3) fields under root: uniform in [0, 3) from one RandomState(seed), in the order
    train A, train B, test A, test B; `same`: B holds A's data; `field(rs, split index, domain index, n, draw)` replaces a
    draw (draw() gives the uniform one)"""
    os.makedirs(str(root), exist_ok=True)
    rs = np.random.RandomState(seed)
    draw = lambda n: rs.uniform(0, 3, (n,) + tuple(hw) + (3,)).astype(np.float32)
    for i, (split, n) in enumerate((("train", n_train), ("test", n_test))):
        a = None
        for j, dom in enumerate("AB"):
            a = a if same and j else (draw(n) if field is None else field(rs, i, j, n, lambda: draw(n)))
            np.savez(os.path.join(str(root), split + dom + ".npz"), data=a)


def make_experiment(root, S, n_train, n_test, n_blocks=1, hw=None, seed=0, native_res=False, field=None):
    """a synthetic .npz split under root/data (the first half of train becomes dev) and the checkpoint <expr_dir>/latest of a
    seeded tiny model of grid S -> dict(chk, data, expr)"""
    from dtgan_amd import options as O
    from dtgan_amd.model import AugmentedCycleGAN
    data = os.path.join(str(root), "data")
    write_dataset(data, hw or (S, S), n_train, n_test, seed=seed, field=field)
    opt = O.TrainOptions().parse(argv=["--name", "exp", "--checkpoints_dir", str(root), "--dataroot", data, "--grid_size", str(S),
                                       "--ngf", "8", "--nef", "8", "--ndf", "8", "--nlatent", "4", "--n_blocks", str(n_blocks),
                                       "--seed", "3"] + (["--native_res"] if native_res else []))
    torch.manual_seed(3)
    AugmentedCycleGAN(opt).save("latest")
    return dict(chk=os.path.join(opt.expr_dir, "latest"), data=data, expr=opt.expr_dir)


@pytest.fixture(scope="module")
def experiment(tmp_path_factory):
    """a .npz dataset (12 train -> 6 dev + 6 train, 5 test) and checkpoint <expr_dir>/latest of a seeded small model; a test
    module that imports the fixture gets an experiment of its own"""
    return make_experiment(tmp_path_factory.mktemp("eval_driver"), S, 12, 5, n_blocks=2)


SMOOTH_S = 32           # the grid of the excursion-set evaluators' experiment


@pytest.fixture(scope="module")
def smooth_model():
    from model_cases import tiny_model
    return tiny_model(grid_size=SMOOTH_S, n_blocks=1)


@pytest.fixture(scope="module")
def smooth_experiment(tmp_path_factory):
    """a synthetic .npz split (10 train -> 5 dev + 5 train, 3 test) of smoothed noise and the checkpoint <expr_dir>/latest of
    a seeded tiny model"""
    import minkowski_ref as K

    def field(rs, i, j, n, draw):
        f = K.make_fields("smooth", n, 3, SMOOTH_S, SMOOTH_S, np.zeros((3, 1), np.float32), seed=10 * i + j)
        return np.ascontiguousarray(np.moveaxis(f, 1, 3) + 1.5)
    return make_experiment(tmp_path_factory.mktemp("minkowski_metric"), SMOOTH_S, 10, 3, field=field)


def parse_test(metric, *extra):
    from dtgan_amd import options as O
    return O.TestOptions().parse(["--chk_path", "c", "--dataroot", "d", "--metric", metric] + list(extra))


def run_test(exp, metric, *extra, timeout=600):
    """`python -m dtgan_amd.test --metric <metric>` on the experiment in a child process -> its output"""
    cmd = [sys.executable, "-m", "dtgan_amd.test", "--chk_path", exp["chk"], "--dataroot", exp["data"], "--metric", metric]
    p = subprocess.run(cmd + [str(a) for a in extra], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=timeout)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-4000:]
    return out


@contextlib.contextmanager
def checkpoint_model(exp):
    """the experiment's checkpoint loaded in process as dtgan_amd.test builds it, under the precision its options name"""
    from dtgan_amd import ops, test as T
    opt = argparse.Namespace(**T.parse_opt_file(os.path.join(exp["expr"], "opt.pkl")))
    opt.gpu_ids = [0]
    prec = ops.get_precision()
    ops.set_precision(opt.precision)
    try:
        model, _ = T._build(opt)
        model.load(exp["chk"])
        yield model
    finally:
        ops.set_precision(prec)


def png_shape(path):
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


def count_sync_warnings(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message) for w in caught)
