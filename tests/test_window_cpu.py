"""CPU tests of the native-resolution host side: ops.window_plan against its rule and tests/window_ref.py, the reference
cut and blend against each other, the --native_res / --window_flip / --overlap / --metric translate options, the native
loader with its centre windows, the window tables of the training step, and the declarations of the two entry points."""
import os
import pickle

import numpy as np
import pytest

import abi
import dtgan_amd  # noqa: F401
from dtgan_amd import _lib, dataloader as DL, ops, options as O
import window_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _origins(p):
    return list(p.oy[:p.ny]), list(p.ox[:p.nx])


@pytest.mark.parametrize("S", [8, 12])
def test_plan_covers_every_extent_and_overlap(S):
    for H in range(S, 3 * S + 2):
        for overlap in range(0, S // 2 + 1):
            p = ops.window_plan(H, S, S, overlap)
            oy, ox = _origins(p)
            assert (p.H, p.W, p.S, p.R) == (H, S, S, max(overlap, 1)) and ox == [0], (H, overlap)
            assert oy == R.plan_axis(H, S, overlap), (H, overlap, oy)
            assert oy[0] == 0 and oy[-1] == H - S and all(0 <= o <= H - S for o in oy), (H, overlap, oy)
            assert (len(oy) == 1) == (H == S), (H, overlap, oy)
            # neighbours ascend and share at least `overlap` pixels
            assert all(a < b and a + S - b >= overlap for a, b in zip(oy, oy[1:])), (H, overlap, oy)
            w = R.weight(S, p.R)
            cover, wsum = np.zeros(H, dtype=int), np.zeros(H)
            for o in oy:
                cover[o:o + S] += 1
                wsum[o:o + S] += w
            assert cover.min() >= 1 and wsum.min() > 0, (H, overlap, oy)
    # both axes are planned alike
    p = ops.window_plan(3 * S + 1, 2 * S - 1, S, 2)
    assert _origins(p) == (R.plan_axis(3 * S + 1, S, 2), R.plan_axis(2 * S - 1, S, 2))


def test_plan_of_the_headline_case():
    p = ops.window_plan(321, 321, 256, 64)
    assert _origins(p) == ([0, 65], [0, 65]) and p.R == 64


def test_plan_refusals():
    for bad in [(7, 8, 8, 0), (8, 7, 8, 0), (16, 16, 8, -1), (16, 16, 8, 5), (16, 16, 9, 5)]:
        with pytest.raises(ValueError):
            ops.window_plan(*bad)
    assert ops.window_plan(16, 16, 9, 4).R == 4
    ops.window_plan(8 + 63 * 4, 8, 8, 4)                     # 64 windows along y
    with pytest.raises(ValueError, match="64"):
        ops.window_plan(8 + 64 * 4, 8, 8, 4)                 # 65
    with pytest.raises(ValueError, match="64"):
        ops.window_plan(8, 8 + 64 * 4, 8, 4)


@pytest.mark.parametrize("case", [(8, 8, 8, 2), (9, 13, 8, 0), (9, 13, 8, 4), (21, 30, 8, 3), (40, 17, 16, 8)])
def test_reference_blend_of_reference_windows_returns_the_field(case):
    H, W, S, overlap = case
    p = R.plan(H, W, S, overlap)
    f = np.random.RandomState(H * W).uniform(-1, 1, (2, 3, H, W))
    tiles = R.gather(f, R.plan_table(p, 2), S)
    assert tiles.shape == (2 * len(p["oy"]) * len(p["ox"]), S, S, 4) and np.all(tiles[..., 3] == 0)
    back, cover = R.blend(tiles, p, 2, 3)
    assert np.abs(back - f).max() <= 1e-12               # a convex combination of equal values
    ky, kx = R.single_source(p)
    assert np.array_equal(ky >= 0, cover == 1) and np.array_equal(kx >= 0, cover == 1)


def test_reference_gather_mirrors():
    f = np.arange(2 * 1 * 3 * 4, dtype=np.float32).reshape(2, 1, 3, 4)
    out = R.gather(f, [(1, 1, 2, 0), (1, 1, 2, 1), (1, 1, 2, 2), (1, 1, 2, 3)], 2)
    win = f[1, 0, 1:3, 2:4]
    assert np.array_equal(out[0, :, :, 0], win) and np.array_equal(out[1, :, :, 0], win[:, ::-1])
    assert np.array_equal(out[2, :, :, 0], win[::-1]) and np.array_equal(out[3, :, :, 0], win[::-1, ::-1])


def test_window_table_check():
    ok = ops.check_window_table([(0, 0, 0, 0), (1, 1, 5, 3)], 2, 9, 13, 8)
    assert ok.dtype.is_floating_point is False and tuple(ok.shape) == (2, 4) and ok.tolist() == [[0, 0, 0, 0], [1, 1, 5, 3]]
    for bad in [(2, 0, 0, 0), (-1, 0, 0, 0), (0, 2, 0, 0), (0, -1, 0, 0), (0, 0, 6, 0), (0, 0, -1, 0), (0, 0, 0, 4), (0, 0, 0, -1)]:
        with pytest.raises(ValueError):
            ops.check_window_table([(0, 0, 0, 0), bad], 2, 9, 13, 8)
    with pytest.raises(ValueError):
        ops.check_window_table(np.zeros((0, 4), dtype=np.int32), 2, 9, 13, 8)


def _parse(tmp_path, *extra):
    return O.TrainOptions().parse(argv=["--name", "exp", "--checkpoints_dir", str(tmp_path), "--gpu_ids", "-1"] + list(extra))


def test_training_options(tmp_path, capsys):
    opt = _parse(tmp_path, "--synthetic", "8")
    assert opt.native_res is False and opt.window_flip == 0
    txt = open(os.path.join(opt.expr_dir, "opt.txt")).read().splitlines()
    assert "native_res: False" in txt and "window_flip: 0" in txt
    opt = _parse(tmp_path, "--dataroot", "d", "--native_res", "--window_flip", "1")
    assert opt.native_res is True and opt.window_flip == 1
    saved = pickle.load(open(os.path.join(opt.expr_dir, "opt.pkl"), "rb"))
    assert saved["native_res"] is True and saved["window_flip"] == 1
    for bad, word in [(["--synthetic", "8", "--native_res"], "--native_res"), (["--dataroot", "d", "--window_flip", "1"], "--window_flip"),
                      (["--dataroot", "d", "--native_res", "--window_flip", "2"], "--window_flip")]:
        with pytest.raises(SystemExit):
            _parse(tmp_path, *bad)
        assert word in capsys.readouterr().err


def test_evaluator_options(capsys):
    base = ["--chk_path", "x/latest", "--dataroot", "d", "--metric", "translate"]
    args = O.TestOptions().parse(base)
    assert args.metric == "translate" and args.overlap is None and args.n_samples == 16
    assert O.TestOptions().parse(base + ["--overlap", "0", "--n_samples", "3"]).overlap == 0
    with pytest.raises(SystemExit):
        O.TestOptions().parse(base + ["--overlap", "-1"])
    assert "--overlap" in capsys.readouterr().err
    assert O.check_overlap(None, 256) == 64 and O.check_overlap(None, 16) == 4
    assert [O.check_overlap(v, 16) for v in (0, 4, 8)] == [0, 4, 8]
    for bad in (9, -1):
        with pytest.raises(ValueError, match="--overlap"):
            O.check_overlap(bad, 16)
    from dtgan_amd import test as T                                # the parsed --overlap wins over a saved one, the default too
    saved = {"overlap": 99, "grid_size": 64}
    assert T._merged_options(saved, O.TestOptions().parse(base + ["--overlap", "3"])).overlap == 3
    merged = T._merged_options(saved, args)
    assert merged.overlap is None and merged.grid_size == 64


def test_header_declares_both_entries_and_keeps_the_version():
    for name in ("acg_window_gather", "acg_window_blend"):
        assert abi.declarations()[name][0] == "int" and name in _lib.SIGNATURES
    assert "acg_window_plan" in abi.structs() and abi.defines()["ACG_WINDOW_MAX"] == 64 and _lib.WINDOW_MAX == 64
    import ctypes
    assert ctypes.sizeof(_lib.WindowPlan) == 4 * (6 + 2 * 64)
    mk = open(os.path.join(ROOT, "domain-transfer-gan_amd", "csrc", "Makefile")).read()
    assert "window.hip" in mk


def _dataset(root, hw, n_train=6, n_test=3):
    rs = np.random.RandomState(1)
    for split, n in (("train", n_train), ("test", n_test)):
        for dom in "AB":
            np.savez(os.path.join(str(root), "%s%s.npz" % (split, dom)), data=rs.uniform(0, 3, (n,) + hw + (2,)).astype(np.float32))


def test_native_load_keeps_shapes_and_cuts_centre_windows(tmp_path):
    _dataset(tmp_path, (11, 14))
    full = DL.load_numpy_data(str(tmp_path), grid_size=8, native_res=True, centre_eval=False)
    assert [a.shape for a in full] == [(3, 2, 11, 14)] * 6 and all(a.dtype == np.float32 for a in full)
    cut = DL.load_numpy_data(str(tmp_path), grid_size=8, native_res=True)
    assert [a.shape for a in cut] == [(3, 2, 11, 14)] * 2 + [(3, 2, 8, 8)] * 4
    for a, c in zip(full[2:], cut[2:]):
        assert np.array_equal(c, a[:, :, 1:9, 3:11]) and c.flags["C_CONTIGUOUS"]       # (11 - 8) // 2, (14 - 8) // 2
    assert np.array_equal(full[0], cut[0])
    # the resized load is what it was: squares of grid_size
    assert [a.shape for a in DL.load_numpy_data(str(tmp_path), grid_size=8)] == [(3, 2, 8, 8)] * 6
    # every field spans [-1, 1] before the cut, as without it
    assert np.allclose(full[0].max(axis=(2, 3)), 1) and np.allclose(full[0].min(axis=(2, 3)), -1)
    assert np.array_equal(DL.centre_windows(full[0], 11)[:, :, :, :], full[0][:, :, :, 1:12])
    with pytest.raises(ValueError, match="11 x 14.*12 x 12"):
        DL.load_numpy_data(str(tmp_path), grid_size=12, native_res=True)
    with pytest.raises(ValueError):
        DL.centre_windows(full[0], 12)


def test_window_tables_of_the_training_step():
    np.random.seed(5)
    a, b = DL.window_tables(64, (11, 14), (9, 20), 8, flip=True)
    assert a.shape == b.shape == (64, 4) and a.dtype == b.dtype == np.int32
    for t, (H, W) in ((a, (11, 14)), (b, (9, 20))):
        assert np.array_equal(t[:, 0], np.arange(64))
        assert t[:, 1].min() == 0 and t[:, 1].max() == H - 8 and t[:, 2].min() == 0 and t[:, 2].max() == W - 8
        assert set(t[:, 3]) == {0, 1, 2, 3}
        ops.check_window_table(t, 64, H, W, 8)
    assert not np.array_equal(a[:, 1:], b[:, 1:])           # drawn independently
    np.random.seed(5)
    a2, b2 = DL.window_tables(64, (11, 14), (9, 20), 8, flip=True)
    assert np.array_equal(a, a2) and np.array_equal(b, b2)  # the seed reproduces them
    assert np.all(DL.window_tables(16, (11, 14), (11, 14), 8)[0][:, 3] == 0)
    # the paired step: one draw, the same rows for A and B
    pa, pb = DL.window_tables(64, (11, 14), (11, 14), 8, flip=True, paired=True)
    assert np.array_equal(pa, pb) and pa is not pb and len(set(map(tuple, pa[:, 1:]))) > 8
    with pytest.raises(ValueError):
        DL.window_tables(4, (11, 14), (11, 15), 8, paired=True)
    with pytest.raises(ValueError):
        DL.window_tables(4, (7, 14), (11, 14), 8)
    # a field of exactly the window has one position
    assert np.all(DL.window_tables(8, (8, 8), (8, 8), 8)[0][:, 1:3] == 0)
