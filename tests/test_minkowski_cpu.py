"""CPU tests of the Minkowski functionals: the histogram reference (tests/minkowski_ref.py) against the brute force that
labels components threshold by threshold, closed forms, additivity, ops.minkowski_summary / minkowski_distance, the option
parser, the header and the host-side refusals of ops.minkowski."""
import os

import numpy as np
import pytest
import torch

import abi
import minkowski_ref as K
from eval_cases import parse_test

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vs_brute(x, thr):
    got = K.functionals(K.counts(x, thr))
    for r in range(x.shape[0]):
        for c in range(x.shape[1]):
            want = K.functionals_brute(x[r, c], thr[c])
            for k in want:
                assert np.array_equal(got[k][r, c], want[k]), (k, r, c, got[k][r, c], want[k])


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("H,W", ((1, 1), (1, 7), (5, 1), (9, 13), (33, 65)))
def test_the_reference_equals_the_brute_force(H, W, kind):
    for T, dup in ((1, False), (5, False), (6, True)):
        thr = K.make_thresholds(2, T, seed=T, duplicates=dup)
        _vs_brute(K.make_fields(kind, 2, 2, H, W, thr, seed=3), thr)


def test_the_reference_equals_the_brute_force_at_the_most_thresholds():
    thr = K.make_thresholds(1, 255, seed=1, duplicates=True)
    assert np.any(thr[0, 1:] == thr[0, :-1])
    for kind in ("smooth", "special"):
        x = K.make_fields(kind, 1, 1, 64, 64, thr, seed=5)
        n = K.counts(x, thr)
        assert n.shape == (1, 1, 255, 5) and n.dtype == np.int64
        assert np.all(np.diff(n, axis=2) <= 0)                     # the sets are nested: every count falls with the threshold
        _vs_brute(x, thr)
    assert len(np.unique(K.levels(K.make_fields("smooth", 1, 1, 64, 64, thr, seed=5), thr))) > 100   # the levels are in use


def test_levels_follow_the_event_convention():
    thr = np.array([[0.0, 0.0, 1.0]], dtype=np.float32)            # a repeated threshold
    x = np.array([-np.inf, -1.0, np.nextafter(np.float32(0), np.float32(-1)), 0.0, 0.5, 1.0, 2.0, np.inf, np.nan], dtype=np.float32)
    assert K.levels(x.reshape(1, 1, 1, -1), thr).ravel().tolist() == [0, 0, 0, 2, 2, 3, 3, 3, 0]


@pytest.mark.parametrize("H,W", ((1, 1), (1, 9), (6, 4), (17, 33)))
def test_a_full_and_an_empty_field(H, W):
    thr = np.array([[0.0, 0.5, 2.0]], dtype=np.float32)
    n = K.counts(np.ones((1, 1, H, W), dtype=np.float32), thr)[0, 0]
    assert n[0].tolist() == n[1].tolist() == [H * W, H * (W + 1) + (H + 1) * W, H * (W - 1) + (H - 1) * W, (H + 1) * (W + 1), (H - 1) * (W - 1)]
    assert n[2].tolist() == [0] * 5                                # nothing reaches 2: the empty set
    f = K.functionals(n)
    assert f["area"].tolist() == [H * W, H * W, 0] and f["perimeter"].tolist() == [2 * (H + W), 2 * (H + W), 0]
    assert f["euler4"].tolist() == [1, 1, 0] and f["euler8"].tolist() == [1, 1, 0]
    assert np.all(K.counts(np.full((1, 1, H, W), np.nan, dtype=np.float32), thr) == 0)


def test_a_ring_and_a_checkerboard():
    thr = np.array([[0.5]], dtype=np.float32)
    ring = np.zeros((1, 1, 7, 9), dtype=np.float32)
    ring[0, 0, 1:6, 2:8] = 1
    ring[0, 0, 2:5, 3:7] = 0                                       # a 5 x 6 frame one cell wide around a 3 x 4 hole
    f = K.functionals(K.counts(ring, thr))
    assert f["area"].item() == 30 - 12 and f["perimeter"].item() == 2 * (5 + 6) + 2 * (3 + 4)
    assert f["euler4"].item() == 0 and f["euler8"].item() == 0     # one component, one hole
    H, W = 6, 7
    board = (np.add.outer(np.arange(H), np.arange(W)) % 2 == 0).astype(np.float32).reshape(1, 1, H, W)
    f = K.functionals(K.counts(board, thr))
    black = int(board.sum())
    # 4-connectivity: every black cell is a component of its own and no white cell is enclosed (white is 8-connected)
    assert f["area"].item() == black and f["perimeter"].item() == 4 * black and f["euler4"].item() == black
    # 8-connectivity: the black cells form one component; its holes are the white cells with four black neighbours, the interior ones
    white_inside = int((1 - board[0, 0, 1:-1, 1:-1]).sum())
    assert f["euler8"].item() == 1 - white_inside and f["euler8"].item() != f["euler4"].item()
    want = K.functionals_brute(board[0, 0], thr[0])
    assert all(f[k].item() == want[k][0] for k in want)


def test_the_counts_add_over_fields_and_do_not_mix_channels():
    thr = K.make_thresholds(3, 7, seed=2)
    x = K.make_fields("special", 4, 3, 12, 10, thr, seed=1)
    n = K.counts(x, thr)
    assert np.array_equal(n.sum(0), sum(K.counts(x[r:r + 1], thr)[0] for r in range(4)))
    for c in range(3):
        assert np.array_equal(n[:, c], K.counts(x[:, c:c + 1], thr[c:c + 1])[:, 0])


def test_summary_and_distance():
    from dtgan_amd import ops
    assert ops.MINK_MAX_T == 255 and ops.MINK_MAX_HW == 1024
    thr = K.make_thresholds(2, 6, seed=4)
    rs = np.random.RandomState(0)
    H = W = 32
    noise = rs.standard_normal((8, 2, H, W)).astype(np.float32) * 0.5
    n = K.counts(noise, thr)
    s = ops.minkowski_summary(n.sum(0), 8 * H * W)
    want = K.functionals(n.sum(0))
    assert set(s) == {f + e for f in ("area", "perimeter", "euler4", "euler8") for e in ("", "_density")}
    for k in want:
        assert s[k].dtype == np.float64 and s[k].shape == (2, 6) and np.array_equal(s[k], want[k].astype(np.float64))
        assert np.array_equal(s[k + "_density"], want[k] / float(8 * H * W))
    per_field = ops.minkowski_summary(n, H * W)                    # leading axes pass through
    assert per_field["euler8"].shape == (8, 2, 6)
    d = ops.minkowski_distance(s, s)
    assert set(d) == set(ops.MINK_FUNCTIONALS) and all(v.shape == (2,) and np.all(v == 0) for v in d.values())
    assert ops.minkowski_distance(per_field, per_field)["area"].shape == (8, 2)
    # the per-pixel mean of independent noise fields: smaller excursions, so fewer components at the outer thresholds
    thr1 = np.array([[0.5]], dtype=np.float32)
    mean = noise.mean(0, keepdims=True)[:, :1]
    s_mem = ops.minkowski_summary(K.counts(noise[:, :1], thr1).sum(0), 8 * H * W)
    s_mean = ops.minkowski_summary(K.counts(mean, thr1).sum(0), H * W)
    assert s_mean["euler4_density"][0, 0] < s_mem["euler4_density"][0, 0] and s_mean["area_density"][0, 0] < s_mem["area_density"][0, 0]
    d = ops.minkowski_distance(s_mean, s_mem)
    assert d["area"][0] == abs(s_mean["area_density"][0, 0] - s_mem["area_density"][0, 0]) > 0
    with pytest.raises(ValueError, match="counts"):
        ops.minkowski_summary(np.zeros((2, 3, 4)), 10)
    with pytest.raises(ValueError, match="counts"):
        ops.minkowski_summary(np.zeros((2, 3, 5)), 0)
    with pytest.raises(ValueError, match="densities"):
        ops.minkowski_distance(s, per_field)


def test_check_thresholds():
    from dtgan_amd import ops
    ok = ops.check_thresholds([[0.0, 0.0, 1.0], [-1.0, 2.0, 2.0]], 2)
    assert ok.dtype == np.float32 and ok.shape == (2, 3) and ok.flags["C_CONTIGUOUS"]
    for bad in ([[1.0, 0.0]], [[0.0, np.nan]], [[0.0, np.inf]], [[-np.inf, 0.0]], np.zeros((2, 2)), np.zeros(3), np.zeros((1, 0)), np.zeros((1, 256))):
        with pytest.raises(ValueError, match="thresholds"):
            ops.check_thresholds(bad, 1)
    assert ops.check_thresholds(np.zeros((1, 255)), 1).shape == (1, 255)


def _parse(*extra):
    return parse_test("minkowski", *extra)


def test_the_parser_takes_the_metric_and_its_bins():
    o = _parse()
    assert o.metric == "minkowski" and o.mink_bins == 32 and o.n_samples == 16 and o.ema == 0
    o = _parse("--mink_bins", "256", "--n_samples", "3", "--ema", "1")
    assert o.mink_bins == 256 and o.n_samples == 3 and o.ema == 1
    assert _parse("--mink_bins", "2").mink_bins == 2
    for bad in ("1", "257", "0", "-4", "x", "2.5"):
        with pytest.raises(SystemExit):
            _parse("--mink_bins", bad)
    from dtgan_amd import options as O
    for metric in ("marginal", "fss", "mse"):                      # the others keep parsing
        assert O.TestOptions().parse(["--chk_path", "c", "--dataroot", "d", "--metric", metric]).metric == metric


def test_the_thresholds_of_the_metric_are_the_training_quantiles():
    from dtgan_amd import ops
    from dtgan_amd import eval_metrics as EM, test as T
    train = np.random.RandomState(2).uniform(-1, 1, (5, 2, 8, 8)).astype(np.float32)
    for bins in (2, 32, 256):
        thr = ops.check_thresholds(EM.marginal_edges(train, bins), 2)
        assert thr.shape == (2, bins - 1)
    assert "minkowski" in T.__doc__ and "mink_bins" in T.__doc__ and "eval_minkowski" in dir(EM)


def test_the_header_declares_both_entries_and_the_binding_matches():
    from dtgan_amd import _lib
    for name, nargs in (("acg_minkowski_workspace_bytes", 5), ("acg_minkowski", 14)):
        assert len(abi.header_args(name)) == len(_lib.SIGNATURES[name][1]) == nargs, name
    mk = open(os.path.join(ROOT, "domain-transfer-gan_amd", "csrc", "Makefile")).read()
    assert "minkowski.hip" in mk
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`acg_minkowski`" in doc and "acg_minkowski_workspace_bytes" in doc and "ops.minkowski_summary" in doc
    lib = _lib.load()
    up = lambda n: (n + 15) // 16 * 16
    # (rows, C, bands, 5, T) 32-bit bins, a band being 8 rows of the (H + 1)-row lattice
    assert lib.acg_minkowski_workspace_bytes(2, 3, 64, 64, 31) == up(2 * 3 * 9 * 5 * 31 * 4)
    assert lib.acg_minkowski_workspace_bytes(1, 1, 7, 5, 1) == up(1 * 5 * 4) and lib.acg_minkowski_workspace_bytes(1, 1, 8, 5, 1) == up(2 * 5 * 4)
    assert lib.acg_minkowski_workspace_bytes(1, 1, 1024, 1024, 255) == up(129 * 5 * 255 * 4)
    for bad in ((0, 1, 8, 8, 1), (1, 0, 8, 8, 1), (1, 1, 0, 8, 1), (1, 1, 8, 1025, 1), (1, 1, 8, 8, 0), (1, 1, 8, 8, 256), (1 << 30, 4, 8, 8, 1)):
        assert lib.acg_minkowski_workspace_bytes(*bad) == 0, bad


def test_ops_refuses_on_the_host_before_any_device_call(monkeypatch):
    from dtgan_amd import _lib, ops

    def no_device(*a, **k):
        raise AssertionError("a refusal reached the library")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(_lib, "query", no_device)
    z = lambda *shape: torch.zeros(shape)
    thr = np.zeros((1, 2), np.float32)
    with pytest.raises(_lib.AcgError, match="layout"):
        ops.minkowski(z(1, 1, 32, 32), 1, "chwn", thr)
    with pytest.raises(_lib.AcgError, match="4-d"):
        ops.minkowski(z(1, 32, 32), 1, "nchw", thr)
    with pytest.raises(_lib.AcgError, match="1024"):
        ops.minkowski(z(1, 1, 4, 1025), 1, "nchw", thr)
    with pytest.raises(_lib.AcgError, match="1024"):
        ops.minkowski(z(1, 1025, 4, 4), 1, "nhwc", thr)
    with pytest.raises(_lib.AcgError, match="channels"):
        ops.minkowski(z(2, 8, 8, 4), 5, "nhwc", np.zeros((5, 1), np.float32))
    for bad in (np.zeros((2, 2), np.float32), np.zeros(2, np.float32), np.zeros((1, 256), np.float32), np.zeros((1, 0), np.float32),
                np.array([[1.0, 0.0]]), np.array([[0.0, np.nan]]), np.array([[0.0, np.inf]])):
        with pytest.raises(_lib.AcgError, match="minkowski: thresholds"):
            ops.minkowski(z(2, 1, 8, 8), 1, "nchw", bad)
    for bad in (torch.zeros(2, 2), torch.zeros(1, 256), torch.zeros(1, 2, dtype=torch.float64)):      # tensors: shape and type only
        with pytest.raises(_lib.AcgError, match="minkowski: thresholds"):
            ops.minkowski(z(2, 1, 8, 8), 1, "nchw", bad)
    for bad in (torch.zeros(2, 1, 2, 5), torch.zeros(2, 1, 2, 4, dtype=torch.int64), torch.zeros(2, 1, 5, 2, dtype=torch.int64).transpose(2, 3)):
        with pytest.raises(_lib.AcgError, match="out"):
            ops.minkowski(z(2, 1, 8, 8), 1, "nchw", thr, out=bad)
    with pytest.raises(_lib.AcgError, match="ROCm device"):          # and a valid call has no CPU path
        ops.minkowski(z(2, 1, 8, 8), 1, "nchw", thr)
    with pytest.raises(_lib.AcgError, match="ROCm device"):
        ops.minkowski(z(2, 1, 8, 8), 1, "nchw", thr, out=torch.zeros(2, 1, 2, 5, dtype=torch.int64))
