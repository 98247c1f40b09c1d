"""CPU tests of the fractions-skill-score training loss: the numpy reference (tests/fss_loss_ref.py) and its analytic gradient
against fp64 autograd, the hard limit against tests/fss_ref.py's integer triples, closed forms, the pooling rule, the float32
bars of the device tests, the option parser, the header, the binding and the documents, and the refusals of ops.fss_loss
that need no device."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

import abi
import fss_loss_ref as R
import fss_ref as F
from model_cases import parse_train as _parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_loss(x, y, thr, windows, tau):
    """the definition once more, in fp64 torch: the window sum as a zero-padded convolution with a kernel of ones"""
    thr = torch.tensor(np.asarray(thr), dtype=torch.float64)
    p = torch.sigmoid((x[:, :, None] - thr[None, :, :, None, None]) / tau)
    q = torch.sigmoid((y[:, :, None] - thr[None, :, :, None, None]) / tau)
    N, C, T, H, W = p.shape
    Rs = []
    for n in windows:
        k = torch.ones(1, 1, n, n, dtype=torch.float64)
        cf = torch.nn.functional.conv2d(p.reshape(-1, 1, H, W), k, padding=n // 2).reshape(p.shape)
        co = torch.nn.functional.conv2d(q.reshape(-1, 1, H, W), k, padding=n // 2).reshape(p.shape)
        Num, Den = ((cf - co) ** 2).sum((0, 3, 4)), (cf ** 2 + co ** 2).sum((0, 3, 4))
        some = Den != 0
        Rs.append(torch.where(some, Num / torch.where(some, Den, torch.ones_like(Den)), torch.zeros_like(Den)))
    return torch.stack(Rs, -1).mean()


@pytest.mark.parametrize("H,W,windows,kind", ((1, 1, (1, 3), "noise"), (5, 7, (9,), "ties"), (5, 7, (1, 3, 9), "noise"),
                                              (33, 31, (65,), "shifted"), (33, 31, (65,), "noise"),
                                              (33, 31, (3, 33, 65), "ties")))
def test_the_analytic_gradient_equals_fp64_autograd_of_the_same_expression(H, W, windows, kind):
    x, y, thr = R.make_case(H, W, 2, 2, 3, kind)
    if kind == "ties":
        thr[:, 0] = 0.5                                            # met exactly by many cells: p = 1/2 there
        assert np.any(x[:, 0] == 0.5)
    tau = 0.25
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    loss = _torch_loss(xt, torch.tensor(y, dtype=torch.float64), thr, windows, tau)
    ref = R.loss(x, y, thr, windows, tau)
    assert abs(loss.item() - ref["loss"]) <= 1e-14
    assert ref["R"].shape == (2, 3, len(windows)) and ref["num"].shape == (2, 2, 3, len(windows)) and (ref["Den"] > 0).all()
    (loss * 0.375).backward()
    g = R.grad(x, y, thr, windows, tau) * 0.375
    # 1e-17 absolute: a window that covers the domain from every cell sees equal totals in a field and its rolled copy
    # ("shifted" at 33 x 31 with n = 65), the true gradient is 0 and both sides hold the roundings of what cancels
    err = np.abs(xt.grad.numpy() - g).max()
    assert err <= 1e-12 * np.abs(g).max() + 1e-17, (err, np.abs(g).max())


def test_the_window_sums_are_fss_refs_box_counts_on_real_planes():
    rs = np.random.RandomState(0)
    for H, W in ((1, 1), (5, 7), (33, 31)):
        b = rs.randint(0, 2, (H, W))
        for n in (1, 3, 9, 65):
            want = F.box_counts_brute(b, n)
            assert np.array_equal(R.box_sum(b, n), want) and np.array_equal(F.box_counts(b, n), want)
            for order in ("sequential", "pairwise"):
                got = R.box_sum(b, n, np.float32, order)
                assert got.dtype == np.float32 and np.array_equal(got, want)        # 0/1 planes: exact integers in float32
    p = rs.uniform(size=(2, 5, 7))
    brute = np.array([[[p[k, max(i - 1, 0):i + 2, max(j - 1, 0):j + 2].sum() for j in range(7)] for i in range(5)] for k in range(2)])
    assert np.allclose(R.box_sum(p, 3), brute, rtol=1e-15)


@pytest.mark.parametrize("H,W", ((1, 1), (5, 7), (33, 31), (65, 130)))
def test_saturated_float32_events_give_the_evaluators_integer_triples(H, W):
    """tau = margin / 200 and every value at least margin from every threshold: p and q are exactly 0 or 1 in float32, and num
    and den in double from float32 window sums equal ff + oo - 2 fo and ff + oo of the integer triples"""
    margin, windows = 1e-3, (1, 3, 9, 33, 65)
    for kind in ("noise", "shifted", "ties", "extremes"):
        x, y, thr = F.make_pair(kind, H, W)
        x, y = R.harden(x, thr, margin), R.harden(y, thr, margin)
        p = R.soft_events32(x, thr, margin / 200)
        assert p.dtype == np.float32 and np.array_equal(p, F.events(x, thr).astype(np.float32))
        tri = F.triples(x, y, thr, windows).astype(np.float64)
        for order in ("sequential", "pairwise"):
            num, den = R.parts32(x, y, thr, windows, margin / 200, order)
            assert np.array_equal(num, tri[..., 0] + tri[..., 1] - 2 * tri[..., 2]), (kind, order)
            assert np.array_equal(den, tri[..., 0] + tri[..., 1]), (kind, order)
        g = R.grad32(x, y, thr, windows, margin / 200)
        assert np.all(g == 0.0)                                    # p (1 - p) is exactly 0, and Den == 0 gives no NaN


def test_closed_forms():
    x, y, thr = R.make_case(16, 16, 2, 2, 2)
    windows = (1, 5, 33)
    same = R.loss(x, x, thr, windows, 0.25)
    assert same["loss"] == 0.0 and np.all(same["R"] == 0.0) and np.all(R.grad(x, x, thr, windows, 0.25) == 0.0)
    # a threshold nothing exceeds at a small tau: exp overflows, p == q == 0, Den == 0 exactly -> R = 0, gradient 0, no NaN
    none = np.full((2, 1), 50.0, dtype=np.float32)
    f = R.loss(x, y, none, windows, 0.005)
    assert np.all(f["Den"] == 0.0) and np.all(f["den"] == 0.0) and np.all(f["R"] == 0.0) and f["loss"] == 0.0
    with np.errstate(all="raise", over="ignore"):
        g = R.grad(x, y, none, windows, 0.005)
    assert np.all(g == 0.0) and not np.isnan(g).any()
    a, b = R.coefficients(f["R"], f["Den"])
    assert np.all(a == 0.0) and np.all(b == 0.0)
    num32, den32 = R.parts32(x, y, none, windows, 0.005)
    assert np.all(den32 == 0.0) and np.all(num32 == 0.0) and np.all(R.grad32(x, y, none, windows, 0.005) == 0.0)
    # at tau = 0.25 the same threshold leaves Den > 0: the rule does not apply and R is a ratio of tiny sums
    assert np.all(R.loss(x, y, none, windows, 0.25)["Den"] > 0)
    # a threshold everything exceeds: p == q == 1, cf == co
    every = np.full((2, 1), -5.0, dtype=np.float32)
    f = R.loss(x, y, every, windows, 0.005)
    assert f["loss"] == 0.0 and np.all(f["Den"] > 0) and np.all(R.grad(x, y, every, windows, 0.005) == 0.0)
    # all against none: co == 0, so (cf - co)^2 == cf^2 + co^2 and R == 1
    hi, lo = np.full((1, 1, 9, 11), 3.0, dtype=np.float32), np.full((1, 1, 9, 11), -3.0, dtype=np.float32)
    f = R.loss(hi, lo, np.zeros((1, 1), dtype=np.float32), (1, 3, 9), 0.005)
    assert np.all(f["R"] == 1.0) and f["loss"] == 1.0
    # a block displaced by its width: no overlap at n = 1, and R falls as the window grows
    y = np.full((1, 1, 32, 32), -1.0, dtype=np.float32)
    x = y.copy()
    y[0, 0, 12:16, 8:12], x[0, 0, 12:16, 12:16] = 1.0, 1.0
    Rn = R.loss(x, y, np.zeros((1, 1), dtype=np.float32), (1, 3, 5, 9, 17), 0.005)["R"][0, 0]
    assert Rn[0] == 1.0 and np.all(np.diff(Rn) < 0) and Rn[-1] < 0.2, Rn


def test_the_batch_is_pooled_before_the_division():
    """two fields by hand, n = 1 and saturated events: field 0 has 3 forecast and 1 observed event with 1 hit, field 1 none
    forecast and 2 observed: Num = (3 + 1 - 2) + 2 = 4, Den = (3 + 1) + 2 = 6, R = 2/3 - not the mean of 1/2 and 1"""
    x = np.full((2, 1, 2, 3), -1.0, dtype=np.float32)
    y = x.copy()
    x[0, 0, 0, :] = 1.0
    y[0, 0, 0, 0] = 1.0
    y[1, 0, 1, 1:] = 1.0
    f = R.loss(x, y, np.zeros((1, 1), dtype=np.float32), (1,), 0.005)
    assert np.array_equal(f["num"][:, 0, 0, 0], [2.0, 2.0]) and np.array_equal(f["den"][:, 0, 0, 0], [4.0, 2.0])
    assert f["Num"][0, 0, 0] == 4.0 and f["Den"][0, 0, 0] == 6.0 and f["loss"] == 4.0 / 6.0 != (0.5 + 1.0) / 2


def test_the_float32_restatement_stays_within_a_quarter_of_the_bars():
    got = R.measure_bars()
    for order in ("sequential", "pairwise"):
        print(order, got[order], (R.FWD_MEASURED[order], R.GRAD_MEASURED[order]))
        assert got[order][0] <= R.FWD_MEASURED[order] and got[order][1] <= R.GRAD_MEASURED[order]
        assert got[order][0] <= R.FWD_BAR / 4 and got[order][1] <= R.GRAD_BAR / 4
        assert got[order][0] >= 0.8 * R.FWD_MEASURED[order] and got[order][1] >= 0.8 * R.GRAD_MEASURED[order]   # the constants are the measurement
    assert R.FWD_BAR == 4 * max(R.FWD_MEASURED.values()) and R.GRAD_BAR == 4 * max(R.GRAD_MEASURED.values())
    assert R.FWD_BAR < 2e-6 and R.GRAD_BAR < 4e-6
    sizes = {c[:2] for c in R.CASES}
    assert {(1, 1), (1, 7), (5, 7), (33, 31), (64, 64), (65, 130), (321, 321), (3, 1024), (R.TILE, R.TILE), (R.TILE - 1, R.TILE - 1),
            (R.TILE + 1, R.TILE + 1)} <= sizes
    assert {c[4] for c in R.CASES} >= {1, 8} and {len(c[5]) for c in R.CASES} >= {1, 8} and {c[2] for c in R.CASES} >= {1, 2, 3}
    assert any(c[:2] == (5, 7) and 9 in c[5] for c in R.CASES) and any(c[:2] == (33, 31) and {33, 65} <= set(c[5]) for c in R.CASES)


def test_the_options_default_to_off_and_are_written(tmp_path):
    opt = _parse(tmp_path)
    assert opt.lambda_fss_A == 0.0 and opt.lambda_fss_B == 0.0 and opt.fss_loss_quantiles == (0.9, 0.99)
    assert opt.fss_loss_thresholds is None and opt.fss_loss_windows == (3, 9, 17) and opt.fss_tau == 0.05
    assert not hasattr(opt, "fss_loss_thr_A")
    opt = _parse(tmp_path, "--supervised", "--lambda_fss_B", "0.25", "--fss_loss_quantiles", "0.5,0.999", "--fss_loss_windows", "65,1,9",
                 "--fss_tau", "0.1", "--fss_loss_thresholds", "0.25,-0.5")
    assert (opt.lambda_fss_A, opt.lambda_fss_B, opt.fss_tau) == (0.0, 0.25, 0.1)
    assert opt.fss_loss_quantiles == (0.5, 0.999) and opt.fss_loss_windows == (65, 1, 9) and opt.fss_loss_thresholds == (0.25, -0.5)
    assert "lambda_fss_B: 0.25" in open(os.path.join(opt.expr_dir, "opt.txt")).read().splitlines()
    saved = pickle.load(open(os.path.join(opt.expr_dir, "opt.pkl"), "rb"))
    assert saved["lambda_fss_B"] == 0.25 and saved["fss_loss_windows"] == (65, 1, 9)
    assert _parse(tmp_path, "--supervised", "--lambda_fss_A", "1", "--grid_size", "1024").grid_size == 1024
    assert _parse(tmp_path, "--grid_size", "2048", "--model", "cycle_gan").lambda_fss_B == 0.0   # off: nothing to refuse


def test_the_parser_refuses_what_the_term_cannot_take(tmp_path, capsys):
    on = ("--supervised", "--lambda_fss_B", "0.1")
    for extra, word in ((("--lambda_fss_B", "-0.1"), "negative"), (("--lambda_fss_A", "-1"), "negative"),
                        (("--lambda_fss_B", "0.1"), "--supervised"), (("--lambda_fss_A", "0.1"), "--supervised"),
                        (on + ("--model", "cycle_gan"), "paired step"), (on + ("--model", "stoch_cycle_gan"), "paired step"),
                        (on + ("--grid_size", "1025"), "1024"), (("--fss_tau", "0"), "positive"), (("--fss_tau", "-0.05"), "positive"),
                        (("--fss_tau", "inf"), "positive"), (("--fss_tau", "nan"), "positive"),
                        (("--fss_loss_windows", "3,4"), "odd"), (("--fss_loss_windows", "67"), "65"), (("--fss_loss_windows", "0"), "odd"),
                        (("--fss_loss_windows", "1,3,5,7,9,11,13,15,17"), "1 to 8"), (("--fss_loss_windows", "3,x"), "integers"),
                        (("--fss_loss_quantiles", "1.5"), "[0, 1]"), (("--fss_loss_quantiles", "0,.1,.2,.3,.4,.5,.6,.7,.8"), "1 to 8"),
                        (("--fss_loss_thresholds", "nan"), "finite"), (("--fss_loss_thresholds", "1,inf"), "finite")):
        with pytest.raises(SystemExit):
            _parse(tmp_path, *extra)
        err = capsys.readouterr().err
        assert word in err and "fss" in err, (extra, err)


def test_the_header_the_binding_and_the_documents_agree():
    from dtgan_amd import _lib, ops
    for name, nargs in (("acg_fss_loss_workspace_bytes", 6), ("acg_fss_loss_fwd", 21), ("acg_fss_loss_bwd", 23)):
        assert len(abi.header_args(name)) == len(_lib.SIGNATURES[name][1]) == nargs, name
    for name, at in (("acg_fss_loss_fwd", 16), ("acg_fss_loss_bwd", 17)):
        floats = [i for i, k in enumerate(abi.header_args(name)) if k == "float"]
        assert floats == [i for i, t in enumerate(_lib.SIGNATURES[name][1]) if t is _lib.c_float] == [at], name
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("`acg_fss_loss_fwd`", "`acg_fss_loss_bwd`", "acg_fss_loss_workspace_bytes", "ops.fss_loss", "--lambda_fss_B"):
        assert word in doc, word
    assert "--lambda_fss_B" in open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 17\. ", design, re.M) and "acg_fss_loss_fwd" in design and "tools/fss_loss_bench.py" in design
    mk = open(os.path.join(ROOT, "domain-transfer-gan_amd", "csrc", "Makefile")).read()
    assert "fss_loss.hip" in mk
    assert "acg_fss_loss_fwd" in ops.FssLoss.__doc__ and "acg_fss_loss_bwd" in ops.FssLoss.__doc__
    lib = _lib.load()
    for args, want in (((16, 3, 256, 256, 2, 3), 4 * 16 * 3 * 2 * 3 * 256 * 256), ((1, 1, 1, 1, 1, 1), 16), ((2, 3, 1, 7, 8, 8), 4 * 2 * 3 * 64 * 7), ((2, 3, 1, 3, 8, 8), 16 * 2 * 3 * 64),
                       ((1, 1, 33, 31, 1, 2), (4 * 2 * 33 * 31 + 15) // 16 * 16)):
        assert lib.acg_fss_loss_workspace_bytes(*args) == want, args
    for args in ((0, 1, 8, 8, 1, 1), (1, 0, 8, 8, 1, 1), (1, 1, 8, 1025, 1, 1), (1, 1, 0, 8, 1, 1), (1, 1, 8, 8, 9, 1), (1, 1, 8, 8, 1, 0)):
        assert lib.acg_fss_loss_workspace_bytes(*args) == 0, args


def test_every_host_side_refusal_comes_before_a_device_is_needed(monkeypatch):
    from dtgan_amd import _lib, ops

    def no_device(*a, **k):
        raise AssertionError("a refusal that needs no device reached the library")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(_lib, "query", no_device)
    z = lambda *shape: torch.zeros(shape)
    x, y, thr = z(2, 3, 8, 8), z(2, 3, 8, 8), np.zeros((3, 2), dtype=np.float32)
    for windows, word in (((3, 4), "odd"), ((), "1 to 8"), ((1,) * 9, "1 to 8"), ((0,), "odd"), ((-3,), "odd"), ((3.5,), "odd"),
                          ((3, 67), "65")):
        with pytest.raises(_lib.AcgError, match="fss_loss: .*" + word):
            ops.fss_loss(x, y, 3, "nchw", thr, windows, 0.05)
    for tau in (0.0, -0.05, float("inf"), float("nan"), 1e-46, 1e50):  # 1 / tau must be a positive finite float32 too
        with pytest.raises(_lib.AcgError, match="fss_loss: tau"):
            ops.fss_loss(x, y, 3, "nchw", thr, (3,), tau)
    for bad in (np.zeros((2, 2), dtype=np.float32), np.zeros((3, 0), dtype=np.float32), np.zeros((3, 9), dtype=np.float32), np.zeros(3),
                torch.zeros(3, 2, dtype=torch.float64)):
        with pytest.raises(_lib.AcgError, match="fss_loss: thresholds"):
            ops.fss_loss(x, y, 3, "nchw", bad, (3,), 0.05)
    with pytest.raises(_lib.AcgError, match="fss_loss: .*do not pair"):
        ops.fss_loss(x, z(3, 3, 8, 8), 3, "nchw", thr, (3,), 0.05)
    with pytest.raises(_lib.AcgError, match="fss_loss: .*do not pair"):
        ops.fss_loss(x, z(2, 3, 8, 9), 3, "nchw", thr, (3,), 0.05)
    with pytest.raises(_lib.AcgError, match="fss_loss: .*layout"):
        ops.fss_loss(x, y, 3, "chwn", thr, (3,), 0.05)
    with pytest.raises(_lib.AcgError, match="fss_loss: .*4-d"):
        ops.fss_loss(z(2, 8, 8), y, 3, "nchw", thr, (3,), 0.05)
    with pytest.raises(_lib.AcgError, match="fss_loss: .*channels"):
        ops.fss_loss(x, y, 4, "nchw", thr, (3,), 0.05)
    with pytest.raises(_lib.AcgError, match="fss_loss: .*1024"):
        ops.fss_loss(z(1, 1, 2, 1025), z(1, 1, 2, 1025), 1, "nchw", thr[:1], (3,), 0.05)
    with pytest.raises(_lib.AcgError, match="fss_loss: .*1024"):
        ops.fss_loss(z(1, 1025, 2, 4), z(1, 1025, 2, 4), 1, "nhwc", thr[:1], (3,), 0.05)
    with pytest.raises(_lib.AcgError, match="no CPU path"):       # what is left is _check: the tensors are on the host
        ops.fss_loss(x, y, 3, "nchw", thr, (3,), 0.05)
    assert ops.check_fss_loss_windows([3, 9, 65]) == (3, 9, 65) and ops.FSS_LOSS_MAX_WINDOW == R.MAX_WINDOW == 65
    assert ops.fss_loss_inv_tau(0.05) == float(np.float32(20.0)) and ops.fss_loss_inv_tau(5e-6) == float(np.float32(1.0 / 5e-6))


def test_the_paired_step_names_its_options_when_the_thresholds_are_missing():
    import argparse
    from dtgan_amd import losses, model as M
    opt = argparse.Namespace(lambda_fss_A=0.0, lambda_fss_B=0.5, input_nc=3, output_nc=3)
    with pytest.raises(ValueError, match="fss_loss_thr_A and fss_loss_thr_B"):
        losses.add_terms(argparse.Namespace(opt=opt), losses.PAIRED, None, None, None, None, pred=(None, None))
    opt.lambda_fss_B = 0.0
    assert losses.add_terms(argparse.Namespace(opt=opt), losses.PAIRED, None, None, None, None, pred=(None, None)) == (None, [], [])
    assert M._hashable([[0.5, 1], [2, 3]]) == ((0.5, 1), (2, 3)) and M._hashable(0.5) == 0.5 and M._hashable(None) is None
