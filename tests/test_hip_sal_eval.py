"""GPU tests of the SAL score above the C ABI: model.translate_sal against tests/sal_ref.py on the members generate_multi
gives for the same codes and on their mean, eval_metrics.eval_sal on a tiny split, and `--metric fss --fss_sal 1` on a saved
tiny checkpoint (test_model, what `python -m dtgan_amd.test` runs): the keys and shapes of sal.npz beside an fss.npz that keeps
its bits."""
import os
import re

import numpy as np
import pytest
import torch

import minkowski_ref as K
import sal_ref as R
from eval_cases import SMOOTH_S as S, smooth_experiment as experiment, smooth_model as model  # noqa: F401  (fixtures: the tiny model, the saved checkpoint)
from sal_ref import check as _check

pytestmark = pytest.mark.gpu

NAMES = ("field", "obj", "shape")
SCORES = ("S", "A", "L1", "L2", "L")
SUMMARIES = ("median_S", "median_A", "median_L", "mean_abs_S", "mean_abs_A", "mean_L", "defined")


def _triple(r, who):
    return tuple(r["%s_%s" % (who, n)].cpu().numpy() for n in NAMES)


def test_translate_sal_equals_the_reference_on_generate_multis_members(model):      # noqa: F811
    from dtgan_amd import ops
    N, M, C, T = 2, 3, 3, 3
    g = torch.Generator(device="cuda").manual_seed(5)
    A = torch.rand(N, 3, S, S, device="cuda", generator=g) * 2 - 1
    B = torch.rand(N, 3, S, S, device="cuda", generator=g) * 2 - 1
    z = torch.randn(N * M, 4, 1, 1, device="cuda", generator=g)
    with torch.no_grad():
        members = model.generate_multi(A, z)                       # (N M, C, S, S), input n at rows n M .. n M + M - 1
    mh = members.cpu().numpy()
    thr = np.quantile(mh.transpose(1, 0, 2, 3).reshape(C, -1).astype(np.float64), (0.5, 0.8, 0.95), axis=1).T.astype(np.float32)
    mean = model.translate_ensemble(A, M, z=z)["mean"].cpu().numpy()           # the kernel's own per-pixel mean, its bits
    for conn, floor in ((8, -1.0), (4, -0.5)):
        before = [(mod, mod.training) for mod in model.netG_A_B.modules()]
        r = model.translate_sal(A, M, B, thr, floor=floor, conn=conn, z=z, chunk=M)     # two groups of one input
        assert all(mod.training == t for mod, t in before) and torch.is_grad_enabled()
        assert set(r) == {"%s_%s" % (who, n) for who in ("members", "ens_mean", "target") for n in NAMES}
        assert r["members_field"].shape == (N, M, C, 3) and r["members_obj"].shape == (N, M, C, T, 4)
        assert r["members_shape"].shape == (N, M, C, T, 2) and r["ens_mean_obj"].shape == r["target_obj"].shape == (N, C, T, 4)
        assert all(v.is_cuda and not v.requires_grad and v.dtype == (torch.float64 if k.endswith("shape") else torch.int64)
                   for k, v in r.items())
        ref = R.sal(mh, thr, conn, floor)
        assert ref[1][..., 0].max() > 1                            # there are objects
        _check(tuple(a.reshape((N * M,) + a.shape[2:]) for a in _triple(r, "members")), ref, ("members", conn))
        _check(_triple(r, "ens_mean"), R.sal(mean, thr, conn, floor), ("ens_mean", conn))
        _check(_triple(r, "target"), R.sal(B.cpu().numpy(), thr, conn, floor), ("target", conn))
        for other in (model.translate_sal(A, M, B, torch.from_numpy(thr).cuda(), floor=floor, conn=conn, z=z, chunk=64),):
            for k in r:
                assert torch.equal(other[k], r[k]), k              # one group, device thresholds: the same bits
        # the scores of every member against its truth are the reference's plain loops
        tgt = _triple(r, "target")
        got = ops.sal_scores(_triple(r, "members"), tuple(a[:, None] for a in tgt), S, S)
        for n in range(N):
            for m in range(M):
                want = R.scores_one(tuple(a[n * M + m] for a in ref), tuple(a[n] for a in R.sal(B.cpu().numpy(), thr, conn, floor)), S, S)
                for k in SCORES:
                    assert np.allclose(got[k][n, m], want[k], rtol=1e-12, atol=1e-14, equal_nan=True), (k, n, m)
        same = ops.sal_scores(tgt, tgt, S, S)                      # identical inputs on both sides
        assert all(np.all(v[~np.isnan(v)] == 0) for v in same.values()) and not np.isnan(same["A"]).any()
    with pytest.raises(ValueError, match="real_B"):
        model.translate_sal(A, M, B[:1], thr, z=z)
    with pytest.raises(ValueError, match="translate_sal: thresholds"):
        model.translate_sal(A, M, B, thr[:, ::-1].copy(), z=z)


def test_eval_sal_on_a_tiny_split(model):      # noqa: F811
    from dtgan_amd import eval_metrics as EM, ops
    A = K.make_fields("smooth", 5, 3, S, S, np.zeros((3, 1), np.float32), seed=1)
    B = K.make_fields("smooth", 5, 3, S, S, np.zeros((3, 1), np.float32), seed=2)
    thr_B, thr_A = EM.fss_thresholds(B, (0.5, 0.9)), EM.fss_thresholds(A, (0.5, 0.9))
    batches = [dict(A=torch.from_numpy(A[:3]), B=torch.from_numpy(B[:3])), dict(A=torch.from_numpy(A[3:]), B=torch.from_numpy(B[3:]))]
    M, C, T = 2, 3, 2
    torch.manual_seed(11)
    res = EM.eval_sal(batches, model, M, thr_B, thr_A, floor=-1.0, conn=8)
    assert set(res) == {"%s_%s" % (s, k) for s in SCORES + SUMMARIES for k in EM.SAL_PAIRS}
    for k in EM.SAL_PAIRS:
        lead = (5, M) if k == "members_B" else (5,)
        for s in SCORES:
            assert res["%s_%s" % (s, k)].shape == lead + ((C, T) if s in ("S", "L2", "L") else (C,)), (s, k)
            assert res["%s_%s" % (s, k)].dtype == np.float64
        flat = {s: res["%s_%s" % (s, k)].reshape((-1,) + res["%s_%s" % (s, k)].shape[len(lead):]) for s in SCORES}
        assert np.array_equal(res["median_S_" + k], np.nanmedian(flat["S"], 0), equal_nan=True) and res["median_S_" + k].shape == (C, T)
        assert np.array_equal(res["median_A_" + k], np.nanmedian(flat["A"], 0)) and res["median_A_" + k].shape == (C,)
        assert np.array_equal(res["mean_L_" + k], np.nanmean(flat["L"], 0), equal_nan=True)
        assert np.allclose(res["mean_abs_A_" + k], np.abs(flat["A"]).mean(0), rtol=1e-14, atol=0)
        assert np.array_equal(res["defined_" + k], (~np.isnan(flat["S"]) & ~np.isnan(flat["L"])).mean(0)) and res["defined_" + k].max() > 0
        ok = ~np.isnan(flat["S"])
        assert np.all(np.abs(flat["S"][ok]) <= 2) and np.all(np.abs(flat["A"]) <= 2) and np.all((flat["L"][ok] >= 0) & (flat["L"][ok] <= 2))
    # B -> A is the reference on predict_A's own fields against the paired A
    with torch.no_grad():
        fake_A = model.predict_A(torch.from_numpy(B).cuda()).cpu().numpy()
    f, o = R.sal(fake_A, thr_A, 8), R.sal(A, thr_A, 8)
    want = ops.sal_scores(f, o, S, S)
    for s in SCORES:
        assert np.allclose(res[s + "_fake_A"], want[s], rtol=1e-12, atol=1e-14, equal_nan=True), s


def _run(experiment, capsys, res_dir, *extra):      # noqa: F811
    from dtgan_amd import ops, test as T
    prec = ops.get_precision()
    try:
        opt = T.test_model(["--chk_path", experiment["chk"], "--dataroot", experiment["data"], "--metric", "fss", "--n_samples", "2",
                            "--fss_windows", "1,5", "--res_dir", res_dir] + list(extra))
    finally:
        ops.set_precision(prec)
    return opt, capsys.readouterr().out, os.path.join(experiment["expr"], res_dir)


def test_metric_fss_with_sal_writes_a_file_of_its_own(experiment, capsys):      # noqa: F811
    from dtgan_amd import eval_metrics as EM
    from dtgan_amd.dataloader import load_numpy_data
    opt0, out0, dir0 = _run(experiment, capsys, "res_sal_off")
    assert opt0.fss_sal == 0 and "SAL" not in out0 and "fss.npz" in os.listdir(dir0) and "sal.npz" not in os.listdir(dir0)
    opt, out, res = _run(experiment, capsys, "res_sal", "--fss_sal", "1", "--sal_quantiles", "0.9,0.5", "--sal_floor", "0", "--sal_conn", "4")
    assert opt.fss_sal == 1 and opt.sal_quantiles == (0.5, 0.9) and opt.sal_floor == 0.0 and opt.sal_conn == 4 and opt.n_samples == 2
    # what was there is there, the same bits: SAL draws its members from a forked generator; the printed lines too
    f0, f1 = dict(np.load(os.path.join(dir0, "fss.npz"))), dict(np.load(os.path.join(res, "fss.npz")))
    assert set(f0) == set(f1) and all(np.array_equal(f0[k], f1[k], equal_nan=True) for k in f0)
    fss_lines = [line for line in out0.splitlines() if "_FSS_" in line]
    assert len(fss_lines) == 1 and all(line in out.splitlines() for line in fss_lines)
    three = r"(?:-?\d+\.\d{4}|nan) (?:-?\d+\.\d{4}|nan) (?:-?\d+\.\d{4}|nan)"
    line = re.search(r"^DEV_SAL_B: (%s), TEST_SAL_B: (%s), TEST_SAL_MEAN_B: (%s), TEST_SAL_A: (%s) \(S, A, L\)$" % ((three,) * 4), out, re.M)
    assert line, out[-2000:]
    a = dict(np.load(os.path.join(res, "sal.npz")))
    C, Tn, M = 3, 2, 2
    trainA, trainB, devA, devB, testA, testB = load_numpy_data(experiment["data"], grid_size=S)
    assert int(a["n_samples"]) == M and float(a["floor"]) == 0.0 and int(a["conn"]) == 4
    assert np.array_equal(a["thresholds_B"], EM.fss_thresholds(trainB, (0.5, 0.9))) and a["thresholds_B"].shape == (C, Tn)
    assert np.array_equal(a["thresholds_A"], EM.fss_thresholds(trainA, (0.5, 0.9)))
    want = {"n_samples", "thresholds_B", "thresholds_A", "floor", "conn"}
    for split, n in (("dev", len(devA)), ("test", len(testA))):
        for k in EM.SAL_PAIRS:
            lead = (n, M) if k == "members_B" else (n,)
            for s in SCORES:
                key = "%s_%s_%s" % (split, s, k)
                want.add(key)
                assert a[key].shape == lead + ((C, Tn) if s in ("S", "L2", "L") else (C,)) and a[key].dtype == np.float64, key
            for s in SUMMARIES:
                key = "%s_%s_%s" % (split, s, k)
                want.add(key)
                assert a[key].shape == ((C,) if s.endswith("_A") else (C, Tn)) and a[key].dtype == np.float64, key
    assert set(a) == want, sorted(set(a) ^ want)
    # the printed numbers: the medians at the highest threshold, the channel means
    for i, (split, k) in enumerate((("dev", "members_B"), ("test", "members_B"), ("test", "ens_mean_B"), ("test", "fake_A"))):
        vals = (a["%s_median_S_%s" % (split, k)][:, -1], a["%s_median_A_%s" % (split, k)], a["%s_median_L_%s" % (split, k)][:, -1])
        for printed, v in zip(line.group(i + 1).split(), vals):
            mean = np.nanmean(v) if np.isfinite(v).any() else np.nan
            assert printed == "nan" and np.isnan(mean) or abs(float(printed) - mean) < 1e-4
    assert np.all(a["test_defined_fake_A"] >= 0) and np.all(a["test_defined_fake_A"] <= 1)
    explicit, _, res = _run(experiment, capsys, "res_sal_thr", "--fss_sal", "1", "--sal_thresholds", "1.6,1.4", "--n_samples", "1", "--ema", "0")
    b = dict(np.load(os.path.join(res, "sal.npz")))
    assert explicit.sal_thresholds == (1.4, 1.6) and np.array_equal(b["thresholds_B"], np.tile(np.float32([1.4, 1.6]), (C, 1)))
    assert float(b["floor"]) == -1.0 and int(b["conn"]) == 8 and b["dev_S_members_B"].shape == (len(devA), 1, C, 2)
