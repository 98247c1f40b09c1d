"""GPU tests of the Minkowski evaluator above the C ABI: model.translate_minkowski against tests/minkowski_ref.py on the
members generate_multi gives for the same codes, eval_metrics.eval_minkowski's real sets against the reference, and `--metric
minkowski` on a saved tiny checkpoint (test_model, what `python -m dtgan_amd.test` runs)."""
import os
import re

import numpy as np
import pytest
import torch

import minkowski_ref as K
from eval_cases import SMOOTH_S as S, smooth_experiment as experiment, smooth_model as model  # noqa: F401  (fixtures: the tiny model, the saved checkpoint)

pytestmark = pytest.mark.gpu

FUNCTIONALS = ("area", "perimeter", "euler4", "euler8")


def test_translate_minkowski_equals_the_reference_on_generate_multis_members(model):
    N, M, C, T = 3, 3, 3, 9
    g = torch.Generator(device="cuda").manual_seed(5)
    A = torch.rand(N, 3, S, S, device="cuda", generator=g) * 2 - 1
    z = torch.randn(N * M, 4, 1, 1, device="cuda", generator=g)
    with torch.no_grad():
        members = model.generate_multi(A, z)                       # (N M, C, S, S), input n at rows n M .. n M + M - 1
    mh = members.cpu().numpy()
    # thresholds that cut through what this generator gives: the deciles of its own members, per channel, one repeated
    thr = np.quantile(mh.transpose(1, 0, 2, 3).reshape(C, -1).astype(np.float64), np.arange(1, T + 1) / (T + 1.0), axis=1).T.astype(np.float32)
    thr[:, 4] = thr[:, 3]
    before = [(mod, mod.training) for mod in model.netG_A_B.modules()]
    r = model.translate_minkowski(A, M, thr, z=z, chunk=6)          # two groups: 2 inputs, then 1
    assert all(mod.training == t for mod, t in before) and torch.is_grad_enabled()
    assert set(r) == {"members", "ens_mean"}
    assert r["members"].shape == (N, M, C, T, 5) and r["ens_mean"].shape == (N, C, T, 5)
    assert all(v.dtype == torch.int64 and v.is_cuda and not v.requires_grad for v in r.values())
    ref = K.counts(mh, thr)
    assert np.array_equal(r["members"].cpu().numpy().reshape(N * M, C, T, 5), ref)
    pooled = ref[..., 0].sum(0)                                     # pooled quantiles: no set is empty or full over the members
    assert 0 < pooled.min() and pooled.max() < N * M * S * S
    mean = model.translate_ensemble(A, M, z=z)["mean"]              # the kernel's own per-pixel mean, its bits
    assert np.array_equal(r["ens_mean"].cpu().numpy(), K.counts(mean.cpu().numpy(), thr))
    for other in (model.translate_minkowski(A, M, torch.from_numpy(thr).cuda(), z=z, chunk=64),     # one group, device thresholds
                  model.translate_minkowski(A, M, thr, z=z, chunk=M)):                               # one input per group
        for k in r:
            assert torch.equal(other[k], r[k]), k
    one = model.translate_minkowski(A, 1, thr, z=z[:N])
    assert torch.equal(one["members"][:, 0], one["ens_mean"])       # M = 1: the mean is the member
    with pytest.raises(ValueError, match="n_samples"):
        model.translate_minkowski(A, 65, thr)
    with pytest.raises(ValueError, match="codes"):
        model.translate_minkowski(A, 2, thr, z=z[:5])
    with pytest.raises(ValueError, match="cannot hold"):
        model.translate_minkowski(A, 4, thr, chunk=3)
    with pytest.raises(ValueError, match="translate_minkowski: thresholds"):
        model.translate_minkowski(A, 2, thr[:2])
    with pytest.raises(ValueError, match="translate_minkowski: thresholds"):
        model.translate_minkowski(A, 2, thr[:, ::-1])


def test_the_real_sets_of_eval_minkowski_are_the_references(model):
    from dtgan_amd import eval_metrics as EM, ops
    rs = np.random.RandomState(7)
    A = K.make_fields("smooth", 5, 3, S, S, np.zeros((3, 1), np.float32), seed=1)
    B = K.make_fields("smooth", 5, 3, S, S, np.zeros((3, 1), np.float32), seed=2)
    B[rs.uniform(size=B.shape) < 0.3] = -1.0                        # mass at one value: the octiles 1/8 and 2/8 coincide
    thr_B, thr_A = EM.marginal_edges(B, 8), EM.marginal_edges(A, 8)
    assert np.any(np.diff(thr_B, axis=1) == 0)
    batches = [dict(A=torch.from_numpy(A[:3]), B=torch.from_numpy(B[:3])), dict(A=torch.from_numpy(A[3:]), B=torch.from_numpy(B[3:]))]
    M = 2
    torch.manual_seed(11)
    res = EM.eval_minkowski(batches, model, M, thr_B, thr_A)
    P = S * S
    for d, x, thr in (("B", B, thr_B), ("A", A, thr_A)):
        ref = K.counts(x, thr).sum(0)
        assert res["counts_real_" + d].dtype == np.int64 and np.array_equal(res["counts_real_" + d], ref)
        assert int(res["cells_real_" + d]) == 5 * P
        f = K.functionals(ref)
        for k in FUNCTIONALS:
            assert np.array_equal(res["%s_real_%s" % (k, d)], f[k].astype(np.float64))
            assert np.array_equal(res["%s_density_real_%s" % (k, d)], f[k] / float(5 * P))
    assert int(res["cells_members_B"]) == 5 * M * P and int(res["cells_ens_mean_B"]) == 5 * P == int(res["cells_fake_A"])
    with torch.no_grad():
        fake_A = model.predict_A(torch.from_numpy(B).cuda()).cpu().numpy()
    assert np.array_equal(res["counts_fake_A"], K.counts(fake_A, thr_A).sum(0))
    for k, real in EM.MINKOWSKI_PAIRS:
        d = ops.minkowski_distance(ops.minkowski_summary(res["counts_" + k], res["cells_" + k]),
                                   ops.minkowski_summary(res["counts_" + real], res["cells_" + real]))
        for f in FUNCTIONALS:
            assert res["dist_%s_%s" % (f, k)].shape == (3,) and np.array_equal(res["dist_%s_%s" % (f, k)], d[f])
    real = ops.minkowski_summary(res["counts_real_B"], res["cells_real_B"])
    assert all(np.all(v == 0) for v in ops.minkowski_distance(real, real).values())


def test_metric_minkowski_writes_its_file(experiment, capsys):
    from dtgan_amd import eval_metrics as EM, ops, test as T
    from dtgan_amd.dataloader import load_numpy_data
    prec = ops.get_precision()
    try:
        opt = T.test_model(["--chk_path", experiment["chk"], "--dataroot", experiment["data"], "--metric", "minkowski", "--n_samples",
                            "2", "--mink_bins", "6", "--res_dir", "res_mink"])
    finally:
        ops.set_precision(prec)
    assert opt.ema == 0 and opt.mink_bins == 6 and opt.n_samples == 2
    out = capsys.readouterr().out
    four = r"\d+\.\d{6} \d+\.\d{6} \d+\.\d{6} \d+\.\d{6}"
    for split in ("DEV", "TEST"):
        assert re.search(r"^%s_MINK_B: %s, %s_MINK_MEAN_B: %s, %s_MINK_A: %s \(area, perimeter, euler4, euler8\)$"
                         % (split, four, split, four, split, four), out, re.M), out[-2000:]
    a = dict(np.load(os.path.join(experiment["expr"], "res_mink", "minkowski.npz")))
    C, Tn, M, P = 3, 5, 2, S * S
    assert int(a["n_samples"]) == M and int(a["bins"]) == 6
    trainA, trainB, devA, devB, testA, testB = load_numpy_data(experiment["data"], grid_size=S)
    for name, train in (("thresholds_B", trainB), ("thresholds_A", trainA)):
        q = np.quantile(np.asarray(train).astype(np.float64).transpose(1, 0, 2, 3).reshape(C, -1), np.arange(1, 6) / 6.0, axis=1).T
        assert a[name].dtype == np.float32 and a[name].shape == (C, Tn) and np.array_equal(a[name], q.astype(np.float32)), name
    want = {"n_samples", "bins", "thresholds_B", "thresholds_A"}
    assert EM.MINKOWSKI_SETS == ("members_B", "ens_mean_B", "fake_A", "real_B", "real_A")
    for split, fields in (("dev", (devA, devB)), ("test", (testA, testB))):
        g = lambda name: a["%s_%s" % (split, name)]
        n = len(fields[0])
        for k in EM.MINKOWSKI_SETS:
            want |= {"%s_counts_%s" % (split, k), "%s_cells_%s" % (split, k)}
            assert g("counts_" + k).shape == (C, Tn, 5) and g("counts_" + k).dtype == np.int64 and np.all(g("counts_" + k) >= 0)
            assert g("cells_" + k).dtype == np.int64 and int(g("cells_" + k)) == n * P * (M if k == "members_B" else 1)
            assert np.all(np.diff(g("counts_" + k), axis=1) <= 0)    # nested sets
            f = K.functionals(g("counts_" + k))
            for name in FUNCTIONALS:
                want |= {"%s_%s_%s" % (split, name, k), "%s_%s_density_%s" % (split, name, k)}
                assert g("%s_%s" % (name, k)).dtype == np.float64 and np.array_equal(g("%s_%s" % (name, k)), f[name].astype(np.float64))
                assert np.array_equal(g("%s_density_%s" % (name, k)), f[name] / float(g("cells_" + k)))
        for (k, real), tag in zip(EM.MINKOWSKI_PAIRS, ("MINK_B", "MINK_MEAN_B", "MINK_A")):
            printed = re.search(r"%s_%s: (%s)" % (split.upper(), tag, four), out).group(1).split()
            for i, name in enumerate(FUNCTIONALS):
                key = "dist_%s_%s" % (name, k)
                want.add("%s_%s" % (split, key))
                d = np.abs(g("%s_density_%s" % (name, k)) - g("%s_density_%s" % (name, real))).mean(-1)
                assert g(key).shape == (C,) and g(key).dtype == np.float64 and np.array_equal(g(key), d)
                assert abs(float(printed[i]) - d.mean()) < 1e-6
        # the real sets are the reference on the split's own fields, exactly
        assert np.array_equal(g("counts_real_A"), K.counts(np.asarray(fields[0]), a["thresholds_A"]).sum(0))
        assert np.array_equal(g("counts_real_B"), K.counts(np.asarray(fields[1]), a["thresholds_B"]).sum(0))
    assert set(a) == want, sorted(set(a) ^ want)

