"""GPU tests of the reliability tables above the C ABI: model.translate_fss(reliability=...) against tests/reliability_ref.py on
the members generate_multi gives for the same codes and on their mean, and `--metric fss --fss_rel 1` on a saved tiny
checkpoint (test_model, what `python -m dtgan_amd.test` runs): the keys and shapes of reliability.npz beside an fss.npz that
keeps its bits."""
import os
import re

import numpy as np
import pytest
import torch

import reliability_ref as R
from eval_cases import SMOOTH_S as S, smooth_experiment as experiment, smooth_model as model  # noqa: F401  (fixtures: the tiny model, the saved checkpoint)

pytestmark = pytest.mark.gpu

SCORES = tuple(k for k in R.SUMMARY_KEYS)


def test_translate_fss_reliability_equals_the_reference_on_generate_multis_members(model):      # noqa: F811
    N, M, C = 2, 3, 3
    g = torch.Generator(device="cuda").manual_seed(5)
    A = torch.rand(N, 3, S, S, device="cuda", generator=g) * 2 - 1
    B = torch.rand(N, 3, S, S, device="cuda", generator=g) * 2 - 1
    z = torch.randn(N * M, 4, 1, 1, device="cuda", generator=g)
    with torch.no_grad():
        members = model.generate_multi(A, z)                       # (N M, C, S, S), input n at rows n M .. n M + M - 1
    mh, Bh = members.cpu().numpy(), B.cpu().numpy()
    thr = np.quantile(mh.transpose(1, 0, 2, 3).reshape(C, -1).astype(np.float64), (0.5, 0.9), axis=1).T.astype(np.float32)
    T, win, rwin = 2, (1, 5), (1, 5, 17)
    mean = model.translate_ensemble(A, M, z=z)["mean"].cpu().numpy()           # the kernel's own per-pixel mean, its bits
    plain = model.translate_fss(A, M, B, thr, win, z=z)
    assert set(plain) == {"members", "ens_prob", "ens_mean"}         # None: no entry more
    before = [(mod, mod.training) for mod in model.netG_A_B.modules()]
    state = torch.cuda.get_rng_state()
    r = model.translate_fss(A, M, B, thr, win, z=z, chunk=M, reliability=rwin)      # two groups of one input
    assert torch.equal(torch.cuda.get_rng_state(), state)          # no random draw of its own
    assert all(mod.training == t for mod, t in before) and torch.is_grad_enabled()
    assert set(r) == set(plain) | {"ens_rel", "members_rel", "ens_mean_rel"}
    assert all(torch.equal(r[k], plain[k]) for k in plain)           # what was there keeps its bits
    assert r["ens_rel"].shape == (N, C, T, 3, M + 1, 2) and r["members_rel"].shape == (N, M, C, T, 3, 2, 2)
    assert r["ens_mean_rel"].shape == (N, C, T, 3, 2, 2)
    assert all(r[k].is_cuda and r[k].dtype == torch.int64 and not r[k].requires_grad for k in ("ens_rel", "members_rel", "ens_mean_rel"))
    ens = r["ens_rel"].cpu().numpy()
    assert np.array_equal(ens, R.tables(mh, Bh, thr, rwin, M)) and 0 < ens[..., 1:M, :].sum()
    assert np.array_equal(r["members_rel"].cpu().numpy().reshape((N * M,) + ens.shape[1:4] + (2, 2)),
                          R.tables(mh, np.repeat(Bh, M, axis=0), thr, rwin, 1))
    assert np.array_equal(r["ens_mean_rel"].cpu().numpy(), R.tables(mean, Bh, thr, rwin, 1))
    one = model.translate_fss(A, M, B, torch.from_numpy(thr).cuda(), win, z=z, chunk=64, scales=True, reliability=list(rwin))
    assert all(torch.equal(one[k], r[k]) for k in r) and "members_scale" in one      # one group, device thresholds, beside the scales
    for bad in ((2,), (1, 67), (), tuple(range(1, 19, 2))):
        with pytest.raises(ValueError, match="windows"):
            model.translate_fss(A, M, B, thr, win, z=z, reliability=bad)


def _run(experiment, capsys, res_dir, *extra):      # noqa: F811
    from dtgan_amd import ops, test as T
    prec = ops.get_precision()
    try:
        opt = T.test_model(["--chk_path", experiment["chk"], "--dataroot", experiment["data"], "--metric", "fss", "--n_samples", "2",
                            "--fss_windows", "1,5", "--fss_quantiles", "0.5,0.9", "--res_dir", res_dir] + list(extra))
    finally:
        ops.set_precision(prec)
    return opt, capsys.readouterr().out, os.path.join(experiment["expr"], res_dir)


def test_metric_fss_with_reliability_writes_a_file_of_its_own(experiment, capsys):      # noqa: F811
    from dtgan_amd import eval_metrics as EM, ops
    from dtgan_amd.dataloader import load_numpy_data
    opt0, out0, dir0 = _run(experiment, capsys, "res_rel_off")
    assert opt0.fss_rel == 0 and "_REL_" not in out0 and "fss.npz" in os.listdir(dir0) and "reliability.npz" not in os.listdir(dir0)
    opt, out, res = _run(experiment, capsys, "res_rel", "--fss_rel", "1", "--rel_windows", "1,9,65")
    assert opt.fss_rel == 1 and opt.rel_windows == (1, 9, 65) and opt.n_samples == 2
    # what was there is there, the same bits: the tables come from the same members; the printed lines too
    f0, f1 = dict(np.load(os.path.join(dir0, "fss.npz"))), dict(np.load(os.path.join(res, "fss.npz")))
    assert set(f0) == set(f1) and all(f0[k].dtype == f1[k].dtype and np.array_equal(f0[k], f1[k], equal_nan=True) for k in f0)
    assert all(f0[k].tobytes() == f1[k].tobytes() for k in f0)
    fss_lines = [line for line in out0.splitlines() if "_FSS_" in line]
    assert len(fss_lines) == 1 and all(line in out.splitlines() for line in fss_lines)
    num = r"(?:-?\d+\.\d{4}|nan)"
    three = "%s %s %s" % (num, num, num)
    line = re.search(r"^DEV_REL_PROB_B: (%s), TEST_REL_PROB_B: (%s) \(BSS, reliability, AUC\), TEST_BSS_B: (%s), TEST_BSS_MEAN_B: (%s), "
                     r"TEST_BSS_A: (%s)$" % (three, three, num, num, num), out, re.M)
    assert line, out[-2000:]
    a = dict(np.load(os.path.join(res, "reliability.npz")))
    C, Tn, M, nw = 3, 2, 2, 3
    trainA, trainB, devA, devB, testA, testB = load_numpy_data(experiment["data"], grid_size=S)
    assert int(a["n_samples"]) == M and a["windows"].tolist() == [1, 9, 65] and a["windows"].dtype == np.int64
    assert np.array_equal(a["thresholds_B"], EM.fss_thresholds(trainB, (0.5, 0.9))) and a["thresholds_B"].shape == (C, Tn)
    assert np.array_equal(a["thresholds_A"], EM.fss_thresholds(trainA, (0.5, 0.9)))
    assert np.array_equal(a["thresholds_B"], f1["thresholds_B"]) and np.array_equal(a["thresholds_A"], f1["thresholds_A"])
    want = {"n_samples", "windows", "thresholds_B", "thresholds_A"}
    lead = (C, Tn, nw)
    for split, n in (("dev", len(devA)), ("test", len(testA))):
        for k in EM.REL_PAIRS:
            Mk = M if k == "ens_prob_B" else 1
            rows = n * (M if k == "members_B" else 1)
            shapes = dict(table=lead + (Mk + 1, 2), n=lead + (Mk + 1,), prob=(Mk + 1,), obs_freq=lead + (Mk + 1,), roc_hit=lead + (Mk + 2,),
                          roc_false=lead + (Mk + 2,))
            for s in ("table",) + SCORES:
                key = "%s_%s_%s" % (split, s, k)
                want.add(key)
                assert a[key].shape == shapes.get(s, lead) and a[key].dtype == (np.int64 if s in ("table", "n") else np.float64), key
            table = a["%s_table_%s" % (split, k)]
            assert np.all(table.sum((-2, -1)) == rows * S * S) and table.min() >= 0, (split, k)
            again = ops.reliability_summary(table)
            assert all(np.array_equal(a["%s_%s_%s" % (split, s, k)], again[s], equal_nan=True) for s in SCORES)
    assert set(a) == want, sorted(set(a) ^ want)
    # window 1 holds the events the fss entries counted: observed events, and the members' forecast events
    for split in ("dev", "test"):
        assert np.array_equal(a[split + "_table_ens_prob_B"][:, :, 0, :, 1].sum(-1), f1[split + "_sums_ens_prob_B"][:, :, 0, 1])
        assert np.array_equal(a[split + "_table_members_B"][:, :, 0, 1, :].sum(-1), f1[split + "_sums_members_B"][:, :, 0, 0])
        assert np.array_equal(a[split + "_table_fake_A"][:, :, 0, 1, 1], f1[split + "_sums_fake_A"][:, :, 0, 2])
    # the printed numbers: the highest threshold, window 1, the channel means
    def mean(v):
        return np.nanmean(v) if np.isfinite(v).any() else np.nan
    vals = [mean(a["%s_%s_ens_prob_B" % (split, s)][:, -1, 0]) for split in ("dev", "test") for s in ("bss", "reliability", "auc")]
    vals += [mean(a["test_bss_%s" % k][:, -1, 0]) for k in EM.REL_PAIRS[1:]]
    printed = line.group(1).split() + line.group(2).split() + [line.group(i) for i in (3, 4, 5)]
    for p, v in zip(printed, vals):
        assert p == "nan" and np.isnan(v) or abs(float(p) - v) < 1e-4, (p, v)
    # beside the other options of the metric: every file, fss.npz with the scales' entries on top of what it held
    _, out2, res2 = _run(experiment, capsys, "res_rel_all", "--fss_rel", "1", "--fss_scales", "1", "--fss_sal", "1", "--n_samples", "1")
    assert {"fss.npz", "sal.npz", "reliability.npz"} <= set(os.listdir(res2)) and "DEV_REL_PROB_B" in out2 and "DEV_SAL_B" in out2
    b = dict(np.load(os.path.join(res2, "reliability.npz")))
    assert b["windows"].tolist() == [1, 5, 17] and b["test_table_ens_prob_B"].shape == (C, Tn, 3, 2, 2) and np.all(np.isnan(b["test_brier_fair_ens_prob_B"]))
    assert np.array_equal(b["test_table_ens_prob_B"], b["test_table_members_B"])      # one member is the ensemble
