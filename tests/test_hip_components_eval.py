"""GPU tests of the connected components above the C ABI: model.translate_minkowski(components=) against
tests/components_ref.py on the members generate_multi gives for the same codes, and `--metric minkowski --mink_components` on
a saved tiny checkpoint (test_model, what `python -m dtgan_amd.test` runs) - the file with the option is the file without it
plus the new entries."""
import os
import re

import numpy as np
import pytest
import torch

import components_ref as R
from eval_cases import SMOOTH_S as S, smooth_experiment as experiment, smooth_model as model  # noqa: F401  (fixtures: the tiny model, the saved checkpoint)

pytestmark = pytest.mark.gpu

SUMMARY = ("components", "holes", "components_density", "holes_density", "mean_area", "weighted_area", "border_fraction", "size_pdf")
DISTANCES = ("components", "holes", "size")


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_translate_minkowski_with_components_equals_the_reference(model):      # noqa: F811
    N, M, C, T = 3, 3, 3, 9
    g = torch.Generator(device="cuda").manual_seed(5)
    A = torch.rand(N, 3, S, S, device="cuda", generator=g) * 2 - 1
    z = torch.randn(N * M, 4, 1, 1, device="cuda", generator=g)
    with torch.no_grad():
        members = model.generate_multi(A, z)                       # (N M, C, S, S), input n at rows n M .. n M + M - 1
    mh = members.cpu().numpy()
    thr = np.quantile(mh.transpose(1, 0, 2, 3).reshape(C, -1).astype(np.float64), np.arange(1, T + 1) / (T + 1.0), axis=1).T.astype(np.float32)
    thr[:, 4] = thr[:, 3]
    plain = model.translate_minkowski(A, M, thr, z=z, chunk=6)
    assert set(plain) == {"members", "ens_mean"}                   # components=0: exactly what it was
    assert set(model.translate_minkowski(A, M, thr, z=z, chunk=6, components=0)) == {"members", "ens_mean"}
    mean = model.translate_ensemble(A, M, z=z)["mean"].cpu().numpy()           # the kernel's own per-pixel mean, its bits
    for conn in (8, 4):
        before = [(mod, mod.training) for mod in model.netG_A_B.modules()]
        r = model.translate_minkowski(A, M, thr, z=z, chunk=6, components=conn)     # two groups: 2 inputs, then 1
        assert all(mod.training == t for mod, t in before) and torch.is_grad_enabled()
        assert set(r) == {"members", "ens_mean", "members_comp", "ens_mean_comp"}
        assert r["members_comp"].shape == (N, M, C, T, 25) and r["ens_mean_comp"].shape == (N, C, T, 25)
        assert all(v.dtype == torch.int64 and v.is_cuda and not v.requires_grad for v in r.values())
        assert torch.equal(r["members"], plain["members"]) and torch.equal(r["ens_mean"], plain["ens_mean"])
        ref = R.stats(mh, thr, conn)
        assert np.array_equal(r["members_comp"].cpu().numpy().reshape(N * M, C, T, 25), ref)
        assert ref[..., 0].max() > 1                               # there are objects to count
        assert np.array_equal(r["ens_mean_comp"].cpu().numpy(), R.stats(mean, thr, conn))
        assert torch.equal(r["members_comp"][..., 1], r["members"][..., 0])    # the two kernels agree on the area
        for other in (model.translate_minkowski(A, M, torch.from_numpy(thr).cuda(), z=z, chunk=64, components=conn),
                      model.translate_minkowski(A, M, thr, z=z, chunk=M, components=conn)):
            for k in r:
                assert torch.equal(other[k], r[k]), k
    for bad in (1, 6, True, "8"):
        with pytest.raises(ValueError, match="components"):
            model.translate_minkowski(A, M, thr, z=z, components=bad)


def _run(experiment, capsys, res_dir, *extra):                     # noqa: F811
    from dtgan_amd import ops, test as T
    prec = ops.get_precision()
    try:
        opt = T.test_model(["--chk_path", experiment["chk"], "--dataroot", experiment["data"], "--metric", "minkowski", "--n_samples",
                            "2", "--mink_bins", "6", "--res_dir", res_dir] + list(extra))
    finally:
        ops.set_precision(prec)
    return opt, capsys.readouterr().out, dict(np.load(os.path.join(experiment["expr"], res_dir, "minkowski.npz")))


def test_metric_minkowski_with_components_writes_the_new_entries(experiment, capsys):      # noqa: F811
    from dtgan_amd import eval_metrics as EM, ops
    from dtgan_amd.dataloader import load_numpy_data
    opt0, out0, a0 = _run(experiment, capsys, "res_comp_off")
    assert opt0.mink_components == 0 and "COMP" not in out0 and "connectivity" not in a0
    assert not any(re.search(r"comp|holes|size_pdf|border|mean_area|weighted_area|connectivity", k) for k in a0)
    opt, out, a = _run(experiment, capsys, "res_comp_on", "--mink_components", "8")
    assert opt.mink_components == 8 and int(a["connectivity"]) == 8 and a["connectivity"].dtype == np.int64
    # what was there is there, the same bits: the same seed draws the same codes; the printed lines too
    assert set(a0) < set(a) and all(_same(a[k], a0[k]) for k in a0)
    mink_lines = [line for line in out0.splitlines() if "_MINK_" in line]
    assert len(mink_lines) == 2 and all(line in out.splitlines() for line in mink_lines)
    three = r"(?:\d+\.\d{6}|nan) (?:\d+\.\d{6}|nan) (?:\d+\.\d{6}|nan)"
    C, Tn, M, P = 3, 5, 2, S * S
    trainA, trainB, devA, devB, testA, testB = load_numpy_data(experiment["data"], grid_size=S)
    want = set(a0) | {"connectivity"}
    for split, fields in (("dev", (devA, devB)), ("test", (testA, testB))):
        line = re.search(r"^%s_COMP_B: (%s), %s_COMP_MEAN_B: (%s), %s_COMP_A: (%s) \(components, holes, size; 8-connected\)$"
                         % (split.upper(), three, split.upper(), three, split.upper(), three), out, re.M)
        assert line, out[-2000:]
        g = lambda name: a["%s_%s" % (split, name)]
        n = len(fields[0])
        summary = {}
        for k in EM.MINKOWSKI_SETS:
            comp = g("comp_" + k)
            want.add("%s_comp_%s" % (split, k))
            assert comp.shape == (C, Tn, 25) and comp.dtype == np.int64 and np.all(comp >= 0)
            assert np.array_equal(comp[..., 1], g("counts_" + k)[..., 0]) and np.array_equal(comp[..., 4:].sum(-1), comp[..., 0])
            rows = n * (M if k == "members_B" else 1)
            summary[k] = ops.components_summary(comp, g("counts_" + k), rows, int(g("cells_" + k)), 8)
            assert int(g("cells_" + k)) == rows * P
            for name in SUMMARY:
                want.add("%s_%s_%s" % (split, name, k))
                assert g("%s_%s" % (name, k)).dtype == np.float64 and _same(g("%s_%s" % (name, k)), summary[k][name]), (name, k)
            assert np.array_equal(g("holes_" + k), comp[..., 0] - g("euler8_" + k)) and np.all(g("holes_" + k) >= 0)
        for i, (k, real) in enumerate(EM.MINKOWSKI_PAIRS):
            d = ops.components_distance(summary[k], summary[real])
            printed = line.group(i + 1).split()
            for j, name in enumerate(DISTANCES):
                key = "dist_%s_%s" % (name, k)
                want.add("%s_%s" % (split, key))
                assert g(key).shape == (C,) and g(key).dtype == np.float64 and _same(g(key), d["dist_" + name])
                mean = np.nanmean(d["dist_" + name]) if np.isfinite(d["dist_" + name]).any() else np.nan
                assert printed[j] == "nan" and np.isnan(mean) or abs(float(printed[j]) - mean) < 1e-6
        # the int64 sums of the real sets are the reference on the split's own fields, exactly
        assert np.array_equal(g("comp_real_A"), R.stats(np.asarray(fields[0]), a["thresholds_A"], 8).sum(0))
        assert np.array_equal(g("comp_real_B"), R.stats(np.asarray(fields[1]), a["thresholds_B"], 8).sum(0))
    assert set(a) == want, sorted(set(a) ^ want)
    new = set(a) - set(a0)
    assert len(new) == 1 + 2 * (5 * (1 + len(SUMMARY)) + 3 * len(DISTANCES))
