"""GPU tests of the per-cell statistics above the C ABI: model.translate_ensemble(cell_stats=...) against
tests/cell_stats_ref.py on the members generate_multi gives for the same codes, model.translate_cell_stats_A against the
reference, and `--metric ensemble --ens_maps 1` on a saved tiny checkpoint (test_model, what `python -m dtgan_amd.test`
runs): the keys, shapes and dtypes of ensemble_maps.npz beside an ensemble.npz and a printed line that keep their bytes."""
import os
import re

import numpy as np
import pytest
import torch

import cell_stats_ref as R
from eval_cases import SMOOTH_S as S, smooth_experiment as experiment, smooth_model as model  # noqa: F401  (fixtures: the tiny model, the saved checkpoint)

pytestmark = pytest.mark.gpu

PARTS = ("mom", "evt", "hist_x", "hist_y")
MAPS3 = ("mean_x", "mean_y", "bias", "std_x", "std_y", "std_ratio", "corr", "rmse", "mae", "rmse_mean", "corr_mean", "spread", "spread_skill")
MAPS_T = ("freq_x", "freq_y", "freq_bias", "brier", "hit_rate", "csi")


def _host(state):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in state.items()}


def test_translate_ensemble_cell_stats_equals_the_reference_on_generate_multis_members(model):      # noqa: F811
    from dtgan_amd import ops
    N, M, C, T, E = 3, 3, 3, 2, 5
    g = torch.Generator(device="cuda").manual_seed(5)
    A = torch.rand(N, 3, S, S, device="cuda", generator=g) * 2 - 1
    B = torch.rand(N, 3, S, S, device="cuda", generator=g) * 2 - 1
    z = torch.randn(N * M, 4, 1, 1, device="cuda", generator=g)
    with torch.no_grad():
        members = model.generate_multi(A, z)                       # (N M, C, S, S), input n at rows n M .. n M + M - 1
    mh, Bh = members.cpu().numpy(), B.cpu().numpy()
    flat = mh.transpose(1, 0, 2, 3).reshape(C, -1).astype(np.float64)
    thr = np.quantile(flat, (0.5, 0.9), axis=1).T.astype(np.float32)
    edges = np.quantile(flat, (0.1, 0.3, 0.5, 0.7, 0.9), axis=1).T.astype(np.float32)
    ref = R.accumulate(R.new_state(C, S, S, T, E), mh, Bh, M, thr, edges)
    plain = model.translate_ensemble(A, M, z=z, real_B=B)
    before = [(mod, mod.training) for mod in model.netG_A_B.modules()]
    rng = torch.cuda.get_rng_state()
    state = ops.cell_state(C, S, S, T, E, "cuda")
    r = model.translate_ensemble(A, M, z=z, real_B=B, chunk=2 * M, cell_stats=(state, thr, edges))      # groups of two inputs and of one
    assert torch.equal(torch.cuda.get_rng_state(), rng)            # no random draw of its own
    assert all(mod.training == t for mod, t in before) and torch.is_grad_enabled()
    assert set(r) == set(plain)
    assert all(r[k].cpu().numpy().tobytes() == plain[k].cpu().numpy().tobytes() for k in plain)      # what was there keeps its bits
    got = _host(state)
    assert got["n"] == N and got["M"] == M and R.same_state(got, ref)
    assert np.all(got["hist_x"].sum(1) == N * M) and np.all(got["hist_y"].sum(1) == N) and 0 < got["evt"][:, :, 2].sum()
    one = ops.cell_state(C, S, S, T, E, "cuda")                    # one group, device tables: the same bits
    model.translate_ensemble(A, M, z=z, real_B=B, cell_stats=(one, torch.from_numpy(thr).cuda(), torch.from_numpy(edges).cuda()))
    assert all(one[k].cpu().numpy().tobytes() == got[k].tobytes() for k in PARTS)
    with pytest.raises(ValueError, match="real_B"):
        model.translate_ensemble(A, M, z=z, cell_stats=(state, thr, edges))
    # B -> A: the deterministic generator, one member, groups of two and one
    with torch.no_grad():
        pa = model.predict_A(B).cpu().numpy()
    sa = ops.cell_state(C, S, S, T, 0, "cuda")
    before = [(mod, mod.training) for mod in model.netG_B_A.modules()]
    assert model.translate_cell_stats_A(B, A, sa, thr, None, chunk=2) is sa
    assert all(mod.training == t for mod, t in before) and torch.equal(torch.cuda.get_rng_state(), rng)
    assert R.same_state(_host(sa), R.accumulate(R.new_state(C, S, S, T, 0), pa, A.cpu().numpy(), 1, thr, None))


def _run(experiment, capsys, res_dir, *extra):      # noqa: F811
    from dtgan_amd import ops, test as T
    prec = ops.get_precision()
    try:
        opt = T.test_model(["--chk_path", experiment["chk"], "--dataroot", experiment["data"], "--metric", "ensemble", "--n_samples", "3",
                            "--res_dir", res_dir] + list(extra))
    finally:
        ops.set_precision(prec)
    return opt, capsys.readouterr().out, os.path.join(experiment["expr"], res_dir)


def test_metric_ensemble_with_maps_writes_a_file_of_its_own(experiment, capsys):      # noqa: F811
    from dtgan_amd import eval_metrics as EM, ops
    from dtgan_amd.dataloader import load_numpy_data
    opt0, out0, dir0 = _run(experiment, capsys, "res_maps_off")
    assert opt0.ens_maps == 0 and "_MAP_" not in out0 and "ensemble_maps.npz" not in os.listdir(dir0)
    opt, out, res = _run(experiment, capsys, "res_maps", "--ens_maps", "1", "--map_quantiles", "0.9,0.5", "--map_bins", "8", "--map_levels", "0.5,0.9")
    assert opt.ens_maps == 1 and opt.map_quantiles == (0.5, 0.9) and opt.map_bins == 8
    # what was there is there, the same bytes: the arrays of the file in their order (the archive itself carries the time it
    # was written), the grid and the printed line
    f0, f1 = dict(np.load(os.path.join(dir0, "ensemble.npz"))), dict(np.load(os.path.join(res, "ensemble.npz")))
    assert list(f0) == list(f1) and all(f0[k].dtype == f1[k].dtype and f0[k].shape == f1[k].shape and f0[k].tobytes() == f1[k].tobytes() for k in f0)
    assert open(os.path.join(dir0, "ensemble_0.png"), "rb").read() == open(os.path.join(res, "ensemble_0.png"), "rb").read()
    crps_lines = [line for line in out0.splitlines() if "DEV_CRPS_B" in line]
    assert len(crps_lines) == 1 and crps_lines[0] in out.splitlines()
    num = r"(?:-?\d+\.\d{4}|nan)"
    four = " ".join([num] * 4)
    line = re.search(r"^DEV_MAP_B: (%s), TEST_MAP_B: (%s) \(domain means" % (four, four), out, re.M)
    assert line, out[-2000:]
    a = dict(np.load(os.path.join(res, "ensemble_maps.npz")))
    C, T, M, nb, L = 3, 2, 3, 8, 2
    trainA, trainB, devA, devB, testA, testB = load_numpy_data(experiment["data"], grid_size=S)
    assert int(a["n_samples"]) == M and a["levels"].tolist() == [0.5, 0.9]
    assert np.array_equal(a["thresholds_B"], EM.fss_thresholds(trainB, (0.5, 0.9))) and np.array_equal(a["thresholds_A"], EM.fss_thresholds(trainA, (0.5, 0.9)))
    assert np.array_equal(a["edges_B"], EM.marginal_edges(trainB, nb)) and np.array_equal(a["edges_A"], EM.marginal_edges(trainA, nb))
    want = {"n_samples", "levels", "thresholds_B", "thresholds_A", "edges_B", "edges_A"}
    shapes = dict(mom=(9, C, S, S), evt=(C, T, 4, S, S), hist_x=(C, nb, S, S), hist_y=(C, nb, S, S), cdf_x=(C, nb - 1, S, S), cdf_y=(C, nb - 1, S, S),
                  q_x=(C, L, S, S), q_y=(C, L, S, S), n=(), members=())
    shapes.update((k, (C, T, S, S)) for k in MAPS_T)
    dtypes = dict(mom=np.float64, evt=np.int64, hist_x=np.int32, hist_y=np.int32, n=np.int64, members=np.int64)
    for split, n in (("dev", len(devA)), ("test", len(testA))):
        want.add(split + "_crps_B")
        assert a[split + "_crps_B"].shape == (C, S, S) and a[split + "_crps_B"].dtype == np.float64 and np.all(a[split + "_crps_B"] >= 0)
        for k in EM.MAP_PAIRS:
            Mk = M if k == "members_B" else 1
            d = k[-1]
            for s in PARTS + ("n", "members") + MAPS3 + MAPS_T + ("cdf_x", "cdf_y", "ks", "q_x", "q_y"):
                key = "%s_%s_%s" % (split, s, k)
                want.add(key)
                assert a[key].shape == shapes.get(s, (C, S, S)) and a[key].dtype == dtypes.get(s, np.float64), key
            get = lambda s: a["%s_%s_%s" % (split, s, k)]
            assert int(get("n")) == n and int(get("members")) == Mk
            assert np.all(get("hist_x").sum(1) == n * Mk) and np.all(get("hist_y").sum(1) == n)
            assert np.all(get("evt")[:, :, 0] <= n * Mk) and np.all(get("evt")[:, :, 1] <= n) and get("evt").min() >= 0
            state = dict(mom=get("mom"), evt=get("evt"), hist_x=get("hist_x"), hist_y=get("hist_y"), n=n, M=Mk)
            again = ops.cell_summary(state, a["thresholds_" + d], a["edges_" + d], (0.5, 0.9))
            assert set(again) == set(MAPS3 + MAPS_T + ("cdf_x", "cdf_y", "ks", "q_x", "q_y"))
            assert all(np.array_equal(get(s), again[s], equal_nan=True) for s in again)
            assert np.all(np.isnan(get("spread"))) == (Mk == 1)
    assert set(a) == want, sorted(set(a) ^ want)
    # the per-input CRPS of ensemble.npz is the domain mean of the per-cell one
    e = dict(np.load(os.path.join(res, "ensemble.npz")))
    assert abs(a["test_crps_B"].mean() - e["test_crps"].mean()) < 1e-5 * max(e["test_crps"].mean(), 1e-3)
    vals = [f(a[split + "_%s_members_B" % s]) for split in ("dev", "test")
            for s, f in (("bias", lambda v: np.abs(v).mean()), ("rmse_mean", np.mean), ("spread_skill", np.nanmean), ("brier", lambda v: v[:, -1].mean()))]
    for p, v in zip(line.group(1).split() + line.group(2).split(), vals):
        assert p == "nan" and np.isnan(v) or abs(float(p) - v) < 1e-4, (p, v)
    # the parts can be switched off
    _, out2, res2 = _run(experiment, capsys, "res_maps_bare", "--ens_maps", "1", "--map_quantiles", "none", "--map_bins", "0", "--n_samples", "1")
    b = dict(np.load(os.path.join(res2, "ensemble_maps.npz")))
    assert not any(k.split("_")[1] in ("evt", "hist", "brier", "cdf", "ks", "q") for k in b if k[:4] in ("dev_", "test")) and "thresholds_B" not in b
    assert b["test_mom_members_B"].shape == (9, C, S, S) and np.all(np.isnan(b["test_spread_members_B"])) and "DEV_MAP_B" in out2
    _, _, res3 = _run(experiment, capsys, "res_maps_thr", "--ens_maps", "1", "--map_thresholds", "2.0,1.0", "--map_bins", "0")
    c = dict(np.load(os.path.join(res3, "ensemble_maps.npz")))
    assert c["thresholds_B"].tolist() == [[1.0, 2.0]] * C and c["dev_evt_fake_A"].shape == (C, 2, 4, S, S) and "dev_hist_x_fake_A" not in c
