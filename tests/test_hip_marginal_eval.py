"""GPU tests of the marginal evaluator above the C ABI: ops.marginal_scores through the real acg_field_sort in every layout
against tests/marginal_eval_ref.py (the bars of tests/test_hip_marginal_scores.py), model.translate_marginal against
ops.marginal_scores on the same translations, and `--metric marginal` in process on a saved tiny checkpoint."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import marginal_eval_ref as R
from eval_cases import make_experiment
from model_cases import tiny_model

pytestmark = pytest.mark.gpu

S = 16
KEYS = ("w", "q", "below")


def _nhwc(x, Cp=4, seed=0):
    """(rows, C, H, W) -> (rows, H, W, Cp) on the device with +-50 garbage in the padded channels"""
    rows, C, H, W = x.shape
    t = np.random.RandomState(seed).uniform(-50, 50, (rows, H, W, Cp)).astype(np.float32)
    t[..., :C] = np.moveaxis(x, 1, 3)
    return torch.from_numpy(t).cuda()


def _nchw(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()


@functools.lru_cache(maxsize=None)
def _case(H, W, kx, ky):
    """6 members against 2 truths of 3 channels, the 16 levels, 256 edges, and the reference; left unchanged"""
    x, y = R.make_fields(kx, H, W, 6, 3, seed=1), R.make_fields(ky, H, W, 2, 3, seed=2)
    edges = R.make_edges(R.sorted_values(x.reshape(6, 3, -1)), 256, seed=H)
    ref = R.scores(x, y, R.LEVELS16, edges, x_per_y=3)
    for a in (x, y, edges) + tuple(ref.values()):
        a.setflags(write=False)
    return x, y, edges, ref


def _within_the_bars(got, ref, P, what):
    assert sorted(got) == sorted(ref), what
    host = {k: v.cpu().numpy() for k, v in got.items()}
    if "below" in ref:
        assert host["below"].dtype == np.int32 and np.array_equal(host["below"], ref["below"]), what
    if "q" in ref:
        assert host["q"].dtype == np.float32 and R.ulp_distance(host["q"], ref["q"]).max() <= 1, what
    if "w" in ref:
        assert host["w"].dtype == np.float64 and np.all(np.abs(host["w"] - ref["w"]) <= P * 2.0 ** -52 * ref["w"]), what


@pytest.mark.parametrize("H, W", [(11, 13), (91, 91)])
@pytest.mark.parametrize("kx, ky", [("masked", "uniform"), ("signed_zeros", "tanh_normal")])
def test_marginal_scores_in_every_layout_through_the_real_sort(H, W, kx, ky):
    from dtgan_amd import ops
    x, y, edges, ref = _case(H, W, kx, ky)
    first = None
    for lx, ly in (("nhwc", "nhwc"), ("nchw", "nchw"), ("nhwc", "nchw"), ("nchw", "nhwc")):
        dx = _nhwc(x, seed=3) if lx == "nhwc" else _nchw(x)
        dy = _nhwc(y, seed=4) if ly == "nhwc" else _nchw(y)
        got = ops.marginal_scores(dx, dy, 3, lx, ly, R.LEVELS16, edges, x_per_y=3)
        assert got["w"].shape == (6, 3, 2) and got["q"].shape == (6, 3, 16) and got["below"].shape == (6, 3, 256)
        _within_the_bars(got, ref, H * W, (lx, ly))
        if first is None:
            first = got
        assert all(torch.equal(got[k], first[k]) for k in KEYS), (lx, ly)     # the sorted fields are planar in every layout
    alone = ops.marginal_scores(_nhwc(x), None, 3, "nhwc", None, R.LEVELS16, torch.from_numpy(np.array(edges)).cuda())
    assert sorted(alone) == ["below", "q"] and torch.equal(alone["q"], first["q"]) and torch.equal(alone["below"], first["below"])
    only_w = ops.marginal_scores(_nchw(x), _nchw(y), 3, "nchw", "nchw", x_per_y=3)
    assert sorted(only_w) == ["w"] and torch.equal(only_w["w"], first["w"])


def test_the_wrappers_refuse_before_a_launch():
    from dtgan_amd import _lib, ops
    x, y = torch.zeros(4, 3, 8, 8, device="cuda"), torch.zeros(2, 3, 8, 8, device="cuda")
    sx, _ = ops.field_sort(x, 3, "nchw", want_rank=False)
    for call, word in ((lambda: ops.marginal_scores(x, y, 3, "nchw", "nchw", x_per_y=1), "do not pair"),
                       (lambda: ops.marginal_scores(x, y, 3, "nchw", "nchw", x_per_y=3), "x_per_y"),
                       (lambda: ops.marginal_scores(x, torch.zeros(2, 3, 8, 4, device="cuda"), 3, "nchw", "nchw", x_per_y=2), "do not pair"),
                       (lambda: ops.marginal_scores(x, None, 3, "nchw", None), "nothing to compute"),
                       (lambda: ops.marginal_scores(x, None, 3, "nchw", None, (1.5,)), "inside"),
                       (lambda: ops.marginal_scores(x, None, 3, "nchw", None, [0.5] * 17), "at most 16"),
                       (lambda: ops.marginal_scores(x, None, 3, "nchw", None, (), np.zeros((2, 4), np.float32)), "edges"),
                       (lambda: ops.marginal_scores(x, None, 3, "nchw", None, (), np.zeros((3, 257), np.float32)), "edges"),
                       (lambda: ops.sorted_scores(sx, None, (0.5,), out=dict(q=torch.empty(4, 3, 2, device="cuda"))), "out"),
                       (lambda: ops.sorted_scores(sx, None, (0.5,), out=dict(w=torch.empty(4, 3, 1, device="cuda"))), "out holds"),
                       (lambda: ops.sorted_scores(sx.cpu(), None, (0.5,)), "ROCm device")):
        with pytest.raises(_lib.AcgError, match=word):
            call()


@pytest.fixture(scope="module")
def model():
    return tiny_model(grid_size=S, n_blocks=1)


def test_translate_marginal_is_marginal_scores_on_the_same_translations(model):
    from dtgan_amd import ops
    from dtgan_amd.model import _ensemble_mean, eval_state, plan_ensemble
    N, M, C = 3, 2, 3
    g = torch.Generator(device="cuda").manual_seed(5)
    A = torch.rand(N, 3, S, S, device="cuda", generator=g) * 2 - 1
    B = torch.tanh(torch.randn(N, 3, S, S, device="cuda", generator=g))
    z = torch.randn(N * M, 4, 1, 1, device="cuda", generator=g)
    levels = R.LEVELS16[:5]
    edges = torch.linspace(-1.2, 1.2, 3 * 7, device="cuda").view(3, 7).contiguous()
    before = [(mod, mod.training) for mod in model.netG_A_B.modules()]
    r = model.translate_marginal(A, M, B, levels, edges, z=z, chunk=4)           # two groups: 2 inputs, then 1
    assert all(mod.training == t for mod, t in before) and torch.is_grad_enabled()
    assert set(r) == {"members", "ens_mean", "target"} and set(r["members"]) == set(KEYS) == set(r["ens_mean"])
    assert set(r["target"]) == {"q", "below"}
    shapes = dict(w=(C, 2), q=(C, 5), below=(C, 7))
    dtypes = dict(w=torch.float64, q=torch.float32, below=torch.int32)
    for name, lead in (("members", (N, M)), ("ens_mean", (N,)), ("target", (N,))):
        for k, v in r[name].items():
            assert tuple(v.shape) == lead + shapes[k] and v.dtype == dtypes[k], (name, k)
    assert float(r["members"]["w"].min()) > 0 and bool(torch.isfinite(r["members"]["q"]).all())
    assert int(r["members"]["below"].max()) <= S * S and int(r["members"]["below"].min()) >= 0
    M_, N_, C_, H, W, zz, per = plan_ensemble("test", model.opt, A, M, z, B, 4, need_B=True)
    assert per == 2
    with eval_state(model.netG_A_B), torch.no_grad():
        for g0, n, members in model.ensemble_groups(A, zz, M, per):
            b = B[g0:g0 + n].contiguous()
            own = ops.marginal_scores(members, b, C, "nhwc", "nchw", levels, edges, x_per_y=M)
            mean = ops.marginal_scores(_ensemble_mean(members, M, C), b, C, "nchw", "nchw", levels, edges)
            tgt = ops.marginal_scores(b, None, C, "nchw", None, levels, edges)
            for k in KEYS:
                assert torch.equal(own[k].view((n, M) + shapes[k]), r["members"][k][g0:g0 + n]), k
                assert torch.equal(mean[k], r["ens_mean"][k][g0:g0 + n]), k
                if k != "w":
                    assert torch.equal(tgt[k], r["target"][k][g0:g0 + n]), k
            host = R.scores(ops.ToNCHW.apply(members, C).cpu().numpy(), b.cpu().numpy(), levels, edges.cpu().numpy(), x_per_y=M)
            _within_the_bars(own, host, S * S, "members of group %d" % g0)
    again = model.translate_marginal(A, M, B, levels, edges.cpu().numpy(), z=z, chunk=64)     # one group: the same bits
    for name in r:
        for k in r[name]:
            assert torch.equal(again[name][k], r[name][k]), (name, k)
    one = model.translate_marginal(A, 1, B, levels, edges, z=z[:N])
    for k in KEYS:
        assert torch.equal(one["members"][k][:, 0], one["ens_mean"][k]), k             # M = 1: the member itself
    with pytest.raises(ValueError, match="translate_marginal"):
        model.translate_marginal(A, M, B[:2], levels, edges, z=z)
    with pytest.raises(ValueError, match="translate_marginal"):
        model.translate_marginal(A, M, B, (), edges, z=z)
    with pytest.raises(ValueError, match="translate_marginal"):
        model.translate_marginal(A, M, B, levels, edges[:2], z=z)


@pytest.fixture(scope="module")
def experiment(tmp_path_factory):
    """a synthetic .npz split (10 train -> 5 dev + 5 train, 3 test) with mass at 0 in domain B, and the checkpoint
    <expr_dir>/latest of a seeded tiny model: the recipe of tests/test_hip_ssim_step.py at 16 x 16"""
    def field(rs, i, j, n, draw):
        f = draw()
        if j == 1:
            f[rs.uniform(size=f.shape) < 0.3] = 0.0
        return f
    return make_experiment(tmp_path_factory.mktemp("marginal_metric"), S, 10, 3, field=field)


def test_metric_marginal_writes_its_file(experiment, capsys):
    from dtgan_amd import eval_metrics as EM, ops, test as T
    prec = ops.get_precision()
    try:
        opt = T.test_model(["--chk_path", experiment["chk"], "--dataroot", experiment["data"], "--metric", "marginal", "--n_samples",
                            "2", "--marg_levels", "0,0.5,0.99,1", "--marg_bins", "10", "--res_dir", "res_marg"])
    finally:
        ops.set_precision(prec)
    assert opt.ema == 0 and opt.marg_bins == 10 and opt.marg_levels == (0.0, 0.5, 0.99, 1.0)     # --ema 0 is the default path
    out = capsys.readouterr().out
    assert re.search(r"DEV_W1_B: \d+\.\d{4}, TEST_W1_B: \d+\.\d{4}, TEST_W1_MEAN_B: ", out) and "TEST_KS_A: " in out, out[-2000:]
    a = dict(np.load(os.path.join(experiment["expr"], "res_marg", "marginal.npz")))
    C, L, E, M, P = 3, 4, 9, 2, S * S
    assert EM.MARGINAL_PAIRS == ("members_B", "ens_mean_B", "fake_A")
    assert a["levels"].dtype == np.float64 and np.array_equal(a["levels"], [0.0, 0.5, 0.99, 1.0]) and int(a["n_samples"]) == M
    for d in "BA":
        e = a["edges_" + d]
        assert e.shape == (C, E) and e.dtype == np.float32 and np.all(np.diff(e, axis=1) >= 0)
    assert np.any(np.diff(a["edges_B"], axis=1) == 0)                       # 30 % of B is exactly the minimum: repeated edges
    want = {"n_samples", "levels", "edges_B", "edges_A"}
    for split, n in (("dev", None), ("test", 3)):
        g = lambda name: a["%s_%s" % (split, name)]
        n = g("w1_members_B_per_input").shape[0] if n is None else n
        assert n >= 1
        for k in EM.MARGINAL_PAIRS:
            per_field = M if k == "members_B" else 1
            for name, shape, dtype in (("w1", (C,), np.float64), ("w2sq", (C,), np.float64), ("w1_%s_per_input", (n, C), np.float64),
                                       ("w2sq_%s_per_input", (n, C), np.float64), ("q", (C, L), np.float64),
                                       ("below", (C, E), np.int64), ("cells", (), np.int64), ("cdf", (C, E), np.float64),
                                       ("ks", (C,), np.float64)):
                key = name % k if "%s" in name else "%s_%s" % (name, k)
                want.add("%s_%s" % (split, key))
                assert g(key).shape == shape and g(key).dtype == dtype, (split, key, g(key).shape, g(key).dtype)
            assert int(g("cells_" + k)) == n * per_field * P
            assert np.allclose(g("w1_%s_per_input" % k).mean(0), g("w1_" + k), rtol=0, atol=1e-12)
            assert np.allclose(g("w2sq_%s_per_input" % k).mean(0), g("w2sq_" + k), rtol=0, atol=1e-12)
            assert np.all(g("w1_" + k) > 0) and np.all(g("w2sq_" + k) >= g("w1_" + k) ** 2 * (1 - 1e-12))   # Jensen, per field
            cdf = g("cdf_" + k)
            assert np.all(cdf >= 0) and np.all(cdf <= 1) and np.all(np.diff(cdf, axis=1) >= 0)     # the edges are sorted
            assert np.array_equal(cdf, g("below_" + k) / float(g("cells_" + k)))
            assert np.all(g("below_" + k) >= 0) and np.all(g("below_" + k) <= g("cells_" + k))
            assert np.all(g("ks_" + k) >= 0) and np.all(g("ks_" + k) <= 1)
            q = g("q_" + k)
            assert np.all(np.diff(q, axis=1) >= 0)                            # the levels ascend, so do the mean quantiles
        for d in "BA":
            want |= {"%s_%s_real_%s" % (split, name, d) for name in ("q", "below", "cells")}
            assert g("q_real_" + d).shape == (C, L) and g("q_real_" + d).dtype == np.float64
            assert g("below_real_" + d).shape == (C, E) and g("below_real_" + d).dtype == np.int64
            assert g("cells_real_" + d).dtype == np.int64 and int(g("cells_real_" + d)) == n * P
            assert np.all(g("below_real_" + d) >= 0) and np.all(g("below_real_" + d) <= g("cells_real_" + d))
            same = ops.marginal_summary(g("below_real_" + d), g("cells_real_" + d), g("below_real_" + d), g("cells_real_" + d))
            assert np.all(same["ks"] == 0.0)
        ks_B = np.abs(g("cdf_members_B") - g("below_real_B") / float(g("cells_real_B"))).max(1)
        assert np.array_equal(ks_B, g("ks_members_B"))
    assert set(a) == want, sorted(set(a) ^ want)


def test_the_real_fields_of_eval_marginal_are_numpys(experiment):
    """eval_marginal's truth entries against NumPy on the batches it was given, and ks of the truths against themselves is 0"""
    from dtgan_amd import eval_metrics as EM, ops
    rs = np.random.RandomState(7)
    A = rs.uniform(-1, 1, (4, 3, S, S)).astype(np.float32)
    B = R.make_fields("masked", S, S, 4, 3)
    levels = (0.0, 0.25, 1.0)
    edges_B, edges_A = EM.marginal_edges(B, 5), EM.marginal_edges(A, 5)

    class Model(object):                                                      # B -> A and A -> B as identities of the truths
        def translate_marginal(self, real_A, n, real_B, lv, e):
            s = ops.marginal_scores(real_B, real_B, 3, "nchw", "nchw", lv, e)
            t = {k: s[k] for k in ("q", "below")}
            return dict(members={k: v.unsqueeze(1) for k, v in s.items()}, ens_mean=s, target=t)

        def predict_A(self, real_B):
            return self.real_A

    m = Model()
    batches = [dict(A=torch.from_numpy(A[:3]), B=torch.from_numpy(B[:3])), dict(A=torch.from_numpy(A[3:]), B=torch.from_numpy(B[3:]))]

    def dataset():
        for b in batches:
            m.real_A = b["A"].cuda()
            yield b
    res = EM.eval_marginal(dataset(), m, 1, levels, edges_B, edges_A)
    for d, x, e in (("B", B, edges_B), ("A", A, edges_A)):
        ref = R.scores(x, None, levels, e)
        assert np.array_equal(res["below_real_" + d], ref["below"].sum(0, dtype=np.int64)) and int(res["cells_real_" + d]) == 4 * S * S
        assert np.allclose(res["q_real_" + d], ref["q"].astype(np.float64).mean(0), rtol=0, atol=1e-12)
    for k in EM.MARGINAL_PAIRS:                                                 # every comparison is a truth against itself
        assert np.all(res["ks_" + k] == 0.0) and np.all(res["w1_" + k] == 0.0) and np.all(res["w2sq_" + k] == 0.0), k
        assert res["w1_%s_per_input" % k].shape == (4, 3)
