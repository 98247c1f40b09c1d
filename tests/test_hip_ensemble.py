"""GPU tests of the ensemble statistics: acg_ensemble_stats against tests/ensemble_ref.py, model.translate_ensemble against
generate_multi and the reference, and `python -m dtgan_amd.test --metric ensemble` in a child process."""
import os
import re

import numpy as np
import pytest
import torch

from ensemble_ref import ensemble_stats as ref_stats
from eval_cases import checkpoint_model, S as EVAL_S, count_sync_warnings as _count_sync_warnings, experiment, png_shape as _png_shape, run_test  # noqa: F401  (the fixture)
from model_cases import ensemble_inputs as _inputs, ensemble_model as _model

pytestmark = pytest.mark.gpu

QS = (0.0, 0.05, 0.5, 0.95, 1.0)


def _members(N, M, C, Cp, npix, seed):
    """(N, M, C, npix) float32 members in [-1, 1] with ties, duplicates and saturated values, a target tied with some of
    them, and both stored NHWC with garbage in the padded channels"""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-1, 1, (N, M, C, npix)).astype(np.float32)
    x[:, :, :, :40] = np.round(x[:, :, :, :40] * 2) / 2          # coarse values: ties among members
    x[:, :, :, 40:60] = 1.0                                       # saturated: every member at +1
    x[:, : M // 2, :, 60:80] = -1.0
    if M > 1:
        x[:, 1, :, 100:200] = x[:, 0, :, 100:200]                  # duplicate members
    y = rs.uniform(-1, 1, (N, C, npix)).astype(np.float32)
    y[:, :, :40] = np.round(y[:, :, :40] * 2) / 2
    y[:, :, 40:50] = 1.0
    y[:, :, 60:70] = -1.0
    y[:, :, 100:150] = x[:, 0, :, 100:150]                         # the target tied with two members

    def nhwc(a):                                                   # (..., C, npix) -> (rows, npix, Cp), garbage padding
        rows = int(np.prod(a.shape[:-2]))
        t = rs.uniform(-50, 50, (rows, npix, Cp)).astype(np.float32)
        t[:, :, :C] = np.moveaxis(a.reshape(rows, C, npix), 1, 2)
        return torch.from_numpy(t).cuda()
    return x, y, nhwc(x), nhwc(y)


def _run(xd, yd, N, M, C, npix, qs, scored=True):
    from dtgan_amd import ops
    x = xd.reshape(N * M, npix, 1, -1)
    y = yd.reshape(N, npix, 1, -1) if scored else None
    out = ops.ensemble_stats(x, y, M, C, qs)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("M", [1, 2, 7, 16, 33, 64])
@pytest.mark.parametrize("C,Cp", [(1, 4), (3, 4), (3, 16)])
def test_kernel_matches_reference(M, C, Cp):
    N, npix = 2, 1031
    x, y, xd, yd = _members(N, M, C, Cp, npix, seed=M * 10 + C + Cp)
    got = _run(xd, yd, N, M, C, npix, QS)
    ref = ref_stats(x[..., None], y[..., None], QS)                 # H = npix, W = 1
    for k in ("mean", "std", "quantiles", "crps_map"):
        assert np.allclose(got[k].reshape(ref[k].shape), ref[k], rtol=0, atol=1e-6), (k, np.abs(got[k].reshape(ref[k].shape) - ref[k]).max())
    assert np.allclose(got["sums"], ref["sums"], rtol=1e-5, atol=1e-5), (got["sums"], ref["sums"])
    assert np.array_equal(got["rank_hist"], ref["rank_hist"])
    again = _run(xd, yd, N, M, C, npix, QS)
    for k in got:
        assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), k
    bare = _run(xd, yd, N, M, C, npix, QS, scored=False)             # no target: the maps alone, the same bits
    assert set(bare) == {"mean", "std", "quantiles"}
    for k in bare:
        assert np.array_equal(bare[k], got[k]), k


def test_kernel_refuses_bad_arguments_before_launching():
    from dtgan_amd import _lib, ops
    _, _, xd, yd = _members(1, 8, 3, 4, 64, seed=0)
    x = xd.reshape(8, 64, 1, 4)
    for M, qs in ((65, (0.5,)), (8, tuple(np.linspace(0, 1, 9)))):
        out = ops.ensemble_outputs(1, 8, 3, 64, 1, 1, True, x.device)
        sentinel = {k: v.clone() for k, v in out.items()}
        levels = (_lib.ctypes.c_float * len(qs))(*qs)
        lib = _lib.load()
        rc = lib.acg_ensemble_stats(ops._ptr(x), ops._ptr(yd), 1, M, 64, 3, 4, levels, len(qs), ops._ptr(out["mean"]),
                                    ops._ptr(out["std"]), ops._ptr(out["quantiles"]), ops._ptr(out["crps_map"]),
                                    ops._ptr(out["sums"]), ops._ptr(out["rank_hist"]), None, 0, ops._stream())
        assert rc == -1 and lib.acg_last_error().decode().startswith("acg_ensemble_stats")
        torch.cuda.synchronize()
        for k in out:
            assert torch.equal(out[k], sentinel[k]), k                 # nothing was written


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_translate_ensemble_equals_generate_multi_and_the_reference(prec):
    from hip_util import precision
    from dtgan_amd import ops
    N, M = 3, 5
    with precision(prec):
        m = _model()
        A, B, g = _inputs(N)
        z = torch.randn(N * M, m.opt.nlatent, 1, 1, device="cuda", generator=g)
        r = m.translate_ensemble(A, M, z=z, real_B=B, quantiles=QS)
        with torch.no_grad():
            members = m.generate_multi(A, z)
        x = ops.ToNHWC.apply(members, True)
        direct = ops.ensemble_stats(x, ops.ToNHWC.apply(B, True), M, 3, QS)
        for k in ("mean", "std", "quantiles", "crps_map"):        # the same members, bit for bit
            assert torch.equal(r[k], direct[k]), k
        ref = ref_stats(members.cpu().numpy().reshape(N, M, 3, 64, 64), B.cpu().numpy(), QS)
        for k in ("mean", "std", "quantiles", "crps_map"):
            assert np.allclose(r[k].cpu().numpy(), ref[k], rtol=0, atol=1e-6), k
        for k in ("crps", "crps_fair", "mse_mean", "spread", "coverage"):
            assert np.allclose(r[k].cpu().numpy(), ref[k], rtol=1e-5, atol=1e-7), k
        assert np.array_equal(r["rank_hist"].cpu().numpy(), ref["rank_hist"])
        one = m.translate_ensemble(A, M, z=z, real_B=B, quantiles=QS, chunk=M)     # one input per group
        for k in r:
            assert torch.equal(r[k], one[k]) or (k == "crps_fair" and torch.allclose(r[k], one[k])), k


def test_cycle_gan_gives_a_degenerate_ensemble():
    N, M = 2, 6
    m = _model("cycle_gan")
    A, B, _ = _inputs(N, seed=5)
    r = m.translate_ensemble(A, M, real_B=B)
    with torch.no_grad():
        one = m.predict_B(A, torch.zeros(N, m.opt.nlatent, 1, 1, device="cuda"))
    assert torch.equal(r["std"], torch.zeros_like(r["std"])) and torch.equal(r["mean"], one)
    assert torch.allclose(r["crps_map"], (one - B).abs(), atol=1e-6)
    hist = r["rank_hist"].cpu().numpy()
    assert hist.sum() == N * 3 * 64 * 64
    assert set(np.nonzero(hist.sum(0))[0]) <= {0, M // 2, M}


def test_translate_ensemble_host_syncs_do_not_grow_with_groups():
    m = _model()
    A, B, _ = _inputs(4, seed=7)
    M = 3
    m.translate_ensemble(A, M, real_B=B)                           # warm-up
    n1 = _count_sync_warnings(lambda: m.translate_ensemble(A, M, real_B=B))
    n4 = _count_sync_warnings(lambda: m.translate_ensemble(A, M, real_B=B, chunk=M))
    assert n1 == n4 and n1 <= 1, (n1, n4)


def test_translate_ensemble_refusals():
    m = _model()
    A, B, _ = _inputs(2)
    with pytest.raises(ValueError, match="n_samples"):
        m.translate_ensemble(A, 65)
    with pytest.raises(ValueError, match="codes"):
        m.translate_ensemble(A, 2, z=torch.zeros(3, m.opt.nlatent, 1, 1, device="cuda"))
    with pytest.raises(ValueError, match="cannot hold"):
        m.translate_ensemble(A, 4, chunk=3)
    with pytest.raises(ValueError, match="does not pair"):
        m.translate_ensemble(A, 2, real_B=B[:1])
    with pytest.raises(ValueError, match="sorted"):
        m.translate_ensemble(A, 2, quantiles=(0.9, 0.1))


def _translate_calls(m, A, B, M):
    thr, win = np.zeros((3, 2), np.float32), (1, 3)
    return dict(ensemble=lambda **kw: m.translate_ensemble(A, M, real_B=B, **kw),
                spectrum=lambda **kw: m.translate_spectrum(A, M, real_B=B, **kw),
                coherence=lambda **kw: m.translate_coherence(A, M, B, **kw),
                fss=lambda **kw: m.translate_fss(A, M, B, thr, win, **kw))


@pytest.mark.parametrize("which", ["ensemble", "spectrum", "coherence", "fss"])
def test_flags_and_grad_mode_survive_a_raising_consumer(which, monkeypatch):
    """every translate_* leaves the generator's .training flags and the grad mode as it found them: after a normal call from
    either state, and when the consumer of a group raises (a host-side exception in place of ops.ensemble_stats) with
    further groups still to come"""
    from dtgan_amd import ops
    m = _model()
    G = m.netG_A_B
    M = 2
    A, B, _ = _inputs(3, seed=9)
    call = _translate_calls(m, A, B, M)[which]
    assert torch.is_grad_enabled()
    for state in (True, False):
        G.train(state)
        call(chunk=M)                                              # three groups
        assert all(mod.training is state for mod in G.modules()) and torch.is_grad_enabled()
    G.train()

    def boom(*a, **kw):
        raise RuntimeError("consumer failed")
    monkeypatch.setattr(ops, "ensemble_stats", boom)
    with pytest.raises(RuntimeError, match="consumer failed"):
        call(chunk=M)
    assert all(mod.training is True for mod in G.modules())
    assert torch.is_grad_enabled()


def test_metric_ensemble(experiment):
    S = EVAL_S
    from dtgan_amd import eval_metrics as EM
    from dtgan_amd.dataloader import AlignedIterator, load_numpy_data
    out = run_test(experiment, "ensemble", "--n_samples", "4", "--res_dir", "res_ensemble")
    pat = r"^DEV_CRPS_B: (\d+\.\d{4}), TEST_CRPS_B: (\d+\.\d{4}), TEST_MSE_MEAN_B: (\d+\.\d{4}), TEST_SPREAD_B: (\d+\.\d{4}), " \
          r"TEST_COVERAGE_B: (\d+\.\d{4})$"
    mt = re.search(pat, out, re.M)
    assert mt, out[-2000:]
    res = os.path.join(experiment["expr"], "res_ensemble")
    arr = np.load(os.path.join(res, "ensemble.npz"))
    assert int(arr["n_samples"]) == 4 and tuple(arr["quantiles"]) == (0.05, 0.5, 0.95)
    for split, n in (("dev", 6), ("test", 5)):
        for k in ("crps", "crps_fair", "mse_mean", "spread", "coverage"):
            assert arr["%s_%s" % (split, k)].shape == (n,), (split, k)
        h = arr["%s_rank_hist" % split]
        assert h.shape == (5,) and h.sum() == n * 3 * S * S
    assert _png_shape(os.path.join(res, "ensemble_0.png")) == (2 + 6 * (S + 2), 2 + 6 * (S + 2))
    # the same numbers in process, from the same seed
    with checkpoint_model(experiment) as model:
        _, _, devA, devB, testA, testB = load_numpy_data(experiment["data"], grid_size=S)
        torch.manual_seed(12345)
        EM.eval_ensemble_B(AlignedIterator(devA, devB, batch_size=len(devA)), model, 4, (0.05, 0.5, 0.95))
        test, _ = EM.eval_ensemble_B(AlignedIterator(testA, testB, batch_size=len(testA)), model, 4, (0.05, 0.5, 0.95))
    assert abs(float(mt.group(2)) - test["crps"].mean()) < 1e-4, (mt.group(2), test["crps"].mean())
    assert np.allclose(arr["test_crps"], test["crps"], rtol=1e-6)

