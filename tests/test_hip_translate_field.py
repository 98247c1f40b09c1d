"""GPU tests of the native-resolution paths above the two window kernels: model.translate_field / translate_field_A (one
window: predict_B / predict_A bit for bit; many windows: a composition made here from torch slices, the same generator
launches and the fp64 blend of tests/window_ref.py), the trainer's random-window step (--native_res) and
`dtgan_amd.test --metric translate`.

Bar of the composition: the tiles are the same launches on the same bits, so only the blend differs from the reference:
2e-6 absolute on values in [-1, 1] (tests/test_hip_window.py), not a convolution tolerance."""
import os

import numpy as np
import pytest
import torch

import window_ref as R
from eval_cases import make_experiment, write_dataset
from model_cases import tiny_model

pytestmark = pytest.mark.gpu

S = 16
BAR = 2e-6


@pytest.fixture(scope="module")
def model():
    return tiny_model(grid_size=S, n_blocks=1)


def _rand(*shape, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(*shape, device="cuda", generator=g) * 2 - 1


def _flags(m):
    return [(mod, mod.training) for net in m._nets() for mod in net.modules()]


def test_one_window_is_predict_B_and_predict_A_bit_for_bit(model):
    from dtgan_amd.model import eval_state
    A, B = _rand(3, 3, S, S, seed=1), _rand(3, 3, S, S, seed=2)
    z = torch.randn(3, 4, 1, 1, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    before = _flags(model)
    got_B = model.translate_field(A, 1, z=z)
    got_A = model.translate_field_A(B)
    assert all(mod.training == t for mod, t in before) and torch.is_grad_enabled()
    assert tuple(got_B.shape) == (3, 1, 3, S, S) and tuple(got_A.shape) == (3, 3, S, S)
    with eval_state(model.netG_A_B), eval_state(model.netG_B_A), torch.no_grad():
        want_B, want_A = model.predict_B(A, z), model.predict_A(B)
    assert torch.equal(got_B[:, 0], want_B) and torch.equal(got_A, want_A)
    assert float(want_B.abs().max()) > 0.01
    # two members of one field: generate_multi's order
    z2 = torch.randn(6, 4, 1, 1, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    with eval_state(model.netG_A_B), torch.no_grad():
        want = model.generate_multi(A, z2)
    assert torch.equal(model.translate_field(A, 2, z=z2).flatten(0, 1), want)


def test_many_windows_equal_a_composition_made_here(model):
    from dtgan_amd import ops
    from dtgan_amd.model import eval_state
    from dtgan_amd.modules import _starts_with_conv, as_latent
    N, M, H, W, overlap = 2, 2, 24, 36, 4
    A, B = _rand(N, 3, H, W, seed=5), _rand(N, 3, H, W, seed=6)
    z = torch.randn(N * M, 4, 1, 1, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    p = R.plan(H, W, S, overlap)
    assert (p["oy"], p["ox"]) == ([0, 8], [0, 10, 20])
    T = len(p["oy"]) * len(p["ox"])
    per = 2                                                     # canvases per generator pass: chunk 13 // 6 windows
    before = _flags(model)
    got_B = model.translate_field(A, M, z=z, overlap=overlap, chunk=2 * T + 1)
    got_A = model.translate_field_A(B, overlap=overlap, chunk=2 * T + 1)
    assert all(mod.training == t for mod, t in before) and torch.is_grad_enabled()
    assert tuple(got_B.shape) == (N, M, 3, H, W) and tuple(got_A.shape) == (N, 3, H, W)

    def compose(G, x, copies, code):
        out = []
        with eval_state(G), torch.no_grad():
            for k0 in range(0, x.size(0) * copies, per):
                ks = range(k0, min(k0 + per, x.size(0) * copies))
                wins = torch.stack([x[k // copies, :, oy:oy + S, ox:ox + S] for k in ks for oy in p["oy"] for ox in p["ox"]])
                t = ops.ToNHWC.apply(wins.contiguous(), _starts_with_conv(G.model))
                if code is None:
                    y = G.forward_nhwc(t)
                else:
                    y = G.forward_nhwc(t, as_latent(torch.stack([code[k] for k in ks for _ in range(T)])))
                out.append(R.blend(y.cpu().numpy()[..., :3], p, len(ks), 3)[0])
        return np.concatenate(out)
    want_B = compose(model.netG_A_B, A, M, model._z(z)).reshape(N, M, 3, H, W)
    want_A = compose(model.netG_B_A, B, 1, None)
    err_B = np.abs(got_B.cpu().numpy().astype(np.float64) - want_B).max()
    err_A = np.abs(got_A.cpu().numpy().astype(np.float64) - want_A).max()
    print("translate_field vs composition: max abs err B %.3g, A %.3g" % (err_B, err_A))
    assert err_B <= BAR and err_A <= BAR, (err_B, err_A)
    assert np.abs(want_B[:, 0] - want_B[:, 1]).max() > 1e-3     # the members differ: each has its own code
    # the default chunk holds every canvas in one pass; each tile is normalised on its own, so the pass size does not matter
    assert torch.equal(model.translate_field(A, M, z=z, overlap=overlap), got_B)
    # the default overlap is grid_size // 4
    assert torch.equal(model.translate_field_A(B), got_A)


def test_refusals(model):
    A = _rand(2, 3, 24, 36, seed=8)
    for bad in (_rand(1, 3, 15, 36), _rand(1, 3, 24, 15)):
        with pytest.raises(ValueError, match="smaller"):
            model.translate_field(bad)
        with pytest.raises(ValueError, match="smaller"):
            model.translate_field_A(bad)
    with pytest.raises(ValueError, match="6 windows"):
        model.translate_field(A, 1, overlap=4, chunk=5)
    with pytest.raises(ValueError, match="6 windows"):
        model.translate_field_A(A, overlap=4, chunk=5)
    with pytest.raises(ValueError, match="codes"):
        model.translate_field(A, 2, z=torch.zeros(3, 4, 1, 1, device="cuda"))
    for M in (0, 65):
        with pytest.raises(ValueError, match="n_samples"):
            model.translate_field(A, M)
    with pytest.raises(ValueError, match="overlap"):
        model.translate_field(A, 1, overlap=9)
    assert torch.is_grad_enabled()


def _train_two_steps(root, name):
    """one epoch of 2 batches (each followed by the paired step) on 72 x 80 fields whose A and B hold the same data ->
    (the inputs the four steps saw, their losses, the generator's parameters after them)"""
    from dtgan_amd.train import Trainer
    tr = Trainer(["--name", name, "--checkpoints_dir", str(root), "--dataroot", str(root / "data"), "--native_res", "--window_flip",
                  "1", "--grid_size", "64", "--batchSize", "2", "--ngf", "8", "--nef", "8", "--ndf", "8", "--nlatent", "4",
                  "--n_blocks", "1", "--seed", "11", "--supervised", "--sup_frac", "1.0", "--print_freq", "1000000",
                  "--display_freq", "1000000"])
    assert tr.train_it.data_A.shape[1:] == (3, 72, 80) and tr.dev_it.data_A.shape[1:] == (3, 64, 64)
    seen, losses = [], []
    for kind in ("train_instance", "supervised_train_instance"):
        def spy(a, b, z, real=getattr(tr.model, kind), kind=kind):
            seen.append((kind, a.clone(), b.clone()))
            out = real(a, b, z)
            losses.append(dict(out[0] if isinstance(out, tuple) else out))
            return out
        setattr(tr.model, kind, spy)
    tr.tick = 0.0
    tr.train_epoch(1)
    if tr.log_f is not None:
        tr.log_f.close()
    params = torch.cat([p.detach().reshape(-1) for p in tr.model.netG_A_B.parameters()]).clone()
    return seen, losses, params, tr


def test_trainer_cuts_random_windows_reproducibly_and_pairs_share_theirs(tmp_path):
    write_dataset(tmp_path / "data", (72, 80), n_train=8, n_test=2, same=True)
    seen, losses, params, tr = _train_two_steps(tmp_path, "one")
    assert [k for k, _, _ in seen] == ["train_instance", "supervised_train_instance"] * 2
    fields = torch.from_numpy(tr.train_it.data_A)
    for kind, a, b in seen:
        assert tuple(a.shape) == tuple(b.shape) == (2, 3, 64, 64)
        if kind == "supervised_train_instance":
            assert torch.equal(a, b)                           # one window and one flip for the pair
        else:
            assert not torch.equal(a, b)
        # every window is a (possibly mirrored) 64 x 64 cut of a stored field, bit for bit
        for w in a.cpu():
            cands = [w, w.flip(2), w.flip(1), w.flip(1, 2)]
            hit = any(torch.equal(c, f[:, oy:oy + 64, ox:ox + 64]) for c in cands for f in fields
                      for oy in range(9) for ox in range(17) if c[0, 0, 0] == f[0, oy, ox])
            assert hit
    assert all(np.isfinite(list(d.values())).all() for d in losses)
    seen2, losses2, params2, _ = _train_two_steps(tmp_path, "two")
    assert all(torch.equal(a, a2) and torch.equal(b, b2) for (_, a, b), (_, a2, b2) in zip(seen, seen2))
    assert losses == losses2 and torch.equal(params, params2)


@pytest.fixture(scope="module")
def experiment(tmp_path_factory):
    """20 x 28 fields (6 train -> 3 dev + 3 train, 2 test) and the checkpoint of a seeded 16 x 16 model"""
    return make_experiment(tmp_path_factory.mktemp("translate_driver"), S, 6, 2, hw=(20, 28), seed=1, native_res=True)


def test_metric_translate_writes_whole_fields_and_repeats(experiment, capsys):
    from dtgan_amd import ops, test as T
    prec = ops.get_precision()
    runs = []
    try:
        for res in ("res_a", "res_b"):
            T.test_model(["--chk_path", experiment["chk"], "--dataroot", experiment["data"], "--metric", "translate",
                          "--n_samples", "3", "--overlap", "5", "--res_dir", res])
            runs.append(dict(np.load(os.path.join(experiment["expr"], res, "translate.npz"))))
    finally:
        ops.set_precision(prec)
    out = capsys.readouterr().out
    assert out.count("DEV_RMSE_MEAN_B: ") == 2 and "TEST_RMSE_MEAN_B: " in out and "TEST_RMSE_A: " in out
    a, b = runs
    want = {"n_samples", "window", "overlap", "origins_y", "origins_x"}
    want |= {"%s_%s" % (s, k) for s in ("dev", "test") for k in ("mean_B", "std_B", "member0_B", "fake_A")}
    assert set(a) == want
    assert (int(a["n_samples"]), int(a["window"]), int(a["overlap"])) == (3, S, 5)
    p = R.plan(20, 28, S, 5)
    assert a["origins_y"].tolist() == p["oy"] and a["origins_x"].tolist() == p["ox"]
    for split, n in (("dev", 3), ("test", 2)):
        for k in ("mean_B", "std_B", "member0_B", "fake_A"):
            v = a["%s_%s" % (split, k)]
            assert v.shape == (n, 3, 20, 28) and v.dtype == np.float32 and np.isfinite(v).all(), (split, k)
        assert a[split + "_std_B"].min() >= 0 and a[split + "_std_B"].max() > 0
        assert np.abs(a[split + "_mean_B"]).max() <= 1 and np.abs(a[split + "_member0_B"] - a[split + "_mean_B"]).max() > 0
    assert all(np.array_equal(a[k], b[k]) for k in want)


def test_existing_metric_reads_centre_windows_for_a_native_run(experiment, capsys):
    """the saved options carry native_res: --metric mse scores the centre 16 x 16 windows of the 20 x 28 fields"""
    from dtgan_amd import ops, test as T
    from dtgan_amd.dataloader import AlignedIterator, centre_windows, load_numpy_data
    from dtgan_amd.evaluate import eval_mse_A
    prec = ops.get_precision()
    try:
        opt = T.test_model(["--chk_path", experiment["chk"], "--dataroot", experiment["data"], "--metric", "mse", "--res_dir", "res_mse"])
        out = capsys.readouterr().out
        got = float(out.split("TEST_MSE_A: ")[1].split()[0])
        arrays = load_numpy_data(experiment["data"], grid_size=S, native_res=True)
        testA, testB = arrays[4], arrays[5]
        assert testA.shape == (2, 3, S, S)
        model, _ = T._build(opt)
        model.load(experiment["chk"])
        want = eval_mse_A(AlignedIterator(testA, testB, batch_size=2), model)
    finally:
        ops.set_precision(prec)
    assert abs(got - want) < 1e-4, (got, want)
