"""GPU tests of the averaged generator weights in the models and the drivers: the training step keeps them without touching
training (eager and as a captured graph, against tests/ema_ref.py on the step's own parameter snapshots), ema_weights() runs
every forward on them and puts the live ones back, checkpoints carry them, and train.py / test.py use them."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ema_ref as E
from eval_cases import write_dataset
from model_cases import build_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECAY = 0.999
AVERAGED = {True: ["netG_A_B", "netG_B_A", "netE_B"], False: ["netG_A_B", "netG_B_A"]}


def _model(aug, tmp_path=None, **opt):
    """as tests/test_hip_step.py builds its graph models; the averages start at the recipe's parameters"""
    kw = dict(input_nc=1, output_nc=1, n_blocks=2)
    kw.update(opt)
    if tmp_path is not None:
        kw["expr_dir"] = str(tmp_path)
    m = build_model(dict(opt=kw, aug=aug, seed=5, flavour="init"))
    for _, f in m._ema:
        f.ema.copy_(f.p)
    return m


def _batches(n, seed=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for _ in range(n):
        a = torch.randn(4, 1, 64, 64, device="cuda", generator=g).clamp_(-1, 1)
        b = torch.randn(4, 1, 64, 64, device="cuda", generator=g).clamp_(-1, 1)
        out.append((a, b, torch.randn(4, 16, 1, 1, device="cuda", generator=g)))
    return out


def _flats(m):
    names = ["f_G_A_B", "f_G_B_A", "f_D_A", "f_D_B"] + (["f_E_B", "f_D_z_B"] if hasattr(m, "f_E_B") else [])
    return {k: getattr(m, k) for k in names}


class Follower(object):
    """the float64 recurrence on a model's own parameter snapshots, one per averaged network"""

    def __init__(self, m):
        self.m = m
        self.ref = {k: f.p.cpu().numpy().astype(np.float64) for k, f in m._ema}
        self.M = max(float(np.abs(r).max()) for r in self.ref.values())
        self.k = 0

    def after_step(self, what):
        self.k += 1
        for k, f in self.m._ema:
            p, e = f.p.cpu().numpy(), f.ema.cpu().numpy()
            self.ref[k] = E.ema_step(self.ref[k], p, DECAY, self.k)
            self.M = max(self.M, float(np.abs(p).max()), float(np.abs(e).max()), float(np.abs(self.ref[k]).max()))
            err, allowed = float(np.abs(e.astype(np.float64) - self.ref[k]).max()), E.bound(self.k, self.M)
            print("%s step %d %s: max |ema - e64| = %.3e, allowed %.3e (d_t = %.6f)"
                  % (what, self.k, k, err, allowed, E.decay_at(DECAY, self.k)))
            assert err <= allowed, (what, self.k, k, err, allowed)
            assert not np.array_equal(e, p)                     # an average, not a copy


@pytest.mark.parametrize("aug", [True, False])
def test_the_averages_follow_the_eager_step_and_do_not_touch_training(aug):
    plain, avg = _model(aug), _model(aug, ema_decay=DECAY)
    assert plain._ema == () and [k for k, _ in avg._ema] == AVERAGED[aug]
    assert all(not hasattr(f, "ema") for f in _flats(plain).values())
    assert sorted(k for k, f in _flats(avg).items() if hasattr(f, "ema")) == sorted("f_" + k[3:] for k in AVERAGED[aug])
    from hip_util import Spy
    follow = Follower(avg)
    for a, b, z in _batches(4):
        with Spy() as spy0:
            l0, _, g0 = plain.train_instance(a, b, z)
        with Spy() as spy1:
            l1, _, g1 = avg.train_instance(a, b, z)
        assert l0 == l1 and g0 == g1
        # the averaging off: no launch of it; on: one behind the Adam launch of each generator-side optimiser, nothing else moves
        calls0, calls1 = [n for n, _ in spy0.seen], [n for n, _ in spy1.seen]
        assert "acg_ema_multi" not in calls0 and "acg_swap_multi" not in calls0 + calls1
        assert calls1.count("acg_ema_multi") == (2 if aug else 1) and [n for n in calls1 if n != "acg_ema_multi"] == calls0
        assert all(calls1[i - 1] == "acg_clip_adam_multi" for i, n in enumerate(calls1) if n == "acg_ema_multi")
        for k, f in _flats(plain).items():
            assert torch.equal(f.p, _flats(avg)[k].p), k
        follow.after_step("eager aug=%d" % aug)


@pytest.mark.parametrize("aug", [True, False])
def test_the_averages_follow_the_replayed_step_with_the_step_number_read_on_the_device(aug):
    """two eager warm-up calls, the capture, four replays: d_t moves from 4/13 at step 3 to 8/17 at step 7, so a launch that
    kept the step number of its capture misses the bound from the second replay on"""
    m = _model(aug, ema_decay=DECAY)
    m.enable_step_graph()
    follow = Follower(m)
    for a, b, z in _batches(7):
        m.train_instance(a, b, z)
        follow.after_step("graph aug=%d" % aug)
    assert m._step_graph.captures == 1 and m._step_graph.graph is not None
    assert all(o.t == 7 for o in m._optimizers().values())


def _predict(m, a, b, z):
    with torch.no_grad():
        return m.predict_B(a, z).clone(), m.predict_A(b).clone()


@pytest.mark.parametrize("aug", [True, False])
def test_ema_weights_runs_the_averaged_model_and_restores_the_live_one(aug, tmp_path):
    m = _model(aug, tmp_path, ema_decay=DECAY)
    batches = _batches(4)
    for a, b, z in batches[:3]:
        m.train_instance(a, b, z)
    a, b, z = batches[3]
    m.save("chk")
    fresh = _model(aug, tmp_path, ema_decay=DECAY)
    fresh.load(os.path.join(str(tmp_path), "chk"), use_ema=True)
    want_B, want_A = _predict(fresh, a, b, z)
    live_B, live_A = _predict(m, a, b, z)
    assert not torch.equal(live_B, want_B) and not torch.equal(live_A, want_A)
    params = {k: f.p.clone() for k, f in _flats(m).items()}
    with m.ema_weights() as inside:
        assert inside is m
        got_B, got_A = _predict(m, a, b, z)
        with pytest.raises(RuntimeError):
            with m.ema_weights():
                pass
        with pytest.raises(RuntimeError):
            m.train_instance(a, b, z)
        if aug:
            with pytest.raises(RuntimeError):
                m.supervised_train_instance(a, b, z)
        with pytest.raises(RuntimeError):
            m.load(os.path.join(str(tmp_path), "chk"))
    assert torch.equal(got_B, want_B) and torch.equal(got_A, want_A)
    again_B, again_A = _predict(m, a, b, z)
    assert torch.equal(again_B, live_B) and torch.equal(again_A, live_A)
    for k, f in _flats(m).items():
        assert torch.equal(f.p, params[k]), k
    with pytest.raises(RuntimeError):
        with _model(aug).ema_weights():
            pass


@pytest.mark.parametrize("aug", [True, False])
def test_a_graph_model_that_enters_the_block_between_replays_equals_one_that_does_not(aug):
    visitor, twin = _model(aug, ema_decay=DECAY), _model(aug, ema_decay=DECAY)
    visitor.enable_step_graph(); twin.enable_step_graph()
    batches = _batches(6)
    for i, (a, b, z) in enumerate(batches):
        if i >= 4:                                              # between replays (calls 3 and 4 replayed the capture)
            live = _predict(visitor, a, b, z)
            with visitor.ema_weights():
                inside = _predict(visitor, a, b, z)
            assert not torch.equal(inside[0], live[0])
        lv, _, gv = visitor.train_instance(a, b, z)
        lt, _, gt = twin.train_instance(a, b, z)
        assert lv == lt and gv == gt, i
        for k, f in _flats(twin).items():
            assert torch.equal(f.p, _flats(visitor)[k].p), (i, k)
        for (k, f), (_, h) in zip(twin._ema, visitor._ema):
            assert torch.equal(f.ema, h.ema), (i, k)
    assert visitor._step_graph.captures == 1 and twin._step_graph.captures == 1


def _tensors(d, prefix=""):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(_tensors(v, "%s%s/" % (prefix, k)))
        elif torch.is_tensor(v):
            out[prefix + str(k)] = v
        elif isinstance(v, (list, tuple)):
            out.update(_tensors({i: x for i, x in enumerate(v) if isinstance(x, dict)}, "%s%s/" % (prefix, k)))
        else:
            out[prefix + str(k)] = torch.tensor(float(v)) if isinstance(v, (int, float)) else v
    return out


def _same_file(x, y):
    x, y = _tensors(x), _tensors(y)
    assert list(x.keys()) == list(y.keys())
    for k in x:
        assert torch.equal(x[k], y[k]) if torch.is_tensor(x[k]) else x[k] == y[k], k


@pytest.mark.parametrize("aug", [True, False])
def test_checkpoints_carry_the_averages(aug, tmp_path, capsys):
    chk = lambda name: os.path.join(str(tmp_path), name)
    batches = _batches(4)
    m = _model(aug, tmp_path, ema_decay=DECAY)
    for a, b, z in batches[:3]:
        m.train_instance(a, b, z)
    m.save("with")
    with m.ema_weights():
        m.save("inside")
    saved, inside = torch.load(chk("with")), torch.load(chk("inside"))
    _same_file(saved, inside)
    plain = _model(aug, tmp_path)
    for a, b, z in batches[:3]:
        plain.train_instance(a, b, z)
    plain.save("without")
    old = torch.load(chk("without"))
    assert set(old.keys()) == set(plain._net_dict()) | set(plain._optimizers())          # exactly today's keys
    assert set(saved.keys()) == set(old.keys()) | set("ema_" + k for k in AVERAGED[aug]) | {"ema_decay"}
    assert saved["ema_decay"] == DECAY
    for k in old:                                               # the reference's keys hold the live weights, unchanged
        _same_file({k: saved[k]}, {k: old[k]})
    for k, f in m._ema:                                         # a full state dict: averaged parameters, live buffers
        assert list(saved["ema_" + k].keys()) == list(saved[k].keys())
        buffers = set(n for n, _ in f.net.named_buffers())
        for name, v in saved["ema_" + k].items():
            assert v.shape == saved[k][name].shape and (name not in buffers or torch.equal(v, saved[k][name])), (k, name)
        assert torch.equal(_flat_of(saved["ema_" + k], f), f.ema) and torch.equal(_flat_of(saved[k], f), f.p), k
    # restore into a new model: the same averages, and the same ones after one more step
    capsys.readouterr()
    again = _model(aug, tmp_path, ema_decay=DECAY)
    again.load(chk("with"))
    assert "averaged" not in capsys.readouterr().out
    for (k, f), (_, h) in zip(m._ema, again._ema):
        assert torch.equal(f.ema, h.ema) and torch.equal(f.p, h.p), k
    a, b, z = batches[3]
    assert m.train_instance(a, b, z)[0] == again.train_instance(a, b, z)[0]
    for (k, f), (_, h) in zip(m._ema, again._ema):
        assert torch.equal(f.ema, h.ema), k
    # a checkpoint without averages: they start at the loaded parameters, said once; use_ema has nothing to load
    late = _model(aug, tmp_path, ema_decay=DECAY)
    late.load(chk("without"))
    said = [ln for ln in capsys.readouterr().out.splitlines() if "averaged" in ln]
    assert len(said) == 1 and all(k in said[0] for k in AVERAGED[aug]), said
    for k, f in late._ema:
        assert torch.equal(f.ema, f.p) and torch.equal(f.p, getattr(plain, "f_" + k[3:]).p), k
    for model in (late, plain):
        with pytest.raises(KeyError) as err:
            model.load(chk("without"), use_ema=True)
        assert "ema_netG_A_B" in str(err.value)
    plain.load(chk("with"))                                     # the averaging off: the keys are ignored
    assert plain._ema == () and torch.equal(plain.f_G_A_B.p, _flat_of(saved["netG_A_B"], plain.f_G_A_B))
    plain.load(chk("with"), use_ema=True)                       # ... and taken as the weights themselves when asked for
    assert torch.equal(plain.f_G_A_B.p, _flat_of(saved["ema_netG_A_B"], plain.f_G_A_B))
    assert torch.equal(plain.f_D_A.p, _flat_of(saved["netD_A"], plain.f_D_A))
    for k, f in m._ema:                                         # an `ema_<net>` entry loads as any state dict does
        f.net.load_state_dict(saved["ema_" + k])
        assert torch.equal(f.p, _flat_of(saved["ema_" + k], f)) and not torch.equal(f.p, _flat_of(saved[k], f)), k


def _flat_of(sd, f):
    out = torch.zeros_like(f.p)
    for (name, p), o in zip(f.net.named_parameters(), f.offs):
        out[o:o + p.numel()] = sd[name].reshape(-1).to(out.device)
    return out


# ------------------------------------------------------------------------------------------------------------- drivers
def _run(cmd, env, limit):
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=limit + 60)
    return p.returncode, p.stdout.decode(errors="replace")


def test_the_drivers_train_save_and_evaluate_the_averaged_weights(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    S = 64
    data = tmp_path / "data"
    write_dataset(data, (S, S), 12, 5)
    train = [sys.executable, "-m", "dtgan_amd.train", "--checkpoints_dir", str(tmp_path), "--synthetic", "8", "--grid_size", str(S),
             "--batchSize", "4", "--niter", "1", "--niter_decay", "0", "--n_blocks", "2", "--step_graph", "--ngf", "8", "--nef", "8",
             "--ndf", "8", "--nlatent", "4", "--print_freq", "4", "--display_freq", "8", "--save_epoch_freq", "1", "--eval_steps", "2",
             "--num_multi", "2", "--seed", "1"]
    rc, out = _run(train + ["--name", "avg", "--ema_decay", "0.99"], env, 900)
    assert rc == 0, out[-4000:]
    d = os.path.join(str(tmp_path), "avg")
    log = open(os.path.join(d, "results.txt")).read()
    assert re.search(r"\[1\] evaluating the averaged weights \(ema_decay 0\.99\)", log), log[-2000:]
    assert re.search(r"\[1\] DEV_MSE_A: ", log) and re.search(r"\[1\] DEV_BPP_B: ", log)
    latest = torch.load(os.path.join(d, "latest"), map_location="cpu")
    names = ["ema_netG_A_B", "ema_netG_B_A", "ema_netE_B"]
    assert all(k in latest for k in names) and latest["ema_decay"] == 0.99
    assert any(not torch.equal(v, latest["netG_A_B"][name]) for name, v in latest["ema_netG_A_B"].items())
    for best in ("best_A", "best_B"):                           # written inside the evaluation: live weights under the usual keys
        chk = torch.load(os.path.join(d, best), map_location="cpu")
        for k in ("netG_A_B", "ema_netG_A_B", "netE_B", "ema_netE_B"):
            for name, v in chk[k].items():
                if "running_" not in name and "num_batches" not in name:    # (the evaluation in between moves BatchNorm statistics)
                    assert torch.equal(v, latest[k][name]), (best, k, name)
    test = [sys.executable, "-m", "dtgan_amd.test", "--dataroot", str(data), "--metric", "mse"]
    rc, out = _run(test + ["--chk_path", os.path.join(d, "latest"), "--ema", "1"], env, 600)
    assert rc == 0, out[-4000:]
    assert "evaluating the averaged weights" in out
    averaged = re.search(r"DEV_MSE_A: (\d+\.\d{4}), TEST_MSE_A: (\d+\.\d{4})", out)
    assert averaged, out[-2000:]
    # a run without --ema_decay (its evaluation skipped): today's checkpoint, which --ema 1 refuses by name
    rc, out = _run(train + ["--name", "plain", "--eval_A_freq", "100", "--eval_B_freq", "100"], env, 900)
    assert rc == 0, out[-4000:]
    assert "averaged" not in out
    d0 = os.path.join(str(tmp_path), "plain")
    assert not any(k.startswith("ema") for k in torch.load(os.path.join(d0, "latest"), map_location="cpu"))
    rc, out = _run(test + ["--chk_path", os.path.join(d0, "latest"), "--ema", "1"], env, 600)
    assert rc != 0 and "ema_netG_A_B" in out and "is missing" in out, out[-2000:]
    assert "Traceback" not in out
