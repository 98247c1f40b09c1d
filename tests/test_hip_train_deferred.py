"""GPU tests of train.py --step_graph --defer_scalars and of the paired step on its own graph (--supervised --step_graph).

Every training run is a fresh child process under its own time limit, on the small synthetic geometry of
test_hip_train.test_train_driver_with_step_graph.  24 training images in batches of 4 are 6 steps per epoch; --print_freq 8
logs every second step and --display_freq 12 visualises every third, so steps 3 and 9 are visualised without being logged."""
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--synthetic", "24", "--grid_size", "64", "--batchSize", "4", "--ngf", "8", "--nef", "8", "--ndf", "8", "--nlatent", "4",
        "--print_freq", "8", "--display_freq", "12", "--save_epoch_freq", "1", "--eval_steps", "2", "--num_multi", "2",
        "--seed", "1"]

# the training run, then what the step graphs did: completed captures per graph
_TRAIN = r"""
import json, os, sys
import dtgan_amd
from dtgan_amd.train import Trainer
tr = Trainer(sys.argv[1:])
tr.run()
m = tr.model
caps = {k: (getattr(m, k).captures if getattr(m, k, None) is not None else None) for k in ("_step_graph", "_sup_step_graph")}
json.dump(caps, open(os.path.join(tr.opt.expr_dir, "graph_captures.json"), "w"))
"""

# host waits of one epoch of Trainer.train_epoch: stream / device synchronisations and blocking copies as the sync debug mode
# reports them, and event waits (torch.cuda.Event.synchronize, which that mode does not report) counted by a wrapper
_SYNCS = r"""
import json, sys, time, warnings
import torch
import dtgan_amd
from dtgan_amd.train import Trainer

def count(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message) for w in caught)

x, y = torch.ones(4, device="cuda"), torch.ones(4)
sees_float = count(lambda: float(x.sum()))
sees_copy = count(lambda: y.cuda())
tr = Trainer(sys.argv[1:])
waits = [0]
event_sync = torch.cuda.Event.synchronize
def counted(self):
    waits[0] += 1
    return event_sync(self)
torch.cuda.Event.synchronize = counted
tr.tick = time.time()
syncs = count(lambda: tr.train_epoch(1))
torch.cuda.Event.synchronize = event_sync
torch.cuda.synchronize()
print(json.dumps(dict(sees_float=sees_float, sees_copy=sees_copy, syncs=syncs, event_waits=waits[0],
                      steps=tr.total_steps // tr.opt.batchSize, captures=tr.model._step_graph.captures)))
"""


def _child(script, args, limit=900):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["PYTHONPATH"] = ROOT
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", script] + list(args), env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=limit + 60)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def _train(tmp_path, name, *extra):
    _child(_TRAIN, ["--name", name, "--checkpoints_dir", str(tmp_path)] + BASE + list(extra))
    d = os.path.join(str(tmp_path), name)
    return d, json.load(open(os.path.join(d, "graph_captures.json")))


_TIME = [(re.compile(r"time: \d+\.\d+"), "time: -"), (re.compile(r"TIME: \d+\.\d+"), "TIME: -"),
         (re.compile(r"Time Taken: \d+ sec"), "Time Taken: -")]


def _log(d):
    """results.txt without its timing fields"""
    text = open(os.path.join(d, "results.txt")).read()
    for pat, sub in _TIME:
        text = pat.sub(sub, text)
    return text.splitlines()


def _loss_lines(d):
    return [ln for ln in _log(d) if re.search(r"(D_A|S_A|gnorm_G_A_B): ", ln)]


def _logged_values(d):
    return [float(v) for ln in _loss_lines(d) for v in re.findall(r": ([-+\w.]+) ", ln.split(") ", 1)[-1])]


def _same_tree(a, b, where="latest"):
    import torch
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), where
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), where
        for k in a:
            _same_tree(a[k], b[k], "%s/%s" % (where, k))
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), where
        for i, (u, v) in enumerate(zip(a, b)):
            _same_tree(u, v, "%s[%d]" % (where, i))
    else:
        assert a == b, where


def _assert_same_run(d0, d1):
    import torch
    assert _log(d1) == _log(d0)
    for f in ("history_mse_A.npy", "history_ubo_B.npy"):
        assert np.array_equal(np.load(os.path.join(d0, f)), np.load(os.path.join(d1, f))), f
    _same_tree(torch.load(os.path.join(d0, "latest"), map_location="cpu"),
               torch.load(os.path.join(d1, "latest"), map_location="cpu"))
    for sub in ("train_vis_cycle", "vis_cycle"):
        names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(d0, sub, "*.png")))
        assert names and names == sorted(os.path.basename(p) for p in glob.glob(os.path.join(d1, sub, "*.png"))), sub
        for n in names:
            assert open(os.path.join(d0, sub, n), "rb").read() == open(os.path.join(d1, sub, n), "rb").read(), (sub, n)


def test_deferred_scalars_are_bit_identical_to_the_step_graph(tmp_path):
    """same seed: identical loss / gnorm lines and evaluation lines, histories, `latest` (optimiser state included) and PNGs —
    a visual taken from the next step's buffers fails the PNG comparison (steps 3 and 9 are visualised, not logged)"""
    extra = ["--niter", "2", "--niter_decay", "0", "--step_graph"]
    d0, c0 = _train(tmp_path, "graph", *extra)
    d1, c1 = _train(tmp_path, "deferred", *extra, "--defer_scalars")
    assert c1 == c0 and c0["_step_graph"] >= 1, (c0, c1)
    assert len(glob.glob(os.path.join(d1, "train_vis_cycle", "*.png"))) == 4          # steps 3, 6 of each epoch
    assert len(_loss_lines(d1)) == 2 * 3 * 2                                          # 3 logged steps per epoch, 2 lines each
    _assert_same_run(d0, d1)


def test_deferred_loop_has_no_per_step_host_waits_on_the_compute_stream(tmp_path):
    """one epoch of n and of 2n steps: the same number of stream / device synchronisations and blocking copies (the eager
    warm-up steps and the capture: a fixed count); the deliberate event waits (run-ahead bound, the prefetcher's copy event,
    the pinned prior ring) stay within three per step"""
    res = {}
    for n in (24, 48):
        out = _child(_SYNCS, ["--name", "syncs%d" % n, "--checkpoints_dir", str(tmp_path), "--synthetic", str(n)] +
                     BASE[2:] + ["--print_freq", "100000", "--display_freq", "100000", "--step_graph", "--defer_scalars"])
        res[n] = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    for n, r in res.items():
        assert r["sees_float"] >= 1, "the sync debug mode does not report float(tensor)"
        assert r["sees_copy"] >= 1, "the sync debug mode does not report a pageable .cuda() copy"
        assert r["steps"] == n // 4 and r["captures"] == 1, r
        assert 0 < r["event_waits"] <= 3 * r["steps"], r
    assert res[48]["syncs"] == res[24]["syncs"], res


def test_supervised_step_graph_matches_eager(tmp_path):
    """--supervised --step_graph, with and without --defer_scalars: the loss lines of an eager --supervised run, and both
    graphs (the unsupervised and the paired step) were captured and replayed"""
    extra = ["--niter", "1", "--niter_decay", "0", "--supervised", "--sup_frac", "0.5"]
    de, ce = _train(tmp_path, "eager", *extra)
    dg, cg = _train(tmp_path, "sup_graph", *extra, "--step_graph")
    dd, cd = _train(tmp_path, "sup_deferred", *extra, "--step_graph", "--defer_scalars")
    assert ce == {"_step_graph": None, "_sup_step_graph": None}
    assert cg == cd and cg["_step_graph"] >= 1 and cg["_sup_step_graph"] >= 1, (cg, cd)
    ref = _loss_lines(de)
    assert len([ln for ln in ref if "S_A: " in ln]) == 3
    assert _loss_lines(dg) == ref
    assert _loss_lines(dd) == ref


def test_deferred_scalars_across_the_learning_rate_change(tmp_path):
    """--niter 1 --niter_decay 2: the learning-rate decay after epoch 2 re-captures the graph; every logged value is finite and
    the deferred run is the --step_graph run, artefact for artefact"""
    extra = ["--niter", "1", "--niter_decay", "2", "--step_graph"]
    d0, c0 = _train(tmp_path, "graph", *extra)
    d1, c1 = _train(tmp_path, "deferred", *extra, "--defer_scalars")
    assert c1 == c0 and c0["_step_graph"] >= 2, (c0, c1)          # the first capture and the one behind the decay
    vals = _logged_values(d1)
    assert len(vals) >= 3 * 3 * 13 and all(np.isfinite(vals)), vals
    assert "End of epoch 3 / 3" in open(os.path.join(d1, "results.txt")).read()
    _assert_same_run(d0, d1)
