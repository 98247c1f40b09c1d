"""CPU tests of train.py --defer_scalars: the option, its dependence on --step_graph, its line in opt.txt, and the host side
of the deferred loop (the pinned upload ring, the loop's use of DeferredStep) with stand-ins for the device pieces."""
import os

import pytest
import torch

import dtgan_amd  # noqa: F401
from dtgan_amd import train as TR
from model_cases import parse_train as _parse


def test_defer_scalars_parses_and_defaults_off(tmp_path):
    assert _parse(tmp_path).defer_scalars is False
    assert _parse(tmp_path, "--step_graph").defer_scalars is False
    opt = _parse(tmp_path, "--step_graph", "--defer_scalars")
    assert opt.defer_scalars is True and opt.step_graph is True


def test_defer_scalars_without_step_graph_is_a_usage_error(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        _parse(tmp_path, "--defer_scalars")
    assert e.value.code == 2
    assert "--defer_scalars requires --step_graph" in capsys.readouterr().err


def test_opt_txt_lists_defer_scalars(tmp_path):
    opt = _parse(tmp_path, "--step_graph", "--defer_scalars")
    txt = open(os.path.join(opt.expr_dir, "opt.txt")).read().splitlines()
    assert "defer_scalars: True" in txt and "step_graph: True" in txt
    opt = _parse(tmp_path)
    assert "defer_scalars: False" in open(os.path.join(opt.expr_dir, "opt.txt")).read().splitlines()


class _Event(object):
    log = []

    def __init__(self):
        self.id = len(_Event.log)

    def record(self):
        _Event.log.append(("record", self.id))

    def synchronize(self):
        _Event.log.append(("sync", self.id))


class _Pinned(object):
    """stands in for a pinned host tensor: .pin_memory() returns itself, .to() hands back a copy of the current values"""

    def __init__(self, t):
        self.t = t

    def pin_memory(self):
        return self

    def copy_(self, src):
        self.t.copy_(src)

    def to(self, device, non_blocking=False):
        assert non_blocking
        return self.t.clone()


def test_pinned_upload_ring_waits_on_the_copy_that_last_read_a_buffer(monkeypatch):
    """three buffers per (name, shape), used in turn; the fourth upload waits on the first one's copy event and no other"""
    monkeypatch.setattr(TR.torch.cuda, "Event", _Event)
    real_empty = torch.empty
    monkeypatch.setattr(TR.torch, "empty", lambda *a, **k: _Pinned(real_empty(*a, **k)))
    _Event.log = []
    up = TR.PinnedUploads("cpu")
    vals = [torch.full((2, 4, 1, 1), float(i)) for i in range(5)]
    outs = [up("prior_z_B", v) for v in vals]
    assert all(torch.equal(o, v) for o, v in zip(outs, vals))
    ring = up.rings[("prior_z_B", (2, 4, 1, 1))]
    assert len(ring["bufs"]) == TR.PinnedUploads.SLOTS == 3
    syncs = [e for e in _Event.log if e[0] == "sync"]
    records = [e for e in _Event.log if e[0] == "record"]
    assert len(records) == 5 and syncs == [("sync", records[0][1]), ("sync", records[1][1])]
    up("sup_A", torch.zeros(3, 1, 2, 2))                 # another name has a ring of its own
    assert len(up.rings) == 2 and [e for e in _Event.log if e[0] == "sync"] == syncs


class _Deferred(TR.DeferredStep):
    def __init__(self, k, log):
        self.k, self.log, self._out = k, log, None

    def wait(self):
        self.log.append(("wait", self.k))

    def result(self):
        self.log.append(("result", self.k))
        return ({"D_A": float(self.k)}, {"real_A": self.k}, {"gnorm_G_A_B": 1.0})


class _Model(object):
    def __init__(self, log):
        self.log, self.k = log, 0

    def train_instance(self, a, b, z):
        self.k += 1
        self.log.append(("enqueue", self.k))
        if self.k <= 2:                                   # the eager warm-up steps return plain tuples
            return ({"D_A": float(self.k)}, {"real_A": self.k}, {"gnorm_G_A_B": 1.0})
        return _Deferred(self.k, self.log)


def test_deferred_loop_reads_only_logged_and_visualised_steps_and_runs_two_ahead():
    import argparse
    log = []
    tr = TR.Trainer.__new__(TR.Trainer)
    tr.opt = argparse.Namespace(nlatent=4, batchSize=1, print_freq=4, display_freq=3, monitor_gnorm=True)
    tr.model, tr.rank, tr.ws, tr.gpu, tr.sup_it, tr.upload, tr.total_steps, tr.tick = _Model(log), 0, 1, False, None, None, 0, 0.0
    batches = [{"A": torch.zeros(1, 1, 2, 2), "B": torch.zeros(1, 1, 2, 2), "n": (1, 1)} for _ in range(10)]
    tr._train_batches = lambda: iter(batches)
    seen = []
    tr._visualize = lambda real_A, visuals, epoch, it: seen.append(("vis", it, visuals["real_A"]))
    tr.log = lambda msg: seen.append(("log", msg.split("D_A: ")[1].split()[0] if "D_A" in msg else msg))
    tr.train_epoch(1)
    # visuals of step k come from step k's own result, read before step k + 1 is enqueued
    assert [(v[1], v[2]) for v in seen if v[0] == "vis"] == [(3, 3), (6, 6), (9, 9)]
    assert [v[1] for v in seen if v[0] == "log" and v[1][0].isdigit()] == ["4.000", "8.000"]
    for k in (3, 4, 6, 8, 9):
        assert log.index(("result", k)) < log.index(("enqueue", k + 1))
    assert not [e for e in log if e[0] == "result" and e[1] in (5, 7, 10)]
    # before step k is enqueued, replayed step k - 2 has completed
    for k in range(5, 11):
        assert ("wait", k - 2) in log[:log.index(("enqueue", k))]
    assert not [e for e in log if e[0] == "wait" and e[1] > 8]
