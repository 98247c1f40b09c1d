"""CPU tests of what the evaluator's metrics share: the table of records (eval_metrics.METRICS) against the parser and
test.py's documentation, the option merge of test_model, ops.channel_table on host inputs and the split accumulator."""
import argparse

import numpy as np
import pytest
import torch

import dtgan_amd  # noqa: F401
from dtgan_amd import _lib, eval_metrics as EM, ops, options as O, test as T

BASE = ["--chk_path", "c/latest", "--dataroot", "d"]


def test_the_table_names_the_parsers_metrics_in_order(capsys):
    names = [m.name for m in EM.METRICS]
    assert names == ["ensemble", "spectrum", "coherence", "fss", "translate", "field_spectrum", "ssim", "marginal", "minkowski"]
    assert O.REFERENCE_METRICS == ("bpp", "mse", "visual", "noise_sens", "mvgauss")
    (metric,) = [a for a in O.TestOptions().parser._actions if a.dest == "metric"]
    assert list(metric.choices) == list(O.REFERENCE_METRICS) + names
    for name in metric.choices:
        assert O.TestOptions().parse(BASE + ["--metric", name]).metric == name
    with pytest.raises(SystemExit):
        O.TestOptions().parse(BASE + ["--metric", "energy"])
    assert "invalid choice: 'energy'" in capsys.readouterr().err
    (n_samples,) = [a for a in O.TestOptions().parser._actions if a.dest == "n_samples"]
    assert n_samples.help == "--metric " + " / ".join(names) + ": translations per input (1..64)"


def test_every_record_is_documented_and_batched_as_the_driver_did():
    assert "--metric " + "|".join(O.REFERENCE_METRICS + tuple(m.name for m in EM.METRICS)) + "\n" in T.__doc__
    at = [T.__doc__.index(m.doc) for m in EM.METRICS]               # every paragraph, whole, in the table's order
    assert at == sorted(at)
    for m in EM.METRICS:
        assert m.doc.startswith("  %s " % m.name) and "(new)" in m.doc and not m.doc.endswith("\n")
        assert callable(m.prepare) and callable(m.report)
    assert {m.name for m in EM.METRICS if m.whole_field} == {"translate", "field_spectrum"}
    assert EM.WHOLE_FIELD_METRICS == ("translate", "field_spectrum")
    assert {m.name: m.batch_size for m in EM.METRICS} == dict(
        dict.fromkeys(("ensemble", "spectrum", "coherence", "fss", "ssim", "marginal", "minkowski"), 200), translate=8, field_spectrum=8)
    assert {m.name: m.dtype for m in EM.METRICS if m.dtype is not None} == dict(spectrum=np.float64, ssim=np.float64, translate=np.float32)


def test_the_parsed_options_go_on_top_of_the_saved_ones():
    args = O.TestOptions().parse(BASE + ["--metric", "fss", "--n_samples", "3"])
    saved = dict(n_samples=99, ngf=8, gpu_ids=[0, 1], dataroot="elsewhere", metric=None)
    opt = T._merged_options(saved, args)
    assert isinstance(opt, argparse.Namespace) and opt.n_samples == 3 and opt.ngf == 8
    assert all(getattr(opt, k) == v for k, v in vars(args).items())      # every parsed key, as parsed
    assert set(vars(opt)) == set(vars(args)) | {"ngf"}
    assert saved["n_samples"] == 99 and args.n_samples == 3         # neither input is written to


ORDERED_BAD = (np.zeros((2, 2), np.float32), np.zeros(2, np.float32), np.zeros((1, 256), np.float32), np.zeros((1, 0), np.float32),
               np.array([[1.0, 0.0]]), np.array([[0.0, np.nan]]), np.array([[0.0, np.inf]]))


@pytest.mark.parametrize("error", [_lib.AcgError, ValueError])
def test_channel_table_on_host_inputs(error):
    table = lambda t, **kw: ops.channel_table("who", error, "thresholds", t, 1, 255, None, **kw)
    for bad in ORDERED_BAD:
        with pytest.raises(error, match="who: thresholds"):
            table(bad, ordered=True)
    assert table(np.array([[1.0, 0.0]])).tolist() == [[1.0, 0.0]]   # the order is checked only where it is asked for
    ok = table([[0.0, 0.0, 1.0]], ordered=True)
    assert ok.dtype == torch.float32 and tuple(ok.shape) == (1, 3) and ok.is_contiguous() and ok.device.type == "cpu"
    assert tuple(table(np.zeros((1, 255)), ordered=True).shape) == (1, 255)
    # no columns: "none" for the marginal edges, refused where a threshold is needed
    edges = lambda t, **kw: ops.channel_table("who", error, "edges", t, 3, 256, None, **kw)
    assert edges(np.zeros((3, 0), np.float32), none_if_empty=True) is None
    with pytest.raises(error, match="edges must be"):
        edges(np.zeros((3, 0), np.float32))
    with pytest.raises(error, match="edges must be"):
        edges(np.zeros((3, 257), np.float32), none_if_empty=True)
    with pytest.raises(error, match="edges must be"):
        edges(np.zeros((2, 4), np.float32), none_if_empty=True)
    # tensors: the shape, and float32 unless the caller has them cast; nothing else is looked at
    for bad in (torch.zeros(3, 4, dtype=torch.float64), torch.zeros(2, 4), torch.zeros(3, 257), torch.zeros(12)):
        with pytest.raises(error, match="who: edges"):
            edges(bad)
    cast = edges(torch.ones(3, 4, dtype=torch.float64), cast=True)
    assert cast.dtype == torch.float32 and cast.tolist() == [[1.0] * 4] * 3
    t = torch.tensor([[1.0, 0.0, float("nan")]] * 3)
    assert edges(t, ordered=True).data_ptr() == t.data_ptr()        # taken as it is: its order is the caller's contract
    assert edges(t.t().contiguous().t()).is_contiguous()
    # a read-only host array is accepted and copied, not aliased
    host = np.linspace(-1, 1, 12, dtype=np.float32).reshape(3, 4)
    host.setflags(write=False)
    got = edges(host, ordered=True)
    assert np.array_equal(got.numpy(), host) and not np.shares_memory(got.numpy(), host)
    got[0, 0] = 5.0
    assert host[0, 0] == -1.0


def test_check_thresholds_and_the_ops_name_their_caller():
    with pytest.raises(ValueError, match="check_thresholds: thresholds"):
        ops.check_thresholds(np.zeros((1, 0)), 1)
    with pytest.raises(_lib.AcgError, match="fss: thresholds"):
        ops.fss(torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, 8, 8), 1, "nchw", "nchw", np.zeros((1, 9), np.float32), (1, 3))
    with pytest.raises(_lib.AcgError, match="sorted_scores: edges must be"):
        ops.sorted_scores(torch.zeros(2, 3, 16), None, (0.5,), np.zeros((2, 4), np.float32))
    with pytest.raises(_lib.AcgError, match=r"out\['q'\]"):
        ops.sorted_scores(torch.zeros(2, 3, 16), None, (0.5,), out=dict(q=torch.zeros(2, 3, 1, dtype=torch.float64)))
    with pytest.raises(_lib.AcgError, match="ens .* int64"):
        ops.fss(torch.zeros(4, 1, 8, 8), torch.zeros(2, 1, 8, 8), 1, "nchw", "nchw", np.zeros((1, 2), np.float32), (1, 3), x_per_y=2,
                ensemble=True, out=(torch.zeros(4, 1, 2, 2, 3, dtype=torch.int64), torch.zeros(2, 1, 2, 2, 3)))


def test_the_accumulator_sums_in_int64_and_float64_batch_by_batch():
    rs = np.random.RandomState(0)
    counts = [np.full((3, 2, 4), 2 ** 31 - 1 - k, dtype=np.int32) for k in range(2)]
    acc = EM._Sum()
    for c in counts:
        acc.add(c, cells_per_row=10)
    assert acc.total.dtype == np.int64 and acc.total.shape == (2, 4) and np.all(acc.total == 3 * (2 ** 32 - 3))
    assert (acc.rows, acc.cells) == (6, 60)
    batches = [rs.standard_normal((5, 3, 7)).astype(np.float32) * 1e3 for _ in range(3)]
    acc, want = EM._Sum(), 0.0
    for b in batches:
        acc.add(b)
        want = want + np.sum(b, axis=0, dtype=np.float64)
    assert acc.total.dtype == np.float64 and np.array_equal(acc.total, want) and (acc.rows, acc.cells) == (15, 0)
    assert not np.array_equal(acc.total, np.sum(np.concatenate(batches), axis=0))      # float32 sums would differ
    # leading axes in front of the kept ones are rows; a batch summed beforehand counts the rows it stands for
    acc = EM._Sum()
    acc.add(np.ones((2, 3, 4, 5), np.int32), cells_per_row=7, keep=2)
    acc.add(np.full((1, 4, 5), 9, np.int64), cells_per_row=7, rows=9)
    assert np.all(acc.total == 15) and acc.total.shape == (4, 5) and (acc.rows, acc.cells) == (15, 105)


def test_domain_tables_are_made_once_on_the_fields_devices():
    seen = []

    def check(table, C):
        seen.append(C)
        return ops.check_thresholds(table, C)
    B, A = torch.zeros(2, 3, 4, 4), torch.zeros(2, 1, 4, 4)
    tables = EM._domain_tables(np.zeros((3, 2)), np.ones((1, 2)), check=check)
    first = tables(B, A)
    assert [tuple(t.shape) for t in first] == [(3, 2), (1, 2)] and all(t.dtype == torch.float32 for t in first)
    assert tables(B, A) is first and seen == [3, 1]
    host = np.arange(6, dtype=np.float32).reshape(3, 2)[:, ::-1]
    t_B, t_A = EM._domain_tables(host, host[:1])(B, A)
    assert t_B.is_contiguous() and np.array_equal(t_B.numpy(), host) and tuple(t_A.shape) == (1, 2)


def test_fss_and_minkowski_leave_a_tensor_of_thresholds_where_it_is_for_check_to_refuse(monkeypatch):
    """a host ARRAY is what the two entry points upload; a tensor that is not on the device reaches _check as it came and is
    refused there, unchecked thresholds on the host never reach a kernel"""
    def no_device(*a, **k):
        raise AssertionError("a refusal reached the library")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(_lib, "query", no_device)
    seen, check = [], ops._check

    def spy(*ts):
        seen.append(ts)
        check(*ts)
    monkeypatch.setattr(ops, "_check", spy)
    x, thr = torch.zeros(2, 1, 8, 8), torch.tensor([[1.0, 0.0]])     # decreasing: a tensor's order is not looked at
    with pytest.raises(_lib.AcgError, match="ROCm device"):
        ops.minkowski(x, 1, "nchw", thr)
    assert seen[-1][-1] is not None and seen[-1][-1].data_ptr() == thr.data_ptr() and not seen[-1][-1].is_cuda
    with pytest.raises(_lib.AcgError, match="ROCm device"):
        ops.fss(x, x, 1, "nchw", "nchw", thr, (1, 3))
    assert seen[-1][-1].data_ptr() == thr.data_ptr() and not seen[-1][-1].is_cuda
    with pytest.raises(_lib.AcgError, match="ROCm device"):          # and on its own it is what _check refuses
        check(thr)
    assert ops.channel_table("who", _lib.AcgError, "thresholds", thr, 1, 8, None).device.type == "cpu"
