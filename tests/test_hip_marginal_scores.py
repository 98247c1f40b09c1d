"""GPU tests of acg_marginal_scores through the C ABI against tests/marginal_eval_ref.py.  The fields are sorted by NumPy on
the host, so nothing here depends on acg_field_sort.  Bars, all derived:
  below  exact (integers);
  q      within 1 float32 ulp of the reference: one differently rounded double operation in front of the final rounding;
  w      within a relative P 2^-52 of the reference: any summation order of P non-negative doubles is within (P - 1) 2^-53 of
         the exact sum, on both sides, and the division by P rounds once on each."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import marginal_eval_ref as R
from guard_util import GUARD, Buf

pytestmark = pytest.mark.gpu

FN = "acg_marginal_scores"


class Guarded(object):
    """an output of n elements of `dtype` inside a poisoned buffer with GUARD guard words in front of it too"""

    def __init__(self, n, dtype):
        self.words = n * np.dtype(dtype).itemsize // 4
        self.n, self.dtype = n, dtype
        self.buf = Buf.out(GUARD + self.words, np.uint32)              # every word 0xFFFFFFFF: a NaN as float and as double
        self.ptr = self.buf.at(GUARD)

    def host(self, shape):
        a = self.buf.host()                                            # asserts the guard words behind the buffer
        assert np.all(a[:GUARD] == 0xFFFFFFFF), "guard words in front of the buffer were overwritten"
        return a[GUARD:].view(self.dtype).reshape(shape).copy()


def _levels(L):
    return {0: (), 1: R.LEVELS1, 16: R.LEVELS16}[L]


@functools.lru_cache(maxsize=None)
def _case(i):
    """case i -> (sx, sy or None, levels, edges or None, the reference dict), computed once and left unchanged"""
    P, rows, C, per, L, E = R.ABI_CASES[i]
    sx, sy = R.abi_case_fields(i)
    levels = _levels(L)
    edges = R.make_edges(sx, E, seed=i) if E else None
    ref = {}
    if sy is not None:
        ref["w"] = R.wasserstein(sx, sy, per)
    if L:
        ref["q"] = R.quantiles(sx, levels)
    if E:
        ref["below"] = R.below(sx, edges)
    for a in (sx, sy, edges) + tuple(ref.values()):
        if a is not None:
            a.setflags(write=False)
    return sx, sy, levels, edges, ref


def _call(sx, sy, per, levels, edges):
    """one call into poisoned, guarded outputs -> dict of host arrays"""
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    rows, C, P = sx.shape
    L, E = len(levels), 0 if edges is None else edges.shape[1]
    dev = lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()      # the cached cases are read-only
    dx, dy, de = dev(sx), dev(sy), dev(edges)
    w = Guarded(rows * C * 2, np.float64) if sy is not None else None
    q = Guarded(rows * C * L, np.float32) if L else None
    b = Guarded(rows * C * E, np.int32) if E else None
    lv = (ctypes.c_double * max(L, 1))(*levels)
    rc = lib.acg_marginal_scores(ops._ptr(dx), ops._ptr(dy), rows, max(per, 1), C, P, lv, L, ops._ptr(de), E,
                                 w.ptr if w else None, q.ptr if q else None, b.ptr if b else None, ops._stream())
    assert rc == 0, lib.acg_last_error().decode()
    out = {}
    if w:
        out["w"] = w.host((rows, C, 2))
    if q:
        out["q"] = q.host((rows, C, L))
    if b:
        out["below"] = b.host((rows, C, E))
    return out


@pytest.mark.parametrize("i", range(len(R.ABI_CASES)), ids=["P%d-%dx%d-per%d-L%d-E%d" % c for c in R.ABI_CASES])
def test_scores_meet_their_bars_are_fully_written_and_repeat(i):
    P, rows, C, per, L, E = R.ABI_CASES[i]
    sx, sy, levels, edges, ref = _case(i)
    got = _call(sx, sy, per, levels, edges)
    assert sorted(got) == sorted(ref)
    if "below" in ref:
        assert got["below"].dtype == np.int32 and np.array_equal(got["below"], ref["below"])
    if "q" in ref:
        assert not np.isnan(got["q"]).any()                            # every element written over the poison
        ulp = R.ulp_distance(got["q"], ref["q"])
        print("q: max ulp distance %d" % ulp.max())
        assert ulp.max() <= 1
    if "w" in ref:
        assert not np.isnan(got["w"]).any()
        err = np.abs(got["w"] - ref["w"])
        print("w: max relative error %.3e, bar %.3e" % ((err / np.maximum(ref["w"], 1e-300)).max(), P * 2.0 ** -52))
        assert np.all(err <= P * 2.0 ** -52 * ref["w"])
    again = _call(sx, sy, per, levels, edges)
    for k in got:
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), k
    Buf.check_all()


def test_an_operand_off_the_16_byte_grid_gives_the_same_bits():
    """the sums keep their order whatever the alignment of the operands (a compiler may widen the loads of aligned ones)"""
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    i = [c[0] for c in R.ABI_CASES].index(4096)
    sx, sy, levels, edges, ref = _case(i)
    rows, C, P = sx.shape
    want = _call(sx, sy, 1, (), None)["w"]
    flat_x = torch.zeros(sx.size + 1, dtype=torch.float32, device="cuda")
    flat_y = torch.zeros(sy.size + 1, dtype=torch.float32, device="cuda")
    flat_x[1:].copy_(torch.from_numpy(np.array(sx)).reshape(-1))
    flat_y[1:].copy_(torch.from_numpy(np.array(sy)).reshape(-1))
    w = Guarded(rows * C * 2, np.float64)
    at = lambda t: ctypes.c_void_p(t.data_ptr() + 4)
    rc = lib.acg_marginal_scores(at(flat_x), at(flat_y), rows, 1, C, P, None, 0, None, 0, w.ptr, None, None, ops._stream())
    assert rc == 0, lib.acg_last_error().decode()
    assert np.array_equal(w.host((rows, C, 2)).view(np.uint64), want.view(np.uint64))
    Buf.check_all()


def test_the_identities_on_the_device():
    """x against itself is exactly 0; level 0 and 1 are the minimum and the maximum; -0.0 and +0.0 edges count alike"""
    x = R.sorted_values(R.make_fields("signed_zeros", 1, 143, 3, 2).reshape(3, 2, 143))
    edges = np.array([[-0.0, 0.0], [0.0, -0.0]], dtype=np.float32)
    got = _call(x, x, 1, (0.0, 1.0), edges)
    assert np.all(got["w"] == 0.0)
    assert np.array_equal(got["q"][..., 0], x[..., 0]) and np.array_equal(got["q"][..., 1], x[..., -1])
    assert np.array_equal(got["below"][..., 0], got["below"][..., 1]) and np.array_equal(got["below"][..., 0], (x < 0).sum(-1))
    Buf.check_all()


def test_refusals_return_minus_one_name_the_entry_and_launch_nothing():
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    st = ops._stream()
    P_ = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rows, C, P = 6, 2, 64
    sx = torch.zeros((rows, C, P), device="cuda")
    sy = torch.zeros((rows // 3, C, P), device="cuda")
    edges = torch.zeros((C, 4), device="cuda")
    w = torch.full((rows, C, 2), 7.0, device="cuda", dtype=torch.float64)
    q = torch.full((rows, C, 16), 7.0, device="cuda")
    below = torch.full((rows, C, 4), 7, device="cuda", dtype=torch.int32)
    lv = (ctypes.c_double * 17)(*([0.5] * 17))

    def levels(*v):
        return (ctypes.c_double * len(v))(*v)
    ok = dict(sx=P_(sx), sy=P_(sy), rows=rows, per=3, C=C, P=P, levels=lv, L=2, edges=P_(edges), E=4, w=P_(w), q=P_(q), below=P_(below))
    order = ("sx", "sy", "rows", "per", "C", "P", "levels", "L", "edges", "E", "w", "q", "below")

    def call(**kw):
        a = dict(ok, **kw)
        return lib.acg_marginal_scores(*([a[k] for k in order] + [st]))
    assert call() == 0, lib.acg_last_error().decode()
    torch.cuda.synchronize()
    w.fill_(7.0), q.fill_(7.0), below.fill_(7)
    nan = float("nan")
    bad = [
        (dict(sx=None), "null"), (dict(w=None), "stray w"), (dict(sy=None), "stray w"), (dict(q=None), "stray q"), (dict(levels=None), "levels"),
        (dict(below=None), "stray below"), (dict(edges=None), "edges"), (dict(L=0), "stray q"), (dict(E=0), "stray below"),
        (dict(sy=None, w=None, L=0, q=None, E=0, below=None), "nothing to compute"),
        (dict(rows=0), "rows"), (dict(C=0), "C >= 1"), (dict(P=0), "pixels"), (dict(P=(1 << 20) + 1), "pixels"),
        (dict(L=17), "levels"), (dict(L=-1), "levels"), (dict(E=257), "edges"), (dict(E=-1), "edges"),
        (dict(per=4), "x_per_y"), (dict(per=0), "x_per_y"), (dict(per=7), "x_per_y"),
        (dict(levels=levels(0.5, 1.5)), "level 1"), (dict(levels=levels(-0.01, 0.5)), "level 0"), (dict(levels=levels(0.5, nan)), "level 1"),
        (dict(w=P_(sx)), "alias"), (dict(w=P_(sy)), "alias"), (dict(q=P_(sx)), "alias"), (dict(q=P_(edges)), "alias"),
        (dict(below=P_(sy)), "alias"), (dict(below=P_(edges)), "alias"), (dict(q=P_(w)), "alias"), (dict(below=P_(w)), "alias"),
        (dict(below=P_(q)), "alias"),
    ]
    for kw, word in bad:
        rc = call(**kw)
        msg = lib.acg_last_error().decode()
        assert rc == -1 and msg.startswith(FN) and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((w == 7.0).all()) and bool((q == 7.0).all()) and bool((below == 7).all())        # nothing was launched
