"""GPU tests of the averaged-weights kernels through the C ABI: acg_ema_multi against the float64 recurrence of tests/ema_ref.py
(sizes around the vector width, the block and the grid cap; eight groups in one launch; misaligned pointers; both branches of
the schedule; the step taken from the host and from the device) and acg_swap_multi's exact exchange, on guarded buffers."""
import ctypes

import numpy as np
import pytest
import torch

import ema_ref as E
from guard_util import Buf, rejected

pytestmark = pytest.mark.gpu

# one element per thread and trip is an f32x4: the kernels launch at most 2048 blocks of 256 threads per group
# (csrc/elementwise.hip EMA_BLOCK_CAP), so the first grid-stride trip of a group covers this many elements
FIRST_TRIP = 2048 * 256 * 4
SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, FIRST_TRIP + 3]
# a case = its groups: (n, words p starts past a 16-byte boundary, the same for e)
CASES = [pytest.param([(n, 0, 0)], id="n%d" % n) for n in SIZES] + [
    pytest.param([(1025, 0, 0), (1, 0, 0), (256, 0, 0), (3, 0, 0), (1023, 0, 0), (5, 0, 0), (257, 0, 0), (4, 0, 0)], id="eight_groups"),
    pytest.param([(1025, 1, 1)], id="both_misaligned"),
    pytest.param([(1025, 0, 1)], id="e_misaligned"),
    pytest.param([(255, 0, 0), (1024, 1, 0), (257, 0, 1)], id="mixed_alignment"),
]
FILL = 7.25      # the words in front of a misaligned body


class Side(object):
    """one of a group's two buffers: `off` filler words, then the n-element body the kernel is given"""

    def __init__(self, n, off, body):
        self.n, self.off = n, off
        self.buf = Buf.of(self._whole(body))
        assert self.buf.t.data_ptr() % 16 == 0

    def _whole(self, body):
        return np.concatenate([np.full(self.off, FILL, np.float32), np.asarray(body, np.float32)])

    def put(self, body):
        self.buf.put(self._whole(body))

    @property
    def addr(self):
        return self.buf.t.data_ptr() + 4 * self.off

    def bits(self):
        h = self.buf.host()                                   # checks the guard words behind the buffer
        assert np.all(h[:self.off] == np.float32(FILL)), "the words in front of the body were overwritten"
        return h[self.off:].view(np.uint32)

    def values(self):
        return self.bits().view(np.float32)


def _table(sides):
    from dtgan_amd import _lib
    arr = (_lib.EmaGroup * len(sides))()
    for i, (p, e) in enumerate(sides):
        arr[i].p, arr[i].e, arr[i].n = p.addr, e.addr, p.n
    return arr


def _lib_and_stream():
    from dtgan_amd import _lib, ops
    return _lib.load(), ops._stream()


def _draw(rs, groups):
    return [rs.uniform(-1, 1, n).astype(np.float32) for n, _, _ in groups]


# (decay, the steps applied in sequence): 0.5 crosses its warm-up at t = 8, so 7, 8, 9 take both branches of the minimum
SEQUENCES = [(0.5, [7, 8, 9]), (0.999, [100000])]


@pytest.mark.parametrize("groups", CASES)
def test_ema_matches_float64_and_the_device_step_gives_the_same_bits(groups):
    lib, st = _lib_and_stream()
    rs = np.random.RandomState(sum(n for n, _, _ in groups))
    for decay, steps in SEQUENCES:
        first = _draw(rs, groups)
        P = [Side(n, po, first[i]) for i, (n, po, _) in enumerate(groups)]
        Eh = [Side(n, eo, first[i]) for i, (n, _, eo) in enumerate(groups)]     # the step number from the host
        Ed = [Side(n, eo, first[i]) for i, (n, _, eo) in enumerate(groups)]     # ... and from the device
        ref = [f.astype(np.float64) for f in first]
        M = max(float(np.abs(f).max()) for f in first)
        step_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
        for k, t in enumerate(steps, 1):
            ps = first if k == 1 else _draw(rs, groups)
            for side, p in zip(P, ps):
                side.put(p)
            step_dev.fill_(t - 1)
            rc = lib.acg_ema_multi(_table(list(zip(P, Eh))), len(groups), decay, t, None, st)
            assert rc == 0, lib.acg_last_error().decode()
            rc = lib.acg_ema_multi(_table(list(zip(P, Ed))), len(groups), decay, 0, ctypes.c_void_p(step_dev.data_ptr()), st)
            assert rc == 0, lib.acg_last_error().decode()
            worst = 0.0
            for i in range(len(groups)):
                ref[i] = E.ema_step(ref[i], ps[i], decay, t)
                M = max(M, float(np.abs(ps[i]).max()), float(np.abs(ref[i]).max()))
                got = Eh[i].values()
                M = max(M, float(np.abs(got).max()))
                assert np.array_equal(P[i].bits(), ps[i].view(np.uint32)), "p was written"
                assert np.array_equal(Ed[i].bits(), Eh[i].bits()), (decay, t, i, "device step differs from the host step")
                worst = max(worst, float(np.abs(got.astype(np.float64) - ref[i]).max()))
            allowed = E.bound(k, M)
            print("decay %g step %d (%d in sequence): max |e - e64| = %.3e, allowed %.3e (M = %.4f)" % (decay, t, k, worst, allowed, M))
            assert worst <= allowed, (decay, t, worst, allowed)
        Buf.check_all()


def test_ema_refuses_bad_arguments_without_touching_the_average():
    lib, st = _lib_and_stream()
    n = 260
    p = Side(n, 0, np.linspace(-1, 1, n))
    e = Side(n, 0, np.zeros(n))
    e.buf = Buf.out(n)                                            # NaN everywhere: any write shows
    before = e.buf.host().view(np.uint32).copy()
    one = _table([(p, e)])
    nine = _table([(p, e)] * 9)
    step_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    dev = ctypes.c_void_p(step_dev.data_ptr())

    def with_(**kw):
        t = _table([(p, e)])
        for k, v in kw.items():
            setattr(t[0], k, v)
        return t
    bad = [(one, 1, 0.0, 1, None, "decay"), (one, 1, 1.0, 1, None, "decay"), (one, 1, -0.5, 1, None, "decay"),
           (one, 1, 1.5, 1, None, "decay"), (one, 1, float("nan"), 1, None, "decay"), (one, 1, 0.0, 0, dev, "decay"),
           (one, 0, 0.9, 1, None, "groups"), (nine, 9, 0.9, 1, None, "groups"), (one, -1, 0.9, 1, None, "groups"),
           (None, 1, 0.9, 1, None, "groups"), (with_(p=None), 1, 0.9, 1, None, "null"), (with_(e=None), 1, 0.9, 1, None, "null"),
           (with_(n=0), 1, 0.9, 1, None, "no elements"), (with_(n=0), 1, 0.9, 0, dev, "no elements"),
           (one, 1, 0.9, 0, None, "step"), (one, 1, 0.9, -3, None, "step")]
    for groups, ng, decay, step, sd, word in bad:
        msg = rejected(lib, "acg_ema_multi", groups, ng, decay, step, sd, st)
        assert word in msg, (word, msg)
    for groups, ng, word in ((one, 0, "groups"), (nine, 9, "groups"), (None, 1, "groups"), (with_(p=None), 1, "null"),
                             (with_(e=None), 1, "null"), (with_(n=0), 1, "no elements")):
        msg = rejected(lib, "acg_swap_multi", groups, ng, st)
        assert word in msg, (word, msg)
    assert np.array_equal(e.buf.host().view(np.uint32), before)
    assert np.array_equal(p.values(), np.linspace(-1, 1, n).astype(np.float32))
    Buf.check_all()


@pytest.mark.parametrize("groups", CASES)
def test_swap_exchanges_exactly_and_twice_is_the_identity(groups):
    lib, st = _lib_and_stream()
    rs = np.random.RandomState(1 + sum(n for n, _, _ in groups))
    a, b = _draw(rs, groups), _draw(rs, groups)
    for x in a + b:                                               # every bit pattern travels: a NaN payload, -0, a denormal
        x[:1].view(np.uint32)[:] = 0x7FC01234
        x[-1:].view(np.uint32)[:] = 0x80000000 if x.size > 1 else 0x00000001
    P = [Side(n, po, a[i]) for i, (n, po, _) in enumerate(groups)]
    Q = [Side(n, eo, b[i]) for i, (n, _, eo) in enumerate(groups)]
    table = _table(list(zip(P, Q)))
    assert lib.acg_swap_multi(table, len(groups), st) == 0, lib.acg_last_error().decode()
    for i in range(len(groups)):
        assert np.array_equal(P[i].bits(), b[i].view(np.uint32)) and np.array_equal(Q[i].bits(), a[i].view(np.uint32)), i
    assert lib.acg_swap_multi(table, len(groups), st) == 0, lib.acg_last_error().decode()
    for i in range(len(groups)):
        assert np.array_equal(P[i].bits(), a[i].view(np.uint32)) and np.array_equal(Q[i].bits(), b[i].view(np.uint32)), i
    Buf.check_all()
