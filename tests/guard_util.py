"""Device buffers for the direct C-ABI tests: every buffer carries GUARD 32-bit guard words after its end which must be
unchanged after the calls (a kernel that writes one element too far fails the test instead of corrupting a neighbour), and an
output buffer starts as NaN everywhere (an element the kernel does not write fails the comparison)."""
import numpy as np
import torch

GUARD = 64
_PATTERN = 0x5A5AC3C3


class Buf(object):
    """n 32-bit words (+ guard).  Buf.of(array): an input; Buf.out(n): a NaN-poisoned fp32 output; Buf.out(n, np.uint32):
    32-bit words poisoned with 0xFFFFFFFF (bit masks); Buf.raw(bytes): a byte blob (pre-split tensors)."""
    live = []

    def __init__(self, n, init=None, dtype=np.float32, poison=True):
        self.n, self.dtype = int(n), dtype
        host = np.full(self.n + GUARD, _PATTERN, np.uint32)
        if init is not None:
            host[:self.n] = np.ascontiguousarray(init, dtype).reshape(-1).view(np.uint32)
        elif poison:
            host[:self.n] = np.float32(np.nan).view(np.uint32) if dtype == np.float32 else 0xFFFFFFFF
        else:
            host[:self.n] = 0
        self.t = torch.from_numpy(host.view(np.int32)).cuda()
        Buf.live.append(self)

    @classmethod
    def of(cls, a, dtype=np.float32):
        a = np.ascontiguousarray(a, dtype)
        return cls(a.size, a, dtype)

    @classmethod
    def out(cls, n, dtype=np.float32):
        return cls(n, None, dtype)

    @classmethod
    def raw(cls, bytes_):
        """pre-split (S16) tensors and other byte blobs, len % 4 == 0"""
        b = np.ascontiguousarray(bytes_).view(np.uint8).reshape(-1)
        return cls(b.size // 4, b.view(np.uint32), np.uint32)

    @property
    def ptr(self):
        import ctypes
        return ctypes.c_void_p(self.t.data_ptr())

    def at(self, word):
        """pointer to word `word` of the buffer (a column block of a wider matrix)"""
        import ctypes
        return ctypes.c_void_p(self.t.data_ptr() + 4 * int(word))

    def put(self, a):
        """overwrite the body (not the guard) with new contents"""
        a = np.ascontiguousarray(a, self.dtype).reshape(-1)
        assert a.size == self.n
        self.t[:self.n].copy_(torch.from_numpy(a.view(np.int32)))

    def host(self, shape=None):
        torch.cuda.synchronize()
        a = self.t.cpu().numpy().view(np.uint32)
        assert np.all(a[self.n:] == _PATTERN), "guard words after the buffer were overwritten"
        a = a[:self.n].view(self.dtype).copy()
        return a if shape is None else a.reshape(shape)

    def bytes(self):
        return self.host().view(np.uint8)

    @classmethod
    def check_all(cls):
        """every live buffer's guard words; then forget them"""
        torch.cuda.synchronize()
        for b in cls.live:
            g = b.t[b.n:].cpu().numpy().view(np.uint32)
            assert np.all(g == _PATTERN), "guard words after a buffer of %d words were overwritten" % b.n
        cls.live = []


def rejected(lib, name, *args):
    """the call must return -1 and leave a message, without a launch"""
    rc = getattr(lib, name)(*args)
    msg = lib.acg_last_error().decode()
    assert rc == -1 and msg, (name, rc, msg)
    return msg
