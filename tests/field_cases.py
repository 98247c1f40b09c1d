"""Operands of the field-metric kernel tests: a host field (rows, C, H, W) placed on the device in a layout, with whatever a
kernel must not read put into the padded channels, and the stride triples and views that go with it."""
import numpy as np
import torch

# (layout, C, Cp) of a single operand: the spectrum family's
LAYOUTS = [("nhwc", 1, 4), ("nhwc", 3, 4), ("nhwc", 3, 16), ("nchw", 1, 1), ("nchw", 3, 3)]
# (layout x, stored channels x, floats x starts off the 16-byte grid, layout y, stored channels y): planar, a pixel's channels
# in one 16-byte load, and the pixel-by-pixel path for a wide pixel and for an unaligned one
PAIR_LAYOUTS = (("nchw", 0, 0, "nchw", 0), ("nhwc", 4, 0, "nhwc", 4), ("nhwc", 16, 0, "nchw", 0), ("nhwc", 4, 1, "nhwc", 4))
# (layout, stored channels, floats off)
OFFSET_LAYOUTS = (("nchw", 0, 0), ("nhwc", 4, 0), ("nhwc", 16, 0), ("nhwc", 4, 1), ("nchw", 0, 1))


def field_host(x, layout, C=None, Cp=0, seed=0, nan=0.0, fill=None):
    """the first C channels of x (rows, >= C, H, W) as the layout stores them, a copy.  NHWC: the padded channels C..Cp-1 hold
    `fill` where given (a constant or NaN), else RandomState(seed)'s +-50 garbage, a share `nan` of it replaced by NaNs"""
    x = x if C is None else x[:, :C]
    if layout == "nchw":
        return np.array(x, order="C")
    rows, C, H, W = x.shape
    if fill is not None:
        t = np.full((rows, H, W, Cp), fill, np.float32)
    else:
        rs = np.random.RandomState(seed)
        t = rs.uniform(-50, 50, (rows, H, W, Cp)).astype(np.float32)
        if nan:
            t[rs.uniform(size=t.shape) < nan] = np.nan
    t[..., :C] = np.moveaxis(x, 1, 3)
    return t


def field_operand(x, layout, C=None, Cp=0, seed=0, nan=0.0, fill=None, off=None):
    """field_host on the device; with `off` (0 included) the operand starts `off` floats behind a 16-byte boundary"""
    h = field_host(x, layout, C, Cp, seed, nan, fill)
    if off is None:
        return torch.from_numpy(h).cuda()
    flat = torch.empty(h.size + 4, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    d = flat[off:off + h.size].view(h.shape)
    d.copy_(torch.from_numpy(h))
    assert d.is_contiguous() and d.data_ptr() % 16 == 4 * off
    return d


def offset_operand(x, layout, Cp=0, off=0, seed=0):
    """every channel of x, `off` floats behind a 16-byte boundary; NHWC: +-50 garbage, a fifth of it NaN, in the padded channels"""
    return field_operand(x, layout, None, Cp, seed, nan=0.2, off=off)


def shifted(t, off):
    """the same tensor `off` floats behind a 16-byte boundary"""
    if not off:
        return t
    flat = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert flat.data_ptr() % 16 == 0
    flat[off:off + t.numel()].copy_(t.reshape(-1))
    return flat[off:off + t.numel()].view(t.shape)


def strides(layout, C, Cp, H, W):
    """(row, channel, pixel) strides in floats"""
    return (H * W * Cp, Cp, 1) if layout == "nhwc" else (C * H * W, 1, H * W)


def valid(gx, layout, C):
    """(rows, C, H, W) of a result in its layout"""
    return np.moveaxis(gx[..., :C], 3, 1) if layout == "nhwc" else gx
