"""Tables and helpers shared by the convolution, network and whole-step parity tests: the module-level convolution cases, the
networks of the golden fixtures, kernel names and array helpers of the fast-path tests, and the oracle-checked step."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from model_cases import make_opt

CONV_CASES = [
    # K, stride, pad, mode, Ci, Co, N, H, W
    (3, 1, 1, "zero", 8, 8, 2, 12, 10),
    (3, 1, 1, "reflect", 32, 32, 2, 9, 11),
    (7, 1, 3, "reflect", 3, 8, 2, 16, 16),
    (7, 1, 3, "zero", 8, 3, 2, 16, 16),
    (3, 2, 1, "zero", 16, 32, 2, 16, 16),
    (3, 2, 1, "zero", 16, 32, 1, 15, 13),
    (4, 2, 1, "zero", 3, 16, 2, 16, 16),
    (4, 1, 1, "zero", 32, 64, 2, 9, 9),
    (4, 1, 0, "zero", 32, 1, 3, 6, 6),
    (1, 1, 0, "zero", 64, 16, 2, 3, 3),
    (3, 1, 1, "reflect", 128, 128, 1, 8, 8),
    (4, 1, 1, "zero", 256, 256, 1, 6, 6),
    (3, 2, 1, "zero", 64, 128, 1, 12, 12),
    (3, 1, 1, "zero", 6, 40, 1, 20, 20),
    # 3x3 stride-1 128-wide layers: the row-taps weight-gradient kernel (32-pixel row segments, partial tails)
    (3, 1, 1, "zero", 128, 128, 2, 9, 37),
    (3, 1, 1, "reflect", 64, 128, 1, 6, 40),
    (3, 1, 0, "zero", 128, 256, 1, 10, 34),
    # 32 <-> 3 channel layers: the patch kernel (8x16 output tiles, partial tiles, reflect / zero halo), forward and
    # as the data gradient of the 3 -> 32 stem
    (7, 1, 3, "reflect", 32, 3, 2, 20, 37),
    (7, 1, 3, "zero", 32, 3, 1, 9, 18),
    (7, 1, 3, "reflect", 3, 32, 2, 18, 21),
    (3, 1, 1, "zero", 32, 3, 1, 10, 10),
    # row-patch variant of the wave-specialised kernel: output width 16 / 32 / 64 / 128 (R = 8 / 4 / 2 / 1 rows per tile)
    (3, 1, 1, "reflect", 128, 128, 1, 16, 16),
    (3, 1, 1, "zero", 128, 128, 2, 8, 32),
    (3, 1, 1, "reflect", 64, 128, 1, 4, 64),
    (4, 1, 1, "zero", 128, 128, 1, 17, 17),
    (3, 1, 1, "reflect", 128, 256, 1, 2, 128),
    (4, 1, 1, "zero", 128, 128, 2, 16, 32),   # its DATA gradient (grid = the 16x32 input, taps with descending dx)
    (3, 1, 1, "zero", 128, 128, 3, 9, 13),    # 13-wide rows: ~11 segments per tile, tiles straddling images
    (3, 1, 1, "reflect", 160, 128, 2, 11, 130),  # 130-wide rows (the padded data-gradient width), Cin = 5 x 32
    # kernel-row weight gradient (conv_wgrad_tr.hip): 128-multiple channels, width a multiple of the 32-pixel run
    (3, 1, 1, "reflect", 128, 128, 2, 6, 32),
    (3, 1, 1, "zero", 128, 256, 1, 5, 64),
    (3, 1, 1, "zero", 256, 128, 3, 4, 32),
    (3, 1, 1, "reflect", 128, 128, 1, 40, 96),   # several splits, runs that cross image rows within a split
    # its 32 <-> 64 channel variant (128-pixel runs, waves split the pixels)
    (3, 1, 1, "zero", 32, 64, 1, 3, 128),
    (3, 1, 1, "reflect", 64, 32, 2, 4, 128),
    (3, 1, 1, "zero", 64, 32, 2, 20, 128),       # several splits
    (3, 1, 1, "reflect", 32, 64, 1, 5, 256),
    # persistent row pipeline (conv_rows.hip): zero-padded 3x3, 32 gathered -> 64 written channels, 128-pixel bands; forward of a
    # 32 -> 64 layer (two bands, two row chunks per band, an odd chunk) and the data gradient of a 64 -> 32 layer
    (3, 1, 1, "zero", 32, 64, 2, 21, 256),
    (3, 1, 1, "zero", 64, 32, 1, 17, 128),
]


def _conv_module(K, stride, pad, mode, Ci, Co):
    from dtgan_amd import modules as M
    if mode == "reflect":
        return M.Sequential(nn.ReflectionPad2d(pad), M.Conv2d(Ci, Co, K, stride=stride, padding=0, bias=True)).cuda()
    return M.Sequential(M.Conv2d(Ci, Co, K, stride=stride, padding=pad, bias=True)).cuda()


def build(meta):
    """the network a 'net' golden fixture was taken from"""
    from dtgan_amd import networks as N
    c, n = meta["cfg"], meta["net"]
    g = [0]
    if n == "netG_B_A":   # --norm batch / --use_dropout fixtures carry the option in their cfg (options.py:64-65)
        return N.define_G(c["input_nc"], c["output_nc"], c["ngf"], norm=c.get("norm", "instance"),
                          use_dropout=c.get("use_dropout", False), gpu_ids=g, n_blocks=c["n_blocks"])
    if n == "netG_A_B":
        return N.define_stochastic_G(c["nlatent"], c["input_nc"], c["output_nc"], c["ngf"],
                                     use_dropout=c.get("use_dropout", False), gpu_ids=g, n_blocks=c["n_blocks"])
    if n == "netD_B":
        return N.define_D_B(c["input_nc"], c["ndf"], "basic", "instance", gpu_ids=g)
    if n == "netD_A":
        return N.define_D_A(c["input_nc"], c["ndf"], "basic", "instance", gpu_ids=g)
    if n == "netE_B":
        return N.define_E(c["nlatent"], c["input_nc"], c["nef"], "batch", gpu_ids=g)
    if n == "netD_z_B":
        return N.define_LAT_D(c["nlatent"], c["ndf"], gpu_ids=g)
    raise KeyError(n)


# ---------------------------------------------------------------------------------------------------------------------
# the specialised bf16x3 kernels, as acg_last_kernel names them
ROWS = "conv_rows_x3<32,64>"
RP = "RP=1"
WS = "igemm_conv_x3_ws"
KROW = "=wgrad_x3_krow"              # '=': the whole kernel name (wgrad_x3_krow is a prefix of its siblings)
KROW_S = "wgrad_x3_krow_s<"
KROWG = "wgrad_x3_krowg<"
PH4 = "igemm_conv_ph4"
THINROW = "conv_thinrow_x3"
PATCHN = "conv_patchn_x3"
THINW = "wgrad_thin_patch_x3"
FAST = [ROWS, RP, WS, "igemm_conv_x3_pre", PH4, "wgrad_x3_krow", THINROW, PATCHN, THINW]
# pre-split trunk: (N, H, W, Ci, Co) of a 3x3 reflect pad-1 layer inside acg_conv2d_s16_supported
S16_CASES = [
    (1, 8, 32, 128, 128), (2, 13, 96, 128, 256), (3, 40, 64, 256, 128), (1, 63, 128, 128, 128), (2, 64, 96, 128, 128),
    (1, 64, 128, 128, 128), (2, 96, 256, 128, 128), (1, 64, 384, 256, 128), (3, 64, 128, 128, 256), (1, 128, 640, 128, 128),
]
_REF_DEV = []


def _ref_device():
    """where the float64 reference convolution runs: the device, or the host if the device has no fp64 convolution"""
    if not _REF_DEV:
        dev = "cuda"
        try:
            a = torch.ones((1, 1, 3, 3), dtype=torch.float64, device=dev)
            F.conv2d(a, a, padding=1).sum().item()
        except RuntimeError:
            dev = "cpu"
        _REF_DEV.append(dev)
    return _REF_DEV[0]


def _match(want, k):
    return k == want[1:] if want.startswith("=") else want in k


def _nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def _nchw(a):
    return np.transpose(a, (0, 3, 1, 2))


def _dev_t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _pad_c(a, C, axis):
    """zero-pad a channel axis to the stored width"""
    if a.shape[axis] == C:
        return a
    pad = [(0, 0)] * a.ndim
    pad[axis] = (0, C - a.shape[axis])
    return np.pad(a, pad)


# ---------------------------------------------------------------------------------------------------------------------
# one whole step against the fp32 oracle
_ORACLE_CACHE = {}
# step 0 against the oracle: (losses, gradient norms, images) — exact fp32 pins indexing and fusion logic, bf16x3 is held to
# the north-star bar (model_cases.STEP_TOL's first row)
ORACLE_TOL = {"f32": (2e-4, 1e-3, 1e-4), "bf16x3": (1e-3, 3e-3, 1e-3)}


def _run_cfg(kw, S, Nb, prec, steps=1, seed=0, in_seed=60):
    from hip_util import t, n, precision, load_recipe
    from dtgan_amd import model as M
    from oracle import recipe
    with precision(prec):
        m = M.AugmentedCycleGAN(make_opt(**kw), testing=True)
        for k, net in m._net_dict().items():
            load_recipe(net, k, seed, "init")
        out = []
        for s in range(steps):
            A, B, z = recipe.inputs(in_seed + s, Nb, kw["input_nc"], kw["output_nc"], S, 16)
            losses, visuals, gnorms = m.train_instance(t(A), t(B), t(z))
            out.append((dict(losses), {k: n(v) for k, v in visuals.items()}, dict(gnorms)))
    return out


def _oracle_step(kw, S, Nb, seed, in_seed):
    """the oracle's step on what _run_cfg(kw, S, Nb, prec, seed=seed, in_seed=in_seed) runs, computed once for both precisions"""
    key = ("step", tuple(sorted(kw.items())), S, Nb, seed, in_seed)
    if key not in _ORACLE_CACHE:
        from oracle import recipe, step
        o = step.AugStep(step.Opt(**kw))
        o.load({k: recipe.values_for(net.shapes, k, seed, "init") for k, net in o.nets().items()})
        _ORACLE_CACHE[key] = o.train_instance(*recipe.inputs(in_seed, Nb, kw["input_nc"], kw["output_nc"], S, 16))
    return _ORACLE_CACHE[key]


def _matches_oracle(got, ref, prec, case, gnorm_tol=None):
    """asserts the whole step — 13 losses, 6 gradient norms, 4 images — within ORACLE_TOL[prec] of the oracle's, and prints the
    worst relative error of each group beside its bound.  `gnorm_tol`: {gradient norm: relative bound} replacing the group's
    bound for single gradient norms (a measured conditioning allowance)"""
    from hip_util import rel
    (l1, v1, g1), (l0, v0, g0) = got, ref
    lt, gt, vt = ORACLE_TOL[prec]
    gts = np.array([(gnorm_tol or {}).get(k, gt) for k in g0])
    assert list(l1.keys()) == list(l0.keys()) and list(g1.keys()) == list(g0.keys())
    worst = lambda a, b: max(abs(a[k] - b[k]) / max(abs(b[k]), 1e-30) for k in b)
    ev = max(rel(v1[k], v0[k]) for k in ("fake_A", "fake_B", "rec_A", "rec_B"))
    print("oracle_err case=%s prec=%s losses=%.2e/%.0e gnorms=%.2e/%.0e images=%.2e/%.0e gnorm_G_A_B=%.2e"
          % (case, prec, worst(l1, l0), lt, worst(g1, g0), gt, ev, vt, worst({0: g1["gnorm_G_A_B"]}, {0: g0["gnorm_G_A_B"]})))
    assert np.allclose(list(l1.values()), list(l0.values()), rtol=lt, atol=2e-6), (l1, l0)
    a, b = np.array(list(g1.values())), np.array(list(g0.values()))
    assert np.all(np.abs(a - b) <= gts * np.abs(b) + 1e-6), (g1, g0)
    for k in ("fake_A", "fake_B", "rec_A", "rec_B"):
        assert v1[k].shape == v0[k].shape, k
        assert rel(v1[k], v0[k]) < vt, (k, rel(v1[k], v0[k]))


# ---------------------------------------------------------------------------------------------------------------------
# the full-resolution layers on operands of 2 to 4 GiB (test_hip_large_operands.py): sizes, layers, expected kernels, ids
NGF = 32
C_LARGE = 2 * NGF                                  # channels of the widest full-resolution tensor (stored as cpad: 64)
SIZES = ((129, 256, 256), (255, 256, 256), (131, 250, 262))
BASE_SIZE = (127, 256, 256)                        # every byte offset below 2^31: where the summed-gradient bars are measured
PERIOD = 12
NLATENT = 16
EDGE = 1e-5   # |pre-activation| below which the ReLU behind a norm counts as sitting on its kink (see _mask_edges)

# name: (input channels, output channels, stride, transposed, the side the large tensor is on)
LAYERS = {
    "conv32to64": (32, 64, 1, False, "out"),
    "conv64to128s2": (64, 128, 2, False, "in"),
    "convT128to64": (128, 64, 2, True, "out"),
    "conv64to32": (64, 32, 1, False, "in"),
}
PASSES = ("fwd", "dgrad", "wgrad")
NORMS = ("in", "cin")
NORM_PASSES = ("eval_fwd", "train_fwd_dx", "train_params")

# short name in the test id -> substring of acg_last_kernel
KERNELS = {"rows": "conv_rows_x3<32,64>", "rp": "RP=1", "ws": "igemm_conv_x3_ws", "ph4": "igemm_conv_ph4", "krow_s": "wgrad_x3_krow_s<",
           "krowg": "wgrad_x3_krowg<NT=3,IS=2,BCI=64>", "bf16tile": "igemm_conv_bf16<", "wgrad_bf16": "wgrad_bf16<",
           "f32tile": "igemm_conv_f32<", "wgrad_f32": "wgrad_f32"}
_FAST = {   # bf16x3, W a multiple of 128: (forward, data gradient, weight gradient)
    "conv32to64": ("rows", "rp", "krow_s"), "conv64to128s2": ("ws", "ph4", "krowg"),
    "convT128to64": ("ph4", "ws", "krowg"), "conv64to32": ("rp", "rows", "krow_s")}
_FALLBACK = {   # bf16x3, W = 262: the wave-specialised tile has no width condition, the others fall to the generic tiles
    "conv32to64": ("bf16tile", "bf16tile", "wgrad_bf16"), "conv64to128s2": ("ws", "bf16tile", "wgrad_bf16"),
    "convT128to64": ("bf16tile", "ws", "wgrad_bf16"), "conv64to32": ("bf16tile", "bf16tile", "wgrad_bf16")}

# max-abs error / max-abs value of the summed gradients at 127 x 256 x 256 against float64 (measured on one MI355X)
BASE_127 = {
    ("conv32to64", "bf16x3"): {"dw": 5.67e-06, "db": 6.22e-07}, ("conv32to64", "f32"): {"dw": 3.49e-06, "db": 1.09e-06},
    ("conv64to128s2", "bf16x3"): {"dw": 4.90e-06, "db": 6.00e-07}, ("conv64to128s2", "f32"): {"dw": 3.78e-06, "db": 8.19e-07},
    ("convT128to64", "bf16x3"): {"dw": 5.76e-06, "db": 5.74e-07}, ("convT128to64", "f32"): {"dw": 4.08e-06, "db": 3.88e-07},
    ("conv64to32", "bf16x3"): {"dw": 6.55e-06, "db": 4.57e-07}, ("conv64to32", "f32"): {"dw": 3.69e-06, "db": 9.24e-07},
    ("in", "norm"): {"dscale": 3.08e-07, "dshift": 2.93e-07},
    ("cin", "norm"): {"dscale_w": 2.08e-07, "dscale_b": 3.45e-07, "dshift_w": 2.75e-07, "dshift_b": 2.97e-07},
}


def expected_kernel(layer, what, size, prec):
    """short name (KERNELS) of the kernel the dispatcher must take for this pass"""
    if prec == "f32":
        return "wgrad_f32" if what == "wgrad" else "f32tile"
    return (_FAST if size[2] % 128 == 0 else _FALLBACK)[layer][PASSES.index(what)]


def layer_shapes(layer, size):
    """-> (input shape, output shape), NHWC, of `layer` when its large side is the 64-channel tensor of `size`"""
    Ci, Co, stride, tr, side = LAYERS[layer]
    N, H, W = size
    assert (Co if side == "out" else Ci) == C_LARGE
    if stride == 1:
        return (N, H, W, Ci), (N, H, W, Co)
    assert H % 2 == 0 and W % 2 == 0
    if tr:
        return (N, H // 2, W // 2, Ci), (N, H, W, Co)
    return (N, H, W, Ci), (N, H // 2, W // 2, Co)


def nbytes(shape):
    n = 4
    for s in shape:
        n *= s
    return n


def image_class(i):
    """-> (k, s): image i is s * base_k"""
    return i % 3, 2.0 ** ((i % 4) - 1)


LARGE_CONV_CASES = [(layer, what, size, prec) for layer in LAYERS for what in PASSES for size in SIZES for prec in ("bf16x3", "f32")]
LARGE_NORM_CASES = [(kind, what, size) for kind in NORMS for what in NORM_PASSES for size in SIZES]


def conv_id(case):
    layer, what, size, prec = case
    return "%s_%s_%dx%dx%d_%s_%s" % ((layer, what) + size + (prec, expected_kernel(layer, what, size, prec)))


def norm_id(case):
    kind, what, size = case
    entry = {"eval_fwd": "norm_stats+norm_apply", "train_fwd_dx": "norm_apply+norm_bwd", "train_params": "norm_bwd"}[what]
    return "%s_%s_%dx%dx%d_%s" % ((kind, what) + size + (entry,))
