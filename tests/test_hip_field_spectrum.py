"""GPU tests of the whole-field spectra: acg_field_spectrum and acg_field_cross_spectrum against tests/field_spectrum_ref.py on
every shape of its list (each names the edge it walks), their exact cases, bits, paths and refusals,
model.translate_field_spectrum against translate_coherence and a composition made here, and
`dtgan_amd.test --metric field_spectrum` on 20 x 28 fields."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import cross_spectrum_ref as X
import field_spectrum_ref as F
import spectrum_ref as R
from eval_cases import make_experiment
from field_cases import LAYOUTS, field_operand as _device
from field_spectrum_ref import CTAU, TAU      # the bars, stated beside the reference
from model_cases import tiny_model

pytestmark = pytest.mark.gpu

ROWS = 2
EVEN_W = ((18, 30), (31, 16), (20, 28), (1024, 1000))


@functools.lru_cache(maxsize=None)
def _case(kind, H, W):
    """the fields (ROWS, 3, H, W), their reference spectra and mean squares"""
    x = F.make_fields(kind, H, W, rows=ROWS, C=3)
    return x, F.rapsd(x), np.mean(x.astype(np.float64) ** 2, axis=(-2, -1))


def _spectrum(xd, C, layout):
    from dtgan_amd import ops
    out = ops.field_spectrum(xd, C, layout)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _cross(xd, yd, C, lx, ly, x_per_y=1):
    from dtgan_amd import ops
    out = ops.field_cross_spectrum(xd, yd, C, lx, ly, x_per_y=x_per_y)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _within(psd, ref, E, what):
    R.within(psd, ref, E, what, TAU)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("H,W", F.SHAPES)
def test_kernel_matches_reference(H, W):
    """every kind at every shape; every layout up to 321 x 321, above one layout per kind, all of them over the kinds"""
    for i, kind in enumerate(F.FIELD_KINDS):
        x, ref, E = _case(kind, H, W)
        for layout, C, Cp in (LAYOUTS if H * W <= F.LARGE else [LAYOUTS[i % len(LAYOUTS)]]):
            got = _spectrum(_device(x, layout, C, Cp), C, layout)
            assert got.shape == (ROWS, C, F.bins(H, W))
            _within(got, ref[:, :C], E[:, :C], "%s %dx%d %s C=%d Cp=%d" % (kind, H, W, layout, C, Cp))


@pytest.mark.parametrize("H,W", F.SHAPES)
def test_exact_cases_leak_nothing(H, W):
    const = np.full((1, 3, H, W), 0.7, dtype=np.float32)
    got = _spectrum(_device(const, "nhwc", 3, 4), 3, "nhwc")
    E = np.float64(np.float32(0.7)) ** 2
    print("constant %dx%d: largest bin beyond 0 %.3e (allowed %.3e)" % (H, W, got[..., 1:].max(), TAU ** 2 * E))
    assert np.all(np.abs(got[..., 1:]) <= TAU ** 2 * E)
    assert np.all(np.abs(got[..., 0] - E * H * W) <= (2 * TAU + TAU ** 2) * E * H * W)     # the bound at ref = E H W
    assert np.allclose(got[..., 0], E * H * W, rtol=1e-4)
    wave, ref, Ew = _case("plane_wave", H, W)
    b = int(F.bin_index(H, W)[3, 4])
    assert b < F.bins(H, W)
    got = _spectrum(_device(wave, "nchw", 3, 3), 3, "nchw")
    others = np.delete(got, b, axis=-1)
    print("plane wave %dx%d: bin %d, largest other bin %.3e (allowed %.3e)" % (H, W, b, np.abs(others).max(), TAU ** 2 * Ew.min()))
    assert np.all(np.abs(others) <= TAU ** 2 * Ew[..., None])
    assert np.allclose(got[..., b], (H * W / 2.) / F.bin_counts(H, W)[b], rtol=1e-4)


@pytest.mark.parametrize("H,W", EVEN_W)
def test_the_nyquist_column_away_from_fy_0(H, W):
    """(-1)^w cos(2 pi m h / H): the cells (+-m, W/2).  The last m whose ring is still a bin holds H W / 2 there; one row
    further the cells are dropped and every ring stays empty"""
    nb, col = F.bins(H, W), F.bin_index(H, W)[:, W // 2]
    inside = [m for m in range(1, (H - 1) // 2 + 1) if col[m] < nb]
    assert inside and inside[-1] + 1 <= (H - 1) // 2
    h, w = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for m, layout, Cp in ((inside[-1], "nhwc", 4), (inside[-1] + 1, "nchw", 3)):
        x = np.broadcast_to((1.0 - 2.0 * (w % 2)) * np.cos(2 * np.pi * m * h / H), (1, 3, H, W)).astype(np.float32)
        E = np.mean(x.astype(np.float64) ** 2, axis=(-2, -1))
        got = _spectrum(_device(x, layout, 3, Cp), 3, layout)
        b = int(col[m])
        empty = np.delete(got, b, axis=-1) if b < nb else got
        print("nyquist column %dx%d m=%d: bin %d, largest empty bin %.3e (allowed %.3e)" % (H, W, m, b, np.abs(empty).max(), TAU ** 2 * E.min()))
        assert np.all(np.isfinite(got)) and np.all(np.abs(empty) <= TAU ** 2 * E[..., None])
        if b < nb:
            assert np.allclose(got[..., b], (H * W / 2.) / F.bin_counts(H, W)[b], rtol=1e-4)


@pytest.mark.parametrize("H,W", [s for s in F.SHAPES if s[0] * s[1] <= F.LARGE] + [(1000, 1024)])
def test_repeatable_and_the_same_bits_in_every_layout(H, W):
    x, _, _ = _case("tanh_red", H, W)
    nhwc, nchw = _device(x, "nhwc", 3, 4), _device(x, "nchw", 3, 3)
    a, b = _spectrum(nhwc, 3, "nhwc"), _spectrum(nhwc, 3, "nhwc")
    assert _same_bits(a, b)
    assert _same_bits(a, _spectrum(nchw, 3, "nchw"))
    assert _same_bits(a, _spectrum(_device(x, "nhwc", 3, 16, seed=1), 3, "nhwc"))


@pytest.mark.parametrize("S", (16, 64, 256))
def test_power_of_two_squares_are_forwarded_bit_for_bit(S):
    from dtgan_amd import _lib, ops
    x, y = R.make_fields("tanh_red", S, rows=3, C=3), R.make_fields("red", S, rows=1, C=3)
    xd, yd = _device(x, "nhwc", 3, 4), _device(y, "nchw", 3, 3)
    assert torch.equal(ops.field_spectrum(xd, 3, "nhwc"), ops.radial_spectrum(xd, 3, "nhwc"))
    want = _lib.query("acg_last_kernel").decode()
    ops.field_spectrum(xd, 3, "nhwc")
    assert _lib.query("acg_last_kernel").decode() == want and want.startswith("spectrum_")
    assert torch.equal(ops.field_cross_spectrum(xd, yd, 3, "nhwc", "nchw", x_per_y=3), ops.cross_spectrum(xd, yd, 3, "nhwc", "nchw", x_per_y=3))
    assert _lib.query("acg_field_spectrum_workspace_bytes", 3, 3, S, S) == _lib.query("acg_radial_spectrum_workspace_bytes", 3, 3, S)
    assert _lib.query("acg_field_cross_spectrum_workspace_bytes", 3, 3, S, S) == _lib.query("acg_cross_spectrum_workspace_bytes", 3, 3, S)


@functools.lru_cache(maxsize=None)
def _pair_case(H, W):
    """x (3 ROWS, 3, H, W): three members per truth, y (ROWS, 3, H, W), the reference triples and the mean squares"""
    x0, y = F.make_pair(H, W, rows=ROWS, C=3)
    x = np.stack([x0, np.float32(0.5) * x0 + np.float32(0.5) * y, F.make_fields("white", H, W, rows=ROWS, C=3)], axis=1)
    x = np.ascontiguousarray(x.reshape(3 * ROWS, 3, H, W))
    yy = np.repeat(y, 3, axis=0)
    ms = lambda v: np.mean(v.astype(np.float64) ** 2, axis=(-2, -1))
    return x, y, F.cross_spectrum(x, yy), ms(x), ms(yy)


def _triples_within(got, ref, Ex, Ey, what):
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    _within(got[..., 0, :], ref[..., 0, :], Ex, what + " pxx")
    _within(got[..., 1, :], ref[..., 1, :], Ey, what + " pyy")
    d = np.abs(got[..., 2, :].astype(np.float64) - ref[..., 2, :])
    bound = X.cross_bound(ref, Ex, Ey, CTAU)
    print("%s cxy: tau needed %.3e (allowed %.3e)" % (what, X.cross_tolerance_needed(got[..., 2, :], ref, Ex, Ey), CTAU))
    assert np.all(d <= bound), (what, float((d / np.maximum(bound, 1e-300)).max()))


@pytest.mark.parametrize("H,W", F.SHAPES)
def test_cross_form_matches_reference_and_shares_the_transform(H, W):
    """three members per truth (x_per_y = 3), x NHWC C4 against a planar y.  Outside the forwarded squares Pxx and Pyy have
    the bits of field_spectrum(x) and field_spectrum(y): the two entry points share the transform and the products; the
    forwarded squares hold them to the bound, as test_hip_cross_spectrum does"""
    x, y, ref, Ex, Ey = _pair_case(H, W)
    xd, yd = _device(x, "nhwc", 3, 4), _device(y, "nchw", 3, 3)
    got = _cross(xd, yd, 3, "nhwc", "nchw", x_per_y=3)
    _triples_within(got, ref, Ex, Ey, "%dx%d" % (H, W))
    forwarded = H == W and H & (H - 1) == 0         # the square kernels' pair form promises its Pxx to the bound only
    if not forwarded:
        assert _same_bits(np.ascontiguousarray(got[:, :, 0]), _spectrum(xd, 3, "nhwc"))
        assert _same_bits(np.ascontiguousarray(got[::3, :, 1]), _spectrum(yd, 3, "nchw"))
    if H * W <= F.LARGE:
        assert _same_bits(got, _cross(_device(x, "nchw", 3, 3), _device(y, "nhwc", 3, 16, seed=2), 3, "nchw", "nhwc", x_per_y=3))
        assert _same_bits(got, _cross(xd, yd, 3, "nhwc", "nchw", x_per_y=3))
        same = _cross(yd, yd, 3, "nchw", "nchw")
        r = F.rapsd(y)
        Eyy = np.mean(y.astype(np.float64) ** 2, axis=(-2, -1))
        _triples_within(same, np.stack([r, r, r], axis=-2), Eyy, Eyy, "%dx%d x = y" % (H, W))
        assert forwarded or _same_bits(np.ascontiguousarray(same[:, :, 0]), np.ascontiguousarray(same[:, :, 1]))


def _padded(N):
    M = 1
    while M < 2 * N - 1:
        M <<= 1
    return N if N & (N - 1) == 0 else M


@pytest.mark.parametrize("H,W", F.SHAPES + ((64, 64), (64, 65)))
def test_the_path_a_shape_takes_and_its_workspace(H, W):
    """power-of-two squares are forwarded; everything else takes the row, column and ring passes, each axis
    direct (M = N) or Bluestein (M >= 2 N - 1); the workspace is the head of chirps and filters, the half spectra and the
    product planes"""
    from dtgan_amd import _lib
    x = F.make_fields("white", H, W, rows=1, C=2)
    xd = _device(x, "nchw", 2, 2)
    _spectrum(xd, 2, "nchw")
    k = _lib.query("acg_last_kernel").decode()
    _cross(xd, xd, 2, "nchw", "nchw")
    kc = _lib.query("acg_last_kernel").decode()
    r16 = lambda v: (v + 15) // 16 * 16
    if H == W and H & (H - 1) == 0:
        assert k in ("spectrum_field<%d>" % H, "spectrum_rows<%d> + spectrum_cols<%d>" % (H, H)), k
        assert kc.startswith("cross_spectrum_"), kc
        want = [_lib.query("acg_radial_spectrum_workspace_bytes", 1, 2, H), _lib.query("acg_cross_spectrum_workspace_bytes", 1, 2, H)]
    else:
        tail = "_rows<W=%d,M=%d> + %%s_cols<H=%d,M=%d> + rings" % (W, _padded(W), H, _padded(H))
        assert k == "field_spectrum" + tail % "field_spectrum", k
        assert kc == "field_cross_spectrum" + tail % "field_cross_spectrum", kc
        head, cells = r16((W + _padded(W) + H + _padded(H)) * 8), 2 * H * (W // 2 + 1)
        want = [head + r16(cells * 8) + r16(cells * 4), head + r16(cells * 16) + r16(cells * 12)]
    assert _lib.query("acg_field_spectrum_workspace_bytes", 1, 2, H, W) == want[0]
    assert _lib.query("acg_field_cross_spectrum_workspace_bytes", 1, 2, H, W) == want[1]


def test_kernels_refuse_bad_arguments_before_launching():
    from dtgan_amd import _lib, ops
    lib = _lib.load()
    x = torch.zeros(1 << 16, device="cuda")
    ws = torch.empty(1 << 22, dtype=torch.uint8, device="cuda")
    need, cneed = lib.acg_field_spectrum_workspace_bytes(2, 1, 20, 28), lib.acg_field_cross_spectrum_workspace_bytes(2, 1, 20, 28)
    assert 0 < need < cneed <= ws.numel()
    ok = dict(H=20, W=28, C=1, rows=2, per=1, row=560, pix=1, ws=ops._ptr(ws), nbytes=ws.numel())
    cases = [dict(H=15), dict(W=15), dict(H=1025), dict(W=2048), dict(C=0), dict(rows=0), dict(pix=0), dict(row=0),
             dict(ws=ctypes.c_void_p(ws.data_ptr() + 8)), dict(nbytes=need - 1, rc=-2, cross_nbytes=cneed - 1)]
    for over in cases:
        a = dict(ok, **over)
        out = torch.full((2, 1, 3, 11), -7.0, device="cuda")
        rc = lib.acg_field_spectrum(ops._ptr(x), a["rows"], a["C"], a["H"], a["W"], a["row"], a["pix"], a["H"] * a["W"], ops._ptr(out),
                                    a["ws"], a["nbytes"], ops._stream())
        msg = lib.acg_last_error().decode()
        assert rc == over.get("rc", -1) and msg.startswith("acg_field_spectrum:"), (over, rc, msg)
        rc = lib.acg_field_cross_spectrum(ops._ptr(x), ops._ptr(x), a["rows"], a["per"], a["C"], a["H"], a["W"], a["row"], a["pix"],
                                          a["H"] * a["W"], a["row"], a["pix"], a["H"] * a["W"], ops._ptr(out), a["ws"],
                                          over.get("cross_nbytes", a["nbytes"]), ops._stream())
        msg = lib.acg_last_error().decode()
        assert rc == over.get("rc", -1) and msg.startswith("acg_field_cross_spectrum:"), (over, rc, msg)
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()), over
    for over in (dict(per=3), dict(per=0)):                            # rows % x_per_y, and a stride of y alone
        out = torch.full((2, 1, 3, 11), -7.0, device="cuda")
        rc = lib.acg_field_cross_spectrum(ops._ptr(x), ops._ptr(x), 2, over["per"], 1, 20, 28, 560, 1, 560, 560, 1, 560, ops._ptr(out),
                                          ops._ptr(ws), ws.numel(), ops._stream())
        assert rc == -1 and lib.acg_last_error().decode().startswith("acg_field_cross_spectrum: x_per_y"), over
        assert bool((out == -7.0).all())
    rc = lib.acg_field_cross_spectrum(ops._ptr(x), ops._ptr(x), 2, 1, 1, 20, 28, 560, 1, 560, 560, 0, 560, ops._ptr(out), ops._ptr(ws),
                                      ws.numel(), ops._stream())
    assert rc == -1 and "strides" in lib.acg_last_error().decode()
    rc = lib.acg_field_spectrum(None, 2, 1, 20, 28, 560, 1, 560, ops._ptr(out), ops._ptr(ws), ws.numel(), ops._stream())
    assert rc == -1 and lib.acg_last_error().decode().startswith("acg_field_spectrum: null")
    assert bool((out == -7.0).all())
    with pytest.raises(_lib.AcgError, match="16..1024"):
        ops.field_spectrum(torch.zeros(1, 1, 8, 8, device="cuda"), 1, "nchw")
    with pytest.raises(_lib.AcgError, match="do not pair"):
        ops.field_cross_spectrum(torch.zeros(2, 1, 20, 28, device="cuda"), torch.zeros(2, 1, 28, 20, device="cuda"), 1, "nchw", "nchw")
    with pytest.raises(_lib.AcgError, match="power of two"):             # the square entry points keep their rule
        ops.radial_spectrum(torch.zeros(1, 1, 192, 192, device="cuda"), 1, "nchw")


# ---- model.translate_field_spectrum ----
S = 16


@pytest.fixture(scope="module")
def model():
    return tiny_model(grid_size=S, n_blocks=1)


def _rand(*shape, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(*shape, device="cuda", generator=g) * 2 - 1


def _flags(m):
    return [(mod, mod.training) for net in m._nets() for mod in net.modules()]


def test_one_window_is_translate_coherence_bit_for_bit(model):
    N, M = 3, 4
    A, B = _rand(N, 3, S, S, seed=1), _rand(N, 3, S, S, seed=2)
    z = torch.randn(N * M, 4, 1, 1, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    before = _flags(model)
    got = model.translate_field_spectrum(A, M, B, z=z)
    assert all(mod.training == t for mod, t in before) and torch.is_grad_enabled()
    want = model.translate_coherence(A, M, B, z=z)
    assert set(got) == {"members", "ens_mean"}
    assert tuple(got["members"].shape) == (N, M, 3, 3, S // 2 + 1) and tuple(got["ens_mean"].shape) == (N, 3, 3, S // 2 + 1)
    assert torch.equal(got["members"], want["members"]) and torch.equal(got["ens_mean"], want["ens_mean"])
    assert float(got["members"][..., 0, :].max()) > 0


def test_whole_fields_equal_a_composition_made_here(model):
    from dtgan_amd import ops
    N, M, H, W = 2, 3, 20, 28
    A, B = _rand(N, 3, H, W, seed=4), _rand(N, 3, H, W, seed=5)
    z = torch.randn(N * M, 4, 1, 1, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    with torch.no_grad():
        before = _flags(model)
        got = model.translate_field_spectrum(A, M, B, z=z, overlap=5)
        assert all(mod.training == t for mod, t in before) and not torch.is_grad_enabled()
    fields = model.translate_field(A, M, z=z, overlap=5)
    nb = F.bins(H, W)
    assert tuple(got["members"].shape) == (N, M, 3, 3, nb) and tuple(got["ens_mean"].shape) == (N, 3, 3, nb)
    want = ops.field_cross_spectrum(fields.flatten(0, 1), B, 3, "nchw", "nchw", x_per_y=M)
    assert torch.equal(got["members"].flatten(0, 1), want)
    f, b = fields.cpu().numpy(), B.cpu().numpy()
    assert np.array_equal(got["members"].cpu().numpy()[:, :, :, 0], ops.field_spectrum(fields.flatten(0, 1), 3, "nchw").view(N, M, 3, nb).cpu().numpy())
    mean = f.astype(np.float64).mean(1)
    ms = lambda v: np.mean(np.asarray(v, dtype=np.float64) ** 2, axis=(-2, -1))
    _triples_within(got["ens_mean"].cpu().numpy(), F.cross_spectrum(mean, b), ms(mean), ms(b), "ensemble mean 20x28")
    with pytest.raises(ValueError, match="does not pair"):
        model.translate_field_spectrum(A, M, B[:, :, :S], z=z)
    with pytest.raises(ValueError, match="does not pair"):
        model.translate_field_spectrum(A, M, None, z=z)
    with pytest.raises(ValueError, match="smaller than"):               # translate_field's own refusal
        model.translate_field_spectrum(A[:, :, :12], M, B[:, :, :12], z=z)


# ---- the driver ----
@pytest.fixture(scope="module")
def experiment(tmp_path_factory):
    """20 x 28 fields (6 train -> 3 dev + 3 train, 2 test) and the checkpoint of a seeded 16 x 16 model: the recipe of
    tests/test_hip_translate_field.py"""
    return make_experiment(tmp_path_factory.mktemp("field_spectrum_driver"), S, 6, 2, hw=(20, 28), seed=1, native_res=True)


def test_metric_field_spectrum_writes_both_families_and_repeats(experiment, capsys):
    from dtgan_amd import ops, test as T
    from dtgan_amd.dataloader import load_numpy_data
    prec = ops.get_precision()
    runs = []
    try:
        for res in ("fs_a", "fs_b"):
            T.test_model(["--chk_path", experiment["chk"], "--dataroot", experiment["data"], "--metric", "field_spectrum",
                          "--n_samples", "3", "--overlap", "5", "--res_dir", res])
            runs.append(dict(np.load(os.path.join(experiment["expr"], res, "field_spectrum.npz"))))
            assert not os.path.exists(os.path.join(experiment["expr"], res, "translate.npz"))
    finally:
        ops.set_precision(prec)
    out = capsys.readouterr().out
    for tag in ("DEV_LSD_B: ", "TEST_LSD_B: ", "DEV_LSD_A: ", "TEST_LSD_A: ", "DEV_K_EFF_B: ", "TEST_K_EFF_B: "):
        assert out.count(tag) == 2, tag
    a, b = runs
    pairs = ("members_B", "ens_mean_B", "fake_A")
    per_split = {"psd_real_B", "psd_members_B", "psd_ens_mean_B", "psd_real_A", "psd_fake_A", "lsd_B", "lsd_mean_B", "lsd_A"}
    per_split |= {"%s_%s" % (n, k) for n in ("sums", "coh", "r", "perr", "k_eff") for k in pairs}
    want = {"n_samples", "window", "overlap", "height", "width"} | {"%s_%s" % (s, k) for s in ("dev", "test") for k in per_split}
    assert set(a) == want
    assert tuple(int(a[k]) for k in ("n_samples", "window", "overlap", "height", "width")) == (3, S, 5, 20, 28)
    nb = 11
    for split in ("dev", "test"):
        for k in ("psd_real_B", "psd_members_B", "psd_ens_mean_B", "psd_real_A", "psd_fake_A"):
            v = a["%s_%s" % (split, k)]
            assert v.shape == (3, nb) and v.dtype == np.float64 and np.isfinite(v).all() and (v > 0).all(), (split, k)
        for k in pairs:
            assert a["%s_sums_%s" % (split, k)].shape == (3, 3, nb) and a["%s_sums_%s" % (split, k)].dtype == np.float64
            for n in ("coh", "r", "perr"):
                v = a["%s_%s_%s" % (split, n, k)]
                assert v.shape == (3, nb) and v.dtype == np.float64 and np.isfinite(v).all(), (split, n, k)
            ke = a["%s_k_eff_%s" % (split, k)]
            assert ke.shape == (3,) and ke.dtype == np.int64 and (ke >= 1).all() and (ke <= nb).all()
            assert (a["%s_coh_%s" % (split, k)] >= 0).all() and (a["%s_coh_%s" % (split, k)] <= 1).all()
        for k in ("lsd_B", "lsd_mean_B", "lsd_A"):
            v = a["%s_%s" % (split, k)]
            assert v.shape == () and np.isfinite(v) and v >= 0
    assert all(np.array_equal(a[k], b[k]) for k in want)
    assert "%.4f" % float(a["test_lsd_B"]) == out.split("TEST_LSD_B: ")[1].split(",")[0].strip()
    # the spectrum of the loaded test B fields, whole: Pyy of the pairs against the float64 reference
    testB = load_numpy_data(experiment["data"], grid_size=S, native_res=True, centre_eval=False)[5]
    assert testB.shape == (2, 3, 20, 28)
    ref, E = F.rapsd(testB), np.mean(testB.astype(np.float64) ** 2, axis=(-2, -1))
    bound = (TAU * np.sqrt(ref * E[..., None]) + TAU ** 2 * E[..., None]).mean(0)
    assert np.all(np.abs(a["test_psd_real_B"] - ref.mean(0)) <= bound)
