"""CPU tests of the connected components of excursion sets: the reference (tests/components_ref.py) against closed forms and
additivity, the holes of ops.components_summary against the labelled holes of minkowski_ref.functionals_brute,
ops.components_summary / components_distance, the option parser, the header and the host-side refusals of ops.components."""
import os

import numpy as np
import pytest
import torch

import abi
import components_ref as R
import minkowski_ref as K
from eval_cases import parse_test

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO = np.zeros((1, 1), np.float32)


def _one(kind, H, W, conn):
    """the 25 values of the kind's mask at threshold 0"""
    return R.stats(R.make_fields(kind, 1, 1, H, W, ZERO), ZERO, conn)[0, 0, 0]


def _hist(*areas):
    h = np.zeros(R.COMP_BINS, dtype=np.int64)
    for a in areas:
        h[int(a).bit_length() - 1] += 1
    return h.tolist()


@pytest.mark.parametrize("H,W", ((1, 1), (1, 9), (6, 4), (33, 65), (70, 130)))
def test_closed_forms_of_the_binary_kinds(H, W):
    P = H * W
    for conn in (4, 8):
        assert _one("full", H, W, conn).tolist() == [1, P, P * P, 1] + _hist(P)
        assert _one("empty", H, W, conn).tolist() == [0] * R.COMP_STATS
        # concentric rings at the even distances d = 0, 2, .. from the border: a component each, every one apart from the others
        rings = _one("rings", H, W, conn)
        dmax = (min(H, W) - 1) // 2
        assert rings[0] == dmax // 2 + 1 and rings[3] == 1
        comb = _one("comb", H, W, conn)                            # the teeth hang together along the last row only
        assert comb[0] == 1 and comb[1] == comb[2] ** 0.5 == (W + 1) // 2 * (H - 1) + W and comb[3] == 1
    black = (P + 1) // 2
    m, edge = R.mask("checker", H, W), np.zeros((H, W), dtype=bool)
    edge[[0, -1]] = edge[:, [0, -1]] = True
    assert _one("checker", H, W, 4).tolist() == [black, black, black, int((m & edge).sum())] + _hist(*[1] * black)
    if min(H, W) >= 2:
        assert _one("checker", H, W, 8).tolist() == [1, black, black * black, 1] + _hist(black)
    diag = R.mask("diag", H, W)
    d4, d8 = _one("diag", H, W, 4), _one("diag", H, W, 8)
    assert d4[0] == d4[1] == d4[2] == diag.sum() and d4[4] == d4[0]           # singletons
    assert d8[0] == (H + W - 2) // 3 + 1 and d8[1] == diag.sum() and d8[3] == d8[0]   # anti-diagonal stripes, all reach the border


def test_the_holes_of_the_rings():
    from dtgan_amd import ops
    for H, W in ((9, 9), (10, 14), (11, 8), (33, 65)):
        x = R.make_fields("rings", 1, 1, H, W, ZERO)
        dmax = (min(H, W) - 1) // 2
        for conn in (4, 8):
            s = ops.components_summary(R.stats(x, ZERO, conn), K.counts(x, ZERO), 1, H * W, conn)
            # the gaps at the odd distances: k - 1 between the k rings, and the centre where the innermost distance is odd
            assert s["components"].item() == dmax // 2 + 1 and s["holes"].item() == (dmax + 1) // 2, (H, W, conn)


@pytest.mark.parametrize("H,W", ((64, 128), (97, 131), (256, 256)))
def test_the_spiral_and_the_comb_are_one_component_in_every_tile(H, W):
    for kind in ("spiral", "comb"):
        m = R.mask(kind, H, W)
        tiles = m[:H // R.TH * R.TH, :W // R.TW * R.TW].reshape(H // R.TH, R.TH, W // R.TW, R.TW).any(axis=(1, 3))
        assert tiles.all()
        for conn in (4, 8):
            out, lab = R.plane(m, conn, labels=True)
            assert out[0] == 1 and out[1] == m.sum() and out[2] == out[1] ** 2 and out[3] == 1
            assert np.array_equal(lab, np.where(m, 1, 0))           # the first cell is (0, 0): label 1
    sp = R.mask("spiral", H, W)
    x = np.where(sp, 1.0, -1.0).astype(np.float32).reshape(1, 1, H, W)
    f = K.functionals(K.counts(x, ZERO))
    assert f["euler8"].item() == 1 and f["euler4"].item() == 1       # an arm with gaps: it encloses nothing, even diagonally
    assert abs(sp.mean() - 0.5) < 0.05


def test_the_corners_join_under_8_and_part_under_4():
    H, W = 3 * R.TH + 5, 3 * R.TW + 5
    m = R.mask("corners", H, W)
    assert m.sum() == 2 * 9
    a4, a8 = R.plane(m, 4), R.plane(m, 8)
    assert a4[:5].tolist() == [18, 18, 18, 0, 18] and a8[:6].tolist() == [9, 18, 36, 0, 0, 9]
    for r0 in range(R.TH, H, R.TH):                                  # both diagonals occur, each across a tile corner
        for c0 in range(R.TW, W, R.TW):
            q = m[r0 - 1:r0 + 1, c0 - 1:c0 + 1]
            assert q.sum() == 2 and (q[0, 0] and q[1, 1] or q[0, 1] and q[1, 0])
    assert m[R.TH - 1, R.TW - 1] and m[R.TH - 1, 2 * R.TW]


def test_percolation_noise_is_ragged():
    for kind, p in (("perc41", 0.41), ("perc59", 0.59)):
        m = R.mask(kind, 256, 256)
        assert abs(m.mean() - p) < 0.01
        n4, n8 = R.plane(m, 4), R.plane(m, 8)
        assert n4[0] > n8[0] >= 1 and n4[1] == n8[1] == m.sum() and n8[2] > n4[2]
        assert n4[4:].sum() == n4[0] and n8[4:].sum() == n8[0]
    assert not np.array_equal(R.mask("perc41", 64, 64, 0), R.mask("perc41", 64, 64, 7))


def test_labels_bins_and_the_mask_convention():
    m = np.array([[1, 1, 0, 0, 1], [0, 0, 0, 1, 0], [1, 0, 0, 0, 0], [1, 1, 1, 0, 1]], dtype=bool)
    out, lab = R.plane(m, 4, labels=True)
    assert out[:4].tolist() == [5, 9, 4 + 1 + 1 + 16 + 1, 4] and out[4:7].tolist() == [3, 1, 1]
    assert lab.tolist() == [[1, 1, 0, 0, 5], [0, 0, 0, 9, 0], [11, 0, 0, 0, 0], [11, 11, 11, 0, 20]]
    out, lab = R.plane(m, 8, labels=True)
    assert out[:4].tolist() == [4, 9, 4 + 4 + 16 + 1, 4] and lab[1, 3] == 5 and lab[0, 4] == 5
    # x == thr inside, NaN outside, +inf inside, repeated thresholds repeat the plane
    thr = np.array([[0.0, 0.0, 1.0]], dtype=np.float32)
    x = np.array([[0.0, np.nan, np.inf], [-1.0, 1.0, np.nextafter(np.float32(0), np.float32(-1))]], dtype=np.float32).reshape(1, 1, 2, 3)
    s, lab = R.stats(x, thr, 8, labels=True)
    assert lab[0, 0, 0].tolist() == lab[0, 0, 1].tolist() == [[1, 0, 1], [0, 1, 0]] and lab[0, 0, 2].tolist() == [[0, 0, 3], [0, 3, 0]]
    assert s[0, 0, :, 0].tolist() == [1, 1, 1] and R.stats(x, thr, 4)[0, 0, :, 0].tolist() == [3, 3, 2]
    assert s.dtype == np.int64 and lab.dtype == np.int32


def test_the_statistics_add_over_fields_and_do_not_mix_channels():
    thr = K.make_thresholds(3, 7, seed=2)
    x = K.make_fields("special", 4, 3, 12, 10, thr, seed=1)
    for conn in (4, 8):
        n = R.stats(x, thr, conn)
        assert n.shape == (4, 3, 7, 25) and np.array_equal(n.sum(0), sum(R.stats(x[r:r + 1], thr, conn)[0] for r in range(4)))
        for c in range(3):
            assert np.array_equal(n[:, c], R.stats(x[:, c:c + 1], thr[c:c + 1], conn)[:, 0])
        assert np.array_equal(n[..., 1], K.counts(x, thr)[..., 0]) and np.array_equal(n[..., 4:].sum(-1), n[..., 0])


@pytest.mark.parametrize("H,W", ((9, 13), (33, 65)))
def test_the_holes_of_the_summary_are_the_labelled_holes(H, W):
    """holes = components - euler: the brute force labels the background of the padded complement"""
    from dtgan_amd import ops
    from scipy import ndimage
    thr = K.make_thresholds(2, 5, seed=5)
    x = K.make_fields("smooth", 2, 2, H, W, thr, seed=3)
    counts = K.counts(x, thr)
    for conn, bg in ((4, R._STRUCTURE[8]), (8, R._STRUCTURE[4])):
        st = R.stats(x, thr, conn)
        per_field = ops.components_summary(st, counts, 1, H * W, conn)
        assert per_field["holes"].shape == (2, 2, 5)
        for r in range(2):
            for c in range(2):
                brute = K.functionals_brute(x[r, c], thr[c])
                assert np.array_equal(st[r, c, :, 0] - per_field["holes"][r, c], brute["euler%d" % conn])
                for t in range(5):
                    with np.errstate(invalid="ignore"):
                        mask = x[r, c] >= thr[c, t]
                    assert per_field["holes"][r, c, t] == ndimage.label(~np.pad(mask, 2), structure=bg)[1] - 1
        pooled = ops.components_summary(st.sum(0), counts.sum(0), 2, 2 * H * W, conn)
        assert np.array_equal(pooled["holes"], per_field["holes"].sum(0))


def test_summary_and_distance():
    from dtgan_amd import ops
    assert ops.COMP_STATS == 25 and ops.COMP_BINS == 21
    H = W = 32
    thr = np.array([[-0.5, 0.0, 0.5, 9.0]] * 2, dtype=np.float32)    # nothing reaches 9: the empty set
    rs = np.random.RandomState(0)
    x = K._box_smooth(rs.standard_normal((6, 2, H, W)), 1).astype(np.float32) * 2
    st, counts = R.stats(x, thr, 8), K.counts(x, thr)
    s = ops.components_summary(st.sum(0), counts.sum(0), 6, 6 * H * W, 8)
    assert set(s) == {"components", "holes", "components_density", "holes_density", "mean_area", "weighted_area", "border_fraction", "size_pdf"}
    tot = st.sum(0).astype(np.float64)
    assert all(v.dtype == np.float64 for v in s.values()) and s["components"].shape == (2, 4) and s["size_pdf"].shape == (2, 4, 21)
    assert np.array_equal(s["components"], tot[..., 0]) and np.array_equal(s["components_density"], tot[..., 0] / (6 * H * W))
    assert np.array_equal(s["holes"], tot[..., 0] - K.functionals(counts.sum(0))["euler8"]) and np.all(s["holes"] >= 0)
    assert np.array_equal(s["holes_density"], s["holes"] / (6 * H * W))
    live = slice(0, 3)
    assert np.array_equal(s["mean_area"][:, live], tot[:, live, 1] / tot[:, live, 0])
    assert np.array_equal(s["weighted_area"][:, live], tot[:, live, 2] / tot[:, live, 1])
    assert np.array_equal(s["border_fraction"][:, live], tot[:, live, 3] / tot[:, live, 0])
    assert np.array_equal(s["size_pdf"][:, live], tot[:, live, 4:] / tot[:, live, :1]) and np.allclose(s["size_pdf"][:, live].sum(-1), 1)
    assert np.all(s["weighted_area"][:, live] >= s["mean_area"][:, live])
    # the empty set: no component, so no mean, no fraction and no distribution; the counts are plain zeros
    for k in ("mean_area", "weighted_area", "border_fraction"):
        assert np.all(np.isnan(s[k][:, 3])), k
    assert np.all(np.isnan(s["size_pdf"][:, 3])) and np.all(s["components"][:, 3] == 0) and np.all(s["holes"][:, 3] == 0)
    s4 = ops.components_summary(R.stats(x, thr, 4).sum(0), counts.sum(0), 6, 6 * H * W, 4)
    assert np.all(s4["components"][:, live] > s["components"][:, live])
    per_field = ops.components_summary(st, counts, 1, H * W, 8)    # leading axes pass through
    assert per_field["size_pdf"].shape == (6, 2, 4, 21)
    d = ops.components_distance(s, s)
    assert set(d) == {"dist_components", "dist_holes", "dist_size"} and all(v.shape == (2,) and np.all(v == 0) for v in d.values())
    d = ops.components_distance(s, s4)
    assert np.array_equal(d["dist_components"], np.abs(s["components_density"] - s4["components_density"]).mean(-1)) and np.all(d["dist_components"] > 0)
    assert np.array_equal(d["dist_holes"], np.abs(s["holes_density"] - s4["holes_density"]).mean(-1))
    tv = 0.5 * np.abs(s["size_pdf"][:, live] - s4["size_pdf"][:, live]).sum(-1)
    assert np.allclose(d["dist_size"], tv.mean(-1), rtol=1e-15, atol=0) and np.all(d["dist_size"] > 0) and np.all(d["dist_size"] <= 1)
    # thresholds where either side has no component are left out; none left: NaN
    only_empty = {k: v[:, 3:] for k, v in s.items()}
    assert np.all(np.isnan(ops.components_distance(only_empty, only_empty)["dist_size"]))
    assert np.all(ops.components_distance(only_empty, only_empty)["dist_components"] == 0)
    half = {k: v.copy() for k, v in s.items()}
    half["size_pdf"][:, 0] = np.nan
    assert np.allclose(ops.components_distance(half, s4)["dist_size"], tv[:, 1:].mean(-1), rtol=1e-15, atol=0)
    assert ops.components_distance(per_field, per_field)["dist_size"].shape == (6, 2)
    for bad in ((np.zeros((2, 3, 24)), np.zeros((2, 3, 5)), 1, 10, 8), (np.zeros((2, 3, 25)), np.zeros((2, 4, 5)), 1, 10, 8),
                (np.zeros((2, 3, 25)), np.zeros((2, 3, 5)), 1, 0, 8), (np.zeros((2, 3, 25)), np.zeros((2, 3, 5)), 0, 10, 8),
                (np.zeros((2, 3, 25)), np.zeros((2, 3, 5)), 1, 10, 6), (np.zeros(25), np.zeros(5), 1, 10, 8)):
        with pytest.raises(ValueError, match="components_summary"):
            ops.components_summary(*bad)
    with pytest.raises(ValueError, match="densities"):
        ops.components_distance(s, per_field)
    with pytest.raises(ValueError, match="size_pdf"):
        ops.components_distance(s, dict(s, size_pdf=s["size_pdf"][..., :20]))


def _parse(*extra):
    return parse_test("minkowski", *extra)


def test_the_parser_takes_the_connectivity():
    from dtgan_amd import eval_metrics as EM, options as O
    assert _parse().mink_components == 0
    assert _parse("--mink_components", "4").mink_components == 4 and _parse("--mink_components", "8").mink_components == 8
    assert _parse("--mink_components", "0", "--mink_bins", "7").mink_components == 0
    for bad in ("1", "6", "-8", "x", "4.0", "48"):
        with pytest.raises(SystemExit):
            _parse("--mink_components", bad)
    for metric in ("marginal", "fss", "mse", "minkowski"):         # the others keep parsing
        assert O.TestOptions().parse(["--chk_path", "c", "--dataroot", "d", "--metric", metric]).metric == metric
    assert "mink_components" in O.TestOptions.__doc__
    doc = [m.doc for m in EM.METRICS if m.name == "minkowski"][0]
    assert doc.startswith("  minkowski ") and "(new)" in doc and "--mink_components" in doc and "ops.components_summary" in doc


def test_the_header_declares_both_entries_and_the_binding_matches():
    from dtgan_amd import _lib
    for name, nargs in (("acg_components_workspace_bytes", 5), ("acg_components", 16)):
        assert len(abi.header_args(name)) == len(_lib.SIGNATURES[name][1]) == nargs, name
    mk = open(os.path.join(ROOT, "domain-transfer-gan_amd", "csrc", "Makefile")).read()
    assert "components.hip" in mk
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`acg_components`" in doc and "acg_components_workspace_bytes" in doc and "ops.components_summary" in doc
    lib = _lib.load()
    up = lambda n: (n + 15) // 16 * 16
    # whole planes of 8 H W bytes (int32 parents, uint32 areas), each rounded up to 16; at most what fits 256 MiB, at least one
    assert lib.acg_components_workspace_bytes(2, 3, 64, 64, 31) == 2 * 3 * 31 * 64 * 64 * 8
    assert lib.acg_components_workspace_bytes(1, 1, 7, 5, 1) == up(7 * 5 * 8) and lib.acg_components_workspace_bytes(1, 2, 1, 1, 3) == 6 * 16
    assert lib.acg_components_workspace_bytes(255, 3, 256, 256, 31) == 256 << 20
    assert lib.acg_components_workspace_bytes(3, 1, 1024, 1024, 255) == 256 << 20
    assert lib.acg_components_workspace_bytes(1, 1, 1024, 1024, 1) == 8 << 20
    for bad in ((0, 1, 8, 8, 1), (1, 0, 8, 8, 1), (1, 1, 0, 8, 1), (1, 1, 8, 1025, 1), (1, 1, 8, 8, 0), (1, 1, 8, 8, 256), (1 << 30, 4, 8, 8, 1)):
        assert lib.acg_components_workspace_bytes(*bad) == 0, bad


def test_ops_refuses_on_the_host_before_any_device_call(monkeypatch):
    from dtgan_amd import _lib, ops

    def no_device(*a, **k):
        raise AssertionError("a refusal reached the library")
    monkeypatch.setattr(_lib, "call", no_device)
    monkeypatch.setattr(_lib, "query", no_device)
    z = lambda *shape: torch.zeros(shape)
    thr = np.zeros((1, 2), np.float32)
    with pytest.raises(_lib.AcgError, match="layout"):
        ops.components(z(1, 1, 32, 32), 1, "chwn", thr)
    with pytest.raises(_lib.AcgError, match="4-d"):
        ops.components(z(1, 32, 32), 1, "nchw", thr)
    with pytest.raises(_lib.AcgError, match="1024"):
        ops.components(z(1, 1, 4, 1025), 1, "nchw", thr)
    with pytest.raises(_lib.AcgError, match="1024"):
        ops.components(z(1, 1025, 4, 4), 1, "nhwc", thr)
    with pytest.raises(_lib.AcgError, match="channels"):
        ops.components(z(2, 8, 8, 4), 5, "nhwc", np.zeros((5, 1), np.float32))
    for bad in (0, 6, 16, "8", None):
        with pytest.raises(_lib.AcgError, match="connectivity"):
            ops.components(z(2, 1, 8, 8), 1, "nchw", thr, conn=bad)
    for bad in (np.zeros((2, 2), np.float32), np.zeros(2, np.float32), np.zeros((1, 256), np.float32), np.zeros((1, 0), np.float32),
                np.array([[1.0, 0.0]]), np.array([[0.0, np.nan]]), np.array([[0.0, np.inf]])):
        with pytest.raises(_lib.AcgError, match="components: thresholds"):
            ops.components(z(2, 1, 8, 8), 1, "nchw", bad)
    for bad in (torch.zeros(2, 2), torch.zeros(1, 256), torch.zeros(1, 2, dtype=torch.float64)):      # tensors: shape and type only
        with pytest.raises(_lib.AcgError, match="components: thresholds"):
            ops.components(z(2, 1, 8, 8), 1, "nchw", bad)
    for bad in (torch.zeros(2, 1, 2, 24), torch.zeros(2, 1, 2, 25), torch.zeros(2, 1, 25, 2, dtype=torch.int64).transpose(2, 3)):
        with pytest.raises(_lib.AcgError, match="out"):
            ops.components(z(2, 1, 8, 8), 1, "nchw", thr, out=bad)
    for bad in (torch.zeros(2, 1, 2, 8, 8), torch.zeros(2, 1, 2, 8, 9, dtype=torch.int32), torch.zeros(2, 1, 2, 8, 8, dtype=torch.int64)):
        with pytest.raises(_lib.AcgError, match="labels"):
            ops.components(z(2, 1, 8, 8), 1, "nchw", thr, labels=bad)
    with pytest.raises(_lib.AcgError, match="labels"):               # 2^31 cells of labels
        ops.components(z(9, 1, 1024, 1024), 1, "nchw", np.zeros((1, 255), np.float32), labels=True)
    with pytest.raises(_lib.AcgError, match="ROCm device"):          # and a valid call has no CPU path
        ops.components(z(2, 1, 8, 8), 1, "nchw", thr)
    with pytest.raises(_lib.AcgError, match="ROCm device"):
        ops.components(z(2, 1, 8, 8), 1, "nchw", thr, out=torch.zeros(2, 1, 2, 25, dtype=torch.int64), labels=True)
