"""Host side of the renderers: the fp64 reference (tests/render_ref.py) held to closed forms, the colour tables, the PNG
writer and view_results.py's flags.  No GPU."""
import math
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import render_ref as R  # noqa: E402
from icsg3d_amd import render as P  # noqa: E402

LUT = P.VIRIDIS


@pytest.mark.parametrize("cam", [(0.0, 0.0), (90.0, 0.0)])
def test_uniform_volume_along_an_axis(cam):
    d, W, H, a = 8, 50, 37, 0.2
    vol = np.full((1, d, d, d, 1), 0.5, np.float32)
    img = R.density(vol, LUT, cam, W, H, mode=0, alpha=a, floor=-1.0)[0]
    p = d * math.sqrt(3.0) / min(W, H)
    u = (np.arange(W) + 0.5 - W / 2.0) * p
    v = (H / 2.0 - (np.arange(H) + 0.5)) * p
    inside = (np.abs(u)[None, :] < d / 2.0) & (np.abs(v)[:, None] < d / 2.0)
    assert inside.any() and (~inside).any()
    a32 = float(np.float32(a))
    np.testing.assert_allclose(img[inside, 3], 1.0 - (1.0 - a32) ** d, rtol=0, atol=1e-12)
    assert (img[~inside] == 0.0).all()
    # premultiplied: colour = alpha * lut[128]
    np.testing.assert_allclose(img[inside, :3], img[inside, 3:4] * LUT[128], rtol=0, atol=1e-12)


def test_single_voxel_lands_where_the_camera_formula_says():
    d, W, H = 8, 64, 48
    lab = np.zeros((1, d, d, d), np.int32)
    lab[0, 1, 2, 5] = 3                       # centre (1.5, 2.5, 5.5): x towards the viewer, y right, z up at (0, 0)
    img = R.labels(lab, P.TAB10, (0.0, 0.0), W, H, alpha=0.5)[0]
    p = d * math.sqrt(3.0) / H
    i = (2.5 - 4.0) / p + W / 2.0 - 0.5       # u = y - d/2
    j = H / 2.0 - 0.5 - (5.5 - 4.0) / p       # v = z - d/2
    jj, ii = np.nonzero(img[..., 3])
    assert len(ii) > 0
    assert abs(ii.mean() - i) < 0.5 and abs(jj.mean() - j) < 0.5
    assert i < W / 2 and j < H / 2            # left of and above the centre: neither flipped nor transposed
    assert np.abs(img[jj, ii, :3] - 0.5 * P.TAB10[2]).max() < 1e-12      # label 3 -> palette[2], one voxel deep
    # from above (elev 90, azim 0): up = -x, right = y
    img = R.labels(lab, P.TAB10, (90.0, 0.0), W, H, alpha=0.5)[0]
    jj, ii = np.nonzero(img[..., 3])
    assert abs(ii.mean() - ((2.5 - 4.0) / p + W / 2.0 - 0.5)) < 0.5
    assert abs(jj.mean() - (H / 2.0 - 0.5 - (-(1.5 - 4.0)) / p)) < 0.5
    # the default camera: the projection of the voxel centre onto right / up
    right, up, _ = R.basis(30.0, -60.0)
    img = R.labels(lab, P.TAB10, (30.0, -60.0), W, H, alpha=0.5)[0]
    jj, ii = np.nonzero(img[..., 3])
    rel = np.array([1.5, 2.5, 5.5]) - d / 2.0
    assert abs(ii.mean() - (rel @ right / p + W / 2.0 - 0.5)) < 0.6
    assert abs(jj.mean() - (H / 2.0 - 0.5 - rel @ up / p)) < 0.6


@pytest.mark.parametrize("cam", [(30.0, -60.0), (0.0, 0.0), (-20.0, 135.0)])
def test_sphere_centre_colour_and_silhouette(cam):
    d, W, H, r = 16, 63, 63, 3.0
    img = R.atoms([(np.array([13]), np.array([[8.0, 8.0, 8.0]]))], P.TAB10, d, cam, W, H, radius=r)[0]
    np.testing.assert_allclose(img[31, 31, :3], P.TAB10[3], atol=1e-12)      # the centre pixel looks down the normal
    assert img[31, 31, 3] == 1.0
    p = d * math.sqrt(3.0) / W
    area = float((img[..., 3] > 0).sum()) * p * p
    assert math.pi * (r - p) ** 2 <= area <= math.pi * (r + p) ** 2
    assert set(np.unique(img[..., 3])) == {0.0, 1.0}


def test_lut_index_rule_and_viridis_table():
    v = np.array([0.0, 1.0, -0.1, 1.5, 255.5 / 256.0])
    assert R.lut_index(v).tolist() == [0, 255, 0, 255, 255]
    assert R.lut_index(np.array([0.5, 1.0 / 256.0, 0.99 / 256.0])).tolist() == [128, 1, 0]
    assert P.VIRIDIS.shape == (256, 3) and P.TAB10.shape == (10, 3)
    try:
        from matplotlib import cm
    except Exception:
        return                                 # this one assertion needs matplotlib
    assert (P.VIRIDIS == cm.viridis(np.arange(256))[:, :3]).all()
    assert (cm.viridis(v)[:, :3] == P.VIRIDIS[R.lut_index(v)]).all()
    assert (P.TAB10 == cm.tab10(np.arange(10))[:, :3]).all()


def test_python_camera_mirror_matches_the_reference():
    for cam in [(30.0, -60.0), (0.0, 0.0), (90.0, 0.0), (-20.0, 135.0), (17.0, 450.0)]:
        for a, b in zip(P.basis(P.camera(*cam)), R.basis(*cam)):
            assert (a == b).all()
        o, _ = R.pixel_origins(cam, 8, 50, 37)
        assert (P.pixel_origins(P.camera(*cam), 8, 50, 37) == o).all()
    right, up, eye = R.basis(90.0, 0.0)
    assert eye.tolist() == [0.0, 0.0, 1.0] and right.tolist() == [0.0, 1.0, 0.0] and up.tolist() == [-1.0, 0.0, 0.0]
    right, up, eye = R.basis(30.0, -60.0)
    np.testing.assert_allclose(np.cross(right, up), eye, atol=1e-15)


def test_over_and_sheet():
    rgba = np.zeros((2, 3, 4), np.float32)
    rgba[0, 0] = (0.5, 0.0, 0.0, 0.5)
    rgb = P.over(rgba)
    assert rgb.dtype == np.uint8 and rgb.shape == (2, 3, 3)
    assert rgb[0, 0].tolist() == [255, 128, 128] and rgb[1, 2].tolist() == [255, 255, 255]
    s = P.sheet([rgb] * 8, 2, 4, pad=4)
    assert s.shape == (2 * (2 + 4) + 4, 4 * (3 + 4) + 4, 3)
    assert (s[4:6, 4:7] == rgb).all() and (s[10:12, 25:28] == rgb).all() and (s[:4] == 255).all()


def test_write_png_round_trips(tmp_path):
    rgb = np.random.default_rng(0).integers(0, 256, (13, 29, 3)).astype(np.uint8)
    path = tmp_path / "a.png"
    P.write_png(str(path), rgb)
    raw = path.read_bytes()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(raw):
        n, kind = struct.unpack(">I4s", raw[pos:pos + 8])
        data = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + data) & 0xFFFFFFFF
        chunks.append((kind, data))
        pos += 12 + n
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert struct.unpack(">IIBBBBB", chunks[0][1]) == (29, 13, 8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(13, 1 + 29 * 3)
    assert (rows[:, 0] == 0).all()                                    # filter 0 on every row
    assert (rows[:, 1:].reshape(13, 29, 3) == rgb).all()


def test_view_results_parser_has_the_reference_defaults():
    import view_results
    a = view_results.build_parser().parse_args([])
    assert (a.name, a.batch_size, a.nrot, a.samples, a.split, a.d) == (None, 1, 10, 78750, 0.8, 32)
    assert (a.channels, a.synthetic, a.count, a.size, a.elev, a.azim, a.mode, a.out, a.seed) == (
        4, False, 8, 256, 30.0, -60.0, "value", None, 0)
    assert view_results.TITLES[4] % 0.1234 == "M Pred, MSE = 0.123" and view_results.TITLES[5] % 0.5 == "S pred F1 = 0.500"


def test_entry_points_refuse_bad_arguments_before_any_device_call():
    """The argument rules of the three render ops that are stated in their entry points."""
    import ctypes
    from icsg3d_amd import _lib as L
    lib = L.load()
    d, W, H = 4, 8, 8
    cam, out = np.array([30.0, -60.0]), np.zeros((1, H, W, 4), np.float32)
    lut, pal = np.zeros((256, 3), np.float32), np.ones((3, 3), np.float32)
    lab = np.zeros((1, d, d, d), np.int32)
    f = ctypes.c_float

    def msg_of(rc):
        assert rc != 0
        return (lib.ics_last_error() or b"").decode()

    m = msg_of(lib.ics_op_render_density(None, 1, d, 1, 0, L.fptr(lut), 0, f(0.5), f(0.0), L.f64ptr(cam), W, H, L.fptr(out)))
    assert m.startswith("ics_op_render_density: null vol ("), m

    def labels(labels_=lab, pal_=pal, npal=3, alpha=0.5):
        return msg_of(lib.ics_op_render_labels(L.i32ptr(labels_), 1, d, L.fptr(pal_), npal, f(alpha), L.f64ptr(cam), W, H,
                                               L.fptr(out)))
    for kw, text in ((dict(labels_=None), "null argument (labels, palette)"), (dict(pal_=None), "null argument (labels, palette)"),
                     (dict(npal=0), "npal must be >= 1"), (dict(alpha=1.5), "alpha must be in [0, 1]"),
                     (dict(alpha=-0.1), "alpha must be in [0, 1]")):
        m = labels(**kw)
        assert m.startswith("ics_op_render_labels: " + text + " ("), (kw, m)

    off, sp, xyz = np.array([0, 1, 2], np.int32), np.array([8, 8], np.int32), np.ones((2, 3))
    out2 = np.zeros((2, H, W, 4), np.float32)

    def atoms(off_=off, sp_=sp, xyz_=xyz, pal_=pal, npal=3, radius=1.0):
        return msg_of(lib.ics_op_render_atoms(L.i32ptr(off_), L.i32ptr(sp_), L.f64ptr(xyz_), 2, d, ctypes.c_double(radius),
                                              L.fptr(pal_), npal, L.f64ptr(cam), W, H, L.fptr(out2)))
    bad_xyz = xyz.copy()
    bad_xyz[1, 2] = np.inf
    for kw, text in ((dict(off_=None), "null argument (offsets, palette)"), (dict(pal_=None), "null argument (offsets, palette)"),
                     (dict(npal=0), "npal must be >= 1"), (dict(radius=0.0), "radius must be finite and > 0"),
                     (dict(radius=float("nan")), "radius must be finite and > 0"),
                     (dict(off_=np.array([1, 1, 2], np.int32)), "offsets[0] must be 0"),
                     (dict(off_=np.array([0, 2, 1], np.int32)), "offsets decrease at sample 1"),
                     (dict(sp_=None), "null species or xyz"), (dict(xyz_=None), "null species or xyz"),
                     (dict(xyz_=bad_xyz), "non-finite coordinate")):
        m = atoms(**kw)
        assert m.startswith("ics_op_render_atoms: " + text + " ("), (kw, m)
