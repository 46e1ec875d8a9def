"""The training monitors on the GPU: the slice, KDE and polyline kernels against tests/monitor_ref.py and scipy's recorded
densities, the resident slices of both engines, every refusal, training with the monitor on and off, and monitor_report.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import monitor_ref as MR  # noqa: E402
from make_kde_golden import CASES, codes  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "kde_golden.npz")
PNG = b"\x89PNG\r\n\x1a\n"
KDE_RTOL, KDE_ATOL = 1e-10, 1e-300      # a positive fp64 sum of <= 1025 terms, exp arguments up to ~745: DESIGN section 18
LINES_TOL = 1e-6                        # one rounding to float32 (6e-8) after fp64 work that differs by ~1e-13


def _lut():
    from icsg3d_amd import render as R
    return np.asarray(R.VIRIDIS, np.float32)


def _lattice_volume(dtype, seed=0):
    """B = 3, d = 5, 4 channels: float values on the lattice k / 64 (every fp32 step of the colour rule is exact there:
    the range is at most 8, so t is a multiple of 2^-9 or a quotient of small integers rounded once on both sides in the
    same way), integers as they are."""
    rng = np.random.default_rng(seed)
    k = rng.integers(-200, 300, (3, 5, 5, 5, 4))
    if dtype == np.float32:
        return (k / 64.0).astype(np.float32)
    if dtype == np.uint8:
        return (k % 256).astype(np.uint8)
    return (k * 1000).astype(np.int32)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8, np.int32], ids=["f32", "u8", "i32"])
def test_slice_is_bit_equal_on_the_lattice(dtype):
    from icsg3d_amd import monitor as M
    vol = _lattice_volume(dtype)
    for axis in (0, 1, 2):
        for index in (0, 2, 4):
            for zoom in (1, 3):
                got = M.slices(vol, channel=2, axis=axis, index=index, zoom=zoom)
                ref = MR.slice_rgba(vol, 2, axis, index, zoom, _lut())
                assert got.shape == (3, 5 * zoom, 5 * zoom, 4)
                assert np.array_equal(got, ref), (axis, index, zoom)
    # axes differ: the picture of axis 2 is not the picture of axis 0
    assert not np.array_equal(M.slices(vol, 2, 0, 2), M.slices(vol, 2, 2, 2))


def test_slice_edge_cases():
    from icsg3d_amd import monitor as M
    lut = _lut()
    vol = _lattice_volume(np.float32, seed=1)
    vol[0, :, :, 2, 2] = 0.75                       # a constant slice -> colour 0
    vol[1, 1, 3, 2, 2] = np.nan                     # a NaN voxel: transparent, out of the range
    vol[1, 4, 0, 2, 2] = np.inf
    vol[2, :, :, 2, 2] = np.nan                     # an image without a finite value
    got = M.slices(vol, channel=2, axis=2, index=2, zoom=2)
    assert np.array_equal(got, MR.slice_rgba(vol, 2, 2, 2, 2, lut))
    assert np.array_equal(got[0], np.broadcast_to(np.append(lut[0], 1.0).astype(np.float32), got[0].shape))
    assert (got[1, 2:4, 6:8] == 0).all() and (got[1, 8:10, 0:2] == 0).all() and (got[1, ..., 3].sum() == 4 * 23)
    assert (got[2] == 0).all()
    # a given range with values below and above it
    got = M.slices(vol[:2], channel=1, axis=0, index=4, zoom=1, vrange=(-1.0, 1.5))
    assert np.array_equal(got, MR.slice_rgba(vol[:2], 1, 0, 4, 1, lut, (-1.0, 1.5)))
    plane = vol[:2, 4, :, :, 1]
    assert (plane < -1.0).any() and (plane > 1.5).any()
    assert np.array_equal(got[plane < -1.0][:, :3], np.broadcast_to(lut[0], ((plane < -1.0).sum(), 3)))
    assert np.array_equal(got[plane > 1.5][:, :3], np.broadcast_to(lut[255], ((plane > 1.5).sum(), 3)))


def test_slice_random_values_at_d33():
    """Random float32 values: the index is the reference's except where t * 256 lies within 1e-4 of an integer; those
    pixels are at most 0.5 % (expectation ~0.02 %), which seed 7 keeps for the numpy reference alone."""
    from icsg3d_amd import monitor as M
    lut = _lut()
    vol = np.random.default_rng(7).normal(size=(2, 33, 33, 33, 1)).astype(np.float32)
    got = M.slices(vol, channel=0, axis=1, index=16, zoom=1)
    near = total = wrong = 0
    for b, p in enumerate(MR.slice_plane(vol, 0, 1, 16)):
        idx, fin, t256 = MR.slice_index(p)
        close = np.abs(t256 - np.rint(t256)) < 1e-4
        near += int(close.sum()); total += close.size
        same = (got[b][..., :3] == lut[idx]).all(axis=-1) & (got[b][..., 3] == 1.0)
        wrong += int((~same & ~close).sum())
    print("d=33: %d of %d pixels within 1e-4 of an index boundary, %d others differ" % (near, total, wrong))
    assert near <= 0.005 * total
    assert wrong == 0


@pytest.mark.parametrize("name", list(CASES))
def test_kde_matches_scipy(name):
    from icsg3d_amd import monitor as M
    g = np.load(GOLD)
    z = codes(name)
    assert float(z.astype(np.float64).sum()) == float(g["sum_" + name])
    n, dim = z.shape
    k = M.Kde(dim, n)
    k.append(z)
    grids = [("x50", "dens_" + name)] + ([("x1", "dens_65x5_p1"), ("x65", "dens_65x5_p65")] if name == "65x5" else [])
    for xk, dk in grids:
        dens, bw, status, count = k.evaluate(g[xk])
        with np.errstate(all="ignore"):
            rel = np.nanmax(np.abs(dens - g[dk]) / np.where(g[dk] > 0, g[dk], np.inf))
        print("kde %s %s: worst relative error %.3g" % (name, xk, rel))
        assert count == n and (status == 0).all()
        np.testing.assert_allclose(dens, g[dk], rtol=KDE_RTOL, atol=KDE_ATOL)
        np.testing.assert_allclose(bw, MR.kde(z, g[xk])[1], rtol=1e-14)
    if CASES[name][3] is not None:
        assert (k.evaluate(g["x50"])[0][CASES[name][3]] == 0).all()          # the narrow column: exactly 0
    k.close()


@pytest.mark.parametrize("n,dim", [(2049, 2), (4100, 1)], ids=["2049x2", "4100x1"])
def test_kde_spans_staging_chunks(n, dim):
    """More codes than one LDS staging chunk holds (2048), with a ragged last chunk of 1 and of 4 codes: every pass
    re-stages the column and the densities accumulate per chunk.  Against the float64 restatement, which
    tests/test_monitor_host.py pins to scipy; the same tolerance (the reorder term n 2^-53 is 4.6e-13 at n = 4100).  The
    last codes sit apart from the rest, so a lost tail changes the far grid points by orders of magnitude."""
    from icsg3d_amd import monitor as M
    rng = np.random.default_rng(100 + n)
    z = (rng.standard_normal((n, dim)) * np.array([0.4, 1.1])[:dim] + np.array([-1.0, 0.3])[:dim]).astype(np.float32)
    z[2048:, 0] = 2.75 + 0.01 * np.arange(n - 2048)
    x = np.linspace(-3, 3, 50)
    ref, ref_bw, ref_status = MR.kde(z, x)
    assert (ref_status == 0).all() and (ref > 0).all()
    k = M.Kde(dim, n)
    k.append(z[:1000]); k.append(z[1000:])
    dens, bw, status, count = k.evaluate(x)
    k.close()
    print("kde %dx%d: worst relative error %.3g" % (n, dim, np.max(np.abs(dens - ref) / ref)))
    assert count == n and (status == 0).all()
    np.testing.assert_allclose(dens, ref, rtol=KDE_RTOL, atol=KDE_ATOL)
    np.testing.assert_allclose(bw, ref_bw, rtol=1e-14)
    # the tail matters to what is compared: without the codes past the first chunk the last grid point falls far outside
    assert MR.kde(z[:2048], x)[0][0, -1] < 0.5 * ref[0, -1]


def test_kde_constant_column_and_split_appends():
    from icsg3d_amd import monitor as M
    g = np.load(GOLD)
    z = codes("65x5").copy()
    z[:, 1] = 0.25
    a = M.Kde(5, 65)
    a.append(z)
    dens, bw, status, _ = a.evaluate(g["x50"])
    assert status.tolist() == [0, 1, 0, 0, 0] and np.isnan(dens[1]).all() and bw[1] == 0
    others = [0, 2, 3, 4]
    np.testing.assert_allclose(dens[others], g["dens_65x5"][others], rtol=KDE_RTOL, atol=KDE_ATOL)
    b = M.Kde(5, 70)
    b.append(z[:7])
    b.append(z[7:])
    for x, y in zip(a.evaluate(g["x50"])[:3], b.evaluate(g["x50"])[:3]):
        assert np.array_equal(x, y, equal_nan=True)
    a.close(); b.close()


def _curves(case):
    rng = np.random.default_rng(11)
    if case == "one":
        return np.array([[[0.5, 0.2], [3.6, 0.9]]]), (17, 13), 1.0
    if case == "crossing":
        return np.array([[[0, 0], [4, 1]], [[0, 1], [4, 0]], [[2, -0.2], [2, 1.2]]], np.float64), (17, 13), 0.5
    if case == "gap":
        return np.array([[[0, 0.1], [1, 0.8], [np.nan, 0.5], [3, 0.2], [4, 0.9], [4, np.nan]]]), (17, 13), 1.0
    if case == "point":
        return np.array([[[2.0, 0.5], [2.0, 0.5]]]), (17, 13), 1.0
    if case == "outside":
        return np.array([[[10.0, 5.0], [12.0, 7.0], [11.0, 9.0]]]), (17, 13), 1.0
    xy = np.empty((300, 50, 2))
    xy[..., 0] = np.linspace(0, 4, 50) + rng.normal(0, 0.01, (300, 50))
    xy[..., 1] = rng.uniform(0, 1, (300, 1)) * 0.2 + np.cumsum(rng.normal(0, 0.03, (300, 50)), axis=1)
    xy[::7, 20] = np.nan
    return xy, (64, 48), 0.5


@pytest.mark.parametrize("case", ["one", "crossing", "gap", "point", "outside", "many"])
def test_lines_match_the_reference(case):
    from icsg3d_amd import monitor as M
    xy, (w, h), alpha = _curves(case)
    win = (0.0, 4.0, 0.0, 1.0)
    got = M.line_plot(xy, win, (w, h), width_px=1.5, alpha=alpha)
    ref = MR.lines(xy, win, M.CYCLE, 1.5, alpha, w, h)
    err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
    print("lines %s: max abs error %.3g, covered pixels %d" % (case, err, int((ref[..., 3] > 0).sum())))
    assert got.shape == (h, w, 4) and err <= LINES_TOL
    if case == "outside":
        assert (got == 0).all()
    elif case == "crossing":      # the order matters: the last curve is on top where they cross
        flipped = MR.lines(xy[::-1], win, M.CYCLE[[2, 1, 0]], 1.5, alpha, w, h)
        assert np.abs(flipped - ref).max() > 1e-2
    else:
        assert (ref[..., 3] > 0).any()
    if case == "many":            # tiles that cull and tiles that do not: part of the picture is empty
        assert (ref[..., 3] == 0).any()


def test_resident_slices_are_the_op_on_the_same_values():
    from icsg3d_amd import monitor as M
    from icsg3d_amd._lib import IcsError
    from icsg3d_amd.synthetic import random_engines, synthetic_batch
    d, C_, B = 16, 4, 2
    ve, un = random_engines(d, C_, B, seed=3)
    X, lab, cond = synthetic_batch(B, d, C_, seed=5, noise=1e-3)
    eps = np.random.default_rng(1).standard_normal((B, ve.latent_dim)).astype(np.float32)
    kw = dict(axis=1, index=5, zoom=2)
    # ---- VAE
    with pytest.raises(IcsError):
        M.resident_slices(ve, 0, 1, **kw)                           # no resident batch
    ve.upload_batch(X, cond, eps)
    with pytest.raises(IcsError):
        M.resident_slices(ve, 1, 1, **kw)                           # no decoder pass
    with pytest.raises(IcsError):
        M.Kde(ve.latent_dim, 8).append_vae(ve, 1, "z")              # an upload is no encoder pass
    zm, _, z = ve.encode(X, cond, eps)
    recon = ve.decode(z, cond)
    for ch in (0, 3):
        assert np.array_equal(M.resident_slices(ve, 0, B, channel=ch, **kw), M.slices(X, channel=ch, **kw))
        assert np.array_equal(M.resident_slices(ve, 1, B, channel=ch, **kw), M.slices(recon, channel=ch, **kw))
    assert np.array_equal(M.resident_slices(ve, 1, 1, vrange=(0.0, 0.5), **kw), M.slices(recon[:1], vrange=(0.0, 0.5), **kw))
    for bad in (dict(which=2, count=1), dict(which=0, count=B + 1), dict(which=0, count=1, channel=C_)):
        with pytest.raises(IcsError):
            M.resident_slices(ve, **bad)
    # ---- KDE fed from the engine, device to device
    a, b = M.Kde(ve.latent_dim, 2 * B), M.Kde(ve.latent_dim, 2 * B)
    a.append_vae(ve, B, "z"); a.append_vae(ve, B, "z_mean")
    b.append(z); b.append(zm)
    x = np.linspace(-3, 3, 50)
    for p, q in zip(a.evaluate(x)[:3], b.evaluate(x)[:3]):
        assert np.array_equal(p, q, equal_nan=True)
    with pytest.raises(IcsError):
        a.append_vae(ve, 1, "z")                                    # past the capacity
    with pytest.raises(IcsError):
        M.Kde(7, 4).append_vae(ve, 1, "z")                          # another latent width
    with pytest.raises(IcsError):
        M.Kde(ve.latent_dim, 8).append_vae(un, 1, "z")              # not a VAE engine
    ve.upload_batch(X[::-1].copy(), cond, eps)                      # a new batch: what the passes left was of the old one
    assert np.array_equal(M.resident_slices(ve, 0, B, **kw), M.slices(X[::-1], **kw))
    with pytest.raises(IcsError):
        M.resident_slices(ve, 1, 1, **kw)
    with pytest.raises(IcsError):
        M.Kde(ve.latent_dim, 8).append_vae(ve, 1, "z_mean")
    # ---- U-Net
    with pytest.raises(IcsError):
        M.resident_slices(un, 0, 1, **kw)                           # no resident batch
    soft, sig = un.predict(X)                                       # uploads without labels
    assert np.array_equal(M.resident_slices(un, 2, B, **kw), M.slices(sig, **kw))
    assert np.array_equal(M.resident_slices(un, 0, B, channel=1, **kw), M.slices(X, channel=1, **kw))
    for which in (1, 3):                                            # probabilities only; no labels uploaded
        with pytest.raises(IcsError):
            M.resident_slices(un, which, 1, **kw)
    un.upload_batch(X, lab)
    assert np.array_equal(M.resident_slices(un, 3, B, **kw), M.slices(lab, **kw))
    with pytest.raises(IcsError):
        M.resident_slices(un, 2, 1, **kw)                           # the probabilities were of the batch before
    sp, _ = un.predict_labels(X)
    un.upload_batch(X, lab)
    un.predict_resident(labels_only=True)
    assert np.array_equal(M.resident_slices(un, 1, B, **kw), M.slices(sp, **kw))
    with pytest.raises(IcsError):
        M.resident_slices(un, 2, 1, **kw)                           # labels only
    un.predict_resident(labels_only=False)
    assert np.array_equal(M.resident_slices(un, 2, B, **kw), M.slices(sig, **kw))
    with pytest.raises(IcsError):
        M.resident_slices(un, 1, 1, **kw)
    with pytest.raises(IcsError):
        M.resident_slices(un, 2, 1, channel=1, **kw)
    un.test_step(X, lab)                                            # another forward pass discards the predict
    with pytest.raises(IcsError):
        M.resident_slices(un, 2, 1, **kw)


def test_refusals_write_nothing():
    from icsg3d_amd import _lib as L
    lib = L.load()
    vol = np.zeros((1, 5, 5, 5, 4), np.float32)
    lut = _lut()
    out = np.full((1, 15, 15, 4), -7.0, np.float32)
    rng_nan, rng_rev = np.array([np.nan, 1], np.float32), np.array([1, 0], np.float32)
    vp = vol.ctypes.data_as(C.c_void_p)
    ok = dict(vol=vp, dtype=0, batch=1, d=5, sc=4, ch=2, axis=2, index=2, lut=L.fptr(lut), rng=None, zoom=3, out=L.fptr(out))

    def slice_(**kw):
        a = dict(ok, **kw)
        return lib.ics_op_render_slice(a["vol"], a["dtype"], a["batch"], a["d"], a["sc"], a["ch"], a["axis"], a["index"],
                                       a["lut"], a["rng"], a["zoom"], a["out"])
    bad = [dict(vol=None), dict(lut=None), dict(out=None), dict(d=0), dict(d=257), dict(axis=3), dict(axis=-1),
           dict(index=5), dict(index=-1), dict(ch=4), dict(ch=-1), dict(dtype=3), dict(dtype=-1), dict(zoom=0),
           dict(zoom=65), dict(d=256, zoom=17), dict(rng=L.fptr(rng_nan)), dict(rng=L.fptr(rng_rev)), dict(batch=0)]
    for kw in bad:
        assert slice_(**kw) != 0, kw
        assert lib.ics_last_error()
    assert (out == -7.0).all()
    assert slice_() == 0 and (out != -7.0).all()
    # lines
    xy = np.zeros((2, 3, 2))
    win = np.array([0.0, 1.0, 0.0, 1.0])
    pal = np.ones((1, 3), np.float32)
    img = np.full((4, 6, 4), -7.0, np.float32)
    okl = dict(xy=L.f64ptr(xy), nc=2, np_=3, win=L.f64ptr(win), pal=L.fptr(pal), npal=1, wpx=1.5, alpha=0.5, w=6, h=4,
               out=L.fptr(img))

    def lines_(**kw):
        a = dict(okl, **kw)
        return lib.ics_op_render_lines(a["xy"], a["nc"], a["np_"], a["win"], a["pal"], a["npal"], a["wpx"], a["alpha"],
                                       a["w"], a["h"], a["out"])
    flat, nanw = np.array([0.0, 0.0, 0.0, 1.0]), np.array([0.0, 1.0, np.nan, 1.0])
    for kw in [dict(xy=None), dict(win=None), dict(pal=None), dict(out=None), dict(np_=1), dict(np_=4097), dict(nc=0),
               dict(nc=65536), dict(win=L.f64ptr(flat)), dict(win=L.f64ptr(nanw)), dict(wpx=0.0), dict(wpx=-1.0),
               dict(alpha=-0.1), dict(alpha=1.1), dict(npal=0)]:
        assert lines_(**kw) != 0, kw
    assert (img == -7.0).all()
    assert lines_() == 0 and (img != -7.0).all()
    # KDE
    h = C.c_void_p()
    for dim, cap in ((0, 8), (4097, 8), (3, 1), (3, (1 << 20) + 1)):
        assert lib.ics_op_kde_create(dim, cap, C.byref(h)) != 0 and not h
    assert lib.ics_op_kde_create(3, 4, C.byref(h)) == 0
    z = np.arange(15, dtype=np.float32).reshape(5, 3)
    x = np.linspace(-1, 1, 4)
    dens = np.full((3, 4), -7.0)
    bw, st = np.full(3, -7.0), np.full(3, -7, np.int32)
    assert lib.ics_op_kde_append(h, L.fptr(z), 1) == 0
    assert lib.ics_op_kde_evaluate(h, L.f64ptr(x), 4, L.f64ptr(dens), L.f64ptr(bw), L.i32ptr(st), None) != 0   # one code
    assert lib.ics_op_kde_append(h, L.fptr(z), 4) != 0                                                         # past capacity
    zbad = z.copy(); zbad[1, 1] = np.inf
    assert lib.ics_op_kde_append(h, L.fptr(zbad), 2) != 0
    assert lib.ics_op_kde_append(h, L.fptr(z[1:]), 2) == 0
    for npts in (0, 4097):
        assert lib.ics_op_kde_evaluate(h, L.f64ptr(x), npts, L.f64ptr(dens), L.f64ptr(bw), L.i32ptr(st), None) != 0
    assert lib.ics_op_kde_evaluate(h, None, 4, L.f64ptr(dens), None, None, None) != 0
    assert lib.ics_op_kde_evaluate(h, L.f64ptr(x), 4, None, None, None, None) != 0
    assert (dens == -7.0).all() and (bw == -7.0).all() and (st == -7).all()
    n = C.c_int(0)
    assert lib.ics_op_kde_evaluate(h, L.f64ptr(x), 4, L.f64ptr(dens), L.f64ptr(bw), L.i32ptr(st), C.byref(n)) == 0
    assert n.value == 3 and np.isfinite(dens).all() and (st == 0).all()
    assert lib.ics_op_kde_destroy(h) == 0


def _write_dataset(root, name, n, d, seed=0):
    """The on-disk layout of create_matrices.py, as tests/test_gpu_dataset.py writes it: n compounds, no rotations."""
    from icsg3d_amd.synthetic import synthetic_batch
    mats = os.path.join(root, "data", name, "matrices")
    for sub in ("density_matrices", "species_matrices", "coordinate_grids"):
        os.makedirs(os.path.join(mats, sub))
    files = ["mp-%d.npy" % (k + 1) for k in range(n)]
    for k, f in enumerate(files):
        X, lab, _ = synthetic_batch(1, d, 4, seed=seed + k, noise=1e-3)
        np.save(os.path.join(mats, "density_matrices", f), X[0, ..., 0].astype(np.float64).ravel())
        np.save(os.path.join(mats, "coordinate_grids", f), X[0, ..., 1:4].astype(np.float64))
        np.save(os.path.join(mats, "species_matrices", f), lab[0].astype(np.int64))
    rng = np.random.default_rng(seed)
    with open(os.path.join(root, "data", name, name + ".csv"), "w") as fh:
        fh.write("task_id,pretty_formula,formation_energy_per_atom,nsites\n")
        for f in files:
            fh.write("%s,X%s,%.6f,%d\n" % (f[:-4], f[:-4].replace("-", ""), rng.normal(), rng.integers(2, 9)))
    return files


def _png_size(path):
    b = open(path, "rb").read()
    assert b[:8] == PNG, path
    return int.from_bytes(b[16:20], "big"), int.from_bytes(b[20:24], "big")


def test_training_is_undisturbed_by_the_monitor(tmp_path, capsys):
    """2 epochs of both train loops on a 4-sample d = 16 dataset with the monitor on and off: bit-identical metrics and
    saved weights, and the monitor run leaves its pictures."""
    from icsg3d_amd.hdf5_min import Hdf5File  # noqa: F401  (the checkpoint readers below go through it)
    from icsg3d_amd.checkpoint import load_weights
    from icsg3d_amd.unet.data import UnetDataGenerator
    from icsg3d_amd.unet.unet import AtomUnet
    from icsg3d_amd.vae.data import VAEDataGenerator
    from icsg3d_amd.vae.lattice_vae import LatticeDFCVAE
    d, bs = 16, 2
    files = _write_dataset(str(tmp_path), "m", 4, d)
    path = os.path.join(str(tmp_path), "data", "m", "matrices")
    csv = os.path.join(str(tmp_path), "data", "m", "m.csv")
    results = {}
    for mon in (False, True):
        out = tmp_path / ("on" if mon else "off")
        os.makedirs(out)
        np.random.seed(123)
        tg = UnetDataGenerator(files, data_path=path, batch_size=bs, dim=(d, d, d), n_channels=1, shuffle=True)
        vg = UnetDataGenerator(files[:2], data_path=path, batch_size=bs, dim=(d, d, d), n_channels=1, shuffle=True)
        unet = AtomUnet(input_shape=(d, d, d, 1), weights=str(out / "unet.best.hdf5"), lr=1e-4, max_batch=bs)
        hist = []
        orig = unet.model.fit_generator
        unet.model.fit_generator = lambda **kw: hist.extend(orig(**kw))
        unet.train_generator(tg, vg, epochs=2, output_dir=str(out / "unet"), monitor=mon)
        uw = load_weights(str(out / "unet.best.h5"), "unet")
        kw = dict(data_path=path, property_csv=csv, batch_size=bs, dim=(d, d, d), n_channels=1, shuffle=True, n_bins=2)
        tv, vv = VAEDataGenerator(files, **kw), VAEDataGenerator(files[:2], **kw)
        vae = LatticeDFCVAE(input_shape=(d, d, d, 1), perceptual_model=unet, cond_shape=2, output_dir=str(out / "vae"))
        vae.train(tv, vv, epochs=2, weights=str(out / "vae.best.hdf5"), monitor=mon)
        vw = load_weights(str(out / "vae.best.h5"), "vae")
        results[mon] = (hist, uw, np.array(vae.losses), vw)
    (h0, u0, l0, v0), (h1, u1, l1, v1) = results[False], results[True]
    assert h0 == h1 and len(h0) == 2, (h0, h1)
    assert np.array_equal(l0, l1) and np.isfinite(l0).all()
    for a, b in ((u0, u1), (v0, v1)):
        assert sorted(a) == sorted(b)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    off = [f for _, _, fs in os.walk(tmp_path / "off") for f in fs if f.endswith(".png") and f != "unet_loss.png"]
    assert off == []
    side, pad = d * 4, 4
    on = tmp_path / "on"
    assert _png_size(on / "unet" / "segmentations_best.png") == (2 * (side + pad) + pad, 1 * (side + pad) + pad)
    assert _png_size(on / "unet" / "segmentations_binary_best.png") == (2 * (side + pad) + pad, 1 * (side + pad) + pad)
    assert _png_size(on / "unet" / "unet_loss.png") == (640, 480)
    assert _png_size(on / "vae" / "vae_reconstructions.png") == (2 * (side + pad) + pad, (bs // 2) * (side + pad) + pad)
    assert _png_size(on / "vae" / "vae_samples.png") == (2 * (side + pad) + pad, (bs // 2) * (side + pad) + pad)
    assert _png_size(on / "vae" / "vae_kde.png") == (640, 480)
    assert _png_size(on / "vae" / "vae_losses.png") == (640, 480)
    k = json.load(open(on / "vae" / "vae_kde.json"))
    assert k["count"] == 1000 and len(k["bandwidth"]) == 256 and len(k["x"]) == 50
    assert os.path.exists(on / "vae" / "vae_kde.svg")
    for stem in ("segmentations_best", "segmentations_binary_best", "unet_loss"):
        assert os.path.exists(on / "unet" / (stem + ".json"))


def test_monitor_report_synthetic_runs_in_a_child_process(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "monitor_report.py"), "--name", "syn", "--which", "both",
                        "--synthetic", "--d", "16", "--channels", "1", "--batch_size", "4", "--out", str(tmp_path / "rep")],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    for f in ("segmentations_best.png", "segmentations_binary_best.png", "vae_reconstructions.png", "vae_samples.png",
              "vae_kde.png", "vae_kde.svg", "vae_kde.json", "run.json"):
        assert os.path.exists(tmp_path / "rep" / f), f
    assert _png_size(tmp_path / "rep" / "vae_kde.png") == (640, 480)
