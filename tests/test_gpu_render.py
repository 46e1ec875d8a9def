"""The three renderers on the device against tests/render_ref.py (fp64), the resident path against the host-pointer op,
and view_results.py end to end.

Shapes: the smallest at which the kernels can still go wrong -- d = 8 and 32; B = 3; 50 x 37 pictures (non-square, no
multiple of the 8-pixel tile or the 16-pixel workgroup) and one 64 x 64; channel strides 1 and 4; the default camera, two
axis-aligned ones (zero components in the ray direction) and one from below and behind.
Bound: 1e-4 absolute in every channel of every pixel.  It covers about 3 d fp32 compositing steps of relative error
~6e-8 each plus the walk's early exit below a transmittance of 1e-5 (which the reference does not take); path-length
weighting keeps a crossing that the two walks round differently at rounding size.  Largest difference observed on an
MI355X: DESIGN.md section 17."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import render_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
CAMS = [(30.0, -60.0), (0.0, 0.0), (90.0, 0.0), (-20.0, 135.0)]
# (d, camera, (W, H)): every camera at both grids on the odd picture, and one 64 x 64
CASES = [(d, cam, (50, 37)) for d in (8, 32) for cam in CAMS] + [(32, CAMS[0], (64, 64))]
IDS = ["d%d-el%g-az%g-%dx%d" % (d, c[0], c[1], s[0], s[1]) for d, c, s in CASES]


def _volume(d, C, seed):
    """B = 3 sparse volumes with values below 0 and above 1 among them"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-0.2, 1.3, (3, d, d, d, C)) * (rng.uniform(size=(3, d, d, d, C)) < 0.3)
    v = v.astype(np.float32)
    v[0, 0, 0, 0, 0] = 1.0
    v[1, d - 1, d - 1, d - 1, 0] = 0.5
    return v


def _check(name, got, ref):
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print("%s: max |device - fp64 reference| = %.3e, max alpha %.3f" % (name, err, ref[..., 3].max()))
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert ref[..., 3].max() > 0.1, "the case draws nothing"
    assert err <= TOL, "%s: %.3e" % (name, err)


@pytest.mark.parametrize("mode,alpha,floor", [("flat", 0.2, -1.0), ("value", 0.9, 0.0), ("flat", 1.0, 0.1)])
@pytest.mark.parametrize("d,cam,size", CASES, ids=IDS)
def test_density_matches_the_reference(d, cam, size, mode, alpha, floor):
    from icsg3d_amd import render as P
    C = 4 if (d == 8) == (cam[0] > 0) else 1                    # both strides at both grids
    vol = _volume(d, C, seed=d + int(abs(cam[1])))
    got = P.density(vol, channel=0, cam=cam, size=size, mode=mode, alpha=alpha, floor=floor)
    ref = R.density(vol, P.VIRIDIS.astype(np.float32), cam, size[0], size[1], 0, P.MODES[mode], alpha, floor)
    _check("density %s C=%d" % (mode, C), got, ref)


@pytest.mark.parametrize("d,cam,size", CASES, ids=IDS)
def test_labels_match_the_reference(d, cam, size):
    from icsg3d_amd import render as P
    rng = np.random.default_rng(d)
    lab = (rng.integers(1, 41, (3, d, d, d)) * (rng.uniform(size=(3, d, d, d)) < 0.2)).astype(np.int32)   # labels above npal = 10
    lab[2] = 0
    lab[2, d // 2:d // 2 + 2, d // 3:d // 3 + 2, d - 2:] = 27        # a lone block, wider than a pixel at d = 32
    got = P.labels(lab, cam=cam, size=size, alpha=0.5)
    ref = R.labels(lab, P.TAB10.astype(np.float32), cam, size[0], size[1], 0.5)
    _check("labels", got, ref)
    assert ref[2, ..., 3].max() > 0 and got[2, ..., 3].max() > 0


@pytest.mark.parametrize("d,cam,size", CASES, ids=IDS)
def test_atoms_match_the_reference(d, cam, size):
    from icsg3d_amd import render as P
    h = d / 2.0
    sets = [(np.array([1, 12, 30]), np.array([[h, h, h], [h + 1.0, h + 0.5, h - 1.0], [2.0, 3.0, d - 2.0]])),   # two overlap
            (np.zeros(0, np.int64), np.zeros((0, 3))),                                                         # no atoms
            (np.array([7]), np.array([[1.0, 1.0, 1.0]]))]
    radius = 0.12 * d
    got = P.atoms(sets, d, cam=cam, size=size, radius=radius)
    ref = R.atoms(sets, P.TAB10.astype(np.float32), d, cam, size[0], size[1], radius)
    _check("atoms", got, ref)
    assert (got[1] == 0).all()


def test_refused_arguments():
    from icsg3d_amd import render as P
    from icsg3d_amd._lib import IcsError
    vol = np.zeros((1, 8, 8, 8, 1), np.float32)
    with pytest.raises(IcsError):
        P.density(vol, size=(0, 16))
    with pytest.raises(IcsError):
        P.density(vol, size=5000)
    with pytest.raises(IcsError):
        P.density(vol, alpha=1.5)
    with pytest.raises(IcsError):
        P.density(vol, channel=1)
    with pytest.raises(IcsError):
        P.labels(np.zeros((1, 8, 8, 8), np.int32), alpha=-0.1)
    with pytest.raises(IcsError):
        P.atoms([(np.array([1]), np.array([[np.nan, 0.0, 0.0]]))], 8)
    with pytest.raises(IcsError):
        P.atoms([(np.array([1]), np.array([[1.0, 1.0, 1.0]]))], 8, radius=0.0)
    assert P.density(vol, size=16).shape == (1, 16, 16, 4)          # still usable


def test_render_resident_is_the_op_on_the_same_values():
    """After a reconstruct_to_atoms at d = 16, B = 2, random weights: the resident input and the reconstruction rendered
    where they lie are the bits of render.density on the input and on the decoder's output."""
    from icsg3d_amd import render as P
    from icsg3d_amd._lib import IcsError
    from icsg3d_amd.synthetic import random_engines, synthetic_batch
    d, C, B = 16, 4, 2
    ve, un = random_engines(d, C, B, seed=3)
    with pytest.raises(RuntimeError):
        ve.render_resident(0, size=32)
    X, _, cond = synthetic_batch(B, d, C, seed=5, noise=1e-3)
    eps = np.random.default_rng(1).standard_normal((B, ve.latent_dim)).astype(np.float32)
    ve.upload_batch(X, cond, eps)
    with pytest.raises(IcsError):                                   # a resident batch, but no decoder pass over it yet
        ve.render_resident(1, size=32)
    ve.reconstruct_to_atoms(un, X, cond, eps, want_regions=True)
    look = dict(cam=(30.0, -60.0), size=(50, 37), mode="value", alpha=0.6)
    got0, got1 = ve.render_resident(0, **look), ve.render_resident(1, **look)
    flat = ve.render_resident(1, cam=(0.0, 0.0), size=32, mode="flat", alpha=0.2, floor=0.05)
    recon = ve.decode(ve.encode(X, cond, eps)[2], cond)             # vae.model.predict
    assert got0.shape == (B, 37, 50, 4) and got0[..., 3].max() > 0.1 and got1[..., 3].max() > 0
    assert np.array_equal(got0, P.density(X, channel=0, **look))
    assert np.array_equal(got1, P.density(recon, channel=0, **look))
    assert np.array_equal(flat, P.density(recon, channel=0, cam=(0.0, 0.0), size=32, mode="flat", alpha=0.2, floor=0.05))
    ve.close(); un.close()


def test_view_results_synthetic_run(tmp_path):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "view_results.py"), "--name", "x", "--synthetic", "--count", "2",
                        "--d", "16", "--size", "64", "--out", str(tmp_path / "view")], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    out = tmp_path / "view"
    run = json.loads((out / "run.json").read_text())
    assert len(run["rendered"]) == 2
    page = (out / "index.html").read_text()
    for sid in run["rendered"]:
        raw = (out / (sid + ".png")).read_bytes()
        assert raw[:8] == b"\x89PNG\r\n\x1a\n"
        assert struct.unpack(">II", raw[16:24]) == (4 * (64 + 4) + 4, 2 * (64 + 4) + 4)
        row = json.loads((out / (sid + ".json")).read_text())
        assert row["titles"][0] == "M True" and row["titles"][4] == "M Pred, MSE = %.3f" % row["mse"]
        assert row["titles"][5] == "S pred F1 = %.3f" % row["f1"] and len(row["titles"]) == 8
        assert row["n_atoms_true"] >= 1 and not row["failed_true"] and not row["failed_pred"]
        assert sid + ".png" in page and row["titles"][4] in page
    assert "samples: rendered 2" in p.stdout


def test_ops_share_one_thread_scratch_and_stream():
    """Ops of different families interleaved on one thread's scratch: a repeated call gives the same bits and the same
    number of launches after another op used the scratch, after the scratch grew (three 160 x 160 pictures are 1.2 MB,
    above its 1 MB floor), from a thread that exits, and after ics_release_caches."""
    import threading
    from icsg3d_amd import _lib as L, evaluate as E, render as P
    lib = L.load()
    rng = np.random.default_rng(5)
    small = (rng.integers(1, 12, (1, 8, 8, 8)) * (rng.uniform(size=(1, 8, 8, 8)) < 0.4)).astype(np.int32)
    big = (rng.integers(1, 12, (3, 8, 8, 8)) * (rng.uniform(size=(3, 8, 8, 8)) < 0.4)).astype(np.int32)
    outs, launches = [], []

    def first_call():
        n0 = lib.ics_kernel_launches()
        outs.append(P.labels(small, size=32))
        launches.append(lib.ics_kernel_launches() - n0)

    first_call()
    pts = rng.uniform(0.0, 5.0, (2, 3, 3))
    assert np.isfinite(E.emd([pts[0]], [pts[1]])).all()
    assert P.labels(big, size=160)[..., 3].max() > 0
    first_call()
    t = threading.Thread(target=first_call)
    t.start()
    t.join()
    assert lib.ics_release_caches() == 0
    first_call()
    assert len(outs) == 4 and outs[0][..., 3].max() > 0
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])
    assert launches[0] >= 1 and launches == [launches[0]] * 4
