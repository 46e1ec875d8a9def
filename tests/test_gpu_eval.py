"""eval.py on the MI355X: ics_op_match_emd held to the reference's own emd (tests/golden/eval_golden.npz) and to scipy
where it imports; the reconstruction chain on the resident batch held bit for bit to encode + decode_to_atoms; the
device feed to the host upload; eval.py end to end in both input modes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_golden.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _split(xyz, off):
    return [xyz[off[k]:off[k + 1]] for k in range(len(off) - 1)]


def _cost(x, y, m):
    """matched distance sum / min(n, m) of a returned matching, recomputed on the host"""
    k = m >= 0
    if min(len(x), len(y)) == 0:
        return np.nan
    return np.sqrt(((x[k] - y[m[k]]) ** 2).sum(-1)).sum() / min(len(x), len(y))


def _check_match(xs, ys, e, ms, ref):
    for b, (x, y, m) in enumerate(zip(xs, ys, ms)):
        assert m.shape == (len(x),) and m.dtype == np.int32
        k = m >= 0
        assert k.sum() == min(len(x), len(y)), b                      # every point of the smaller set matched
        assert len(np.unique(m[k])) == k.sum() and (m[k] < len(y)).all(), b   # injective, in range
        if np.isnan(ref[b]):
            assert np.isnan(e[b]), b
            continue
        tol = 1e-12 * max(abs(ref[b]), 1e-300)
        assert abs(e[b] - ref[b]) <= tol, (b, e[b], ref[b])
        assert abs(_cost(x, y, m) - ref[b]) <= max(tol, 1e-15), (b, _cost(x, y, m), ref[b])


def test_match_emd_equals_the_reference_and_is_deterministic():
    from icsg3d_amd.evaluate import emd
    g = np.load(GOLDEN)
    xs, ys = _split(g["a_xyz"], g["a_off"]), _split(g["b_xyz"], g["b_off"])
    e1, m1 = emd(xs, ys, return_match=True)
    _check_match(xs, ys, e1, m1, g["emd"])
    e2, m2 = emd(xs, ys, return_match=True)
    assert np.array_equal(e1.view(np.uint64), e2.view(np.uint64))
    assert all(np.array_equal(a, b) for a, b in zip(m1, m2))
    assert np.array_equal(emd(xs, ys).view(np.uint64), e1.view(np.uint64))     # without the matching: same values
    # one sample at a time gives what the batch gave (chunk / workgroup-size independence)
    for k in (0, 7, 12, 16):
        assert emd([xs[k]], [ys[k]])[0] == e1[k] or (np.isnan(e1[k]) and np.isnan(emd([xs[k]], [ys[k]])[0]))


def test_match_emd_random_sweep_against_scipy():
    scipy_opt = pytest.importorskip("scipy.optimize")
    from scipy.spatial.distance import cdist
    from icsg3d_amd.evaluate import emd
    rng = np.random.default_rng(11)
    xs, ys = [], []
    for c in range(200):
        n, m = int(rng.integers(0, 70)), int(rng.integers(1, 70))
        if c % 4 == 0:                                   # ties: integer lattice points, duplicates
            xs.append(rng.integers(0, 3, (n, 3)).astype(np.float64))
            ys.append(rng.integers(0, 3, (m, 3)).astype(np.float64))
        else:
            xs.append(rng.normal(0, 3, (n, 3)))
            ys.append(rng.normal(0, 3, (m, 3)))
    xs.append(rng.uniform(0, 20, (256, 3))); ys.append(rng.uniform(0, 20, (700, 3)))
    ref = []
    for x, y in zip(xs, ys):
        if min(len(x), len(y)) == 0:
            ref.append(np.nan)
            continue
        dist = cdist(x, y)
        r, c = scipy_opt.linear_sum_assignment(dist)
        ref.append(dist[r, c].sum() / min(len(x), len(y)))
    e, ms = emd(xs, ys, return_match=True)
    _check_match(xs, ys, e, ms, np.array(ref))


def test_match_emd_refuses_bad_input_and_stays_usable():
    from icsg3d_amd import _lib as L
    lib = L.load()
    a = np.random.default_rng(0).uniform(0, 1, (10, 3))
    b = a[::-1].copy()
    ao = np.array([0, 4, 10], np.int32)
    bo = np.array([0, 6, 10], np.int32)
    emd = np.full(2, -7.0)
    match = np.full(10, -7, np.int32)

    def call(a_, ao_, b_, bo_, n):
        return lib.ics_op_match_emd(L.f64ptr(a_), L.i32ptr(ao_), L.f64ptr(b_), L.i32ptr(bo_), n, L.f64ptr(emd),
                                    L.i32ptr(match))
    big = np.zeros((2049, 3))
    cases = [(big, np.array([0, 2049], np.int32), big, np.array([0, 3], np.int32), 1, "2049"),
             (a, np.array([1, 4, 10], np.int32), b, bo, 2, "_off[0]"),
             (a, np.array([0, 6, 4], np.int32), b, bo, 2, "decreases at sample 1"),
             (a, ao, b, bo, 0, "batch"),
             (np.where(np.arange(30).reshape(10, 3) == 13, np.nan, a), ao, b, bo, 2, "sample 1"),
             (a, ao, np.where(np.arange(30).reshape(10, 3) == 2, np.inf, b), bo, 2, "sample 0")]
    for a_, ao_, b_, bo_, n, msg in cases:
        assert call(a_, ao_, b_, bo_, n) != 0, msg
        err = lib.ics_last_error().decode()
        assert msg in err, (msg, err)
        assert (emd == -7.0).all() and (match == -7).all(), msg       # nothing written
    assert call(a, ao, b, bo, 2) == 0
    assert np.isfinite(emd).all()
    assert (match[:4] >= 0).all() and (match[4:] >= 0).sum() == 4           # sample 1: 6 points against 4


def _engines(d, C, mb, seed):
    from icsg3d_amd.synthetic import random_engines
    return random_engines(d, C, mb, seed)


def _inputs(structs, d, B, rng):
    from icsg3d_amd.matrices import voxelise
    M, _, p = voxelise(structs, d=d, want=("M", "p"))
    x = np.concatenate([M[..., None], p], -1).astype(np.float32)[:B]
    cond = np.eye(10, dtype=np.float32)[rng.integers(0, 10, B)]
    eps = rng.standard_normal((B, 256)).astype(np.float32)
    return x, cond, eps


def _structs(rng, n):
    from icsg3d_amd.matrices import Structures
    sites = []
    for _ in range(n):
        ns = int(rng.integers(2, 9))
        sites.append((rng.uniform(0.05, 0.95, (ns, 3)), rng.integers(1, 90, ns).astype(float),
                      rng.uniform(0.6, 1.6, ns), np.r_[rng.uniform(3, 7, 3), 90.0, 90.0, 90.0]))
    return Structures.from_sites(sites)


def _same(o1, o2):
    for k in ("species", "mask", "density", "coord_minmax", "regions", "n_components", "n_atoms", "stats", "bounds",
              "failed"):
        a, b = o1[k], o2[k]
        assert (a is None) == (b is None), k
        if a is not None:
            assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
    assert len(o1["atoms"]) == len(o2["atoms"])
    for (s1, m1), (s2, m2) in zip(o1["atoms"], o2["atoms"]):
        assert np.array_equal(np.asarray(s1), np.asarray(s2))
        assert np.array_equal(np.asarray(m1, np.float64), np.asarray(m2, np.float64))


def _thresh(ve, un, z, cond):
    """a mask threshold that keeps ~30 % of the voxels of these random weights' reconstructions (segmentation work)"""
    _, sig = un.predict(ve.decode(z, cond))
    return float(np.quantile(sig, 0.7))


@pytest.mark.parametrize("d", [16, 32])
def test_chain_equals_encode_then_decode_to_atoms(d):
    rng = np.random.default_rng(d)
    ve, un = _engines(d, 4, 5, seed=d)                 # max_batch 5 handles running a batch of 3
    x, cond, eps = _inputs(_structs(rng, 3), d, 3, rng)
    _, _, z = ve.encode(x, cond, eps)
    th = _thresh(ve, un, z, cond)
    kw = dict(thresh=th, min_voxels=3, max_atoms=512, want_regions=True)
    ref = ve.decode_to_atoms(un, z, cond, **kw)
    assert ref["n_atoms"].sum() > 0
    ve.upload_batch(x, cond, eps)
    got = ve.reconstruct_to_atoms(un, **kw)
    _same(got, ref)
    _same(ve.reconstruct_to_atoms(un, **kw), ref)      # the resident batch is left unchanged
    _same(ve.reconstruct_to_atoms(un, x, cond, eps, **kw), ref)
    # the refusals: a U-Net of another C, a resident batch above the U-Net's max_batch
    from icsg3d_amd.engine import UnetEngine
    from icsg3d_amd._lib import IcsError
    with pytest.raises(IcsError, match="do not match"):
        ve.reconstruct_to_atoms(UnetEngine(in_channels=1, d=d, max_batch=5))
    with pytest.raises(IcsError, match="max_batch"):
        ve.reconstruct_to_atoms(UnetEngine(in_channels=4, d=d, max_batch=2))


def test_no_resident_batch_is_refused():
    from icsg3d_amd import _lib as L
    ve, un = _engines(16, 4, 2, seed=3)
    counts = np.zeros((2, 2), np.int32)
    stats = np.zeros((2, 8, 11), np.int32)
    lib = L.load()
    assert lib.ics_vae_reconstruct_resident_to_unet_atoms(ve._h, un._h, 0.8, 3, 8, None, None, None, None, None,
                                                          L.i32ptr(counts), L.i32ptr(stats), None) != 0
    assert "no resident batch" in lib.ics_last_error().decode()
    with pytest.raises(RuntimeError):
        ve.reconstruct_to_atoms(un)


def test_feed_equals_host_upload():
    from icsg3d_amd.matrices import make_jobs
    rng = np.random.default_rng(5)
    d, B = 16, 3
    ve, un = _engines(d, 4, 5, seed=7)
    s = _structs(rng, B)
    x, cond, eps = _inputs(s, d, B, rng)
    _, _, z = ve.encode(x, cond, eps)
    kw = dict(thresh=_thresh(ve, un, z, cond), want_regions=True)
    ve.upload_batch(x, cond, eps)
    ref = ve.reconstruct_to_atoms(un, **kw)
    ve.voxelise_batch(s, make_jobs(B), cond, eps)
    _same(ve.reconstruct_to_atoms(un, **kw), ref)


def _reference_emd(x, y):
    """emd() of eval.py:45-53 (cdist + linear_sum_assignment, sum / min(n, m))"""
    from scipy.optimize import linear_sum_assignment
    from scipy.spatial.distance import cdist
    dist = cdist(x, y)
    assign = linear_sum_assignment(dist)
    with np.errstate(invalid="ignore"):
        return dist[assign].sum() / min(len(x), len(y))


def test_eval_end_to_end_both_modes(tmp_path):
    import test_voxelise_host as H
    from icsg3d_amd.evaluate import emd
    from icsg3d_amd.unet.unet import AtomUnet
    from icsg3d_amd.vae.lattice_vae import LatticeDFCVAE
    from icsg3d_amd.matrices import Structures
    d, name = 16, "x"
    root = str(tmp_path)
    rng = np.random.default_rng(21)
    H._write_sites(os.path.join(root, "data"), name, rng, n=14)
    with open(os.path.join(root, "data", name, name + ".csv"), "w") as fh:
        fh.write("task_id,pretty_formula,formation_energy_per_atom,nsites\n")
        for i in range(14):
            fh.write("mp-%d,X%d,%.6f,4\n" % (100 + i, i, rng.normal()))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "create_matrices.py"), "--name", name, "--d", str(d),
                        "--nrot", "0"], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # random weights; the mask threshold moved (sig bias) so that the reconstructions segment into several atoms
    wdir_u = os.path.join(root, "saved_models", "unet", name)
    wdir_v = os.path.join(root, "saved_models", "vae", name)
    os.makedirs(wdir_u); os.makedirs(wdir_v)
    np.random.seed(3)
    unet = AtomUnet(input_shape=(d, d, d, 4), max_batch=4)
    unet.model.save(os.path.join(wdir_u, "unet_weights_x.best.h5"))
    vae = LatticeDFCVAE(input_shape=(d, d, d, 4), perceptual_model=os.path.join(wdir_u, "unet_weights_x.best.h5"),
                        cond_shape=4)
    vae._set_model(batch_size=4)
    s = Structures.from_sites(_read_sites(os.path.join(root, "data", name, "sites"))[:4])
    x, _, _ = _inputs(s, d, 4, rng)
    cond = np.eye(4, dtype=np.float32)[[0, 1, 2, 3]]
    recon = vae.model.predict([x, cond], eps=rng.standard_normal((4, 256)))
    _, sig = unet.model.predict(recon)
    logit = lambda p: np.log(p) - np.log1p(-p)                                  # noqa: E731
    w = unet._get_weights()
    w["sig/bias"] = w["sig/bias"] + np.float32(logit(0.8) - logit(np.clip(np.quantile(sig, 0.7), 1e-6, 1 - 1e-6)))
    unet._set_weights(w)
    unet.model.save_weights(os.path.join(wdir_u, "unet_weights_x.best.hdf5"))
    vae.model.save_weights(os.path.join(wdir_v, "vae_weights_x.best.hdf5"))

    outs = []
    for extra in ([], ["--from_sites"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "eval.py"), "--name", name, "--d", str(d),
                            "--batch_size", "2", "--ncond", "4", "--split", "0.5", "--seed", "9"] + extra,
                           cwd=root, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        assert "MEAN EMD:" in r.stdout and "MEAN DAtoms:" in r.stdout
        odir = os.path.join(root, "output", "eval", name)
        outs.append((dict(np.load(os.path.join(odir, "per_sample.npz"))), json.load(open(os.path.join(odir, "metrics.json")))))
    (p1, m1), (p2, m2) = outs
    assert sorted(p1) == sorted(p2)
    for k in p1:
        assert p1[k].shape == p2[k].shape and np.array_equal(p1[k], p2[k], equal_nan=p1[k].dtype.kind == "f"), k
    assert m1["evaluated"] + m1["failed"] == 6 and m1["evaluated"] >= 1          # 7 validation ids, whole batches of 2
    assert {k: v for k, v in m1.items() if k != "args"} == pytest.approx(
        {k: v for k, v in m2.items() if k != "args"}, nan_ok=True)
    # the written EMDs: the device op on the written atoms and the sites' true positions, and the reference's emd
    pred = _split(p1["atom_xyz"], p1["atom_offsets"])
    assert sum(len(q) for q in pred) > 0
    true = []
    for i in p1["ids"]:
        f = np.load(os.path.join(root, "data", name, "sites", str(i).replace(".npy", ".npz")))
        true.append(Structures.from_sites([(f["frac_coords"], f["Z"], f["radii"], f["lattice"])]).xyz[0])
        np.testing.assert_array_equal(p1["lattice_true"][len(true) - 1], f["lattice"][:3])
    e = emd(pred, true)
    assert np.array_equal(e, p1["emd"], equal_nan=True)
    try:
        import scipy.optimize  # noqa: F401
        ref = np.array([_reference_emd(a, b) for a, b in zip(pred, true)])
        fin = np.isfinite(ref)
        assert np.array_equal(fin, np.isfinite(e))
        np.testing.assert_allclose(e[fin], ref[fin], rtol=1e-12, atol=0)
    except ImportError:
        pass
    assert np.array_equal(p1["n_pred"], np.diff(p1["atom_offsets"]))
    dl = np.abs(p1["lattice_true"] - p1["lattice_pred"])
    with np.errstate(all="ignore"):
        want = {"mean_emd": np.mean(p1["emd"]), "mean_datoms": np.mean(np.abs(p1["n_true"] - p1["n_pred"])),
                "mean_da": np.mean(dl[:, 0]), "mean_db": np.mean(dl[:, 1]), "mean_dc": np.mean(dl[:, 2])}
    assert {k: m1[k] for k in want} == pytest.approx(want, rel=1e-15, nan_ok=True)


def _read_sites(src):
    out = []
    for fname in sorted(os.listdir(src)):
        f = np.load(os.path.join(src, fname))
        out.append((f["frac_coords"], f["Z"], f["radii"], f["lattice"]))
    return out
