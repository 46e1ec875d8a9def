"""generate.py's structure stage on the MI355X: ics_op_structure_screen held to the fp64 restatement
tests/structure_ref.py (brute force over +-4 lattice translations), its refusals, its repeatability, and generate.py's
CIF / results outputs against screen() on the coordinates the script saved.

Bounds.  Distances, volume, lattice and fractional coordinates: 1e-12 relative -- both sides are fp64 and a value is a
handful of operations on O(10) numbers (the bound ics_op_match_emd is held to); entries of the lattice and fractional
coordinates that are zero or near it are compared against the scale of their array (the longest cell edge, 1), since a
relative error of a rounding residue means nothing.  Pairs, counts, flags and histograms: equal.  Before anything is
compared, the restatement's own values must decide every discrete output with margin (> 1e-6): |dmin - tol| and the
gap between the two smallest pair distances."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import structure_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 0.5
RTOL = 1e-12


def draws(n=300, seed=7, lo=2, hi=40):
    """The issue's set: abc ~ U(3, 12); angles alternately 90/90/90 and integers in [60, 120] (a draw of angles with
    volume < 0.3 abc is discarded and drawn again); lo..hi atoms at U(-0.1, 1.1) abc; species 1..94."""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(n):
        abc = rng.uniform(3, 12, 3)
        ang = np.array([90.0, 90.0, 90.0])
        while k % 2:
            ang = rng.randint(60, 121, 3).astype(np.float64)
            M = R.lattice_from_parameters(*abc, *ang)
            if np.linalg.det(M) >= 0.3 * abc.prod():
                break
        na = rng.randint(lo, hi + 1)
        out.append((rng.randint(1, 95, na).astype(np.int32), rng.uniform(-0.1, 1.1, (na, 3)) * abc, abc, ang))
    return out


def pack(structs):
    off = np.zeros(len(structs) + 1, np.int32)
    off[1:] = np.cumsum([len(s[0]) for s in structs])
    sp = np.concatenate([np.asarray(s[0], np.int32).reshape(-1) for s in structs]) if off[-1] else np.zeros(0, np.int32)
    xyz = np.concatenate([np.asarray(s[1], np.float64).reshape(-1, 3) for s in structs]) if off[-1] else np.zeros((0, 3))
    return off, sp, xyz, np.array([s[2] for s in structs], np.float64), np.array([s[3] for s in structs], np.float64)


def check_against_ref(structs, o, off, images=4, margins=True, shortcut=True):
    n_wrong27 = 0
    for k, (sp, xyz, abc, ang) in enumerate(structs):
        r = R.screen_ref(sp, xyz, abc, ang, TOL, images)
        a0, a1 = off[k], off[k + 1]
        if margins and len(sp) >= 2:
            print("structure %d: n %d dmin %.6f |dmin - tol| %.3e second - dmin %.3e" % (
                k, len(sp), r["min_dist"], abs(r["min_dist"] - TOL), r["second"] - r["min_dist"]))
            assert abs(r["min_dist"] - TOL) > 1e-6, k
            assert r["second"] - r["min_dist"] > 1e-6, k
            assert np.abs(r["pairs"] - TOL).min() > 1e-9, k            # every pair's side of tol is decided too
        np.testing.assert_allclose(o["lattice"][k], r["lattice"], rtol=RTOL, atol=RTOL * float(np.max(abc)), err_msg=str(k))
        np.testing.assert_allclose(o["volume"][k], r["volume"], rtol=RTOL, err_msg=str(k))
        np.testing.assert_allclose(o["frac"][a0:a1], r["frac"], rtol=RTOL, atol=RTOL, err_msg=str(k))
        np.testing.assert_allclose(o["min_dist"][k], r["min_dist"], rtol=RTOL, err_msg=str(k))
        np.testing.assert_allclose(o["nearest"][a0:a1], r["nearest"], rtol=RTOL, err_msg=str(k))
        assert tuple(o["min_pair"][k]) == r["min_pair"], (k, o["min_pair"][k], r["min_pair"])
        assert o["n_close"][k] == r["n_close"] and o["valid"][k] == r["valid"] and o["reason"][k] == r["reason"], k
        assert np.array_equal(o["hist"][k], r["hist"]), k
        if shortcut and len(sp) >= 2:
            d27 = R.pair_distances_27(r["frac"], r["lattice"])[np.triu_indices(len(sp), 1)]
            n_wrong27 += bool((d27 > r["pairs"] + 1e-9).any())       # some pair's nearest image is outside the 27
    return n_wrong27


def test_screen_equals_the_restatement_on_300_random_cells():
    from icsg3d_amd import structures as S
    structs = draws()
    off, sp, xyz, abc, ang = pack(structs)
    o = S.screen_packed(off, sp, xyz, abc, ang, TOL)
    wrong27 = check_against_ref(structs, o, off)
    print("27-image shortcut wrong on", wrong27, "of", len(structs), "cells; invalid:", int((o["valid"] == 0).sum()))
    assert wrong27 >= 1                      # the set exercises the exact search
    assert 0 < o["valid"].sum() < len(structs)
    # two runs: the same bits
    o2 = S.screen_packed(off, sp, xyz, abc, ang, TOL)
    for k in o:
        assert o[k].tobytes() == o2[k].tobytes(), k


def test_screen_large_structures():
    """Above one wave's 64 atoms a whole workgroup owns the structure: 65 and 300 atoms in skewed cells against the +-4
    brute force, 2048 atoms (the limit) in an orthorhombic cell, where +-1 translations are exact, mixed with small ones
    in one call."""
    from icsg3d_amd import structures as S
    rng = np.random.RandomState(11)
    structs = []
    for na, abc, ang in ((65, [9.0, 10.0, 11.0], [75.0, 100.0, 118.0]), (3, [5.0, 5.0, 5.0], [90.0, 90.0, 90.0]),
                         (300, [20.0, 14.0, 17.0], [62.0, 95.0, 110.0]), (64, [9.0, 9.5, 12.0], [90.0, 90.0, 120.0])):
        abc, ang = np.array(abc), np.array(ang)
        structs.append((rng.randint(1, 95, na).astype(np.int32), rng.uniform(-0.1, 1.1, (na, 3)) * abc, abc, ang))
    off, sp, xyz, abc, ang = pack(structs)
    o = S.screen_packed(off, sp, xyz, abc, ang, TOL)
    check_against_ref(structs, o, off)
    abc = np.array([60.0, 70.0, 80.0])
    big = [(rng.randint(1, 95, 2048).astype(np.int32), rng.uniform(-0.1, 1.1, (2048, 3)) * abc, abc, np.array([90.0] * 3))]
    off, sp, xyz, abc, ang = pack(big)
    o = S.screen_packed(off, sp, xyz, abc, ang, TOL)
    check_against_ref(big, o, off, images=1, shortcut=False)
    o2 = S.screen_packed(off, sp, xyz, abc, ang, TOL)
    for k in o:
        assert o[k].tobytes() == o2[k].tobytes(), k


def test_screen_edge_cases():
    from icsg3d_amd import structures as S
    cub, r90 = np.array([4.0, 4.0, 4.0]), np.array([90.0] * 3)
    structs = [(np.zeros(0, np.int32), np.zeros((0, 3)), cub, r90),                      # no atoms
               (np.array([3], np.int32), np.array([[1.0, 1, 1]]), cub, r90),              # one site: valid
               (np.array([8, 8], np.int32), np.array([[1.0, 1, 1], [1.0, 1, 1]]), cub, r90),   # coincident
               (np.array([0, 95, 8, -7], np.int32), np.array([[0.0, 0, 0], [2, 2, 2], [1, 3, 1], [3, 1, 3]]), cub, r90),
               (np.array([26, 26], np.int32), np.array([[0.0, 0, 0], [2, 2, 2]]), cub, r90),   # 2 sqrt 3
               (np.array([8, 8], np.int32), np.array([[0.5, 1, 1], [9.5, 1, 1]]), np.array([10.0] * 3), r90),
               (np.array([8, 8], np.int32), np.array([[0, 0, 0], [0.875 * 2, 0.625 * 12, 0]]), np.array([2.0, 12, 5]),
                np.array([90.0, 90, 120])),
               (np.array([8, 8, 8], np.int32), np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0]]), np.array([8.0] * 3), r90)]
    off, sp, xyz, abc, ang = pack(structs)
    o = S.screen_packed(off, sp, xyz, abc, ang, TOL)
    check_against_ref(structs, o, off, margins=False)
    assert list(o["valid"]) == [0, 1, 0, 0, 1, 1, 1, 1] and list(o["reason"]) == [4, 0, 1, 2, 0, 0, 0, 0]
    assert np.isinf(o["min_dist"][0]) and np.isinf(o["min_dist"][1]) and tuple(o["min_pair"][1]) == (-1, -1)
    assert o["min_dist"][2] == 0.0 and o["n_close"][2] == 1 and np.isinf(o["nearest"][0])
    np.testing.assert_allclose(o["min_dist"][4:7], [2 * np.sqrt(3), 1.0, 2.25 * np.sqrt(3)], rtol=RTOL)
    assert tuple(o["min_pair"][7]) == (0, 1)                                              # the tie rule
    # the Python surface: a list per sample, failed samples passed through, a sample without a cell flagged, not raised
    res = S.screen(np.array([[4.0, 4, 4], [4, 4, 4], [0, 4, 4], [np.nan, 1, 1], [4, 4, 4]]),
                   [([57, 26, 8, 8, 8], [[0, 0, 0], [2, 2, 2], [2, 2, 0], [2, 0, 2], [0, 2, 2]]), None,
                    ([8], [[0, 0, 0]]), ([8], [[0, 0, 0]]), ([], np.zeros((0, 3)))], gamma=120)
    assert res[1] is None and res[0]["valid"] and res[0]["formula"] == "La1 Fe1 O3"
    np.testing.assert_allclose(res[0]["lattice"], R.lattice_from_parameters(4, 4, 4, 90, 90, 120), rtol=RTOL, atol=4e-12)
    assert [r["reason"] for r in (res[2], res[3], res[4])] == [S.REASON_CELL, S.REASON_CELL, S.REASON_EMPTY]
    with pytest.raises(ValueError):
        S.screen(np.array([[4.0, 4, 4]]), [([8], [[0, 0, 0]])], alpha=60, beta=60, gamma=120)


def test_screen_refusals_leave_the_outputs_untouched():
    from icsg3d_amd import _lib as L
    lib = L.load()
    structs = draws(6, seed=2)
    off, sp, xyz, abc, ang = pack(structs)
    B, N = len(structs), len(sp)

    def call(off_=off, sp_=sp, xyz_=xyz, abc_=abc, ang_=ang, b=B, tol=TOL):
        outs = [np.full((B, 9), 7.5), np.full(B, 7.5), np.full((N, 3), 7.5), np.full(B, 7.5), np.full((B, 2), 77, np.int32),
                np.full(B, 77, np.int32), np.full(B, 77, np.int32), np.full(B, 77, np.int32), np.full(N, 7.5),
                np.full((B, 95), 77, np.int32)]
        ptr = [L.f64ptr(a) if a.dtype == np.float64 else L.i32ptr(a) for a in outs]
        rc = lib.ics_op_structure_screen(L.i32ptr(off_), L.i32ptr(sp_), L.f64ptr(xyz_), L.f64ptr(abc_), L.f64ptr(ang_), b,
                                         ctypes.c_double(tol), ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], ptr[5], ptr[6],
                                         ptr[7], ptr[8], ptr[9])
        untouched = all(np.all(a == (7.5 if a.dtype == np.float64 else 77)) for a in outs)
        return rc, untouched

    def mod(a, idx, v):
        b = a.copy()
        b[idx] = v
        return b

    assert call() == (0, False)
    big_off = np.array([0, 2049], np.int32)
    cases = {
        "non-finite xyz": dict(xyz_=mod(xyz, (3, 1), np.nan)), "infinite xyz": dict(xyz_=mod(xyz, (0, 0), np.inf)),
        "huge xyz": dict(xyz_=mod(xyz, (0, 0), 1e200)),
        "non-finite abc": dict(abc_=mod(abc, (1, 1), np.nan)), "non-finite angle": dict(ang_=mod(ang, (1, 1), np.inf)),
        "non-finite tol": dict(tol=float("nan")), "negative tol": dict(tol=-1.0),
        "abc zero": dict(abc_=mod(abc, (2, 0), 0.0)), "abc negative": dict(abc_=mod(abc, (2, 0), -3.0)),
        "angles without a cell": dict(ang_=mod(ang, 1, [60.0, 60.0, 120.0])),
        "angles without a cell 2": dict(ang_=mod(ang, 1, [10.0, 100.0, 150.0])),
        "angle 180": dict(ang_=mod(ang, 1, [90.0, 90.0, 180.0])), "angle 0": dict(ang_=mod(ang, 1, [0.0, 90.0, 90.0])),
        "image range": dict(abc_=mod(abc, 0, [0.1, 100.0, 5.0])),
        "image range skew": dict(ang_=mod(ang, 1, [90.0, 90.0, 179.0])),
        "offsets[0]": dict(off_=mod(off, 0, 1)), "offsets decrease": dict(off_=mod(off, 2, off[1] - 1)),
        "2049 atoms": dict(off_=big_off, sp_=np.ones(2049, np.int32), xyz_=np.zeros((2049, 3)), b=1),
        "batch 0": dict(b=0),
    }
    for name, kw in cases.items():
        rc, untouched = call(**kw)
        assert rc != 0 and untouched, name
        assert lib.ics_last_error(), name
    assert call() == (0, False)                       # still usable


def test_results_writer_rows_cifs_and_numbering(tmp_path):
    """generate.py's tail on constructed samples: valid, duplicate formula, too close, species 0, failed, no atoms."""
    from icsg3d_amd import structures as S
    perov = ([57, 26, 8, 8, 8], np.array([[0.0, 0, 0], [2, 2, 2], [2, 2, 0], [2, 0, 2], [0, 2, 2]]))
    shifted = (perov[0], perov[1] + 0.25)
    close = ([8, 8], np.array([[1.0, 1, 1], [1.2, 1, 1]]))
    atoms = [perov, None, close, shifted, ([0, 8], np.array([[0.0, 0, 0], [2, 2, 2]])), ([], np.zeros((0, 3))),
             ([14, 14], np.array([[0.0, 0, 0], [1, 1, 3]]))]
    lp = np.tile([4.0, 4.0, 4.0], (len(atoms), 1))
    w = S.ResultsWriter(str(tmp_path), 90, 90, 120, training_names={"LaFeO3"}, target_value=-1.5)
    res = w.add_batch(range(10, 10 + len(atoms)), lp, atoms)
    counts = w.finish()
    assert counts == {"generated": 7, "failed": 1, "invalid": 3, "written": 3}
    assert w.invalid_reasons == {12: "atoms closer than tol", 14: "species outside 1..94", 15: "no atoms"}
    rows = S.read_results_csv(str(tmp_path / "results.csv"))
    assert [r["id"] for r in rows] == ["La1 Fe1 O3", "La1 Fe1 O3_1", "Si2"]          # sorted by id
    assert [r["sample"] for r in rows] == [10, 13, 16] and [r["training"] for r in rows] == [1, 1, 0]
    assert [r["anon_formula"] for r in rows] == ["ABC3", "ABC3", "A"] and rows[0]["target"] == -1.5
    assert sorted(os.listdir(tmp_path / "cifs")) == ["La1 Fe1 O3.cif", "La1 Fe1 O3_1.cif", "Si2.cif"]
    for r in rows:
        c, s = S.read_cif(r["cif"]), res[r["sample"] - 10]
        np.testing.assert_allclose(c["abc"], [4, 4, 4], atol=1e-8)
        np.testing.assert_allclose(c["angles"], [90, 90, 120], atol=1e-8)
        np.testing.assert_allclose(c["frac"], s["frac"], atol=1e-8, rtol=0)
        np.testing.assert_allclose(c["volume"], 64 * np.sin(np.radians(120)), atol=1e-7)
        assert np.array_equal(c["species"], s["species"]) and r["natoms"] == len(s["species"])
        assert r["min_distance"] == s["min_dist"] and r["volume"] == s["volume"]
    np.testing.assert_allclose(rows[0]["electronegativity"], (1.10 + 1.83 + 3 * 3.44) / 5, rtol=1e-12)
    assert open(tmp_path / "results.json").read().count("'formula'") == 3


def test_generate_script_writes_cifs_and_results(tmp_path):
    """generate.py --synthetic --gamma 120 on random weights (the mask threshold moved so that samples segment into
    atoms): results.csv, the CIFs and the summary counts agree with screen() called on the saved coords/*.npy."""
    from icsg3d_amd import structures as S
    from icsg3d_amd.synthetic import synthetic_batch
    from icsg3d_amd.unet.unet import AtomUnet
    from icsg3d_amd.vae.lattice_vae import LatticeDFCVAE
    d, name, root, ns = 16, "x", str(tmp_path), 6
    wdir_u, wdir_v = os.path.join(root, "saved_models", "unet", name), os.path.join(root, "saved_models", "vae", name)
    os.makedirs(wdir_u); os.makedirs(wdir_v)
    np.random.seed(3)
    unet = AtomUnet(input_shape=(d, d, d, 4), max_batch=4)
    unet.model.save(os.path.join(wdir_u, "unet_weights_x.best.h5"))
    vae = LatticeDFCVAE(input_shape=(d, d, d, 4), perceptual_model=os.path.join(wdir_u, "unet_weights_x.best.h5"), cond_shape=4)
    vae._set_model(batch_size=4)
    x = synthetic_batch(4, d, 4, seed=0)[0]
    cond = np.tile(np.eye(4, dtype=np.float32)[0], (4, 1))
    recon = vae.model.predict([x, cond], eps=np.random.RandomState(0).standard_normal((4, 256)))
    _, sig = unet.model.predict(recon)
    logit = lambda p: np.log(p) - np.log1p(-p)                                  # noqa: E731
    w = unet._get_weights()
    w["sig/bias"] = w["sig/bias"] + np.float32(logit(0.8) - logit(np.clip(np.quantile(sig, 0.7), 1e-6, 1 - 1e-6)))
    unet._set_weights(w)
    unet.model.save_weights(os.path.join(wdir_u, "unet_weights_x.best.hdf5"))
    vae.model.save_weights(os.path.join(wdir_v, "vae_weights_x.best.hdf5"))

    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate.py"), "--name", name, "--synthetic", "--d", str(d),
                        "--batch_size", "2", "--nsamples", str(ns), "--ncond", "4", "--gamma", "120", "--var", "0.5"],
                       cwd=root, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = os.path.join(root, "output", "results", "synthetic__v=0.5")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("structures:")][-1]
    print(line)
    num = [int(t) for t in line.replace("/", " ").split() if t.isdigit()]
    generated, failed, invalid, written = num
    rows = S.read_results_csv(os.path.join(res, "results.csv"))
    assert generated == ns and generated == failed + invalid + written and written == len(rows)
    assert [r_["id"] for r_ in rows] == sorted(r_["id"] for r_ in rows)
    # screen() on what the script saved: coords/<k>.npy = [species, xyz]; the lattice parameters back from the voxel
    # edges (to_voxel_params: dv = 1.5 l / d)
    ks = sorted(int(f[:-4]) for f in os.listdir(os.path.join(res, "coords")))
    assert len(ks) == generated - failed
    coords = [np.load(os.path.join(res, "coords", "%d.npy" % k)).reshape(-1, 4) for k in ks]
    lp = np.array([np.load(os.path.join(res, "voxel_params", "%d.npy" % k)) * d / 1.5 for k in ks])
    scr = S.screen(lp, [(c[:, 0].astype(np.int64), c[:, 1:]) for c in coords], 90, 90, 120)
    good = [k for k, s in zip(ks, scr) if s["valid"]]
    print("samples", ks, "valid", good, "reasons", [S.reason_text(s["reason"]) for s in scr])
    assert sorted(r_["sample"] for r_ in rows) == good and invalid == len(ks) - len(good)
    seen = []
    by_sample = {r_["sample"]: r_ for r_ in rows}
    for k, s in zip(ks, scr):
        if not s["valid"]:
            continue
        row = by_sample[k]
        assert row["formula"] == s["formula"] and row["id"] == S.numbered(s["formula"], seen)
        seen.append(s["formula"])
        assert row["training"] == 0 and row["target"] is None and row["natoms"] == len(s["species"])
        assert row["anon_formula"] == S.anonymized_formula(s["hist"])
        np.testing.assert_allclose(row["min_distance"], s["min_dist"], rtol=1e-9)
        np.testing.assert_allclose(row["volume"], s["volume"], rtol=1e-9)
        c = S.read_cif(os.path.join(root, row["cif"]))
        np.testing.assert_allclose(c["abc"], s["abc"], atol=2e-8, rtol=0)
        np.testing.assert_allclose(c["angles"], [90, 90, 120], atol=1e-8, rtol=0)
        np.testing.assert_allclose(c["frac"], s["frac"], atol=2e-8, rtol=0)
        assert np.array_equal(c["species"], s["species"])
    assert sorted(os.listdir(os.path.join(res, "cifs"))) == sorted(r_["id"] + ".cif" for r_ in rows)
