"""ics_op_structure_fingerprint and ics_op_fingerprint_nearest on the device against the brute-force restatement
(tests/structure_fingerprint_ref.py).

Bounds.  count and rdf: |delta| <= 1e-10 max(1, the largest bin of that structure) -- the bar the fp64 KDE kernel is held
to; two fp64 evaluations of this Lipschitz-continuous definition differ by rounding (~1e-14), a missed or doubled image
moves a raw count by O(1).  nn_dist: 1e-12 relative.  n_pairs, cn, reason: EQUAL -- a condition on the inputs, which the
case builders assert on the CPU (no pair within 1e-9 relative of R or of (1 + cn_tol) nn_dist).  Nearest op: distances
1e-12 relative, div_sum 1e-10 relative, indices equal (the builders assert that the best and second-best partner of every
row differ by more than 1e-9 relative unless they are bit-equal rows).  Every comparison prints its worst gap."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import structure_fingerprint_cases as C
import structure_fingerprint_ref as FR
from icsg3d_amd import _lib as L
from icsg3d_amd import structures as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("rdf", "count", "n_pairs", "nn_dist", "cn", "reason")
NEAR_KEYS = ("q_ref", "q_ref_d", "ref_q", "ref_q_d", "q_q", "q_q_d")


def run(structs, eligible=None, r_max=6.0, n_bins=60, w=0.1, cn_tol=0.1):
    off, sp, fr, lat = C.pack(structs)
    el = np.ones(len(structs), np.int32) if eligible is None else np.asarray(eligible, np.int32)
    return S.fingerprint_packed(off, sp, fr, lat, el, r_max, n_bins, w, cn_tol)


def compare(o, r, what=""):
    """Device `o` against restatement `r`: integers equal, floats within the bounds above; returns the worst gaps."""
    C.assert_robust(r)
    for k in ("n_pairs", "cn", "reason"):
        assert np.array_equal(np.asarray(o[k]), np.asarray(r[k])), (what, k, np.asarray(o[k]).tolist()[:40], np.asarray(r[k]).tolist()[:40])
    ok = r["reason"] == 0
    gap = {"count": 0.0, "rdf": 0.0, "nn_dist": 0.0}
    for k in ("count", "rdf"):
        assert np.array_equal(np.isnan(o[k]), np.isnan(r[k])), (what, k)
        for s in np.where(ok)[0]:
            gap[k] = max(gap[k], float(np.abs(o[k][s] - r[k][s]).max() / max(1.0, np.abs(r[k][s]).max())))
    assert np.array_equal(np.isnan(o["nn_dist"]), np.isnan(r["nn_dist"])), what
    fin = np.isfinite(r["nn_dist"])
    if fin.any():
        gap["nn_dist"] = float(np.abs(o["nn_dist"][fin] / r["nn_dist"][fin] - 1.0).max())
    print(what, "worst gaps:", " ".join("%s %.2e" % kv for kv in gap.items()))
    assert gap["count"] <= 1e-10 and gap["rdf"] <= 1e-10 and gap["nn_dist"] <= 1e-12, (what, gap)
    return gap


@pytest.fixture(scope="module")
def sized():
    """n = 1 (self-images only), 2, 63 / 64 / 65 (the wave / workgroup hand-over) and 256, with the restatement's answer."""
    rng = np.random.default_rng(41)
    structs = [C.sized(rng, n) for n in (1, 2, 63, 64, 65, 256)]
    return structs, FR.fingerprint_ref(structs, None, **C.PARAMS)


@pytest.fixture(scope="module")
def cells():
    structs = list(C.cell_cases().values()) + [C.too_dense()]
    return structs, FR.fingerprint_ref(structs, None, **C.PARAMS)


def test_atom_counts_on_both_sides_of_the_wave_workgroup_boundary(sized):
    structs, r = sized
    assert [len(s[0]) for s in structs] == [1, 2, 63, 64, 65, 256]
    o = run(structs)
    compare(o, r, "sizes")
    assert o["cn"][0] >= 1 and o["n_pairs"][0] > 0            # one atom: its own images are its neighbours


def test_cells_cubic_hexagonal_triclinic_thin_and_one_out_of_range(cells):
    structs, r = cells
    assert r["reason"].tolist() == [0, 0, 0, 0, 0, 2]
    assert FR.image_range(structs[0][2], 6.1).tolist() == [3, 3, 3] and FR.image_range(structs[3][2], 6.1).tolist() == [3, 3, 1]
    o = run(structs)
    compare(o, r, "cells")
    assert o["cn"][0] == 6 and o["nn_dist"][0] == 3.0 and o["n_pairs"][0] == 32
    assert o["count"][0][59] == 3.0                            # the shell of 6 at 2a = r_max: exactly half of each
    assert abs(o["count"][0].sum() - 29.0) <= 1e-12
    assert o["n_pairs"][5] == -1 and np.all(np.isnan(o["rdf"][5])) and o["cn"][-1] == -1      # bit 2: no refusal


@pytest.mark.parametrize("n_bins,w", [(1, 0.1), (60, 0.03), (60, 0.25), (61, 0.1), (256, 0.1)])
def test_bin_counts_and_widths_below_and_above_a_bin(n_bins, w):
    """1, 60, 61 and 256 bins (one to four bins per lane); w = 0.03 < a bin of 0.1 < w = 0.25; 256 bins are 0.023 wide."""
    rng = np.random.default_rng(43)
    structs = [C.triclinic5(), C.cell_cases()["hex"], C.thin_long(), C.sized(rng, 65), C.cubic()]
    r = FR.fingerprint_ref(structs, None, 6.0, n_bins, w, 0.1)
    compare(run(structs, None, 6.0, n_bins, w, 0.1), r, "bins %d w %g" % (n_bins, w))


def test_other_parameters_and_the_neighbour_reach():
    """r_max below the shortest lattice vector: the neighbour sweep, not R, sets the image range; cn_tol 0.35."""
    structs = [C.cell_cases()["perovskite"], C.triclinic5(), C.thin_long()]
    r = FR.fingerprint_ref(structs, None, 2.0, 20, 0.05, 0.35)
    o = run(structs, None, 2.0, 20, 0.05, 0.35)
    compare(o, r, "r_max 2")
    assert o["cn"][:5].tolist() == r["cn"][:5].tolist() and o["nn_dist"][0] > 2.05     # La-O at 2.76: beyond R


def _raw(structs, eligible, n_bins=8, sentinel=-7.0):
    off, sp, fr, lat = C.pack(structs)
    ns, N = len(structs), len(sp)
    lat = np.ascontiguousarray(lat.reshape(ns, 9))
    el = np.asarray(eligible, np.int32)
    b = {"rdf": np.full((ns, 2, n_bins), sentinel), "count": np.full((ns, n_bins), sentinel), "n_pairs": np.full(ns, -7, np.int64),
         "nn_dist": np.full(N, sentinel), "cn": np.full(N, -7, np.int32), "reason": np.full(ns, -7, np.int32)}
    rc = L.load().ics_op_structure_fingerprint(
        L.i32ptr(off), L.i32ptr(sp), L.f64ptr(fr), L.f64ptr(lat), L.i32ptr(el), ns, 6.0, n_bins, 0.1, 0.1, L.f64ptr(b["rdf"]),
        L.f64ptr(b["count"]), L.i64ptr(b["n_pairs"]), L.f64ptr(b["nn_dist"]), L.i32ptr(b["cn"]), L.i32ptr(b["reason"]))
    return rc, b


def test_257_atoms_refused_by_name_or_neutral_when_ineligible():
    rng = np.random.default_rng(44)
    big = (np.full(257, 8, np.int32), rng.uniform(size=(257, 3)), C.lat([19.0, 20.0, 21.0]))
    structs = [C.cubic(), big]
    rc, b = _raw(structs, [1, 1])
    msg = L.load().ics_last_error().decode()
    assert rc != 0 and "eligible structure 1" in msg and "257" in msg, msg
    for k, v in b.items():
        assert np.all(v == -7), k                                   # nothing written
    rc, b = _raw(structs, [1, 0])
    assert rc == 0 and b["reason"].tolist() == [0, 1] and b["n_pairs"].tolist() == [32, -1]
    assert np.all(np.isnan(b["rdf"][1])) and np.all(np.isnan(b["nn_dist"][1:])) and np.all(b["cn"][1:] == -1) and b["cn"][0] == 6
    for bad in (dict(r_max=0.0), dict(r_max=float("nan")), dict(n_bins=0), dict(n_bins=257), dict(w=0.0), dict(cn_tol=-0.1)):
        with pytest.raises(Exception):
            run([C.cubic()], **bad)


def chunk_worker(path):
    """Run in a fresh process with ICSG3D_FINGERPRINT_CHUNK_BYTES / _PAIRS set (they are read once per process)."""
    structs, el = C.ragged()
    o = run(structs, el)
    fp, valid = C.nearest_table(52, 300, 700, 121, invalid=(7, 150, 300, 999), duplicates=((40, 12), (650, 12), (320, 12)))
    n = S.fingerprint_nearest(fp, valid, 300, 700)
    np.savez(path, **o, **{k: n[k] for k in NEAR_KEYS}, div_sum=n["div_sum"], div_pairs=n["div_pairs"])
    print("chunked run written")


@pytest.fixture(scope="module")
def ragged():
    structs, el = C.ragged()
    return structs, el, FR.fingerprint_ref(structs, el, **C.PARAMS)


@pytest.fixture(scope="module")
def chunked(tmp_path_factory):
    """Both ops in a fresh child at a chunk of 20 000 bytes (a structure of the batch takes 1.6 to 5 kB: more than twenty
    chunks of two kernel kinds) and 100 000 pairs (a segment of 512 partners x 300 rows is more: one segment per launch)."""
    path = str(tmp_path_factory.mktemp("fp") / "chunked.npz")
    env = dict(os.environ, ICSG3D_FINGERPRINT_CHUNK_BYTES="20000", ICSG3D_FINGERPRINT_CHUNK_PAIRS="100000",
               PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", "import test_gpu_structure_fingerprint as T; T.chunk_worker(%r)" % path], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "chunked run written" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
    return np.load(path)


def test_ragged_batch_against_the_restatement_chunked_and_twice_the_same_bits(ragged, chunked):
    structs, el, r = ragged
    assert len(structs) == 300 and 40 <= (el == 0).sum() <= 45 and max(len(s[0]) for s in structs) == 257
    assert set(r["reason"].tolist()) == {0, 1, 2} and sum(len(s[0]) > 64 for s, e in zip(structs, el) if e) >= 5
    a, b = run(structs, el), run(structs, el)
    compare(a, r, "ragged")
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
        assert a[k].tobytes() == chunked[k].tobytes(), k


# ---------------------------------------------------------------- the nearest op
def compare_nearest(o, r, what=""):
    C.assert_separated(r)
    for k in ("q_ref", "ref_q", "q_q"):
        assert np.array_equal(o[k], r[k]), (what, k, o[k].tolist()[:40], r[k].tolist()[:40])
    gap = 0.0
    for k in ("q_ref_d", "ref_q_d", "q_q_d"):
        assert np.array_equal(np.isinf(o[k]), np.isinf(r[k])), (what, k)
        fin = np.isfinite(r[k])
        assert np.array_equal(o[k][fin] == 0.0, r[k][fin] == 0.0), (what, k, "an exact copy must give exactly 0")
        nz = fin & (r[k] > 0)
        if nz.any():
            gap = max(gap, float(np.abs(o[k][nz] / r[k][nz] - 1.0).max()))
    assert o["div_pairs"] == r["div_pairs"], what
    dgap = abs(o["div_sum"] - r["div_sum"]) / r["div_sum"] if r["div_sum"] else abs(o["div_sum"])
    print(what, "worst gaps: distances %.2e div_sum %.2e" % (gap, dgap))
    assert gap <= 1e-12 and dgap <= 1e-10, (what, gap, dgap)


@pytest.mark.parametrize("nq,nref,length", [(1, 0, 1), (2, 0, 120), (1, 1, 121), (65, 130, 1), (65, 130, 120), (65, 130, 121)])
def test_nearest_small_shapes(nq, nref, length):
    n = nq + nref
    inv = (3, 70, 100) if n > 100 else ()
    dup = ((20, 5), (90, 5), (150, 5), (64, 180)) if n > 100 else ()
    fp, valid = C.nearest_table(50 + length, nq, nref, length, invalid=inv, duplicates=dup)
    o = S.fingerprint_nearest(fp, valid, nq, nref)
    compare_nearest(o, FR.nearest_ref(fp, valid, nq, nref), "nearest %d x %d x %d" % (nq, nref, length))
    if dup:
        assert o["q_q"][5] == 20 and o["q_q_d"][5] == 0.0 and o["q_q"][20] == 5           # the lower index of the copies
        assert o["q_ref"][5] == 90 - nq and o["q_ref_d"][20] == 0.0 and o["ref_q"][150 - nq] == 5 and o["ref_q"][180 - nq] == 64
        assert o["q_ref"][3] == -1 and np.isinf(o["q_q_d"][3]) and o["ref_q"][70 - nq] == -1 and 3 not in o["q_q"].tolist()
    if (nq, nref) == (2, 0):
        assert o["q_q"].tolist() == [1, 0] and o["q_q_d"][0] == o["q_q_d"][1] == o["div_sum"] and o["div_pairs"] == 1
    if nq == 1:
        assert o["q_q"].tolist() == [-1] and o["div_pairs"] == 0 and o["div_sum"] == 0.0


def test_nearest_300_by_700_chunked_and_twice_the_same_bits(chunked):
    """More than one block of rows and more than one segment of partners; invalid rows of both kinds; copies."""
    fp, valid = C.nearest_table(52, 300, 700, 121, invalid=(7, 150, 300, 999), duplicates=((40, 12), (650, 12), (320, 12)))
    a, b = S.fingerprint_nearest(fp, valid, 300, 700), S.fingerprint_nearest(fp, valid, 300, 700)
    compare_nearest(a, FR.nearest_ref(fp, valid, 300, 700), "nearest 300 x 700 x 121")
    assert a["q_ref"][12] == 20 and a["q_q"][12] == 40 and a["ref_q"][350] == 12 and a["q_ref"][7] == -1 and a["ref_q"][0] == -1
    for k in NEAR_KEYS:
        assert a[k].tobytes() == b[k].tobytes() and a[k].tobytes() == chunked[k].tobytes(), k
    assert a["div_sum"] == b["div_sum"] == float(chunked["div_sum"]) and a["div_pairs"] == int(chunked["div_pairs"])
    bad = fp.copy()
    bad[5, 3] = np.inf
    with pytest.raises(L.IcsError, match="valid row 5"):
        S.fingerprint_nearest(bad, valid, 300, 700)
    bad[5, 3], bad[7, 0] = 0.0, np.inf                              # an invalid row is not read
    S.fingerprint_nearest(bad, valid, 300, 700)


# ---------------------------------------------------------------- end to end
def _ortho_samples(rng, n):
    out = []
    for k in range(n):
        abc = rng.uniform(3.5, 6.5, size=3)
        Z, f, M = C.random_p1(rng, int(rng.integers(2, 9)), C.lat(abc), dmin=0.9)
        out.append((rng.choice([8, 14, 22, 38], size=len(Z)).astype(np.int32), f, abc))
    return out


def test_results_writer_against_a_sites_folder(tmp_path):
    """ResultsWriter(fingerprinter=...) from atom lists with a three-file sites folder: a reference that is a sample under
    one of the 24 rotations is that sample's nearest training structure at distance <= 1e-10; the summary's quantiles are
    those of the arrays; a delta at the median gives a precision within one sample of 0.5."""
    rng = np.random.default_rng(45)
    samples = _ortho_samples(rng, 9)
    P = S.signed_permutations(1)[17]
    Z, f, abc = samples[4]
    f2 = f @ P.T
    others = _ortho_samples(rng, 2)
    sites = tmp_path / "data" / "toy" / "sites"
    os.makedirs(sites)
    for name, (z, fr, l) in (("mp-1", others[0]), ("mp-2", (Z, f2 - np.floor(f2), np.abs(P) @ abc)), ("mp-3", others[1])):
        np.savez(sites / (name + ".npz"), frac_coords=fr, Z=z.astype(float), radii=np.ones(len(z)), lattice=np.r_[l, 90.0, 90.0, 90.0])
    ref = S.ReferenceSet.from_sites(str(sites))
    assert ref.ids == ["mp-1", "mp-2", "mp-3"]
    atoms = [(z, fr * l) for z, fr, l in samples]
    lp = np.array([l for _, _, l in samples])

    def finish(out, deltas):
        w = S.ResultsWriter(str(tmp_path / out), fingerprinter=S.Fingerprinter(ref, deltas=deltas))
        w.add_batch(range(len(atoms)), lp, atoms)
        return w, w.finish()
    w, counts = finish("a", ())
    assert counts["written"] == 9 and counts["fingerprinted"] == 9, counts
    rows = {r["sample"]: r for r in w.rows}
    print("nearest_training_dist of the rotated copy: %.3e" % rows[4]["nearest_training_dist"])
    assert rows[4]["nearest_training"] == "mp-2" and rows[4]["nearest_training_dist"] <= 1e-10
    head = open(tmp_path / "a" / "results.csv").readline().strip().split(",")
    assert tuple(head[1:]) == S.ResultsWriter.COLUMNS + S.ResultsWriter.FINGERPRINT_COLUMNS
    near, sm = w.fingerprint_results["nearest"], w.fingerprint_summary
    assert sm["coverage"] == [] and sm["samples"] == 9 and sm["references"] == 3
    z = np.load(tmp_path / "a" / "fingerprints.npz")
    D = np.sqrt(((z["fp"][:, None, :] - z["fp"][None, :, :]) ** 2).mean(-1))
    np.fill_diagonal(D, np.inf)
    np.testing.assert_allclose(sm["nearest_generated_dist"], np.quantile(D.min(1), S.FP_QUANTILES), rtol=1e-12)
    np.testing.assert_allclose(sm["diversity"], D[np.triu_indices(9, 1)].mean(), rtol=1e-12)
    assert sm["nearest_training_dist"] == [float(x) for x in np.quantile(near["q_ref_d"], S.FP_QUANTILES)]
    median = sm["nearest_training_dist"][3]
    w2, _ = finish("b", (median,))
    prec = w2.fingerprint_summary["coverage"][0]["coverage_precision"]
    assert abs(prec - 0.5) <= 1.0 / 9 + 1e-12, prec
    assert w2.fingerprint_summary["coverage"][0]["coverage_recall"] >= 1.0 / 3         # mp-2 has its copy


SIG_QUANTILE = 0.7
COORD_SCALE = 100.0       # random decoder weights give cells of a fraction of an Angstrom: the coordinate channels are scaled up


def write_generate_inputs(root, name="x", d=16, quantile=SIG_QUANTILE, coord_scale=COORD_SCALE):
    """What generate.py reads: random U-Net / VAE weights with the mask threshold moved so that samples segment into atoms
    (as tests/test_gpu_structures.py does), a data/<name> folder in the on-disk format with eight compounds, and a
    three-file sites/ folder.  Returns the site ids."""
    from icsg3d_amd.synthetic import synthetic_batch
    from icsg3d_amd.unet.unet import AtomUnet
    from icsg3d_amd.vae.lattice_vae import LatticeDFCVAE
    wdir_u, wdir_v = os.path.join(root, "saved_models", "unet", name), os.path.join(root, "saved_models", "vae", name)
    os.makedirs(wdir_u)
    os.makedirs(wdir_v)
    np.random.seed(3)
    unet = AtomUnet(input_shape=(d, d, d, 4), max_batch=4)
    unet.model.save(os.path.join(wdir_u, "unet_weights_%s.best.h5" % name))
    vae = LatticeDFCVAE(input_shape=(d, d, d, 4), perceptual_model=os.path.join(wdir_u, "unet_weights_%s.best.h5" % name), cond_shape=4)
    vae._set_model(batch_size=4)
    wv = vae._get_weights()
    wv["dout/gamma"] = wv["dout/gamma"] * np.array([1.0, coord_scale, coord_scale, coord_scale], np.float32)
    vae._set_weights(wv)
    x = synthetic_batch(4, d, 4, seed=0)[0]
    cond = np.tile(np.eye(4, dtype=np.float32)[0], (4, 1))
    recon = vae.model.predict([x, cond], eps=np.random.RandomState(0).standard_normal((4, 256)))
    _, sig = unet.model.predict(recon)
    logit = lambda p: np.log(p) - np.log1p(-p)                                  # noqa: E731
    w = unet._get_weights()
    w["sig/bias"] = w["sig/bias"] + np.float32(logit(0.8) - logit(np.clip(np.quantile(sig, quantile), 1e-6, 1 - 1e-6)))
    unet._set_weights(w)
    unet.model.save_weights(os.path.join(wdir_u, "unet_weights_%s.best.hdf5" % name))
    vae.model.save_weights(os.path.join(wdir_v, "vae_weights_%s.best.hdf5" % name))
    mats = os.path.join(root, "data", name, "matrices")
    for sub in ("density_matrices", "coordinate_grids"):
        os.makedirs(os.path.join(mats, sub))
    rng = np.random.default_rng(46)
    with open(os.path.join(root, "data", name, name + ".csv"), "w") as fh:
        fh.write("task_id,pretty_formula,formation_energy_per_atom,nsites\n")
        for k in range(8):
            X = synthetic_batch(1, d, 4, seed=k, noise=1e-3)[0]
            np.save(os.path.join(mats, "density_matrices", "mp-%d.npy" % k), X[0, ..., 0].astype(np.float64).ravel())
            np.save(os.path.join(mats, "coordinate_grids", "mp-%d.npy" % k), X[0, ..., 1:4].astype(np.float64))
            fh.write("mp-%d,Xmp%d,%.6f,%d\n" % (k, k, rng.normal(), rng.integers(2, 9)))
    sites = os.path.join(root, "data", name, "sites")
    os.makedirs(sites)
    ids = ["mp-1", "mp-2", "mp-3"]
    for sid, (z, fr, l) in zip(ids, _ortho_samples(rng, 3)):
        np.savez(os.path.join(sites, sid + ".npz"), frac_coords=fr, Z=z.astype(float), radii=np.ones(len(z)), lattice=np.r_[l, 90.0, 90.0, 90.0])
    return ids


def run_generate(root, extra, name="x", d=16):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "generate.py"), "--name", name, "--d", str(d), "--batch_size", "16",
                        "--nsamples", "32", "--ncond", "4", "--fingerprint"] + extra,
                       cwd=root, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    print([ln for ln in p.stdout.splitlines() if ln.startswith(("structures:", "fingerprint:"))])


def _rms(a, b):
    """D between every row of a and every row of b, from the differences."""
    return np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).mean(-1))


@pytest.fixture(scope="module")
def generate_root(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("gen"))
    return root, write_generate_inputs(root)


DELTAS = (0.05, 0.2, 0.5, 1.0, 2.0)


def test_generate_with_a_sites_folder(generate_root):
    """generate.py --base mp-3 --match --fingerprint --fp_delta ... on an on-disk dataset with a three-file sites/ folder:
    samples are written, every one names its nearest training structure among the site ids, and the nearest_* columns, the
    quantiles, the diversity and the coverage rows of run.json are those recomputed here from fingerprints.npz and the
    fingerprints of the site folder."""
    root, ids = generate_root
    run_generate(root, ["--base", "mp-3", "--match"] + [x for dl in DELTAS for x in ("--fp_delta", str(dl))])
    res = os.path.join(root, "output", "results", "Xmp3__v=0.5")
    rows = list(csv.DictReader(open(os.path.join(res, "results.csv"), newline="")))
    assert tuple(list(rows[0])[1:]) == S.ResultsWriter.COLUMNS + S.ResultsWriter.MATCH_COLUMNS + S.ResultsWriter.FINGERPRINT_COLUMNS
    info = json.load(open(os.path.join(res, "run.json")))
    blk = info["fingerprint"]
    z = np.load(os.path.join(res, "fingerprints.npz"))
    ok = np.isfinite(z["fp"]).all(1)
    print("written %d, fingerprinted %d" % (len(rows), ok.sum()))
    assert len(z["ids"]) == len(rows) and ok.sum() >= 2
    assert info["fp_delta"] == list(DELTAS) and info["match"]["references"] == 3
    assert (blk["r_max"], blk["n_bins"], blk["width"], blk["cn_tol"], blk["samples"], blk["references"]) == (6.0, 60, 0.1, 0.1, int(ok.sum()), 3)
    ref = S.ReferenceSet.from_sites(os.path.join(root, "data", "x", "sites"))
    assert ref.ids == ids
    rfp = np.array([d["fp"] for d in S.fingerprint(ref.screened())])
    fp = z["fp"][ok]
    names = [i for i, o in zip(z["ids"].tolist(), ok) if o]
    Dr, Dq = _rms(fp, rfp), _rms(fp, fp)
    np.fill_diagonal(Dq, np.inf)
    by_id = {r["id"]: r for r in rows}
    for k, n in enumerate(names):
        r = by_id[n]
        assert r["fp_reason"] == "" and r["nearest_training"] == ids[int(np.argmin(Dr[k]))], (n, r["nearest_training"], Dr[k])
        np.testing.assert_allclose(float(r["nearest_training_dist"]), Dr[k].min(), rtol=1e-9)
        assert r["nearest_generated"] in names and r["nearest_generated"] != n
        np.testing.assert_allclose(float(r["nearest_generated_dist"]), Dq[k].min(), rtol=1e-9, atol=1e-300)
        cn = z["cn"][z["offsets"][z["ids"].tolist().index(n)]:z["offsets"][z["ids"].tolist().index(n) + 1]]
        assert (int(r["cn_min"]), int(r["cn_max"])) == (cn.min(), cn.max()) and abs(float(r["cn_mean"]) - cn.mean()) < 1e-12
    q = S.FP_QUANTILES
    np.testing.assert_allclose(blk["nearest_training_dist"], np.quantile(Dr.min(1), q), rtol=1e-9)
    np.testing.assert_allclose(blk["nearest_sample_of_training_dist"], np.quantile(Dr.min(0), q), rtol=1e-9)
    np.testing.assert_allclose(blk["nearest_generated_dist"], np.quantile(Dq.min(1), q), rtol=1e-9, atol=1e-300)
    np.testing.assert_allclose(blk["diversity"], Dq[np.triu_indices(len(fp), 1)].mean(), rtol=1e-9)
    assert [c["delta"] for c in blk["coverage"]] == list(DELTAS)
    for c in blk["coverage"]:
        assert c["coverage_recall"] == float((Dr.min(0) <= c["delta"]).sum()) / 3, c
        assert c["coverage_precision"] == float((Dr.min(1) <= c["delta"]).sum()) / len(fp), c


def test_generate_synthetic_with_fingerprint(generate_root):
    """generate.py --synthetic --fingerprint has no reference set: samples are written, the training columns are empty and
    the sample-to-sample quantiles and the diversity in run.json are those recomputed from fingerprints.npz."""
    root, _ = generate_root
    run_generate(root, ["--synthetic"])
    res = os.path.join(root, "output", "results", "synthetic__v=0.5")
    rows = list(csv.DictReader(open(os.path.join(res, "results.csv"), newline="")))
    assert tuple(list(rows[0])[1:]) == S.ResultsWriter.COLUMNS + S.ResultsWriter.FINGERPRINT_COLUMNS
    info = json.load(open(os.path.join(res, "run.json")))
    blk = info["fingerprint"]
    z = np.load(os.path.join(res, "fingerprints.npz"))
    ok = np.isfinite(z["fp"]).all(1)
    print("written %d, fingerprinted %d" % (len(rows), ok.sum()))
    assert len(z["ids"]) == len(rows) and ok.sum() >= 2 and blk["samples"] == int(ok.sum())
    assert "match" not in info and info["fp_delta"] is None and blk["coverage"] == []
    assert blk["references"] == 0 and blk["nearest_training_dist"] is None and blk["nearest_sample_of_training_dist"] is None
    assert all(r["nearest_training"] == "" and r["nearest_training_dist"] == "" for r in rows)
    fp = z["fp"][ok]
    Dq = _rms(fp, fp)
    np.fill_diagonal(Dq, np.inf)
    np.testing.assert_allclose(blk["nearest_generated_dist"], np.quantile(Dq.min(1), S.FP_QUANTILES), rtol=1e-9, atol=1e-300)
    np.testing.assert_allclose(blk["diversity"], Dq[np.triu_indices(len(fp), 1)].mean(), rtol=1e-9)
