"""The fingerprint's definition on the host: the restatement (tests/structure_fingerprint_ref.py) against closed forms and
its own invariances, the nearest op's restatement on exact copies, the Python layer (fingerprint, Fingerprinter,
ResultsWriter, generate.py's flags) with the two wrappers replaced by the restatement, and the stand-alone sanitizer
check of fingerprint.h.  No GPU.

The first four tests (closed forms, invariances, reason bits, the nearest restatement) run the numpy restatement alone:
they pin the REFERENCE the device ops are held against, not the feature, and need nothing this change adds outside tests/.
The tests from the Python layer on exercise the feature."""
import csv
import io
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import structure_fingerprint_cases as C
import structure_fingerprint_ref as FR
from icsg3d_amd import structures as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.PARAMS


def test_simple_cubic_closed_forms():
    """a = 3, one atom, w = 0.1, 60 bins to 6: shells of 6, 12 and 8 images at a, a sqrt 2 and a sqrt 3, and the shell of 6
    at 2a = r_max deposits exactly half: 3."""
    Z, f, M = C.cubic(3.0)
    o = FR.fingerprint_checked(Z, f, M, **P)
    r = FR.edges(6.0, 60)
    for d, want in ((3.0, 6.0), (3.0 * 2 ** 0.5, 12.0), (3.0 * 3 ** 0.5, 8.0)):
        touched = (r[1:] > d - 0.1) & (r[:-1] < d + 0.1)
        assert abs(o["count"][touched].sum() - want) <= 1e-12, (d, o["count"][touched])
    last = (r[1:] > 6.0 - 0.1)
    assert o["count"][last].sum() == 3.0
    assert abs(o["count"].sum() - (6 + 12 + 8 + 3)) <= 1e-12 and o["n_pairs"] == 32
    assert o["cn"].tolist() == [6] and o["nn_dist"].tolist() == [3.0]
    assert np.allclose(o["rdf"][0], o["rdf"][1], rtol=1e-15)                 # one species: Z_i Z_j / Zbar^2 = 1
    # the same crystal with an unwrapped coordinate, and without wrapping at all
    assert np.array_equal(FR.fingerprint_one(Z, f + [3.0, -2.0, 1.0], M, **P)["count"], o["count"])
    u = FR.fingerprint_one(Z, f + [3.0, -2.0, 1.0], M, wrap=False, **P)
    assert np.abs(u["count"] - o["count"]).max() <= 1e-12 and u["cn"].tolist() == [6]


def _same(a, b, what, bound=1e-12):
    gap = max(np.abs(a["rdf"] - b["rdf"]).max(), np.abs(np.sort(a["nn_dist"]) - np.sort(b["nn_dist"])).max())
    print(what, "gap %.2e" % gap)
    assert gap <= bound, (what, gap)
    assert sorted(a["cn"].tolist()) == sorted(b["cn"].tolist()), what


def test_invariances_of_the_restatement():
    """Supercells, a permutation of the atoms, a signed axis permutation of the cell and a rigid shift leave g, gZ and the
    neighbour lists unchanged to 1e-12 (the raw counts scale with the cell: n_pairs by the number of cells)."""
    S0 = C.triclinic5()
    o = FR.fingerprint_checked(*S0, **P)
    assert o["gap"] > C.GAP
    for reps in ((2, 1, 1), (2, 2, 1)):
        sc = FR.fingerprint_checked(*C.supercell(S0, reps), **P)
        m = int(np.prod(reps))
        assert sc["n_pairs"] == m * o["n_pairs"] and np.abs(sc["count"] - m * o["count"]).max() <= 1e-11
        _same({**sc, "nn_dist": sc["nn_dist"][::m], "cn": sc["cn"][::m]}, o, "supercell %s" % (reps,))
    Z, f, M = S0
    perm = np.array([3, 0, 4, 2, 1])
    _same(FR.fingerprint_checked(Z[perm], f[perm], M, **P), o, "atom permutation")
    for k in (5, 13, 22):
        _same(FR.fingerprint_checked(*C.rotated(S0, k), **P), o, "signed axis permutation %d" % k)
    _same(FR.fingerprint_checked(Z, f + [0.37, -1.21, 2.5], M, **P), o, "rigid shift")
    # g tends to 1: the mean over the last third of a long range is within a few percent for a 5-atom cell
    far = FR.fingerprint_one(Z, f, M, r_max=12.0, n_bins=60, w=0.3, cn_tol=0.1)
    assert abs(far["rdf"][0][40:].mean() - 1.0) < 0.1 and abs(far["rdf"][1][40:].mean() - 1.0) < 0.15


def test_reason_bits_and_neutral_outputs_of_the_restatement():
    structs = [C.cubic(), C.too_dense(), C.triclinic5()]
    o = FR.fingerprint_ref(structs, [1, 1, 0], **P)
    assert o["reason"].tolist() == [0, 2, 1] and o["n_pairs"].tolist()[1:] == [-1, -1]
    assert np.all(np.isnan(o["rdf"][1:])) and np.all(np.isnan(o["nn_dist"][1:])) and np.all(o["cn"][1:] == -1)


def test_nearest_restatement_copies_ties_and_invalid_rows():
    fp, valid = C.nearest_table(3, 6, 5, 7, invalid=(2, 8), duplicates=((4, 1), (7, 1), (9, 1), (10, 3)))
    o = FR.nearest_ref(fp, valid, 6, 5)
    assert o["q_ref"][1] == 1 and o["q_ref_d"][1] == 0.0           # rows 7 and 9 copy query 1: the lower reference
    assert o["q_q"][1] == 4 and o["q_q"][4] == 1 and o["q_q_d"][4] == 0.0
    assert o["ref_q"][1] == 1 and o["ref_q"][3] == 1 and o["ref_q_d"][3] == 0.0 and o["ref_q"][4] == 3
    assert o["q_ref"][2] == -1 and np.isinf(o["q_q_d"][2]) and o["ref_q"][2] == -1 and np.isinf(o["ref_q_d"][2])
    assert 2 not in o["q_q"].tolist() and 2 not in o["ref_q"].tolist() and 2 not in o["q_ref"].tolist()
    assert o["div_pairs"] == 10
    want = sum(FR.distance(fp[a], fp[b]) for a in range(6) for b in range(a + 1, 6) if a != 2 and b != 2)
    assert abs(o["div_sum"] - want) <= 1e-12 * want
    one = FR.nearest_ref(fp[:1], valid[:1], 1, 0)
    assert one["q_q"].tolist() == [-1] and one["div_pairs"] == 0 and one["div_sum"] == 0.0 and len(one["ref_q"]) == 0


# ---------------------------------------------------------------- the Python layer on the restatement
@pytest.fixture()
def on_ref(monkeypatch):
    monkeypatch.setattr(S, "fingerprint_packed", FR.packed_ref)
    monkeypatch.setattr(S, "fingerprint_nearest", FR.nearest_packed_ref)


def _ortho(abc, Z, f):
    return np.array(Z, np.int32), np.array(f, np.float64), C.lat(abc)


def _samples():
    b = C.base_cases()
    return [b["perovskite"], _ortho([4.0, 5.0, 6.0], [22, 8, 8], [[0, 0, 0], [.3, .2, .1], [.7, .2, .9]]), b["rocksalt"],
            b["perovskite"], _ortho([3.0, 4.5, 5.5], [14, 8], [[.1, .1, .1], [.6, .5, .4]])]


def _fake_screen(structs, invalid=2):
    def screen(lattice_params, atoms, alpha=90, beta=90, gamma=90, tol=0.5):
        out = []
        for at in atoms:
            if at is None:
                out.append(None)
                continue
            r = dict(C.as_result(structs[at[0]]))
            r["formula"] = S.formula(r["hist"])
            r["valid"] = at[0] != invalid
            r["reason"] = 0 if r["valid"] else S.REASON_CLOSE
            out.append(r)
        return out
    return screen


def _reference(structs):
    """A ReferenceSet whose screened() is built here (the device screen is not available)."""
    ids = ["ref-%d" % k for k in range(len(structs))]
    ref = S.ReferenceSet(ids, [s[0] for s in structs], [s[1] for s in structs],
                         [np.r_[np.sqrt((s[2] ** 2).sum(1)), 90.0, 90.0, 90.0] for s in structs])
    ref._screened = [C.as_result(s) for s in structs]
    return ref


def test_fingerprint_over_screen_dicts(on_ref):
    structs = _samples()
    res = [C.as_result(s) for s in structs] + [None]
    res[1] = dict(res[1], valid=False)
    big = C.as_result((np.full(257, 8, np.int32), np.random.default_rng(0).uniform(size=(257, 3)), C.lat([20.0] * 3)))
    out = S.fingerprint(res + [big], r_max=6.0, n_bins=60, width=0.1, cn_tol=0.1)
    assert [d["fp_reason"] for d in out] == [0, 1, 0, 0, 0, 1, 1]
    assert out[1]["fp"] is None and out[5]["rdf"] is None and out[6]["cn"] is None
    o = FR.fingerprint_checked(*structs[0], **P)
    assert out[0]["fp"].shape == (120,) and np.array_equal(out[0]["fp"], o["rdf"].reshape(-1))
    assert np.array_equal(out[0]["fp"][:60], out[0]["rdf"][0]) and np.array_equal(out[0]["cn"], o["cn"])
    assert np.array_equal(out[0]["fp"], out[3]["fp"])
    assert all(d["fp"] is None for d in S.fingerprint([None, None]))
    with pytest.raises(ValueError):
        S.fingerprint(res, n_bins=257)
    with pytest.raises(ValueError):
        S.Fingerprinter(width=0.0)


def test_wrappers_check_lengths_before_the_call():
    with pytest.raises(ValueError):
        S.fingerprint_nearest(np.zeros((3, 4)), np.ones(2), 2, 1)
    with pytest.raises(ValueError):
        S.fingerprint_nearest(np.zeros((3, 4)), np.ones(3), 0, 3)
    with pytest.raises(ValueError):
        S.fingerprint_packed(np.array([0, 1]), [8], np.zeros((2, 3)), np.eye(3)[None], [1])
    with pytest.raises(ValueError):
        S.fingerprint_packed(np.array([0, 1]), [8], np.zeros((1, 3)), np.eye(3)[None], [1], n_bins=0)


def test_results_writer_with_and_without_a_fingerprinter(on_ref, tmp_path, monkeypatch):
    """Without fingerprinter= the files are text built here from the untouched pieces; with it the same files plus the new
    columns, fingerprints.npz and the summary, the reference fingerprinted once."""
    structs = _samples()
    monkeypatch.setattr(S, "screen", _fake_screen(structs))
    atoms = [(k, None) for k in range(len(structs))] + [None]
    plain, fpd = str(tmp_path / "plain"), str(tmp_path / "fp")
    w = S.ResultsWriter(plain, training_names=("LaFeO3",), target_value=1.5)
    w.add_batch(range(6), np.ones((6, 3)), atoms)
    counts = w.finish()
    assert counts == {"generated": 6, "failed": 1, "invalid": 1, "written": 4} and w.fingerprint_summary is None
    assert w.structs == []
    rows, seen, js = [], [], ""
    for k in (0, 1, 3, 4):
        r = C.as_result(structs[k])
        f = S.formula(r["hist"])
        fid = S.numbered(f, seen)
        seen.append(f)
        path = os.path.join(plain, "cifs", fid + ".cif")
        rd = {"formula": f, "id": fid, "training": int(S.reduced_formula(r["hist"]) in {"LaFeO3"}), "target": 1.5,
              "anon_formula": S.anonymized_formula(r["hist"]), "electronegativity": S.average_electroneg(r["hist"]),
              "cif": path, "sample": k, "natoms": len(r["species"]), "min_distance": r["min_dist"], "volume": r["volume"]}
        rows.append(rd)
        js += json.dumps(str(rd))
    assert open(os.path.join(plain, "results.json")).read() == js
    buf = io.StringIO(newline="")
    cw = csv.writer(buf)
    cw.writerow(("",) + S.ResultsWriter.COLUMNS)
    for i in sorted(range(len(rows)), key=lambda i: rows[i]["id"]):
        cw.writerow([i] + [repr(rows[i][c]) if isinstance(rows[i][c], float) else rows[i][c] for c in S.ResultsWriter.COLUMNS])
    assert open(os.path.join(plain, "results.csv"), newline="").read() == buf.getvalue()
    assert sorted(os.listdir(plain)) == ["cifs", "results.csv", "results.json"]

    # ---- with a fingerprinter: references = the rocksalt, a rotated copy of sample 1 and an unrelated cell
    refs = [C.base_cases()["rocksalt"], C.rotated(structs[1], 9), _ortho([5.0, 5.0, 7.0], [26, 16], [[0, 0, 0], [.5, .5, .4]])]
    calls = []
    ref = _reference(refs)
    monkeypatch.setattr(S, "fingerprint_packed", lambda *a, **k: (calls.append(len(a[0]) - 1), FR.packed_ref(*a, **k))[1])
    fpr = S.Fingerprinter(ref, deltas=(1e-9, 1e9))
    w2 = S.ResultsWriter(fpd, training_names=("LaFeO3",), target_value=1.5, fingerprinter=fpr)
    w2.add_batch(range(6), np.ones((6, 3)), atoms)
    c2 = w2.finish()
    assert c2 == dict(counts, fingerprinted=4)
    assert open(os.path.join(fpd, "results.json")).read() == js.replace(plain, fpd)
    got = list(csv.DictReader(open(os.path.join(fpd, "results.csv"), newline="")))
    old = list(csv.DictReader(open(os.path.join(plain, "results.csv"), newline="")))
    assert list(got[0])[-8:] == list(S.ResultsWriter.FINGERPRINT_COLUMNS)
    assert list(got[0])[:-8] == list(old[0])
    by_id = {r["id"]: r for r in got}
    for a, b in zip(got, old):
        assert all(a[c] == b[c] for c in S.ResultsWriter.COLUMNS if c != "cif") and a["fp_reason"] == ""
    assert by_id["Ti1 O2"]["nearest_training"] == "ref-1" and float(by_id["Ti1 O2"]["nearest_training_dist"]) <= 1e-10
    # the two perovskites are bit-equal structures: each is the other's nearest sample at distance 0
    assert by_id["La1 Fe1 O3"]["nearest_generated"] == "La1 Fe1 O3_1" and float(by_id["La1 Fe1 O3"]["nearest_generated_dist"]) == 0.0
    assert by_id["La1 Fe1 O3_1"]["nearest_generated"] == "La1 Fe1 O3"
    assert (by_id["La1 Fe1 O3"]["cn_min"], by_id["La1 Fe1 O3"]["cn_max"]) == ("2", "12")       # O: 2 Fe; La: 12 O
    assert abs(float(by_id["La1 Fe1 O3"]["cn_mean"]) - (12 + 6 + 2 * 3) / 5) < 1e-12
    z = np.load(os.path.join(fpd, "fingerprints.npz"))
    assert z["ids"].tolist() == [r["id"] for r in w2.rows] and z["fp"].shape == (4, 120) and z["rdf"].shape == (4, 2, 60)
    assert z["offsets"].tolist() == [0, 5, 8, 13, 15] and len(z["cn"]) == 15 and len(z["nn_dist"]) == 15
    assert (float(z["r_max"]), int(z["n_bins"]), float(z["width"]), float(z["cn_tol"])) == (6.0, 60, 0.1, 0.1)
    assert np.array_equal(z["fp"][0], FR.fingerprint_checked(*structs[0], **P)["rdf"].reshape(-1))
    sm = w2.fingerprint_summary
    assert (sm["samples"], sm["references"], sm["r_max"], sm["n_bins"]) == (4, 3, 6.0, 60)
    near = w2.fingerprint_results["nearest"]
    assert sm["diversity"] == near["div_sum"] / 6 and sm["quantiles"] == list(S.FP_QUANTILES)
    assert sm["nearest_training_dist"] == [float(x) for x in np.quantile(near["q_ref_d"], S.FP_QUANTILES)]
    assert sm["nearest_generated_dist"][0] == 0.0 and len(sm["nearest_sample_of_training_dist"]) == 7
    assert [c["delta"] for c in sm["coverage"]] == [1e-9, 1e9]
    assert sm["coverage"][0] == {"delta": 1e-9, "coverage_recall": 1 / 3, "coverage_precision": 1 / 4}
    assert sm["coverage"][1] == {"delta": 1e9, "coverage_recall": 1.0, "coverage_precision": 1.0}
    json.dumps(sm)
    # the reference set is fingerprinted once, whatever is called again
    assert calls == [4, 3]
    fpr(w2.structs)
    assert calls == [4, 3, 4]
    # no reference: the sample-to-sample columns only, and no delta means no coverage rows
    w3 = S.ResultsWriter(str(tmp_path / "noref"), fingerprinter=S.Fingerprinter())
    w3.add_batch(range(6), np.ones((6, 3)), atoms)
    w3.finish()
    assert all(r["nearest_training"] is None and r["nearest_training_dist"] is None for r in w3.rows)
    assert w3.fingerprint_summary["coverage"] == [] and w3.fingerprint_summary["nearest_training_dist"] is None
    assert w3.fingerprint_summary["references"] == 0 and w3.fingerprint_summary["diversity"] == sm["diversity"]


def test_generate_lists_the_flags():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "generate.py"), "--help"], capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    for flag in ("--fingerprint", "--fp_rmax", "--fp_bins", "--fp_width", "--fp_cn_tol", "--fp_delta"):
        assert flag in p.stdout, flag
    import importlib.util
    spec = importlib.util.spec_from_file_location("generate_script", os.path.join(ROOT, "generate.py"))
    generate = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(generate)
    a = generate.build_parser().parse_args(["--fingerprint", "--fp_delta", "0.1", "--fp_delta", "0.2"])
    assert a.fp_delta == [0.1, 0.2] and (a.fp_rmax, a.fp_bins, a.fp_width, a.fp_cn_tol) == (6.0, 60, 0.1, 0.1)
    assert generate.build_parser().parse_args([]).fp_delta is None


def test_fingerprint_header_is_clean_under_asan_ubsan():
    """`make build-asan/fingerprint_check`: fingerprint.h compiled as plain C++ with the host sanitizers into a stand-alone
    program (its own main) and run: H, the deposits, the image range, the argument checks."""
    csrc = os.path.join(ROOT, "icsg3d_amd", "csrc")
    assert shutil.which("make") and os.path.exists("/opt/rocm/lib/llvm/bin/clang++"), "no toolchain: fingerprint.h is not checked"
    p = subprocess.run(["make", "-C", csrc, "build-asan/fingerprint_check"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    r = subprocess.run([os.path.join(csrc, "build-asan", "fingerprint_check")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "fingerprint_check: ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
