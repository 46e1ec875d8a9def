"""ics_op_structure_match on the MI355X against the fp64 restatement tests/structure_match_ref.py.

Decisions, indices and counts must be equal.  rms must agree within 1e-9 Angstrom: both sides are fp64 sums of at most 256
terms of order 1 Angstrom, so rounding is ~1e-13 and the bound is slack by derivation.  (op, anchor) are compared only
where the restatement's runner-up rms differs by more than 1e-6 Angstrom (symmetric structures tie).

The kernel does not report how many ops were admissible; where a case is about that count it is asserted on the
restatement (known by construction) and shows on the device through the decisions and the chosen op.

Lattice thresholds.  The predicate bounds the METRIC tensor: |G'_kl - G_B,kl| <= ltol sqrt(G_B,kk G_B,ll).  "Scaled by
1 +- 0.8 ltol" is therefore built on G (cell edges times sqrt(1 +- 0.8 ltol)): that matches, 1 +- 1.3 ltol does not.  The
same factors put on the cell EDGES change G by 1.6 / 2.6 ltol; the predicate as stated rejects all four, and the test
holds the device to the restatement on those too.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import structure_match_cases as C
import structure_match_ref as MR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, LTOL = C.TOL, C.LTOL
RMS_TOL = 1e-9
KEYS = ("dup_of", "dup_rms", "dup_op", "ref_of", "ref_rms", "ref_op", "n_cmp")


def run(structs, nq, eligible=None, ops_mode=1, tol=TOL, ltol=LTOL):
    from icsg3d_amd import structures as S
    off, sp, fr, lattice = C.pack(structs)
    el = np.ones(len(structs), np.int32) if eligible is None else np.asarray(eligible, np.int32)
    return S.match_packed(off, sp, fr, lattice, el, nq, len(structs) - nq, tol, ltol, ops_mode)


def compare(o, r, nq):
    """Device outputs o against the restatement r."""
    print("dup_of", o["dup_of"].tolist(), "ref_of", o["ref_of"].tolist())
    print("dup_rms", o["dup_rms"].tolist(), "ref_rms", o["ref_rms"].tolist())
    for k in ("dup_of", "ref_of", "n_cmp"):
        assert np.array_equal(o[k], r[k]), (k, o[k].tolist(), r[k].tolist())
    for q in range(nq):
        for of, rms, op, pair in (("dup_of", "dup_rms", "dup_op", lambda q: (r["dup_of"][q], q)),
                                  ("ref_of", "ref_rms", "ref_op", lambda q: (q, nq + r["ref_of"][q]))):
            if r[of][q] < 0:
                assert np.isinf(o[rms][q]) and tuple(o[op][q]) == (-1, -1), (q, of)
                continue
            assert abs(o[rms][q] - r[rms][q]) <= RMS_TOL, (q, rms, o[rms][q], r[rms][q])
            p = r["pairs"][pair(q)]
            if p["runner_up"] - p["rms"] > 1e-6:
                assert tuple(o[op][q]) == tuple(r[op][q]), (q, op, o[op][q], r[op][q])


def check(structs, nq, eligible=None, ops_mode=1, tol=TOL, ltol=LTOL):
    el = np.ones(len(structs), np.int32) if eligible is None else np.asarray(eligible, np.int32)
    r = MR.match_ref(structs, el, nq, tol, ltol, ops_mode)
    o = run(structs, nq, el, ops_mode, tol, ltol)
    compare(o, r, nq)
    return o, r


def sized(rng, n, abc=(9.0, 10.0, 11.0)):
    """n atoms, three species, the first one alone (one anchor), orthorhombic."""
    Z = [38] + [22] * ((n - 1) // 3) + [8] * (n - 1 - (n - 1) // 3)
    return C.motif(rng, Z[:n], C.lat(abc), dmin=0.9)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 256])
def test_sizes_on_both_sides_of_the_wave_workgroup_split(n):
    rng = np.random.RandomState(100 + n)
    A = sized(rng, n, (9.0, 10.0, 11.0) if n <= 65 else (15.0, 16.0, 17.0))
    ops = MR.signed_permutations(1)
    B = C.derive(rng, A, ops[5], C.noise_max(rng, n, 0.5 * TOL) if n > 1 else None)[0]
    far = C.derive(rng, A, ops[2], C.noise_one(rng, n, n // 2, 2.5 * TOL) if n > 2 else None)[0]
    ref = C.derive(rng, A, ops[0], C.noise_max(rng, n, 0.2 * TOL) if n > 1 else None)[0]
    o, r = check([A, B, far, ref], 3)
    assert o["dup_of"][1] == 0 and o["ref_of"][0] == 0 and (n <= 2 or o["dup_of"][2] == -1)


def test_no_references_and_a_query_without_candidate():
    rng = np.random.RandomState(1)
    A = C.motif(rng, [57, 26, 8, 8, 8], C.lat([4.4, 5.6, 6.8]))
    lone = C.motif(rng, [3, 9], C.lat([4.0, 4.0, 4.0]))
    o, r = check([A, lone, C.derive(rng, A)[0]], 3)
    assert o["dup_of"].tolist() == [-1, -1, 0] and o["ref_of"].tolist() == [-1, -1, -1]
    assert o["n_cmp"].tolist() == [[0, 0], [0, 0], [1, 0]]


def test_exact_copy_and_the_invariances():
    rng = np.random.RandomState(2)
    A = C.motif(rng, [14, 14, 8, 8, 8, 8, 3, 3], C.lat([5.2, 6.1, 7.3]))
    copy = (A[0].copy(), A[1].copy(), A[2].copy())
    moved = C.derive(rng, A)[0]                        # translation, lattice-vector shifts of single atoms, shuffled order
    o, r = check([A, copy, moved], 3)
    assert o["dup_of"].tolist() == [-1, 0, 0] and o["dup_rms"][1] <= 1e-12 and o["dup_rms"][2] <= 1e-9


def test_orthorhombic_every_op_is_found():
    rng = np.random.RandomState(3)
    A = C.motif(rng, [57, 26, 8, 8, 8], C.lat([4.4, 5.6, 6.8]))
    ops = MR.signed_permutations(2)
    structs = [A] + [C.derive(rng, A, P)[0] for P in ops]
    # A is the query, its 48 images the references: each pair on its own, ops_mode 2
    for k0 in range(0, 48, 16):
        part = [A] + structs[1 + k0:1 + k0 + 16]
        r = MR.match_ref(part, np.ones(len(part), np.int32), 1, TOL, LTOL, 2)
        for k in range(16):
            p = r["pairs"][(0, 1 + k)]
            assert p["n_admissible"] == 8 and p["match"] and p["op"] == k0 + k, (k0 + k, p)    # 8 sign patterns keep G
        o = run(part, 1, ops_mode=2)
        compare(o, r, 1)
    # one reference at a time: the op that was applied comes back
    for k in (0, 7, 13, 29, 47):
        o = run([A, structs[1 + k]], 1, ops_mode=2)
        assert o["ref_of"][0] == 0 and o["ref_op"][0, 0] == k and o["ref_rms"][0] <= 1e-9, k
    # with the 24 rotations only an improper image is not found
    o, r = check([A, structs[1 + 1]], 1, ops_mode=1)      # op 1 = (+, +, -): determinant -1
    assert o["ref_of"][0] == -1


def test_cubic_all_48_admissible_and_the_op_is_found():
    rng = np.random.RandomState(4)
    A = C.motif(rng, [57, 26, 8, 8, 8, 9, 9], C.lat([5.0, 5.0, 5.0]))
    ops = MR.signed_permutations(2)
    for k in (0, 11, 22, 37, 46):
        B = C.derive(rng, A, ops[k], C.noise_max(rng, 7, 0.3 * TOL))[0]
        o, r = check([A, B], 1, ops_mode=2)
        assert r["pairs"][(0, 1)]["n_admissible"] == 48
        assert o["ref_of"][0] == 0 and o["ref_op"][0, 0] == k, k


def test_gamma_120_atoms_across_cell_faces():
    rng = np.random.RandomState(5)
    M = C.lat([5.1, 5.1, 6.4], (90.0, 90.0, 120.0))
    Z, f, _ = C.motif(rng, [22, 8, 8, 38, 8, 8], M)
    for k in range(4):                                                     # four atoms on cell faces, either side
        f[k, k % 3] = rng.randint(2) + rng.uniform(-0.02, 0.02)
    A = (Z, f, M)
    ops = MR.signed_permutations(2)
    keep = [k for k, P in enumerate(ops) if np.allclose(P @ M @ M.T @ P.T, M @ M.T)]
    assert len(keep) == 8
    for k in (keep[3], keep[6]):
        B = C.derive(rng, A, ops[k], C.noise_max(rng, 6, 0.4 * TOL))[0]
        o, r = check([A, B], 1, ops_mode=2)
        assert r["pairs"][(0, 1)]["n_admissible"] == 8 and o["ref_of"][0] == 0
    B = (Z, f @ ops[8].T, M)                      # the image by an op that does not keep G, in the unchanged cell: the
    assert not np.allclose(ops[8] @ M @ M.T @ ops[8].T, M @ M.T)           # eight are admissible, none maps the atoms
    o, r = check([A, B], 1, ops_mode=2)
    assert o["ref_of"][0] == -1 and o["n_cmp"][0, 1] == 1


def test_thresholds_on_the_residual():
    rng = np.random.RandomState(6)
    A = C.motif(rng, [57, 26, 8, 8, 8], C.lat([4.4, 5.6, 6.8]))
    ok = C.derive(rng, A, None, C.noise_max(rng, 5, 0.8 * TOL))[0]
    no = C.derive(rng, A, None, C.noise_one(rng, 5, 3, 1.25 * TOL))[0]
    o, r = check([A, ok, no], 1)
    assert r["pairs"][(0, 1)]["match"] and not r["pairs"][(0, 2)]["match"] and o["ref_of"][0] == 0
    np.testing.assert_allclose(o["ref_rms"][0], r["ref_rms"][0], atol=RMS_TOL)
    # the mean shift: the anchor alone displaced.  n = 4, 1.2 tol: every other atom is 1.2 tol off the anchored image,
    # the common shift taken out leaves 0.9 tol at the anchor and 0.3 tol elsewhere
    A4 = C.motif(rng, [57, 8, 8, 8], C.lat([4.4, 5.6, 6.8]))
    d = np.zeros((4, 3)); d[0] = [1.2 * TOL, 0, 0]
    o, r = check([A4, C.derive(rng, A4, None, d)[0]], 1)
    assert o["ref_of"][0] == 0 and abs(o["ref_rms"][0] - TOL * np.sqrt((0.9 ** 2 + 3 * 0.3 ** 2) / 4)) < 1e-9
    A8 = C.motif(rng, [57, 8, 8, 8, 8, 8, 8, 8], C.lat([5.4, 5.6, 6.8]))
    d = np.zeros((8, 3)); d[0] = [0, 1.5 * TOL, 0]                       # 7/8 of 1.5 tol = 1.31 tol at the anchor
    o, r = check([A8, C.derive(rng, A8, None, d)[0]], 1)
    assert o["ref_of"][0] == -1
    # two atoms of different species exchanged: the same histogram, another structure
    Z, f, M = A
    sw = f.copy(); sw[[0, 2]] = sw[[2, 0]]
    o, r = check([A, (Z, sw, M)], 1)
    assert o["ref_of"][0] == -1 and o["n_cmp"][0, 1] == 1


def test_thresholds_on_the_lattice():
    rng = np.random.RandomState(7)
    A = C.motif(rng, [57, 26, 8], C.lat([3.6, 4.2, 4.9]), dmin=1.5)
    for fac, expect in ((1 + 0.8 * LTOL, True), (1 - 0.8 * LTOL, True), (1 + 1.3 * LTOL, False), (1 - 1.3 * LTOL, False)):
        B = (A[0], A[1], A[2] * np.sqrt(fac))         # the metric tensor times fac
        o, r = check([A, B], 1)
        assert r["pairs"][(0, 1)]["n_admissible"] == (4 if expect else 0) and (o["ref_of"][0] == 0) == expect, fac
        o, r = check([A, (A[0], A[1], A[2] * fac)], 1)                   # the same factor on the cell edges
        assert r["pairs"][(0, 1)]["n_admissible"] == 0 and o["ref_of"][0] == -1, fac


def test_duplicates_and_reference_choice():
    rng = np.random.RandomState(8)
    A = C.motif(rng, [57, 26, 8, 8, 8], C.lat([4.4, 5.6, 6.8]))
    B = C.motif(rng, [57, 26, 8, 8, 8], C.lat([4.4, 5.6, 6.8]))
    Cc = C.motif(rng, [14, 8, 8], C.lat([4.0, 4.5, 5.0]))
    ops = MR.signed_permutations(1)
    v = lambda S, amp, k=0: C.derive(rng, S, ops[k], C.noise_max(rng, len(S[0]), amp * TOL))[0]   # noqa: E731
    queries = [A, B, v(A, 0.3, 3), Cc, v(A, 0.2, 0), v(B, 0.3, 0)]
    near, nearer = v(A, 0.4), v(A, 0.1)
    refs = [near, v(B, 0.2), nearer, (nearer[0].copy(), nearer[1].copy(), nearer[2].copy())]
    o, r = check(queries + refs, 6)
    assert o["dup_of"].tolist() == [-1, -1, 0, -1, 0, 1]
    assert o["ref_of"][0] == 2 and o["ref_rms"][0] < 0.11 * TOL            # the smaller rms, the lower index on the tie
    assert o["ref_of"][1] == 1 and o["ref_of"][3] == -1
    # ineligible structures are never partners
    el = np.ones(10, np.int32); el[[0, 8]] = 0
    o, r = check(queries + refs, 6, eligible=el)
    assert o["dup_of"].tolist() == [-1, -1, -1, -1, 2, 1] and o["n_cmp"][0].tolist() == [0, 0]
    assert o["ref_of"][0] == -1 and np.isinf(o["dup_rms"][0]) and o["ref_of"][2] in (0, 3)


@pytest.fixture(scope="module")
def sweep():
    structs = C.sweep()
    base, bad = C.robust(structs, 40)
    return structs, base, bad


def test_sweep_every_pair_robust_then_equal(sweep):
    structs, base, bad = sweep
    assert not bad, bad                    # EVERY compared pair: the same decision and combination at 0.95 and 1.05
    assert len(base["pairs"]) > 300 and 50 < sum(p["match"] for p in base["pairs"].values()) < len(base["pairs"]) - 50
    o = run(structs, 40)
    compare(o, base, 40)


def test_sweep_twice_the_same_bits(sweep):
    structs = sweep[0]
    a, b = run(structs, 40), run(structs, 40)
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k


def chunk_worker():
    """Run in a fresh process with ICSG3D_MATCH_CHUNK_PAIRS set (it is read once per process)."""
    rng = np.random.RandomState(9)
    A = C.motif(rng, [57, 26, 8, 8, 8], C.lat([4.4, 5.6, 6.8]))
    Bp = C.motif(rng, [57, 26, 8, 8, 8], C.lat([4.4, 5.6, 6.8]))
    ops = MR.signed_permutations(1)
    structs = []
    for k in range(70):                    # one bucket of 70: 12 queries, 58 references; 66 + 696 pairs
        S = A if k % 3 else Bp
        structs.append(C.derive(rng, S, ops[rng.randint(24)], C.noise_max(rng, 5, 0.3 * TOL))[0])
    big = C.motif(rng, [38] + [8] * 69, C.lat([12.0, 13.0, 14.0]), dmin=0.9)           # workgroup pairs behind them
    structs = structs[:12] + [big, C.derive(rng, big)[0]] + structs[12:]
    r = MR.match_ref(structs, np.ones(len(structs), np.int32), 14, TOL, LTOL, 1)
    o = run(structs, 14)
    compare(o, r, 14)
    assert o["n_cmp"][11].tolist() == [11, 58] and o["dup_of"][13] == 12
    print("chunked bucket equal")


def test_bucket_of_70_across_several_chunks():
    env = dict(os.environ, ICSG3D_MATCH_CHUNK_PAIRS="97", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", "import test_gpu_structure_match as T; T.chunk_worker()"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "chunked bucket equal" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def test_results_writer_with_a_matcher(tmp_path):
    """Hand-made atom lists through ResultsWriter(matcher=...): a training structure turned by rot90 (axes 0 and 1:
    x' = 1 - y, y' = x, the cell edges exchanged) and jittered by 0.5 tol comes back as its training id."""
    from icsg3d_amd import structures as S
    rng = np.random.RandomState(10)
    abc = np.array([4.4, 5.6, 6.8])
    Z, f, _ = C.motif(rng, [57, 26, 8, 8, 8], C.lat(abc))
    Z2, f2, _ = C.motif(rng, [57, 26, 8, 8, 8], C.lat(abc))
    ref = S.ReferenceSet(["mp-1", "mp-2"], [Z, [14, 8, 8]], [f, [[0, 0, 0], [0.5, 0.5, 0], [0, 0.5, 0.5]]],
                         [list(abc) + [90, 90, 90], [4, 4, 4, 90, 90, 90]])
    turned = np.stack([1 - f[:, 1], f[:, 0], f[:, 2]], 1)
    abc_t = abc[[1, 0, 2]]
    jit = C.noise_max(rng, 5, 0.5 * TOL)
    atoms = [(Z, turned * abc_t + jit), (Z2, f2 * abc), (Z, f * abc_t + 0.3), (Z2, f2 * abc + C.noise_max(rng, 5, 0.3 * TOL)),
             ([8, 8], np.array([[1.0, 1, 1], [1.2, 1, 1]]))]
    lp = np.array([abc_t, abc, abc_t, abc, abc])
    w = S.ResultsWriter(str(tmp_path), matcher=S.Matcher(ref, TOL, LTOL, 1))
    w.add_batch(range(3), lp[:3], atoms[:3])
    w.add_batch(range(3, 5), lp[3:], atoms[3:])
    counts = w.finish()
    print(counts, w.match_summary)
    assert counts == {"generated": 5, "failed": 0, "invalid": 1, "written": 4, "unique": 3, "novel": 2, "ineligible": 0}
    import csv
    rows = {int(r["sample"]): r for r in csv.DictReader(open(tmp_path / "results.csv"))}
    head = open(tmp_path / "results.csv").readline().strip().split(",")
    assert tuple(head[1:]) == S.ResultsWriter.COLUMNS + S.ResultsWriter.MATCH_COLUMNS
    assert rows[0]["training_match"] == "mp-1" and 0.1 * TOL < float(rows[0]["training_rms"]) <= 0.5 * TOL
    assert rows[0]["duplicate_of"] == "" and rows[1]["training_match"] == "" and rows[2]["training_match"] == ""
    assert rows[3]["duplicate_of"] == rows[1]["id"] and float(rows[3]["duplicate_rms"]) <= 0.3 * TOL
    assert all(r["match_reason"] == "" for r in rows.values())
