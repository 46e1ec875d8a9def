"""Structure matching without a GPU: the fp64 restatement tests/structure_match_ref.py (what the GPU tests hold
ics_op_structure_match to) on hand-built cases whose answers are known by construction, the op table, the eligibility
bits, ReferenceSet, the entry point's refusals (they come before any device work), and ResultsWriter with and without a
matcher around a host stand-in for the device screen."""
import csv
import ctypes
import os

import numpy as np
import pytest

import structure_match_cases as C
import structure_match_ref as MR
import structure_ref as SR
from icsg3d_amd import structures as S

TOL, LTOL = C.TOL, C.LTOL


def test_restatement_on_cases_known_by_construction():
    rng = np.random.RandomState(6)
    A = C.motif(rng, [57, 26, 8, 8, 8], C.lat([4.4, 5.6, 6.8]))
    # an exact copy moved, shifted by lattice vectors and shuffled; the residuals of zero-mean noise are the noise
    B, perm = C.derive(rng, A)
    r = MR.match_pair(A, B, TOL, LTOL, 1)
    assert r["match"] and r["rms"] < 1e-12 and r["op"] == 0 and r["n_admissible"] == 4
    assert r["anchor"] == int(np.nonzero(perm == 1)[0][0])          # Fe (Z 26) is the lower Z of the two single species
    d = C.noise_max(rng, 5, 0.8 * TOL)
    r = MR.match_pair(A, C.derive(rng, A, None, d)[0], TOL, LTOL, 1)
    assert r["match"] and abs(r["rms"] - np.sqrt((d * d).sum(1).mean())) < 1e-12
    assert not MR.match_pair(A, C.derive(rng, A, None, C.noise_one(rng, 5, 3, 1.25 * TOL))[0], TOL, LTOL, 1)["match"]
    # the mean shift: the anchor alone displaced by 1.2 tol in n = 4 leaves 0.9 tol at the anchor, 0.3 tol elsewhere
    A4 = C.motif(rng, [57, 8, 8, 8], C.lat([4.4, 5.6, 6.8]))
    d = np.zeros((4, 3)); d[0] = [1.2 * TOL, 0, 0]
    r = MR.match_pair(A4, C.derive(rng, A4, None, d)[0], TOL, LTOL, 1)
    assert r["match"] and abs(r["rms"] - TOL * np.sqrt((0.81 + 3 * 0.09) / 4)) < 1e-12
    A8 = C.motif(rng, [57, 8, 8, 8, 8, 8, 8, 8], C.lat([5.4, 5.6, 6.8]))
    d = np.zeros((8, 3)); d[0] = [0, 1.5 * TOL, 0]
    assert not MR.match_pair(A8, C.derive(rng, A8, None, d)[0], TOL, LTOL, 1)["match"]
    # other compositions are not compared; a swap of two species is compared and is another structure
    assert not MR.match_pair(A, A4)["compared"]
    sw = A[1].copy(); sw[[0, 2]] = sw[[2, 0]]
    r = MR.match_pair(A, (A[0], sw, A[2]))
    assert r["compared"] and not r["match"]
    # every op applied to an orthorhombic cell is found again; the 8 sign patterns of its permutation keep G
    ops = MR.signed_permutations(2)
    for k in (0, 9, 21, 30, 47):
        r = MR.match_pair(A, C.derive(rng, A, ops[k])[0], TOL, LTOL, 2)
        assert r["match"] and r["op"] == k and r["n_admissible"] == 8 and r["rms"] < 1e-12
    # the metric tensor times 1 +- 0.8 ltol is admissible, 1 +- 1.3 ltol is not
    S3 = C.motif(rng, [57, 26, 8], C.lat([3.6, 4.2, 4.9]), dmin=1.5)
    for fac, ok in ((1.04, True), (0.96, True), (1.065, False), (0.935, False)):
        assert MR.match_pair(S3, (S3[0], S3[1], S3[2] * np.sqrt(fac)), TOL, LTOL, 1)["match"] == ok
    # per query: the smallest earlier duplicate, the reference of smallest rms, the lower index on a tie
    v = lambda amp: C.derive(rng, A, None, C.noise_max(rng, 5, amp * TOL))[0]          # noqa: E731
    near = v(0.1)
    o = MR.match_ref([A, v(0.2), v(0.3), v(0.4), near, near], np.ones(6, np.int32), 3)
    assert o["dup_of"].tolist() == [-1, 0, 0] and o["ref_of"].tolist()[0] == 1 and o["n_cmp"].tolist() == [[0, 3], [1, 3], [2, 3]]
    o = MR.match_ref([A, v(0.2), v(0.3), v(0.4), near, near], np.array([0, 1, 1, 1, 0, 1]), 3)
    assert o["dup_of"].tolist() == [-1, -1, 1] and o["ref_of"][0] == -1 and o["ref_of"][1] == 2


def test_signed_permutations():
    for mode, n in ((0, 1), (1, 24), (2, 48)):
        ops = S.signed_permutations(mode)
        assert ops.shape == (n, 3, 3) and np.array_equal(ops[0], np.eye(3))
        assert np.array_equal(ops, MR.signed_permutations(mode))
        assert np.all(np.abs(ops).sum(1) == 1) and np.all(np.abs(ops).sum(2) == 1)
        keys = {P.astype(int).tobytes() for P in ops}
        assert len(keys) == n
        for P in ops:                                           # closed under product
            for Q in ops[::5]:
                assert (P @ Q).astype(int).tobytes() in keys
    dets = np.round(np.linalg.det(S.signed_permutations(2)))
    assert (dets == 1).sum() == 24 and np.all(np.round(np.linalg.det(S.signed_permutations(1))) == 1)
    assert np.array_equal(S.signed_permutations(2)[dets == 1], S.signed_permutations(1))       # the +1 subset, in order
    # lexicographic over (permutation, sign pattern): op 1 flips z, op 8 exchanges y and z
    assert np.array_equal(S.signed_permutations(2)[1], np.diag([1.0, 1, -1]))
    assert np.array_equal(S.signed_permutations(2)[8], [[1, 0, 0], [0, 0, 1], [0, 1, 0]])
    with pytest.raises(ValueError):
        S.signed_permutations(3)


def _res(n=3, min_dist=2.0, lattice=None, valid=True):
    return {"species": np.full(n, 8, np.int32), "frac": np.zeros((n, 3)), "min_dist": min_dist, "valid": valid,
            "lattice": np.diag([4.0, 5.0, 6.0]) if lattice is None else lattice}


def test_eligibility_bits_at_each_boundary():
    tol = 0.1
    r = [_res(), None, _res(valid=False), _res(256), _res(257), _res(min_dist=0.4), _res(min_dist=np.nextafter(0.4, 1)),
         _res(min_dist=np.inf, n=1), _res(lattice=np.diag([0.4, 5.0, 6.0])), _res(lattice=np.diag([0.41, 5.0, 6.0])),
         _res(257, 0.3, np.diag([0.3, 5.0, 6.0])), _res(0)]
    bits = S.eligibility(r, tol).tolist()
    A, Cl, T, I = S.INELIGIBLE_ATOMS, S.INELIGIBLE_CLOSE, S.INELIGIBLE_THIN, S.INELIGIBLE_INVALID
    assert bits == [0, I, I, 0, A, Cl, 0, 0, T, 0, A | Cl | T, I]       # 2 tol / 0.4 = 0.5: thin; min_dist = 4 tol: close
    assert S.ineligible_text(A | T) == "more than 256 atoms, cell too thin for tol" and S.ineligible_text(0) == "eligible"
    # a skewed cell: the inverse-column norm, not the edge, decides
    M = SR.lattice_from_parameters(1.0, 1.0, 6.0, 90, 90, 150)
    assert np.linalg.norm(np.linalg.inv(M), axis=0).max() > 1.9 and S.eligibility([_res(lattice=M)], 0.13)[0] == T
    assert S.eligibility([_res(lattice=M)], 0.12)[0] == 0


def test_reference_set_from_a_sites_folder(tmp_path):
    sites = tmp_path / "sites"
    sites.mkdir()
    rng = np.random.RandomState(0)
    want = {}
    for name, n in (("mp-20", 4), ("mp-3", 2), ("mp-100", 7)):
        frac, Z = rng.uniform(0, 1, (n, 3)), rng.randint(1, 95, n).astype(np.float64)
        lat = np.array([4.0 + n, 5.0, 6.0, 90.0, 100.0, 120.0 if n == 7 else 90.0])
        np.savez(sites / (name + ".npz"), frac_coords=frac, Z=Z, radii=np.ones(n), lattice=lat)
        want[name] = (frac, Z, lat)
    (sites / "notes.txt").write_text("not a structure")
    ref = S.ReferenceSet.from_sites(str(sites))
    assert ref.ids == ["mp-100", "mp-20", "mp-3"] and len(ref) == 3               # sorted by file name, ids kept
    for k, name in enumerate(ref.ids):
        frac, Z, lat = want[name]
        assert np.array_equal(ref.frac[k], frac) and np.array_equal(ref.species[k], Z.astype(np.int32))
        assert ref.species[k].dtype == np.int32 and np.array_equal(ref.lattice_params[k], lat)
    np.testing.assert_allclose(S.cell(ref.lattice_params[0, :3], ref.lattice_params[0, 3:])[0],
                               SR.lattice_from_parameters(*ref.lattice_params[0]), atol=1e-13)
    assert S.match([], ref) == [] and S.match([None], None)[0]["match_reason"] == S.INELIGIBLE_INVALID


def test_entry_point_refusals_name_the_structure():
    from icsg3d_amd import _lib as L
    lib = L.load()
    rng = np.random.RandomState(1)
    structs = [C.motif(rng, [57, 26, 8], C.lat([4.0, 5.0, 6.0])) for _ in range(4)]
    off, sp, fr, lat = C.pack(structs)
    el = np.ones(4, np.int32)

    def call(off_=off, sp_=sp, fr_=fr, lat_=lat, el_=el, nq=3, nref=1, tol=0.1, ltol=0.05, mode=1, null=None):
        outs = [np.full(3, 77, np.int32), np.full(3, 7.5), np.full((3, 2), 77, np.int32), np.full(3, 77, np.int32),
                np.full(3, 7.5), np.full((3, 2), 77, np.int32), np.full((3, 2), 77, np.int32)]
        ins = {"off": L.i32ptr(off_), "sp": L.i32ptr(sp_), "fr": L.f64ptr(fr_), "lat": L.f64ptr(lat_), "el": L.i32ptr(el_)}
        ptr = [L.f64ptr(a) if a.dtype == np.float64 else L.i32ptr(a) for a in outs]
        if null in ins:
            ins[null] = None
        if null == "out":
            ptr[4] = None
        rc = lib.ics_op_structure_match(ins["off"], ins["sp"], ins["fr"], ins["lat"], ins["el"], nq, nref,
                                        ctypes.c_double(tol), ctypes.c_double(ltol), mode, *ptr)
        untouched = all(np.all(a == (7.5 if a.dtype == np.float64 else 77)) for a in outs)
        return rc, untouched, (lib.ics_last_error() or b"").decode()

    def mod(a, idx, v):
        b = a.copy()
        b[idx] = v
        return b

    big = C.pack([(np.full(257, 8), np.zeros((257, 3)), C.lat([30.0, 30.0, 30.0]))])
    cases = {
        "nq 0": (dict(nq=0), "nq"), "nref -1": (dict(nref=-1), "nref"),
        "null offsets": (dict(null="off"), "null"), "null species": (dict(null="sp"), "null"),
        "null frac": (dict(null="fr"), "null"), "null lattice": (dict(null="lat"), "null"),
        "null eligible": (dict(null="el"), "null"), "null output": (dict(null="out"), "null output"),
        "tol 0": (dict(tol=0.0), "tol"), "tol nan": (dict(tol=float("nan")), "tol"), "tol inf": (dict(tol=float("inf")), "tol"),
        "ltol negative": (dict(ltol=-0.05), "ltol"), "ltol nan": (dict(ltol=float("nan")), "ltol"),
        "ops_mode 3": (dict(mode=3), "ops_mode"), "ops_mode -1": (dict(mode=-1), "ops_mode"),
        "offsets[0]": (dict(off_=mod(off, 0, 1)), "offsets[0]"),
        "offsets decrease": (dict(off_=mod(off, 2, off[1] - 1)), "structure 1"),
        "257 atoms": (dict(off_=big[0], sp_=big[1], fr_=big[2], lat_=big[3], el_=np.ones(1, np.int32), nq=1, nref=0),
                      "structure 0 has 257 atoms"),
        "no atoms": (dict(off_=mod(off, 4, off[3])), "structure 3 has no atoms"),
        "frac nan": (dict(fr_=mod(fr, (7, 1), np.nan)), "structure 2"),
        "frac inf": (dict(fr_=mod(fr, (0, 0), np.inf)), "structure 0"),
        "lattice nan": (dict(lat_=mod(lat, (1, 1, 1), np.nan)), "structure 1"),
        "species 0": (dict(sp_=mod(sp, 4, 0)), "structure 1 has a species"),
        "species 95": (dict(sp_=mod(sp, 11, 95)), "structure 3 has a species"),
        "volume 0": (dict(lat_=mod(lat, (2, 2), [0.0, 0.0, 0.0])), "structure 2 has a lattice volume"),
        "volume negative": (dict(lat_=mod(lat, (2, 2, 2), -6.0)), "structure 2 has a lattice volume"),
        "thin cell": (dict(lat_=mod(lat, (3, 0, 0), 0.39)), "structure 3: the cell is too thin"),
        "thin for this tol": (dict(tol=1.1), "structure 0: the cell is too thin"),
    }
    for name, (kw, text) in cases.items():
        rc, untouched, msg = call(**kw)
        assert rc != 0 and untouched, name
        assert "ics_op_structure_match" in msg and text in msg, (name, msg)
    # the same faults in an INELIGIBLE structure are not looked at: the checks pass and the call goes on to the device
    # (which this machine may not have, so only the message is looked at)
    rc, _, msg = call(sp_=mod(sp, 4, 0), el_=np.array([1, 0, 1, 1], np.int32))
    assert rc == 0 or "ics_op_structure_match:" not in msg


def host_screen(lattice_params, atoms, alpha=90, beta=90, gamma=90, tol=0.5):
    """screen() without the device, from the fp64 restatement of the screen (orthogonal cells: volume = a b c)."""
    res = []
    for lp, at in zip(np.asarray(lattice_params, np.float64), atoms):
        if at is None:
            res.append(None)
            continue
        r = SR.screen_ref(at[0], at[1], lp, [alpha, beta, gamma], tol, images=1)
        res.append({"species": np.asarray(at[0], np.int32), "frac": r["frac"], "abc": lp.copy(),
                    "angles": np.array([alpha, beta, gamma], np.float64), "lattice": r["lattice"],
                    "volume": float(lp[0] * lp[1] * lp[2]), "min_dist": float(r["min_dist"]), "min_pair": r["min_pair"],
                    "n_close": r["n_close"], "nearest": r["nearest"], "hist": r["hist"], "valid": bool(r["valid"]),
                    "reason": r["reason"], "formula": S.formula(r["hist"])})
    return res


PEROV = ([57, 26, 8, 8, 8], np.array([[0.0, 0, 0], [2, 2, 2], [2, 2, 0], [2, 0, 2], [0, 2, 2]]))
ATOMS = [PEROV, None, ([8, 8], np.array([[1.0, 1, 1], [1.25, 1, 1]])), (PEROV[0], PEROV[1] + 0.25),
         ([14, 14], np.array([[0.0, 0, 0], [1, 1, 3]]))]
# what the code before the matcher existed wrote for ATOMS (recorded from it, not from the code under test)
CSV = (",formula,id,training,target,anon_formula,electronegativity,cif,sample,natoms,min_distance,volume\n"
       "0,La1 Fe1 O3,La1 Fe1 O3,1,-1.5,ABC3,2.65,out/cifs/La1 Fe1 O3.cif,10,5,2.0,64.0\n"
       "1,La1 Fe1 O3,La1 Fe1 O3_1,1,-1.5,ABC3,2.65,out/cifs/La1 Fe1 O3_1.cif,13,5,2.0,64.0\n"
       "2,Si2,Si2,0,-1.5,A,1.9,out/cifs/Si2.cif,14,2,1.7320508075688772,64.0\n")
JSON = ("\"{'formula': 'La1 Fe1 O3', 'id': 'La1 Fe1 O3', 'training': 1, 'target': -1.5, 'anon_formula': 'ABC3', "
        "'electronegativity': 2.65, 'cif': 'out/cifs/La1 Fe1 O3.cif', 'sample': 10, 'natoms': 5, 'min_distance': 2.0, "
        "'volume': 64.0}\"\"{'formula': 'La1 Fe1 O3', 'id': 'La1 Fe1 O3_1', 'training': 1, 'target': -1.5, "
        "'anon_formula': 'ABC3', 'electronegativity': 2.65, 'cif': 'out/cifs/La1 Fe1 O3_1.cif', 'sample': 13, 'natoms': 5, "
        "'min_distance': 2.0, 'volume': 64.0}\"\"{'formula': 'Si2', 'id': 'Si2', 'training': 0, 'target': -1.5, "
        "'anon_formula': 'A', 'electronegativity': 1.9, 'cif': 'out/cifs/Si2.cif', 'sample': 14, 'natoms': 2, "
        "'min_distance': 1.7320508075688772, 'volume': 64.0}\"")
CIF = ("data_LaFeO3\n_symmetry_space_group_name_H-M   'P 1'\n_cell_length_a   4.00000000\n_cell_length_b   4.00000000\n"
       "_cell_length_c   4.00000000\n_cell_angle_alpha   90.00000000\n_cell_angle_beta   90.00000000\n"
       "_cell_angle_gamma   90.00000000\n_symmetry_Int_Tables_number   1\n_chemical_formula_structural   LaFeO3\n"
       "_chemical_formula_sum   'La1 Fe1 O3'\n_cell_volume   64.00000000\n_cell_formula_units_Z   1\nloop_\n"
       " _symmetry_equiv_pos_site_id\n _symmetry_equiv_pos_as_xyz\n  1  'x, y, z'\nloop_\n _atom_site_type_symbol\n"
       " _atom_site_label\n _atom_site_symmetry_multiplicity\n _atom_site_fract_x\n _atom_site_fract_y\n"
       " _atom_site_fract_z\n _atom_site_occupancy\n  La  La0  1  0.06250000  0.06250000  0.06250000  1\n"
       "  Fe  Fe1  1  0.56250000  0.56250000  0.56250000  1\n  O  O2  1  0.56250000  0.56250000  0.06250000  1\n"
       "  O  O3  1  0.56250000  0.06250000  0.56250000  1\n  O  O4  1  0.06250000  0.56250000  0.56250000  1\n")


def _write(tmp_path, monkeypatch, **kw):
    monkeypatch.setattr(S, "screen", host_screen)
    monkeypatch.chdir(tmp_path)
    lp = np.tile([4.0, 4.0, 4.0], (len(ATOMS), 1))
    w = S.ResultsWriter("out", training_names={"LaFeO3"}, target_value=-1.5, **kw)
    w.add_batch(range(10, 13), lp[:3], ATOMS[:3])
    w.add_batch(range(13, 15), lp[3:], ATOMS[3:])
    return w, w.finish()


def test_results_writer_without_a_matcher_writes_what_it_wrote_before(tmp_path, monkeypatch):
    w, counts = _write(tmp_path, monkeypatch)
    assert counts == {"generated": 5, "failed": 1, "invalid": 1, "written": 3}
    assert S.ResultsWriter.COLUMNS == ("formula", "id", "training", "target", "anon_formula", "electronegativity", "cif",
                                       "sample", "natoms", "min_distance", "volume")
    assert open("out/results.csv", newline="").read().replace("\r\n", "\n") == CSV
    assert open("out/results.json").read() == JSON
    assert open("out/cifs/La1 Fe1 O3_1.cif").read() == CIF
    assert sorted(os.listdir("out/cifs")) == ["La1 Fe1 O3.cif", "La1 Fe1 O3_1.cif", "Si2.cif"] and w.match_summary is None


def test_results_writer_with_a_matcher_adds_columns_and_counts(tmp_path, monkeypatch):
    seen = []

    def matcher(structs):                      # stands in for Matcher: the second perovskite repeats the first
        seen.append(len(structs))
        out = [{"duplicate_of": -1, "duplicate_rms": None, "training_match": None, "training_rms": None, "match_reason": 0}
               for _ in structs]
        out[0].update(training_match="mp-19", training_rms=0.03125)
        out[1].update(duplicate_of=0, duplicate_rms=0.0625, training_match="mp-19", training_rms=0.0625)
        out[2]["match_reason"] = S.INELIGIBLE_CLOSE | S.INELIGIBLE_THIN
        return out

    w, counts = _write(tmp_path, monkeypatch, matcher=matcher)
    assert seen == [3]                                                     # once, over the whole run, in finish()
    assert counts == {"generated": 5, "failed": 1, "invalid": 1, "written": 3, "unique": 1, "novel": 0, "ineligible": 1}
    assert w.match_summary == {"unique": 1, "novel": 0, "ineligible": 1,
                               "ineligible_by_reason": {"atoms within 4 tol": 1, "cell too thin for tol": 1}}
    text = open("out/results.csv", newline="").read().replace("\r\n", "\n").splitlines()
    old = CSV.splitlines()
    assert text[0] == old[0] + ",duplicate_of,duplicate_rms,training_match,training_rms,match_reason"
    assert text[1] == old[1] + ",,,mp-19,0.03125,"
    assert text[2] == old[2] + ",La1 Fe1 O3,0.0625,mp-19,0.0625,"
    assert text[3] == old[3] + ',,,,,"atoms within 4 tol, cell too thin for tol"'
    assert open("out/results.json").read() == JSON and open("out/cifs/La1 Fe1 O3_1.cif").read() == CIF
    rows = list(csv.DictReader(open("out/results.csv")))
    assert [r["duplicate_of"] for r in rows] == ["", "La1 Fe1 O3", ""]
    with pytest.raises(ValueError):
        S.Matcher(tol=0.0)
    with pytest.raises(ValueError):
        S.Matcher(ops_mode=4)
