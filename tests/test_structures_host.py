"""generate.py's structure stage without a GPU: the fp64 restatement tests/structure_ref.py (what the GPU tests hold
ics_op_structure_screen to) against hand-derived cases, and the host side of icsg3d_amd.structures: formulas, the CIF
writer / reader, the duplicate numbering."""
import ctypes
import math

import numpy as np
import pytest

import structure_ref as R
from icsg3d_amd import structures as S


def _hist(**amounts):
    h = np.zeros(S.HIST, np.int32)
    for sym, n in amounts.items():
        h[S.SYMBOLS.index(sym)] = n
    return h


def test_restatement_on_hand_derived_distances():
    # cubic a = 4, atoms at the corner and the body centre: half the body diagonal
    r = R.screen_ref([26, 26], [[0, 0, 0], [2, 2, 2]], [4, 4, 4], [90, 90, 90])
    assert abs(r["min_dist"] - 2 * math.sqrt(3)) < 1e-14 and r["min_pair"] == (0, 1) and r["valid"] == 1
    # a = 10, x = 0.5 and 9.5: 1 Angstrom through the boundary, not 9 inside the cell
    r = R.screen_ref([8, 8], [[0.5, 1, 1], [9.5, 1, 1]], [10, 10, 10], [90, 90, 90])
    assert abs(r["min_dist"] - 1.0) < 1e-14 and r["n_close"] == 0 and r["valid"] == 1
    r = R.screen_ref([8, 8], [[0.2, 1, 1], [9.9, 1, 1]], [10, 10, 10], [90, 90, 90])
    assert abs(r["min_dist"] - 0.3) < 1e-14 and r["n_close"] == 1 and r["valid"] == 0 and r["reason"] == 1
    # gamma = 120, a = 2, b = 12: va = (2, 0, 0), vb = (-6, 6 sqrt 3, 0).  Atoms at frac (0, 0, 0) and (7/8, 5/8, 0): the
    # translation (-2, -1, 0) gives x = 2 (7/8 - 2) - 6 (5/8 - 1) = 0, y = 6 sqrt 3 (5/8 - 1): d = 2.25 sqrt 3.  That image
    # is outside the 27-neighbour set, whose best is larger
    M = R.lattice_from_parameters(2, 12, 5, 90, 90, 120)
    np.testing.assert_allclose(M, [[2, 0, 0], [-6, 6 * math.sqrt(3), 0], [0, 0, 5]], atol=1e-14)
    f = np.array([[0, 0, 0], [0.875, 0.625, 0]])
    r = R.screen_ref([8, 8], f * [2, 12, 5], [2, 12, 5], [90, 90, 120])
    assert abs(r["min_dist"] - 2.25 * math.sqrt(3)) < 1e-13
    assert R.pair_distances_27(f, M)[0, 1] > r["min_dist"] + 0.4
    # +-4 images change nothing against +-6 here
    assert R.pair_distances(f, M, 6)[0, 1] == R.pair_distances(f, M, 4)[0, 1]


def test_restatement_edge_cases():
    r = R.screen_ref([], np.zeros((0, 3)), [4, 4, 4], [90, 90, 90])
    assert r["valid"] == 0 and r["reason"] == 4 and r["min_pair"] == (-1, -1) and np.isinf(r["min_dist"])
    r = R.screen_ref([3], [[1, 1, 1]], [4, 4, 4], [90, 90, 90])
    assert r["valid"] == 1 and r["reason"] == 0 and np.isinf(r["nearest"][0]) and r["hist"][3] == 1
    r = R.screen_ref([0, 95, 8], [[0, 0, 0], [2, 2, 2], [1, 3, 1]], [4, 4, 4], [90, 90, 90])
    assert r["valid"] == 0 and r["reason"] == 2 and r["hist"].sum() == 1
    r = R.screen_ref([8, 8], [[1, 1, 1], [1, 1, 1]], [4, 4, 4], [90, 90, 90])
    assert r["min_dist"] == 0.0 and r["valid"] == 0 and r["n_close"] == 1
    # ties go to the lexicographically smallest pair: three atoms in a row, equal spacing
    r = R.screen_ref([8, 8, 8], [[0, 0, 0], [1, 0, 0], [2, 0, 0]], [8, 8, 8], [90, 90, 90])
    assert r["min_pair"] == (0, 1) and r["min_dist"] == 1.0 and list(r["nearest"]) == [1.0, 1.0, 1.0]


def test_lattice_formula_recovers_the_six_parameters():
    rng = np.random.RandomState(3)
    for _ in range(50):
        p = list(rng.uniform(3, 12, 3)) + list(rng.randint(60, 121, 3).astype(float))
        M = R.lattice_from_parameters(*p)
        if np.linalg.det(M) < 0.3 * p[0] * p[1] * p[2]:
            continue
        np.testing.assert_allclose(R.lattice_parameters(M), p, rtol=1e-12)
        # the package's host copy of the cell (used for the per-sample skew rule) is the same lattice
        M2, vol, g = S.cell(p[:3], p[3:])
        np.testing.assert_allclose(M2, M, rtol=0, atol=1e-13 * max(p[:3]))
        np.testing.assert_allclose(vol, np.linalg.det(M), rtol=1e-13)
        np.testing.assert_allclose(g, np.linalg.norm(np.linalg.inv(M), axis=0), rtol=1e-12)
    M = R.lattice_from_parameters(4, 5, 6, 90, 90, 90)
    np.testing.assert_allclose(M, np.diag([4.0, 5.0, 6.0]), rtol=0, atol=1e-15)     # cos(arccos(0)) is 6e-17, not 0
    for bad in ([90, 90, 180], [60, 60, 120], [10, 100, 150], [0, 90, 90]):
        with pytest.raises(ValueError):
            S.cell([4, 4, 4], bad)


def test_formulas():
    h = _hist(La=1, Fe=1, O=3)
    assert S.formula(h) == "La1 Fe1 O3" and S.reduced_formula(h) == "LaFeO3" and S.anonymized_formula(h) == "ABC3"
    assert abs(S.average_electroneg(h) - (1.10 + 1.83 + 3 * 3.44) / 5) < 1e-12
    h2 = _hist(La=2, Fe=2, O=6)                    # the doubled cell
    assert S.formula(h2) == "La2 Fe2 O6" and S.reduced_formula(h2) == "LaFeO3" and S.anonymized_formula(h2) == "ABC3"
    assert abs(S.average_electroneg(h2) - S.average_electroneg(h)) < 1e-12
    h3 = _hist(Ar=1, O=2, He=4, Na=2)              # no electronegativity: last, by Z (He before Ar)
    assert S.formula(h3) == "Na2 O2 He4 Ar1" and S.reduced_formula(h3) == "Na2O2He4Ar"
    assert S.anonymized_formula(h3) == "AB2C2D4" and math.isnan(S.average_electroneg(h3))
    assert S.formula(_hist(Si=4)) == "Si4" and S.reduced_formula(_hist(Si=4)) == "Si" and S.anonymized_formula(_hist(Si=4)) == "A"
    z = np.zeros(S.HIST, np.int32)
    assert S.formula(z) == "" and S.reduced_formula(z) == "" and math.isnan(S.average_electroneg(z))
    assert S.SYMBOLS[26] == "Fe" and S.SYMBOLS[57] == "La" and S.SYMBOLS[94] == "Pu" and S.SYMBOLS[8] == "O"


def test_duplicate_numbering():
    seen, ids = [], []
    for f in ["La1 Fe1 O3", "La1 O3", "La1 Fe1 O3", "La1 Fe1 O3", "La1 O3"]:
        ids.append(S.numbered(f, seen))
        seen.append(f)
    assert ids == ["La1 Fe1 O3", "La1 O3", "La1 Fe1 O3_1", "La1 Fe1 O3_2", "La1 O3_1"]


def test_cif_round_trip(tmp_path):
    rng = np.random.RandomState(1)
    species = np.array([57, 26, 8, 8, 8, 18])
    frac = rng.uniform(-0.1, 1.1, (6, 3))
    abc, angles = np.array([3.912345678, 5.5, 7.123456789012]), np.array([90.0, 101.0, 120.0])
    M = R.lattice_from_parameters(*abc, *angles)
    path = str(tmp_path / "x.cif")
    S.write_cif(path, abc, angles, species, frac, volume=np.linalg.det(M))
    text = open(path).read()
    assert text.startswith("data_LaFeO3Ar\n")
    for tag in ("_cell_length_a", "_cell_length_b", "_cell_length_c", "_cell_angle_alpha", "_cell_angle_beta",
                "_cell_angle_gamma", "_cell_volume", "_symmetry_space_group_name_H-M   'P 1'",
                "_chemical_formula_sum   'La1 Fe1 O3 Ar1'", "_cell_formula_units_Z   1", "'x, y, z'", "  La  La0  1  ",
                "  O  O4  1  ", "_atom_site_occupancy"):
        assert tag in text, tag
    c = S.read_cif(path)
    np.testing.assert_allclose(c["abc"], abc, atol=1e-8, rtol=0)
    np.testing.assert_allclose(c["angles"], angles, atol=1e-8, rtol=0)
    np.testing.assert_allclose(c["frac"], frac, atol=1e-8, rtol=0)
    np.testing.assert_allclose(c["volume"], np.linalg.det(M), atol=1e-7, rtol=0)
    assert np.array_equal(c["species"], species) and c["labels"][3] == "O3" and c["formula_sum"] == "La1 Fe1 O3 Ar1"
    # the volume written without one passed in is the cell's
    S.write_cif(path, abc, angles, species, frac)
    np.testing.assert_allclose(S.read_cif(path)["volume"], np.linalg.det(M), atol=1e-7, rtol=0)
    with pytest.raises(ValueError):
        S.write_cif(path, abc, angles, [0, 8], frac[:2])


def test_screen_entry_point_refuses_null_outputs():
    """The output-pointer rules of ics_op_structure_screen, refused before any device call."""
    from icsg3d_amd import _lib as L
    lib = L.load()
    off, sp = np.array([0, 2], np.int32), np.array([8, 8], np.int32)
    xyz, abc, ang = np.array([[0.0, 0, 0], [2.0, 2, 2]]), np.array([[4.0, 4, 4]]), np.array([[90.0, 90, 90]])

    def call(null):
        outs = {"lattice": np.zeros(9), "volume": np.zeros(1), "frac": np.zeros(6), "min_dist": np.zeros(1),
                "min_pair": np.zeros(2, np.int32), "n_close": np.zeros(1, np.int32), "valid": np.zeros(1, np.int32),
                "reason": np.zeros(1, np.int32), "nearest": np.zeros(2), "hist": np.zeros(95, np.int32)}
        ptr = [None if k == null else (L.f64ptr(a) if a.dtype == np.float64 else L.i32ptr(a)) for k, a in outs.items()]
        rc = lib.ics_op_structure_screen(L.i32ptr(off), L.i32ptr(sp), L.f64ptr(xyz), L.f64ptr(abc), L.f64ptr(ang), 1,
                                         ctypes.c_double(0.5), *ptr)
        return rc, (lib.ics_last_error() or b"").decode()

    for null in ("lattice", "volume", "min_dist", "min_pair", "n_close", "valid", "reason", "hist"):
        rc, msg = call(null)
        assert rc != 0 and msg.startswith("ics_op_structure_screen: null output ("), (null, msg)
    for null in ("frac", "nearest"):
        rc, msg = call(null)
        assert rc != 0 and msg.startswith("ics_op_structure_screen: null frac or nearest ("), (null, msg)
