"""ics_op_structure_symmetry on the device against the brute-force restatement.

Integers -- counts, codes, anchors, orbits, multiplicities, reason bits, rotation types -- must be EQUAL.  op_rms,
sym_shift, sym_resid, op_t (modulo 1, measured with M), sym_frac (measured with M) within 1e-9 Angstrom and sym_G within
1e-9 relative: fp64 sums of at most 256 x 192 terms of order 1 round at ~1e-12.  Every comparison prints its worst gap.
Worst gaps observed on an MI355X: op_t 1.8e-15, op_rms 1.4e-17, sym_frac 6.2e-16, sym_shift 5.2e-16, sym_resid 1.5e-15
Angstrom, sym_G 0."""
import os
import subprocess
import sys

import numpy as np
import pytest

import structure_symmetry_cases as C
import structure_symmetry_ref as MR
from icsg3d_amd import _lib as L
from icsg3d_amd import structures as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, LTOL = C.TOL, C.LTOL
INT_KEYS = ("n_lat", "n_ops", "n_point", "n_trans", "types", "reason", "op_code", "op_anchor", "orbit", "mult")
KEYS = INT_KEYS + ("op_t", "op_rms", "sym_frac", "sym_G", "sym_shift", "sym_resid")
BOUND = 1e-9


def run(structs, eligible=None, tol=TOL, ltol=LTOL, max_ops=192):
    off, sp, fr, lat = C.pack(structs)
    el = np.ones(len(structs), np.int32) if eligible is None else np.asarray(eligible, np.int32)
    return S.symmetry_packed(off, sp, fr, lat, el, tol, ltol, max_ops)


def compare(o, r, structs, what=""):
    """Device `o` against restatement `r`: integers equal, floats within BOUND; returns the worst gaps."""
    for k in INT_KEYS:
        assert np.array_equal(np.asarray(o[k]), np.asarray(r[k])), (what, k, np.asarray(o[k]).tolist()[:40], np.asarray(r[k]).tolist()[:40])
    off = np.zeros(len(structs) + 1, np.int64)
    off[1:] = np.cumsum([len(s[0]) for s in structs])
    gap = {"op_t": 0.0, "op_rms": 0.0, "sym_frac": 0.0, "sym_G": 0.0, "sym_shift": 0.0, "sym_resid": 0.0}
    for s, (Z, f, M) in enumerate(structs):
        keep = min(int(r["n_ops"][s]), o["op_code"].shape[1])
        assert np.all(np.isnan(o["op_rms"][s, keep:])) and np.all(np.isnan(o["op_t"][s, keep:]))
        if keep:
            d = o["op_t"][s, :keep] - r["op_t"][s, :keep]
            d -= np.rint(d)
            gap["op_t"] = max(gap["op_t"], float(np.sqrt(((d @ M) ** 2).sum(1)).max()))
            gap["op_rms"] = max(gap["op_rms"], float(np.abs(o["op_rms"][s, :keep] - r["op_rms"][s, :keep]).max()))
        d = o["sym_frac"][off[s]:off[s + 1]] - r["sym_frac"][off[s]:off[s + 1]]
        if len(d):
            gap["sym_frac"] = max(gap["sym_frac"], float(np.sqrt(((d @ np.asarray(M).reshape(3, 3)) ** 2).sum(1)).max()))
        g = np.abs(o["sym_G"][s] - r["sym_G"][s]).max() / np.abs(r["sym_G"][s]).max()
        gap["sym_G"] = max(gap["sym_G"], float(g))
    gap["sym_shift"] = float(np.abs(o["sym_shift"] - r["sym_shift"]).max())
    gap["sym_resid"] = float(np.abs(o["sym_resid"] - r["sym_resid"]).max())
    print(what, "worst gaps:", " ".join("%s %.2e" % kv for kv in gap.items()))
    assert all(np.isfinite(v) and v <= BOUND for v in gap.values()), (what, gap)
    return gap


@pytest.fixture(scope="module")
def base():
    return C.base_cases()


@pytest.fixture(scope="module")
def named(base):
    """The seven cases and their noisy, shifted versions with the restatement's answer (computed once)."""
    rng = np.random.default_rng(21)
    structs = [base[n] for n in C.NAMES] + [C.noisy(rng, base[n], 0.3) for n in C.NAMES]
    return structs, MR.symmetry_ref(structs, None, TOL, LTOL, 192)


@pytest.fixture(scope="module")
def sized():
    """n = 1, 64, 65, 256: random P1 cells with a unique rarest atom."""
    rng = np.random.default_rng(22)
    M = C.lat([12.0, 13.0, 14.0])
    s64 = C.random_p1(rng, 64, M)
    structs = [C.random_p1(rng, 1, C.lat([4.0, 5.0, 6.0])), s64, C.add_atom(rng, s64), C.random_p1(rng, 256, C.lat([19.0, 20.0, 21.0]))]
    return structs, MR.symmetry_ref(structs, None, TOL, LTOL, 192)


@pytest.fixture(scope="module")
def supercells(base):
    p222 = C.supercell(base["perovskite"], (2, 2, 2))
    r442 = C.supercell(base["rocksalt"], (4, 4, 2))
    return p222, MR.symmetry_ref([p222], None, TOL, LTOL, 384), r442, MR.symmetry_ref([r442], None, TOL, LTOL, 192)


def test_named_cases_and_their_noisy_versions_in_one_call(named):
    structs, r = named
    o = run(structs)
    compare(o, r, structs, "named")
    for k, n in enumerate(C.NAMES * 2):
        pg = S.POINT_GROUPS[tuple(int(v) for v in o["types"][k])][0]
        assert (o["n_ops"][k], o["n_point"][k], o["n_trans"][k], pg) == C.EXPECT[n] and o["reason"][k] == 0
    assert o["n_lat"][C.NAMES.index("tetragonal")] == 16
    assert np.all(o["sym_shift"] <= TOL) and np.all(o["sym_resid"] <= BOUND)


def test_atom_counts_on_both_sides_of_the_wave_workgroup_boundary(sized):
    structs, r = sized
    assert [len(s[0]) for s in structs] == [1, 64, 65, 256]
    assert r["n_lat"].tolist() == [8, 8, 8, 8] and r["n_ops"].tolist() == [8, 1, 1, 1]     # one atom: every W passes
    o = run(structs)
    compare(o, r, structs, "sizes")


def _raw(structs, eligible, sentinel=-7):
    """The C entry point with output buffers pre-filled with a sentinel: (rc, buffers)."""
    off, sp, fr, lat = C.pack(structs)
    ns, N, mo = len(structs), len(sp), 4
    lat = np.ascontiguousarray(lat.reshape(ns, 9))
    el = np.asarray(eligible, np.int32)
    ib = {k: np.full(shape, sentinel, np.int32) for k, shape in (("n_lat", ns), ("n_ops", ns), ("n_point", ns), ("n_trans", ns),
          ("types", (ns, 10)), ("reason", ns), ("op_code", (ns, mo)), ("op_anchor", (ns, mo)), ("orbit", N), ("mult", N))}
    db = {k: np.full(shape, float(sentinel)) for k, shape in (("op_t", (ns, mo, 3)), ("op_rms", (ns, mo)), ("sym_frac", (N, 3)),
          ("sym_G", (ns, 9)), ("sym_shift", ns), ("sym_resid", ns))}
    rc = L.load().ics_op_structure_symmetry(
        L.i32ptr(off), L.i32ptr(sp), L.f64ptr(fr), L.f64ptr(lat), L.i32ptr(el), ns, TOL, LTOL, mo, L.i32ptr(ib["n_lat"]),
        L.i32ptr(ib["n_ops"]), L.i32ptr(ib["n_point"]), L.i32ptr(ib["n_trans"]), L.i32ptr(ib["types"]), L.i32ptr(ib["reason"]),
        L.i32ptr(ib["op_code"]), L.i32ptr(ib["op_anchor"]), L.f64ptr(db["op_t"]), L.f64ptr(db["op_rms"]), L.i32ptr(ib["orbit"]),
        L.i32ptr(ib["mult"]), L.f64ptr(db["sym_frac"]), L.f64ptr(db["sym_G"]), L.f64ptr(db["sym_shift"]), L.f64ptr(db["sym_resid"]))
    return rc, {**ib, **db}


def test_257_atoms_refused_by_name_or_neutral_when_ineligible(base):
    rng = np.random.default_rng(23)
    big = C.random_p1(rng, 257, C.lat([19.0, 20.0, 21.0]))
    structs = [base["perovskite"], big]
    rc, b = _raw(structs, [1, 1])
    msg = L.load().ics_last_error().decode()
    assert rc != 0 and "eligible structure 1" in msg and "257" in msg, msg
    for k, v in b.items():
        assert np.all(v == -7), k                                   # nothing written
    rc, b = _raw(structs, [1, 0])
    assert rc == 0
    assert b["reason"].tolist() == [4, 1] and b["n_ops"].tolist() == [48, 0] and b["n_lat"].tolist() == [48, 0]
    assert np.array_equal(b["orbit"][5:], np.arange(257)) and np.all(b["mult"][5:] == 1)
    f = big[1] - np.floor(big[1])
    assert np.array_equal(b["sym_frac"][5:], f) and np.all(b["op_code"][1] == -1) and np.all(np.isnan(b["op_t"][1]))
    np.testing.assert_allclose(b["sym_G"][1].reshape(3, 3), big[2] @ big[2].T, rtol=1e-15)
    assert b["sym_shift"][1] == 0 and b["sym_resid"][1] == 0 and np.all(b["types"][1] == 0)
    for bad in (dict(tol=0.0), dict(ltol=float("nan")), dict(max_ops=0), dict(max_ops=4097), dict(tol=1.5)):
        with pytest.raises(Exception):
            run([base["perovskite"]], **bad)


def test_capacity_of_the_operation_lists(supercells):
    p222, rp, r442, rr = supercells
    assert len(p222[0]) == 40 and rp["n_ops"][0] == 384 and rp["reason"][0] == 0
    full = run([p222], max_ops=384)
    compare(full, rp, [p222], "2x2x2 perovskite, max_ops 384")
    assert full["n_point"][0] == 48 and full["n_trans"][0] == 8 and full["mult"].max() == 24
    cut = run([p222], max_ops=383)
    assert cut["reason"][0] == 4 and cut["n_ops"][0] == 384 and cut["n_point"][0] == 48 and cut["n_trans"][0] == 8
    for k in ("op_code", "op_anchor", "op_t", "op_rms"):
        assert cut[k][0].tobytes() == full[k][0][:383].tobytes(), k
    assert np.array_equal(cut["types"], full["types"]) and np.array_equal(cut["orbit"], np.arange(40))
    assert len(r442[0]) == 256 and rr["n_ops"][0] == 2048 and rr["reason"][0] == 4
    o = run([r442], max_ops=192)
    compare(o, rr, [r442], "4x4x2 rock salt, max_ops 192")
    assert (o["n_lat"][0], o["n_point"][0], o["n_trans"][0]) == (16, 16, 128)


def test_lattice_operation_overflow(base):
    s = [base["triclinic"], base["perovskite"]]
    r = MR.symmetry_ref(s, None, TOL, 10.0, 192)
    assert r["reason"].tolist() == [2, 2] and r["n_lat"].tolist() == [6960, 6960]
    compare(run(s, ltol=10.0), r, s, "ltol 10")


def mixed(base):
    """Everything above in shuffled order, with one ineligible entry."""
    rng = np.random.default_rng(24)
    structs = [base[n] for n in C.NAMES] + [C.noisy(rng, base[n], 0.3) for n in C.NAMES]
    M = C.lat([12.0, 13.0, 14.0])
    s64 = C.random_p1(rng, 64, M)
    structs += [s64, C.add_atom(rng, s64), C.random_p1(rng, 256, C.lat([19.0, 20.0, 21.0])),
                C.supercell(base["perovskite"], (2, 2, 2)), C.supercell(base["rocksalt"], (4, 4, 2)),
                C.supercell(base["rocksalt"], (2, 2, 2)), C.noisy(rng, base["perovskite"], 0.75, shift=False)]
    structs += [C.noisy(rng, base[n], 0.2) for n in C.NAMES]
    order = rng.permutation(len(structs))
    structs = [structs[k] for k in order]
    el = np.ones(len(structs), np.int32)
    el[3] = 0
    return structs, el


def chunk_worker(path):
    """Run in a fresh process with ICSG3D_SYMMETRY_CHUNK_BYTES set (it is read once per process)."""
    structs, el = mixed(C.base_cases())
    o = run(structs, el)
    np.savez(path, **o)
    print("chunked run written")


def test_mixed_batch_chunked_unchunked_and_twice_the_same_bits(base, tmp_path):
    """A chunk holds at most cap / (192 x 44 bytes of operation lists) = 7 structures at a cap of 60 000 bytes and the
    batch has 28 eligible ones in two kernel kinds: at least five chunks.  The restatement is not needed here: the
    structures are those of the other tests; what is checked is that no bit depends on the chunking or the run."""
    structs, el = mixed(base)
    assert len(structs) == 28 and el.sum() == 27
    a, b = run(structs, el), run(structs, el)
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["reason"][3] == 1 and set(a["reason"].tolist()) >= {0, 1, 4}
    path = str(tmp_path / "chunked.npz")
    env = dict(os.environ, ICSG3D_SYMMETRY_CHUNK_BYTES="60000", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", "import test_gpu_structure_symmetry as T; T.chunk_worker(%r)" % path], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "chunked run written" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
    c = np.load(path)
    for k in KEYS:
        assert a[k].tobytes() == c[k].tobytes(), k


def test_sweep_robust_on_the_restatement_then_equal():
    """84 structures.  First, on the restatement alone: which structures keep their operation list -- the same (code,
    anchor) pairs -- when tol and ltol are scaled by 0.95 and 1.05; every noise-free one must (its residuals are rounding
    or lattice-sized).  Then the device equals the restatement on every structure that does, integers exactly."""
    sw = C.sweep()
    structs = [s for _, _, s in sw]
    r = MR.symmetry_ref(structs, None, TOL, LTOL, 192)
    def op_list(S_, tol, ltol):
        ops = MR.all_operations(S_[0], S_[1], S_[2], tol, ltol)[2]
        return None if ops is None else [(o["code"], o["anchor"]) for o in ops]
    keys = []
    for sc in (0.95, 1.05):
        keys.append([op_list(structs[k], TOL * sc, LTOL * sc) == list(zip(r["op_code"][k][:r["n_ops"][k]].tolist(),
                                                                           r["op_anchor"][k][:r["n_ops"][k]].tolist()))
                     for k in range(len(structs))])
    robust = np.array(keys[0]) & np.array(keys[1])
    print("robust %d of %d; by noise level: %s" % (robust.sum(), len(structs),
          {lvl: int(sum(robust[k] for k in range(len(sw)) if sw[k][1] == lvl)) for lvl in (0.0, 0.2, 0.4)}))
    assert all(robust[k] for k in range(len(sw)) if sw[k][1] == 0.0)
    assert robust.sum() >= 56                          # the noise-free and the 0.2 tol ones: 0.2 tol is far from both limits
    o = run(structs)
    idx = np.where(robust)[0]
    off = np.zeros(len(structs) + 1, np.int64)
    off[1:] = np.cumsum([len(s[0]) for s in structs])
    atoms = np.concatenate([np.arange(off[k], off[k + 1]) for k in idx])
    sub = lambda d: {k: (d[k][atoms] if k in ("orbit", "mult", "sym_frac") else d[k][idx]) for k in KEYS}
    compare(sub(o), sub(r), [structs[k] for k in idx], "sweep")
    for k in idx:
        if r["reason"][k] == 0:
            name = sw[k][0]
            pg = S.POINT_GROUPS[tuple(int(v) for v in o["types"][k])][0]
            assert (o["n_ops"][k], pg) == (C.EXPECT[name][0], C.EXPECT[name][3]) or sw[k][1] > 0


def test_symmetry_and_results_writer_on_the_device(base, tmp_path):
    """The public path: symmetry() over screen-shaped dicts, and ResultsWriter(symmetriser=...) from atom lists."""
    rng = np.random.default_rng(25)
    near = C.noisy(rng, base["perovskite"], 0.75, shift=False)
    out = S.symmetry([C.as_result(base["hcp"]), None, C.as_result(near), C.as_result(base["rocksalt"])], TOL, LTOL)
    assert out[0]["point_group"] == "6/mmm" and out[1]["sym_reason"] == S.SYM_NOT_ELIGIBLE
    assert out[2]["sym_reason"] == 0 and out[2]["tol_used"] <= TOL
    assert out[3]["point_group"] == "m-3m" and out[3]["n_centring"] == 4 and len(out[3]["ops"]) == 192
    Z, f, M = base["perovskite"]
    Z2, f2, M2 = C.noisy(rng, base["rocksalt"], 0.3)
    atoms = [(Z, f * 3.9 + 0.01 * rng.normal(size=f.shape)), (Z2, (f2 - np.floor(f2)) * 5.6), ([8, 8], np.array([[1.0, 1, 1], [1.2, 1, 1]]))]
    w = S.ResultsWriter(str(tmp_path), symmetriser=S.Symmetriser(TOL, LTOL))
    w.add_batch(range(3), np.array([[3.9] * 3, [5.6] * 3, [4.0] * 3]), atoms)
    counts = w.finish()
    print(counts, w.symmetry_summary)
    assert counts == {"generated": 3, "failed": 0, "invalid": 1, "written": 2, "symmetrised": 2}
    assert w.symmetry_summary == {"symmetrised": 2, "by_point_group": {"m-3m": 2}, "by_crystal_system": {"cubic": 2}}
    head = open(tmp_path / "results.csv").readline().strip().split(",")
    assert tuple(head[1:]) == S.ResultsWriter.COLUMNS + S.ResultsWriter.SYMMETRY_COLUMNS
    for name in os.listdir(tmp_path / "cifs_sym"):
        d = S.read_cif_symmetry(str(tmp_path / "cifs_sym" / name))
        z, ff = S.expand_symmetry(d["species"], d["frac"], d["ops"])
        assert len(z) == len(S.read_cif(str(tmp_path / "cifs" / name))["species"]) and d["point_group"] == "m-3m"
