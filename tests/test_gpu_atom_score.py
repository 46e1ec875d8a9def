"""The atom score on the device: atom_score_kernel against the brute-force restatement in
tests/atom_score_ref.py -- through ics_op_atom_score, through ics_op_atom_score_volumes with ics_op_segment_atoms as
the source of the atoms, and through the engine's accumulator with the engine's own predict_labels -- and eval_unet.py
--atoms on top of it.

Every tally is an integer, every match an index and every distance sum a serial fp64 sum in a fixed order: every
comparison is array_equal, and no tolerance appears in this file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import atom_score_cases as AC
import atom_score_ref as AR
import confusion_cases as CC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TALLIES = ("matrix", "dist_q", "dist2_q", "dup", "shadowed", "hist", "totals")


def _equal_tallies(got, want):
    for k in TALLIES:
        assert got[k].dtype == np.int64
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def _check_op(T, TS, P, PS, ncls, tol):
    from icsg3d_amd.atomscore import score
    want, matches, stats, sums = AR.score_batch(T, TS, P, PS, ncls, tol)
    got = score(T, TS, P, PS, ncls, tol, per_sample=True)
    _equal_tallies(got, want)
    for b in range(len(T)):
        np.testing.assert_array_equal(got["match"][b], matches[b], err_msg="sample %d" % b)
    np.testing.assert_array_equal(got["sample_stats"], stats)
    np.testing.assert_array_equal(got["dist_sum"].view(np.uint64), sums.view(np.uint64))       # the same fp64 bits
    lean = score(T, TS, P, PS, ncls, tol)                               # without the per-sample outputs: the same tallies
    _equal_tallies(lean, want)
    assert want["totals"][0] == len(T) and want["matrix"].sum() == want["totals"][3] + want["totals"][4] - want["totals"][5]
    return want


# ----------------------------------------------------------------------------------------------------------------------
# 1. ics_op_atom_score against the restatement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncls", [2, 17, 127])
@pytest.mark.parametrize("kind", ["generic", "lattice"])
def test_op_equals_restatement(kind, ncls):
    T, TS, P, PS = AC.batch(kind, AC.SIZE_PAIRS, ncls, seed=ncls + (kind == "lattice"))
    want = _check_op(T, TS, P, PS, ncls, 1.5)
    assert want["totals"][5] > 1000 and want["matrix"][:ncls, ncls].sum() > 100 and want["matrix"][ncls, :ncls].sum() > 100
    assert want["dup"].sum() > 10 and want["shadowed"].sum() > 10 and (PS[-1] == 0).sum() > 10
    if kind == "lattice":
        assert want["hist"][0] > 100 and want["dist_q"].sum() > 0      # coincident points matched at distance 0, others not


def test_ragged_batch_crosses_workgroups_and_a_chunk():
    from icsg3d_amd.atomscore import limits
    threads, max_atoms, chunk_samples, chunk_atoms = limits()
    assert threads == 256 and max_atoms == 1024 and chunk_samples >= 70
    rng = np.random.default_rng(70)
    pairs = [(int(rng.integers(0, 700)), int(rng.integers(0, 700))) for _ in range(70)]
    assert sum(n + m for n, m in pairs) > chunk_atoms                   # more than one launch
    T, TS, P, PS = AC.batch("generic", pairs, 17, seed=71)
    _check_op(T, TS, P, PS, 17, 1.5)


def test_strictness():
    t, p = [np.zeros((1, 3))], [np.array([[3.0, 4.0, 0.0]])]
    s = [np.array([1], np.int32)]
    want = _check_op(t, s, p, s, 2, 5.0)                                # d2 == tol2 exactly: not admissible
    assert want["totals"][5] == 0 and want["matrix"][1, 2] == 1 and want["matrix"][2, 1] == 1
    want = _check_op(t, s, p, s, 2, float(np.nextafter(5.0, 6.0)))
    assert want["totals"][5] == 1 and want["matrix"][1, 1] == 1 and want["hist"][15] == 1


def test_many_rounds():
    t, p = AC.chain(64)
    match, rounds = AR.mutual_best(t, p, 1.5 * 1.5)
    assert rounds == 64 and (match >= 0).all()                          # one pair a round: the loop runs to its bound
    np.testing.assert_array_equal(match, AR.greedy_sorted(t, p, 1.5 * 1.5))
    s = np.ones(64, np.int32)
    want = _check_op([t], [s], [p], [s], 3, 1.5)
    assert want["totals"][5] == 64 and want["totals"][2] == 1


def test_planted_dup_and_shadowed():
    one, two = np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0], [0.5, 0.0, 0.0]])
    s1, s2 = np.array([4], np.int32), np.array([4, 2], np.int32)
    want = _check_op([one, two], [s1, s2], [two, one], [s2, s1], 6, 2.0)
    assert want["dup"].tolist() == [0, 0, 0, 0, 1, 0] and want["shadowed"].tolist() == [0, 0, 0, 0, 1, 0]
    assert want["matrix"][4, 2] == 1 and want["matrix"][2, 4] == 1 and want["matrix"][6, 4] == 1 and want["matrix"][4, 6] == 1


def test_op_refusals():
    import ctypes as C
    from icsg3d_amd import _lib as L
    from icsg3d_amd.atomscore import empty_tallies, score
    lib = L.load()
    ncls = 5
    T, TS, P, PS = AC.batch("generic", [(3, 2), (0, 4), (5, 5)], ncls, seed=3)
    xyz_t, sp_t = np.concatenate(T), np.concatenate(TS)
    xyz_p, sp_p = np.concatenate(P), np.concatenate(PS)
    off_t, off_p = np.array([0, 3, 3, 8], np.int32), np.array([0, 2, 6, 11], np.int32)
    out = {k: np.full_like(v, -7) for k, v in empty_tallies(127).items()}
    match, stats, dsum = np.full(8, -7, np.int32), np.full((3, 6), -7, np.int32), np.full(3, -7.0)

    def call(**kw):
        a = dict(t_xyz=xyz_t, t_sp=sp_t, t_off=off_t, p_xyz=xyz_p, p_sp=sp_p, p_off=off_p, batch=3, ncls=ncls, tol=2.0,
                 **{k: out[k] for k in TALLIES})
        a.update(kw)
        rc = lib.ics_op_atom_score(L.f64ptr(a["t_xyz"]), L.i32ptr(a["t_sp"]), L.i32ptr(a["t_off"]), L.f64ptr(a["p_xyz"]),
                                   L.i32ptr(a["p_sp"]), L.i32ptr(a["p_off"]), a["batch"], a["ncls"], C.c_double(a["tol"]),
                                   *[L.i64ptr(a[k]) for k in TALLIES], L.i32ptr(match), L.i32ptr(stats), L.f64ptr(dsum))
        return rc, lib.ics_last_error().decode()

    def changed(a, at, value):
        b = a.copy()
        b.reshape(-1)[at] = value
        return b

    big = np.arange(0, 1026, 1025).astype(np.int32)                     # one sample of 1025 atoms
    calls = [("null", dict(t_off=None)), ("null", dict(p_off=None)), ("null", dict(t_xyz=None)), ("null", dict(p_sp=None)),
             ("batch", dict(batch=0)), ("num_classes", dict(ncls=1)), ("num_classes", dict(ncls=128)),
             ("tol", dict(tol=0.0)), ("tol", dict(tol=-1.0)), ("tol", dict(tol=float("nan"))), ("tol", dict(tol=float("inf"))),
             ("t_off[0]", dict(t_off=changed(off_t, 0, 1))), ("decreases at sample 1", dict(p_off=changed(off_p, 2, 1))),
             ("sample 0 has 1025 atoms in t", dict(t_off=big, t_xyz=np.zeros((1025, 3)), t_sp=np.zeros(1025, np.int32),
                                                   p_off=np.zeros(2, np.int32), batch=1)),
             ("sample 2 has a species", dict(t_sp=changed(sp_t, 4, ncls))), ("sample 0 has a species", dict(p_sp=changed(sp_p, 1, -1))),
             ("sample 2 has a non-finite", dict(p_xyz=changed(xyz_p, 3 * 7 + 1, np.nan))),
             ("sample 0 has a non-finite", dict(t_xyz=changed(xyz_t, 2, np.inf))),
             ("sample 1 has a non-finite", dict(p_xyz=changed(xyz_p, 3 * 2, 2e150)))]
    calls += [("null", {k: None}) for k in TALLIES]
    for word, kw in calls:
        rc, msg = call(**kw)
        assert rc != 0, word
        assert "ics_op_atom_score" in msg and word in msg, (word, msg)
    for a in list(out.values()) + [match, stats]:
        assert (a == -7).all()                                          # nothing was written by any refused call
    assert (dsum == -7.0).all()
    rc, msg = call()                                                    # ... and the same arrays are accepted unchanged
    assert rc == 0, msg
    want = AR.score_batch(T, TS, P, PS, ncls, 2.0)[0]
    np.testing.assert_array_equal(out["totals"][:8], want["totals"])
    with pytest.raises(ValueError):
        score(T, TS, P[:-1], PS[:-1], ncls)


# ----------------------------------------------------------------------------------------------------------------------
# 2. ics_op_atom_score_volumes against ics_op_segment_atoms + the restatement
# ----------------------------------------------------------------------------------------------------------------------
def _atoms_of_volumes(mask, species, d, min_voxels, max_atoms, ncls):
    """the existing op on the volumes (a grid below 16 in the corner of a zeroed 16^3 one) -> per sample (xyz, species),
    and failed (B,)"""
    from icsg3d_amd.watershed import segment_atoms
    if d < 16:
        big = np.zeros((mask.shape[0], 16, 16, 16), np.uint8)
        bm, bs = big.copy(), big.copy()
        bm[:, :d, :d, :d], bs[:, :d, :d, :d] = mask, species
        mask, species = bm, bs
    seg = segment_atoms(mask, species, min_voxels=min_voxels, max_atoms=max_atoms, num_species=ncls, want_regions=False)
    atoms = [AR.atoms_of_stats(seg["stats"][b, :seg["n_atoms"][b]]) for b in range(mask.shape[0])]
    return atoms, seg["failed"]


def _volumes_ref(lab, sp, mk, d, min_voxels, max_atoms, ncls, tol):
    pa, pf = _atoms_of_volumes(mk, sp, d, min_voxels, max_atoms, ncls)
    ta, tf = _atoms_of_volumes(lab, lab, d, 0, max_atoms, ncls)
    failed = pf | tf
    return AR.score_batch([a[0] for a in ta], [a[1] for a in ta], [a[0] for a in pa], [a[1] for a in pa], ncls, tol, failed), ta, pa


@pytest.mark.parametrize("d", [8, 16])
def test_volumes_with_planted_boxes(d):
    from icsg3d_amd.atomscore import score_volumes
    ncls, tol, max_atoms = 17, 2.0, 16
    lab, sp, mk = AC.volumes(d)
    (want, matches, stats, sums), ta, pa = _volumes_ref(lab, sp, mk, d, 3, max_atoms, ncls, tol)
    # what was planted, read off the restatement before the device is compared with it
    assert [len(a[1]) for a in ta] == [4, 3, 0] and [len(a[1]) for a in pa] == [5, 1, 0]
    M = want["matrix"]
    assert M[3, 3] == 1 and M[5, 5] == 1 and M[7, 9] == 1 and M[4, 4] == 1          # hit, shifted, wrong species, the nearer half
    assert M[ncls, 4] == 1 and want["dup"][4] == 1                                     # the other half: found twice
    assert M[6, 6] == 1 and M[8, ncls] == 1 and want["shadowed"][8] == 1              # bridged: one matched, one shadowed
    assert M[2, ncls] == 1 and want["shadowed"][2] == 0 and want["dup"].sum() == 1    # the small component: missed, not predicted
    assert want["totals"].tolist() == [3, 0, 1, 7, 6, 5, 3, 1] and want["dist_q"][5] == 1 << 20
    got = score_volumes(lab, sp, mk, ncls, tol, min_voxels=3, max_atoms=max_atoms, per_sample=True)
    _equal_tallies(got, want)
    for b in range(3):
        np.testing.assert_array_equal(got["match"][b, :len(matches[b])], matches[b])
        assert (got["match"][b, len(matches[b]):] == -1).all()
    np.testing.assert_array_equal(got["sample_stats"], stats)
    np.testing.assert_array_equal(got["dist_sum"].view(np.uint64), sums.view(np.uint64))
    _equal_tallies(score_volumes(lab, sp, mk, ncls, tol, min_voxels=3, max_atoms=max_atoms), want)


@pytest.mark.parametrize("d", [8, 16])
def test_volumes_failed_sample(d):
    from icsg3d_amd.atomscore import score_volumes
    ncls, tol = 17, 2.0
    lab, sp, mk = AC.volumes_failed(d)
    (want, matches, stats, sums), ta, pa = _volumes_ref(lab, sp, mk, d, 3, 2, ncls, tol)
    assert want["totals"].tolist() == [3, 1, 2, 1, 1, 1, 0, 1] and want["matrix"].sum() == 1 and want["matrix"][11, 11] == 1
    got = score_volumes(lab, sp, mk, ncls, tol, min_voxels=3, max_atoms=2, per_sample=True)
    _equal_tallies(got, want)
    assert got["sample_stats"][0].tolist() == [3, 3, -1, -1, -1, -1] and np.isnan(got["dist_sum"][0])
    assert (got["match"][0] == -1).all() and got["match"][2].tolist() == [0, -1]
    np.testing.assert_array_equal(got["sample_stats"][1:], stats[1:])
    whole = score_volumes(lab, sp, mk, ncls, tol, min_voxels=3, max_atoms=3)          # with room for it nothing fails
    assert whole["totals"].tolist() == [3, 0, 3, 4, 4, 4, 0, 1]


def test_volumes_refusals():
    from icsg3d_amd._lib import IcsError
    from icsg3d_amd.atomscore import score_volumes
    lab, sp, mk = AC.volumes(16)
    for word, kw in (("max_atoms", dict(max_atoms=1025)), ("max_atoms", dict(max_atoms=0)), ("min_voxels", dict(min_voxels=-1)),
                     ("num_classes", dict(num_classes=128)), ("tol", dict(tol=0.0))):
        a = dict(num_classes=17, tol=2.0, min_voxels=3, max_atoms=16)
        a.update(kw)
        with pytest.raises(IcsError, match="ics_op_atom_score_volumes.*" + word):
            score_volumes(lab, sp, mk, **a)
    with pytest.raises(IcsError, match="ics_op_atom_score_volumes.*power of two"):
        score_volumes(lab[:, :12, :12, :12], sp[:, :12, :12, :12], mk[:, :12, :12, :12], 17)
    with pytest.raises(ValueError):
        score_volumes(lab, sp[:2], mk, 17)


# ----------------------------------------------------------------------------------------------------------------------
# 3. the engine's accumulator
# ----------------------------------------------------------------------------------------------------------------------
NCLS, TOL, MIN_VOXELS, MAX_ATOMS = 17, 2.0, 3, 64
_engine_ref = {}


def _batch_ref(eng, a, b):
    """the restated tallies of samples [a, b) from the engine's own predict_labels + ics_op_segment_atoms; computed once"""
    if (a, b) not in _engine_ref:
        case = CC.engine_case(NCLS)
        sp, mk = eng.predict_labels(case["X"][a:b], CC.THRESH)
        sp, mk = sp.reshape(b - a, CC.D, CC.D, CC.D), mk.reshape(b - a, CC.D, CC.D, CC.D)
        lab = case["lab"][a:b].reshape(b - a, CC.D, CC.D, CC.D)
        (want, _, stats, _), ta, pa = _volumes_ref(lab, sp, mk, CC.D, MIN_VOXELS, MAX_ATOMS, NCLS, TOL)
        _engine_ref[(a, b)] = (want, stats, (sp, mk))
    return _engine_ref[(a, b)]


def test_engine_accumulator():
    from confusion_ref import confusion_ref
    from icsg3d_amd.atomscore import empty_tallies
    case = CC.engine_case(NCLS)
    X, lab = case["X"], case["lab"]
    eng = CC.make_engine(NCLS)
    refs = [_batch_ref(eng, a, b) for a, b in CC.BATCHES]
    # preconditions, before any comparison: the five samples hold atoms on both sides, matched and missed ones
    whole = refs[1][0]
    assert whole["totals"][4] >= 8 and whole["totals"][3] >= 20 and whole["totals"][5] >= 8, whole["totals"]
    assert whole["matrix"][:NCLS, NCLS].sum() >= 8 and whole["totals"][1] == 0
    eng.atom_score_open(TOL, MIN_VOXELS, MAX_ATOMS)
    _equal_tallies(eng.atom_score_read(), empty_tallies(NCLS))
    tot = AR.empty(NCLS)
    for (a, b), (want, _, _) in zip(CC.BATCHES, refs):
        tot = AR.add(tot, want)
        eng.atom_score_batch(X[a:b], lab[a:b], CC.THRESH)
        _equal_tallies(eng.atom_score_read(), tot)
    _equal_tallies(eng.atom_score_read(), tot)                           # read twice: the same, nothing reset
    assert tot["totals"][0] == 9
    # the step on a resident batch equals the batch call, and leaves the labels where a labels predict leaves them
    a, b = CC.BATCHES[0]
    eng.upload_batch(X[a:b], lab[a:b])
    eng.atom_score_step(CC.THRESH)
    _equal_tallies(eng.atom_score_read(), AR.add(tot, refs[0][0]))
    # with_confusion = 0 left no confusion accumulator behind; with_confusion = 1 adds what confusion_batch adds
    with pytest.raises(Exception, match="no open accumulator"):
        eng.confusion_read()
    eng.confusion_open()
    eng.confusion_batch(X[a:b], lab[a:b], CC.THRESH)
    alone = eng.confusion_read()
    m, o, _ = confusion_ref(lab[a:b], refs[0][2][0], refs[0][2][1], NCLS)
    np.testing.assert_array_equal(alone["matrix"], m)
    eng.atom_score_batch(X[a:b], lab[a:b], CC.THRESH, with_confusion=False)
    same = eng.confusion_read()
    np.testing.assert_array_equal(same["matrix"], m)                      # untouched
    assert same["voxels"] == alone["voxels"]
    eng.atom_score_batch(X[a:b], lab[a:b], CC.THRESH, with_confusion=True)
    both = eng.confusion_read()
    np.testing.assert_array_equal(both["matrix"], 2 * m)
    np.testing.assert_array_equal(both["occupancy"], 2 * o)
    assert both["voxels"] == 2 * alone["voxels"] and both["out_of_range"] == 0
    # a later open changes tol and min_voxels and zeroes; reset zeroes
    eng.atom_score_reset()
    _equal_tallies(eng.atom_score_read(), empty_tallies(NCLS))
    eng.atom_score_open(1.0, 0, MAX_ATOMS)
    eng.atom_score_step(CC.THRESH)
    sp, mk = refs[0][2]
    (want1, _, _, _), _, _ = _volumes_ref(lab[a:b].reshape(sp.shape), sp, mk, CC.D, 0, MAX_ATOMS, NCLS, 1.0)
    _equal_tallies(eng.atom_score_read(), want1)
    eng.close()


def test_engine_nothing_is_trained_and_guards_stay_clean(monkeypatch):
    monkeypatch.setenv("ICSG3D_DEBUG_CANARY", "1")
    case = CC.engine_case(NCLS)
    X, lab = case["X"][:3], case["lab"][:3]
    eng = CC.make_engine(NCLS)
    eng.set_class_weights(CC.K.weight_vector(NCLS))
    eng.train_step(X, lab)                                              # moving statistics and Adam moments worth comparing
    weights, (m, v, t), cw = eng.get_weights(), eng.get_optimizer_state(), eng.get_class_weights()
    assert eng.check_canaries()[0] == 0
    eng.confusion_open()
    eng.atom_score_open(TOL, MIN_VOXELS, MAX_ATOMS)
    for with_confusion in (False, True, True):
        eng.atom_score_batch(X, lab, CC.THRESH, with_confusion=with_confusion)
    eng.atom_score_step(CC.THRESH)
    r = eng.atom_score_read()
    assert r["totals"][0] == 12 and r["totals"][3] >= 12 and eng.confusion_read()["voxels"] == 2 * lab.size
    assert eng.check_canaries() == (0, "")
    after, (m2, v2, t2) = eng.get_weights(), eng.get_optimizer_state()
    assert sorted(after) == sorted(weights) and any(k.endswith("moving_variance") or k.endswith("var") for k in weights)
    for k in weights:
        np.testing.assert_array_equal(after[k], weights[k], err_msg=k)
    np.testing.assert_array_equal(m2, m); np.testing.assert_array_equal(v2, v)
    assert t2 == t
    np.testing.assert_array_equal(eng.get_class_weights(), cw)
    eng.close()


def test_engine_refusals():
    from icsg3d_amd import _lib as L
    from icsg3d_amd._lib import IcsError
    from icsg3d_amd.atomscore import empty_tallies
    from icsg3d_amd.engine import VaeEngine
    case = CC.engine_case(NCLS)
    X, lab = case["X"][:2], case["lab"][:2]
    eng = CC.make_engine(NCLS)
    lib = L.load()
    for name, call in (("ics_unet_atom_score_step", lambda: eng.atom_score_step()),
                       ("ics_unet_atom_score_batch", lambda: eng.atom_score_batch(X, lab)),
                       ("ics_unet_atom_score_read", lambda: eng.atom_score_read()),
                       ("ics_unet_atom_score_reset", lambda: eng.atom_score_reset())):
        with pytest.raises(IcsError, match=name + ".*no open accumulator"):
            call()
    for word, args in (("tol", (0.0, 3, 64)), ("tol", (float("nan"), 3, 64)), ("min_voxels", (2.0, -1, 64)),
                       ("max_atoms", (2.0, 3, 0)), ("max_atoms", (2.0, 3, 1025))):
        with pytest.raises(IcsError, match="ics_unet_atom_score_open.*" + word):
            eng.atom_score_open(*args)
    with pytest.raises(IcsError, match="no open accumulator"):
        eng.atom_score_read()                                           # a refused open opened nothing
    eng.atom_score_open(TOL, MIN_VOXELS, MAX_ATOMS)
    with pytest.raises(IcsError, match="ics_unet_atom_score_step.*no resident batch"):
        eng.atom_score_step()
    eng.predict_labels(X)                                               # a resident batch WITHOUT labels
    with pytest.raises(IcsError, match="ics_unet_atom_score_step.*without labels"):
        eng.atom_score_step()
    with pytest.raises(IcsError, match="ics_unet_atom_score_batch.*open confusion accumulator"):
        eng.atom_score_batch(X, lab, with_confusion=True)
    eng.upload_batch(X, lab)
    with pytest.raises(IcsError, match="ics_unet_atom_score_step.*open confusion accumulator"):
        eng.atom_score_step(with_confusion=True)
    eng.atom_score_batch(X, lab)
    good = eng.atom_score_read()
    assert good["totals"][0] == 2 and good["totals"][3] >= 2
    with pytest.raises(IcsError, match="ics_unet_atom_score_open.*max_atoms differs"):
        eng.atom_score_open(TOL, MIN_VOXELS, MAX_ATOMS + 1)
    for args in ((None, L.u8ptr(lab)), (L.fptr(X), None)):
        assert lib.ics_unet_atom_score_batch(eng._h, args[0], args[1], 2, 0.8, 0) != 0
        assert "ics_unet_atom_score_batch" in lib.ics_last_error().decode() and "null" in lib.ics_last_error().decode()
    for batch in (0, CC.MAX_BATCH + 1):
        assert lib.ics_unet_atom_score_batch(eng._h, L.fptr(X), L.u8ptr(lab), batch, 0.8, 0) != 0
        assert "ics_unet_atom_score_batch" in lib.ics_last_error().decode()
    out = {k: np.full_like(v, -7) for k, v in empty_tallies(NCLS).items()}
    ptr = [L.i64ptr(out[k]) for k in TALLIES]
    for k in range(len(ptr)):
        args = list(ptr)
        args[k] = None
        assert lib.ics_unet_atom_score_read(eng._h, *args) != 0
        assert "ics_unet_atom_score_read" in lib.ics_last_error().decode() and "null" in lib.ics_last_error().decode()
    assert lib.ics_unet_atom_score_open(None, 2.0, 3, 64) != 0 and "null handle" in lib.ics_last_error().decode()
    unet = CC.make_engine(95)
    vae = VaeEngine(unet, in_channels=1, d=CC.D, max_batch=2)
    for name, fn in (("ics_unet_atom_score_open", lambda: lib.ics_unet_atom_score_open(vae._h, 2.0, 3, 64)),
                     ("ics_unet_atom_score_reset", lambda: lib.ics_unet_atom_score_reset(vae._h)),
                     ("ics_unet_atom_score_step", lambda: lib.ics_unet_atom_score_step(vae._h, 0.8, 0)),
                     ("ics_unet_atom_score_batch", lambda: lib.ics_unet_atom_score_batch(vae._h, L.fptr(X), L.u8ptr(lab), 2, 0.8, 0)),
                     ("ics_unet_atom_score_read", lambda: lib.ics_unet_atom_score_read(vae._h, *ptr))):
        assert fn() != 0
        assert name in lib.ics_last_error().decode() and "U-Net engine is required" in lib.ics_last_error().decode()
    assert all((a == -7).all() for a in out.values())
    _equal_tallies(eng.atom_score_read(), good)                         # the accumulator is what it was
    eng.close()


# ----------------------------------------------------------------------------------------------------------------------
# 4. eval_unet.py --atoms, end to end in a child process
# ----------------------------------------------------------------------------------------------------------------------
def _eval_unet(tmp_path, name, extra):
    argv = ["--name", name, "--synthetic", "16", "--d", "16", "--channels", "1", "--batch_size", "5", "--nclasses", "17"] + extra
    out = subprocess.run([sys.executable, os.path.join(ROOT, "eval_unet.py")] + argv, capture_output=True, text=True,
                         timeout=600, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    return tmp_path / "output" / "eval_unet" / name, out.stdout


def test_eval_unet_atoms(tmp_path):
    sdir, stdout = _eval_unet(tmp_path, "atom_demo", ["--atoms"])
    assert sorted(os.listdir(str(sdir))) == ["atom_confusion.npy", "atom_report.csv", "atom_report.json", "confusion.npy",
                                             "report.csv", "report.json", "run.json"]
    M = np.load(str(sdir / "atom_confusion.npy"))
    rep, run = json.load(open(str(sdir / "atom_report.json"))), json.load(open(str(sdir / "run.json")))
    tot = dict(zip(("samples", "failed", "perfect", "true_atoms", "pred_atoms", "matched"), rep["tallies"]["totals"]))
    assert M.dtype == np.int64 and M.shape == (18, 18)
    assert M.sum() == tot["true_atoms"] + tot["pred_atoms"] - tot["matched"] and tot["true_atoms"] > 0
    assert tot["samples"] == 4 == run["samples"] and tot["failed"] == 0          # the validation split of 16 grids at 0.8
    assert run["atoms"]["true_atoms"] == tot["true_atoms"] and run["args"]["atoms"] is True and run["args"]["atom_tol"] == 2.0
    # (the synthetic labels run to 94 whatever --nclasses says: those voxels are out of range for the voxel matrix)
    assert np.load(str(sdir / "confusion.npy")).sum() + run["out_of_range"] == run["voxels"] == 4 * 16 ** 3
    assert "worst typed recall" in stdout and "top atom confusions" in stdout and "worst recall" in stdout
    plain, stdout = _eval_unet(tmp_path, "plain_demo", [])
    assert sorted(os.listdir(str(plain))) == ["confusion.npy", "report.csv", "report.json", "run.json"]
    assert "atom" not in stdout and not any("atom" in k for k in json.load(open(str(plain / "run.json")))["args"])
    for f in ("confusion.npy", "report.csv", "report.json"):               # one forward for both scores: the same voxel counts
        assert open(str(plain / f), "rb").read() == open(str(sdir / f), "rb").read(), f
