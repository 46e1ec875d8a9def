"""Atom score on the device: what the op and the accumulator loop cost against the host.

  1. ics_op_atom_score on 32 / 1024 / 16384 samples of 40 x 40 atoms, host pointers in and tallies out -- the upload is
     inside the time -- against the same greedy matching as a numpy loop over the samples (matching only: the host loop
     leaves the tallies out, so the ratio flatters the host);
  2. eval_unet.py's loop with --atoms (atom_score_batch with the voxel counts, one read at the end) against the loop
     without (confusion_batch), and against predict_labels + ics_op_segment_atoms twice + the numpy matching per batch, on
     one engine (B = 32, d = 32, C = 1, 95 classes); the kernels' own time per launch comes from the engine's profiler in
     a separate pass.  The engine has random weights: the totals of the tallies are recorded next to the times, so the
     number of atoms the matching saw can be read off.

  python scripts/atom_score_bench.py [--out profiles/atom_score_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchutil import timeit  # noqa: E402

NCLS, ATOMS, TOL = 95, 40, 2.0


def greedy_numpy(t, p, tol2):
    """the rule on the host: admissible pairs sorted by (d2, i, j), taken when both are free -> match (n,)"""
    match = np.full(len(t), -1, np.int64)
    if not len(t) or not len(p):
        return match
    dx, dy, dz = (t[:, None, k] - p[None, :, k] for k in range(3))
    D = ((dx * dx + dy * dy) + dz * dz)
    ii, jj = np.nonzero(D < tol2)
    order = np.lexsort((jj, ii, D[ii, jj]))
    taken = np.zeros(len(p), bool)
    for i, j in zip(ii[order].tolist(), jj[order].tolist()):
        if match[i] < 0 and not taken[j]:
            match[i], taken[j] = j, True
    return match


def op_bench():
    from icsg3d_amd.atomscore import _ragged, score_packed
    rng = np.random.default_rng(0)
    out = {"how": "ics_op_atom_score on samples of %d x %d atoms (true atoms uniform in a 32^3 box, predictions = the true "
                  "atoms moved by N(0, 0.5) in a random order), %d classes, tol %.1f: median of 5 calls after 1, host "
                  "pointers in and tallies out; the numpy loop runs the matching alone, once" % (ATOMS, ATOMS, NCLS, TOL)}
    for batch in (32, 1024, 16384):
        T = [rng.uniform(0, 32, (ATOMS, 3)) for _ in range(batch)]
        P = [(t + rng.normal(0, 0.5, t.shape))[rng.permutation(ATOMS)] for t in T]
        S = [rng.integers(1, NCLS, ATOMS).astype(np.int32) for _ in range(batch)]
        tp, pp = _ragged(T, S), _ragged(P, S)                           # packed once, outside the time
        dev = timeit(lambda: score_packed(*tp, *pp, NCLS, TOL), 5, 1)
        packed = timeit(lambda: score_packed(*tp, *pp, NCLS, TOL, per_sample=True), 3, 1)
        t0 = time.perf_counter()
        host = [greedy_numpy(t, p, TOL * TOL) for t, p in zip(T, P)]
        host_ms = (time.perf_counter() - t0) * 1e3
        r = score_packed(*tp, *pp, NCLS, TOL, per_sample=True)
        assert all(np.array_equal(a, b) for a, b in zip(r["match"], host))
        out[str(batch)] = {"samples": batch, "op_ms_median": dev["median_ms"], "op_ms_min": dev["min_ms"],
                           "op_with_per_sample_outputs_ms_median": packed["median_ms"],
                           "samples_per_s": batch / dev["median_ms"] * 1e3, "numpy_loop_ms": host_ms,
                           "numpy_over_op": host_ms / dev["median_ms"], "matched": int(r["totals"][5])}
        print(batch, out[str(batch)], flush=True)
    return out


def loop_bench(batches=20, B=32, d=32, max_atoms=512, min_voxels=3):
    from icsg3d_amd.engine import UnetEngine
    from icsg3d_amd.synthetic import synthetic_batch
    from icsg3d_amd.watershed import segment_atoms
    X, lab, _ = synthetic_batch(B, d, 1, seed=0, noise=1e-3)
    X, lab = np.asarray(X, np.float32), np.asarray(lab, np.uint8).reshape(B, d, d, d)
    eng = UnetEngine(in_channels=1, num_classes=NCLS, d=d, max_batch=B)
    eng.confusion_open()
    eng.atom_score_open(TOL, min_voxels, max_atoms)

    def atoms_loop():
        eng.confusion_reset()
        eng.atom_score_reset()
        for _ in range(batches):
            eng.atom_score_batch(X, lab, 0.8, with_confusion=True)
        return eng.confusion_read(), eng.atom_score_read()

    def plain_loop():
        eng.confusion_reset()
        for _ in range(batches):
            eng.confusion_batch(X, lab, 0.8)
        return eng.confusion_read()

    def rows_to_atoms(seg, b):
        st = seg["stats"][b, :seg["n_atoms"][b]].astype(np.float64)
        return np.stack([st[:, 4] / st[:, 1], st[:, 3] / st[:, 1], st[:, 2] / st[:, 1]], 1).reshape(-1, 3)

    def host_loop():
        matched = 0
        for _ in range(batches):
            sp, mk = eng.predict_labels(X, 0.8)
            pred = segment_atoms(mk.reshape(lab.shape), sp.reshape(lab.shape), min_voxels, max_atoms, NCLS, want_regions=False)
            true = segment_atoms(lab, lab, 0, max_atoms, NCLS, want_regions=False)
            for b in range(B):
                matched += int((greedy_numpy(rows_to_atoms(true, b), rows_to_atoms(pred, b), TOL * TOL) >= 0).sum())
        return matched

    def resident_loop():
        eng.atom_score_reset()
        eng.upload_batch(X, lab)
        for _ in range(batches):
            eng.atom_score_step(0.8)
        return eng.atom_score_read()

    conf, tallies = atoms_loop()
    assert np.array_equal(conf["matrix"], plain_loop()["matrix"]) and int(tallies["totals"][5]) == host_loop()
    ta, tp, th, tr = timeit(atoms_loop, 5, 1), timeit(plain_loop, 5, 1), timeit(host_loop, 3, 1), timeit(resident_loop, 5, 1)
    eng.profile_enable(True)
    resident_loop()
    rows = {r["label"]: r for r in eng.profile_rows()}
    eng.profile_enable(False)

    def per_launch(label):
        k = rows.get(label)
        return None if not k else {"ms_per_step": k["ms"] / batches, "launches_per_step": k["launches"] / batches}

    gps = lambda t: batches * B / t["median_ms"] * 1e3                   # noqa: E731
    out = {"how": "one engine with random weights, B = %d, d = %d, C = 1, %d classes, max_atoms %d, %d batches per loop, "
                  "median of 5 loops after 1 (3 for the host loop); grids/s = batches * B / loop time"
                  % (B, d, NCLS, max_atoms, batches),
           "atom_score_batch_with_confusion_loop": {"ms_median": ta["median_ms"], "grids_per_s": gps(ta)},
           "confusion_batch_loop": {"ms_median": tp["median_ms"], "grids_per_s": gps(tp)},
           "atoms_over_plain": ta["median_ms"] / tp["median_ms"],
           "predict_labels_segment_atoms_numpy_loop": {"ms_median": th["median_ms"], "grids_per_s": gps(th)},
           "atom_score_step_resident_loop": {"ms_median": tr["median_ms"], "grids_per_s": gps(tr)},
           "atom_score_kernel": per_launch("atom_score"), "segmentation_kernels": per_launch("atom_segment"),
           "totals_of_one_loop": dict(zip(("samples", "failed", "perfect", "true_atoms", "pred_atoms", "matched", "abs_dn",
                                           "no_true"), (int(v) for v in tallies["totals"])))}
    print(out, flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "atom_score_bench.json"))
    a = ap.parse_args()
    t0 = time.time()
    rec = {"what": "atom score on the device (DESIGN.md section 28): the op against a numpy greedy loop, eval_unet.py's loop "
                   "with --atoms against without and against predict_labels + ics_op_segment_atoms + numpy",
           "op": op_bench(), "loop": loop_bench()}
    rec["seconds"] = time.time() - t0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)
