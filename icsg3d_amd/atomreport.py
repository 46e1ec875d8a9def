"""Per-species atom scores from the tallies of the atom matching (eval_unet.py --atoms).  Host code: numpy, fp64, no GPU.
The tallies are counted on the device (UnetEngine.atom_score_*, icsg3d_amd.atomscore, csrc/atomscore.hip); this module
only divides, with classreport's conventions: a ratio with a zero denominator is NaN in the arrays, null in JSON, an empty
cell in the CSV.

matrix[t, p] with K = num_classes: matched pairs of true species t and predicted species p; matrix[t, K] unmatched true
atoms (missed); matrix[K, p] unmatched predicted atoms (spurious)."""
from __future__ import annotations

import csv
import json
import os

import numpy as np

from .atomscore import FIX, HIST_BINS, TALLIES, TOTALS
from .classreport import _div, _json, _mean, reduce_over_ranks  # noqa: F401  (reduce_over_ranks: the scripts' rank sum)

COUNTS = ("true_atoms", "pred_atoms", "detected", "typed", "dup", "shadowed")
RATIOS = ("detection_recall", "typed_recall", "precision", "f1", "mean_error", "rms_error")


def _check(t, num_classes=None):
    for k in TALLIES:
        if k not in t:
            raise ValueError("tallies lack %r" % k)
        a = np.asarray(t[k])
        if not np.issubdtype(a.dtype, np.integer) or (a < 0).any():
            raise ValueError("%s must hold non-negative integer counts" % k)
    M = np.asarray(t["matrix"])
    if M.ndim != 2 or M.shape[0] != M.shape[1] or M.shape[0] < 3:
        raise ValueError("matrix must be (K + 1, K + 1) with K >= 2, got %s" % (M.shape,))
    K = M.shape[0] - 1
    if num_classes is not None and K != num_classes:
        raise ValueError("matrix is for %d classes, not %d" % (K, num_classes))
    for k in ("dist_q", "dist2_q", "dup", "shadowed"):
        if np.asarray(t[k]).shape != (K,):
            raise ValueError("%s must have one entry per class (%d)" % (k, K))
    if np.asarray(t["hist"]).shape != (HIST_BINS,) or np.asarray(t["totals"]).shape != (len(TOTALS),):
        raise ValueError("hist must have %d bins and totals %d entries" % (HIST_BINS, len(TOTALS)))
    return K


def _scores(true_atoms, pred_atoms, detected, typed, dist_q, dist2_q):
    return {"detection_recall": _div(detected, true_atoms), "typed_recall": _div(typed, true_atoms),
            "precision": _div(typed, pred_atoms), "f1": _div(2 * typed, true_atoms + pred_atoms),
            "mean_error": _div(np.asarray(dist_q, np.float64) / FIX, detected),
            "rms_error": np.sqrt(_div(np.asarray(dist2_q, np.float64) / FIX, detected))}


def report(tallies, tol=None, names=None, top=20):
    """dict of
      classes, names                   species ids and their names (default str(i)); "none" stands for no atom
      true_atoms, pred_atoms           int64 per species: row and column sums of the matrix (missed / spurious included)
      detected, typed                  matched to any species (the row without its last column), and to the same one
      detection_recall, typed_recall   detected / true_atoms, typed / true_atoms
      precision, f1                    typed / pred_atoms, 2 typed / (true_atoms + pred_atoms)
      mean_error, rms_error            localisation error of the detected atoms in voxels, from the fixed-point sums
      dup, shadowed                    unmatched predicted atoms next to a true atom (by predicted species), unmatched true
                                       atoms next to a predicted atom (by true species)
      overall                          the same figures over all species, plus samples, failed, perfect,
                                       perfect_share and mean_abs_dn (both over the samples that did not fail), no_true
      macro_<ratio>                    plain means over the species with true atoms
      top_confusions                   the `top` largest off-diagonal entries of the whole matrix, largest first (ties in
                                       row-major order): dict(true, predicted, count, share_of_row)
      hist, hist_edges                 matched distances in 16 bins of tol / 16 (edges only when tol is given)"""
    K = _check(tallies)
    M = np.asarray(tallies["matrix"]).astype(np.int64)
    names = [str(i) for i in range(K)] if names is None else [str(n) for n in names]
    if len(names) != K:
        raise ValueError("names must have one entry per class (%d), got %d" % (K, len(names)))
    dist_q, dist2_q = np.asarray(tallies["dist_q"], np.int64), np.asarray(tallies["dist2_q"], np.int64)
    dup, shadowed = np.asarray(tallies["dup"], np.int64), np.asarray(tallies["shadowed"], np.int64)
    tot = dict(zip(TOTALS, (int(v) for v in np.asarray(tallies["totals"]))))
    true_atoms, pred_atoms = M[:K].sum(1), M[:, :K].sum(0)
    detected, typed = M[:K, :K].sum(1), np.diag(M)[:K].copy()
    r = {"classes": list(range(K)), "names": names, "true_atoms": true_atoms, "pred_atoms": pred_atoms, "detected": detected,
         "typed": typed, "dup": dup, "shadowed": shadowed}
    r.update(_scores(true_atoms, pred_atoms, detected, typed, dist_q, dist2_q))
    present = true_atoms > 0
    for key in RATIOS:
        r["macro_" + key] = _mean(r[key][present])
    scored = tot["samples"] - tot["failed"]
    overall = {"true_atoms": int(true_atoms.sum()), "pred_atoms": int(pred_atoms.sum()), "detected": int(detected.sum()),
               "typed": int(typed.sum()), "dup": int(dup.sum()), "shadowed": int(shadowed.sum()),
               "missed": int(M[:K, K].sum()), "spurious": int(M[K, :K].sum())}
    overall.update(_scores(true_atoms.sum(), pred_atoms.sum(), detected.sum(), typed.sum(), dist_q.sum(), dist2_q.sum()))
    overall.update({"samples": tot["samples"], "failed": tot["failed"], "perfect": tot["perfect"], "no_true": tot["no_true"],
                    "perfect_share": _div(tot["perfect"], scored), "mean_abs_dn": _div(tot["abs_dn"], scored)})
    r["overall"] = overall
    off = M.copy()
    np.fill_diagonal(off, 0)
    rows = M.sum(1)
    order = np.argsort(-off.reshape(-1), kind="stable")[:max(int(top), 0)]
    r["top_confusions"] = [{"true": int(i // (K + 1)), "predicted": int(i % (K + 1)), "count": int(off.flat[i]),
                            "share_of_row": _div(off.flat[i], rows[i // (K + 1)])} for i in order if off.flat[i] > 0]
    r["hist"] = np.asarray(tallies["hist"], np.int64)
    r["hist_edges"] = None if tol is None else np.arange(HIST_BINS + 1, dtype=np.float64) * (float(tol) / HIST_BINS)
    return r


def write(sdir, tallies, tol=None, names=None, top=20, extra=None):
    """Writes <sdir>/atom_confusion.npy (the int64 matrix), atom_report.csv (one row per species) and atom_report.json
    (everything `report` returns, the raw tallies, plus `extra`); returns the report."""
    r = report(tallies, tol, names, top)
    os.makedirs(sdir, exist_ok=True)
    np.save(os.path.join(sdir, "atom_confusion.npy"), np.asarray(tallies["matrix"], np.int64))
    with open(os.path.join(sdir, "atom_report.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(("class", "name") + COUNTS + RATIOS)
        for c in r["classes"]:
            row = [c, r["names"][c]] + [int(r[k][c]) for k in COUNTS]
            row += ["" if np.isnan(r[k][c]) else repr(float(r[k][c])) for k in RATIOS]
            w.writerow(row)
    raw = {k: np.asarray(tallies[k], np.int64) for k in TALLIES if k != "matrix"}
    with open(os.path.join(sdir, "atom_report.json"), "w") as f:
        json.dump(_json(dict(r, tallies=raw, **(extra or {}))), f, allow_nan=False)
    return r


def _name(r, i):
    return r["names"][i] if i < len(r["names"]) else "none"


def table(r, worst=10, top=10):
    """A short text table: the overall figures, the `worst` species by typed recall among those with true atoms, then
    the `top` largest atom confusions."""
    o = r["overall"]
    lines = ["atoms: true %d  predicted %d  detected %d  typed %d  missed %d  spurious %d  dup %d  shadowed %d"
             % (o["true_atoms"], o["pred_atoms"], o["detected"], o["typed"], o["missed"], o["spurious"], o["dup"], o["shadowed"]),
             "detection recall %.4f  typed recall %.4f  precision %.4f  F1 %.4f  mean error %.4f  rms %.4f voxels"
             % (o["detection_recall"], o["typed_recall"], o["precision"], o["f1"], o["mean_error"], o["rms_error"]),
             "samples %d  failed %d  perfect %.4f  mean |dN| %.4f"
             % (o["samples"], o["failed"], o["perfect_share"], o["mean_abs_dn"])]
    have = [c for c in r["classes"] if r["true_atoms"][c] > 0]
    lines.append("worst typed recall (of %d species with true atoms):" % len(have))
    lines.append("  %-8s %8s %8s %9s %9s %9s %9s %6s %8s" % ("species", "true", "pred", "detected", "typed", "precision",
                                                              "error", "dup", "shadowed"))
    for c in sorted(have, key=lambda c: (r["typed_recall"][c], c))[:worst]:
        lines.append("  %-8s %8d %8d %9.4f %9.4f %9.4f %9.4f %6d %8d"
                     % (r["names"][c], r["true_atoms"][c], r["pred_atoms"][c], r["detection_recall"][c], r["typed_recall"][c],
                        r["precision"][c], r["mean_error"][c], r["dup"][c], r["shadowed"][c]))
    lines.append("top atom confusions (true -> predicted, count, share of the true species' atoms):")
    for e in r["top_confusions"][:top]:
        lines.append("  %-8s -> %-8s %8d %8.4f" % (_name(r, e["true"]), _name(r, e["predicted"]), e["count"], e["share_of_row"]))
    return "\n".join(lines)
