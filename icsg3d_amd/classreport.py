"""Per-class scores from a confusion matrix (eval_unet.py, train_unet.py --class_report).  Host code: numpy, fp64, no GPU.
The matrix itself is counted on the device (UnetEngine.confusion_*, csrc/confusion.hip); this module only divides.

Conventions: matrix[t, p] = voxels of true class t predicted as p; occupancy[a, b] = voxels with (true != 0) == a and
(sigmoid >= thresh) == b.  A ratio with a zero denominator is NaN in the arrays, null in JSON, an empty cell in the CSV.
"""
from __future__ import annotations

import csv
import json
import os

import numpy as np

PER_CLASS = ("support", "predicted", "tp", "precision", "recall", "f1", "iou")
RATIOS = ("precision", "recall", "f1", "iou")


def _div(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.full(np.broadcast(a, b).shape, np.nan)
    np.divide(a, b, out=out, where=b != 0)
    return out if out.ndim else float(out)


def _mean(values, weights=None):
    """mean over the defined (non-NaN) values; NaN when there is none"""
    values = np.asarray(values, np.float64)
    ok = ~np.isnan(values)
    if weights is None:
        return _div(values[ok].sum(), ok.sum())
    w = np.asarray(weights, np.float64)[ok]
    return _div((values[ok] * w).sum(), w.sum())


def report(matrix, occupancy=None, names=None, top=20):
    """dict of
      classes, names                         class ids and their names (names[i], default str(i))
      support, predicted, tp                 int64 per class: row sums, column sums, the diagonal
      precision, recall, f1, iou             float64 per class: tp / predicted, tp / support, 2 tp / (support + predicted),
                                             tp / (support + predicted - tp)
      voxels, accuracy, accuracy_non_background    trace / total, and the same over the rows of classes 1..
      macro_<ratio>, weighted_<ratio>        over the classes with support > 0 (plain, and weighted by support); a class
                                             with support and no prediction has no precision and is left out of that mean
      top_confusions                         the `top` largest off-diagonal entries, largest first (ties: lower true, then
                                             lower predicted id): dict(true, predicted, count, share_of_row)
      occupancy                              with an occupancy table: dict(tn, fp, fn, tp, precision, recall, f1)"""
    M = np.asarray(matrix)
    if M.ndim != 2 or M.shape[0] != M.shape[1] or M.shape[0] < 2:
        raise ValueError("matrix must be (K, K) with K >= 2, got %s" % (M.shape,))
    if not np.issubdtype(M.dtype, np.integer) or (M < 0).any():
        raise ValueError("matrix must hold non-negative integer counts")
    M = M.astype(np.int64)
    K = M.shape[0]
    names = [str(i) for i in range(K)] if names is None else [str(n) for n in names]
    if len(names) != K:
        raise ValueError("names must have one entry per class (%d), got %d" % (K, len(names)))
    support, predicted, tp = M.sum(1), M.sum(0), np.diag(M).copy()
    r = {"classes": list(range(K)), "names": names, "support": support, "predicted": predicted, "tp": tp,
         "precision": _div(tp, predicted), "recall": _div(tp, support), "f1": _div(2 * tp, support + predicted),
         "iou": _div(tp, support + predicted - tp), "voxels": int(M.sum()), "accuracy": _div(tp.sum(), M.sum()),
         "accuracy_non_background": _div(tp[1:].sum(), support[1:].sum())}
    present = support > 0
    for key in RATIOS:
        r["macro_" + key] = _mean(r[key][present])
        r["weighted_" + key] = _mean(r[key][present], support[present])
    off = M.copy()
    np.fill_diagonal(off, 0)
    order = np.argsort(-off.reshape(-1), kind="stable")[:max(int(top), 0)]      # stable: ties in row-major order
    r["top_confusions"] = [{"true": int(i // K), "predicted": int(i % K), "count": int(off.flat[i]),
                            "share_of_row": _div(off.flat[i], support[i // K])} for i in order if off.flat[i] > 0]
    if occupancy is not None:
        O = np.asarray(occupancy).astype(np.int64).reshape(2, 2)
        tn, fp, fn, otp = int(O[0, 0]), int(O[0, 1]), int(O[1, 0]), int(O[1, 1])
        r["occupancy"] = {"tn": tn, "fp": fp, "fn": fn, "tp": otp, "precision": _div(otp, otp + fp),
                          "recall": _div(otp, otp + fn), "f1": _div(2 * otp, 2 * otp + fp + fn)}
    return r


def _json(v):
    """numpy -> plain JSON values; NaN -> null"""
    if isinstance(v, dict):
        return {k: _json(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_json(x) for x in v]
    if isinstance(v, np.ndarray):
        return [_json(x) for x in v.tolist()]
    if isinstance(v, (float, np.floating)):
        return None if np.isnan(v) else float(v)
    if isinstance(v, np.integer):
        return int(v)
    return v


def write(sdir, matrix, occupancy=None, names=None, top=20, stem="", extra=None, report_name="report"):
    """Writes <sdir>/confusion<stem>.npy (int64), <report_name><stem>.csv (one row per class) and <report_name><stem>.json
    (everything `report` returns, plus `extra`); returns the report."""
    r = report(matrix, occupancy, names, top)
    os.makedirs(sdir, exist_ok=True)
    np.save(os.path.join(sdir, "confusion%s.npy" % stem), np.asarray(matrix, np.int64))
    with open(os.path.join(sdir, "%s%s.csv" % (report_name, stem)), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(("class", "name") + PER_CLASS)
        for c in range(len(r["classes"])):
            row = [c, r["names"][c]] + [int(r[k][c]) for k in PER_CLASS[:3]]
            row += ["" if np.isnan(r[k][c]) else repr(float(r[k][c])) for k in RATIOS]
            w.writerow(row)
    with open(os.path.join(sdir, "%s%s.json" % (report_name, stem)), "w") as f:
        json.dump(_json(dict(r, **(extra or {}))), f, allow_nan=False)
    return r


def reduce_over_ranks(dist, arrays):
    """Sums integer arrays over the ranks of the torch.distributed process group the scripts hold (dataparallel.from_env:
    gloo, the control plane); `dist` None (one process) returns int64 copies.  Every rank receives the sums."""
    arrays = [np.ascontiguousarray(a, np.int64) for a in arrays]
    if dist is None or dist.get_world_size() <= 1:
        return [a.copy() for a in arrays]
    import torch
    flat = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrays]))
    dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    flat, out, at = flat.numpy(), [], 0
    for a in arrays:
        out.append(flat[at:at + a.size].reshape(a.shape).copy())
        at += a.size
    return out


def table(r, worst=10, top=10):
    """A short text table: the `worst` classes by recall among those with support, then the `top` largest confusions."""
    lines = ["voxels %d  accuracy %.4f  non-background %.4f  macro recall %.4f  macro F1 %.4f"
             % (r["voxels"], r["accuracy"], r["accuracy_non_background"], r["macro_recall"], r["macro_f1"])]
    if "occupancy" in r:
        o = r["occupancy"]
        lines.append("occupancy head: precision %.4f  recall %.4f  F1 %.4f" % (o["precision"], o["recall"], o["f1"]))
    have = [c for c in r["classes"] if r["support"][c] > 0]
    lines.append("worst recall (of %d classes with support):" % len(have))
    lines.append("  %-8s %10s %10s %9s %9s %9s" % ("class", "support", "predicted", "recall", "precision", "IoU"))
    for c in sorted(have, key=lambda c: (r["recall"][c], c))[:worst]:
        lines.append("  %-8s %10d %10d %9.4f %9.4f %9.4f" % (r["names"][c], r["support"][c], r["predicted"][c], r["recall"][c],
                                                             r["precision"][c], r["iou"][c]))
    lines.append("top confusions (true -> predicted, count, share of the true class):")
    for e in r["top_confusions"][:top]:
        lines.append("  %-8s -> %-8s %10d %8.4f" % (r["names"][e["true"]], r["names"][e["predicted"]], e["count"], e["share_of_row"]))
    return "\n".join(lines)
