"""Plain restatements of what the confusion kernel counts and of what classreport.report derives from the counts, for
tests/test_confusion_host.py and tests/test_gpu_confusion.py.  Nothing here is shared with the code under test."""
import math

import numpy as np


def _is_class_id(v, ncls):
    """a true label is a class id when it is a whole number in [0, ncls): decided on the value in its own dtype"""
    v = float(v)                                   # uint8, float32 and float64 all convert exactly
    if math.isnan(v) or math.isinf(v):
        return False
    return 0.0 <= v < float(ncls) and v == math.floor(v)


def confusion_ref(true, pred, mask, ncls):
    """(matrix [ncls, ncls] of Python-int counts as int64, occupancy [2, 2] or None, out_of_range): a pair is counted at
    [t, p] when t is a class id and p < ncls, else in out_of_range; occupancy [(t != 0), (mask != 0)] over the pairs
    whose t is a class id, whatever p is."""
    t = np.asarray(true).reshape(-1)
    p = np.asarray(pred, np.uint8).reshape(-1)
    m = None if mask is None else np.asarray(mask, np.uint8).reshape(-1)
    assert p.size == t.size and (m is None or m.size == t.size)
    # the rare values go through the scalar rule one by one; the bulk (exact small whole numbers) is decided in numpy
    # by a comparison against the table of class ids in the array's own dtype
    ids = np.arange(ncls).astype(t.dtype)
    t_ok = np.isin(t, ids)
    for i in np.flatnonzero(~t_ok):
        assert not _is_class_id(t[i], ncls)
    for i in np.flatnonzero(t_ok)[:64]:
        assert _is_class_id(t[i], ncls)
    p_ok = p.astype(np.int64) < ncls
    both = t_ok & p_ok
    matrix = np.zeros((ncls, ncls), np.int64)
    np.add.at(matrix, (t[both].astype(np.int64), p[both].astype(np.int64)), 1)
    oor = int(t.size - int(both.sum()))
    occ = None
    if m is not None:
        occ = np.zeros((2, 2), np.int64)
        np.add.at(occ, ((t[t_ok] != 0).astype(np.int64), (m[t_ok] != 0).astype(np.int64)), 1)
    return matrix, occ, oor


def _ratio(a, b):
    return float("nan") if b == 0 else a / b


def report_ref(matrix, occupancy=None, top=20):
    """The per-class table, the averages and the largest confusions, with explicit loops over Python numbers."""
    M = [[int(v) for v in row] for row in np.asarray(matrix)]
    K = len(M)
    total = sum(sum(row) for row in M)
    per = []
    for c in range(K):
        support = sum(M[c][j] for j in range(K))
        predicted = sum(M[i][c] for i in range(K))
        tp = M[c][c]
        precision, recall = _ratio(tp, predicted), _ratio(tp, support)
        f1 = _ratio(2 * tp, support + predicted)
        iou = _ratio(tp, support + predicted - tp)
        per.append(dict(support=support, predicted=predicted, tp=tp, precision=precision, recall=recall, f1=f1, iou=iou))
    diag = sum(M[c][c] for c in range(K))
    nb_total = sum(per[c]["support"] for c in range(1, K))
    nb_diag = sum(M[c][c] for c in range(1, K))
    out = dict(per_class=per, accuracy=_ratio(diag, total), accuracy_non_background=_ratio(nb_diag, nb_total), voxels=total)
    present = [c for c in range(K) if per[c]["support"] > 0]
    for key in ("precision", "recall", "f1", "iou"):
        # a class with support and no prediction has an undefined precision: the average runs over the defined values
        vals = [per[c][key] for c in present if not math.isnan(per[c][key])]
        out["macro_" + key] = _ratio(sum(vals), len(vals))
        num, den = 0.0, 0
        for c in present:
            if not math.isnan(per[c][key]):
                num += per[c][key] * per[c]["support"]
                den += per[c]["support"]
        out["weighted_" + key] = _ratio(num, den)
    off = []
    for i in range(K):
        for j in range(K):
            if i != j and M[i][j] > 0:
                off.append((M[i][j], i, j))
    off.sort(key=lambda e: (-e[0], e[1], e[2]))
    out["top_confusions"] = [dict(true=i, predicted=j, count=n, share_of_row=_ratio(n, per[i]["support"]))
                             for n, i, j in off[:top]]
    if occupancy is not None:
        O = [[int(v) for v in row] for row in np.asarray(occupancy)]
        tp, fp, fn = O[1][1], O[0][1], O[1][0]
        out["occupancy"] = dict(tp=tp, fp=fp, fn=fn, tn=O[0][0], precision=_ratio(tp, tp + fp), recall=_ratio(tp, tp + fn),
                                f1=_ratio(2 * tp, 2 * tp + fp + fn))
    return out
