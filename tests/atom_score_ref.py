"""The atom score restated by brute force (DESIGN.md "atom score"): all pairs, Python `sorted` on (d2, i, j), the
take-if-free loop; the tallies and the report in explicit loops; and the synchronous mutual-best rounds the kernel uses,
with their round count.  Plain numpy fp64: `((dx*dx + dy*dy) + dz*dz)` on numpy scalars or arrays forms no FMA."""
import math

import numpy as np

FIX = float(1 << 20)
HIST_BINS = 16
TOTALS = ("samples", "failed", "perfect", "true_atoms", "pred_atoms", "matched", "abs_dn", "no_true")


def d2_matrix(t, p):
    """(n, m) squared distances in the rule's order of operations"""
    t = np.asarray(t, np.float64).reshape(-1, 3)
    p = np.asarray(p, np.float64).reshape(-1, 3)
    dx = t[:, None, 0] - p[None, :, 0]
    dy = t[:, None, 1] - p[None, :, 1]
    dz = t[:, None, 2] - p[None, :, 2]
    return ((dx * dx + dy * dy) + dz * dz)


def greedy_sorted(t, p, tol2):
    """the rule itself: every admissible pair, sorted by (d2, true index, predicted index), taken when both are free.
    Returns match (n,) int: the predicted index of every true atom or -1."""
    D = d2_matrix(t, p)
    n, m = D.shape
    ii, jj = np.nonzero(D < tol2)                                       # strictly below
    pairs = sorted((float(D[i, j]), int(i), int(j)) for i, j in zip(ii, jj))
    match, taken = [-1] * n, [False] * m
    for _, i, j in pairs:
        if match[i] < 0 and not taken[j]:
            match[i], taken[j] = j, True
    return np.array(match, np.int64).reshape(n)


def mutual_best(t, p, tol2):
    """synchronous mutual-best rounds -> (match, rounds that matched something)"""
    D = d2_matrix(t, p)
    n, m = D.shape
    match, partner = [-1] * n, [-1] * m
    rounds = 0
    while True:
        pick_t, pick_p = [-1] * n, [-1] * m
        for i in range(n):
            if match[i] >= 0:
                continue
            best = None
            for j in range(m):
                if partner[j] < 0 and D[i, j] < tol2 and (best is None or (D[i, j], j) < best):
                    best = (D[i, j], j)
            pick_t[i] = -1 if best is None else best[1]
        for j in range(m):
            if partner[j] >= 0:
                continue
            best = None
            for i in range(n):
                if match[i] < 0 and D[i, j] < tol2 and (best is None or (D[i, j], i) < best):
                    best = (D[i, j], i)
            pick_p[j] = -1 if best is None else best[1]
        any_matched = False
        for i in range(n):
            j = pick_t[i]
            if match[i] < 0 and j >= 0 and pick_p[j] == i:
                match[i], partner[j] = j, i
                any_matched = True
        if not any_matched:
            break
        rounds += 1
    return np.array(match, np.int64).reshape(n), rounds


def empty(ncls):
    return {"matrix": np.zeros((ncls + 1, ncls + 1), np.int64), "dist_q": np.zeros(ncls, np.int64),
            "dist2_q": np.zeros(ncls, np.int64), "dup": np.zeros(ncls, np.int64), "shadowed": np.zeros(ncls, np.int64),
            "hist": np.zeros(HIST_BINS, np.int64), "totals": np.zeros(len(TOTALS), np.int64)}


def add(a, b):
    return {k: a[k] + b[k] for k in a}


def score_sample(t, ts, p, ps, ncls, tol, failed=False):
    """the tallies of ONE sample in explicit loops -> (tallies, match, sample_stats (6,), dist_sum)"""
    t = np.asarray(t, np.float64).reshape(-1, 3)
    p = np.asarray(p, np.float64).reshape(-1, 3)
    n, m = len(t), len(p)
    out = empty(ncls)
    out["totals"][0] += 1
    if failed:
        out["totals"][1] += 1
        return out, np.full(n, -1, np.int64), np.array([n, m, -1, -1, -1, -1]), float("nan")
    tol2 = np.float64(tol) * np.float64(tol)
    hist_scale = np.float64(16.0) / np.float64(tol)
    D = d2_matrix(t, p)
    match = greedy_sorted(t, p, tol2)
    taken = set(int(j) for j in match if j >= 0)
    matched = agree = dup = shadowed = 0
    dist_sum = np.float64(0.0)
    for i in range(n):
        j = int(match[i])
        if j >= 0:
            d2 = D[i, j]
            dist = np.sqrt(d2)                                          # correctly rounded
            out["matrix"][ts[i], ps[j]] += 1
            out["dist_q"][ts[i]] += int(np.rint(dist * FIX))            # half to even
            out["dist2_q"][ts[i]] += int(np.rint(d2 * FIX))
            out["hist"][min(15, int(math.floor(dist * hist_scale)))] += 1
            matched += 1
            agree += int(ts[i] == ps[j])
            dist_sum = dist_sum + dist
        else:
            out["matrix"][ts[i], ncls] += 1
            if any(D[i, q] < tol2 for q in range(m)):
                out["shadowed"][ts[i]] += 1
                shadowed += 1
    for j in range(m):
        if j not in taken:
            out["matrix"][ncls, ps[j]] += 1
            if any(D[q, j] < tol2 for q in range(n)):
                out["dup"][ps[j]] += 1
                dup += 1
    perfect = matched == n and matched == m and agree == matched
    out["totals"] += np.array([0, 0, int(perfect), n, m, matched, abs(n - m), int(n == 0)])
    return out, match, np.array([n, m, matched, agree, dup, shadowed]), float(dist_sum)


def score_batch(T, TS, P, PS, ncls, tol, failed=None):
    """sum of score_sample over a batch -> (tallies, [match], sample_stats (B, 6), dist_sum (B,))"""
    tot, matches, stats, sums = empty(ncls), [], [], []
    for b in range(len(T)):
        o, mt, st, ds = score_sample(T[b], TS[b], P[b], PS[b], ncls, tol, failed is not None and bool(failed[b]))
        tot = add(tot, o)
        matches.append(mt); stats.append(st); sums.append(ds)
    return tot, matches, np.array(stats, np.int64).reshape(len(T), 6), np.array(sums, np.float64)


def atoms_of_stats(stats_rows):
    """statistics rows {species, voxels, sum z, sum y, sum x, ...} -> (positions (n, 3) as (x, y, z), species (n,))"""
    st = np.asarray(stats_rows)
    v = st[:, 1].astype(np.float64)
    xyz = np.stack([st[:, 4].astype(np.float64) / v, st[:, 3].astype(np.float64) / v, st[:, 2].astype(np.float64) / v], 1)
    return xyz.reshape(-1, 3), st[:, 0].astype(np.int64)


def _ratio(a, b):
    return float("nan") if b == 0 else float(a) / float(b)


def report_ref(t):
    """the report's figures in explicit loops: dict of per-species lists and an `overall` dict"""
    M = np.asarray(t["matrix"])
    K = M.shape[0] - 1
    r = {k: [] for k in ("true_atoms", "pred_atoms", "detected", "typed", "detection_recall", "typed_recall", "precision",
                         "f1", "mean_error", "rms_error")}
    sums = dict(true=0, pred=0, det=0, typed=0, dq=0, d2q=0)
    for s in range(K):
        true = sum(int(M[s, q]) for q in range(K + 1))
        pred = sum(int(M[q, s]) for q in range(K + 1))
        det = sum(int(M[s, q]) for q in range(K))
        typed = int(M[s, s])
        for k, v in zip(("true_atoms", "pred_atoms", "detected", "typed"), (true, pred, det, typed)):
            r[k].append(v)
        r["detection_recall"].append(_ratio(det, true))
        r["typed_recall"].append(_ratio(typed, true))
        r["precision"].append(_ratio(typed, pred))
        r["f1"].append(_ratio(2 * typed, true + pred))
        r["mean_error"].append(_ratio(int(t["dist_q"][s]) / FIX, det))
        rms = _ratio(int(t["dist2_q"][s]) / FIX, det)
        r["rms_error"].append(rms if math.isnan(rms) else math.sqrt(rms))
        sums["true"] += true; sums["pred"] += pred; sums["det"] += det; sums["typed"] += typed
        sums["dq"] += int(t["dist_q"][s]); sums["d2q"] += int(t["dist2_q"][s])
    tot = dict(zip(TOTALS, (int(v) for v in t["totals"])))
    scored = tot["samples"] - tot["failed"]
    rms = _ratio(sums["d2q"] / FIX, sums["det"])
    r["overall"] = {"true_atoms": sums["true"], "pred_atoms": sums["pred"], "detected": sums["det"], "typed": sums["typed"],
                    "detection_recall": _ratio(sums["det"], sums["true"]), "typed_recall": _ratio(sums["typed"], sums["true"]),
                    "precision": _ratio(sums["typed"], sums["pred"]), "f1": _ratio(2 * sums["typed"], sums["true"] + sums["pred"]),
                    "mean_error": _ratio(sums["dq"] / FIX, sums["det"]), "rms_error": rms if math.isnan(rms) else math.sqrt(rms),
                    "perfect_share": _ratio(tot["perfect"], scored), "mean_abs_dn": _ratio(tot["abs_dn"], scored),
                    "failed": tot["failed"], "samples": tot["samples"],
                    "missed": sum(int(M[s, K]) for s in range(K)), "spurious": sum(int(M[K, s]) for s in range(K)),
                    "dup": sum(int(v) for v in t["dup"]), "shadowed": sum(int(v) for v in t["shadowed"])}
    off = sorted(((-int(M[i, j]), i, j) for i in range(K + 1) for j in range(K + 1) if i != j and M[i, j] > 0))
    r["top_confusions"] = [(i, j, -c) for c, i, j in off]
    return r
