"""Brute-force fp64 restatement of ics_op_structure_fingerprint and ics_op_fingerprint_nearest, written from the text in
include/icsg3d.h (not from the kernels): every (i, j, T) of the image range plus a margin is enumerated in numpy, and
widening the margin must change nothing.  The device ops are held against this (tests/test_gpu_structure_fingerprint.py)."""
import math

import numpy as np

MAX_IMAGE = 32


def H(t):
    """The integral of the triangular kernel of half-width 1 from -inf to t."""
    t = np.clip(np.asarray(t, np.float64), -1.0, 1.0)
    return np.where(t <= 0.0, 0.5 * (1.0 + t) ** 2, 1.0 - 0.5 * (1.0 - t) ** 2)


def edges(r_max, n_bins):
    return np.arange(n_bins + 1, dtype=np.float64) * r_max / n_bins


def reach(M, r_max, w, cn_tol):
    """max(R, (1 + cn_tol) l), l the shortest lattice vector: an atom's own image along it bounds nn_dist."""
    return max(r_max + w, (1.0 + cn_tol) * float(np.sqrt((np.asarray(M, np.float64) ** 2).sum(1)).min()))


def image_range(M, r):
    """|T_k| <= floor(r g_k + 1), g the norms of the columns of inv(M)."""
    g = np.linalg.norm(np.linalg.inv(np.asarray(M, np.float64)), axis=0)
    return np.floor(r * g + 1.0).astype(np.int64)


def _distances(f, M, T):
    """d[i, j, t] = |(f_j - f_i + T_t) M| for the images |T_k| <= T[k], T lexicographic."""
    tr = np.array([[a, b, c] for a in range(-T[0], T[0] + 1) for b in range(-T[1], T[1] + 1)
                   for c in range(-T[2], T[2] + 1)], np.float64)
    n = len(f)
    d = np.empty((n, n, len(tr)))
    for i in range(n):
        v = ((f - f[i])[:, None, :] + tr[None, :, :]) @ M
        d[i] = np.sqrt((v ** 2).sum(-1))
    return d


def fingerprint_one(Z, f, M, r_max=6.0, n_bins=60, w=0.1, cn_tol=0.1, margin=1, wrap=True):
    """One structure: dict(count, countz, rdf (2, n_bins), n_pairs, nn_dist, cn, gap) -- gap is the smallest relative
    distance of any pair to a threshold the integer outputs hang on (R for n_pairs, (1 + cn_tol) nn_dist for cn)."""
    Z = np.asarray(Z, np.int64)
    f = np.asarray(f, np.float64).reshape(len(Z), 3)
    M = np.asarray(M, np.float64).reshape(3, 3)
    if wrap:
        f = f - np.floor(f)
    n, V, R = len(Z), float(np.linalg.det(M)), r_max + w
    span = R if wrap else R + float(np.abs(f).max() + 1.0) * float(np.sqrt((M ** 2).sum(1)).sum())
    T = image_range(M, max(span, reach(M, r_max, w, cn_tol))) + margin
    d = _distances(f, M, T)
    pos = d > 0.0
    r = edges(r_max, n_bins)
    zbar = Z.sum() / n
    wz = (Z[:, None] * Z[None, :]).astype(np.float64) / (zbar * zbar)
    sel = pos & (d < R)
    dd = d[sel]
    ww = np.broadcast_to(wz[:, :, None], d.shape)[sel]
    count, countz = np.zeros(n_bins), np.zeros(n_bins)
    for k in range(n_bins):
        near = (dd > r[k] - w) & (dd < r[k + 1] + w)
        dep = H((r[k + 1] - dd[near]) / w) - H((r[k] - dd[near]) / w)
        count[k] = math.fsum(dep)
        countz[k] = math.fsum(dep * ww[near])
    norm = n * (n / V) * 4.0 * math.pi / 3.0 * (r[1:] ** 3 - r[:-1] ** 3)
    dpos = np.where(pos, d, np.inf).reshape(n, -1)
    nn = dpos.min(1)
    thr = (1.0 + cn_tol) * nn
    cn = (dpos <= thr[:, None]).sum(1).astype(np.int32)
    gap = min(float(np.abs(dpos / R - 1.0).min()), float(np.abs(dpos / thr[:, None] - 1.0).min()))
    return {"count": count, "countz": countz, "rdf": np.stack([count / norm, countz / norm]), "n_pairs": int(sel.sum()),
            "nn_dist": nn, "cn": cn, "gap": gap}


def fingerprint_checked(Z, f, M, r_max=6.0, n_bins=60, w=0.1, cn_tol=0.1):
    """fingerprint_one with the assertion that a wider margin changes nothing."""
    a = fingerprint_one(Z, f, M, r_max, n_bins, w, cn_tol, margin=1)
    b = fingerprint_one(Z, f, M, r_max, n_bins, w, cn_tol, margin=2)
    assert a["n_pairs"] == b["n_pairs"] and np.array_equal(a["cn"], b["cn"]) and np.array_equal(a["nn_dist"], b["nn_dist"])
    assert np.abs(a["count"] - b["count"]).max() <= 1e-13 * max(1.0, a["count"].max())
    assert np.abs(a["countz"] - b["countz"]).max() <= 1e-13 * max(1.0, a["countz"].max())
    return a


def fingerprint_ref(structs, eligible=None, r_max=6.0, n_bins=60, w=0.1, cn_tol=0.1):
    """The op's outputs for a list of (Z, frac, M): rdf, count, n_pairs, nn_dist, cn, reason, and `gap` (see
    fingerprint_one; the smallest over the batch)."""
    ns = len(structs)
    el = np.ones(ns, np.int32) if eligible is None else np.asarray(eligible, np.int32)
    off = np.zeros(ns + 1, np.int64)
    off[1:] = np.cumsum([len(s[0]) for s in structs])
    out = {"rdf": np.full((ns, 2, n_bins), np.nan), "count": np.full((ns, n_bins), np.nan),
           "n_pairs": np.full(ns, -1, np.int64), "nn_dist": np.full(int(off[-1]), np.nan),
           "cn": np.full(int(off[-1]), -1, np.int32), "reason": np.zeros(ns, np.int32), "gap": np.inf}
    for s, (Z, f, M) in enumerate(structs):
        if not el[s]:
            out["reason"][s] = 1
            continue
        if image_range(M, reach(M, r_max, w, cn_tol)).max() > MAX_IMAGE:
            out["reason"][s] = 2
            continue
        o = fingerprint_checked(Z, f, M, r_max, n_bins, w, cn_tol)
        out["rdf"][s], out["count"][s], out["n_pairs"][s] = o["rdf"], o["count"], o["n_pairs"]
        out["nn_dist"][off[s]:off[s + 1]], out["cn"][off[s]:off[s + 1]] = o["nn_dist"], o["cn"]
        out["gap"] = min(out["gap"], o["gap"])
    return out


def packed_ref(offsets, species, frac, lattice, eligible, r_max=6.0, n_bins=60, width=0.1, cn_tol=0.1):
    """fingerprint_packed's signature on the restatement: what the Python layer runs on without a GPU."""
    offsets = np.asarray(offsets)
    frac = np.asarray(frac, np.float64).reshape(-1, 3)
    structs = [(np.asarray(species)[offsets[k]:offsets[k + 1]], frac[offsets[k]:offsets[k + 1]],
                np.asarray(lattice, np.float64).reshape(-1, 3, 3)[k]) for k in range(len(offsets) - 1)]
    o = fingerprint_ref(structs, eligible, r_max, n_bins, width, cn_tol)
    o.pop("gap")
    return o


def distance(a, b):
    """D(a, b) = sqrt((1 / len) sum_k (a_k - b_k)^2), from the differences."""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return math.sqrt(math.fsum(d * d) / len(d))


def nearest_ref(fp, valid, nq, nref):
    """The op's outputs, and `gap`: the smallest relative difference between the best and the second-best partner of any
    row whose two best are not bit-equal rows (the indices hang on it)."""
    fp = np.asarray(fp, np.float64)
    valid = np.asarray(valid).astype(bool)
    n = nq + nref
    out = {"q_ref": np.full(nq, -1, np.int32), "q_ref_d": np.full(nq, np.inf), "ref_q": np.full(nref, -1, np.int32),
           "ref_q_d": np.full(nref, np.inf), "q_q": np.full(nq, -1, np.int32), "q_q_d": np.full(nq, np.inf)}
    gap = [np.inf]

    def best(row, lo, hi, key_i, key_d, slot):
        cand = [p for p in range(lo, hi) if valid[p] and p != row]
        if not cand:
            return
        d = np.sqrt(((fp[cand] - fp[row]) ** 2).sum(1) / fp.shape[1])
        k = int(np.argmin(d))                                         # the first minimum: the lower index
        out[key_i][slot], out[key_d][slot] = cand[k] - lo, distance(fp[row], fp[cand[k]])
        other = ~(fp[cand] == fp[cand[k]]).all(1)                     # rows that are not bit-equal to the best one
        if other.any():
            gap[0] = min(gap[0], float((np.abs(d[other] - d[k]) / np.maximum(d[other], 1e-300)).min()))
    for q in range(nq):
        if valid[q]:
            best(q, nq, n, "q_ref", "q_ref_d", q)
            best(q, 0, nq, "q_q", "q_q_d", q)
    for r in range(nq, n):
        if valid[r]:
            best(r, 0, nq, "ref_q", "ref_q_d", r - nq)
    vq = [q for q in range(nq) if valid[q]]
    terms = []
    for a, q in enumerate(vq):
        rest = vq[a + 1:]
        if rest:
            terms.append(np.sqrt(((fp[rest] - fp[q]) ** 2).sum(1) / fp.shape[1]))
    out["div_sum"] = math.fsum(np.concatenate(terms)) if terms else 0.0
    out["div_pairs"] = len(vq) * (len(vq) - 1) // 2
    out["gap"] = gap[0]
    return out


def nearest_packed_ref(fp, valid, nq, nref):
    """fingerprint_nearest's signature on the restatement."""
    o = nearest_ref(fp, valid, nq, nref)
    o.pop("gap")
    return o
