"""fp64 brute-force restatement of the structure-match predicate (include/icsg3d.h, ics_op_structure_match) that the GPU
tests hold the kernel to.  The predicate is the project's own; no parity with pymatgen's StructureMatcher is claimed.

A structure is (Z (n,), frac (n, 3), M (3, 3) with rows va, vb, vc).  Everything is plain numpy over all (op, anchor)
combinations, with no bucket ordering, no species grouping and no early exit: slow, simple, and independent of the
kernel's work mapping.
"""
import functools
import itertools

import numpy as np


@functools.lru_cache(maxsize=None)
def signed_permutations(ops_mode):
    """The op list in the documented order: lexicographic over (permutation, sign pattern), + before -.  (k, 3, 3)."""
    ops = []
    for perm in itertools.permutations(range(3)):
        for sign in itertools.product((1, -1), repeat=3):
            P = np.zeros((3, 3))
            for k in range(3):
                P[k, perm[k]] = sign[k]
            ops.append(P)
    if ops_mode == 0:
        return np.array(ops[:1])
    if ops_mode == 1:
        return np.array([P for P in ops if round(np.linalg.det(P)) == 1])
    assert ops_mode == 2
    return np.array(ops)


def comparable(A, B):
    ZA, ZB = np.asarray(A[0]), np.asarray(B[0])
    return len(ZA) == len(ZB) and np.array_equal(np.sort(ZA), np.sort(ZB))


def admissible(MA, MB, P, ltol):
    GA, GB = MA @ MA.T, MB @ MB.T
    Gp = P @ GA @ P.T
    d = np.sqrt(np.diag(GB))
    return bool(np.all(np.abs(Gp - GB) <= ltol * np.outer(d, d)))


def anchor_atom(Z):
    """The lowest-index atom of the species with the smallest count (ties between species to the lower Z)."""
    Z = np.asarray(Z)
    zs, cnt = np.unique(Z, return_counts=True)          # ascending Z
    z0 = zs[np.argmin(cnt)]                             # first minimum = lower Z
    return int(np.nonzero(Z == z0)[0][0]), int(z0)


def combination(A, B, P, j, tol):
    """One (P, j): (passes, rms, nb, u)."""
    ZA, fA, _ = A
    ZB, fB, MB = B
    fA = fA - np.floor(fA)
    fB = fB - np.floor(fB)
    a0, _ = anchor_atom(ZA)
    t = fB[j] - P @ fA[a0]
    n = len(ZA)
    p = fA @ P.T + t                                    # p_i = P f_i + t
    D = fB[None, :, :] - p[:, None, :]
    D -= np.rint(D)
    v = D @ MB                                          # u = M_B^T D, for every (i, atom of B)
    d2 = (v * v).sum(-1)
    d2[np.asarray(ZA)[:, None] != np.asarray(ZB)[None, :]] = np.inf
    nb = d2.argmin(1)                                   # first minimum = lower index
    u = v[np.arange(n), nb]
    r = u - u.mean(0)
    rn = np.sqrt((r * r).sum(1))
    ok = bool(np.all(np.sqrt((u * u).sum(1)) <= 2 * tol) and len(set(nb.tolist())) == n and rn.max() <= tol)
    return ok, float(np.sqrt((rn * rn).mean())), nb, u


def match_pair(A, B, tol=0.1, ltol=0.05, ops_mode=1):
    """dict(compared, match, rms, op, anchor, n_admissible, runner_up): runner_up is the second-smallest rms over the
    passing combinations (inf below two)."""
    out = {"compared": comparable(A, B), "match": False, "rms": np.inf, "op": -1, "anchor": -1, "n_admissible": 0,
           "runner_up": np.inf}
    if not out["compared"]:
        return out
    ZA, fA, MA = (np.asarray(A[0]), np.asarray(A[1], np.float64).reshape(-1, 3), np.asarray(A[2], np.float64))
    ZB, fB, MB = (np.asarray(B[0]), np.asarray(B[1], np.float64).reshape(-1, 3), np.asarray(B[2], np.float64))
    _, z0 = anchor_atom(ZA)
    passing = []
    for o, P in enumerate(signed_permutations(ops_mode)):
        if not admissible(MA, MB, P, ltol):
            continue
        out["n_admissible"] += 1
        for j in np.nonzero(ZB == z0)[0]:
            ok, rms, _, _ = combination((ZA, fA, MA), (ZB, fB, MB), P, int(j), tol)
            if ok:
                passing.append((rms, o, int(j)))
    if passing:
        passing.sort()                                  # (rms, op, anchor): ties to the lower (op, anchor)
        out.update(match=True, rms=passing[0][0], op=passing[0][1], anchor=passing[0][2])
        if len(passing) > 1:
            out["runner_up"] = passing[1][0]
    return out


def match_ref(structs, eligible, nq, tol=0.1, ltol=0.05, ops_mode=1):
    """The per-query outputs of ics_op_structure_match for structs = queries then references, plus `pairs`: the
    match_pair record of every compared pair, keyed (A index, B index)."""
    ns = len(structs)
    out = {"dup_of": np.full(nq, -1, np.int32), "dup_rms": np.full(nq, np.inf), "dup_op": np.full((nq, 2), -1, np.int32),
           "ref_of": np.full(nq, -1, np.int32), "ref_rms": np.full(nq, np.inf), "ref_op": np.full((nq, 2), -1, np.int32),
           "n_cmp": np.zeros((nq, 2), np.int32), "pairs": {}}
    for q in range(nq):
        if not eligible[q]:
            continue
        for e in range(q):
            if eligible[e] and comparable(structs[e], structs[q]):
                out["n_cmp"][q, 0] += 1
                r = out["pairs"][(e, q)] = match_pair(structs[e], structs[q], tol, ltol, ops_mode)
                if r["match"] and out["dup_of"][q] < 0:
                    out["dup_of"][q], out["dup_rms"][q], out["dup_op"][q] = e, r["rms"], (r["op"], r["anchor"])
        for k in range(nq, ns):
            if eligible[k] and comparable(structs[q], structs[k]):
                out["n_cmp"][q, 1] += 1
                r = out["pairs"][(q, k)] = match_pair(structs[q], structs[k], tol, ltol, ops_mode)
                if r["match"] and r["rms"] < out["ref_rms"][q]:
                    out["ref_of"][q], out["ref_rms"][q], out["ref_op"][q] = k - nq, r["rms"], (r["op"], r["anchor"])
    return out
