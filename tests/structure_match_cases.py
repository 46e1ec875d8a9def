"""Hand-built structures for the structure-match tests (CPU: the restatement against answers known by construction;
GPU: ics_op_structure_match against the restatement).  A structure is (Z, frac, M) as in tests/structure_match_ref.py.

derive() makes B from A by an op P (f' = P f, M' = P M: the same atoms in space, G' = P G P^T; for an improper P the
cell is inverted through the origin as well, which keeps G and the volume positive), cartesian displacements,
a random translation, whole lattice-vector shifts of single atoms and a shuffled atom order.  With displacements d_i of
zero mean the combination (P, true anchor) has u_i = d_i - d_a0 and residuals r_i = d_i exactly, whatever the anchor's
own displacement: that is what fixes the outcomes below by construction.
"""
import numpy as np

import structure_match_ref as MR
import structure_ref as SR

TOL, LTOL = 0.1, 0.05


def lat(abc, ang=(90.0, 90.0, 90.0)):
    return SR.lattice_from_parameters(*abc, *ang)


def motif(rng, Z, M, dmin=1.2):
    """Random fractional coordinates whose periodic distances all exceed dmin (added one atom at a time)."""
    Z = np.asarray(Z, np.int32)
    f = np.zeros((0, 3))
    inv_rows = M
    while len(f) < len(Z):
        c = rng.uniform(0, 1, 3)
        if len(f):
            d = f - c
            d -= np.rint(d)
            best = np.inf
            for n in np.ndindex(3, 3, 3):
                v = (d + (np.array(n) - 1.0)) @ inv_rows
                best = min(best, np.sqrt((v * v).sum(1)).min())
            if best <= dmin:
                continue
        f = np.vstack([f, c])
    return Z, f, M


def noise_max(rng, n, amp):
    """Zero-mean displacements whose largest norm is exactly amp."""
    d = rng.standard_normal((n, 3))
    d -= d.mean(0)
    return d * (amp / np.sqrt((d * d).sum(1)).max())


def noise_one(rng, n, k, amp):
    """Atom k displaced by amp, the others by -v / (n - 1): zero mean, residual amp at k."""
    v = rng.standard_normal(3)
    v *= amp / np.linalg.norm(v)
    d = np.tile(-v / (n - 1), (n, 1))
    d[k] = v
    return d


def derive(rng, A, P=None, disp=None, translate=True, shifts=True, shuffle=True):
    """B = the structure A seen through P, displaced by disp (cartesian, A's atom order).  Returns (B, perm) with B's
    atom k = A's atom perm[k]."""
    Z, f, M = np.asarray(A[0], np.int32), np.asarray(A[1], np.float64), np.asarray(A[2], np.float64)
    P = np.eye(3) if P is None else np.asarray(P, np.float64)
    fB, MB = f @ P.T, P @ M
    if np.linalg.det(MB) < 0:                  # an improper P: the mirror image, in a right-handed cell with the same G
        MB = -MB
    if disp is not None:
        fB = fB + np.asarray(disp) @ np.linalg.inv(MB)
    if translate:
        fB = fB + rng.uniform(-1, 1, 3)
    if shifts:
        fB = fB + rng.randint(-2, 3, fB.shape) * (rng.uniform(size=(len(Z), 1)) < 0.5)
    perm = rng.permutation(len(Z)) if shuffle else np.arange(len(Z))
    return (Z[perm].copy(), fB[perm].copy(), MB), perm


def pack(structs):
    off = np.zeros(len(structs) + 1, np.int32)
    off[1:] = np.cumsum([len(s[0]) for s in structs])
    sp = np.concatenate([np.asarray(s[0], np.int32).reshape(-1) for s in structs])
    fr = np.concatenate([np.asarray(s[1], np.float64).reshape(-1, 3) for s in structs])
    return off, sp, fr, np.array([s[2] for s in structs], np.float64)


def prototypes(rng):
    """Six prototypes with n = 3, 5, 8, 20: four orthorhombic, one cubic, one with gamma = 120."""
    return [motif(rng, [8, 26, 26], lat([4.1, 5.3, 6.2])),
            motif(rng, [57, 26, 8, 8, 8], lat([5.0, 5.0, 5.0])),
            motif(rng, [57, 26, 8, 8, 8], lat([4.4, 5.6, 6.8])),
            motif(rng, [14, 14, 8, 8, 8, 8, 3, 3], lat([5.2, 6.1, 7.3])),
            motif(rng, [12] * 2 + [14] * 6 + [8] * 12, lat([7.0, 8.2, 9.1])),
            motif(rng, [22, 8, 8, 38, 8], lat([5.1, 5.1, 6.4], (90.0, 90.0, 120.0)))]


def sweep(seed=5, nq=40, nref=40):
    """40 queries and 40 references from the six prototypes: random op of the 24, translation, lattice shifts, order,
    and noise of two classes -- max residual 0.3 tol (the same structure) or one atom at 2.5 tol (another one)."""
    rng = np.random.RandomState(seed)
    protos = prototypes(rng)
    ops = MR.signed_permutations(1)
    out = []
    for k in range(nq + nref):
        A = protos[rng.randint(len(protos))]
        n = len(A[0])
        d = noise_max(rng, n, 0.3 * TOL) if rng.uniform() < 0.7 else noise_one(rng, n, rng.randint(n), 2.5 * TOL)
        out.append(derive(rng, A, ops[rng.randint(len(ops))], d)[0])
    return out


def robust(structs, nq, ops_mode=1, scales=(0.95, 1.05)):
    """(reference result at TOL / LTOL, list of compared pairs whose decision or chosen combination changes when tol and
    ltol are scaled)."""
    el = np.ones(len(structs), np.int32)
    base = MR.match_ref(structs, el, nq, TOL, LTOL, ops_mode)
    bad = []
    for s in scales:
        o = MR.match_ref(structs, el, nq, TOL * s, LTOL * s, ops_mode)
        assert sorted(o["pairs"]) == sorted(base["pairs"])
        for key, r in base["pairs"].items():
            r2 = o["pairs"][key]
            if (r["match"], r["op"], r["anchor"]) != (r2["match"], r2["op"], r2["anchor"]):
                bad.append((key, s))
    return base, bad
