"""Structures and fingerprint tables for the fingerprint tests.  Every builder that feeds an exact-integer comparison
asserts, on the CPU, the condition that comparison rests on: no pair within 1e-9 (relative) of R or of
(1 + cn_tol) nn_dist, and no row whose best and second-best partners are closer than 1e-9 (relative) unless bit-equal."""
import numpy as np

import structure_fingerprint_ref as FR
from structure_symmetry_cases import as_result, base_cases, lat, pack, random_p1, supercell   # noqa: F401

PARAMS = dict(r_max=6.0, n_bins=60, w=0.1, cn_tol=0.1)
GAP = 1e-9


def cubic(a=3.0, z=29):
    return np.array([z], np.int32), np.zeros((1, 3)), lat([a] * 3)


def triclinic5():
    return (np.array([22, 8, 8, 38, 8], np.int32),
            np.array([[0, 0, 0], [.3, .2, .1], [.6, .25, .8], [.45, .7, .4], [.85, .6, .15]], np.float64),
            lat([4.0, 5.0, 6.0], [80, 100, 70]))


def thin_long():
    """2.5 x 2.5 x 20 Angstrom: the image range differs per axis (3, 3, 1 at R = 6.1)."""
    return (np.array([14, 8, 8, 6], np.int32),
            np.array([[0.1, 0.2, 0.05], [0.6, 0.7, 0.3], [0.35, 0.15, 0.55], [0.8, 0.45, 0.81]], np.float64), lat([2.5, 2.5, 20.0]))


def too_dense():
    """A cell of 0.18 Angstrom: floor(6.1 / 0.18 + 1) = 34 images per axis, above the 32 the sweep covers."""
    return np.array([1], np.int32), np.array([[0.2, 0.3, 0.4]]), lat([0.18] * 3)


def sized(rng, n):
    """n atoms of three species at random; n = 1 has only its own images."""
    side = max(4.0, (12.0 * n) ** (1.0 / 3.0))
    Z, f, M = random_p1(rng, n, lat([side, side * 1.07, side * 0.93], [85, 95, 100]))
    Z = np.where(np.arange(n) % 3 == 1, 22, Z).astype(np.int32)
    return Z, f, M


def cell_cases():
    b = base_cases()
    return {"cubic3": cubic(), "hex": b["hcp"], "triclinic": triclinic5(), "thin_long": thin_long(), "perovskite": b["perovskite"]}


def ragged(seed=31, ns=300):
    """About 300 structures of 1..14 atoms with a few of 65..90 (the workgroup kernel), every seventh ineligible (some of
    them empty, one with 257 atoms that must not be looked at) and one whose image range is above 32.
    Returns (structs, eligible)."""
    rng = np.random.default_rng(seed)
    structs, el = [], []
    for s in range(ns):
        if s % 7 == 3:
            n = (0, 3, 257)[s % 3]
            structs.append((np.full(n, 8, np.int32), rng.uniform(size=(n, 3)), lat([5.0, 6.0, 7.0])))
            el.append(0)
            continue
        if s == 100:
            structs.append(too_dense())
        elif s % 50 == 10:
            structs.append(sized(rng, int(rng.integers(65, 91))))
        else:
            n = int(rng.integers(1, 15))
            abc = rng.uniform(3.0, 7.0, size=3)
            ang = rng.uniform(75.0, 105.0, size=3)
            Z, f, M = random_p1(rng, n, lat(abc, ang))
            Z = rng.choice([8, 14, 22, 38, 57], size=n).astype(np.int32)
            structs.append((Z, f + rng.integers(-2, 3, size=(n, 3)), M))         # unwrapped coordinates
        el.append(1)
    return structs, np.array(el, np.int32)


def assert_robust(ref):
    """The exact-integer comparison is a condition on the inputs: no pair near a threshold."""
    assert ref["gap"] > GAP, "a pair lies within %.1e (relative) of R or of (1 + cn_tol) nn_dist: %.3e" % (GAP, ref["gap"])
    return ref


def nearest_table(seed, nq, nref, length, invalid=(), duplicates=()):
    """fp (nq + nref, length), valid: smooth positive rows around a few centres (so nearest partners are not arbitrary);
    rows in `invalid` are marked invalid and filled with NaN (they must not be read); duplicates = [(dst, src)] copies
    row src onto row dst exactly."""
    rng = np.random.default_rng(seed)
    n = nq + nref
    centres = rng.uniform(0.0, 2.0, size=(5, length))
    fp = centres[rng.integers(0, 5, size=n)] + 0.3 * rng.normal(size=(n, length))
    for dst, src in duplicates:
        fp[dst] = fp[src]
    valid = np.ones(n, np.int32)
    for k in invalid:
        valid[k] = 0
        fp[k] = np.nan
    return fp, valid


def assert_separated(ref):
    assert ref["gap"] > GAP, "a row's best and second-best partners are within %.1e (relative): %.3e" % (GAP, ref["gap"])
    return ref


def rotated(S, k):
    """S under the k-th of the 24 proper signed axis permutations of its cell: the same crystal, another setting."""
    from icsg3d_amd.structures import signed_permutations
    P = signed_permutations(1)[k]
    Z, f, M = S
    # f' = P f in the cell M' = P M P^T: the Cartesian positions f'^T M' = (f^T M) P^T are the old ones rotated by P
    return Z, np.asarray(f) @ P.T, P @ np.asarray(M) @ P.T
