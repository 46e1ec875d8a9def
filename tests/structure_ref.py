"""fp64 restatement of the structure stage of generate.py (to_pymatgen_structure + structure.is_valid(), reference
generate.py:250-263, utils.py:225-239) that the GPU tests hold ics_op_structure_screen to.  pymatgen's semantics as the
project states them (parity with pymatgen itself is unpinned: no fixture was recorded from it):

- Lattice.from_parameters(a, b, c, alpha, beta, gamma): rows va = [a sin(beta), 0, a cos(beta)],
  vb = [-b sin(alpha) cos(g), b sin(alpha) sin(g), b cos(alpha)], vc = [0, 0, c],
  g = arccos(clamp((cos(alpha) cos(beta) - cos(gamma)) / (sin(alpha) sin(beta)), -1, 1)); sine and cosine of exactly 90
  degrees are 1 and 0.
- the atoms are placed with the 90-degree lattice (frac = xyz / abc) and keep their fractional coordinates when the
  lattice is swapped.
- is_valid(tol): one site is valid; otherwise min over i < j of the shortest periodic distance > tol.

The shortest periodic distance is found by brute force over +-`images` translations per axis of the wrapped fractional
difference: slow, simple, and independent of the kernel's range derivation.
"""
import itertools

import numpy as np


def lattice_from_parameters(a, b, c, alpha, beta, gamma):
    ang = np.array([alpha, beta, gamma], np.float64)
    sn = np.where(ang == 90.0, 1.0, np.sin(np.radians(ang)))
    cs = np.where(ang == 90.0, 0.0, np.cos(np.radians(ang)))
    val = np.clip((cs[0] * cs[1] - cs[2]) / (sn[0] * sn[1]), -1.0, 1.0)
    gs = np.arccos(val)
    return np.array([[a * sn[1], 0.0, a * cs[1]],
                     [-b * sn[0] * np.cos(gs), b * sn[0] * np.sin(gs), b * cs[0]],
                     [0.0, 0.0, float(c)]], np.float64)


def lattice_parameters(M):
    """(a, b, c, alpha, beta, gamma) back from the rows of M."""
    ln = np.linalg.norm(M, axis=1)
    ang = [np.degrees(np.arccos(np.clip(np.dot(M[i], M[j]) / (ln[i] * ln[j]), -1, 1))) for i, j in ((1, 2), (0, 2), (0, 1))]
    return tuple(ln) + tuple(ang)


def pair_distances(frac, M, images=4):
    """(n, n) shortest periodic distances by brute force over (2 images + 1)^3 translations."""
    frac = np.asarray(frac, np.float64).reshape(-1, 3)
    w = frac - np.floor(frac)
    df = w[None, :, :] - w[:, None, :]
    df -= np.round(df)
    best = np.full(df.shape[:2], np.inf)
    for n in itertools.product(range(-images, images + 1), repeat=3):
        v = (df + np.array(n, np.float64)) @ M
        best = np.minimum(best, np.sqrt((v * v).sum(-1)))
    return best


def pair_distances_27(frac, M):
    """The 27-neighbour shortcut over coordinates wrapped into [0, 1): NOT exact for skewed cells."""
    frac = np.asarray(frac, np.float64).reshape(-1, 3)
    w = frac - np.floor(frac)
    df = w[None, :, :] - w[:, None, :]
    best = np.full(df.shape[:2], np.inf)
    for n in itertools.product((-1, 0, 1), repeat=3):
        v = (df + np.array(n, np.float64)) @ M
        best = np.minimum(best, np.sqrt((v * v).sum(-1)))
    return best


def screen_ref(species, xyz, abc, angles, tol=0.5, images=4):
    """One structure: dict(lattice, volume, frac, min_dist, min_pair, n_close, valid, reason, nearest, hist, second) --
    `second` is the second-smallest pair distance (inf below two pairs) and `pairs` the distances of all pairs i < j in
    row-major order, for the tests' tie margins."""
    species = np.asarray(species, np.int64).reshape(-1)
    n = len(species)
    xyz = np.asarray(xyz, np.float64).reshape(n, 3)
    abc = np.asarray(abc, np.float64)
    M = lattice_from_parameters(*abc, *angles)
    frac = xyz / abc
    inside = (species >= 1) & (species <= 94)
    hist = np.bincount(species[inside], minlength=95).astype(np.int32)
    reason = (0 if inside.all() else 2) | (4 if n == 0 else 0)
    out = {"lattice": M, "volume": float(np.linalg.det(M)), "frac": frac, "hist": hist, "min_dist": np.inf,
           "min_pair": (-1, -1), "n_close": 0, "nearest": np.full(n, np.inf), "second": np.inf,
           "pairs": np.zeros(0)}
    if n >= 2:
        D = pair_distances(frac, M, images)
        iu = np.triu_indices(n, 1)
        d = out["pairs"] = D[iu]
        k = int(np.argmin(d))                    # first occurrence in row-major order = lexicographically smallest pair
        out["min_dist"], out["min_pair"] = float(d[k]), (int(iu[0][k]), int(iu[1][k]))
        out["n_close"] = int((d <= tol).sum())
        out["second"] = float(np.sort(d)[1]) if len(d) > 1 else np.inf
        np.fill_diagonal(D, np.inf)
        out["nearest"] = D.min(axis=1)
        if out["n_close"]:
            reason |= 1
    out["reason"], out["valid"] = reason, int(reason == 0)
    return out
