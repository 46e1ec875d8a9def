"""Structures for the symmetry tests: the seven named cases with the counts the predicate gives them, noisy and shifted
versions, supercells, random P1 cells, the 84-structure sweep, and packing for the op."""
import numpy as np

from icsg3d_amd.structures import cell

TOL, LTOL = 0.1, 0.05


def lat(abc, angles=(90, 90, 90)):
    return cell(abc, angles)[0]


def base_cases():
    """name -> (Z, frac, M)"""
    na = [[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]]
    cl = [[.5, .5, .5], [0, 0, .5], [0, .5, 0], [.5, 0, 0]]
    c = {
        "perovskite": ([57, 26, 8, 8, 8], [[0, 0, 0], [.5, .5, .5], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]], lat([3.9] * 3)),
        "rocksalt": ([11] * 4 + [17] * 4, na + cl, lat([5.6] * 3)),
        "hcp": ([12, 12], [[1 / 3, 2 / 3, .25], [2 / 3, 1 / 3, .75]], lat([3.2, 3.2, 5.2], [90, 90, 120])),
        "tetragonal": ([22, 8, 8], [[0, 0, 0], [.3, .3, 0], [.7, .7, 0]], lat([4.0, 4.0, 6.0])),
        "monoclinic": ([22, 8, 8], [[0, 0, 0], [.3, .2, .1], [.7, .2, .9]], lat([4.0, 5.0, 6.0], [90, 100, 90])),
        "triclinic": ([22, 8, 8], [[0, 0, 0], [.3, .2, .1], [.6, .25, .8]], lat([4.0, 5.0, 6.0], [80, 100, 70])),
        "fcc_prim": ([29], [[0.1, 0.2, 0.3]], lat([4.0] * 3, [60, 60, 60])),
    }
    return {k: (np.array(Z, np.int32), np.array(f, np.float64), M) for k, (Z, f, M) in c.items()}


# name -> (n_ops, n_point, n_trans, point group) at tol 0.1, ltol 0.05
EXPECT = {"perovskite": (48, 48, 1, "m-3m"), "rocksalt": (192, 48, 4, "m-3m"), "hcp": (24, 24, 1, "6/mmm"),
          "tetragonal": (8, 8, 1, "mmm"), "monoclinic": (2, 2, 1, "2"), "triclinic": (1, 1, 1, "1"),
          "fcc_prim": (48, 48, 1, "m-3m")}
EXPECT_N_LAT = {"tetragonal": 16}
NAMES = tuple(EXPECT)


def noisy(rng, S, level, shift=True, tol=TOL):
    """S with a random origin shift and, per atom, a displacement of length level * tol in a random direction."""
    Z, f, M = S
    f = f + (rng.normal(size=3) if shift else 0.0)
    if level > 0:
        e = rng.normal(size=f.shape)
        e *= level * tol / np.linalg.norm(e, axis=1)[:, None]
        f = f + e @ np.linalg.inv(M)
    return Z, f, M


def supercell(S, reps):
    Z, f, M = S
    reps = np.asarray(reps)
    sh = np.array([[i, j, k] for i in range(reps[0]) for j in range(reps[1]) for k in range(reps[2])], np.float64)
    # species-major keeps equal species together, as the base cells have them
    zz = np.repeat(Z, len(sh))
    ff = ((f[:, None, :] + sh[None, :, :]) / reps).reshape(-1, 3)
    return zz.astype(np.int32), ff, M * reps[:, None]


def random_p1(rng, n, M, dmin=0.45):
    """n atoms at random with every periodic distance above dmin; one Sr (the unique rarest species), the rest O."""
    f = np.zeros((0, 3))
    while len(f) < n:
        p = rng.uniform(size=3)
        D = f - p
        D -= np.rint(D)
        if len(f) == 0 or np.sqrt(((D @ M) ** 2).sum(1)).min() > dmin:
            f = np.vstack([f, p])
    Z = np.full(n, 8, np.int32)
    Z[n // 3] = 38
    return Z, f, M


def add_atom(rng, S, dmin=0.45):
    Z, f, M = S
    while True:
        p = rng.uniform(size=3)
        D = f - p
        D -= np.rint(D)
        if np.sqrt(((D @ M) ** 2).sum(1)).min() > dmin:
            return np.append(Z, 8).astype(np.int32), np.vstack([f, p]), M


def sweep(seed=11):
    """84 structures: the seven cases x four origin shifts x noise {0, 0.2, 0.4} tol."""
    rng = np.random.default_rng(seed)
    base = base_cases()
    out = []
    for name in NAMES:
        for rep in range(4):
            for lvl in (0.0, 0.2, 0.4):
                out.append((name, lvl, noisy(rng, base[name], lvl)))
    return out


def pack(structs):
    off = np.zeros(len(structs) + 1, np.int32)
    off[1:] = np.cumsum([len(s[0]) for s in structs])
    return (off, np.concatenate([np.asarray(s[0], np.int32) for s in structs]),
            np.concatenate([np.asarray(s[1], np.float64).reshape(-1, 3) for s in structs]),
            np.array([s[2] for s in structs], np.float64))


def as_result(S, tol=TOL):
    """A dict in the layout icsg3d_amd.structures.screen returns, for symmetry() and ResultsWriter on the host."""
    Z, f, M = S
    n = len(Z)
    md = np.inf
    fw = f - np.floor(f)
    for i in range(n):
        D = fw - fw[i]
        D -= np.rint(D)
        d = np.sqrt(((D @ M) ** 2).sum(1))
        d[i] = np.inf
        if n > 1:
            md = min(md, d.min())
    G = M @ M.T
    abc = np.sqrt(np.diag(G))
    ang = np.degrees(np.arccos([G[1, 2] / abc[1] / abc[2], G[0, 2] / abc[0] / abc[2], G[0, 1] / abc[0] / abc[1]]))
    if n == 1:
        md = float(min(abc))
    return {"species": np.asarray(Z, np.int32), "frac": np.asarray(f, np.float64), "abc": abc, "angles": ang,
            "lattice": np.asarray(M, np.float64), "volume": float(np.linalg.det(M)), "min_dist": float(md),
            "hist": np.bincount(Z, minlength=95).astype(np.int32), "valid": True, "reason": 0}


def ref_packed(MR):
    """symmetry_packed's signature on the restatement: what symmetry(packed=...) takes on a machine without a GPU."""
    def run(offsets, species, frac, lattice, eligible, tol, ltol, max_ops):
        structs = [(species[offsets[k]:offsets[k + 1]], frac[offsets[k]:offsets[k + 1]], np.asarray(lattice[k]).reshape(3, 3))
                   for k in range(len(offsets) - 1)]
        return MR.symmetry_ref(structs, eligible, tol, ltol, max_ops)
    return run
