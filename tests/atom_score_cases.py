"""Inputs of the atom-score tests (tests/test_atom_score_host.py, tests/test_gpu_atom_score.py): atom sets with generic
and with integer-lattice positions, the many-round chain, and label volumes with planted boxes.  Builders only."""
import numpy as np

SIZES = (0, 1, 2, 63, 64, 65, 257, 1024)
# (n_true, n_pred) drawn from SIZES x SIZES: both empty, each side empty, every size on each side, 1024 on both
SIZE_PAIRS = ((0, 0), (0, 1), (1, 0), (1, 1), (2, 1), (1, 2), (2, 2), (63, 64), (64, 63), (64, 64), (65, 64), (64, 65),
              (65, 257), (257, 65), (257, 257), (1024, 0), (0, 1024), (1024, 1), (2, 1024), (1024, 257), (63, 1024),
              (1024, 1024))


def species(n, ncls, rng, zeros=False):
    s = rng.integers(0, ncls, size=n)
    if zeros and n:
        s[rng.uniform(size=n) < 0.2] = 0                                # species 0 on the predicted side
    return s.astype(np.int32)


def generic_sample(n, m, rng):
    """uniform fp64 positions at a density at which an atom has one or two partners within 1.5: picks collide"""
    side = 2.0 * max(n, m, 1) ** (1.0 / 3.0)
    return rng.uniform(0.0, side, size=(n, 3)), rng.uniform(0.0, side, size=(m, 3))


def lattice_sample(n, m, rng, box=4):
    """integer positions in a box^3 box: ties at every distance, coincident points on both sides"""
    return rng.integers(0, box, size=(n, 3)).astype(np.float64), rng.integers(0, box, size=(m, 3)).astype(np.float64)


def batch(kind, pairs, ncls, seed):
    """-> (T, TS, P, PS): lists with one array per sample"""
    rng = np.random.default_rng(seed)
    make = generic_sample if kind == "generic" else lattice_sample
    T, TS, P, PS = [], [], [], []
    for n, m in pairs:
        t, p = make(n, m, rng)
        T.append(t); P.append(p)
        TS.append(species(n, ncls, rng)); PS.append(species(m, ncls, rng, zeros=True))
    return T, TS, P, PS


def chain(n=64):
    """the 1-D chain that takes exactly n rounds at tol 1.5: gaps shrink along the chain, so only the last free pair is
    mutually best in every round -> (true (n, 3), predicted (n, 3))"""
    gaps = np.array([1.0 - j * 0.5 / (2 * n) for j in range(2 * n - 1)])
    x = np.concatenate([[0.0], np.cumsum(gaps)])
    z = np.zeros(n)
    return np.stack([x[1::2], z, z], 1), np.stack([x[0::2], z, z], 1)


def _box(vol, b, z, y, x, value, off):
    vol[b, off + z[0]:off + z[1], off + y[0]:off + y[1], off + x[0]:off + x[1]] = value


def volumes(d):
    """(true_labels, pred_species, pred_mask) uint8 (3, d, d, d) for d = 8 or 16, min_voxels 3, tol 2.0, and what is planted:
    sample 0: an exact hit (species 3), a blob shifted by one voxel (5), one of the wrong species (true 7, predicted 9), one
              true atom (4) whose prediction a zero plane splits in two;
    sample 1: two true atoms (6, 8) bridged by one predicted blob, and a 3-voxel component (2): dropped on the predicted
              side, kept on the true side;
    sample 2: empty.  Blobs keep at least one empty voxel between them in every direction, diagonals included."""
    off = 0 if d == 8 else 5
    lab = np.zeros((3, d, d, d), np.uint8)
    sp, mk = lab.copy(), lab.copy()
    _box(lab, 0, (0, 2), (0, 2), (0, 2), 3, off); _box(sp, 0, (0, 2), (0, 2), (0, 2), 3, off); _box(mk, 0, (0, 2), (0, 2), (0, 2), 1, off)
    _box(lab, 0, (0, 2), (0, 2), (4, 6), 5, off); _box(sp, 0, (0, 2), (0, 2), (5, 7), 5, off); _box(mk, 0, (0, 2), (0, 2), (5, 7), 200, off)
    _box(lab, 0, (0, 2), (4, 6), (0, 2), 7, off); _box(sp, 0, (0, 2), (4, 6), (0, 2), 9, off); _box(mk, 0, (0, 2), (4, 6), (0, 2), 1, off)
    _box(lab, 0, (4, 8), (0, 2), (0, 2), 4, off); _box(sp, 0, (4, 8), (0, 2), (0, 2), 4, off)
    _box(mk, 0, (4, 5), (0, 2), (0, 2), 1, off); _box(mk, 0, (6, 8), (0, 2), (0, 2), 1, off)          # plane z = 5 is zero
    _box(lab, 1, (0, 2), (0, 2), (0, 2), 6, off); _box(lab, 1, (0, 2), (0, 2), (3, 5), 8, off)
    _box(sp, 1, (0, 2), (0, 2), (0, 5), 6, off); _box(mk, 1, (0, 2), (0, 2), (0, 5), 1, off)
    _box(lab, 1, (4, 5), (4, 5), (4, 7), 2, off); _box(sp, 1, (4, 5), (4, 5), (4, 7), 2, off); _box(mk, 1, (4, 5), (4, 5), (4, 7), 1, off)
    return lab, sp, mk


def volumes_failed(d):
    """sample 0: three atoms (true and predicted); sample 1: empty; sample 2: one exact hit.  At max_atoms = 2 sample 0 fails."""
    off = 0 if d == 8 else 5
    lab = np.zeros((3, d, d, d), np.uint8)
    for k, (y, x) in enumerate(((0, 0), (0, 4), (4, 0))):
        _box(lab, 0, (0, 2), (y, y + 2), (x, x + 2), 3 + k, off)
    _box(lab, 2, (2, 4), (2, 4), (2, 4), 11, off)
    return lab, lab.copy(), (lab != 0).astype(np.uint8)


def random_tallies(ncls, rng, scale=50):
    """a tally block with arbitrary counts (not the result of a matching: the report only divides)"""
    M = rng.integers(0, scale, size=(ncls + 1, ncls + 1)).astype(np.int64)
    M[ncls, ncls] = 0
    det = M[:ncls, :ncls].sum(1)
    return {"matrix": M, "dist_q": (det * rng.uniform(0, 2, ncls) * (1 << 20)).astype(np.int64),
            "dist2_q": (det * rng.uniform(0, 4, ncls) * (1 << 20)).astype(np.int64),
            "dup": rng.integers(0, 5, ncls).astype(np.int64), "shadowed": rng.integers(0, 5, ncls).astype(np.int64),
            "hist": rng.integers(0, scale, 16).astype(np.int64),
            "totals": np.array([40, 3, 11, M[:ncls].sum(), M[:, :ncls].sum(), M[:ncls, :ncls].sum(), 17, 2], np.int64)}
