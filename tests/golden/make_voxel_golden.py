"""Generates tests/golden/voxel_golden.npz by running the REFERENCE's own voxeliser on seeded structures.

  ** reference functions, run as they stand **  The reference's utils.py cannot be imported (pymatgen, func_timeout,
  skimage, sklearn absent).  Its `coordinate_grid`, `density_matrix` and `random_rotation_3d` need only numpy, scipy
  and itertools: the three FunctionDefs are pulled out of the file with `ast`, their decorators (func_timeout's
  180 s limit) dropped, compiled and executed.  It is the reference's code that runs -- none of its text is written to
  the repo; the fixture is data (inputs and the arrays the reference returns).

  Cases: d = 16 / 32 / 64, 1-40 sites, sigma wide enough that the two-sites-in-radius branch of the species loop is
  common, a site exactly on a voxel centre, label_frac 0.6 / 1.0, eps_frac 0.25 / 0.1.  Rotations (d = 16):
  np.random.seed(s) before random_rotation_3d; the axes it drew are recorded by replaying np.random.seed(s);
  np.random.choice(3, 3).

  What is stored, to keep the file small (fp64 densities barely compress): S in full for every case; M in full at
  d = 16, on two i-planes at d = 32 and one at d = 64 (M_idx_<i>); p as its three axes (p[i, j, k] =
  (px[i], py[j], pz[k]), checked exactly here); rotated copies in full.

    python tests/golden/make_voxel_golden.py <reference checkout>
"""
import ast
import os
import sys
from itertools import product

import numpy as np
import scipy
import scipy.ndimage
from scipy.spatial.distance import cdist, euclidean

HERE = os.path.dirname(os.path.abspath(__file__))
WANT = ("coordinate_grid", "density_matrix", "random_rotation_3d")


def load_reference(ref_utils):
    tree = ast.parse(open(ref_utils).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANT]
    assert sorted(f.name for f in fns) == sorted(WANT)
    for f in fns:
        f.decorator_list = []
    mod = ast.Module(body=fns, type_ignores=[])
    # scipy.ndimage.interpolation.rotate is the reference's spelling of scipy.ndimage.rotate
    ns = {"np": np, "scipy": scipy, "product": product, "cdist": cdist, "euclidean": euclidean}
    exec(compile(mod, ref_utils, "exec"), ns)
    return ns


# (d, nsites, sigma_frac, label_frac, eps_frac, site on a voxel centre, rotations)
CASES = [
    (16, 1, 1.0, 1.0, 0.25, False, 0),
    (16, 5, 1.0, 0.6, 0.1, False, 1),
    (16, 40, 1.5, 1.0, 0.1, False, 1),
    (16, 12, 2.5, 0.6, 0.25, False, 0),
    (32, 12, 2.5, 1.0, 0.25, False, 0),
    (32, 20, 1.0, 0.6, 0.25, False, 0),
    (32, 6, 1.0, 1.0, 0.25, True, 0),
    (64, 8, 1.0, 1.0, 0.25, False, 0),
]


def main():
    ref = load_reference(os.path.join(sys.argv[1], "utils.py"))
    rng = np.random.default_rng(2020)
    n, ms = len(CASES), max(c[1] for c in CASES)
    out = dict(d=np.array([c[0] for c in CASES], np.int32), nsites=np.array([c[1] for c in CASES], np.int32),
               label_frac=np.array([c[3] for c in CASES]), eps_frac=np.array([c[4] for c in CASES]),
               xyz=np.full((n, ms, 3), np.nan), z=np.full((n, ms), np.nan), sigma=np.full((n, ms), np.nan),
               abc=np.zeros((n, 3)))
    rot_case, rot_seed, rot_axes = [], [], []
    for i, (d, ns, sf, lf, ef, on_centre, nrot) in enumerate(CASES):
        abc = rng.uniform(3.0, 9.0, 3)
        frac = rng.uniform(0.0, 1.0, (ns, 3))
        frac = frac - frac.min(axis=0)                      # get_sites' min-shift (utils.py:83-84)
        N = frac * abc                                      # create_matrices.py:140
        if on_centre:                                       # site 0 exactly on the centre of voxel (3, 5, 7)
            for ax, idx in enumerate((3, 5, 7)):
                a = abc[ax]
                c = np.linspace(-a * ef, a + (a * ef), d + 1)[:-1][idx] + ((a + (2 * a * ef)) / d) / 2
                N[0, ax] = c
        z = rng.integers(1, 95, ns).astype(np.float64)
        sigma = sf * rng.uniform(0.5, 2.0, ns)
        M, S = ref["density_matrix"](N, z, l=list(abc), sigma=sigma, dims=(d, d, d), label_frac=lf, eps_frac=ef)
        p = ref["coordinate_grid"](abc, dim=d, eps_frac=ef)
        out["xyz"][i, :ns], out["z"][i, :ns], out["sigma"][i, :ns], out["abc"][i] = N, z, sigma, abc
        midx = np.arange(d) if d == 16 else (np.array([3, d // 2]) if d == 32 else np.array([d // 2]))
        px, py, pz = p[:, 0, 0, 0], p[0, :, 0, 1], p[0, 0, :, 2]
        assert np.array_equal(np.stack(np.meshgrid(px, py, pz, indexing="ij"), -1), p)
        out["M_%d" % i], out["M_idx_%d" % i], out["S_%d" % i] = M[midx], midx, S
        out["px_%d" % i], out["py_%d" % i], out["pz_%d" % i] = px, py, pz
        for r in range(nrot):
            seed = 1000 * i + r
            np.random.seed(seed)
            Mr, Sr, pr = ref["random_rotation_3d"](M, S, p)
            np.random.seed(seed)
            axes = np.random.choice(3, 3)
            k = len(rot_case)
            out["rot_M_%d" % k], out["rot_S_%d" % k], out["rot_p_%d" % k] = Mr, Sr, pr
            rot_case.append(i), rot_seed.append(seed), rot_axes.append(axes)
        print("case %d: d=%d sites=%d S>0 %d voxels, rotations %d" % (i, d, ns, int((S > 0).sum()), nrot))
    out["rot_case"] = np.array(rot_case, np.int32)
    out["rot_seed"] = np.array(rot_seed, np.int64)
    out["rot_axes"] = np.array(rot_axes, np.int32).reshape(-1, 3)
    path = os.path.join(HERE, "voxel_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
