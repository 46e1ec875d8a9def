"""create_matrices.py (reference create_matrices.py) on the GPU: the density matrices, species matrices, lattice
vectors and coordinate grids (and --nrot randomly rotated copies of each) that train_unet.py / train_vae.py read.

Input: data/<name>/sites/<id>.npz per structure with frac_coords (n,3), Z (n,), radii (n,) (ionic radii) and
lattice (6,) = a, b, c, alpha, beta, gamma -- what get_sites / crystal.lattice give for a CIF (INTEGRATION.md shows the
three pymatgen lines; CIF parsing itself needs pymatgen and stays outside this repo).
Output: data/<name>/matrices/{density_matrices,species_matrices,lattice_vectors,coordinate_grids}/<id>[_rot_k].npy,
float64, in the reference's shapes.

The reference's host rules apply (create_matrices.py:117-145): structures with more than --max_sites sites and those
with a NaN radius are skipped; a min-shifted fractional coordinate outside [0, 1] stops the run (non-zero exit, naming
the file).  Each rotated copy's three axes are np.random.RandomState(--seed).choice(3, 3), drawn per structure in id
order; the grids of --batch structures x (1 + nrot) jobs come from one device call.

    python create_matrices.py --name heusler --d 32 --nrot 10
"""
import argparse
import os
import sys

import numpy as np

from icsg3d_amd import matrices
from icsg3d_amd.matrices import accept, load_sites

KINDS = ("density_matrices", "species_matrices", "lattice_vectors", "coordinate_grids")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--name", type=str, required=True, help="Name of data folder")
    p.add_argument("--d", type=int, default=32, help="Dimensionality of the matrices")
    p.add_argument("--nrot", type=int, default=10, help="Number of rotations to apply")
    p.add_argument("--label_frac", type=float, default=1.0, help="Fraction of ionic radius to label in species matrices")
    p.add_argument("--sigma_frac", type=float, default=1.0, help="Fraction of ionic radius to use as Gaussian width")
    p.add_argument("--eps_frac", type=float, default=0.25, help="Fraction of unit cell to add along each dimension")
    p.add_argument("--max_sites", type=int, default=40, help="Maximum number of sites in the unit cell")
    p.add_argument("--seed", type=int, default=0, help="Seed of the rotation-axis draws")
    p.add_argument("--batch", type=int, default=8, help="Structures per device call")
    p.add_argument("--root", type=str, default="data", help="Directory holding <name>/")
    return p.parse_args(argv)


def write_batch(sdir, ids, sites, rots, a):
    """Voxelise len(ids) structures x (1 + nrot) jobs in one call and save every array."""
    structs = matrices.Structures.from_sites(sites, sigma_frac=a.sigma_frac)
    jobs = []
    for i in range(len(ids)):
        jobs.append((i, -1, -1, -1))
        jobs += [(i, *r) for r in rots[i]]
    jobs = np.array(jobs, np.int32)
    M, S, p = matrices.voxelise(structs, jobs=jobs, d=a.d, eps_frac=a.eps_frac, label_frac=a.label_frac)
    j = 0
    for i, sid in enumerate(ids):
        lattice_vector = np.asarray(sites[i][3], np.float64)
        for k in range(-1, len(rots[i])):
            name = sid if k < 0 else "%s_rot_%d" % (sid, k)
            np.save(os.path.join(sdir, "density_matrices", name), M[j])
            np.save(os.path.join(sdir, "species_matrices", name), S[j])
            np.save(os.path.join(sdir, "lattice_vectors", name), lattice_vector)
            np.save(os.path.join(sdir, "coordinate_grids", name), p[j])
            j += 1


def main(argv=None):
    a = parse_args(argv)
    if a.d < 2 or a.nrot < 0 or a.batch < 1 or not 1 <= a.max_sites <= matrices.MAX_SITES:
        raise SystemExit("bad arguments: need --d >= 2, --nrot >= 0, --batch >= 1, 1 <= --max_sites <= %d"
                         % matrices.MAX_SITES)
    src = os.path.join(a.root, a.name, "sites")
    sdir = os.path.join(a.root, a.name, "matrices")
    for k in KINDS:
        os.makedirs(os.path.join(sdir, k), exist_ok=True)
    rng = np.random.RandomState(a.seed)
    files = sorted(f for f in os.listdir(src) if f.endswith(".npz"))
    ids, sites, rots = [], [], []
    written = skipped = 0
    for fname in files:
        frac, Z, radii, lattice = load_sites(os.path.join(src, fname))
        if not accept(fname, frac, radii, a.max_sites):
            skipped += 1
            continue
        ids.append(os.path.splitext(fname)[0])
        sites.append((frac, Z, radii, lattice))
        rots.append([tuple(int(v) for v in rng.choice(3, 3)) for _ in range(a.nrot)])
        if len(ids) == a.batch:
            write_batch(sdir, ids, sites, rots, a)
            written += len(ids)
            ids, sites, rots = [], [], []
    if ids:
        write_batch(sdir, ids, sites, rots, a)
        written += len(ids)
    print("create_matrices: %d structures written (%d files each), %d skipped -> %s"
          % (written, 1 + a.nrot, skipped, sdir))
    return 0


if __name__ == "__main__":
    sys.exit(main())
