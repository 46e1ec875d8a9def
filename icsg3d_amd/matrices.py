"""The arrays create_matrices.py builds per crystal, computed on the GPU (ics_op_voxelise, include/icsg3d.h):

- density M and species S       utils.density_matrix    (reference utils.py:97-144)
- coordinate grid p             utils.coordinate_grid   (reference utils.py:88-94)
- 90-degree rotations           utils.random_rotation_3d (reference utils.py:193-222), applied as np.rot90

in the reference's semantics (no periodic images, lattice angles ignored, float64).  There is no CPU fallback: every
grid comes from libicsg3d_hip.so.
"""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from . import _lib as L

ROTATION_AXES = ((0, 1), (0, 2), (1, 2))   # random_rotation_3d's axes_choices (utils.py:203)
MAX_SITES = 256                            # sites per structure the kernel stages


class Structures:
    """A batch of structures in the layout of ics_structures: [count][max_sites] site arrays, rows >= nsites[i]
    padded with NaN (never read).  xyz are cartesian (min-shifted fractional coordinates times abc), sigma the
    Gaussian widths."""

    def __init__(self, nsites, xyz, z, sigma, abc, lattice=None):
        self.nsites = np.ascontiguousarray(nsites, np.int32)
        self.xyz = np.ascontiguousarray(xyz, np.float64)
        self.z = np.ascontiguousarray(z, np.float64)
        self.sigma = np.ascontiguousarray(sigma, np.float64)
        self.abc = np.ascontiguousarray(abc, np.float64)
        n, ms = self.z.shape
        if (self.nsites.shape != (n,) or self.xyz.shape != (n, ms, 3) or self.sigma.shape != (n, ms)
                or self.abc.shape != (n, 3)):
            raise ValueError("inconsistent structure arrays")
        self.lattice = None if lattice is None else np.ascontiguousarray(lattice, np.float64)

    def __len__(self):
        return len(self.nsites)

    @classmethod
    def from_cartesian(cls, xyz_list, z_list, sigma_list, abc_list, lattice=None):
        """Per structure: cartesian sites (n,3), atomic numbers (n,), Gaussian widths (n,), lengths (3,)."""
        count = len(xyz_list)
        ms = max(1, max(len(np.atleast_1d(z)) for z in z_list))
        nsites = np.zeros(count, np.int32)
        xyz = np.full((count, ms, 3), np.nan)
        z = np.full((count, ms), np.nan)
        sigma = np.full((count, ms), np.nan)
        for i in range(count):
            zi = np.atleast_1d(np.asarray(z_list[i], np.float64))
            n = len(zi)
            nsites[i] = n
            xyz[i, :n] = np.asarray(xyz_list[i], np.float64).reshape(n, 3)
            z[i, :n] = zi
            sigma[i, :n] = np.broadcast_to(np.asarray(sigma_list[i], np.float64), (n,))
        abc = np.array([np.asarray(a, np.float64)[:3] for a in abc_list]).reshape(count, 3)
        return cls(nsites, xyz, z, sigma, abc, lattice)

    @classmethod
    def from_sites(cls, sites, sigma_frac=1.0):
        """sites: iterable of (frac_coords (n,3), Z (n,), ionic radii (n,), lattice (6,) = a, b, c, alpha, beta, gamma)
        as get_sites / crystal.lattice give them.  Applies get_sites' min-shift (utils.py:83-84), frac * abc
        (create_matrices.py:140) and sigma = sigma_frac * radii (create_matrices.py:150)."""
        xyz_l, z_l, s_l, abc_l, lat_l = [], [], [], [], []
        for frac, zz, radii, lattice in sites:
            N = np.asarray(frac, np.float64).reshape(-1, 3)
            N = N - np.min(N, axis=0)
            lattice = np.asarray(lattice, np.float64)
            xyz_l.append(np.multiply(N, lattice[:3]))
            z_l.append(np.asarray(zz, np.float64))
            s_l.append(sigma_frac * np.asarray(radii, np.float64))
            abc_l.append(lattice[:3])
            lat_l.append(lattice)
        return cls.from_cartesian(xyz_l, z_l, s_l, abc_l, lattice=np.array(lat_l).reshape(len(lat_l), -1))

    def c_struct(self):
        """The ics_structures view (valid while self lives)."""
        return L.Structures(len(self), self.z.shape[1], L.i32ptr(self.nsites), L.f64ptr(self.xyz), L.f64ptr(self.z),
                            L.f64ptr(self.sigma), L.f64ptr(self.abc))


def make_jobs(structs_or_count, rotations=None):
    """Job table [n][4] = {structure, r0, r1, r2}.  rotations: None (one unrotated job per structure) or (count, 3)
    rotation-axis indices per structure (-1 = none)."""
    count = structs_or_count if isinstance(structs_or_count, (int, np.integer)) else len(structs_or_count)
    jobs = np.full((count, 4), -1, np.int32)
    jobs[:, 0] = np.arange(count)
    if rotations is not None:
        jobs[:, 1:] = np.asarray(rotations, np.int32).reshape(count, 3)
    return jobs


def _jobs(structs, jobs, rotations):
    if jobs is None:
        jobs = make_jobs(structs, rotations)
    jobs = np.ascontiguousarray(jobs, np.int32)
    if jobs.ndim != 2 or jobs.shape[1] != 4 or len(jobs) < 1:
        raise ValueError("jobs must be (n, 4) int32 {structure, r0, r1, r2}, got %s" % (jobs.shape,))
    return jobs


def voxelise(structs: Structures, jobs=None, rotations=None, d=32, eps_frac=0.25, label_frac=1.0,
             want=("M", "S", "p")):
    """(M (n,d,d,d), S (n,d,d,d), p (n,d,d,d,3)) float64 for each job; outputs not in `want` are None."""
    jobs = _jobs(structs, jobs, rotations)
    n = len(jobs)
    M = np.empty((n, d, d, d)) if "M" in want else None
    S = np.empty((n, d, d, d)) if "S" in want else None
    p = np.empty((n, d, d, d, 3)) if "p" in want else None
    cs = structs.c_struct()
    L.check(L.load().ics_op_voxelise(C.byref(cs), L.i32ptr(jobs), n, int(d), float(eps_frac), float(label_frac),
                                     L.f64ptr(M), L.f64ptr(S), L.f64ptr(p)))
    return M, S, p


def density_matrix(N, z, l, dims=(32, 32, 32), sigma=0.5, dist=None, label_frac=1.0, eps_frac=0.25):
    """utils.density_matrix (utils.py:97-144): cartesian sites N (n,3), atomic numbers z, lengths l -> (M, S), each
    of shape dims.  Euclidean distance only (the reference's default); cubic grids only."""
    if dist is not None and getattr(dist, "__name__", "") != "euclidean":
        raise ValueError("only the euclidean distance is implemented")
    dims = tuple(int(v) for v in dims)
    if len(dims) != 3 or len(set(dims)) != 1:
        raise ValueError("cubic grids only, got dims=%s" % (dims,))
    s = Structures.from_cartesian([N], [z], [sigma], [l])
    M, S, _ = voxelise(s, d=dims[0], eps_frac=eps_frac, label_frac=label_frac, want=("M", "S"))
    return M[0], S[0]


def coordinate_grid(l, dim=32, eps_frac=0.25):
    """utils.coordinate_grid (utils.py:88-94): (dim, dim, dim, 3) float64."""
    s = Structures.from_cartesian([np.zeros((1, 3))], [0.0], [1.0], [l])
    _, _, p = voxelise(s, d=int(dim), eps_frac=eps_frac, want=("p",))
    return p[0]


def load_sites(path):
    """(frac (n,3), Z, radii, lattice (6,)) of one data/<name>/sites/<id>.npz, float64"""
    f = np.load(path)
    frac = np.asarray(f["frac_coords"], np.float64).reshape(-1, 3)
    return frac, np.asarray(f["Z"], np.float64), np.asarray(f["radii"], np.float64), np.asarray(f["lattice"], np.float64)


def accept(fname, frac, radii, max_sites):
    """The reference's per-structure rules (create_matrices.py:117-145): False = skip; an out-of-cell coordinate
    raises SystemExit naming the file."""
    if len(frac) > max_sites:
        return False
    N = frac - np.min(frac, axis=0)
    if not np.all((N <= 1.0) & (N >= 0)):
        print(fname, N)
        sys.stdout.flush()
        raise SystemExit("%s: fractional coordinates outside [0, 1] after the min-shift" % fname)
    if any(np.isnan(radii)):
        return False
    return True
