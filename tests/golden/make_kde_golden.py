#!/usr/bin/env python3
"""Records tests/golden/kde_golden.npz from scipy.stats.gaussian_kde (scipy 1.15.3 when this was run): the densities the
reference's plot_kde (vae/lattice_vae.py:359-386) would draw for float32 codes the tests regenerate from seeds.

    python tests/golden/make_kde_golden.py          (CPU, needs scipy; a few seconds)

Cases (n, dim) = (2, 1), (3, 3), (65, 5), (1000, 256), (1025, 2): `codes(name)` below builds each from its seed; the small
ones are stored too, the two large ones only as a float64 checksum (their codes would be a megabyte).  One column of the
n = 65 and n = 1000 cases is narrow (sigma = 1e-3 around 0.03), so every grid value underflows to exactly 0.
  dens_<name>      gaussian_kde(z[:, j])(x) for every column j, x = linspace(-3, 3, 50)
  dens_65x5_p1, dens_65x5_p65   the n = 65 case on the one-point grid [0.5] and on linspace(-3, 3, 65)
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# name: (seed, n, dim, narrow column or None)
CASES = {"2x1": (1, 2, 1, None), "3x3": (2, 3, 3, None), "65x5": (3, 65, 5, 3), "1000x256": (4, 1000, 256, 7),
         "1025x2": (5, 1025, 2, None)}
STORED = ("2x1", "3x3", "65x5")
X50 = np.linspace(-3, 3, 50)
X1 = np.array([0.5])
X65 = np.linspace(-3, 3, 65)
NARROW_MEAN, NARROW_SIGMA = 0.03, 1e-3


def codes(name):
    seed, n, dim, narrow = CASES[name]
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, dim)) * rng.uniform(0.3, 1.5, dim) + rng.uniform(-1.0, 1.0, dim)
    if narrow is not None:
        z[:, narrow] = NARROW_MEAN + NARROW_SIGMA * rng.standard_normal(n)
    return z.astype(np.float32)


def scipy_density(z, x):
    from scipy.stats import gaussian_kde
    return np.stack([gaussian_kde(z[:, j].astype(np.float64))(x) for j in range(z.shape[1])])


def main():
    out = {"x50": X50, "x1": X1, "x65": X65}
    for name in CASES:
        z = codes(name)
        out["sum_" + name] = np.float64(z.astype(np.float64).sum())
        if name in STORED:
            out["codes_" + name] = z
        out["dens_" + name] = scipy_density(z, X50)
    z = codes("65x5")
    out["dens_65x5_p1"] = scipy_density(z, X1)
    out["dens_65x5_p65"] = scipy_density(z, X65)
    for name in ("65x5", "1000x256"):
        assert (out["dens_" + name][CASES[name][3]] == 0).all(), "the narrow column must underflow to exactly 0"
    path = os.path.join(HERE, "kde_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
