#!/usr/bin/env python3
"""interpolate.py (reference interpolate.py:67-202) on the MI355X engine: for every condition bin pick two crystals of
that bin at random, encode both, walk a line between their latent codes and decode every point on it -- all bins in ONE
call (icsg3d_amd.interpolate.interpolate_pairs: a device-resident chain per group of pairs).

Flags: the reference's, same names and defaults (interpolate.py:69-106): --name --ninterps --projection --enda --endb
--ncond.  As there, the pair of bin i is np.random.choice(ids of the bin, 2, replace=False) over pd.qcut bins of
formation_energy_per_atom from data/<name>/<name>.csv, endpoint a is <id>_rot_2.npy and b is <id>_rot_4.npy of
density_matrices/ (+ coordinate_grids/).  --enda / --endb are parsed and unused by the reference; they are accepted and
recorded in run.json.  --projection is recorded too (the 3D scatter needs the reference's interactive viz module).
Added: --synthetic (Gaussian-blob endpoints and, where no checkpoint exists under saved_models/, seeded random weights:
no dataset exists offline), --channels (the reference hard-codes 4), --d, --seed (pair choice and the sampling draws eps),
--mode lerp|slerp, --batch_size (engine batch), --atoms: every frame continued to atoms
(LatticeDFCVAE.interpolate_segment_atoms), per-frame coordinates written with generate.py's voxel -> Angstrom
conversion and the EMD between consecutive frames of each row (icsg3d_amd.evaluate.emd; NaN across a failed frame).

Writes output/interpolation/<name>_rows.npz (rows (ncond, ninterps + 2, d, d, d, C), zs (ncond, ninterps + 2, latent), ids,
formulae, alpha, mode; with --atoms also frame_emd (ncond, ninterps - 1), n_atoms, failed and atoms/<row>_<frame>.npy =
[species, x, y, z]) and run.json.  The reference's figure (row[j, :, :, 12, 0] per cell, the slice index scaled to d) is
written as output/interpolation/<name>_rows.svg only when matplotlib imports, with the Agg back end and no plt.show.  The
reference builds its file name as "interpolation" + mode -- a file NEXT to the folder it has just made; this script
writes inside the folder.

    python interpolate.py --name perovskite --enda CeCrO3 --endb YbCrO3
"""
import argparse
import json
import os
import sys

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--name", metavar="name", type=str, help="Name of data folder")
    p.add_argument("--ninterps", metavar="ninterps", type=int, help="Number of interpolations", default=8)
    p.add_argument("--projection", metavar="projection", type=str, help="Dimensionality of visualisation", default=None)
    p.add_argument("--enda", metavar="enda", type=str, help="End member of full interpolation", default="CeCrO3")
    p.add_argument("--endb", metavar="endb", type=str, help="End member of full interpolation", default="YbCrO3")
    p.add_argument("--ncond", metavar="ncond", type=int, help="Number of condition bins", default=10)
    p.add_argument("--synthetic", action="store_true", help="Gaussian-blob endpoints instead of data/<name>")
    p.add_argument("--channels", type=int, default=4, help="input channels (density + 3 coordinate grids)")
    p.add_argument("--d", type=int, default=32, help="Dimension of density matrices (number of voxels)")
    p.add_argument("--seed", type=int, default=0, help="seed of the pair choice and of the sampling draws eps")
    p.add_argument("--mode", choices=("lerp", "slerp"), default="lerp", help="the walk between the two latent codes")
    p.add_argument("--atoms", action="store_true", help="continue every frame to atoms; EMD between consecutive frames")
    p.add_argument("--batch_size", type=int, default=20, help="engine batch (the reference's _set_model(batch_size=20))")
    return p


def synthetic_pairs(ncond, d, C, seed):
    """one pair of Gaussian-blob grids per condition bin: A, B (ncond, d, d, d, C), ids, formulae"""
    from icsg3d_amd.synthetic import synthetic_batch
    X = synthetic_batch(2 * ncond, d, C, seed=seed)[0]
    ids = [("synthetic-%d" % (2 * i), "synthetic-%d" % (2 * i + 1)) for i in range(ncond)]
    return X[0::2], X[1::2], ids, ids


def dataset_pairs(name, ncond, d, C):
    """the reference's choice (interpolate.py:131-170); draws from np.random, seeded by the caller"""
    import pandas as pd
    data_path = os.path.join("data", name, "matrices")
    df = pd.read_csv(os.path.join("data", name, name + ".csv"))
    df["bin"] = pd.qcut(df["formation_energy_per_atom"], ncond, np.arange(ncond)).astype(int)
    A, B, ids, formulae = [], [], [], []
    for i in range(ncond):
        bin_ids = df[df["bin"] == i]["task_id"].values
        bin_formulae = df[df["bin"] == i]["pretty_formula"].values
        idxs = np.random.choice(np.arange(len(bin_ids)), 2, replace=False)
        pair = []
        for idx, rot in zip(idxs, ("_rot_2.npy", "_rot_4.npy")):
            M = np.load(os.path.join(data_path, "density_matrices", bin_ids[idx] + rot)).reshape(d, d, d, 1)
            if C > 1:
                G = np.load(os.path.join(data_path, "coordinate_grids", bin_ids[idx] + rot)).reshape(d, d, d, 3)
                M = np.concatenate([M, G], axis=-1)
            pair.append(M)
        A.append(pair[0]); B.append(pair[1])
        ids.append((str(bin_ids[idxs[0]]), str(bin_ids[idxs[1]])))
        formulae.append((str(bin_formulae[idxs[0]]), str(bin_formulae[idxs[1]])))
    return np.stack(A).astype(np.float32), np.stack(B).astype(np.float32), ids, formulae


def draw_eps(seed, ncond, latent):
    return np.random.RandomState(seed).normal(size=(ncond, 2, latent)).astype(np.float32)


def plot_rows(rows, formulae, n_interps, d, path):
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return False
    fig, axes = plt.subplots(len(rows), n_interps + 2, figsize=(15, 15), squeeze=False)
    for i, row in enumerate(rows):
        for j in range(n_interps + 2):
            if j == 0:
                axes[i][j].set_title(formulae[i][0], fontsize=12)
            if j == n_interps + 1:
                axes[i][j].set_title(formulae[i][1], fontsize=12)
            axes[i][j].imshow(row[j, :, :, (12 * d) // 32, 0])
            axes[i][j].set_xticks([])
            axes[i][j].set_yticks([])
    plt.subplots_adjust(bottom=0.05, top=0.95, hspace=0.3)
    plt.savefig(path, format="svg")
    plt.close(fig)
    return True


def main(argv=None):
    a = build_parser().parse_args(argv)
    from icsg3d_amd.cli import load_models
    from icsg3d_amd.interpolate import interpolate_pairs
    name, d, C, n = a.name, a.d, a.channels, a.ninterps
    projection = None if a.projection == "None" else a.projection
    out_dir = os.path.join("output", "interpolation")
    os.makedirs(out_dir, exist_ok=True)

    vae, unet = load_models(name, d, C, a.ncond, a.batch_size, a.synthetic, a.seed, a.atoms)
    np.random.seed(a.seed)
    if a.synthetic:
        A, B, ids, formulae = synthetic_pairs(a.ncond, d, C, a.seed)
    else:
        A, B, ids, formulae = dataset_pairs(name, a.ncond, d, C)
    conds = np.eye(a.ncond, dtype=np.float32)                      # to_categorical(i, ncond) for i in range(ncond)
    eps = draw_eps(a.seed, a.ncond, vae.latent_dim)
    alpha = np.linspace(0, 1, n)

    rows, zs = interpolate_pairs(A, B, conds, vae, num_interps=n, return_zs=True, mode=a.mode, eps=eps)
    extra = {}
    if a.atoms:
        from icsg3d_amd.evaluate import emd, predicted_coordinates
        out = vae.interpolate_segment_atoms(A, B, conds, unet, num_interps=n, mode=a.mode, eps=eps, thresh=0.8,
                                            min_voxels=3, max_atoms=2048, split=True)
        os.makedirs(os.path.join(out_dir, name + "_atoms"), exist_ok=True)
        xyz = []
        for f, mu in enumerate(predicted_coordinates(out["atoms"], out["coord_minmax"], d=d)):    # generate.py:237-241
            species = out["atoms"][f][0]
            if out["failed"][f]:
                mu = mu[:0]
            else:
                np.save(os.path.join(out_dir, name + "_atoms", "%d_%d.npy" % (f // n, f % n)),
                        np.concatenate([np.array(species, np.float64).reshape(-1, 1), mu], axis=-1))
            xyz.append(mu)
        frame_emd = np.full((a.ncond, max(n - 1, 0)), np.nan)
        pairs = [(p * n + k, p * n + k + 1) for p in range(a.ncond) for k in range(n - 1)
                 if not (out["failed"][p * n + k] or out["failed"][p * n + k + 1])]
        if pairs:
            e = emd([xyz[i] for i, _ in pairs], [xyz[j] for _, j in pairs])
            for (i, _), v in zip(pairs, e):
                frame_emd[i // n, i % n] = v
        extra = {"frame_emd": frame_emd, "n_atoms": np.where(out["failed"], -1, out["n_atoms"]).reshape(a.ncond, n),
                 "failed": np.asarray(out["failed"]).reshape(a.ncond, n)}

    np.savez(os.path.join(out_dir, name + "_rows.npz"), rows=rows, zs=zs, ids=np.array(ids, dtype=str),
             formulae=np.array(formulae, dtype=str), alpha=alpha, mode=np.array(a.mode), **extra)
    figure = projection is None and plot_rows(rows, formulae, n, d, os.path.join(out_dir, name + "_rows.svg"))
    with open(os.path.join(out_dir, "run.json"), "w") as f:
        json.dump(dict(vars(a), ids=ids, formulae=formulae, figure=bool(figure), rows_shape=list(rows.shape)), f, indent=1)
    print("wrote", os.path.join(out_dir, name + "_rows.npz"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
