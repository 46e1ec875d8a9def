#!/usr/bin/env python3
"""eval.py (reference eval.py:130-227) on the MI355X engine: reconstruct every validation structure through the VAE,
segment it with the U-Net and watershed_clustering, and score it against the true crystal --

    EMD          the optimal one-to-one matching of predicted and true atom positions in Angstrom (eval.py:45-53),
                 one device launch per batch (icsg3d_amd.evaluate.emd -> ics_op_match_emd);
    lattice      |a, b, c true - predicted|;
    atom count   |N true - N predicted|.

Per batch, vae.model.predict -> unet.model.predict -> argmax / 0.8 threshold -> components run as one device-resident
chain (VaeEngine.reconstruct_to_atoms); the convexity test and the recursive split follow on the host (refine_atoms,
--clus_iters).  A sample whose segmentation fails is left out of every metric, as the reference's except: continue.

Flags: the reference's, same names and defaults (eval.py:57-111): --name --batch_size --samples --eps_frac --ncond
--clus_iters --split --d.  The validation ids are the reference's (data_split(..., n_rot=0), whole batches of
VAEDataGenerator(shuffle=False), qcut condition bins from data/<name>/<name>.csv).  True structures come from
data/<name>/sites/<id>.npz, the input create_matrices.py reads (CIF parsing needs pymatgen and stays outside this repo):
true lattice = lattice[:3], true positions = the min-shifted frac * abc.  Lattice parameters are read with the engine's d
(the reference hard-codes 32; the same at d = 32).
Added: --channels (the reference hard-codes 4); --from_sites: voxelise sites/ on the device straight into the VAE's
resident batch instead of reading matrices/ (--sigma_frac / --label_frac / --max_sites: create_matrices.py's, used only
then); --seed: the sampling draws eps.
Writes output/eval/<name>/metrics.json (counts, means, arguments) and per_sample.npz (ids, EMD, true / predicted lattice
and atom counts, the predicted atoms: species and Angstrom coordinates packed with offsets).  The reference's plots are
not drawn.

    python eval.py --name heusler --samples 5000
"""
import argparse
import json
import os
import sys

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--name", metavar="name", type=str, help="Name of data folder")
    p.add_argument("--batch_size", metavar="batch_size", type=int, help="Batch size", default=10)
    p.add_argument("--samples", metavar="samples", type=int, help="Number of samples", default=78750)
    p.add_argument("--eps_frac", metavar="eps_frac", type=float, help="Eps of lattice vector", default=0.25)
    p.add_argument("--ncond", metavar="ncond", type=int, help="Number of condition bins", default=10)
    p.add_argument("--clus_iters", metavar="clus_iters", type=int, help="Number of iterations for watershed clustering",
                   default=5)
    p.add_argument("--split", metavar="split", type=float, help="Train-test split fraction", default=0.8)
    p.add_argument("--d", metavar="d", type=int, help="Dimension of density matrices (number of voxels)", default=32)
    p.add_argument("--channels", type=int, default=4, help="input channels (density + 3 coordinate grids)")
    p.add_argument("--from_sites", action="store_true", help="voxelise data/<name>/sites on the device instead of "
                   "reading data/<name>/matrices")
    p.add_argument("--sigma_frac", type=float, default=1.0, help="--from_sites: fraction of ionic radius used as "
                   "Gaussian width (create_matrices.py)")
    p.add_argument("--label_frac", type=float, default=1.0, help="--from_sites: fraction of ionic radius to label in "
                   "species matrices (create_matrices.py)")
    p.add_argument("--max_sites", type=int, default=40, help="--from_sites: structures with more sites are skipped, as "
                   "create_matrices.py does")
    p.add_argument("--seed", type=int, default=0, help="seed of the sampling draws eps")
    return p


def load_true(sites_dir, ids, sigma_frac):
    """Structures of the ids' site files (stem of "<id>.npy") and their (frac, Z, radii, lattice) tuples."""
    from icsg3d_amd.matrices import Structures, load_sites
    sites = [load_sites(os.path.join(sites_dir, os.path.splitext(i)[0] + ".npz")) for i in ids]
    return Structures.from_sites(sites, sigma_frac=sigma_frac), sites


def site_listing(sites_dir, max_sites):
    """The "<id>.npy" names create_matrices.py would write for sites_dir (its skip rules), sorted."""
    from icsg3d_amd.matrices import accept, load_sites
    names = []
    for fname in sorted(f for f in os.listdir(sites_dir) if f.endswith(".npz")):
        frac, _, radii, _ = load_sites(os.path.join(sites_dir, fname))
        if accept(fname, frac, radii, max_sites):
            names.append(os.path.splitext(fname)[0] + ".npy")
    return sorted(names)


def main(argv=None):
    a = build_parser().parse_args(argv)
    from icsg3d_amd.cli import load_models
    from icsg3d_amd.evaluate import reconstruction_metrics
    from icsg3d_amd.utils import data_split, data_split_names
    from icsg3d_amd.vae.data import VAEDataGenerator
    from icsg3d_amd.watershed import refine_atoms

    mode, d, C, bs, eps = a.name, a.d, a.channels, a.batch_size, a.eps_frac
    data_path = os.path.join("data", mode, "matrices")
    sites_dir = os.path.join("data", mode, "sites")
    csv_path = os.path.join("data", mode, mode + ".csv")
    out_dir = os.path.join("output", "eval", mode)
    os.makedirs(out_dir, exist_ok=True)

    if a.from_sites:
        _, validation_ids = data_split_names(site_listing(sites_dir, a.max_sites), a.samples, frac=a.split, n_rot=0)
    else:
        _, validation_ids = data_split(data_path, a.samples, frac=a.split, n_rot=0)
    gen = VAEDataGenerator(validation_ids, data_path=data_path, property_csv=csv_path, batch_size=bs, dim=(d, d, d),
                           n_channels=C, shuffle=False, n_bins=a.ncond)

    vae, unet = load_models(mode, d, C, a.ncond, bs, False, a.seed, True)
    rng = np.random.RandomState(a.seed)

    ids_out, failed_ids, emds, lt, lpred, nt, npred, species, coords = [], [], [], [], [], [], [], [], []
    for k in range(len(gen)):
        ids = gen.list_IDs[k * bs:(k + 1) * bs]
        eps_draw = rng.normal(size=(bs, vae.latent_dim))
        structs, sites = load_true(sites_dir, ids, a.sigma_frac)
        if a.from_sites:
            from icsg3d_amd.matrices import make_jobs
            cond = np.stack([gen.property_to_categorical(i) for i in ids])
            eng = vae._engine(bs)
            ueng = unet._engine(bs)
            eng.voxelise_batch(structs, make_jobs(len(ids)), cond, eps_draw, eps_frac=eps, label_frac=a.label_frac)
            out = eng.reconstruct_to_atoms(ueng, thresh=0.8, min_voxels=3, max_atoms=2048, want_regions=True)
            refine_atoms(out, max_iters=a.clus_iters, num_species=unet.num_classes)
        else:
            M, cond = gen[k]
            out = vae.reconstruct_segment_atoms(M, cond, unet, eps=eps_draw, thresh=0.8, min_voxels=3, max_atoms=2048,
                                                split=True, max_iters=a.clus_iters)
        true_xyz = [structs.xyz[i, :structs.nsites[i]] for i in range(len(ids))]
        true_lat = np.array([s[3][:3] for s in sites])
        m = reconstruction_metrics(out["atoms"], out["coord_minmax"], true_xyz, true_lat, out["failed"], eps, d)
        for i in np.flatnonzero(~m["keep"]):
            print(ids[i], "failed")
            failed_ids.append(ids[i])
        ids_out += [ids[i] for i in np.flatnonzero(m["keep"])]
        emds.append(m["emd"]); lt.append(m["lattice_true"]); lpred.append(m["lattice_pred"])
        nt.append(m["n_true"]); npred.append(m["n_pred"]); species += m["species"]; coords += m["coords"]

    emds = np.concatenate(emds) if emds else np.zeros(0)
    lt = np.concatenate(lt) if lt else np.zeros((0, 3))
    lpred = np.concatenate(lpred) if lpred else np.zeros((0, 3))
    nt = np.concatenate(nt) if nt else np.zeros(0, np.int64)
    npred = np.concatenate(npred) if npred else np.zeros(0, np.int64)
    dn = np.abs(nt - npred)
    dl = np.abs(lt - lpred)
    print("\nMEAN EMD: ", np.mean(emds))
    print("\nMEAN DAtoms: ", np.mean(dn))

    off = np.zeros(len(coords) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in coords])
    np.savez(os.path.join(out_dir, "per_sample.npz"), ids=np.array(ids_out, dtype=str), emd=emds, lattice_true=lt,
             lattice_pred=lpred, n_true=nt, n_pred=npred, atom_offsets=off,
             atom_species=np.concatenate(species) if species else np.zeros(0, np.int64),
             atom_xyz=np.concatenate(coords) if coords else np.zeros((0, 3)),
             failed_ids=np.array(failed_ids, dtype=str))
    with np.errstate(all="ignore"):
        metrics = {"evaluated": int(len(emds)), "failed": len(failed_ids), "mean_emd": float(np.mean(emds)),
                   "mean_datoms": float(np.mean(dn)), "mean_da": float(np.mean(dl[:, 0])),
                   "mean_db": float(np.mean(dl[:, 1])), "mean_dc": float(np.mean(dl[:, 2])), "args": vars(a)}
    with open(os.path.join(out_dir, "metrics.json"), "w") as f:
        json.dump(metrics, f, indent=1)
    print("wrote", out_dir)
    return 0


if __name__ == "__main__":
    sys.exit(main())
