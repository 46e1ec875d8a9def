#!/usr/bin/env python3
"""Hot-path portion of /root/reference/generate.py on the MI355X engine: encode a base compound, sample
z ~ N(z_mean, var), decode, segment with the U-Net, argmax species + 0.8 binary threshold, then connected
components + majority vote + centroids -- one device-resident chain per batch (generate.py:196-236 ->
ics_vae_decode_to_unet_atoms) -- and watershed_clustering's convexity test + recursive marker watershed for the
non-convex components (icsg3d_amd/watershed.py; the scikit-image routines behind it are restated, parity unpinned).
Written under output/results/<formula>__v=<var>/: densities, species, binary masks, voxel parameters and per-sample
atom coordinates (.npy).  Then the reference's structure stage (generate.py:250-318, utils.py:225-239) without pymatgen:
every batch is screened in one device call (icsg3d_amd.structures.screen -> ics_op_structure_screen: the periodic
structure in the --alpha/--beta/--gamma cell, exact shortest periodic distances, is_valid's 0.5 A rule), and per valid
sample cifs/<formula_count>.cif, a row of results.csv (sorted by id) and a results.json record are written; a sample with
no atoms, a species outside 1..94 or no usable cell is counted invalid, not raised.  pymatgen's semantics are restated,
parity with it is unpinned.  CGCNN property prediction and the oxidation-state guess ("charge
balanced") stay out of scope.

Flags: the reference's, same names and defaults (generate.py:52-102): --name --base --batch_size --nsamples --var
--eps_frac --clus_iters --alpha --beta --gamma --target --ncond --d.  --alpha/--beta/--gamma are the angles of the cell
the structures are screened and written in (to_pymatgen_structure); --clus_iters is watershed_clustering's max_iters.
--eps_frac goes where the reference puts it: the shift of the atom coordinates (generate.py:237-241); like the
reference, to_lattice_params / to_voxel_params keep their default 0.25 (generate.py:211,214).
Added: --channels (the reference hard-codes 4) and --synthetic (a Gaussian-blob base compound, condition bin
--cond_bin; no dataset exists offline).  --match (with --match_tol, --match_ltol, --match_ops {none,rot,all}): after the
last batch all written samples are matched in one device call (icsg3d_amd.structures.match -> ics_op_structure_match,
the project's own predicate): against each other for duplicates and against data/<name>/sites/*.npz
for training hits; results.csv gains duplicate_of, duplicate_rms, training_match, training_rms, match_reason and run.json
a `match` block with the parameters, the ineligible counts by reason and the validity / uniqueness / novelty rates.
--synthetic runs have no site folder and report duplicates only.
--symmetry (with --sym_tol, --sym_ltol, --sym_max_ops): after the last batch (and after --match, with which it
composes) the symmetry of all written samples is found in one device call plus its retry rounds
(icsg3d_amd.structures.symmetry -> ics_op_structure_symmetry, the project's own predicate): results.csv
gains point_group, crystal_system, n_symops, n_centring, sym_shift, sym_tol, sym_reason; cifs_sym/<id>.cif holds the
symmetrised structure with its operations and asymmetric unit; run.json gains a `symmetry` block with the parameters, the
counts by point group and crystal system, the base compound's own point group when data/<name>/sites/<base id>.npz
exists, and the share of symmetrised samples that keep it.  No space-group name or number is produced.
--fingerprint (with --fp_rmax, --fp_bins, --fp_width, --fp_cn_tol and, repeatable, --fp_delta): after the last batch (and
after --match and --symmetry, with which it composes) every written sample gets a structural fingerprint -- its radial
distribution function, plain and Z-weighted, and the coordination numbers of its atoms -- in one device call
(icsg3d_amd.structures.fingerprint -> ics_op_structure_fingerprint, the project's own descriptor; no
parity with pymatgen's or matminer's fingerprints is claimed), the structures of data/<name>/sites/*.npz get theirs (the
reference set --match builds, built once when both flags are given), and one more call finds every nearest partner
(ics_op_fingerprint_nearest): results.csv gains nearest_training, nearest_training_dist, nearest_generated,
nearest_generated_dist, cn_mean, cn_min, cn_max, fp_reason; fingerprints.npz holds the fingerprints; run.json gains a
`fingerprint` block with the parameters, the numbers fingerprinted, the diversity (mean distance between two samples), the
quantiles of the nearest distances and, for every --fp_delta, coverage recall and precision.  There is no default delta:
the scale of these distances on real data has not been measured.  --synthetic runs have no site folder and report the
sample-to-sample columns only.
"""
import argparse
import json
import os
import sys

import numpy as np

from icsg3d_amd.cli import checkpoint_paths
from icsg3d_amd.evaluate import predicted_coordinates
from icsg3d_amd.structures import OPS_MODES, Fingerprinter, Matcher, ReferenceSet, ResultsWriter, Symmetriser
from icsg3d_amd.synthetic import synthetic_batch
from icsg3d_amd.utils import to_lattice_params_from_minmax, to_voxel_params
from icsg3d_amd.unet.unet import AtomUnet
from icsg3d_amd.vae.lattice_vae import LatticeDFCVAE


def base_compound_from_csv(csv_path, base, target, ncond):
    """generate.py:112-137,190-191: the base compound's task id, formula, target value and qcut condition bin."""
    import pandas as pd
    df = pd.read_csv(csv_path)
    df["interval"] = pd.qcut(df[target], ncond, np.arange(ncond))
    if base.startswith("mp-"):
        formula = df[df["task_id"] == base]["pretty_formula"].values[0]
        task_id = base
    else:
        formula = df[df["pretty_formula"] == base]["pretty_formula"].values[0]
        task_id = df[df["pretty_formula"] == base]["task_id"].values[0]
    row = df[df["task_id"] == task_id]
    return task_id, formula, float(row[target].values[0]), int(row["interval"].values[0])


def training_formulas(csv_path):
    """generate.py:139: the pretty_formula column of the dataset's CSV (the `training` flag of a generated formula)."""
    import pandas as pd
    return set(pd.read_csv(csv_path)["pretty_formula"].values)


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--name", metavar="name", type=str, help="Name of data folder")
    p.add_argument("--base", metavar="base", type=str, help="Base Compound", default="LaFeO3")
    p.add_argument("--batch_size", metavar="batch_size", type=int, help="Batch size", default=100)
    p.add_argument("--nsamples", metavar="nsamples", type=int, help="Number of samples", default=100)
    p.add_argument("--var", metavar="var", type=float, help="Variance of sampling", default=0.5)
    p.add_argument("--eps_frac", metavar="eps_frac", type=float, help="Eps of lattice vector", default=0.25)
    p.add_argument("--clus_iters", metavar="clus_iters", type=int, help="Iterations of Clustering", default=5)
    p.add_argument("--alpha", metavar="alpha", type=int, help="alpha", default=90)
    p.add_argument("--beta", metavar="beta", type=int, help="beta", default=90)
    p.add_argument("--gamma", metavar="gamma", type=int, help="gamma", default=90)
    p.add_argument("--target", metavar="target", type=str, default="formation_energy_per_atom")
    p.add_argument("--ncond", metavar="ncond", type=int, help="Number of condition bins", default=10)
    p.add_argument("--d", "--dim", dest="d", metavar="d", type=int, help="Number of map voxels", default=32)
    p.add_argument("--channels", type=int, default=4, help="input channels (density + 3 coordinate grids)")
    p.add_argument("--synthetic", action="store_true", help="Gaussian-blob base compound instead of data/<name>")
    p.add_argument("--cond_bin", type=int, default=0, help="--synthetic: condition bin of the base compound")
    p.add_argument("--match", action="store_true", help="match the written samples: duplicates and training structures")
    p.add_argument("--match_tol", type=float, default=0.1, help="--match: site tolerance in Angstrom")
    p.add_argument("--match_ltol", type=float, default=0.05, help="--match: relative tolerance on the metric tensor")
    p.add_argument("--match_ops", choices=sorted(OPS_MODES), default="rot",
                   help="--match: cell operations tried (none, the 24 rotations, all 48 signed axis permutations)")
    p.add_argument("--symmetry", action="store_true", help="find the symmetry of the written samples and write cifs_sym/")
    p.add_argument("--sym_tol", type=float, default=0.1, help="--symmetry: site tolerance in Angstrom")
    p.add_argument("--sym_ltol", type=float, default=0.05, help="--symmetry: relative tolerance on the metric tensor")
    p.add_argument("--sym_max_ops", type=int, default=192, help="--symmetry: operations kept per structure")
    p.add_argument("--fingerprint", action="store_true",
                   help="fingerprint the written samples: nearest training structure, nearest sample, coverage, diversity")
    p.add_argument("--fp_rmax", type=float, default=6.0, help="--fingerprint: range of the distribution function in Angstrom")
    p.add_argument("--fp_bins", type=int, default=60, help="--fingerprint: number of bins (1..256)")
    p.add_argument("--fp_width", type=float, default=0.1, help="--fingerprint: half-width of the deposit kernel in Angstrom")
    p.add_argument("--fp_cn_tol", type=float, default=0.1, help="--fingerprint: neighbour-distance slack of the coordination number")
    p.add_argument("--fp_delta", type=float, action="append", default=None,
                   help="--fingerprint: a distance to report coverage recall / precision at (repeatable; no default)")
    return p


def base_point_group(sites_path, symmetriser):
    """The point group the symmetriser finds for the structure stored in a sites file (None if it finds none)."""
    from icsg3d_amd.matrices import load_sites
    frac, Z, _, lattice = load_sites(sites_path)
    ref = ReferenceSet(["base"], [np.rint(Z).astype(np.int32)], [frac], [np.asarray(lattice, np.float64).reshape(-1)[:6]])
    res = symmetriser(ref.screened())[0]
    return res["point_group"] if res["sym_reason"] == 0 else None


def main(argv=None):
    a = build_parser().parse_args(argv)

    mode, d, C, bs, eps = a.name, a.d, a.channels, a.batch_size, a.eps_frac
    path = os.path.join("data", mode, "matrices")
    vae_weights, unet_weights, perceptual_model = checkpoint_paths(mode)

    if a.synthetic:
        base_compound, base_formula, base_target_value, cond_bin = "synthetic", "synthetic", None, a.cond_bin
        M_base = synthetic_batch(1, d, C, seed=0)[0]
    else:
        base_compound, base_formula, base_target_value, cond_bin = base_compound_from_csv(
            os.path.join("data", mode, mode + ".csv"), a.base, a.target, a.ncond)
        M_base = np.load(os.path.join(path, "density_matrices", base_compound + ".npy")).reshape(1, d, d, d, 1)
        if C > 1:
            C_base = np.load(os.path.join(path, "coordinate_grids", base_compound + ".npy")).reshape(1, d, d, d, 3)
            M_base = np.concatenate([M_base, C_base], axis=-1)
    cond = np.zeros((1, a.ncond), np.float32)
    cond[0, cond_bin] = 1.0

    out_dir = os.path.join("output", "results", base_formula + "_" + "_v=" + str(a.var))
    for sub in ("densities", "species", "binary", "voxel_params", "coords"):
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    shown = {k: v for k, v in vars(a).items() if (a.match or not k.startswith("match"))     # without the flags: today's keys
             and (a.symmetry or not k.startswith("sym")) and (a.fingerprint or not k.startswith(("fp_", "fingerprint")))}
    run_info = dict(shown, base_compound=base_compound, base_formula=base_formula, base_target=base_target_value,
                    cond_bin=cond_bin)
    with open(os.path.join(out_dir, "run.json"), "w") as f:
        json.dump(run_info, f)

    vae = LatticeDFCVAE(input_shape=(d, d, d, C), perceptual_model=perceptual_model, cond_shape=a.ncond)
    vae._set_model(vae_weights, batch_size=bs)
    unet = AtomUnet(weights=unet_weights, input_shape=(d, d, d, C), max_batch=bs)

    z_mu_base, z_logvar_base, z_base = vae.encoder.predict([M_base, cond])
    n_atoms = []
    training_names = set() if a.synthetic else training_formulas(os.path.join("data", mode, mode + ".csv"))
    matcher = reference = None
    if (a.match or a.fingerprint) and not a.synthetic:        # one reference set for both
        sites = os.path.join("data", mode, "sites")
        reference = ReferenceSet.from_sites(sites) if os.path.isdir(sites) else None
    if a.match:
        matcher = Matcher(reference, a.match_tol, a.match_ltol, OPS_MODES[a.match_ops])
    symmetriser = Symmetriser(a.sym_tol, a.sym_ltol, a.sym_max_ops) if a.symmetry else None
    fingerprinter = (Fingerprinter(reference, a.fp_rmax, a.fp_bins, a.fp_width, a.fp_cn_tol, a.fp_delta or ())
                     if a.fingerprint else None)
    results = ResultsWriter(out_dir, a.alpha, a.beta, a.gamma, training_names=training_names,
                            target_value=base_target_value, matcher=matcher, symmetriser=symmetriser,
                            fingerprinter=fingerprinter)
    for batch in range(int(a.nsamples / bs)):
        print("Batch", batch)
        z_samples = np.random.normal(z_mu_base, a.var, size=(bs, vae.latent_dim))
        # generate.py:204-236 as one device-resident chain: decoder -> U-Net -> argmax / 0.8 threshold -> connected
        # components (> 3 voxels) -> majority vote + centroids.  The reconstruction and the label volumes stay in HBM;
        # back come 2 bytes per voxel, the density channel, the coordinate channels' min / max (all to_lattice_params
        # reads, generate.py:211-217) and one row of integers per atom.
        # then, per sample, the convexity test and the recursive marker watershed of the non-convex components
        # (watershed.py:76-150, --clus_iters): icsg3d_amd/watershed.py.  A sample that fails is skipped like in the
        # reference ("Failed", continue: generate.py:228-236)
        out = vae.decode_segment_atoms(z_samples, np.tile(cond, (bs, 1)), unet, thresh=0.8, min_voxels=3, max_atoms=2048,
                                       split=True, max_iters=a.clus_iters)
        l_prime = to_lattice_params_from_minmax(out["coord_minmax"], d=d)
        dv_pred = to_voxel_params(l_prime, d=d)
        xyz = predicted_coordinates(out["atoms"], out["coord_minmax"], eps, d)         # generate.py:237-241
        batch_atoms = [None] * bs
        for i in range(bs):
            k = batch * bs + i
            if out["failed"][i]:
                print("Failed", k)
                continue
            species_sample, mu = out["atoms"][i][0], xyz[i]
            coords = np.concatenate([np.array(species_sample, np.float64).reshape(-1, 1), mu], axis=-1)
            n_atoms.append(len(species_sample))
            np.save(os.path.join(out_dir, "densities", "%d.npy" % k), out["density"][i])
            np.save(os.path.join(out_dir, "species", "%d.npy" % k), out["species"][i])
            np.save(os.path.join(out_dir, "binary", "%d.npy" % k), out["mask"][i])
            np.save(os.path.join(out_dir, "voxel_params", "%d.npy" % k), dv_pred[i])
            np.save(os.path.join(out_dir, "coords", "%d.npy" % k), coords)
            batch_atoms[i] = (species_sample, mu)
        # generate.py:250-318: structure, formula, is_valid, CIF and results row -- the batch screened in one device call
        results.add_batch(range(batch * bs, batch * bs + bs), l_prime, batch_atoms)
    counts = results.finish()
    print("structures: generated %(generated)d / failed %(failed)d / invalid %(invalid)d / written %(written)d" % counts)
    if matcher is not None:
        compared = counts["written"] - counts["ineligible"]
        run_info["match"] = dict(
            tol=a.match_tol, ltol=a.match_ltol, ops=a.match_ops, references=len(matcher.reference) if matcher.reference else 0,
            unique=counts["unique"], novel=counts["novel"] if matcher.reference else None, ineligible=counts["ineligible"],
            ineligible_by_reason=results.match_summary["ineligible_by_reason"],
            validity=counts["written"] / counts["generated"] if counts["generated"] else None,
            uniqueness=counts["unique"] / compared if compared else None,
            novelty=counts["novel"] / counts["unique"] if matcher.reference and counts["unique"] else None)
        with open(os.path.join(out_dir, "run.json"), "w") as f:
            json.dump(run_info, f)
        print("match: unique %d / novel %s / ineligible %d of %d written" % (
            counts["unique"], counts["novel"] if matcher.reference else "n/a", counts["ineligible"], counts["written"]))
    if symmetriser is not None:
        summary = results.symmetry_summary
        base_sites = os.path.join("data", mode, "sites", base_compound + ".npz")
        base_pg = base_point_group(base_sites, symmetriser) if not a.synthetic and os.path.isfile(base_sites) else None
        kept = summary["by_point_group"].get(base_pg, 0) if base_pg is not None else None
        run_info["symmetry"] = dict(
            tol=a.sym_tol, ltol=a.sym_ltol, max_ops=a.sym_max_ops, symmetrised=summary["symmetrised"],
            by_point_group=summary["by_point_group"], by_crystal_system=summary["by_crystal_system"],
            base_point_group=base_pg, keep_base_point_group=kept,
            keep_base_share=kept / summary["symmetrised"] if kept is not None and summary["symmetrised"] else None)
        with open(os.path.join(out_dir, "run.json"), "w") as f:
            json.dump(run_info, f)
        print("symmetry: %d of %d written symmetrised; point groups %s" % (
            summary["symmetrised"], counts["written"], summary["by_point_group"]))
    if fingerprinter is not None:
        summary = results.fingerprint_summary
        run_info["fingerprint"] = summary
        with open(os.path.join(out_dir, "run.json"), "w") as f:
            json.dump(run_info, f)
        print("fingerprint: %d of %d written fingerprinted against %d references; diversity %s" % (
            summary["samples"], counts["written"], summary["references"], summary["diversity"]))
    print("wrote", out_dir, "- atoms per sample: mean %.1f" % (np.mean(n_atoms) if n_atoms else 0.0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
