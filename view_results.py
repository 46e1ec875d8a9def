#!/usr/bin/env python3
"""view_results.py (reference view_results.py:93-189) on the MI355X engine: for validation samples, one sheet of eight
pictures that shows every stage of the pipeline, true side above and VAE reconstruction below --

    M True | S True        | WS True | Coords True
    M Pred | S pred        | WS Pred | Coords Pred        (with the sample's MSE and F1 in the captions)

It is the tool to open when a trained model gives a poor MEAN EMD: it shows which link of the chain went wrong.  The
reference opens a TkAgg window, blocks on input("...") and shrinks every density to 10^3 because ax.voxels draws one
polygon set per voxel; here every panel is a ray cast of the full-resolution volume on the GPU (icsg3d_amd.render) and
the sheets are written as files.  The M panels are rendered from the engine's resident batch and reconstruction where
they lie in device memory (VaeEngine.render_resident); the label and atom panels go through ics_op_render_labels /
ics_op_render_atoms.  The pictures are this project's own: no parity with matplotlib's renderer is claimed.

Per batch the true side runs through watershed_clustering(..., return_ws=True) and the predicted side through one
reconstruct_to_atoms(want_regions=True) chain plus refine_atoms.  A sample whose segmentation fails on either side is
skipped and counted, as the reference's except: continue.  MSE is the mean over all channels of the sample
(mean_squared_error, view_results.py:132-134) from vae.model.predict; F1 is f1_m of the U-Net on the reconstruction
against the true labels (view_results.py:137), one sample at a time.

Flags: the reference's, same names and defaults: --name --batch_size --nrot --samples --split --d.
Added: --channels (the reference hard-codes 4); --synthetic (Gaussian-blob samples and, where no checkpoint exists under
saved_models/, seeded random weights); --count N samples to render (replaces the input("...") loop); --size pixels per
panel side; --elev --azim the camera; --mode value|flat for the M panels (flat: the reference's uniform alpha = 0.2 fog);
--out; --seed (shuffle, sampling draws).
Writes <out>/<id>.png (the 2x4 sheet), <out>/<id>.json (captions, mse, f1, atom counts, failure flags), index.html and
run.json.

    python view_results.py --name heusler --count 8
"""
import argparse
import html
import json
import os
import sys

import numpy as np

TITLES = ("M True", "S True", "WS True", "Coords True", "M Pred, MSE = %.3f", "S pred F1 = %.3f", "WS Pred",
          "Coords Pred")


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--name", metavar="name", type=str, help="Name of data folder")
    p.add_argument("--batch_size", metavar="batch_size", type=int, help="Batch size", default=1)
    p.add_argument("--nrot", metavar="nrot", type=int, help="nrot", default=10)
    p.add_argument("--samples", metavar="samples", type=int, help="Number of samples", default=78750)
    p.add_argument("--split", metavar="split", type=float, help="Train-test split fraction", default=0.8)
    p.add_argument("--d", metavar="d", type=int, help="Dimension of density matrices (number of voxels)", default=32)
    p.add_argument("--channels", type=int, default=4, help="input channels (density + 3 coordinate grids)")
    p.add_argument("--synthetic", action="store_true", help="Gaussian-blob samples instead of data/<name>")
    p.add_argument("--count", type=int, default=8, help="validation samples to render")
    p.add_argument("--size", type=int, default=256, help="pixels per panel side")
    p.add_argument("--elev", type=float, default=30.0, help="camera elevation in degrees (matplotlib's)")
    p.add_argument("--azim", type=float, default=-60.0, help="camera azimuth in degrees (matplotlib's)")
    p.add_argument("--mode", choices=("value", "flat"), default="value", help="M panels: opacity from the density, or "
                   "the reference's flat alpha")
    p.add_argument("--out", type=str, default=None, help="output folder (default output/view/<name>)")
    p.add_argument("--seed", type=int, default=0, help="seed of the shuffle and of the sampling draws eps")
    return p


def batches(a, ncond):
    """Yields (ids, M, cond, S uint8 (B,d,d,d), S_b (B,d,d,d)) per batch of validation samples."""
    d, C, bs = a.d, a.channels, a.batch_size
    if a.synthetic:
        from icsg3d_amd.synthetic import synthetic_batch
        for k in range(max(4 * a.count, 8)):                   # a few spare batches for skipped samples
            X, S, cond = synthetic_batch(bs, d, C, seed=a.seed + k)
            yield ["synthetic-%d" % (k * bs + i) for i in range(bs)], X, cond[:, :ncond], S, (S != 0)
        return
    from icsg3d_amd.utils import data_split
    from icsg3d_amd.vae.data import VAEDataGenerator
    path = os.path.join("data", a.name, "matrices")
    _, validation_ids = data_split(path, a.samples, frac=a.split, n_rot=a.nrot)
    np.random.seed(a.seed)                                     # the generator shuffles with np.random, as the reference
    gen = VAEDataGenerator(validation_ids, data_path=path, property_csv=os.path.join("data", a.name, a.name + ".csv"),
                           batch_size=bs, dim=(d, d, d), n_channels=C, shuffle=True, return_S=True, n_bins=ncond)
    for M, t in gen:
        yield list(gen.list_IDs_temp), M, t[0], t[1], t[2][..., 0] != 0


def atom_set(species, means):
    """(species, voxel-index means) -> what render.atoms takes: a voxel's index is its corner, its centre is +0.5."""
    xyz = np.asarray(means, np.float64).reshape(-1, 3) + 0.5
    return np.asarray(species, np.int64).reshape(-1), xyz


def write_index(out_dir, rows):
    parts = ["<!doctype html><html><head><meta charset='utf-8'><title>view_results</title></head><body>"]
    for r in rows:
        parts.append("<h3>%s</h3><p>%s</p><img src='%s'>" % (html.escape(r["id"]), html.escape(" | ".join(r["titles"])),
                                                            html.escape(r["png"])))
    parts.append("</body></html>")
    with open(os.path.join(out_dir, "index.html"), "w") as f:
        f.write("\n".join(parts))


def main(argv=None):
    a = build_parser().parse_args(argv)
    from icsg3d_amd import render as R
    from icsg3d_amd.cli import load_models
    from icsg3d_amd.watershed import refine_atoms, watershed_clustering

    name, d, bs, ncond = a.name, a.d, a.batch_size, 10
    out_dir = a.out or os.path.join("output", "view", str(name))
    os.makedirs(out_dir, exist_ok=True)
    vae, unet = load_models(name, d, a.channels, ncond, bs, a.synthetic, a.seed, True)
    eng, ueng = vae._engine(bs), unet._engine(bs)
    rng = np.random.RandomState(a.seed)
    cam = (a.elev, a.azim)
    look = dict(cam=cam, size=a.size)

    rows, skipped = [], []
    for ids, M, cond, S, Sb in batches(a, ncond):
        if len(rows) >= a.count:
            break
        eps = rng.normal(size=(len(ids), vae.latent_dim))
        out = eng.reconstruct_to_atoms(ueng, M, cond, eps, thresh=0.8, min_voxels=3, max_atoms=2048, want_regions=True)
        m_true = eng.render_resident(0, mode=a.mode, **look)      # the batch and its reconstruction, where they lie
        m_pred = eng.render_resident(1, mode=a.mode, **look)
        refine_atoms(out, max_iters=5, num_species=unet.num_classes)
        M_recon = vae.model.predict([M, cond], eps=eps)
        for i, sid in enumerate(ids):
            if len(rows) >= a.count:
                break
            try:
                sp_t, mu_t, ws_t = watershed_clustering(M[i, ..., 0], S[i], Sb[i], return_ws=True, max_iters=5)
            except Exception as e:                                # the reference's except: continue
                print(sid, "failed (true side):", type(e).__name__)
                skipped.append({"id": sid, "failed_true": True, "failed_pred": bool(out["failed"][i])})
                continue
            if out["failed"][i]:
                print(sid, "failed (predicted side)")
                skipped.append({"id": sid, "failed_true": False, "failed_pred": True})
                continue
            sp_p, mu_p = out["atoms"][i]
            mse = float(np.mean((M[i].astype(np.float64) - M_recon[i].astype(np.float64)) ** 2))
            f1 = float(ueng.test_step(M_recon[i:i + 1], np.ascontiguousarray(S[i:i + 1], np.uint8))[3])
            vols = np.stack([S[i], ws_t, out["species"][i], out["regions"][i]]).astype(np.int32)
            lab = R.labels(vols, **look)
            pts = R.atoms([atom_set(sp_t, mu_t), atom_set(sp_p, mu_p)], d, **look)
            panels = [m_true[i], lab[0], lab[1], pts[0], m_pred[i], lab[2], lab[3], pts[1]]
            stem = os.path.splitext(str(sid))[0]
            R.write_png(os.path.join(out_dir, stem + ".png"), R.sheet([R.over(p) for p in panels], 2, 4, pad=4))
            titles = [t % v if "%" in t else t for t, v in zip(TITLES, (0, 0, 0, 0, mse, f1, 0, 0))]
            row = {"id": str(sid), "png": stem + ".png", "titles": titles, "mse": mse, "f1": f1,
                   "n_atoms_true": int(len(sp_t)), "n_atoms_pred": int(len(sp_p)), "failed_true": False,
                   "failed_pred": False, "split_pred": bool(out["split"][i])}
            with open(os.path.join(out_dir, stem + ".json"), "w") as f:
                json.dump(row, f, indent=1)
            rows.append(row)

    write_index(out_dir, rows)
    with open(os.path.join(out_dir, "run.json"), "w") as f:
        json.dump({"rendered": [r["id"] for r in rows], "skipped": skipped, "panel_size": a.size, "camera": list(cam),
                   "args": vars(a)}, f, indent=1)
    with np.errstate(all="ignore"):
        print("samples: rendered %d / failed %d" % (len(rows), len(skipped)))
        print("wrote", out_dir, "- mean MSE %.3f, mean F1 %.3f" % (
            (np.mean([r["mse"] for r in rows]), np.mean([r["f1"] for r in rows])) if rows else (0.0, 0.0)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
