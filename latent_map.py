#!/usr/bin/env python3
"""The t-SNE map of the VAE's latent space (reference viz.py tsne_latent, the paper's annotated latent-space figure) on the
MI355X engine: every structure of the chosen split is encoded, its z_mean is appended to the t-SNE handle device to
device, and the map is computed with exact repulsion (icsg3d_amd.tsne.latent_map; scikit-learn's objective at angle = 0).

Flags in eval.py's style: --name --samples --split --nrot --batch_size --d --ncond --target --perplexity --max_iter
--which {val,train,all}; ids and condition bins as eval.py takes them (data_split, VAEDataGenerator(shuffle=False)).
Added: --synthetic (Gaussian-blob grids and, where no checkpoint exists under saved_models/, seeded random weights: no
dataset exists offline), --channels, --seed, --thumbnails (density slices drawn on the figure).

Writes output/latent/<name>_tsne.npz (embedding (N, 2), ids, cond_bin, target, kl_divergence, n_iter) and run.json.  When
matplotlib imports, output/latent/<name>_tsne.svg is written with the Agg back end and no plt.show: a scatter coloured by
condition bin with a density slice thumbnail on a subsample of the points (the reference's imscatter).

    python latent_map.py --name perovskite --which val
    python latent_map.py --name demo --synthetic --samples 512 --d 16 --channels 1
"""
import argparse
import json
import os
import sys

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--name", metavar="name", type=str, help="Name of data folder")
    p.add_argument("--samples", metavar="samples", type=int, help="Number of samples", default=78750)
    p.add_argument("--split", metavar="split", type=float, help="Train-test split fraction", default=0.8)
    p.add_argument("--nrot", metavar="nrot", type=int, help="Number of rotations per structure", default=0)
    p.add_argument("--batch_size", metavar="batch_size", type=int, help="Batch size", default=20)
    p.add_argument("--d", metavar="d", type=int, help="Dimension of density matrices (number of voxels)", default=32)
    p.add_argument("--ncond", metavar="ncond", type=int, help="Number of condition bins", default=10)
    p.add_argument("--target", metavar="target", type=str, help="Property column the condition bins are cut from",
                   default="formation_energy_per_atom")
    p.add_argument("--perplexity", type=float, default=30.0, help="t-SNE perplexity")
    p.add_argument("--max_iter", type=int, default=1000, help="t-SNE iterations")
    p.add_argument("--which", choices=("val", "train", "all"), default="val", help="the ids that are mapped")
    p.add_argument("--synthetic", action="store_true", help="Gaussian-blob grids instead of data/<name>")
    p.add_argument("--channels", type=int, default=4, help="input channels (density + 3 coordinate grids)")
    p.add_argument("--seed", type=int, default=0, help="seed of the synthetic grids and random weights")
    p.add_argument("--thumbnails", type=int, default=40, help="density slices drawn on the figure")
    return p


def plot_map(emb, bins, thumbs, thumb_idx, path):
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        from matplotlib.offsetbox import AnnotationBbox, OffsetImage
    except ImportError:
        return False
    fig, ax = plt.subplots(figsize=(10, 10))
    sc = ax.scatter(emb[:, 0], emb[:, 1], c=bins, s=6, cmap="viridis")
    for im, i in zip(thumbs, thumb_idx):                              # imscatter: a slice of the density per point
        ax.add_artist(AnnotationBbox(OffsetImage(im, zoom=1.0, cmap="gray"), (emb[i, 0], emb[i, 1]), frameon=False))
    fig.colorbar(sc, ax=ax, label="condition bin")
    ax.set_xticks([]); ax.set_yticks([])
    plt.savefig(path, format="svg")
    plt.close(fig)
    return True


def main(argv=None):
    a = build_parser().parse_args(argv)
    from icsg3d_amd.cli import load_models
    from icsg3d_amd.tsne import latent_map
    name, d, C, bs = a.name, a.d, a.channels, a.batch_size
    out_dir = os.path.join("output", "latent")
    os.makedirs(out_dir, exist_ok=True)

    target = None
    if a.synthetic:
        from icsg3d_amd.vae.data import SyntheticVAEGenerator
        gen = SyntheticVAEGenerator(a.samples, batch_size=bs, dim=(d, d, d), n_channels=C, n_bins=a.ncond, seed=a.seed)
    else:
        from icsg3d_amd.utils import data_split
        from icsg3d_amd.vae.data import VAEDataGenerator
        data_path = os.path.join("data", name, "matrices")
        train_ids, val_ids = data_split(data_path, a.samples, frac=a.split, n_rot=a.nrot)
        ids = {"val": val_ids, "train": train_ids, "all": list(train_ids) + list(val_ids)}[a.which]
        gen = VAEDataGenerator(ids, data_path=data_path, property_csv=os.path.join("data", name, name + ".csv"),
                               batch_size=bs, dim=(d, d, d), n_channels=C, shuffle=False, n_bins=a.ncond, target=a.target)
        target = dict(zip(gen.property_df["task_id"], gen.property_df[a.target]))
    n = len(gen) * bs
    if n < 2:
        raise SystemExit("fewer than 2 structures in whole batches of %d" % bs)
    vae, _ = load_models(name, d, C, a.ncond, bs, a.synthetic, a.seed, False)   # checkpoints or seeded random weights

    ids, bins, thumbs, thumb_idx = [], [], [], []
    every = max(1, n // max(a.thumbnails, 1))

    def batches():
        for x, cond in gen:
            for r in range(len(x)):
                if a.thumbnails > 0 and len(ids) % every == 0 and len(thumbs) < a.thumbnails:
                    thumbs.append(np.array(x[r, :, :, (12 * d) // 32, 0])); thumb_idx.append(len(ids))
                ids.append(gen.list_IDs_temp[r]); bins.append(int(np.argmax(cond[r])))
            yield x, cond

    res = latent_map(vae, batches(), capacity=n, perplexity=a.perplexity, max_iter=a.max_iter)
    import re
    tvals = np.array([np.nan if target is None else float(target.get(re.split(r"_|\.", i)[0], np.nan)) for i in ids])
    np.savez(os.path.join(out_dir, name + "_tsne.npz"), embedding=res.embedding_, ids=np.array(ids, dtype=str),
             cond_bin=np.array(bins, np.int32), target=tvals, kl_divergence=np.float64(res.kl_divergence_),
             n_iter=np.int32(res.n_iter_))
    figure = plot_map(res.embedding_, np.array(bins), thumbs, thumb_idx, os.path.join(out_dir, name + "_tsne.svg"))
    with open(os.path.join(out_dir, "run.json"), "w") as f:
        json.dump(dict(vars(a), n=n, kl_divergence=float(res.kl_divergence_), n_iter=int(res.n_iter_),
                       seconds=res.seconds, figure=bool(figure)), f, indent=1)
    print("wrote", os.path.join(out_dir, name + "_tsne.npz"), "N =", n, "KL =", res.kl_divergence_)
    return 0


if __name__ == "__main__":
    sys.exit(main())
