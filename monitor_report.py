#!/usr/bin/env python3
"""monitor_report.py: the training monitors' pictures from saved checkpoints and the validation split, without training.

What `train_unet.py --monitor` and `train_vae.py --monitor` write when the validation loss improves (the reference's
TrainingPlot, unet/unet.py:39-157, and the VAE loop's plot_reconstructions / plot_samples / plot_kde,
vae/lattice_vae.py:327-337, 359-436), drawn once on the GPU (icsg3d_amd/monitor.py):

    --which unet   segmentations_best.png, segmentations_binary_best.png
    --which vae    vae_reconstructions.png, vae_samples.png, vae_kde.png / .svg / .json
    --which both   all of them

each PNG with its .json sidecar, plus run.json.  Checkpoints and paths as the other inference scripts
(icsg3d_amd.cli); --synthetic: Gaussian-blob batches and, where no checkpoint exists under saved_models/, seeded
random weights, the way view_results.py --synthetic runs.

    python monitor_report.py --name heusler --which both
"""
import argparse
import json
import os
import sys

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--name", type=str, required=True, help="Name of data folder")
    p.add_argument("--which", choices=("unet", "vae", "both"), default="both")
    p.add_argument("--synthetic", action="store_true", help="Gaussian-blob samples instead of data/<name>")
    p.add_argument("--batch_size", type=int, default=20)
    p.add_argument("--samples", type=int, default=40000)
    p.add_argument("--nrot", type=int, default=10)
    p.add_argument("--split", type=float, default=0.8)
    p.add_argument("--ncond", type=int, default=10)
    p.add_argument("--cond", type=str, default="formation_energy_per_atom")
    p.add_argument("--d", "--dim", dest="d", type=int, default=32)
    p.add_argument("--channels", type=int, default=4)
    p.add_argument("--zoom", type=int, default=4, help="pixels per voxel in the slice pictures")
    p.add_argument("--out", type=str, default=None, help="output folder (default output/monitor/<name>)")
    p.add_argument("--seed", type=int, default=0, help="seed of the sampling draws and of the synthetic batches")
    return p


def generators(a):
    """(U-Net validation generator, VAE validation generator) over the validation split, as the train scripts build them."""
    from icsg3d_amd.unet.data import SyntheticUnetGenerator, UnetDataGenerator
    from icsg3d_amd.vae.data import SyntheticVAEGenerator, VAEDataGenerator
    d, bs = a.d, a.batch_size
    if a.synthetic:
        n = 10 * bs
        return (SyntheticUnetGenerator(n, bs, (d, d, d), a.channels, 95, seed=10 ** 6 + a.seed),
                SyntheticVAEGenerator(n, bs, (d, d, d), a.channels, a.ncond, seed=10 ** 6 + a.seed))
    from icsg3d_amd.utils import data_split
    path = os.path.join("data", a.name, "matrices")
    _, val = data_split(path, a.samples, frac=a.split, n_rot=a.nrot)
    val = val[:len(val) // bs * bs]
    ug = UnetDataGenerator(val, data_path=path, batch_size=bs, dim=(d, d, d), n_channels=a.channels, shuffle=False)
    vg = VAEDataGenerator(val, data_path=path, property_csv=os.path.join("data", a.name, a.name + ".csv"), batch_size=bs,
                          dim=(d, d, d), n_channels=a.channels, shuffle=False, n_bins=a.ncond, target=a.cond)
    return ug, vg


def main(argv=None):
    a = build_parser().parse_args(argv)
    from icsg3d_amd import monitor as M
    from icsg3d_amd.cli import load_models
    out_dir = a.out or os.path.join("output", "monitor", str(a.name))
    os.makedirs(out_dir, exist_ok=True)
    vae, unet = load_models(a.name, a.d, a.channels, a.ncond, a.batch_size, a.synthetic, a.seed, True)
    ugen, vgen = generators(a)
    wrote = []
    if a.which in ("unet", "both"):
        mon = M.UnetMonitor(ugen, out_dir, model=unet, zoom=a.zoom)
        mon.draw_sheets()
        wrote += ["segmentations_best.png", "segmentations_binary_best.png"]
    if a.which in ("vae", "both"):
        mon = M.VaeMonitor(vae, vgen, out_dir, seed=a.seed, zoom=a.zoom)
        mon.best()
        wrote += ["vae_reconstructions.png", "vae_samples.png", "vae_kde.png", "vae_kde.svg", "vae_kde.json"]
        k = json.load(open(os.path.join(out_dir, "vae_kde.json")))
        print("latent KDE over %d codes: %d of %d dimensions collapsed" % (k["count"], k["collapsed"], len(k["status"])))
    with open(os.path.join(out_dir, "run.json"), "w") as f:
        json.dump({"wrote": wrote, "args": vars(a)}, f, indent=1)
    print("wrote", out_dir, "-", ", ".join(wrote))
    return 0


if __name__ == "__main__":
    sys.exit(main())
