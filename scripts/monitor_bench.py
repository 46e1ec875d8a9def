#!/usr/bin/env python3
"""The training monitors on one MI355X -> profiles/monitor_bench.json (or --out).

  ops       the three operations at the monitors' own sizes: ics_op_render_slice of 10 float32 slices at d = 32, zoom 4
            (one sheet column) and the same through ics_vae_render_slice_resident; ics_op_kde_evaluate of 1000 codes x 256
            dimensions on 50 points; ics_op_render_lines of the 256 KDE curves of 50 points at 592 x 432 and of two loss
            curves of 100 points.
  monitor   one whole VaeMonitor.best() call at d = 32, batch 20: reconstructions, samples and the KDE trio, 50 encoder
            passes included, files written to a temporary folder.
  reference where scipy and matplotlib import: the same pictures by the reference's route (scipy.stats.gaussian_kde per
            dimension, imshow / plot / savefig under Agg), for comparison only -- other pictures by another method.

Every time is the host clock around calls that end in a device synchronise; median of --reps after --warmup.  Nothing is
gated on these numbers.
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchutil import timeit  # noqa: E402


def reference_route(X, z, x, losses, folder):
    """plot_reconstructions-like sheet, plot_kde and plot_losses as the reference draws them"""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from scipy.stats import gaussian_kde

    def sheet():
        fig, axes = plt.subplots(10, 2, figsize=(4, 20))
        for i in range(10):
            for j in range(2):
                axes[i][j].imshow(X[i, :, :, 16, 0])
        plt.savefig(os.path.join(folder, "ref_sheet.png"))
        plt.close(fig)

    def kde():
        plt.figure()
        for j in range(z.shape[1]):
            plt.plot(x, gaussian_kde(z[:, j])(x))
        plt.savefig(os.path.join(folder, "ref_kde.png"))
        plt.close()

    def loss():
        plt.figure()
        plt.plot(losses[:, 0]); plt.plot(losses[:, 1])
        plt.savefig(os.path.join(folder, "ref_loss.png"))
        plt.close()
    return {"sheet_10x2": timeit(sheet, 3, 1), "kde_256": timeit(kde, 3, 1), "losses": timeit(loss, 3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "monitor_bench.json"))
    a = ap.parse_args()
    from icsg3d_amd import _lib as L
    from icsg3d_amd import monitor as M
    from icsg3d_amd.synthetic import random_weights, synthetic_batch
    from icsg3d_amd.vae.data import SyntheticVAEGenerator
    from icsg3d_amd.vae.lattice_vae import LatticeDFCVAE
    assert L.device_count() >= 1, "no HIP device visible"
    d, bs, latent = 32, 20, 256
    rng = np.random.default_rng(0)
    X, _, cond = synthetic_batch(bs, d, 1, seed=0)
    z = (rng.standard_normal((1000, latent)) * rng.uniform(0.05, 1.2, latent)).astype(np.float32)
    x = np.linspace(-3, 3, 50)
    losses = np.stack([3.0 / (1 + np.arange(100.0)), 3.2 / (1 + np.arange(100.0)) + 0.05], axis=1)
    res = {"d": d, "batch": bs, "latent": latent, "codes": 1000, "reps": a.reps, "warmup": a.warmup}

    kde = M.Kde(latent, 1000)
    kde.append(z)
    dens = kde.evaluate(x)[0]
    kcurves = np.stack([np.broadcast_to(x, dens.shape), dens], axis=2)
    lcurves = np.stack([np.stack([np.arange(100.0), losses[:, k]], axis=1) for k in range(2)])
    ops = {"slice_10_d32_zoom4": timeit(lambda: M.slices(X[:10], zoom=4), a.reps, a.warmup),
           "kde_1000x256_50pts": timeit(lambda: kde.evaluate(x), a.reps, a.warmup),
           "lines_kde_256x50_592x432": timeit(lambda: M.line_plot(kcurves, (-3, 3, 0, float(dens.max())), (592, 432),
                                                                  alpha=0.6), a.reps, a.warmup),
           "lines_losses_2x100_592x432": timeit(lambda: M.line_plot(lcurves, (0, 99, 0, 3.3), (592, 432)), a.reps,
                                                a.warmup)}
    kde.close()

    uw, vw = random_weights(d, 1, 0)
    vae = LatticeDFCVAE(input_shape=(d, d, d, 1), perceptual_model=uw, cond_shape=10)
    vae._set_model(None, batch_size=bs)
    vae._set_weights(vw)
    gen = SyntheticVAEGenerator(10 * bs, bs, (d, d, d), 1, 10, seed=1)
    eng = vae._engine(bs)
    eps = rng.standard_normal((bs, latent)).astype(np.float32)
    eng.decode(eng.encode(X, cond, eps)[2], cond)
    ops["slice_resident_10_d32_zoom4"] = timeit(lambda: M.resident_slices(eng, 1, 10, zoom=4), a.reps, a.warmup)
    res["ops"] = ops
    print("ops", json.dumps(ops), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        mon = M.VaeMonitor(vae, gen, tmp, seed=0)
        res["monitor"] = {"vae_best_epoch_call": timeit(lambda: mon.best(0), max(a.reps // 4, 3), 1)}
        print("monitor", json.dumps(res["monitor"]), flush=True)
        try:
            res["reference_route"] = reference_route(X, z.astype(np.float64), x, losses, tmp)
        except ImportError:
            res["reference_route"] = None
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
