"""Training-loop throughput with and without fed steps ("Fed steps"): not the contract bench.

Writes a dataset in the on-disk format of create_matrices.py (float64 density, coordinate and species grids) to /dev/shm
and times the two class-level loops -- AtomUnet.model.fit_generator and LatticeDFCVAE.train -- at d = 32, B = 32 for
C = 1 and C = 4, four ways in one process:

  unfed      feed=False: loader threads cast / concatenate / convert on the host, the step uploads from pageable
             memory on the compute stream and waits for its metrics (the path before fed steps existed)
  fed        feed=True over the same file generators: raw payloads into pinned slots, upload on the copy stream, pack
             kernel, metrics through the ring
  generator  feed=False and feed=True over a generator with the reference's contract (float64 X; for the U-Net a
             one-hot float32 y), which the Feeder copies without a host cast
  resident   the bare resident step on an uploaded batch: the ceiling of any loop

Each figure is grids/s over >= 50 steps, repeated --repeats times (median, min, max).  One JSON document:

    python scripts/loop_bench.py --out profiles/feed_loop.json
"""
import argparse
import contextlib
import io
import json
import os
import re
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from benchutil import timeit  # noqa: E402

D, B, NCOND = 32, 32, 10


def write_dataset(root, samples):
    """`samples` files per kind; the grids repeat with period 64 (their content does not matter to the clock)"""
    from icsg3d_amd.synthetic import synthetic_batch
    X, lab, _ = synthetic_batch(64, D, 4, seed=0, noise=1e-3)
    X = X.astype(np.float64)
    for sub in ("density_matrices", "species_matrices", "coordinate_grids"):
        os.makedirs(os.path.join(root, sub))
    ids = ["mp-%d.npy" % i for i in range(samples)]
    for k, f in enumerate(ids):
        np.save(os.path.join(root, "density_matrices", f), X[k % 64, ..., 0].ravel())
        np.save(os.path.join(root, "coordinate_grids", f), X[k % 64, ..., 1:4])
        np.save(os.path.join(root, "species_matrices", f), lab[k % 64].astype(np.float64))
    csv = os.path.join(root, "property.csv")
    rng = np.random.default_rng(0)
    with open(csv, "w") as fh:
        fh.write("task_id,formation_energy_per_atom,nsites\n")
        for i in range(samples):
            fh.write("mp-%d,%.6f,%d\n" % (i, rng.normal(), 2 + i % 30))
    return ids, csv


class ReferenceContract:
    """the reference's generators: float64 X; for the U-Net [one-hot float32 y, mask], for the VAE the condition"""

    def __init__(self, gen, vae):
        self.gen, self.vae, self.batch_size, self.list_IDs = gen, vae, gen.batch_size, gen.list_IDs

    def __len__(self):
        return len(self.gen)

    def __getitem__(self, i):
        g = self.gen
        ids = [g.list_IDs[k] for k in g.indexes[i * g.batch_size:(i + 1) * g.batch_size]]
        X = np.stack([g.create_lattice_meshgrid(f, g.n_channels) for f in ids])
        if self.vae:
            return X, np.stack([g.property_to_categorical(f) for f in ids])
        y = np.stack([np.load(os.path.join(g.data_path, "species_matrices", f)).reshape(g.dim) for f in ids]).astype(np.int64)
        return X, [np.eye(g.n_classes, dtype=np.float32)[y], (y != 0).astype(np.float32)[..., None]]


def summary(rates, resident):
    rates = sorted(rates)
    return {"grids_per_s": float(np.median(rates)), "min": rates[0], "max": rates[-1], "repeats": len(rates),
            "frac_of_resident": float(np.median(rates)) / resident}


def unet_config(C, ids, root, epochs, repeats, gen_epochs):
    from icsg3d_amd.unet.data import UnetDataGenerator
    from icsg3d_amd.unet.unet import AtomUnet
    np.random.seed(0)
    unet = AtomUnet(input_shape=(D, D, D, C), lr=1e-6, max_batch=B)
    gen = UnetDataGenerator(ids, root, batch_size=B, dim=(D, D, D), n_channels=C)
    steps = len(gen)

    def loop(g, feed, n_epochs):
        t0 = time.perf_counter()
        unet.model.fit_generator(g, epochs=n_epochs, verbose=0, feed=feed)
        unet._eng.sync()
        return n_epochs * steps * B / (time.perf_counter() - t0)

    loop(gen, False, 1)                                     # engine creation, first-touch
    loop(gen, True, 1)
    X, (y, _) = gen[0]
    unet._eng.upload_batch(X, y)
    res = timeit(lambda: ([unet._eng.train_step_resident() for _ in range(50)], unet._eng.sync()), repeats, 1)
    resident = 50 * B / (res["median_ms"] * 1e-3)
    out = {"steps_per_figure": epochs * steps, "resident_grids_per_s": resident, "resident_step_ms": res["median_ms"] / 50}
    unfed, fed = [], []
    for _ in range(repeats):                                # alternating: both see the same machine
        unfed.append(loop(gen, False, epochs))
        fed.append(loop(gen, True, epochs))
    out["unfed"], out["fed"] = summary(unfed, resident), summary(fed, resident)
    ref = ReferenceContract(gen, vae=False)
    out["generator_unfed"] = summary([loop(ref, False, gen_epochs)], resident)
    out["generator_fed"] = summary([loop(ref, True, gen_epochs)], resident)
    out["generator_steps_per_figure"] = gen_epochs * steps
    weights = unet._get_weights()
    unet._eng.close()
    return out, weights


def vae_config(C, ids, root, csv, pm_weights, epochs, repeats, gen_epochs, tmp):
    from icsg3d_amd.vae.data import VAEDataGenerator
    from icsg3d_amd.vae.lattice_vae import LatticeDFCVAE
    kw = dict(data_path=root, dim=(D, D, D), n_channels=C, property_csv=csv, n_bins=NCOND)
    gen = VAEDataGenerator(ids, batch_size=B, **kw)
    val = VAEDataGenerator(ids[:B], batch_size=B, **kw)       # one validation batch per epoch: train() needs one
    steps = len(gen)
    np.random.seed(0)
    vae = LatticeDFCVAE(input_shape=(D, D, D, C), perceptual_model=pm_weights, cond_shape=NCOND, output_dir=tmp)

    def loop(g, v, feed, groups, n_epochs):
        """one train() call of 1 + groups * n_epochs epochs; the epoch clock train() prints (train + validation steps,
        without the checkpoint writes); the first epoch warms up"""
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            vae.train(g, v, epochs=1 + groups * n_epochs, weights=os.path.join(tmp, "vae_%d.best.hdf5" % C), feed=feed)
        secs = [float(s) for s in re.findall(r"Time: ([0-9.]+) s", buf.getvalue())][1:]
        assert len(secs) == groups * n_epochs, buf.getvalue()[-2000:]
        return [n_epochs * (steps + 1) * B / sum(secs[k * n_epochs:(k + 1) * n_epochs]) for k in range(groups)]

    unfed, fed = [], []
    for _ in range(repeats):                                # alternating: both see the same machine
        unfed += loop(gen, val, False, 1, epochs)
        fed += loop(gen, val, True, 1, epochs)
    M, cond = gen[0]
    eps = np.random.default_rng(1).standard_normal((B, 256)).astype(np.float32)
    vae._eng.upload_batch(M, cond, eps)
    res = timeit(lambda: ([vae._eng.train_step_resident() for _ in range(50)], vae._eng.sync()), repeats, 1)
    resident = 50 * B / (res["median_ms"] * 1e-3)
    out = {"steps_per_figure": epochs * (steps + 1), "resident_grids_per_s": resident, "resident_step_ms": res["median_ms"] / 50}
    out["unfed"], out["fed"] = summary(unfed, resident), summary(fed, resident)
    rg, rv = ReferenceContract(gen, vae=True), ReferenceContract(val, vae=True)
    out["generator_unfed"] = summary(loop(rg, rv, False, 1, gen_epochs), resident)
    out["generator_fed"] = summary(loop(rg, rv, True, 1, gen_epochs), resident)
    out["generator_steps_per_figure"] = gen_epochs * (steps + 1)
    vae._eng.close(); vae._pm_eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed_loop.json"))
    ap.add_argument("--samples", type=int, default=512, help="files per kind (16 batches of 32)")
    ap.add_argument("--epochs", type=int, default=4, help="epochs per figure: 4 x 16 = 64 steps")
    ap.add_argument("--gen-epochs", type=int, default=1, help="epochs per figure of the reference-contract generator")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--channels", type=int, nargs="*", default=[1, 4])
    ap.add_argument("--tmp", default="/dev/shm")
    a = ap.parse_args()
    from icsg3d_amd import _lib
    tmp = tempfile.mkdtemp(prefix="icsg3d_loop_bench_", dir=a.tmp)
    doc = {"d": D, "batch": B, "samples": a.samples, "configs": {}, "version": _lib.load().ics_version().decode()}
    try:
        t0 = time.perf_counter()
        ids, csv = write_dataset(os.path.join(tmp, "matrices"), a.samples)
        doc["dataset_seconds"] = time.perf_counter() - t0
        for C in a.channels:
            r, pm = unet_config(C, ids, os.path.join(tmp, "matrices"), a.epochs, a.repeats, a.gen_epochs)
            doc["configs"]["unet_c%d" % C] = r
            print("unet C=%d: %s" % (C, json.dumps(r)), flush=True)
            r = vae_config(C, ids, os.path.join(tmp, "matrices"), csv, pm, a.epochs, a.repeats, a.gen_epochs, tmp)
            doc["configs"]["vae_c%d" % C] = r
            print("vae C=%d: %s" % (C, json.dumps(r)), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
