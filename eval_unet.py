#!/usr/bin/env python3
"""Score the U-Net per species: the confusion matrix of a whole split, counted on the GPU.

The reference scores its segmentation with two global ratios (unet/unet.py:159-193) that the ~98 % background voxels
dominate.  This script runs every batch of the validation (or training) split through the engine's eval-mode forward,
argmax / sig >= thresh (generate.py:220-225) and the confusion kernel, accumulates on the device, reads the matrix once at
the end and writes per-class support, precision, recall, F1 and IoU, the largest confusions and the occupancy head's
scores (icsg3d_amd/classreport.py) to output/eval_unet/<name>/{confusion.npy,report.csv,report.json,run.json}.

Same flags, paths and checkpoint conventions as train_unet.py; new: --which val|train, --thresh, --top.

--atoms also scores the split atom by atom in the same forward passes: the connected components of the predictions and of
the true labels are matched on the GPU (icsg3d_amd/atomscore.py; --atom_tol voxels, components above --min_voxels voxels,
at most --max_atoms a sample) and atom_confusion.npy, atom_report.csv and atom_report.json are written next to the others
(icsg3d_amd/atomreport.py).  Without --atoms nothing changes.

  python3 eval_unet.py --name heusler --samples 5000
  python3 eval_unet.py --name demo --synthetic 64 --channels 1 --d 16 --batch_size 8

Data parallel: --gpus N (or torch.distributed.run) deals the ids round-robin over the ranks; the integer counts are
summed over the process group at the end and rank 0 writes.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

from icsg3d_amd import atomreport, classreport
from icsg3d_amd.cli import checkpoint_paths


def parser():
    p = argparse.ArgumentParser()
    p.add_argument("--name", type=str, help="Name of data folder")
    p.add_argument("--samples", type=int, default=20000, help="Total number of training and validation samples")
    p.add_argument("--d", "--dim", dest="d", type=int, default=32, help="Dimension of density matrices (number of voxels)")
    p.add_argument("--batch_size", type=int, default=10)
    p.add_argument("--nrot", type=int, default=10)
    p.add_argument("--nclasses", type=int, default=95)
    p.add_argument("--split", type=float, default=0.8)
    p.add_argument("--channels", type=int, default=4, help="input channels (density + 3 coordinate grids)")
    p.add_argument("--synthetic", type=int, default=0, help="score N synthetic grids instead of data/<name>")
    p.add_argument("--which", choices=("val", "train"), default="val", help="the split to score")
    p.add_argument("--thresh", type=float, default=0.8, help="threshold of the occupancy (sigmoid) head")
    p.add_argument("--top", type=int, default=20, help="how many of the largest confusions to report")
    p.add_argument("--atoms", action="store_true", help="also score the split atom by atom (atom_report.*)")
    p.add_argument("--atom_tol", type=float, default=2.0, help="--atoms: matching distance in voxels (strict)")
    p.add_argument("--min_voxels", type=int, default=3, help="--atoms: predicted components of at most this many voxels are dropped")
    p.add_argument("--max_atoms", type=int, default=512, help="--atoms: a sample with more components fails (at most 1024)")
    p.add_argument("--gpus", type=int, default=0,
                   help="data parallel over N GPUs of this node (icsg3d_amd/launcher.py); 0 = whatever the environment says")
    return p


def generators(a, rank=0, world=1):
    """The generators whose batches, in order, are this rank's share of the chosen split: whole batches of --batch_size,
    then one short batch with what is left (the training loop drops it; a score must not)."""
    from icsg3d_amd.unet.data import SyntheticUnetGenerator, UnetDataGenerator
    from icsg3d_amd.utils import data_split
    d, bs = a.d, a.batch_size
    if a.synthetic:
        n_train = int(a.synthetic * a.split)
        n, seed = (a.synthetic - n_train, 10 ** 6) if a.which == "val" else (n_train, 0)     # train_unet.py's streams
        n = len(range(rank, n, world))
        seed += rank * 10 ** 7
        gens = [SyntheticUnetGenerator(n - n % bs, bs, (d, d, d), a.channels, a.nclasses, seed=seed)]
        if n % bs:
            gens.append(SyntheticUnetGenerator(n % bs, n % bs, (d, d, d), a.channels, a.nclasses, seed=seed + n // bs))
        return gens
    path = os.path.join("data", a.name, "matrices")
    train_ids, val_ids = data_split(path, a.samples, frac=a.split, n_rot=a.nrot)
    ids = list(val_ids if a.which == "val" else train_ids)[rank::world]
    whole = len(ids) - len(ids) % bs
    kw = dict(data_path=path, dim=(d, d, d), n_channels=a.channels, n_classes=a.nclasses, shuffle=False)
    gens = [UnetDataGenerator(ids[:whole], batch_size=bs, **kw)]
    if len(ids) % bs:
        gens.append(UnetDataGenerator(ids[whole:], batch_size=len(ids) % bs, **kw))
    return gens


ATOM_FLAGS = ("atoms", "atom_tol", "min_voxels", "max_atoms")


def accumulate(engine, gens, num_classes, thresh, atoms=False):
    """every batch of every generator through confusion_batch -- with atoms through atom_score_batch, which counts the
    voxels of the same labels too -- enqueued only; returns the number of samples"""
    from icsg3d_amd.unet.unet import _to_labels
    n = 0
    for gen in gens:
        for i in range(len(gen)):
            X, y = gen[i]
            X, lab = np.asarray(X, np.float32), _to_labels(y[0] if isinstance(y, (list, tuple)) else y, num_classes)
            if atoms:
                engine.atom_score_batch(X, lab, thresh, with_confusion=True)
            else:
                engine.confusion_batch(X, lab, thresh)
            n += len(X)
    return n


def main(argv=None):
    a = parser().parse_args(argv)
    if a.gpus:                                   # before anything touches the GPU; exits with the ranks' status
        from icsg3d_amd.launcher import ensure_ranks
        ensure_ranks(a.gpus, os.path.abspath(__file__), sys.argv[1:] if argv is None else list(argv))
    from icsg3d_amd.dataparallel import from_env
    from icsg3d_amd.unet.unet import AtomUnet
    dp = from_env()
    rank, world = (dp[1], dp[2]) if dp else (0, 1)
    weights = checkpoint_paths(a.name)[1]
    if not os.path.exists(weights):
        if not a.synthetic:
            raise SystemExit("eval_unet.py: no checkpoint at %s (train_unet.py --name %s writes it)" % (weights, a.name))
        np.random.seed(0)                        # --synthetic without a checkpoint: the same random weights on every rank
    unet = AtomUnet(num_classes=a.nclasses, input_shape=(a.d, a.d, a.d, a.channels), weights=weights, max_batch=a.batch_size)
    gens = generators(a, rank, world)
    eng = unet._engine(a.batch_size)
    eng.confusion_open()
    if a.atoms:
        eng.atom_score_open(a.atom_tol, a.min_voxels, a.max_atoms)
    t0 = time.time()
    samples = accumulate(eng, gens, a.nclasses, a.thresh, a.atoms)
    acc = eng.confusion_read()                   # the one wait
    tallies = eng.atom_score_read() if a.atoms else None
    seconds = time.time() - t0
    matrix, occ, tail = classreport.reduce_over_ranks(
        dp[0] if dp else None, [acc["matrix"], acc["occupancy"], np.array([acc["out_of_range"], acc["voxels"], samples])])
    if a.atoms:                                  # integer sums over the ranks, like the voxel counts
        keys = list(tallies)
        tallies = dict(zip(keys, atomreport.reduce_over_ranks(dp[0] if dp else None, [tallies[k] for k in keys])))
    if rank == 0:
        sdir = os.path.join("output", "eval_unet", a.name)
        args = {k: v for k, v in vars(a).items() if a.atoms or k not in ATOM_FLAGS}
        run = {"args": args, "checkpoint": weights if os.path.exists(weights) else None, "ranks": world,
               "samples": int(tail[2]), "voxels": int(tail[1]), "out_of_range": int(tail[0]), "seconds_rank0": seconds,
               "grids_per_s_rank0": samples / seconds if seconds > 0 else None}
        r = classreport.write(sdir, matrix, occ, top=a.top, extra={"thresh": a.thresh, "which": a.which, "out_of_range": int(tail[0])})
        if a.atoms:
            ar = atomreport.write(sdir, tallies, tol=a.atom_tol, top=a.top,
                                  extra={"thresh": a.thresh, "which": a.which, "atom_tol": a.atom_tol,
                                         "min_voxels": a.min_voxels, "max_atoms": a.max_atoms})
            o = ar["overall"]
            run["atoms"] = {k: o[k] for k in ("samples", "failed", "perfect", "true_atoms", "pred_atoms", "detected", "typed",
                                              "missed", "spurious", "dup", "shadowed")}
        with open(os.path.join(sdir, "run.json"), "w") as f:
            json.dump(run, f, indent=1)
        print(classreport.table(r, worst=10, top=min(a.top, 10)))
        if a.atoms:
            print(atomreport.table(ar, worst=10, top=min(a.top, 10)))
            print("wrote %s/{confusion.npy,report.csv,report.json,run.json,atom_confusion.npy,atom_report.csv,atom_report.json}" % sdir)
        else:
            print("wrote %s/{confusion.npy,report.csv,report.json,run.json}" % sdir)
    if dp:
        dp[0].barrier()
        dp[0].destroy_process_group()


if __name__ == "__main__":
    main()
