"""Rotation augmentation drawn per epoch instead of baked into the dataset (train_unet.py / train_vae.py --augment).

The reference augments ahead of time: create_matrices.py --nrot 10 writes ten rotated copies of every compound, each three
quarter-turns about randomly chosen axis pairs (random_rotation_3d, reference utils.py:193-222).  Here the same tables are
drawn anew every epoch and applied while a batch is packed -- on the device by the rotating pack kernel of a fed step
(csrc/feed.hip), on the host by `rotate_host` everywhere else -- so a dataset needs no rotated files.

A rotation table is three entries in {-1, 0, 1, 2}, the r0, r1, r2 of ics_op_voxelise: entry r >= 0 is
np.rot90(X, 1, axes=ROTATION_AXES[r]), applied in the order r0, r1, r2; -1 is nothing.  It turns the three spatial axes of
every per-voxel array of a sample; channels travel with their voxel and no value changes (the reference rotates the
coordinate grids as pictures too: utils.py:216-218)."""
from __future__ import annotations

import numpy as np

from .matrices import ROTATION_AXES

IDENTITY = (-1, -1, -1)


def rotate_host(X, rot):
    """X (d,d,d[,c]) through the table `rot`: the np.rot90 composition, as a view."""
    for r in rot:
        if r >= 0:
            X = np.rot90(X, 1, axes=ROTATION_AXES[int(r)])
    return X


def draw_rotations(rng, n):
    """(n,3) int32 tables, every entry uniform in {0,1,2}: random_rotation_3d's distribution (utils.py:202-203)."""
    return rng.integers(0, 3, (int(n), 3)).astype(np.int32)


def epoch_plan(n_ids, n_rot, seed, epoch, rank=0, world=1, batch_size=1, fixed=False):
    """One epoch over n_ids compounds: every id once un-rotated and n_rot times with a drawn table, in shuffled order.
    Returns (index (m,) int64 into the id list, rotations (m,3) int32), this rank's share.

    Everything comes from np.random.default_rng([seed, epoch]) -- [seed] when `fixed`: the same plan every epoch, for a
    validation set whose loss has to stay comparable -- and never from the global np.random.  The plan is the same on
    every rank; a rank takes plan[rank::world], cut to the same whole number of batches on every rank (as
    dataparallel.shard_ids does: a rank with one batch more would wait for ever in the gradient all-reduce)."""
    n_ids, n_rot = int(n_ids), int(n_rot)
    rng = np.random.default_rng([int(seed)] if fixed else [int(seed), int(epoch)])
    index = np.repeat(np.arange(n_ids, dtype=np.int64), n_rot + 1)
    rot = np.full((n_ids, n_rot + 1, 3), -1, np.int32)
    rot[:, 1:] = draw_rotations(rng, n_ids * n_rot).reshape(n_ids, n_rot, 3)
    rot = rot.reshape(-1, 3)
    order = rng.permutation(len(index))
    index, rot = index[order], rot[order]
    n = len(index) // (int(world) * int(batch_size)) * int(batch_size)
    return index[rank::world][:n], rot[rank::world][:n]


class AugmentPlan:
    """What a generator keeps of --augment: (n_rot, seed, rank, world, fixed) and the epoch it is in."""

    def __init__(self, n_rot, seed=28, rank=0, world=1, fixed=False):
        self.n_rot, self.seed, self.rank, self.world, self.fixed = int(n_rot), int(seed), int(rank), int(world), bool(fixed)
        self.epoch = -1

    @classmethod
    def of(cls, augment):
        """an AugmentPlan, or one from a dict of its arguments"""
        return augment if isinstance(augment, cls) else cls(**augment)

    def next_epoch(self, n_ids, batch_size):
        self.epoch += 1
        return epoch_plan(n_ids, self.n_rot, self.seed, self.epoch, self.rank, self.world, batch_size, self.fixed)
