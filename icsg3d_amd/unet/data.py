"""U-Net batch generators: same `__len__/__getitem__/on_epoch_end` contract as
/root/reference/unet/data.py:20-100 (X (B,d,d,d,C), [y, b]) over the same on-disk layout
data/<name>/matrices/{density_matrices,species_matrices,coordinate_grids}/<id>.npy.
y is handed over as uint8 class ids (the engine's native label format) unless one_hot=True.

augment (an icsg3d_amd.augment.AugmentPlan or a dict of its arguments): list_IDs are base ids, and every epoch follows a
freshly drawn plan -- each id once as it is and n_rot times through a drawn rotation table (augment.epoch_plan).
__getitem__ rotates on the host; fill writes the raw payloads and rotations(index) hands the batch's table to the feed."""
import os

import numpy as np

from ..augment import AugmentPlan, rotate_host
from ..synthetic import synthetic_batch


_FEED_LABEL_KINDS = {np.dtype(np.uint8): "u8", np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}


def _raw(path):
    """a saved grid as it lies in its file: memory-mapped, no copy, no cast"""
    return np.load(path, mmap_mode="r")


def _read_into(path, dst):
    """The payload of a saved grid into dst, a flat C-contiguous view of a staging slot.  A file of dst's dtype is read
    straight into it (one copy, no temporary array, no mapping to set up and tear down per file: with two files per
    sample that overhead, not the bytes, bounded a fed DFC-VAE loop: DESIGN section 24, "Before"); any other file is
    loaded and cast while copied.  read_magic / read_array_header_1_0 / _2_0 are numpy.lib.format's documented readers of
    the .npy header (what np.load itself calls); a file of a later format version takes the np.load path."""
    F = np.lib.format
    with open(path, "rb") as f:
        version = F.read_magic(f)
        if version in ((1, 0), (2, 0)):
            shape, fortran, dtype = (F.read_array_header_1_0 if version == (1, 0) else F.read_array_header_2_0)(f)
            if dtype == dst.dtype and not dtype.hasobject and int(np.prod(shape)) == dst.size and (not fortran or len(shape) <= 1):
                if f.readinto(memoryview(dst).cast("B")) != dst.nbytes:
                    raise ValueError("%s is shorter than its header says" % path)
                return
    np.copyto(dst, np.load(path).reshape(-1), casting="unsafe")


def _feed_x_spec(data_path, ID, n_channels):
    """(x_channels, x_dtypes) of the files behind create_lattice_meshgrid, or None when the pack kernel does not read them"""
    names = ["density_matrices"] + (["coordinate_grids"] if n_channels != 1 else [])
    dts = tuple(_raw(os.path.join(data_path, n, ID)).dtype for n in names)
    if n_channels not in (1, 4) or any(t not in (np.dtype(np.float32), np.dtype(np.float64)) for t in dts):
        return None
    return ((1,) if n_channels == 1 else (1, 3)), dts


def _fill_x(data_path, ID, views, i):
    """sample i of a slot: the density grid into part 0, the coordinate grids into part 1, as raw payloads"""
    _read_into(os.path.join(data_path, "density_matrices", ID), views["x"][0][i].reshape(-1))
    if len(views["x"]) == 2:
        _read_into(os.path.join(data_path, "coordinate_grids", ID), views["x"][1][i].reshape(-1))


class UnetDataGenerator:
    def __init__(self, list_IDs, data_path, batch_size=2, dim=(32, 32, 32), n_channels=7, n_classes=95,
                 shuffle=False, one_hot=False, augment=None):
        self.dim, self.batch_size, self.list_IDs = tuple(dim), batch_size, list(list_IDs)
        self.n_channels, self.n_classes, self.shuffle = n_channels, n_classes, shuffle
        self.data_path, self.one_hot = data_path, one_hot
        self.augment = None if augment is None else AugmentPlan.of(augment)
        self.on_epoch_end()

    def __len__(self):
        if self.augment is not None:
            return len(self.indexes) // self.batch_size
        return int(np.floor(len(self.list_IDs) / self.batch_size))

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def on_epoch_end(self):
        if self.augment is not None:                 # the next epoch's plan, shuffled by its own generator
            self.indexes, self.rot = self.augment.next_epoch(len(self.list_IDs), self.batch_size)
            return
        self.indexes = np.arange(len(self.list_IDs))
        if self.shuffle:
            np.random.shuffle(self.indexes)

    def rotations(self, index):
        """the rotation table (B,3) of batch `index`, None without augment"""
        return None if self.augment is None else self.rot[index * self.batch_size:(index + 1) * self.batch_size]

    def __getitem__(self, index):
        idx = self.indexes[index * self.batch_size:(index + 1) * self.batch_size]
        rot = self.rotations(index)
        self.list_IDs_temp = [self.list_IDs[k] for k in idx]
        X = np.empty((self.batch_size, *self.dim, self.n_channels), np.float32)
        y = np.empty((self.batch_size, *self.dim), np.uint8)
        for i, ID in enumerate(self.list_IDs_temp):
            X[i] = self.create_lattice_meshgrid(ID, self.n_channels)
            y[i] = np.load(os.path.join(self.data_path, "species_matrices", ID)).reshape(self.dim)
            if rot is not None:
                X[i], y[i] = rotate_host(X[i], rot[i]).copy(), rotate_host(y[i], rot[i]).copy()
        b = (y != 0).astype(np.float32)[..., None]
        if self.one_hot:
            y = np.eye(self.n_classes, dtype=np.float32)[y]
        return X, [y, b]

    def create_lattice_meshgrid(self, ID, channels=4):
        M = np.load(os.path.join(self.data_path, "density_matrices", ID)).reshape(*self.dim, 1)
        if channels == 1:
            return M
        p = np.load(os.path.join(self.data_path, "coordinate_grids", ID)).reshape(*self.dim, 3)
        return np.concatenate((M, p), axis=-1)

    # ---- fed steps (icsg3d_amd.feed.Feeder): the files' payloads go into a staging slot as they are; the cast to float32,
    # the (M | p) concatenate and the uint8 labels happen on the device
    def feed_spec(self):
        """(x_channels, x_dtypes, label_kind) of the files, or None: then the Feeder copies __getitem__'s arrays"""
        if not self.list_IDs:
            return None
        x = _feed_x_spec(self.data_path, self.list_IDs[0], self.n_channels)
        # ids saved in another dtype (integers, say) are cast to uint8 on the host while they are copied: a byte per voxel
        kind = _FEED_LABEL_KINDS.get(_raw(os.path.join(self.data_path, "species_matrices", self.list_IDs[0])).dtype, "u8")
        return None if x is None else x + (kind,)

    def fill(self, index, views, map=lambda f, it: [f(i) for i in it]):
        """batch `index` into the views of a slot (UnetEngine.feed_slot), one sample per call of `map`; returns its size"""
        ids = [self.list_IDs[k] for k in self.indexes[index * self.batch_size:(index + 1) * self.batch_size]]

        def one(i):
            _fill_x(self.data_path, ids[i], views, i)
            _read_into(os.path.join(self.data_path, "species_matrices", ids[i]), views["labels"][i].reshape(-1))

        map(one, range(len(ids)))
        return len(ids)


class SyntheticUnetGenerator:
    """Same contract, Gaussian-blob grids of SURVEY 8(d) instead of files (no dataset offline)."""

    def __init__(self, n_samples, batch_size=2, dim=(32, 32, 32), n_channels=1, n_classes=95, seed=0, shuffle=False):
        self.batch_size, self.dim, self.n_channels, self.n_classes = batch_size, tuple(dim), n_channels, n_classes
        self.list_IDs = ["synthetic_%06d" % i for i in range(n_samples)]
        self.seed, self.shuffle = seed, shuffle
        self.on_epoch_end()

    def __len__(self):
        return len(self.list_IDs) // self.batch_size

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def on_epoch_end(self):
        self.indexes = np.arange(len(self.list_IDs))
        if self.shuffle:
            np.random.shuffle(self.indexes)

    def __getitem__(self, index):
        X, lab, _ = synthetic_batch(self.batch_size, self.dim[0], self.n_channels, seed=self.seed + index, noise=1e-3)
        return X, [lab, (lab != 0).astype(np.float32)[..., None]]
