"""Class weights for the U-Net loss (mirror of /root/reference/unet/get_weights.py:19-33): inverse
frequency of each species over the un-rotated training matrices; np.ones(n) when no path is given
(the form `custom_objects` uses).  Note SURVEY F11: the reference's training loss never uses them;
AtomUnet(weighted_loss=True) does."""
import os

import numpy as np

_CHUNK_BYTES = 64 << 20      # device=True: species files are gathered into chunks of about this size per histogram call


def _species_files(path, training_ids):
    ids = set(training_ids)
    folder = os.path.join(path, "species_matrices")
    for fname in os.listdir(folder):
        if not fname.endswith(".npy") or "_rot_" in fname or fname not in ids:
            continue
        yield os.path.join(folder, fname)


def _device_counts(files, n_classes):
    """The host loop's counts from ics_op_label_counts: exact integers, so the order of files and chunks is irrelevant."""
    from ..engine import label_counts
    total = np.zeros(n_classes, np.int64)

    def flush(parts):
        if not parts:
            return
        c, oor = label_counts(np.concatenate(parts), n_classes)
        if oor:
            raise IndexError("%d species values are not class ids in 0..%d" % (oor, n_classes - 1))
        total[:] += c

    parts, size, dtype = [], 0, None
    for f in files:
        a = np.load(f).reshape(-1)
        if a.dtype not in (np.uint8, np.float32, np.float64):
            a = a.astype(np.float64)
        if parts and (a.dtype != dtype or size + a.nbytes > _CHUNK_BYTES):
            flush(parts)
            parts, size = [], 0
        parts.append(a)
        size, dtype = size + a.nbytes, a.dtype
    flush(parts)
    return total.astype(np.float64)


def get_weights(path="", training_ids=(), n_classes=95, device=False):
    """device=True: the species files are loaded in chunks and counted on the GPU (label_counts_kernel); the weights are
    element for element those of the host loop.  A species value that is no class id raises IndexError."""
    if not path:
        return np.ones(n_classes)
    if device:
        counts = _device_counts(_species_files(path, training_ids), n_classes)
    else:
        counts = np.zeros(n_classes)
        for fname in _species_files(path, training_ids):
            values, n = np.unique(np.load(fname), return_counts=True)
            for v, c in zip(values, n):
                counts[int(v)] += c
    with np.errstate(divide="ignore"):
        w = counts.sum() / counts
    w[np.isinf(w)] = 0
    return w
