"""The scoring of the reference's eval.py (/root/reference/eval.py:45-53,163-214): how far a reconstruction's atoms lie
from the true crystal's.

- emd               eval.py:45-53 -- cdist + linear_sum_assignment, matched distance sum / min(n, m) -- as one device
                    launch for a whole batch (ics_op_match_emd: exact fp64 shortest augmenting paths, one workgroup per
                    sample).  No host solver: a missing library is an error.
- predicted_coordinates
                    eval.py:172-175,207-209 -- atom centroids in voxels to Angstrom: mu * dv - eps * l + dv / 2, with l the
                    lattice parameters read from the reconstruction's coordinate channels (to_lattice_params).
- reconstruction_metrics
                    the per-sample numbers eval.py accumulates: EMD, |a, b, c true - predicted|, |N true - N predicted|;
                    failed samples are left out of every metric (eval.py:193-199, except: continue).
"""
from __future__ import annotations

import numpy as np

from . import _lib as L
from .utils import to_lattice_params_from_minmax, to_voxel_params

MAX_POINTS = 2048   # points per set ics_op_match_emd accepts


def _pack(sets):
    """list of (n, 3) arrays -> (xyz (N, 3) float64, offsets (len + 1,) int32)."""
    arrs = [np.asarray(s, np.float64).reshape(-1, 3) for s in sets]
    off = np.zeros(len(arrs) + 1, np.int32)
    off[1:] = np.cumsum([len(a) for a in arrs])
    xyz = np.ascontiguousarray(np.concatenate(arrs) if arrs and off[-1] else np.zeros((0, 3)), np.float64)
    return xyz, off


def emd(xs, ys, return_match=False):
    """emd(x, y) of eval.py:45-53 for every pair (xs[b], ys[b]): (B,) float64, NaN where either set is empty.  With
    return_match also the matching: per sample an int32 array of len(xs[b]) holding the index into ys[b] of each point
    of xs[b] (-1 = unmatched)."""
    if len(xs) != len(ys):
        raise ValueError("emd needs as many predicted as true point sets (%d != %d)" % (len(xs), len(ys)))
    if len(xs) == 0:
        return (np.zeros(0), []) if return_match else np.zeros(0)
    a, ao = _pack(xs)
    b, bo = _pack(ys)
    out = np.empty(len(xs), np.float64)
    match = np.empty(max(int(ao[-1]), 1), np.int32) if return_match else None
    L.check(L.load().ics_op_match_emd(L.f64ptr(a), L.i32ptr(ao), L.f64ptr(b), L.i32ptr(bo), len(xs), L.f64ptr(out),
                                      L.i32ptr(match)))
    if return_match:
        return out, [match[ao[k]:ao[k + 1]].copy() for k in range(len(xs))]
    return out


def predicted_coordinates(atoms, coord_minmax, eps_frac=0.25, d=32):
    """eval.py:172-175,207-209: per sample the atom centroids (atoms[b] = (species, means in voxels), as
    decode_to_atoms / reconstruct_to_atoms return them) in Angstrom, (n, 3) float64 each.  The lattice parameters come
    from the coordinate channels' min / max with to_lattice_params' default eps (0.25), as the reference calls it;
    eps_frac is the shift of eval.py:207 (--eps_frac)."""
    lp = to_lattice_params_from_minmax(coord_minmax, d=d)
    dv = to_voxel_params(lp, d=d)
    out = []
    for i, (species, mu) in enumerate(atoms):
        mu = np.array(mu, np.float64).reshape(len(species), 3)
        lpp = eps_frac * lp[i, :3].reshape(1, 3)
        out.append(mu * dv[i] - lpp + (dv[i] / 2.0))
    return out


def reconstruction_metrics(atoms, coord_minmax, true_xyz, true_lattice, failed=None, eps_frac=0.25, d=32):
    """Per-sample metrics of one batch, over the samples that did not fail (eval.py:177-214):
    dict(keep (B,) bool, emd (K,), lattice_true (K, 3), lattice_pred (K, 3), n_true (K,), n_pred (K,),
    species [K arrays], coords [K (n, 3) arrays]) -- K = number of kept samples, in batch order."""
    B = len(atoms)
    keep = np.ones(B, bool) if failed is None else ~np.asarray(failed, bool)
    coords = predicted_coordinates(atoms, coord_minmax, eps_frac, d)
    lp = to_lattice_params_from_minmax(coord_minmax, d=d)
    idx = np.flatnonzero(keep)
    pred = [coords[i] for i in idx]
    true = [np.asarray(true_xyz[i], np.float64).reshape(-1, 3) for i in idx]
    return {"keep": keep,
            "emd": emd(pred, true),
            "lattice_true": np.asarray(true_lattice, np.float64).reshape(B, -1)[idx, :3],
            "lattice_pred": lp[idx],
            "n_true": np.array([len(t) for t in true], np.int64),
            "n_pred": np.array([len(p) for p in pred], np.int64),
            "species": [np.asarray(atoms[i][0], np.int64) for i in idx],
            "coords": pred}
