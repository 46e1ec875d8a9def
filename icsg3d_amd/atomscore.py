"""Atom-level scores of a segmentation, matched and tallied on the GPU (include/icsg3d.h "atom score",
csrc/atomscore.hip).  score() takes atom sets a caller brings, score_volumes() label volumes; both return the tallies as
a dict of int64 arrays that icsg3d_amd.atomreport turns into a report.  UnetEngine.atom_score_* accumulates the same
tallies over a whole split in the engine's own memory.

The rule: d2 = ((dx*dx + dy*dy) + dz*dz) in fp64; a pair is admissible when d2 < tol*tol, strictly; the matching is the
greedy one under the order (d2, true index, predicted index)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

# the tallies in the order the C entry points take them
TALLIES = ("matrix", "dist_q", "dist2_q", "dup", "shadowed", "hist", "totals")
TOTALS = ("samples", "failed", "perfect", "true_atoms", "pred_atoms", "matched", "abs_dn", "no_true")
HIST_BINS = 16
FIX = float(1 << 20)     # the fixed-point scale of dist_q / dist2_q


def empty_tallies(num_classes):
    k = max(int(num_classes), 0)
    return {"matrix": np.zeros((k + 1, k + 1), np.int64), "dist_q": np.zeros(k, np.int64), "dist2_q": np.zeros(k, np.int64),
            "dup": np.zeros(k, np.int64), "shadowed": np.zeros(k, np.int64), "hist": np.zeros(HIST_BINS, np.int64),
            "totals": np.zeros(len(TOTALS), np.int64)}


def limits():
    """(lanes per workgroup, atoms per side and sample, samples per launch, atoms per launch) of ics_op_atom_score"""
    v = [C.c_int(0) for _ in range(4)]
    L.check(L.load().ics_op_atom_score_limits(*[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def _ragged(sets, species):
    """a list of (n_i, 3) arrays and a list of (n_i,) species arrays -> (xyz (N, 3) float64, species int32, off int32)"""
    if len(sets) != len(species):
        raise ValueError("positions and species must have one entry per sample")
    off = np.zeros(len(sets) + 1, np.int32)
    xs, ss = [], []
    for i, (x, s) in enumerate(zip(sets, species)):
        x = np.asarray(x, np.float64).reshape(-1, 3)
        s = np.asarray(s, np.int32).reshape(-1)
        if len(x) != len(s):
            raise ValueError("sample %d: %d positions but %d species" % (i, len(x), len(s)))
        off[i + 1] = off[i] + len(x)
        xs.append(x)
        ss.append(s)
    xyz = np.ascontiguousarray(np.concatenate(xs) if xs else np.zeros((0, 3)), np.float64)
    return xyz, np.ascontiguousarray(np.concatenate(ss) if ss else np.zeros(0), np.int32), off


def score(true_xyz, true_species, pred_xyz, pred_species, num_classes, tol=2.0, per_sample=False):
    """ics_op_atom_score.  true_xyz / pred_xyz: one (n, 3) array of voxel positions per sample; true_species /
    pred_species: one (n,) array of ids in [0, num_classes) per sample.  Returns the tallies (TALLIES); with per_sample
    also "match" (one int32 array per sample: the predicted index of every true atom or -1), "sample_stats" int32
    (batch, 6) = {n_true, n_pred, matched, species_agree, dup, shadowed} and "dist_sum" float64 (batch,)."""
    return score_packed(*_ragged(true_xyz, true_species), *_ragged(pred_xyz, pred_species), num_classes, tol, per_sample)


def score_packed(t_xyz, t_sp, t_off, p_xyz, p_sp, p_off, num_classes, tol=2.0, per_sample=False):
    """score() on sets that are packed already, in ics_op_match_emd's layout: xyz (N, 3) float64, species (N,) int32 and
    off (batch + 1,) int32 per side."""
    t_xyz, p_xyz = np.ascontiguousarray(t_xyz, np.float64), np.ascontiguousarray(p_xyz, np.float64)
    t_sp, p_sp = np.ascontiguousarray(t_sp, np.int32), np.ascontiguousarray(p_sp, np.int32)
    t_off, p_off = np.ascontiguousarray(t_off, np.int32), np.ascontiguousarray(p_off, np.int32)
    if len(t_off) != len(p_off) or len(t_off) < 1:
        raise ValueError("true and predicted sets must have the same number of samples")
    if t_xyz.size != 3 * t_sp.size or p_xyz.size != 3 * p_sp.size or t_sp.size < t_off[-1] or p_sp.size < p_off[-1]:
        raise ValueError("positions, species and offsets do not fit together")
    batch = len(t_off) - 1
    out = empty_tallies(num_classes)
    match = np.full(max(int(t_off[-1]), 1), -1, np.int32) if per_sample else None
    stats = np.zeros((max(batch, 1), 6), np.int32) if per_sample else None
    dsum = np.zeros(max(batch, 1), np.float64) if per_sample else None
    L.check(L.load().ics_op_atom_score(L.f64ptr(t_xyz), L.i32ptr(t_sp), L.i32ptr(t_off), L.f64ptr(p_xyz), L.i32ptr(p_sp),
                                       L.i32ptr(p_off), batch, int(num_classes), float(tol),
                                       *[L.i64ptr(out[k]) for k in TALLIES], L.i32ptr(match), L.i32ptr(stats), L.f64ptr(dsum)))
    if per_sample:
        out["match"] = [match[t_off[i]:t_off[i + 1]].copy() for i in range(batch)]
        out["sample_stats"], out["dist_sum"] = stats[:batch], dsum[:batch]
    return out


def score_volumes(true_labels, pred_species, pred_mask, num_classes, tol=2.0, min_voxels=3, max_atoms=512, per_sample=False):
    """ics_op_atom_score_volumes.  Three uint8 volumes (batch, d, d, d): the true labels, the argmax species and the
    thresholded mask.  Predicted atoms are the mask's components above min_voxels voxels, true atoms all components of
    the label volume.  With per_sample also "match" int32 (batch, max_atoms), "sample_stats" and "dist_sum"."""
    t = np.ascontiguousarray(true_labels, np.uint8)
    s = np.ascontiguousarray(pred_species, np.uint8)
    m = np.ascontiguousarray(pred_mask, np.uint8)
    if t.ndim != 4 or t.shape[1] != t.shape[2] or t.shape[1] != t.shape[3] or s.shape != t.shape or m.shape != t.shape:
        raise ValueError("the three volumes must share one shape (batch, d, d, d)")
    batch, d = t.shape[0], t.shape[1]
    out = empty_tallies(num_classes)
    match = np.full((batch, max(int(max_atoms), 1)), -1, np.int32) if per_sample else None
    stats = np.zeros((batch, 6), np.int32) if per_sample else None
    dsum = np.zeros(batch, np.float64) if per_sample else None
    L.check(L.load().ics_op_atom_score_volumes(L.u8ptr(t), L.u8ptr(s), L.u8ptr(m), batch, d, int(min_voxels), int(max_atoms),
                                               int(num_classes), float(tol), *[L.i64ptr(out[k]) for k in TALLIES],
                                               L.i32ptr(match), L.i32ptr(stats), L.f64ptr(dsum)))
    if per_sample:
        out["match"], out["sample_stats"], out["dist_sum"] = match, stats, dsum
    return out
