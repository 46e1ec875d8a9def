"""The last stage of the reference's generate.py (generate.py:250-318, utils.py:225-239): the periodic
structure of every generated sample, its formula, the validity screen and the CIF file.

The reference builds a pymatgen Structure per sample; pymatgen is not a dependency here.  Its semantics are restated
(parity with pymatgen is UNPINNED: no fixture can be recorded from it -- DESIGN section 16):

- screen            to_pymatgen_structure + structure.is_valid() for a whole batch in one device call
                    (ics_op_structure_screen: exact fp64 shortest periodic distances over all lattice translations).
                    No host fallback: a missing library is an error.
- formula, reduced_formula, anonymized_formula, average_electroneg
                    Composition's, from the species histogram the op returns.
- write_cif / read_cif
                    a P1 CIF 1.1 file as CifWriter lays it out, and a reader for that subset.
- numbered          the duplicate-formula numbering of generate.py:257-260.
- ResultsWriter     generate.py:250-318 around them: per batch one screen, then per valid sample the CIF, the results
                    row and the results.json record; results.csv at the end.
- match, Matcher, ReferenceSet, eligibility, match_packed, signed_permutations
                    which written samples are the same crystal as an earlier one and which are a training structure
                    (ics_op_structure_match: the project's own predicate; no parity with pymatgen's
                    StructureMatcher is claimed).  No host fallback either.
- symmetry, Symmetriser, symmetry_packed, lattice_op, POINT_GROUPS, write_cif_symmetry, read_cif_symmetry, expand_symmetry
                    which symmetry a written sample has: its operations (W, t), point group, crystal system, centring
                    translations, orbits and the symmetrised structure (ics_op_structure_symmetry: the project's own
                    predicate; no parity with spglib or pymatgen's SpacegroupAnalyzer is claimed, no
                    space-group name or number is produced).
- fingerprint, Fingerprinter, fingerprint_packed, fingerprint_nearest
                    how close a written sample is to the training set and to the other samples: a radial distribution
                    function per crystal (plain and Z-weighted) with every atom's nearest distance and coordination
                    number (ics_op_structure_fingerprint), and the nearest partners by rms distance between fingerprints
                    with the run's coverage and diversity (ics_op_fingerprint_nearest).  The project's own descriptor,
                    DESIGN section 29; no parity with pymatgen's or matminer's fingerprints is claimed.  No host fallback.
"""
from __future__ import annotations

import csv
import json
import math
import os
import string
from functools import reduce

import numpy as np

from . import _lib as L

MAX_ATOMS = 2048        # atoms per structure ics_op_structure_screen accepts
HIST = 95               # histogram row: atomic numbers 0..94
MAX_IMAGE = 32          # lattice translations per axis its image search covers
REASON_CLOSE, REASON_SPECIES, REASON_EMPTY = 1, 2, 4     # the op's reason bits
REASON_CELL = 8         # set here: the sample's own cell lengths or coordinates are not finite and positive
REASONS = {REASON_CLOSE: "atoms closer than tol", REASON_SPECIES: "species outside 1..94", REASON_EMPTY: "no atoms",
           REASON_CELL: "no cell"}

# Element symbols by atomic number 1..94 and Pauling electronegativities (public tables; None = no value).
SYMBOLS = ("X H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Y Zr "
           "Nb Mo Tc Ru Rh Pd Ag Cd In Sn Sb Te I Xe Cs Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho Er Tm Yb Lu Hf Ta W Re Os Ir "
           "Pt Au Hg Tl Pb Bi Po At Rn Fr Ra Ac Th Pa U Np Pu").split()
ELECTRONEG = (None, 2.20, None, 0.98, 1.57, 2.04, 2.55, 3.04, 3.44, 3.98, None, 0.93, 1.31, 1.61, 1.90, 2.19, 2.58, 3.16,
              None, 0.82, 1.00, 1.36, 1.54, 1.63, 1.66, 1.55, 1.83, 1.88, 1.91, 1.90, 1.65, 1.81, 2.01, 2.18, 2.55, 2.96,
              3.00, 0.82, 0.95, 1.22, 1.33, 1.60, 2.16, 1.90, 2.20, 2.28, 2.20, 1.93, 1.69, 1.78, 1.96, 2.05, 2.10, 2.66,
              2.60, 0.79, 0.89, 1.10, 1.12, 1.13, 1.14, 1.13, 1.17, 1.20, 1.20, 1.10, 1.22, 1.23, 1.24, 1.25, 1.10, 1.27,
              1.30, 1.50, 2.36, 1.90, 2.20, 2.20, 2.28, 2.54, 2.00, 1.62, 2.33, 2.02, 2.00, 2.20, 2.20, 0.70, 0.90, 1.10,
              1.30, 1.50, 1.38, 1.36, 1.28)
assert len(SYMBOLS) == HIST and len(ELECTRONEG) == HIST


# ---------------------------------------------------------------- composition
def _ordered(hist):
    """[(Z, amount)] of the elements present, ordered as Composition.formula: by electronegativity, elements without a
    value last, ties by Z."""
    hist = np.asarray(hist).reshape(-1)
    zs = [z for z in range(1, min(len(hist), HIST)) if hist[z] > 0]
    return [(z, int(hist[z])) for z in sorted(zs, key=lambda z: (ELECTRONEG[z] is None, ELECTRONEG[z] or 0.0, z))]


def formula(hist):
    """Composition.formula: "La1 Fe1 O3"."""
    return " ".join("%s%d" % (SYMBOLS[z], n) for z, n in _ordered(hist))


def reduced_formula(hist):
    """The amounts divided by their gcd, 1s dropped: "LaFeO3"."""
    el = _ordered(hist)
    if not el:
        return ""
    g = reduce(math.gcd, [n for _, n in el])
    return "".join(SYMBOLS[z] + (str(n // g) if n // g != 1 else "") for z, n in el)


def anonymized_formula(hist):
    """Composition.anonymized_formula: reduced amounts ascending, letters A, B, C...: "ABC3"."""
    el = _ordered(hist)
    if not el:
        return ""
    g = reduce(math.gcd, [n for _, n in el])
    return "".join(c + (str(n) if n != 1 else "") for c, n in zip(string.ascii_uppercase, sorted(n // g for _, n in el)))


def average_electroneg(hist):
    """Composition.average_electroneg: the amount-weighted mean; NaN when an element has no value or there is no atom."""
    el = _ordered(hist)
    if not el or any(ELECTRONEG[z] is None for z, _ in el):
        return float("nan")
    return sum(ELECTRONEG[z] * n for z, n in el) / sum(n for _, n in el)


def numbered(name, seen):
    """generate.py:257-260: name + "_" + str(count) when `name` occurs `count` > 0 times in `seen`."""
    c = list(seen).count(name)
    return name + "_" + str(c) if c else name


# ---------------------------------------------------------------- the device screen
def cell(abc, angles):
    """Lattice.from_parameters as ics_op_structure_screen builds it: (lattice (3, 3) with rows va, vb, vc, volume, norms
    of the columns of its inverse).  Sine and cosine of exactly 90 degrees are 1 and 0.  ValueError for angles that
    make no cell."""
    a, b, c = (float(v) for v in abc)
    ang = [float(t) for t in angles]
    if not all(0.0 < t < 180.0 for t in ang):
        raise ValueError("angles %s make no cell" % (ang,))
    sn = [1.0 if t == 90.0 else math.sin(math.radians(t)) for t in ang]
    cs = [0.0 if t == 90.0 else math.cos(math.radians(t)) for t in ang]
    val = (cs[0] * cs[1] - cs[2]) / (sn[0] * sn[1])
    if not abs(val) < 1.0:
        raise ValueError("angles %s make no cell" % (ang,))
    gs = math.acos(val)
    M = np.array([[a * sn[1], 0.0, a * cs[1]], [-b * sn[0] * math.cos(gs), b * sn[0] * math.sin(gs), b * cs[0]],
                  [0.0, 0.0, c]])
    vol = float(np.dot(M[0], np.cross(M[1], M[2])))
    if not vol > 0.0:
        raise ValueError("angles %s make no cell" % (ang,))
    g = np.array([np.linalg.norm(np.cross(M[1], M[2])), np.linalg.norm(np.cross(M[2], M[0])),
                  np.linalg.norm(np.cross(M[0], M[1]))]) / vol
    return M, vol, g


def screen_packed(offsets, species, xyz, abc, angles, tol=0.5):
    """ics_op_structure_screen on packed arrays: offsets (B + 1,), species (N,), xyz (N, 3), abc and angles (B, 3).
    Returns the op's outputs as a dict of arrays."""
    offsets = np.ascontiguousarray(offsets, np.int32)
    B = len(offsets) - 1
    if B < 1:
        raise ValueError("screen needs at least one structure")
    species = np.ascontiguousarray(species, np.int32).reshape(-1)
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    abc = np.ascontiguousarray(abc, np.float64).reshape(-1, 3)
    angles = np.ascontiguousarray(angles, np.float64).reshape(-1, 3)
    N = len(species)
    if len(xyz) != N or len(abc) != B or len(angles) != B or (B >= 1 and int(offsets[-1]) != N):
        raise ValueError("screen: array lengths do not agree (atoms %d / %d / %d, structures %d / %d / %d)"
                         % (N, len(xyz), int(offsets[-1]), B, len(abc), len(angles)))
    out = {"lattice": np.zeros((B, 3, 3)), "volume": np.zeros(B), "frac": np.zeros((max(N, 1), 3)),
           "min_dist": np.zeros(B), "min_pair": np.zeros((B, 2), np.int32), "n_close": np.zeros(B, np.int32),
           "valid": np.zeros(B, np.int32), "reason": np.zeros(B, np.int32), "nearest": np.zeros(max(N, 1)),
           "hist": np.zeros((B, HIST), np.int32)}
    L.check(L.load().ics_op_structure_screen(
        L.i32ptr(offsets), L.i32ptr(species), L.f64ptr(xyz), L.f64ptr(abc), L.f64ptr(angles), B, float(tol),
        L.f64ptr(out["lattice"]), L.f64ptr(out["volume"]), L.f64ptr(out["frac"]), L.f64ptr(out["min_dist"]),
        L.i32ptr(out["min_pair"]), L.i32ptr(out["n_close"]), L.i32ptr(out["valid"]), L.i32ptr(out["reason"]),
        L.f64ptr(out["nearest"]), L.i32ptr(out["hist"])))
    out["frac"], out["nearest"] = out["frac"][:N], out["nearest"][:N]
    return out


def screen(lattice_params, atoms, alpha=90, beta=90, gamma=90, tol=0.5):
    """to_pymatgen_structure(l_prime[b], coords, alpha, beta, gamma) and is_valid(tol) for every sample of a batch.
    lattice_params (B, 3); atoms[b] = (species (n,), xyz (n, 3) in Angstrom) or None for a sample to leave out (a failed
    one).  One device call for the batch.  Returns a list of B entries: None where atoms[b] is None, else a dict
    (species, frac (n, 3), abc, angles, lattice (3, 3), volume, min_dist, min_pair, n_close, nearest (n,), hist (95,),
    valid, reason, formula).  A sample whose own numbers make no cell (non-finite or non-positive lengths, non-finite
    coordinates, more than 2048 atoms) is returned invalid with reason REASON_CELL instead of failing the batch; angles
    that make no cell are the caller's and raise."""
    lp = np.asarray(lattice_params, np.float64).reshape(-1, 3)
    if len(lp) != len(atoms):
        raise ValueError("screen: %d lattice parameter rows for %d samples" % (len(lp), len(atoms)))
    angles = np.array([alpha, beta, gamma], np.float64)
    cell(np.ones(3), angles)      # raises for angles that make no cell
    res = [None] * len(atoms)
    keep, sp_l, xyz_l = [], [], []
    for b, at in enumerate(atoms):
        if at is None:
            continue
        sp = np.asarray(at[0], np.int64).reshape(-1)
        xyz = np.asarray(at[1], np.float64).reshape(len(sp), 3)
        ok = (np.all(np.isfinite(lp[b])) and np.all(lp[b] >= 1e-6) and np.all(lp[b] <= 1e6) and np.all(np.isfinite(xyz))
              and np.all(np.abs(xyz) <= 1e12) and len(sp) <= MAX_ATOMS and np.all(np.abs(sp) < 2 ** 31))
        # the op's image search covers 32 translations per axis (it refuses the whole call above that)
        ok = ok and 0.5 * lp[b].sum() * cell(lp[b], angles)[2].max() + 0.5 <= MAX_IMAGE - 0.1
        if not ok:
            hist = np.bincount(sp[(sp >= 1) & (sp < HIST)], minlength=HIST).astype(np.int32)
            res[b] = {"species": sp.astype(np.int32), "frac": np.full((len(sp), 3), np.nan), "abc": lp[b].copy(),
                      "angles": angles.copy(), "lattice": np.full((3, 3), np.nan), "volume": float("nan"),
                      "min_dist": float("nan"), "min_pair": (-1, -1), "n_close": 0, "nearest": np.full(len(sp), np.nan),
                      "hist": hist, "valid": False, "reason": REASON_CELL, "formula": formula(hist)}
            continue
        keep.append(b)
        sp_l.append(sp.astype(np.int32))
        xyz_l.append(xyz)
    if not keep:
        return res
    off = np.zeros(len(keep) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in sp_l])
    o = screen_packed(off, np.concatenate(sp_l), np.concatenate(xyz_l), lp[keep], np.tile(angles, (len(keep), 1)), tol)
    for k, b in enumerate(keep):
        a0, a1 = int(off[k]), int(off[k + 1])
        res[b] = {"species": sp_l[k], "frac": o["frac"][a0:a1].copy(), "abc": lp[b].copy(), "angles": angles.copy(),
                  "lattice": o["lattice"][k].copy(), "volume": float(o["volume"][k]), "min_dist": float(o["min_dist"][k]),
                  "min_pair": (int(o["min_pair"][k, 0]), int(o["min_pair"][k, 1])), "n_close": int(o["n_close"][k]),
                  "nearest": o["nearest"][a0:a1].copy(), "hist": o["hist"][k].copy(), "valid": bool(o["valid"][k]),
                  "reason": int(o["reason"][k]), "formula": formula(o["hist"][k])}
    return res


# ---------------------------------------------------------------- structure matching (ics_op_structure_match)
MATCH_MAX_ATOMS = 256   # atoms per structure the match kernel takes
OPS_MODES = {"none": 0, "rot": 1, "all": 2}
# reason bits of a structure that is never compared (eligibility)
INELIGIBLE_ATOMS, INELIGIBLE_CLOSE, INELIGIBLE_THIN, INELIGIBLE_INVALID = 1, 2, 4, 8
INELIGIBLE = {INELIGIBLE_ATOMS: "more than 256 atoms", INELIGIBLE_CLOSE: "atoms within 4 tol",
              INELIGIBLE_THIN: "cell too thin for tol", INELIGIBLE_INVALID: "invalid or failed"}


def signed_permutations(ops_mode=1):
    """The op table of ics_op_structure_match, (k, 3, 3) with f' = P f: lexicographic over (permutation, sign pattern),
    + before -, identity first.  ops_mode 0: the identity; 1: the 24 of determinant +1 in that order; 2: all 48."""
    if ops_mode not in (0, 1, 2):
        raise ValueError("ops_mode must be 0, 1 or 2")
    perms = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
    parity = (1, -1, -1, 1, 1, -1)
    ops = []
    for perm, par in zip(perms, parity):
        for s in range(8):
            sign = (-1 if s & 4 else 1, -1 if s & 2 else 1, -1 if s & 1 else 1)
            if (ops_mode == 0 and ops) or (ops_mode == 1 and par * sign[0] * sign[1] * sign[2] != 1):
                continue
            P = np.zeros((3, 3))
            for k in range(3):
                P[k, perm[k]] = sign[k]
            ops.append(P)
    return np.array(ops)


def eligibility(results, tol=0.1):
    """The reason bits (0 = eligible) per entry of `results` (the dicts screen returns; None = a failed sample): more
    than 256 atoms, screen min_dist <= 4 tol, 2 tol max(g) >= 0.5 for the inverse-column norms g of the cell, invalid or
    failed.  With these the predicate means "the same crystal": only the wrapped image can lie within 2 tol, and the
    nearest-atom map is forced to be a bijection."""
    out = np.zeros(len(results), np.int32)
    for k, r in enumerate(results):
        if r is None or not r["valid"] or len(r["species"]) == 0 or not np.all(np.isfinite(r["lattice"])):
            out[k] = INELIGIBLE_INVALID
            continue
        if len(r["species"]) > MATCH_MAX_ATOMS:
            out[k] |= INELIGIBLE_ATOMS
        if r["min_dist"] <= 4.0 * tol:
            out[k] |= INELIGIBLE_CLOSE
        g = np.linalg.norm(np.linalg.inv(np.asarray(r["lattice"], np.float64)), axis=0)
        if not 2.0 * tol * g.max() < 0.5:
            out[k] |= INELIGIBLE_THIN
    return out


def ineligible_text(bits):
    return ", ".join(t for bit, t in INELIGIBLE.items() if bits & bit) or "eligible"


def match_packed(offsets, species, frac, lattice, eligible, nq, nref, tol=0.1, ltol=0.05, ops_mode=1):
    """ics_op_structure_match on packed arrays: nq queries then nref references; offsets (nq + nref + 1,), species (N,),
    frac (N, 3), lattice (nq + nref, 3, 3) with rows va, vb, vc, eligible (nq + nref,).  Returns the op's outputs as a
    dict of arrays (dup_of, dup_rms, dup_op (nq, 2) = (op, anchor), ref_of, ref_rms, ref_op, n_cmp (nq, 2))."""
    offsets = np.ascontiguousarray(offsets, np.int32)
    species = np.ascontiguousarray(species, np.int32).reshape(-1)
    frac = np.ascontiguousarray(frac, np.float64).reshape(-1, 3)
    lattice = np.ascontiguousarray(lattice, np.float64).reshape(-1, 9)
    eligible = np.ascontiguousarray(eligible, np.int32).reshape(-1)
    nq, nref = int(nq), int(nref)
    ns = nq + nref
    if nq >= 1 and nref >= 0 and (len(offsets) != ns + 1 or len(lattice) != ns or len(eligible) != ns
                                  or len(frac) != len(species) or int(offsets[-1]) != len(species)):
        raise ValueError("match: array lengths do not agree (structures %d / %d / %d / %d, atoms %d / %d / %d)"
                         % (ns, len(offsets) - 1, len(lattice), len(eligible), len(species), len(frac), int(offsets[-1])))
    n = max(nq, 1)
    out = {"dup_of": np.full(n, -1, np.int32), "dup_rms": np.full(n, np.inf), "dup_op": np.full((n, 2), -1, np.int32),
           "ref_of": np.full(n, -1, np.int32), "ref_rms": np.full(n, np.inf), "ref_op": np.full((n, 2), -1, np.int32),
           "n_cmp": np.zeros((n, 2), np.int32)}
    L.check(L.load().ics_op_structure_match(
        L.i32ptr(offsets), L.i32ptr(species), L.f64ptr(frac), L.f64ptr(lattice), L.i32ptr(eligible), nq, nref, float(tol),
        float(ltol), int(ops_mode), L.i32ptr(out["dup_of"]), L.f64ptr(out["dup_rms"]), L.i32ptr(out["dup_op"]),
        L.i32ptr(out["ref_of"]), L.f64ptr(out["ref_rms"]), L.i32ptr(out["ref_op"]), L.i32ptr(out["n_cmp"])))
    return out


class ReferenceSet:
    """The structures generated samples are held against: ids, species, fractional coordinates as stored, and the
    lattice of the six parameters through cell().  from_sites reads data/<name>/sites/*.npz (matrices.load_sites),
    sorted by file name.  screened() runs the device screen over the set once (tol 0: only coincident atoms, a species
    outside 1..94 or no atoms make a reference invalid) and keeps its dicts -- min_dist is what eligibility needs."""

    def __init__(self, ids, species, frac, lattice_params):
        self.ids = [str(i) for i in ids]
        self.species = [np.asarray(s, np.int32).reshape(-1) for s in species]
        self.frac = [np.asarray(f, np.float64).reshape(len(s), 3) for f, s in zip(frac, self.species)]
        self.lattice_params = np.asarray(lattice_params, np.float64).reshape(len(self.ids), 6)
        if not len(self.ids) == len(self.species) == len(self.frac):
            raise ValueError("ReferenceSet: ids, species and frac differ in length")
        self._screened = None
        self._fingerprints = {}       # (r_max, n_bins, width, cn_tol) -> fingerprint(self.screened(), ...): Fingerprinter's

    @classmethod
    def from_sites(cls, folder):
        from .matrices import load_sites
        names = sorted(f for f in os.listdir(folder) if f.endswith(".npz"))
        ids, sp, fr, lp = [], [], [], []
        for f in names:
            frac, Z, _, lattice = load_sites(os.path.join(folder, f))
            ids.append(f[:-4])
            sp.append(np.rint(Z).astype(np.int32))
            fr.append(frac)
            lp.append(np.asarray(lattice, np.float64).reshape(-1)[:6])
        return cls(ids, sp, fr, np.array(lp, np.float64).reshape(len(ids), 6))

    def __len__(self):
        return len(self.ids)

    def screened(self):
        """One dict per reference in screen()'s layout (frac: the stored coordinates), or None where the six parameters
        make no usable cell."""
        if self._screened is not None:
            return self._screened
        res, keep, cells = [None] * len(self), [], []
        for k in range(len(self)):
            abc, ang, sp, fr = self.lattice_params[k, :3], self.lattice_params[k, 3:], self.species[k], self.frac[k]
            try:
                ok = (np.all(np.isfinite(abc)) and np.all(abc >= 1e-6) and np.all(abc <= 1e6) and np.all(np.isfinite(fr))
                      and np.all(np.abs(fr) <= 1e6) and len(sp) <= MAX_ATOMS)
                M, vol, g = cell(abc, ang)
                ok = ok and 0.5 * abc.sum() * g.max() + 0.5 <= MAX_IMAGE - 0.1
            except ValueError:
                ok = False
            if ok:
                keep.append(k)
                cells.append((M, vol))
        if keep:
            off = np.zeros(len(keep) + 1, np.int32)
            off[1:] = np.cumsum([len(self.species[k]) for k in keep])
            o = screen_packed(off, np.concatenate([self.species[k] for k in keep]),
                              np.concatenate([self.frac[k] * self.lattice_params[k, :3] for k in keep]),
                              self.lattice_params[keep, :3], self.lattice_params[keep, 3:], 0.0)
            for i, k in enumerate(keep):
                res[k] = {"species": self.species[k], "frac": self.frac[k], "abc": self.lattice_params[k, :3].copy(),
                          "angles": self.lattice_params[k, 3:].copy(), "lattice": cells[i][0], "volume": cells[i][1],
                          "min_dist": float(o["min_dist"][i]), "hist": o["hist"][i].copy(), "valid": bool(o["valid"][i]),
                          "reason": int(o["reason"][i])}
        self._screened = res
        return res


def match(results, reference=None, tol=0.1, ltol=0.05, ops_mode=1):
    """Duplicates and training hits of a run.  results: the dicts screen returns, in sample order (None = failed);
    reference: a ReferenceSet or None.  One device call.  Returns one dict per sample: duplicate_of (index into results
    of the first earlier sample that is the same structure, -1 if none), duplicate_rms, duplicate_op (op, anchor),
    training_match (the reference's id, None if none), training_rms, training_op, match_reason (eligibility bits: a
    sample with a bit set was not compared), n_compared (earlier samples, references)."""
    nq = len(results)
    qbits = eligibility(results, tol)
    out = [{"duplicate_of": -1, "duplicate_rms": None, "duplicate_op": (-1, -1), "training_match": None,
            "training_rms": None, "training_op": (-1, -1), "match_reason": int(qbits[k]), "n_compared": (0, 0)}
           for k in range(nq)]
    if nq == 0 or not np.any(qbits == 0):
        return out
    refs = reference.screened() if reference is not None and len(reference) else []
    allr = list(results) + list(refs)
    bits = np.concatenate([qbits, eligibility(refs, tol)])
    sp_l, fr_l, lat = [], [], np.zeros((len(allr), 3, 3))
    for k, r in enumerate(allr):
        if bits[k] == 0:
            sp_l.append(np.asarray(r["species"], np.int32))
            fr_l.append(np.asarray(r["frac"], np.float64).reshape(-1, 3))
            lat[k] = r["lattice"]
        else:                                   # not compared: passed as an empty, ineligible entry
            sp_l.append(np.zeros(0, np.int32))
            fr_l.append(np.zeros((0, 3)))
    off = np.zeros(len(allr) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in sp_l])
    o = match_packed(off, np.concatenate(sp_l), np.concatenate(fr_l), lat, (bits == 0).astype(np.int32), nq, len(refs),
                     tol, ltol, ops_mode)
    for k in range(nq):
        d = out[k]
        d["n_compared"] = (int(o["n_cmp"][k, 0]), int(o["n_cmp"][k, 1]))
        if o["dup_of"][k] >= 0:
            d["duplicate_of"], d["duplicate_rms"] = int(o["dup_of"][k]), float(o["dup_rms"][k])
            d["duplicate_op"] = (int(o["dup_op"][k, 0]), int(o["dup_op"][k, 1]))
        if o["ref_of"][k] >= 0:
            d["training_match"], d["training_rms"] = reference.ids[int(o["ref_of"][k])], float(o["ref_rms"][k])
            d["training_op"] = (int(o["ref_op"][k, 0]), int(o["ref_op"][k, 1]))
    return out


class Matcher:
    """The matching parameters ResultsWriter(matcher=...) runs with: reference (a ReferenceSet or None: duplicates
    only), tol (Angstrom), ltol (relative, on the metric tensor), ops_mode (0 identity, 1 the 24 rotations, 2 all 48)."""

    def __init__(self, reference=None, tol=0.1, ltol=0.05, ops_mode=1):
        if not (tol > 0 and ltol > 0 and math.isfinite(tol) and math.isfinite(ltol)):
            raise ValueError("Matcher: tol and ltol must be finite and > 0")
        if ops_mode not in (0, 1, 2):
            raise ValueError("Matcher: ops_mode must be 0, 1 or 2")
        self.reference, self.tol, self.ltol, self.ops_mode = reference, float(tol), float(ltol), int(ops_mode)

    def __call__(self, results):
        return match(results, self.reference, self.tol, self.ltol, self.ops_mode)


# ---------------------------------------------------------------- symmetry (ics_op_structure_symmetry)
SYM_MAX_OPS = 4096      # the largest max_ops the op accepts
SYM_LAT_CAP = 64        # admissible lattice operations per structure
SYM_NOT_ELIGIBLE, SYM_LATTICE_OVERFLOW, SYM_OPS_OVERFLOW, SYM_NOT_CLOSED = 1, 2, 4, 8     # the op's reason bits
SYM_REASONS = {SYM_NOT_ELIGIBLE: "not eligible", SYM_LATTICE_OVERFLOW: "more than 64 lattice operations",
               SYM_OPS_OVERFLOW: "more operations than max_ops", SYM_NOT_CLOSED: "operations not closed"}
TYPE_ORDER = (-6, -4, -3, -2, -1, 1, 2, 3, 4, 6)      # the columns of the op's `types` histogram


def _pg(rows):
    return {tuple(int(c) for c in hist): (sym, system) for system, pairs in rows for sym, hist in pairs}


# The 32 crystallographic point groups by their histogram of rotation types (TYPE_ORDER) -> (Hermann-Mauguin symbol,
# crystal system).  The histograms are distinct; tests/test_structure_symmetry_host.py re-derives them by enumerating the
# subgroups of the cubic and hexagonal holohedries.
POINT_GROUPS = _pg((
    ("triclinic", (("1", "0000010000"), ("-1", "0000110000"))),
    ("monoclinic", (("2", "0000011000"), ("m", "0001010000"), ("2/m", "0001111000"))),
    ("orthorhombic", (("222", "0000013000"), ("mm2", "0002011000"), ("mmm", "0003113000"))),
    ("tetragonal", (("4", "0000011020"), ("-4", "0200011000"), ("4/m", "0201111020"), ("422", "0000015020"),
                    ("4mm", "0004011020"), ("-42m", "0202013000"), ("4/mmm", "0205115020"))),
    ("trigonal", (("3", "0000010200"), ("-3", "0020110200"), ("32", "0000013200"), ("3m", "0003010200"),
                  ("-3m", "0023113200"))),
    ("hexagonal", (("6", "0000011202"), ("-6", "2001010200"), ("6/m", "2021111202"), ("622", "0000017202"),
                   ("6mm", "0006011202"), ("-6m2", "2004013200"), ("6/mmm", "2027117202"))),
    ("cubic", (("23", "0000013800"), ("m-3", "0083113800"), ("432", "0000019860"), ("-43m", "0606013800"),
               ("m-3m", "0689119860"))),
))


def lattice_op(code):
    """The integer matrix W (3, 3) of a lattice-operation code: code = sum_k (W[k // 3][k % 3] + 1) 3^(8 - k); f' = W f + t."""
    code = int(code)
    if not 0 <= code < 3 ** 9:
        raise ValueError("lattice_op: code outside 0..19682")
    return np.array([(code // 3 ** (8 - k)) % 3 - 1 for k in range(9)], np.int64).reshape(3, 3)


IDENTITY_CODE = 16484
assert np.array_equal(lattice_op(IDENTITY_CODE), np.eye(3, dtype=np.int64))


def symmetry_reason_text(bits):
    return ", ".join(t for bit, t in SYM_REASONS.items() if bits & bit)


def symmetry_packed(offsets, species, frac, lattice, eligible, tol=0.1, ltol=0.05, max_ops=192):
    """ics_op_structure_symmetry on packed arrays: offsets (ns + 1,), species (N,), frac (N, 3), lattice (ns, 3, 3) with
    rows va, vb, vc, eligible (ns,).  Returns the op's outputs as a dict of arrays: n_lat, n_ops, n_point, n_trans,
    reason (ns,), types (ns, 10), op_code, op_anchor, op_rms (ns, max_ops), op_t (ns, max_ops, 3), orbit, mult (N,),
    sym_frac (N, 3), sym_G (ns, 9), sym_shift, sym_resid (ns,)."""
    offsets = np.ascontiguousarray(offsets, np.int32)
    species = np.ascontiguousarray(species, np.int32).reshape(-1)
    frac = np.ascontiguousarray(frac, np.float64).reshape(-1, 3)
    lattice = np.ascontiguousarray(lattice, np.float64).reshape(-1, 9)
    eligible = np.ascontiguousarray(eligible, np.int32).reshape(-1)
    ns, N, max_ops = len(offsets) - 1, len(species), int(max_ops)
    if ns < 1:
        raise ValueError("symmetry needs at least one structure")
    if len(lattice) != ns or len(eligible) != ns or len(frac) != N or int(offsets[-1]) != N:
        raise ValueError("symmetry: array lengths do not agree (structures %d / %d / %d, atoms %d / %d / %d)"
                         % (ns, len(lattice), len(eligible), N, len(frac), int(offsets[-1])))
    if not 1 <= max_ops <= SYM_MAX_OPS:
        raise ValueError("symmetry: max_ops must be in 1..%d" % SYM_MAX_OPS)
    A = max(N, 1)
    out = {"n_lat": np.zeros(ns, np.int32), "n_ops": np.zeros(ns, np.int32), "n_point": np.zeros(ns, np.int32),
           "n_trans": np.zeros(ns, np.int32), "types": np.zeros((ns, 10), np.int32), "reason": np.zeros(ns, np.int32),
           "op_code": np.full((ns, max_ops), -1, np.int32), "op_anchor": np.full((ns, max_ops), -1, np.int32),
           "op_t": np.full((ns, max_ops, 3), np.nan), "op_rms": np.full((ns, max_ops), np.nan),
           "orbit": np.zeros(A, np.int32), "mult": np.zeros(A, np.int32), "sym_frac": np.zeros((A, 3)),
           "sym_G": np.zeros((ns, 9)), "sym_shift": np.zeros(ns), "sym_resid": np.zeros(ns)}
    L.check(L.load().ics_op_structure_symmetry(
        L.i32ptr(offsets), L.i32ptr(species), L.f64ptr(frac), L.f64ptr(lattice), L.i32ptr(eligible), ns, float(tol),
        float(ltol), max_ops, L.i32ptr(out["n_lat"]), L.i32ptr(out["n_ops"]), L.i32ptr(out["n_point"]),
        L.i32ptr(out["n_trans"]), L.i32ptr(out["types"]), L.i32ptr(out["reason"]), L.i32ptr(out["op_code"]),
        L.i32ptr(out["op_anchor"]), L.f64ptr(out["op_t"]), L.f64ptr(out["op_rms"]), L.i32ptr(out["orbit"]),
        L.i32ptr(out["mult"]), L.f64ptr(out["sym_frac"]), L.f64ptr(out["sym_G"]), L.f64ptr(out["sym_shift"]),
        L.f64ptr(out["sym_resid"])))
    out["orbit"], out["mult"], out["sym_frac"] = out["orbit"][:N], out["mult"][:N], out["sym_frac"][:N]
    return out


def metric_parameters(G):
    """(abc (3,), angles (3,) in degrees) of a metric tensor G (9,) or (3, 3)."""
    G = np.asarray(G, np.float64).reshape(3, 3)
    abc = np.sqrt(np.diag(G))
    cs = np.array([G[1, 2] / (abc[1] * abc[2]), G[0, 2] / (abc[0] * abc[2]), G[0, 1] / (abc[0] * abc[1])])
    return abc, np.degrees(np.arccos(np.clip(cs, -1.0, 1.0)))


def symmetry(results, tol=0.1, ltol=0.05, max_ops=192, retries=3, shrink=0.7, packed=None):
    """The symmetry of every entry of `results` (the dicts screen returns, None = a failed sample).  One device call for
    all structures; those that come back not closed (bit 8: a noisy structure near tol can pass some operations and miss
    their products) are called again at tol * shrink, up to `retries` times, each round in one call over the remaining
    subset -- at a small enough tol only the identity passes, and that is closed.  Eligibility is `eligibility(results,
    tol)`, as for match.  packed: the callable that evaluates a packed table (symmetry_packed: the device op).
    Returns one dict per sample: point_group and crystal_system (None when the histogram is in no row of POINT_GROUPS,
    which only a result that is not closed can give, or when the sample was not analysed), n_ops, n_centring, n_lattice,
    types, tol_used, sym_reason (the op's reason bits; 0 = symmetrised), ops [(W (3, 3) int, t (3,))], species, orbit, mult,
    sym_frac, sym_abc, sym_angles, sym_shift, sym_resid."""
    packed = symmetry_packed if packed is None else packed
    if not (tol > 0 and ltol > 0 and math.isfinite(tol) and math.isfinite(ltol) and 0 < shrink < 1 and retries >= 0):
        raise ValueError("symmetry: tol and ltol must be finite and > 0, shrink in (0, 1), retries >= 0")
    ns = len(results)
    bits = eligibility(results, tol)
    out = [None] * ns
    for k, r in enumerate(results):
        n = 0 if r is None else len(r["species"])
        out[k] = {"point_group": None, "crystal_system": None, "n_ops": 0, "n_centring": 0, "n_lattice": 0,
                  "types": (0,) * 10, "tol_used": None, "sym_reason": SYM_NOT_ELIGIBLE, "ops": [],
                  "species": None if r is None else np.asarray(r["species"], np.int32).copy(),
                  "orbit": np.arange(n, dtype=np.int32), "mult": np.ones(n, np.int32),
                  "sym_frac": None if r is None else np.asarray(r["frac"], np.float64).reshape(-1, 3).copy(),
                  "sym_abc": None if r is None else np.asarray(r["abc"], np.float64).copy(),
                  "sym_angles": None if r is None else np.asarray(r["angles"], np.float64).copy(), "sym_shift": 0.0,
                  "sym_resid": 0.0, "eligibility": int(bits[k])}
    todo = [k for k in range(ns) if bits[k] == 0]
    t = float(tol)
    for attempt in range(int(retries) + 1):
        if not todo:
            break
        sp_l = [np.asarray(results[k]["species"], np.int32) for k in todo]
        off = np.zeros(len(todo) + 1, np.int32)
        off[1:] = np.cumsum([len(s) for s in sp_l])
        o = packed(off, np.concatenate(sp_l), np.concatenate([np.asarray(results[k]["frac"], np.float64).reshape(-1, 3)
                                                              for k in todo]),
                   np.array([results[k]["lattice"] for k in todo], np.float64), np.ones(len(todo), np.int32), t, ltol,
                   max_ops)
        again = []
        for i, k in enumerate(todo):
            a0, a1, d = int(off[i]), int(off[i + 1]), out[k]
            types = tuple(int(v) for v in o["types"][i])
            pg = POINT_GROUPS.get(types)
            keep = min(int(o["n_ops"][i]), int(max_ops))
            abc, ang = metric_parameters(o["sym_G"][i])
            d.update(point_group=pg[0] if pg else None, crystal_system=pg[1] if pg else None, n_ops=int(o["n_ops"][i]),
                     n_centring=int(o["n_trans"][i]), n_lattice=int(o["n_lat"][i]), types=types, tol_used=t,
                     sym_reason=int(o["reason"][i]),
                     ops=[(lattice_op(o["op_code"][i, g]), o["op_t"][i, g].copy()) for g in range(keep)],
                     orbit=o["orbit"][a0:a1].copy(), mult=o["mult"][a0:a1].copy(), sym_frac=o["sym_frac"][a0:a1].copy(),
                     sym_abc=abc, sym_angles=ang, sym_shift=float(o["sym_shift"][i]), sym_resid=float(o["sym_resid"][i]))
            if int(o["reason"][i]) & SYM_NOT_CLOSED:
                again.append(k)
        todo, t = again, t * float(shrink)
    return out


class Symmetriser:
    """The symmetry parameters ResultsWriter(symmetriser=...) runs with: tol (Angstrom), ltol (relative, on the metric
    tensor), max_ops (operations kept per structure), retries and shrink (the rounds at a smaller tol for structures
    whose operations are not closed)."""

    def __init__(self, tol=0.1, ltol=0.05, max_ops=192, retries=3, shrink=0.7, packed=None):
        if not (tol > 0 and ltol > 0 and math.isfinite(tol) and math.isfinite(ltol)):
            raise ValueError("Symmetriser: tol and ltol must be finite and > 0")
        if not 1 <= int(max_ops) <= SYM_MAX_OPS:
            raise ValueError("Symmetriser: max_ops must be in 1..%d" % SYM_MAX_OPS)
        if not (0 < shrink < 1 and retries >= 0):
            raise ValueError("Symmetriser: shrink must be in (0, 1) and retries >= 0")
        self.tol, self.ltol, self.max_ops = float(tol), float(ltol), int(max_ops)
        self.retries, self.shrink, self.packed = int(retries), float(shrink), packed

    def __call__(self, results):
        return symmetry(results, self.tol, self.ltol, self.max_ops, self.retries, self.shrink, self.packed)

# ---------------------------------------------------------------- fingerprints (ics_op_structure_fingerprint / _nearest)
FP_MAX_BINS = 256       # the largest n_bins the op accepts
FP_NOT_ELIGIBLE, FP_IMAGE_RANGE = 1, 2      # the op's reason bits
FP_REASONS = {FP_NOT_ELIGIBLE: "not eligible", FP_IMAGE_RANGE: "image range above 32"}
FP_QUANTILES = (0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0)


def fingerprint_reason_text(bits):
    return ", ".join(t for bit, t in FP_REASONS.items() if bits & bit)


def _fp_params(r_max, n_bins, width, cn_tol):
    r_max, n_bins, width, cn_tol = float(r_max), int(n_bins), float(width), float(cn_tol)
    if not (math.isfinite(r_max) and r_max > 0 and math.isfinite(width) and width > 0 and math.isfinite(cn_tol)
            and cn_tol >= 0 and 1 <= n_bins <= FP_MAX_BINS):
        raise ValueError("fingerprint: r_max and width must be finite and > 0, cn_tol finite and >= 0, n_bins in 1..%d"
                         % FP_MAX_BINS)
    return r_max, n_bins, width, cn_tol


def fingerprint_packed(offsets, species, frac, lattice, eligible, r_max=6.0, n_bins=60, width=0.1, cn_tol=0.1):
    """ics_op_structure_fingerprint on packed arrays: offsets (ns + 1,), species (N,), frac (N, 3), lattice (ns, 3, 3) with
    rows va, vb, vc, eligible (ns,).  Returns the op's outputs as a dict of arrays: rdf (ns, 2, n_bins) = (g, gZ), count
    (ns, n_bins), n_pairs (ns,) int64, nn_dist (N,), cn (N,) int32, reason (ns,)."""
    offsets = np.ascontiguousarray(offsets, np.int32)
    species = np.ascontiguousarray(species, np.int32).reshape(-1)
    frac = np.ascontiguousarray(frac, np.float64).reshape(-1, 3)
    lattice = np.ascontiguousarray(lattice, np.float64).reshape(-1, 9)
    eligible = np.ascontiguousarray(eligible, np.int32).reshape(-1)
    r_max, n_bins, width, cn_tol = _fp_params(r_max, n_bins, width, cn_tol)
    ns, N = len(offsets) - 1, len(species)
    if ns < 1:
        raise ValueError("fingerprint needs at least one structure")
    if len(lattice) != ns or len(eligible) != ns or len(frac) != N or int(offsets[-1]) != N:
        raise ValueError("fingerprint: array lengths do not agree (structures %d / %d / %d, atoms %d / %d / %d)"
                         % (ns, len(lattice), len(eligible), N, len(frac), int(offsets[-1])))
    A = max(N, 1)
    out = {"rdf": np.zeros((ns, 2, n_bins)), "count": np.zeros((ns, n_bins)), "n_pairs": np.zeros(ns, np.int64),
           "nn_dist": np.zeros(A), "cn": np.zeros(A, np.int32), "reason": np.zeros(ns, np.int32)}
    L.check(L.load().ics_op_structure_fingerprint(
        L.i32ptr(offsets), L.i32ptr(species), L.f64ptr(frac), L.f64ptr(lattice), L.i32ptr(eligible), ns, r_max, n_bins,
        width, cn_tol, L.f64ptr(out["rdf"]), L.f64ptr(out["count"]), L.i64ptr(out["n_pairs"]), L.f64ptr(out["nn_dist"]),
        L.i32ptr(out["cn"]), L.i32ptr(out["reason"])))
    out["nn_dist"], out["cn"] = out["nn_dist"][:N], out["cn"][:N]
    return out


def fingerprint_nearest(fp, valid, nq, nref):
    """ics_op_fingerprint_nearest: fp (nq + nref, len) float64, queries first; valid (nq + nref,).  Returns q_ref, q_ref_d,
    q_q, q_q_d (nq,), ref_q, ref_q_d (nref,), div_sum, div_pairs."""
    fp = np.ascontiguousarray(fp, np.float64)
    valid = np.ascontiguousarray(valid, np.int32).reshape(-1)
    nq, nref = int(nq), int(nref)
    if fp.ndim != 2 or nq < 1 or nref < 0 or fp.shape[0] != nq + nref or len(valid) != nq + nref or fp.shape[1] < 1:
        raise ValueError("fingerprint_nearest: fp must be (nq + nref, len >= 1) with nq >= 1, nref >= 0 and one valid flag "
                         "per row (fp %s, valid %d, nq %d, nref %d)" % (fp.shape, len(valid), nq, nref))
    m = max(nref, 1)
    out = {"q_ref": np.full(nq, -1, np.int32), "q_ref_d": np.full(nq, np.inf), "ref_q": np.full(m, -1, np.int32),
           "ref_q_d": np.full(m, np.inf), "q_q": np.full(nq, -1, np.int32), "q_q_d": np.full(nq, np.inf)}
    div_sum, div_pairs = np.zeros(1), np.zeros(1, np.int64)
    L.check(L.load().ics_op_fingerprint_nearest(
        L.f64ptr(fp), L.i32ptr(valid), fp.shape[1], nq, nref, L.i32ptr(out["q_ref"]), L.f64ptr(out["q_ref_d"]),
        L.i32ptr(out["ref_q"]), L.f64ptr(out["ref_q_d"]), L.i32ptr(out["q_q"]), L.f64ptr(out["q_q_d"]), L.f64ptr(div_sum),
        L.i64ptr(div_pairs)))
    out["ref_q"], out["ref_q_d"] = out["ref_q"][:nref], out["ref_q_d"][:nref]
    out["div_sum"], out["div_pairs"] = float(div_sum[0]), int(div_pairs[0])
    return out


def fingerprint(results, r_max=6.0, n_bins=60, width=0.1, cn_tol=0.1):
    """The fingerprint of every entry of `results` (the dicts screen returns, None = a failed sample) in one device call.
    Eligible: not None, valid, 1..256 atoms, a finite lattice.  Returns one dict per entry: fp (the concatenation g || gZ,
    length 2 n_bins, or None where fp_reason != 0), rdf (2, n_bins) or None, cn (n,) int32 and nn_dist (n,) or None,
    fp_reason (the op's reason bits)."""
    r_max, n_bins, width, cn_tol = _fp_params(r_max, n_bins, width, cn_tol)
    ns = len(results)
    out = [{"fp": None, "rdf": None, "cn": None, "nn_dist": None, "fp_reason": FP_NOT_ELIGIBLE} for _ in range(ns)]
    ok = [r is not None and bool(r["valid"]) and 1 <= len(r["species"]) <= MATCH_MAX_ATOMS
          and bool(np.all(np.isfinite(r["lattice"]))) for r in results]
    if not any(ok):
        return out
    sp_l = [np.asarray(r["species"], np.int32) if e else np.zeros(0, np.int32) for r, e in zip(results, ok)]
    fr_l = [np.asarray(r["frac"], np.float64).reshape(-1, 3) if e else np.zeros((0, 3)) for r, e in zip(results, ok)]
    lat = np.zeros((ns, 3, 3))
    for k, r in enumerate(results):
        if ok[k]:
            lat[k] = r["lattice"]
    off = np.zeros(ns + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in sp_l])
    o = fingerprint_packed(off, np.concatenate(sp_l), np.concatenate(fr_l), lat, np.array(ok, np.int32), r_max, n_bins,
                           width, cn_tol)
    for k in range(ns):
        d, a0, a1 = out[k], int(off[k]), int(off[k + 1])
        d["fp_reason"] = int(o["reason"][k])
        if d["fp_reason"] == 0:
            d["rdf"] = o["rdf"][k].copy()
            d["fp"] = d["rdf"].reshape(-1).copy()
            d["cn"], d["nn_dist"] = o["cn"][a0:a1].copy(), o["nn_dist"][a0:a1].copy()
    return out


class Fingerprinter:
    """The fingerprint parameters ResultsWriter(fingerprinter=...) runs with: reference (a ReferenceSet or None:
    sample-to-sample only), r_max, n_bins, width, cn_tol, and deltas, the distances coverage is reported at (none by
    default: the scale of these distances on real data has not been measured).  A call fingerprints the samples and, once
    and kept on the ReferenceSet, reference.screened(); then one fingerprint_nearest over both."""

    def __init__(self, reference=None, r_max=6.0, n_bins=60, width=0.1, cn_tol=0.1, deltas=()):
        self.r_max, self.n_bins, self.width, self.cn_tol = _fp_params(r_max, n_bins, width, cn_tol)
        self.deltas = tuple(float(d) for d in deltas)
        if not all(math.isfinite(d) and d >= 0 for d in self.deltas):
            raise ValueError("Fingerprinter: deltas must be finite and >= 0")
        self.reference = reference

    @property
    def params(self):
        return {"r_max": self.r_max, "n_bins": self.n_bins, "width": self.width, "cn_tol": self.cn_tol}

    def reference_fingerprints(self):
        """The fingerprints of the reference set (computed once per parameter set, kept on the ReferenceSet)."""
        if self.reference is None or not len(self.reference):
            return []
        cache, key = self.reference._fingerprints, (self.r_max, self.n_bins, self.width, self.cn_tol)
        if key not in cache:
            cache[key] = fingerprint(self.reference.screened(), *key)
        return cache[key]

    def __call__(self, results):
        """{"samples": fingerprint()'s list, "references": the same for the reference set, "nearest": fingerprint_nearest's
        dict over (samples, references) or None when there is no sample at all}."""
        samples = fingerprint(results, self.r_max, self.n_bins, self.width, self.cn_tol)
        refs = self.reference_fingerprints()
        near = None
        if samples:
            both = samples + list(refs)
            valid = np.array([d["fp"] is not None for d in both], np.int32)
            fp = np.zeros((len(both), 2 * self.n_bins))
            for k, d in enumerate(both):
                if d["fp"] is not None:
                    fp[k] = d["fp"]
            near = fingerprint_nearest(fp, valid, len(samples), len(refs))
        return {"samples": samples, "references": refs, "nearest": near}


def reason_text(reason):
    return ", ".join(t for bit, t in REASONS.items() if reason & bit) or "valid"


# ---------------------------------------------------------------- CIF
def write_cif(path, abc, angles, species, frac, volume=None):
    """A P1 CIF 1.1 file of one structure: cell lengths (Angstrom) and angles (degrees), atomic numbers, fractional
    coordinates (written as they are, 8 decimals)."""
    species = np.asarray(species, np.int64).reshape(-1)
    frac = np.asarray(frac, np.float64).reshape(len(species), 3)
    hist = np.bincount(species, minlength=HIST)
    if len(hist) > HIST or (len(species) and species.min() < 1):
        raise ValueError("write_cif: species outside 1..94")
    if volume is None:
        ca, cb, cg = (0.0 if t == 90 else math.cos(math.radians(t)) for t in angles)
        volume = abc[0] * abc[1] * abc[2] * math.sqrt(max(0.0, 1 - ca * ca - cb * cb - cg * cg + 2 * ca * cb * cg))
    f = formula(hist)
    lines = ["data_" + reduced_formula(hist), "_symmetry_space_group_name_H-M   'P 1'"]
    lines += ["_cell_length_%s   %.8f" % (n, v) for n, v in zip("abc", abc)]
    lines += ["_cell_angle_%s   %.8f" % (n, v) for n, v in zip(("alpha", "beta", "gamma"), angles)]
    lines += ["_symmetry_Int_Tables_number   1", "_chemical_formula_structural   " + reduced_formula(hist),
              "_chemical_formula_sum   '%s'" % f, "_cell_volume   %.8f" % volume, "_cell_formula_units_Z   %d"
              % (reduce(math.gcd, [int(n) for n in hist if n]) if len(species) else 0),
              "loop_", " _symmetry_equiv_pos_site_id", " _symmetry_equiv_pos_as_xyz", "  1  'x, y, z'",
              "loop_", " _atom_site_type_symbol", " _atom_site_label", " _atom_site_symmetry_multiplicity",
              " _atom_site_fract_x", " _atom_site_fract_y", " _atom_site_fract_z", " _atom_site_occupancy"]
    for k, (z, p) in enumerate(zip(species, frac)):
        lines.append("  %s  %s%d  1  %.8f  %.8f  %.8f  1" % (SYMBOLS[z], SYMBOLS[z], k, p[0], p[1], p[2]))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def read_cif(path):
    """The subset write_cif writes: dict(name, abc (3,), angles (3,), volume, formula_sum, species (n,) atomic numbers,
    labels [n], frac (n, 3))."""
    tags, loops, cols, rows = {}, [], None, None
    for raw in open(path):
        ln = raw.strip()
        if not ln or ln.startswith("#"):
            continue
        if ln.startswith("data_"):
            tags["name"] = ln[5:]
        elif ln == "loop_":
            cols, rows = [], []
            loops.append((cols, rows))
        elif ln.startswith("_"):
            if cols is not None and not rows:
                if len(ln.split()) == 1:
                    cols.append(ln)
                    continue
            cols = None
            k, _, v = ln.partition(" ")
            tags[k] = v.strip().strip("'")
        elif cols is not None:
            rows.append(ln)
    site = [(c, r) for c, r in loops if "_atom_site_fract_x" in c]
    if not site:
        raise ValueError("%s: no atom-site loop" % path)
    c, r = site[0]
    rec = [x.split() for x in r]
    sym = [x[c.index("_atom_site_type_symbol")] for x in rec]
    return {"name": tags.get("name", ""),
            "abc": np.array([float(tags["_cell_length_" + n]) for n in "abc"]),
            "angles": np.array([float(tags["_cell_angle_" + n]) for n in ("alpha", "beta", "gamma")]),
            "volume": float(tags["_cell_volume"]), "formula_sum": tags.get("_chemical_formula_sum", ""),
            "species": np.array([SYMBOLS.index(s) for s in sym], np.int32),
            "labels": [x[c.index("_atom_site_label")] for x in rec],
            "frac": np.array([[float(x[c.index("_atom_site_fract_" + a)]) for a in "xyz"] for x in rec],
                             np.float64).reshape(len(rec), 3)}


def _xyz_row(W, t):
    """One row of a _symmetry_equiv_pos_as_xyz loop: '-y+0.25000000, x, z+0.50000000'."""
    parts = []
    for r in range(3):
        term = ""
        for c, name in enumerate("xyz"):
            w = int(W[r][c])
            if w:
                term += ("-" if w < 0 else ("+" if term else "")) + (name if abs(w) == 1 else "%d%s" % (abs(w), name))
        v = float(t[r]) - math.floor(float(t[r]))
        text = "%.8f" % v
        if text.startswith("1."):
            text = "0.00000000"
        if text != "0.00000000" or not term:
            term += ("+" if term else "") + text
        parts.append(term)
    return ", ".join(parts)


def _parse_xyz_row(text):
    """The inverse of _xyz_row: (W (3, 3) int, t (3,))."""
    import re
    W, t = np.zeros((3, 3), np.int64), np.zeros(3)
    parts = text.split(",")
    if len(parts) != 3:
        raise ValueError("not a symmetry operation: %r" % text)
    for r, part in enumerate(parts):
        part = part.replace(" ", "")
        pos = 0
        for m in re.finditer(r"([+-]?)(\d*)([xyz])|([+-]?)(\d+\.\d*|\d+/\d+|\d+)", part):
            if m.start() != pos:
                raise ValueError("not a symmetry operation: %r" % text)
            pos = m.end()
            if m.group(3):
                W[r, "xyz".index(m.group(3))] += (-1 if m.group(1) == "-" else 1) * int(m.group(2) or 1)
            else:
                num = m.group(5)
                v = float(num.split("/")[0]) / float(num.split("/")[1]) if "/" in num else float(num)
                t[r] += -v if m.group(4) == "-" else v
        if pos != len(part) or not part:
            raise ValueError("not a symmetry operation: %r" % text)
    return W, t


def write_cif_symmetry(path, result, species=None):
    """The symmetrised structure of one entry of symmetry()'s list (sym_reason 0; species: its atomic numbers, or others):
    the symmetrised cell, the crystal system and point group, every operation as one row of the
    _symmetry_equiv_pos_as_xyz loop (W and the fitted translation, 8 decimals), and the atom-site loop over the orbit
    representatives only, with their multiplicities.  No space-group name is written: none is determined."""
    if result["sym_reason"] != 0 or not result["ops"]:
        raise ValueError("write_cif_symmetry: the structure was not symmetrised (%s)"
                         % symmetry_reason_text(result["sym_reason"]))
    species = np.asarray(result["species"] if species is None else species, np.int64).reshape(-1)
    frac = np.asarray(result["sym_frac"], np.float64).reshape(len(species), 3)
    orbit, mult = np.asarray(result["orbit"]), np.asarray(result["mult"])
    hist = np.bincount(species, minlength=HIST)
    if len(hist) > HIST or species.min() < 1:
        raise ValueError("write_cif_symmetry: species outside 1..94")
    abc, angles = result["sym_abc"], result["sym_angles"]
    ca, cb, cg = (math.cos(math.radians(t)) for t in angles)
    volume = abc[0] * abc[1] * abc[2] * math.sqrt(max(0.0, 1 - ca * ca - cb * cb - cg * cg + 2 * ca * cb * cg))
    lines = ["data_" + reduced_formula(hist), "_symmetry_space_group_name_H-M   ?",
             "_space_group_crystal_system   %s" % (result["crystal_system"] or "?"),
             "_space_group_point_group_H-M   '%s'" % (result["point_group"] or "?")]
    lines += ["_cell_length_%s   %.8f" % (n, v) for n, v in zip("abc", abc)]
    lines += ["_cell_angle_%s   %.8f" % (n, v) for n, v in zip(("alpha", "beta", "gamma"), angles)]
    lines += ["_chemical_formula_structural   " + reduced_formula(hist), "_chemical_formula_sum   '%s'" % formula(hist),
              "_cell_volume   %.8f" % volume,
              "_cell_formula_units_Z   %d" % reduce(math.gcd, [int(n) for n in hist if n]),
              "loop_", " _symmetry_equiv_pos_site_id", " _symmetry_equiv_pos_as_xyz"]
    lines += ["  %d  '%s'" % (k + 1, _xyz_row(W, t)) for k, (W, t) in enumerate(result["ops"])]
    lines += ["loop_", " _atom_site_type_symbol", " _atom_site_label", " _atom_site_symmetry_multiplicity",
              " _atom_site_fract_x", " _atom_site_fract_y", " _atom_site_fract_z", " _atom_site_occupancy"]
    for k in range(len(species)):
        if orbit[k] == k:
            p, z = frac[k], species[k]
            lines.append("  %s  %s%d  %d  %.8f  %.8f  %.8f  1" % (SYMBOLS[z], SYMBOLS[z], k, mult[k], p[0], p[1], p[2]))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def read_cif_symmetry(path):
    """The file write_cif_symmetry writes: read_cif's dict for the asymmetric unit, plus crystal_system, point_group,
    ops [(W, t)] and mult (n,)."""
    d = read_cif(path)
    tags, rows, mult, state = {}, [], [], None
    for raw in open(path):
        ln = raw.strip()
        if ln == "loop_":
            state = "loop"
        elif ln.startswith("_space_group_"):
            k, _, v = ln.partition(" ")
            tags[k] = v.strip().strip("'")
        elif ln == "_symmetry_equiv_pos_as_xyz":
            state = "ops"
        elif ln == "_atom_site_occupancy":
            state = "sites"
        elif ln and not ln.startswith("_") and state == "ops":
            rows.append(ln.split(None, 1)[1].strip().strip("'"))
        elif ln and not ln.startswith("_") and state == "sites":
            mult.append(int(ln.split()[2]))
    d["crystal_system"], d["point_group"] = tags.get("_space_group_crystal_system"), tags.get("_space_group_point_group_H-M")
    d["ops"] = [_parse_xyz_row(r) for r in rows]
    d["mult"] = np.array(mult, np.int32)
    return d


def expand_symmetry(species, frac, ops, merge=1e-6):
    """The full cell of an asymmetric unit: every operation applied to every site, wrapped into [0, 1), images of a site
    within `merge` (fractional, periodic) of an earlier one dropped.  Returns (species (n,), frac (n, 3)), the sites of
    one representative together, in operation order."""
    species = np.asarray(species, np.int32).reshape(-1)
    frac = np.asarray(frac, np.float64).reshape(len(species), 3)
    out_z, out_f = [], []
    for z, p in zip(species, frac):
        mine = []
        for W, t in ops:
            q = np.asarray(W, np.float64) @ p + np.asarray(t, np.float64)
            q -= np.floor(q)
            if all(np.abs((q - m) - np.rint(q - m)).max() > merge for m in mine):
                mine.append(q)
        out_z += [int(z)] * len(mine)
        out_f += mine
    return np.array(out_z, np.int32), np.array(out_f, np.float64).reshape(len(out_z), 3)


# ---------------------------------------------------------------- generate.py:250-318
class ResultsWriter:
    """The tail of generate.py's sample loop.  add_batch screens one batch on the device and, per sample in order:
    builds the formula, numbers a formula seen before (formula_count), SKIPS an invalid structure, writes
    cifs/<formula_count>.cif, appends the row and its results.json record.  finish() writes results.csv sorted by id (the
    reference sorts by the CGCNN target, which is not predicted here) and returns the counts.
    With matcher= (a Matcher), finish() first matches ALL written samples in one device call -- a duplicate may lie in
    any earlier batch -- and every row carries MATCH_COLUMNS after COLUMNS: duplicate_of (the id of the first earlier
    row that is the same structure), duplicate_rms, training_match (the reference's id), training_rms, match_reason (""
    or why the sample was not compared); the counts gain unique (compared, no earlier duplicate), novel (unique and no
    training match) and ineligible, and match_summary holds them with the ineligible counts by reason.  results.json is
    written per batch and keeps today's records.  Without matcher= nothing changes.
    With symmetriser= (a Symmetriser), finish() then finds the symmetry of ALL written samples in one device call (plus
    the retry rounds) and every row carries SYMMETRY_COLUMNS after the others: point_group, crystal_system, n_symops,
    n_centring, sym_shift, sym_tol (the tol the result was found at), sym_reason ("" or why the sample has no symmetrised
    structure); cifs_sym/<id>.cif holds the symmetrised structure of every sample with an empty sym_reason, and
    symmetry_summary the counts by point group and crystal system and the number symmetrised.  Without symmetriser=
    every file, column and count is what it is without it.
    With fingerprinter= (a Fingerprinter), finish() then fingerprints ALL written samples and, once, the reference set,
    and finds every nearest partner in one device call; every row carries FINGERPRINT_COLUMNS after the others:
    nearest_training (the reference's id) and nearest_training_dist, nearest_generated (the id of the nearest other row)
    and nearest_generated_dist, cn_mean, cn_min, cn_max (the coordination numbers of its atoms), fp_reason ("" or why the
    sample has no fingerprint).  fingerprints.npz holds ids, fp, rdf, the atom offsets, cn, nn_dist and the parameters;
    fingerprint_summary the parameters, the numbers fingerprinted on both sides, diversity (the mean distance between two
    samples), the quantiles FP_QUANTILES of the three nearest-distance arrays and, for every delta of the fingerprinter,
    coverage_recall (the share of fingerprinted references with a sample within delta) and coverage_precision (the share of
    fingerprinted samples with a reference within delta).  Without fingerprinter= nothing changes."""
    COLUMNS = ("formula", "id", "training", "target", "anon_formula", "electronegativity", "cif", "sample", "natoms",
               "min_distance", "volume")
    MATCH_COLUMNS = ("duplicate_of", "duplicate_rms", "training_match", "training_rms", "match_reason")
    SYMMETRY_COLUMNS = ("point_group", "crystal_system", "n_symops", "n_centring", "sym_shift", "sym_tol", "sym_reason")
    FINGERPRINT_COLUMNS = ("nearest_training", "nearest_training_dist", "nearest_generated", "nearest_generated_dist",
                           "cn_mean", "cn_min", "cn_max", "fp_reason")

    def __init__(self, out_dir, alpha=90, beta=90, gamma=90, tol=0.5, training_names=(), target_value=None, matcher=None,
                 symmetriser=None, fingerprinter=None):
        self.fingerprinter, self.fingerprint_summary, self.fingerprint_results = fingerprinter, None, None
        self.matcher, self.structs, self.match_summary = matcher, [], None
        self.symmetriser, self.symmetry_summary, self.symmetry_results = symmetriser, None, None
        self.out_dir, self.angles, self.tol = out_dir, (alpha, beta, gamma), tol
        self.training_names, self.target_value = set(training_names), target_value
        self.formulae, self.rows = [], []
        self.counts = {"generated": 0, "failed": 0, "invalid": 0, "written": 0}
        self.invalid_reasons = {}
        os.makedirs(os.path.join(out_dir, "cifs"), exist_ok=True)
        open(os.path.join(out_dir, "results.json"), "w").close()      # the records of THIS run (appended per row below)

    def add_batch(self, ks, lattice_params, atoms):
        """ks: the sample indices; atoms[b] = (species, xyz in Angstrom), or None for a failed sample."""
        res = screen(lattice_params, atoms, *self.angles, tol=self.tol)
        for k, r in zip(ks, res):
            self.counts["generated"] += 1
            if r is None:
                self.counts["failed"] += 1
                continue
            if not r["valid"]:
                self.counts["invalid"] += 1
                self.invalid_reasons[int(k)] = reason_text(r["reason"])
                continue
            f = r["formula"]
            fid = numbered(f, self.formulae)
            path = os.path.join(self.out_dir, "cifs", fid + ".cif")
            write_cif(path, r["abc"], r["angles"], r["species"], r["frac"], r["volume"])
            rd = {"formula": f, "id": fid, "training": int(reduced_formula(r["hist"]) in self.training_names),
                  "target": self.target_value, "anon_formula": anonymized_formula(r["hist"]),
                  "electronegativity": average_electroneg(r["hist"]), "cif": path, "sample": int(k),
                  "natoms": int(len(r["species"])), "min_distance": r["min_dist"], "volume": r["volume"]}
            self.rows.append(rd)
            if self.matcher is not None or self.symmetriser is not None or self.fingerprinter is not None:
                self.structs.append(r)
            self.formulae.append(f)
            self.counts["written"] += 1
            with open(os.path.join(self.out_dir, "results.json"), "a+") as wf:      # generate.py:313-314
                json.dump(str(rd), wf)
        return res

    def _match_rows(self):
        """The matcher over all written samples: the extra columns into the rows, the summary into match_summary."""
        m = self.matcher(self.structs)
        by_reason = {}
        unique = novel = ineligible = 0
        for rd, d in zip(self.rows, m):
            rd["duplicate_of"] = self.rows[d["duplicate_of"]]["id"] if d["duplicate_of"] >= 0 else None
            rd["duplicate_rms"], rd["training_match"], rd["training_rms"] = d["duplicate_rms"], d["training_match"], d["training_rms"]
            rd["match_reason"] = ineligible_text(d["match_reason"]) if d["match_reason"] else None
            if d["match_reason"]:
                ineligible += 1
                for bit, text in INELIGIBLE.items():
                    if d["match_reason"] & bit:
                        by_reason[text] = by_reason.get(text, 0) + 1
            elif d["duplicate_of"] < 0:
                unique += 1
                novel += d["training_match"] is None
        self.match_summary = {"unique": unique, "novel": novel, "ineligible": ineligible, "ineligible_by_reason": by_reason}
        self.counts.update(unique=unique, novel=novel, ineligible=ineligible)

    def _symmetry_rows(self):
        """The symmetriser over all written samples: the extra columns into the rows, cifs_sym/, symmetry_summary."""
        res = self.symmetriser(self.structs)
        os.makedirs(os.path.join(self.out_dir, "cifs_sym"), exist_ok=True)
        by_group, by_system, done = {}, {}, 0
        for rd, r, d in zip(self.rows, self.structs, res):
            ok = d["sym_reason"] == 0
            rd["point_group"], rd["crystal_system"] = d["point_group"], d["crystal_system"]
            rd["n_symops"], rd["n_centring"] = int(d["n_ops"]), int(d["n_centring"])
            rd["sym_shift"], rd["sym_tol"] = (float(d["sym_shift"]), d["tol_used"]) if ok else (None, d["tol_used"])
            rd["sym_reason"] = None if ok else symmetry_reason_text(d["sym_reason"])
            if ok:
                done += 1
                by_group[d["point_group"]] = by_group.get(d["point_group"], 0) + 1
                by_system[d["crystal_system"]] = by_system.get(d["crystal_system"], 0) + 1
                write_cif_symmetry(os.path.join(self.out_dir, "cifs_sym", rd["id"] + ".cif"), d, r["species"])
        self.symmetry_results = res
        self.symmetry_summary = {"symmetrised": done, "by_point_group": by_group, "by_crystal_system": by_system}
        self.counts.update(symmetrised=done)

    def _fingerprint_rows(self):
        """The fingerprinter over all written samples: the extra columns into the rows, fingerprints.npz, the summary."""
        fpr = self.fingerprinter
        res = fpr(self.structs)
        samples, refs, near = res["samples"], res["references"], res["nearest"]
        nb = fpr.n_bins
        for k, (rd, d) in enumerate(zip(self.rows, samples)):
            ok = d["fp"] is not None
            t = int(near["q_ref"][k]) if ok else -1
            g = int(near["q_q"][k]) if ok else -1
            rd["nearest_training"] = fpr.reference.ids[t] if t >= 0 else None
            rd["nearest_training_dist"] = float(near["q_ref_d"][k]) if t >= 0 else None
            rd["nearest_generated"] = self.rows[g]["id"] if g >= 0 else None
            rd["nearest_generated_dist"] = float(near["q_q_d"][k]) if g >= 0 else None
            rd["cn_mean"] = float(np.mean(d["cn"])) if ok else None
            rd["cn_min"], rd["cn_max"] = (int(d["cn"].min()), int(d["cn"].max())) if ok else (None, None)
            rd["fp_reason"] = None if ok else fingerprint_reason_text(d["fp_reason"])
        n = len(samples)
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([len(r["species"]) for r in self.structs])
        fp, rdf = np.full((n, 2 * nb), np.nan), np.full((n, 2, nb), np.nan)
        cn, nnd = np.full(int(off[-1]), -1, np.int32), np.full(int(off[-1]), np.nan)
        for k, d in enumerate(samples):
            if d["fp"] is not None:
                fp[k], rdf[k], cn[off[k]:off[k + 1]], nnd[off[k]:off[k + 1]] = d["fp"], d["rdf"], d["cn"], d["nn_dist"]
        np.savez(os.path.join(self.out_dir, "fingerprints.npz"), ids=np.array([rd["id"] for rd in self.rows], dtype=str), fp=fp,
                 rdf=rdf, offsets=off, cn=cn, nn_dist=nnd, r_max=fpr.r_max, n_bins=nb, width=fpr.width, cn_tol=fpr.cn_tol)

        def quantiles(v):
            v = np.asarray(v, np.float64)
            v = v[np.isfinite(v)]
            return [float(x) for x in np.quantile(v, FP_QUANTILES)] if len(v) else None
        nq = sum(d["fp"] is not None for d in samples)
        nr = sum(d["fp"] is not None for d in refs)
        empty = np.zeros(0)
        q_ref_d, ref_q_d, q_q_d = (near[k] for k in ("q_ref_d", "ref_q_d", "q_q_d")) if near else (empty, empty, empty)
        summary = dict(fpr.params, samples=nq, references=nr, quantiles=list(FP_QUANTILES),
                       diversity=near["div_sum"] / near["div_pairs"] if near and near["div_pairs"] else None,
                       nearest_training_dist=quantiles(q_ref_d), nearest_sample_of_training_dist=quantiles(ref_q_d),
                       nearest_generated_dist=quantiles(q_q_d), coverage=[])
        for delta in fpr.deltas:
            summary["coverage"].append({
                "delta": delta,
                "coverage_recall": float(np.sum(np.asarray(ref_q_d) <= delta)) / nr if nr else None,
                "coverage_precision": float(np.sum(np.asarray(q_ref_d) <= delta)) / nq if nq and nr else None})
        self.fingerprint_results, self.fingerprint_summary = res, summary
        self.counts.update(fingerprinted=nq)

    def finish(self):
        columns = self.COLUMNS
        if self.matcher is not None:
            self._match_rows()
            columns = self.COLUMNS + self.MATCH_COLUMNS
        if self.symmetriser is not None:
            self._symmetry_rows()
            columns = columns + self.SYMMETRY_COLUMNS
        if self.fingerprinter is not None:
            self._fingerprint_rows()
            columns = columns + self.FINGERPRINT_COLUMNS
        order = sorted(range(len(self.rows)), key=lambda i: self.rows[i]["id"])
        with open(os.path.join(self.out_dir, "results.csv"), "w", newline="") as fh:
            w = csv.writer(fh)
            w.writerow(("",) + columns)                               # the index column DataFrame.to_csv writes
            for i in order:
                w.writerow([i] + ["" if self.rows[i][c] is None else repr(self.rows[i][c]) if isinstance(self.rows[i][c], float)
                                  else self.rows[i][c] for c in columns])
        return dict(self.counts)


def read_results_csv(path):
    """results.csv back as a list of dicts (numbers converted)."""
    out = []
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            row.pop("", None)
            for c in ("training", "sample", "natoms"):
                row[c] = int(row[c])
            for c in ("electronegativity", "min_distance", "volume"):
                row[c] = float(row[c])
            row["target"] = float(row["target"]) if row["target"] != "" else None
            out.append(row)
    return out
