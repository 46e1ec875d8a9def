#!/usr/bin/env python3
"""Structure fingerprints on one MI355X -> profiles/fingerprint_bench.json (or --out).

  op       ics_op_structure_fingerprint (icsg3d_amd.structures.fingerprint_packed: host packing, one upload per chunk, the
           sweep kernel, the downloads) at 5, 20, 64 and 256 atoms per structure (4 096, 4 096, 2 048 and 256 structures:
           random P1 motifs in triclinic cells of 12 cubic Angstrom per atom, each with its own shift), default
           parameters; structures/s and pairs/s (the op's n_pairs: triples within R) follow from the time of the call.
  nearest  ics_op_fingerprint_nearest at 5 000 queries x 20 000 references x 120 components: pairs/s counts the distinct
           pairs (nq nref + nq (nq - 1) / 2); the kernels evaluate 2 nq nref + nq^2 distances (D is symmetric bit for bit,
           so references x queries is a second pass instead of column minima) and that rate is recorded too.
  host     the first structures of each n, and 200 x 2 000 rows, through the numpy restatement
           tests/structure_fingerprint_ref.py, timed on the host and compared with the device first.
  writer   one 5 000-sample ResultsWriter run (50 batches of 100 hand-made samples): finish() without and with a
           fingerprinter over a 2 000-structure reference set.  Without one, finish() is the code path it was before.

One child process per leg, each under --leg_seconds; a leg that ends on a signal or its time limit stops the run.  Every
time is the host clock around calls that end in a device synchronise; median of --reps after one warm-up call.  These
are recorded numbers; no threshold is set on them and no ratio is promised.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from benchutil import timeit  # noqa: E402

OP_LEGS = {"op_n5": (5, 4096, 16), "op_n20": (20, 4096, 8), "op_n64": (64, 2048, 4), "op_n256": (256, 256, 1)}


def structures(C, n, count, seed):
    """`count` structures of n atoms: eight random motifs, each copy with its own shift and 0.05 Angstrom of noise."""
    rng = np.random.default_rng(seed)
    protos = [C.sized(rng, n) for _ in range(8)]
    out = []
    for k in range(count):
        Z, f, M = protos[k % 8]
        out.append((Z, f + rng.uniform(size=3) + rng.normal(0, 0.05, f.shape) @ np.linalg.inv(M), M))
    return out


def leg_op(a, leg):
    import structure_fingerprint_cases as C
    import structure_fingerprint_ref as FR
    from icsg3d_amd import structures as S
    n, count, hs = OP_LEGS[leg]
    count = min(count, a.structures)
    structs = structures(C, n, count, 1)
    off, sp, fr, lat = C.pack(structs)
    el = np.ones(count, np.int32)
    call = lambda: S.fingerprint_packed(off, sp, fr, lat, el)      # noqa: E731
    o = call()
    assert np.all(o["reason"] == 0)
    t = timeit(call, a.reps, 1)
    sec = t["median_ms"] / 1e3
    pairs = int(o["n_pairs"].sum())
    row = {"leg": leg, "n": n, "structures": count, "pairs": pairs, **t, "structures_per_s": count / sec, "pairs_per_s": pairs / sec,
           "image_range": FR.image_range(structs[0][2], FR.reach(structs[0][2], 6.0, 0.1, 0.1)).tolist()}
    t0 = time.perf_counter()
    r = [FR.fingerprint_one(*st, **C.PARAMS) for st in structs[:hs]]     # each structure once, without the margin check
    th = time.perf_counter() - t0
    assert o["n_pairs"][:hs].tolist() == [x["n_pairs"] for x in r] and np.array_equal(o["cn"][:off[hs]], np.concatenate([x["cn"] for x in r]))
    row["host"] = {"structures": hs, "numpy_seconds": th, "numpy_structures_per_s": hs / th,
                   "worst_count_gap": float(np.abs(o["count"][:hs] - np.array([x["count"] for x in r])).max())}
    return row


def leg_nearest(a, leg):
    import structure_fingerprint_cases as C
    import structure_fingerprint_ref as FR
    from icsg3d_amd import structures as S
    nq, nref, length = a.nq, a.nref, 120
    fp, valid = C.nearest_table(7, nq, nref, length)
    call = lambda: S.fingerprint_nearest(fp, valid, nq, nref)      # noqa: E731
    o = call()
    t = timeit(call, a.reps, 1)
    sec = t["median_ms"] / 1e3
    pairs, evals = nq * nref + nq * (nq - 1) // 2, 2 * nq * nref + nq * nq
    row = {"leg": leg, "nq": nq, "nref": nref, "len": length, **t, "pairs": pairs, "pairs_per_s": pairs / sec,
           "distance_evaluations": evals, "distance_evaluations_per_s": evals / sec,
           "component_operations_per_s": evals * length / sec, "diversity": o["div_sum"] / o["div_pairs"]}
    hq, hr = min(200, nq), min(2000, nref)
    sub = np.concatenate([fp[:hq], fp[nq:nq + hr]])
    t0 = time.perf_counter()
    r = FR.nearest_ref(sub, np.ones(hq + hr, np.int32), hq, hr)
    th = time.perf_counter() - t0
    d = S.fingerprint_nearest(sub, np.ones(hq + hr, np.int32), hq, hr)
    assert all(np.array_equal(d[k], r[k]) for k in ("q_ref", "ref_q", "q_q"))
    row["host"] = {"nq": hq, "nref": hr, "numpy_seconds": th, "numpy_pairs_per_s": (hq * hr + hq * (hq - 1) // 2) / th,
                   "worst_distance_gap": float(np.abs(d["q_ref_d"] / r["q_ref_d"] - 1).max())}
    return row


def leg_writer(a, leg):
    import structure_fingerprint_cases as C
    from icsg3d_amd import structures as S
    rng = np.random.default_rng(2)
    base = C.base_cases()
    protos = [base["perovskite"], base["rocksalt"], base["tetragonal"]]
    for k in range(20):                      # and P1 motifs of 5 - 12 atoms in orthorhombic cells
        protos.append(C.random_p1(rng, 5 + k % 8, C.lat([4.0 + 0.1 * (k % 7), 5.0 + 0.1 * (k % 5), 6.0 + 0.1 * (k % 3)]), dmin=1.0))

    def draw():
        Z, f, M = protos[rng.integers(len(protos))]
        abc = np.linalg.norm(M, axis=1)
        f = f + rng.uniform(size=3)
        f = f - np.floor(f)
        return Z, f + rng.normal(0, 0.01, f.shape) / abc, abc
    samples = [draw() for _ in range(a.samples)]
    fpr = None
    if leg == "writer_with":
        refs = [draw() for _ in range(a.references)]
        ref = S.ReferenceSet(["r%d" % k for k in range(len(refs))], [r[0] for r in refs], [r[1] for r in refs],
                             [np.r_[r[2], 90.0, 90.0, 90.0] for r in refs])
        fpr = S.Fingerprinter(ref)
    tmp = tempfile.mkdtemp()
    try:
        w = S.ResultsWriter(tmp, fingerprinter=fpr) if fpr is not None else S.ResultsWriter(tmp)
        for b in range(0, a.samples, 100):
            part = samples[b:b + 100]
            w.add_batch(range(b, b + len(part)), np.array([p[2] for p in part]), [(p[0], p[1] * p[2]) for p in part])
        t0 = time.perf_counter()
        counts = w.finish()
        row = {"leg": leg, "samples": a.samples, "references": a.references if fpr else 0,
               "finish_seconds": time.perf_counter() - t0, "counts": counts}
        if fpr is not None:
            t0 = time.perf_counter()
            fpr(w.structs)
            row["fingerprinter_again_seconds"] = time.perf_counter() - t0          # the reference set is kept
            row["fingerprint_summary"] = w.fingerprint_summary
        return row
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fingerprint_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--structures", type=int, default=4096)
    ap.add_argument("--nq", type=int, default=5000)
    ap.add_argument("--nref", type=int, default=20000)
    ap.add_argument("--samples", type=int, default=5000)
    ap.add_argument("--references", type=int, default=2000)
    ap.add_argument("--leg_seconds", type=int, default=240)
    ap.add_argument("--legs", default="op_n5,op_n20,op_n64,op_n256,nearest,writer_without,writer_with")
    ap.add_argument("--leg", help="(internal) run one leg in this process and print its JSON row")
    a = ap.parse_args()
    if a.leg:
        row = leg_op(a, a.leg) if a.leg in OP_LEGS else (leg_nearest(a, a.leg) if a.leg == "nearest" else leg_writer(a, a.leg))
        print("ROW " + json.dumps(row), flush=True)
        return 0
    from icsg3d_amd import _lib
    name = (_lib.C.c_char * 256)()
    cus, mem = _lib.C.c_int(0), _lib.C.c_size_t(0)
    _lib.check(_lib.load().ics_device_info(name, _lib.C.byref(cus), _lib.C.byref(mem)))
    device = name.value.decode() or "(the runtime reports no device name)"
    out = {"device": device, "compute_units": cus.value, "hbm_bytes": mem.value, "library": _lib.load().ics_version().decode(),
           "r_max": 6.0, "n_bins": 60, "width": 0.1, "cn_tol": 0.1,
           "legs": []}
    for leg in a.legs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg] + [x for k in ("reps", "structures", "nq", "nref", "samples",
                                                                                  "references") for x in ("--" + k, str(getattr(a, k)))]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_seconds)
        except subprocess.TimeoutExpired:
            out["legs"].append({"leg": leg, "error": "time limit of %d s" % a.leg_seconds})
            print(leg, "ran into its time limit: stopping", flush=True)
            break
        rows = [ln[4:] for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
        if p.returncode != 0 or not rows:
            out["legs"].append({"leg": leg, "error": "exit %d" % p.returncode, "stderr": p.stderr[-1500:]})
            print(leg, "failed with exit", p.returncode, p.stderr[-1500:], flush=True)
            break                            # a failed leg: nothing more is started on the device
        out["legs"].append(json.loads(rows[-1]))
        print(rows[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
