#!/usr/bin/env python3
"""Structure symmetry on one MI355X -> profiles/symmetry_bench.json (or --out).

  op      ics_op_structure_symmetry (icsg3d_amd.structures.symmetry_packed: host packing, one upload, the lattice,
          operation, scan and group kernels, the downloads) on 4 096 structures of n = 5 atoms (cubic perovskite, 48
          operations), n = 8 (conventional rock salt, 192) and n = 40 (2x2x2 perovskite supercell, 384 operations,
          max_ops 384), each with its own origin shift and 0.2 tol of noise.  A combination is one (lattice operation,
          anchor): 48, 192 and 384 per structure; structures/s and combinations/s follow from the time of the call.
  host    the first --host_subset structures of each n through the numpy restatement tests/structure_symmetry_ref.py,
          integers compared with the device first.
  writer  one 5 000-sample ResultsWriter run (50 batches of 100 hand-made samples): finish() without and with a
          symmetriser.  Without one, finish() is the code path it was before the symmetriser existed.

One child process per leg, each under --leg_seconds; a leg that ends on a signal or its time limit stops the run.  Every
time is the host clock around calls that end in a device synchronise; median of --reps after one warm-up call.  These
are recorded numbers; no threshold is set on them.
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

OP_LEGS = {"op_n5": ("perovskite", None, 192, 48), "op_n8": ("rocksalt", None, 192, 192),
           "op_n40": ("perovskite", (2, 2, 2), 384, 384)}


def structures(C, name, reps, count, seed):
    rng = np.random.default_rng(seed)
    s = C.base_cases()[name]
    if reps:
        s = C.supercell(s, reps)
    return [C.noisy(rng, s, 0.2) for _ in range(count)]


def leg_op(a, leg):
    import structure_symmetry_cases as C
    import structure_symmetry_ref as MR
    from icsg3d_amd import structures as S
    name, reps, max_ops, nops = OP_LEGS[leg]
    structs = structures(C, name, reps, a.structures, 1)
    off, sp, fr, lat = C.pack(structs)
    el = np.ones(len(structs), np.int32)
    call = lambda: S.symmetry_packed(off, sp, fr, lat, el, C.TOL, C.LTOL, max_ops)      # noqa: E731
    o = call()
    assert np.all(o["n_ops"] == nops) and np.all(o["reason"] == 0), (np.unique(o["n_ops"]), np.unique(o["reason"]))
    t = timeit(call, a.reps, 1)
    sec = t["median_ms"] / 1e3
    combos = int((o["n_lat"].astype(np.int64) * (nops // 48)).sum())
    row = {"leg": leg, "n": len(structs[0][0]), "structures": len(structs), "max_ops": max_ops, "operations": nops,
           "combinations": combos, **t, "structures_per_s": len(structs) / sec, "combinations_per_s": combos / sec,
           "worst_sym_resid": float(o["sym_resid"].max()), "worst_sym_shift": float(o["sym_shift"].max())}
    hs = a.host_subset
    sub = structs[:hs]
    t0 = time.perf_counter()
    r = MR.symmetry_ref(sub, None, C.TOL, C.LTOL, max_ops)
    th = time.perf_counter() - t0
    off, sp, fr, lat = C.pack(sub)
    call = lambda: S.symmetry_packed(off, sp, fr, lat, el[:hs], C.TOL, C.LTOL, max_ops)  # noqa: E731
    o = call()
    for k in ("n_lat", "n_ops", "n_point", "n_trans", "types", "reason", "op_code", "op_anchor", "orbit", "mult"):
        assert np.array_equal(o[k], r[k]), k
    td = timeit(call, a.reps, 1)
    row["host"] = {"structures": hs, "numpy_seconds": th, "device_ms": td["median_ms"], "numpy_structures_per_s": hs / th,
                   "worst_sym_frac_gap": float(np.abs(o["sym_frac"] - r["sym_frac"]).max())}
    return row


def leg_writer(a, leg):
    import structure_symmetry_cases as C
    from icsg3d_amd import structures as S
    rng = np.random.default_rng(2)
    base = C.base_cases()
    protos = [base["perovskite"], base["rocksalt"], base["tetragonal"]]
    for k in range(20):                      # and P1 motifs of 5 - 12 atoms in orthorhombic cells
        protos.append(C.random_p1(rng, 5 + k % 8, C.lat([4.0 + 0.1 * (k % 7), 5.0 + 0.1 * (k % 5), 6.0 + 0.1 * (k % 3)]), dmin=1.0))
    samples = []
    for _ in range(a.samples):
        Z, f, M = protos[rng.integers(len(protos))]
        abc = np.linalg.norm(M, axis=1)
        f = f + rng.uniform(size=3)
        f = f - np.floor(f)
        samples.append((abc, (Z, f * abc + rng.normal(0, 0.01, f.shape))))
    sym = S.Symmetriser(C.TOL, C.LTOL, 192) if leg == "writer_with" else None
    tmp = tempfile.mkdtemp()
    try:
        w = S.ResultsWriter(tmp, symmetriser=sym) if sym is not None else S.ResultsWriter(tmp)
        for b in range(0, a.samples, 100):
            part = samples[b:b + 100]
            w.add_batch(range(b, b + len(part)), np.array([p[0] for p in part]), [p[1] for p in part])
        t0 = time.perf_counter()
        counts = w.finish()
        return {"leg": leg, "samples": a.samples, "finish_seconds": time.perf_counter() - t0, "counts": counts,
                "symmetry_summary": w.symmetry_summary}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "symmetry_bench.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--structures", type=int, default=4096)
    ap.add_argument("--host_subset", type=int, default=32)
    ap.add_argument("--samples", type=int, default=5000)
    ap.add_argument("--leg_seconds", type=int, default=240)
    ap.add_argument("--legs", default="op_n5,op_n8,op_n40,writer_without,writer_with")
    ap.add_argument("--leg", help="(internal) run one leg in this process and print its JSON row")
    a = ap.parse_args()
    if a.leg:
        row = leg_op(a, a.leg) if a.leg in OP_LEGS else leg_writer(a, a.leg)
        print("ROW " + json.dumps(row), flush=True)
        return 0
    import structure_symmetry_cases as C
    out = {"tol": C.TOL, "ltol": C.LTOL, "legs": []}
    for leg in a.legs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps", str(a.reps), "--structures", str(a.structures),
               "--host_subset", str(a.host_subset), "--samples", str(a.samples)]
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
            if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
                break                        # a signal: nothing more is started on the device
            continue
        out["legs"].append(json.loads(rows[-1]))
        print(rows[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
