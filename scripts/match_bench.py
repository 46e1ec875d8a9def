#!/usr/bin/env python3
"""Structure matching on one MI355X -> profiles/match_bench.json (or --out).

  op      ics_op_structure_match (icsg3d_amd.structures.match_packed: the host planner, one upload, the kernels, one
          download) on one composition bucket of 256 and of 4 096 structures with n = 5, 20 and 64 atoms, all queries:
          B (B - 1) / 2 pairs.  The cells are cubic (all 24 rotations admissible) and one species occurs once (one
          anchor), so a pair is 24 combinations; pairs/s and combinations/s follow from the time of the call.
  host    the same pairs through the numpy restatement tests/structure_match_ref.py on the first --host_bucket
          structures of each n (a subset small enough to finish), decisions compared with the device first.
  writer  one 5 000-sample ResultsWriter run (50 batches of 100 hand-made samples of 5 - 12 atoms, 60 prototypes):
          finish() without and with a matcher (200 references).

Every time is the host clock around calls that end in a device synchronise; median of --reps after one warm-up call.
These are recorded numbers; no threshold is set on them.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def bucket(C, MR, rng, n, size, edge):
    """`size` structures of one composition from 8 prototypes: random rotation, translation, order, noise 0.3 tol."""
    Z = [38] + [22] * ((n - 1) // 3) + [8] * (n - 1 - (n - 1) // 3)
    protos = [C.motif(rng, Z, C.lat([edge] * 3), dmin=1.0) for _ in range(8)]
    ops = MR.signed_permutations(1)
    return [C.derive(rng, protos[rng.randint(8)], ops[rng.randint(24)], C.noise_max(rng, n, 0.3 * C.TOL))[0]
            for _ in range(size)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_bench.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host_bucket", type=int, default=48)
    ap.add_argument("--samples", type=int, default=5000)
    a = ap.parse_args()
    import structure_match_cases as C
    import structure_match_ref as MR
    from icsg3d_amd import structures as S

    rng = np.random.RandomState(0)
    out = {"tol": C.TOL, "ltol": C.LTOL, "ops_mode": 1, "op": [], "host": [], "writer": {}}
    for n, edge in ((5, 5.0), (20, 8.0), (64, 12.0)):
        structs = bucket(C, MR, rng, n, 4096, edge)
        for size in (256, 4096):
            off, sp, fr, lat = C.pack(structs[:size])
            el = np.ones(size, np.int32)
            call = lambda: S.match_packed(off, sp, fr, lat, el, size, 0, C.TOL, C.LTOL, 1)       # noqa: E731
            t = median_time(call, a.reps)
            o = call()
            pairs = size * (size - 1) // 2
            assert int(o["n_cmp"][:, 0].sum()) == pairs
            row = {"n": n, "bucket": size, "pairs": pairs, "combinations": 24 * pairs, "seconds": t,
                   "pairs_per_s": pairs / t, "combinations_per_s": 24 * pairs / t,
                   "duplicates": int((o["dup_of"] >= 0).sum())}
            print(row, flush=True)
            out["op"].append(row)
        hb = a.host_bucket
        el = np.ones(hb, np.int32)
        t0 = time.perf_counter()
        r = MR.match_ref(structs[:hb], el, hb, C.TOL, C.LTOL, 1)
        th = time.perf_counter() - t0
        off, sp, fr, lat = C.pack(structs[:hb])
        o = S.match_packed(off, sp, fr, lat, el, hb, 0, C.TOL, C.LTOL, 1)
        assert np.array_equal(o["dup_of"], r["dup_of"]) and np.allclose(o["dup_rms"], r["dup_rms"], atol=1e-9)
        td = median_time(lambda: S.match_packed(off, sp, fr, lat, el, hb, 0, C.TOL, C.LTOL, 1), a.reps)
        row = {"n": n, "bucket": hb, "pairs": hb * (hb - 1) // 2, "numpy_seconds": th, "device_seconds": td,
               "numpy_pairs_per_s": hb * (hb - 1) / 2 / th}
        print(row, flush=True)
        out["host"].append(row)

    # ---- the writer: 5 000 samples, finish() without and with the matcher
    protos = []
    for k in range(60):
        n = 5 + k % 8
        Z = [57, 26] + [8] * (n - 2) if k % 2 else [38, 22] + [8] * (n - 2)
        protos.append(C.motif(rng, Z, C.lat([4.0 + 0.1 * (k % 7), 5.0 + 0.1 * (k % 5), 6.0 + 0.1 * (k % 3)]), dmin=1.0))
    ops = MR.signed_permutations(1)
    samples = []
    for _ in range(a.samples):
        Z, f, M = C.derive(rng, protos[rng.randint(60)], ops[rng.randint(24)], None)[0]
        abc = np.linalg.norm(M, axis=1)
        f = f - np.floor(f)
        samples.append((abc, (Z, f * abc + rng.normal(0, 0.02, f.shape))))
    ref = S.ReferenceSet(["ref-%d" % k for k in range(200)], [protos[k % 60][0] for k in range(200)],
                         [protos[k % 60][1] + 0.001 * (k // 60) for k in range(200)],
                         [list(np.linalg.norm(protos[k % 60][2], axis=1)) + [90, 90, 90] for k in range(200)])
    ref.screened()
    for name, matcher in (("without", None), ("with", S.Matcher(ref, C.TOL, C.LTOL, 1))):
        tmp = tempfile.mkdtemp()
        try:
            w = S.ResultsWriter(tmp, matcher=matcher)
            for b in range(0, a.samples, 100):
                part = samples[b:b + 100]
                w.add_batch(range(b, b + len(part)), np.array([p[0] for p in part]), [p[1] for p in part])
            t0 = time.perf_counter()
            counts = w.finish()
            out["writer"][name] = {"finish_seconds": time.perf_counter() - t0, "counts": counts}
            print(name, out["writer"][name], flush=True)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
