#!/usr/bin/env python3
"""eval.py's pieces on one MI355X -> profiles/eval_bench.json (or --out).

  chain    per B = 32, d = 32, C = 4 batch: VaeEngine.reconstruct_to_atoms on the resident batch against the two-call
           path encode + decode_to_atoms (z to the host and back);
  feed     voxelise_batch (sites -> resident batch on the device) against upload_batch of host float32 grids;
  match    ics_op_match_emd on 32 / 1024 / 16384 samples of 40 x 40 points and on 256 x 2048, against a per-sample
           cdist + linear_sum_assignment loop on the host (skipped if scipy does not import);
  loop     the eval loop end to end (voxelise feed, chain, refine_atoms, metrics incl. the EMD) in grids/s, random
           weights: their masks are not a trained model's, so the host refine cost is not representative.

Every time is the host clock around calls that end in a device synchronise; median of --reps after --warmup.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchutil import timeit  # noqa: E402


def structures(rng, n, max_sites=40):
    from icsg3d_amd.matrices import Structures
    sites = []
    for _ in range(n):
        ns = int(rng.integers(2, max_sites + 1))
        sites.append((rng.uniform(0.0, 1.0, (ns, 3)), rng.integers(1, 90, ns).astype(float),
                      rng.uniform(0.6, 1.6, ns), np.r_[rng.uniform(3, 9, 3), 90.0, 90.0, 90.0]))
    return Structures.from_sites(sites)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop_batches", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.json"))
    a = ap.parse_args()
    from icsg3d_amd import _lib as L
    from icsg3d_amd.evaluate import emd, reconstruction_metrics
    from icsg3d_amd.matrices import make_jobs, voxelise
    from icsg3d_amd.synthetic import random_engines
    from icsg3d_amd.watershed import refine_atoms
    assert L.device_count() >= 1, "no HIP device visible"
    rng = np.random.default_rng(0)
    res = {"reps": a.reps, "warmup": a.warmup}

    B, d, C = 32, 32, 4
    ve, un = random_engines(d, C, B)
    s = structures(rng, B)
    jobs = make_jobs(B)
    M, _, p = voxelise(s, d=d, want=("M", "p"))
    x = np.concatenate([M[..., None], p], -1).astype(np.float32)
    cond = np.eye(10, dtype=np.float32)[rng.integers(0, 10, B)]
    eps = rng.standard_normal((B, 256)).astype(np.float32)

    def two_call():
        _, _, z = ve.encode(x, cond, eps)
        ve.decode_to_atoms(un, z, cond)

    def chain_upload():
        ve.upload_batch(x, cond, eps)
        ve.reconstruct_to_atoms(un)

    def chain_feed():
        ve.voxelise_batch(s, jobs, cond, eps)
        ve.reconstruct_to_atoms(un)

    ve.upload_batch(x, cond, eps)
    res["chain"] = {"B": B, "d": d, "C": C,
                    "encode_plus_decode_to_atoms": timeit(two_call, a.reps, a.warmup),
                    "upload_plus_chain": timeit(chain_upload, a.reps, a.warmup),
                    "voxelise_feed_plus_chain": timeit(chain_feed, a.reps, a.warmup)}

    def feed():
        ve.voxelise_batch(s, jobs, cond, eps)
        ve.sync()

    def upload():
        ve.upload_batch(x, cond, eps)
        ve.sync()
    res["feed"] = {"voxelise_batch": timeit(feed, a.reps, a.warmup), "upload_batch": timeit(upload, a.reps, a.warmup),
                   "host_grid_bytes": int(x.nbytes)}

    try:
        from scipy.optimize import linear_sum_assignment
        from scipy.spatial.distance import cdist
    except ImportError:
        linear_sum_assignment = None
    match = {}
    for name, n, na, nb in (("40x40_x32", 32, 40, 40), ("40x40_x1024", 1024, 40, 40), ("40x40_x16384", 16384, 40, 40),
                            ("256x2048_x1", 1, 256, 2048)):
        xs = [rng.uniform(0, 10, (na, 3)) for _ in range(n)]
        ys = [rng.uniform(0, 10, (nb, 3)) for _ in range(n)]
        reps = max(3, a.reps // (4 if n > 1000 else 1))
        row = {"samples": n, "points": [na, nb], "device_op": timeit(lambda: emd(xs, ys), reps, a.warmup)}
        if linear_sum_assignment is not None:
            def host():
                for xx, yy in zip(xs, ys):
                    dist = cdist(xx, yy)
                    r, c = linear_sum_assignment(dist)
                    dist[r, c].sum()
            row["host_loop"] = timeit(host, max(1, reps // 4), 1)
            row["host_over_device"] = row["host_loop"]["median_ms"] / row["device_op"]["median_ms"]
        match[name] = row
    res["match"] = match

    # the eval loop end to end: sites -> device feed -> chain -> refine_atoms -> metrics (EMD on the device)
    s_all = structures(rng, B * a.loop_batches)
    from icsg3d_amd.matrices import Structures
    ntimes = []
    for rep in range(2):
        t0 = time.perf_counter()
        for k in range(a.loop_batches):
            idx = np.arange(k * B, (k + 1) * B)
            sb = Structures(s_all.nsites[idx], s_all.xyz[idx], s_all.z[idx], s_all.sigma[idx], s_all.abc[idx])
            ve.voxelise_batch(sb, make_jobs(B), cond, eps)
            out = ve.reconstruct_to_atoms(un, max_atoms=2048, want_regions=True)
            refine_atoms(out, max_iters=5)
            reconstruction_metrics(out["atoms"], out["coord_minmax"], [sb.xyz[i, :sb.nsites[i]] for i in range(B)],
                                   sb.abc, out["failed"], 0.25, d)
        ntimes.append(time.perf_counter() - t0)
    t = min(ntimes[1:] or ntimes)
    res["loop"] = {"grids": B * a.loop_batches, "seconds": t, "grids_per_s": B * a.loop_batches / t,
                   "note": "random weights: masks unlike a trained model's, refine cost not representative"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
