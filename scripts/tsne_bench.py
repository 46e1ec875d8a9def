#!/usr/bin/env python3
"""The t-SNE map on one MI355X -> profiles/tsne_bench.json (or --out).

For each N of --sizes (default 2000 20000 78750; D = 256, perplexity 30, clustered codes from a seed):

  stages     wall time of the neighbour search, the affinities and the symmetrisation (host), from ics_op_tsne_prepare;
  iteration  wall time per iteration: the host clock around ics_op_tsne_run chunks of 50 iterations (each ends in a
             device synchronise and carries one KL check), median over the chunks after a warm-up chunk;
  total      stages + 1000 iterations (run in full while N <= --full-max, else stages + 1000 x the median iteration);
  kernels    per-kernel average from `rocprofv3 --kernel-trace --stats` over a run of its own (a child process, 100
             iterations): repulsion, slab combine, attraction + update;
  pair rate  N^2 pairs over the repulsion kernel's time, and its share of the fp32 vector peak (157.3 TFLOP/s): 16 floating
             point operations are counted per pair -- 2 subtractions, 2 fused multiply-adds for 1 + |d|^2 (4), the
             reciprocal (1), its Newton step (2 FMA = 4), q^2 (1), the sum of q (1), 2 FMA into the force (4), and the
             1/16 share of the three fp64 additions per 16 pairs is left out;
  sklearn    sklearn.manifold.TSNE() (Barnes-Hut, angle 0.5, n_jobs=16) on the host at N <= --sklearn-max, where
             scikit-learn imports.

A record, not a gate.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOP_PER_PAIR = 16
PEAK_FP32_VECTOR = 157.3e12


def codes(n, dim=256, seed=0, clusters=10):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(clusters, dim)) * 4.0
    return (centres[rng.integers(0, clusters, n)] + rng.normal(size=(n, dim))).astype(np.float32)


def prepared(n):
    from icsg3d_amd.tsne import Tsne, pca_init
    x = codes(n)
    t = Tsne(x.shape[1], n, perplexity=30.0)
    t.append(x)
    t.prepare(pca_init(x))
    return t, x


def child(n, iters):
    t, _ = prepared(n)
    t.run(iters)
    t.close()


def kernel_stats(n, iters, out_dir):
    d = os.path.join(out_dir, "tsne_prof_%d" % n)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "-o", "prof", "--", sys.executable,
           os.path.abspath(__file__), "--child", str(n), "--child-iters", str(iters)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        return {"error": (r.stderr or r.stdout)[-400:]}
    rows = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            for key in ("tsne_repulsion", "tsne_combine", "tsne_step", "tsne_knn", "tsne_affinity", "tsne_reduce2"):
                if key + "_kernel" in row["Name"]:
                    rows[key] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 20000, 78750])
    ap.add_argument("--full-max", type=int, default=20000)
    ap.add_argument("--sklearn-max", type=int, default=20000)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--child-iters", type=int, default=100)
    ap.add_argument("--scratch", default=os.path.join(ROOT, "output", "tsne_prof"), help="where the traces go")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsne_bench.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.child_iters)

    res = {"dim": 256, "perplexity": 30.0, "flop_per_pair": FLOP_PER_PAIR, "sizes": {}}
    for n in a.sizes:
        t, x = prepared(n)
        r = {"stages_s": t.seconds, "edges": int(t.graph()[0][-1])}
        t.run(50)                                                     # warm-up chunk
        chunks = []
        for _ in range(6):
            t0 = time.perf_counter()
            t.run(50)
            chunks.append((time.perf_counter() - t0) / 50)
        r["iteration_ms"] = {"median": 1e3 * float(np.median(chunks)), "min": 1e3 * float(np.min(chunks)), "chunks": 6}
        stages = sum(t.seconds.values())
        if n <= a.full_max:
            t0 = time.perf_counter()
            t.prepare(np.zeros((n, 2), np.float32) + 1e-4 * x[:, :2])
            while not t.run(250):
                pass
            r["total_1000_s"] = {"measured": time.perf_counter() - t0, "n_iter": t.read(False)["n_iter"]}
        else:
            r["total_1000_s"] = {"stages_plus_1000_median_iterations": stages + float(np.median(chunks)) * 1000}
        t.close()
        if not a.no_trace:
            r["kernels"] = k = kernel_stats(n, a.child_iters, a.scratch)
            if "tsne_repulsion" in k:
                rate = float(n) * n / (k["tsne_repulsion"]["average_us"] * 1e-6)
                r["repulsion"] = {"pairs_per_s": rate, "share_of_fp32_vector_peak": rate * FLOP_PER_PAIR / PEAK_FP32_VECTOR}
        if n <= a.sklearn_max:
            try:
                from sklearn.manifold import TSNE
                t0 = time.perf_counter()
                TSNE(n_components=2, n_jobs=16).fit(x)
                r["sklearn_default_s"] = time.perf_counter() - t0
            except ImportError:
                r["sklearn_default_s"] = None
        res["sizes"][str(n)] = r
        print(n, json.dumps(r), flush=True)
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        res["commit"] = None
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
