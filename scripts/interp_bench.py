#!/usr/bin/env python3
"""interpolate.py's chain on one MI355X -> profiles/interp_bench.json (or --out).

10 pairs x 8 steps at d = 32, C = 4 on handles of max_batch 80 (one group), random weights:

  chain      VaeEngine.interpolate (ics_vae_interpolate): endpoints in, z_ends / z_path / 80 frames out;
  composed   the same result from encoder calls x2, the numpy walk and a decoder call (VaeEngine.encode x2 + lerp_path +
             VaeEngine.decode) -- the only way before the chain existed;
  atoms      VaeEngine.interpolate_to_atoms against encode x2 + lerp_path + decode_to_atoms on the host-made path.

A record, not a gate.  Every time is the host clock around calls that end in a device synchronise; median of --reps after
--warmup.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchutil import timeit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interp_bench.json"))
    a = ap.parse_args()
    from icsg3d_amd.interpolate import lerp_path
    from icsg3d_amd.synthetic import random_engines, synthetic_batch
    P, S, d, C = a.pairs, a.steps, a.d, a.channels
    ve, un = random_engines(d, C, P * S)
    rng = np.random.default_rng(0)
    X = synthetic_batch(2 * P, d, C, seed=1, noise=1e-3)[0].astype(np.float32)
    A, B = np.ascontiguousarray(X[0::2]), np.ascontiguousarray(X[1::2])
    cond = np.eye(10, dtype=np.float32)[rng.integers(0, 10, P)]
    eps = rng.standard_normal((P, 2, 256)).astype(np.float32)
    ea, eb = np.ascontiguousarray(eps[:, 0]), np.ascontiguousarray(eps[:, 1])
    alpha = np.linspace(0, 1, S)
    tiled = np.repeat(cond, S, axis=0)

    def path():
        z_a, z_b = ve.encode(A, cond, ea)[2], ve.encode(B, cond, eb)[2]
        return lerp_path(z_a, z_b, alpha).reshape(P * S, 256)
    _, sig = un.predict(ve.decode(path()[:8], tiled[:8]))
    thresh = float(np.quantile(sig, 0.7))          # ~30 % of the voxels pass: segmentation work with random weights
    kw = dict(thresh=thresh, min_voxels=3, max_atoms=512)

    res = {"pairs": P, "steps": S, "d": d, "channels": C, "max_batch": P * S, "mask_threshold": thresh,
           "chain": timeit(lambda: ve.interpolate(A, B, cond, ea, eb, alpha), a.reps, a.warmup),
           "composed": timeit(lambda: ve.decode(path(), tiled), a.reps, a.warmup),
           "atoms_chain": timeit(lambda: ve.interpolate_to_atoms(un, A, B, cond, ea, eb, alpha, **kw), a.reps, a.warmup),
           "atoms_composed": timeit(lambda: ve.decode_to_atoms(un, path(), tiled, **kw), a.reps, a.warmup)}
    res["chain_speedup"] = res["composed"]["median_ms"] / res["chain"]["median_ms"]
    res["atoms_chain_speedup"] = res["atoms_composed"]["median_ms"] / res["atoms_chain"]["median_ms"]
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
