#!/usr/bin/env python3
"""view_results.py's renderers on one MI355X -> profiles/render_bench.json (or --out).

  ops       images/s of ics_op_render_density (both modes), ics_op_render_labels and ics_op_render_atoms at d = 32, B = 32,
            256 x 256: one upload, one launch, one download of 32 float RGBA pictures (33.5 MB) per call.
            The op time is dominated by the download; the kernels' own times come from a kernel trace of this script
            (rocprofv3 --kernel-trace --stats -- python scripts/render_bench.py --reps 5).  An LDS-staged form of the
            density kernel was measured that way against the global-read form and dropped.
  resident  VaeEngine.render_resident(1) after a reconstruct_to_atoms against upload plus op: render.density on the same
            reconstruction held on the host (the download that route also needs is not counted).
  context   when matplotlib imports: one ax.voxels panel of a 10^3 volume under Agg, the reference's picture
            (viz.py:43-66 after its resize), for scale only -- it is another picture by another method.

Every time is the host clock around calls that end in a device synchronise; median of --reps after --warmup.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchutil import timeit  # noqa: E402


def per_second(row, images):
    row["images_per_s"] = images / (row["median_ms"] * 1e-3)
    return row


def voxels_panel(vol10):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from matplotlib import cm
    fig = plt.figure(figsize=(2.56, 2.56), dpi=100)
    ax = fig.add_subplot(111, projection="3d")
    ax.voxels(np.ones(vol10.shape, bool), facecolors=cm.viridis(vol10), alpha=0.2)
    fig.canvas.draw()
    plt.close(fig)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    a = ap.parse_args()
    from icsg3d_amd import _lib as L
    from icsg3d_amd import render as P
    from icsg3d_amd.synthetic import random_engines, synthetic_batch
    assert L.device_count() >= 1, "no HIP device visible"
    d, B, size = 32, 32, 256
    X, S, cond = synthetic_batch(B, d, 1, seed=0)
    X = np.minimum(X, 1.0).astype(np.float32)
    rng = np.random.default_rng(0)
    sets = [(rng.integers(1, 95, 20), rng.uniform(2, d - 2, (20, 3))) for _ in range(B)]
    res = {"d": d, "B": B, "size": size, "reps": a.reps, "warmup": a.warmup}

    ops = {}
    for name, fn in (("density_value", lambda: P.density(X, size=size, mode="value", alpha=0.6)),
                     ("density_flat", lambda: P.density(X, size=size, mode="flat", alpha=0.2, floor=-1.0)),
                     ("labels", lambda: P.labels(S, size=size)),
                     ("atoms", lambda: P.atoms(sets, d, size=size))):
        ops[name] = per_second(timeit(fn, a.reps, a.warmup), B)
        print(name, json.dumps(ops[name]), flush=True)
    res["ops"] = ops

    # the resident path against upload + op
    ve, un = random_engines(d, 1, B, seed=0)
    eps = rng.standard_normal((B, ve.latent_dim)).astype(np.float32)
    ve.reconstruct_to_atoms(un, X, cond, eps)
    recon = ve.decode(ve.encode(X, cond, eps)[2], cond)
    kw = dict(size=size, mode="value", alpha=0.6)
    assert np.array_equal(ve.render_resident(1, **kw), P.density(recon, **kw))
    res["resident"] = {"render_resident": per_second(timeit(lambda: ve.render_resident(1, **kw), a.reps, a.warmup), B),
                       "upload_plus_op": per_second(timeit(lambda: P.density(recon, **kw), a.reps, a.warmup), B)}
    print("resident", json.dumps(res["resident"]), flush=True)

    try:
        vol10 = X[0, ::3, ::3, ::3, 0][:10, :10, :10]
        voxels_panel(vol10)
        res["context_matplotlib_voxels_10cubed"] = timeit(lambda: voxels_panel(vol10), 3, 0)
    except ImportError:
        res["context_matplotlib_voxels_10cubed"] = None
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
