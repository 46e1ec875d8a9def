"""Confusion matrix on the device: what the op and the accumulator loop cost against the host.

  1. ics_op_confusion on 16 777 216 pairs (98 % background) per label kind, host pointers in and counts out -- the upload
     is inside the time -- against np.bincount(t * ncls + p, minlength = ncls^2) of the same arrays on the host;
  2. eval_unet.py's loop (confusion_batch per batch, one read at the end) in grids/s against predict_labels plus a host
     bincount per batch, on one engine (B = 32, d = 32, C = 1, 95 classes); the kernel's own time per launch comes from the
     engine's profiler in a separate pass.

  python scripts/confusion_bench.py [--out profiles/confusion_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchutil import timeit  # noqa: E402

N, NCLS = 1 << 24, 95


def op_bench():
    from icsg3d_amd.engine import confusion
    rng = np.random.default_rng(0)
    t = np.where(rng.uniform(size=N) < 0.98, 0, rng.integers(0, NCLS, size=N)).astype(np.uint8)
    p = np.where(rng.uniform(size=N) < 0.9, t, rng.integers(0, NCLS, size=N)).astype(np.uint8)
    m = (t != 0).astype(np.uint8)
    out = {"how": "ics_op_confusion on %d pairs, 98 %% background, %d classes, median of 5 calls after 2, host pointers in and "
                  "counts out (the upload is inside the time); np.bincount(t * ncls + p) of the same arrays on the host, "
                  "median of 3" % (N, NCLS)}
    for name, dtype in (("uint8", np.uint8), ("float32", np.float32), ("float64", np.float64)):
        tt = t.astype(dtype)
        dev = timeit(lambda: confusion(tt, p, NCLS, mask=m), 5, 2)
        nomask = timeit(lambda: confusion(tt, p, NCLS), 5, 2)
        host = timeit(lambda: np.bincount(tt.astype(np.int64) * NCLS + p, minlength=NCLS * NCLS), 3, 1)
        matrix, _, oor = confusion(tt, p, NCLS, mask=m)
        assert oor == 0 and np.array_equal(matrix.reshape(-1), np.bincount(tt.astype(np.int64) * NCLS + p, minlength=NCLS * NCLS))
        nbytes = N * (np.dtype(dtype).itemsize + 2)
        out[name] = {"n": N, "op_ms_median": dev["median_ms"], "op_ms_min": dev["min_ms"],
                     "op_without_mask_ms_median": nomask["median_ms"],
                     "op_GBps_incl_upload": nbytes / dev["median_ms"] / 1e6,
                     "host_bincount_ms_median": host["median_ms"], "host_over_op": host["median_ms"] / dev["median_ms"]}
        print(name, out[name], flush=True)
    return out


def loop_bench(batches=20, B=32, d=32):
    from icsg3d_amd.engine import UnetEngine
    from icsg3d_amd.synthetic import synthetic_batch
    X, lab, _ = synthetic_batch(B, d, 1, seed=0, noise=1e-3)
    X, lab = np.asarray(X, np.float32), np.asarray(lab, np.uint8)
    eng = UnetEngine(in_channels=1, num_classes=NCLS, d=d, max_batch=B)
    eng.confusion_open()

    def device_loop():
        eng.confusion_reset()
        for _ in range(batches):
            eng.confusion_batch(X, lab, 0.8)
        return eng.confusion_read()

    def host_loop():
        total = np.zeros(NCLS * NCLS, np.int64)
        occ = np.zeros(4, np.int64)
        for _ in range(batches):
            sp, mk = eng.predict_labels(X, 0.8)
            total += np.bincount(lab.reshape(-1).astype(np.int64) * NCLS + sp.reshape(-1), minlength=NCLS * NCLS)
            occ += np.bincount((lab.reshape(-1) != 0) * 2 + (mk.reshape(-1) != 0), minlength=4)
        return total, occ

    def resident_loop():                       # no upload at all: the forward pass and the count
        eng.confusion_reset()
        eng.upload_batch(X, lab)
        for _ in range(batches):
            eng.confusion_step(0.8)
        return eng.confusion_read()

    r = device_loop()
    total, occ = host_loop()
    assert np.array_equal(r["matrix"].reshape(-1), total) and np.array_equal(r["occupancy"].reshape(-1), occ)
    td, th, tr = timeit(device_loop, 5, 1), timeit(host_loop, 5, 1), timeit(resident_loop, 5, 1)
    eng.profile_enable(True)
    resident_loop()
    rows = {r["label"]: r for r in eng.profile_rows()}
    eng.profile_enable(False)
    k = rows.get("confusion")
    out = {"how": "one engine, B = %d, d = %d, C = 1, %d classes, %d batches per loop, median of 5 loops after 1; grids/s = "
                  "batches * B / loop time" % (B, d, NCLS, batches),
           "confusion_batch_loop": {"ms_median": td["median_ms"], "grids_per_s": batches * B / td["median_ms"] * 1e3},
           "predict_labels_plus_host_bincount_loop": {"ms_median": th["median_ms"], "grids_per_s": batches * B / th["median_ms"] * 1e3},
           "confusion_step_resident_loop": {"ms_median": tr["median_ms"], "grids_per_s": batches * B / tr["median_ms"] * 1e3},
           "kernel_per_launch_ms": None if not k else k["ms"] / max(k["launches"], 1),
           "kernel_pairs_per_launch": B * d ** 3,
           "kernel_GBps": None if not k or not k["ms"] else 3.0 * B * d ** 3 * k["launches"] / k["ms"] / 1e6}
    print(out, flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "confusion_bench.json"))
    a = ap.parse_args()
    t0 = time.time()
    rec = {"what": "confusion matrix on the device (DESIGN.md section 26): the op against np.bincount, the accumulator loop "
                   "against predict_labels + a host bincount per batch", "op": op_bench(), "loop": loop_bench()}
    rec["seconds"] = time.time() - t0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)
