"""What the *_bench.py scripts share (they run as `python scripts/x_bench.py`, so a sibling import finds this)."""
import time

import numpy as np


def timeit(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * float(np.min(ts)), "reps": reps}
