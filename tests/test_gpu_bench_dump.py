"""bench.py --dump-outputs: what the last timed U-Net step computed, written after exactly --steps timed steps from
inputs that are the same on every run -- so that two runs of one build agree bit for bit, with or without --full, and
two builds can be compared output for output; and the line's `metric` is the same text on every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 4


def _bench(out_dir, steps, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--batch", str(B), "--dump-outputs", str(out_dir), *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    files = sorted(os.listdir(out_dir))
    assert files == ["unet_metric_sums.npy", "unet_state.npy"]
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in files) <= 64 << 20
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in files}


@pytest.mark.timeout(900)
def test_bench_dump_outputs_are_reproducible_and_follow_steps(tmp_path):
    from bench import DUMP_STATE_VALUES
    r2, a = _bench(tmp_path / "a", 2)
    r2b, b = _bench(tmp_path / "b", 2, "--full", "--no-cpu-baseline", "--no-inference", "--soak-seconds", "0")
    r3, c = _bench(tmp_path / "c", 3)
    assert r2["steps"] == r2b["steps"] == 2 and r3["steps"] == 3
    assert r2["ms_per_step"] > 0 and r2b["ms_per_step"] > 0 and r3["ms_per_step"] > 0
    # the line names its measurement with the same text on every run (measured rates only in the numeric fields)
    assert r2["metric"] == r2b["metric"] == r3["metric"] and "secondary" in r2b and r2b["unet_plus_vae"]["value"] > 0
    # a plain run measures only the headline; the events-off repeat and the DFC-VAE block are --full's
    assert r2b["ms_per_step_events_off"] > 0 and r2b["kernel_launches_per_step"] > 0
    assert not {"secondary", "unet_plus_vae", "ms_per_step_events_off", "kernel_launches_per_step"} & set(r2)
    sums, state = a["unet_metric_sums"], a["unet_state"]
    assert sums.dtype == np.float64 and sums.shape == (7,) and np.all(np.isfinite(sums))
    assert sums[6] == B * 32 ** 3                           # voxels of the batch the step saw
    assert state.dtype == np.float32 and state.shape == (DUMP_STATE_VALUES,) and np.all(np.isfinite(state))
    for k in a:                          # same inputs, same outputs: what --full adds runs after the dump
        assert np.array_equal(a[k], b[k]), k
    # one more timed step: one more Adam update of the state the dump samples
    assert not np.array_equal(a["unet_state"], c["unet_state"])
