"""Voxelisation measurements: not the contract bench.

1. ics_op_voxelise's kernel per job at d = 32 / 64 / 128, 40 sites, 256 jobs: a child process runs the op under
   `rocprofv3 --kernel-trace` (kernel time from the trace, HIP-event clocked by the profiler), and the result is set
   against the fp64 vector peak (nominal operations per voxel-site pair below) and HBM write bandwidth.
2. Training throughput (grids/s) of the U-Net step (B = 32, C = 4, d = 32) and the DFC-VAE step (same batch) fed two
   ways: ics_*_voxelise_batch from site data, and the on-disk loaders (UnetDataGenerator / VAEDataGenerator) over the
   files create_matrices.py wrote, uploaded with upload_batch.  Host clock around K steps ending in a device sync.

    python scripts/voxel_bench.py --out voxel_bench.json
Every stage is bounded by --timeout seconds (the profiled child by `timeout -k 10`).
"""
import argparse
import csv
import glob
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

OP_DS = (32, 64, 128)
OP_JOBS, OP_SITES = 256, 40
FP64_PEAK = 78.6e12        # MI355X fp64 vector, spec
HBM_PEAK = 8.0e12          # spec; 6.3 TB/s measured for a float4 copy
# per voxel-site pair: 3 sub, 3 mul, 2 add (distance^2), sqrt, 2 compares, mul (D^2), mul (scale), exp, mul, add;
# sqrt and exp count 1 each although gfx950 runs each as a multi-instruction fp64 sequence
NOMINAL_FLOP = 16


def structures(rng, count, nsites, ncls=95):
    from icsg3d_amd.matrices import Structures
    sites = []
    for _ in range(count):
        sites.append((rng.uniform(0, 1, (nsites, 3)), rng.integers(1, ncls, nsites).astype(float),
                      rng.uniform(0.6, 1.6, nsites), np.r_[rng.uniform(3, 9, 3), 90.0, 90.0, 90.0]))
    return Structures.from_sites(sites), sites


def op_child():
    from icsg3d_amd.matrices import voxelise
    rng = np.random.default_rng(0)
    s, _ = structures(rng, 16, OP_SITES)
    jobs = np.array([(k % 16, k % 4 - 1, (k // 4) % 4 - 1, (k // 16) % 4 - 1) for k in range(OP_JOBS)], np.int32)
    for d in OP_DS:
        want = ("M", "S", "p") if d < 128 else ("M",)     # d = 128: 256 jobs of all three would be 21 GB of host arrays
        voxelise(s, jobs=jobs[:8], d=d, want=want)        # warm-up
        t0 = time.perf_counter()
        voxelise(s, jobs=jobs, d=d, want=want)
        print("op d=%d %s: %.3f s including copies" % (d, "".join(want), time.perf_counter() - t0), flush=True)


def op_measure(out_dir, timeout):
    prof = os.path.join(out_dir, "voxel_op_trace")
    shutil.rmtree(prof, ignore_errors=True)
    cmd = ["timeout", "-k", "10", str(timeout), "rocprofv3", "--kernel-trace", "-f", "csv", "-d", prof, "-o", "op", "--",
           sys.executable, os.path.abspath(__file__), "--op-child"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("profiled op run failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-3000:]))
    traces = glob.glob(os.path.join(prof, "**", "*kernel_trace.csv"), recursive=True)
    rows = [row for f in traces for row in csv.DictReader(open(f)) if "voxelise_kernel" in row["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    gkey = "Grid_Size_X" if rows and "Grid_Size_X" in rows[0] else "Grid_Size"
    ykey = "Grid_Size_Y" if rows and "Grid_Size_Y" in rows[0] else None
    res = {}
    for d in OP_DS:
        V = d ** 3
        gx = -(-V // 1024) * 256                     # threads along x of one launch at this d
        ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if int(r[gkey]) == gx]
        # the timed call's launches: every launch after the 8-job warm-up's (one chunk each)
        chunk_jobs = [int(r[ykey]) if ykey else 0 for r in rows if int(r[gkey]) == gx]
        k = 1                                         # skip the warm-up launch
        t = sum(ns[k:]) * 1e-9
        jobs = sum(chunk_jobs[k:]) or OP_JOBS
        outs = 5 if d < 128 else 1
        per_job = t / jobs
        flop = float(V) * OP_SITES * NOMINAL_FLOP
        byts = float(V) * 8 * outs
        res["d%d" % d] = dict(jobs=jobs, launches=len(ns) - k, kernel_us_per_job=per_job * 1e6,
                              outputs="M,S,p" if outs == 5 else "M", nominal_fp64_tflops=flop / per_job / 1e12,
                              frac_fp64_peak=flop / per_job / FP64_PEAK, write_tbps=byts / per_job / 1e12,
                              frac_hbm_peak=byts / per_job / HBM_PEAK)
    shutil.rmtree(prof, ignore_errors=True)
    res["log"] = r.stdout[-1500:]
    return res


def loop_measure(steps, warmup, tmp):
    import create_matrices as CM
    from icsg3d_amd.engine import UnetEngine, VaeEngine
    from icsg3d_amd.matrices import Structures
    from icsg3d_amd.synthetic import glorot_params, unet_param_shapes
    from icsg3d_amd.unet.data import UnetDataGenerator
    from icsg3d_amd.vae.data import VAEDataGenerator
    B, d, C, nrot, nstruct = 32, 32, 4, 3, 64
    rng = np.random.default_rng(1)
    src = os.path.join(tmp, "bench", "sites")
    os.makedirs(src)
    sites = []
    for i in range(nstruct):
        ns = int(rng.integers(4, 41))
        site = (rng.uniform(0, 1, (ns, 3)), rng.integers(1, 95, ns).astype(float), rng.uniform(0.6, 1.6, ns),
                np.r_[rng.uniform(3, 9, 3), 90.0, 90.0, 90.0])
        sites.append(site)
        np.savez(os.path.join(src, "mp-%d.npz" % (1000 + i)), frac_coords=site[0], Z=site[1], radii=site[2], lattice=site[3])
    t0 = time.perf_counter()
    CM.main(["--name", "bench", "--root", tmp, "--d", str(d), "--nrot", str(nrot), "--seed", "0", "--batch", "16"])
    t_create = time.perf_counter() - t0
    sdir = os.path.join(tmp, "bench", "matrices")
    with open(os.path.join(tmp, "property.csv"), "w") as f:
        f.write("task_id,formation_energy_per_atom,nsites\n")
        for i in range(nstruct):
            f.write("mp-%d,%f,%d\n" % (1000 + i, rng.normal(), len(sites[i][1])))
    ids = sorted(os.listdir(os.path.join(sdir, "density_matrices")))
    structs = Structures.from_sites(sites)
    rs = np.random.RandomState(0)
    jobs_all = np.array([(i, *rs.choice(3, 3)) if k else (i, -1, -1, -1) for i in range(nstruct) for k in range(1 + nrot)],
                        np.int32)
    nb = len(jobs_all) // B
    res = dict(grids_on_disk=len(ids), create_matrices_s=t_create, B=B, d=d, C=C, steps=steps)

    def timed(step_fn):
        for i in range(warmup):
            step_fn(i)
        eng_sync()
        t0 = time.perf_counter()
        for i in range(steps):
            step_fn(warmup + i)
        eng_sync()
        dt = (time.perf_counter() - t0) / steps
        return dict(ms_per_step=dt * 1e3, grids_per_s=B / dt)

    ue = UnetEngine(in_channels=C, d=d, max_batch=B, lr=1e-6)
    ue.set_weights(glorot_params(unet_param_shapes(C, 95), 1))
    eng_sync = ue.sync
    gen = UnetDataGenerator(ids, sdir, batch_size=B, dim=(d, d, d), n_channels=C)

    def unet_loader(i):
        X, (y, _) = gen[i % len(gen)]
        ue.upload_batch(X, y)
        ue.train_step_resident(False)

    def unet_feed(i):
        ue.voxelise_batch(structs, jobs_all[(i % nb) * B:(i % nb + 1) * B])
        ue.train_step_resident(False)

    def unet_resident(i):
        ue.train_step_resident(False)

    res["unet_loader"] = timed(unet_loader)
    res["unet_feed"] = timed(unet_feed)
    res["unet_resident_only"] = timed(unet_resident)
    del ue

    pu = UnetEngine(in_channels=C, d=d, max_batch=B)
    pu.set_weights(glorot_params(unet_param_shapes(C, 95), 2))
    ve = VaeEngine(pu, in_channels=C, d=d, max_batch=B)
    eng_sync = ve.sync
    vgen = VAEDataGenerator(ids, sdir, batch_size=B, dim=(d, d, d), n_channels=C,
                            property_csv=os.path.join(tmp, "property.csv"))
    eps = np.random.default_rng(3).standard_normal((B, 256)).astype(np.float32)
    conds = [vgen[i][1] for i in range(len(vgen))]

    def vae_loader(i):
        X, cond = vgen[i % len(vgen)]
        ve.upload_batch(X, cond, eps)
        ve.train_step_resident(False)

    def vae_feed(i):
        ve.voxelise_batch(structs, jobs_all[(i % nb) * B:(i % nb + 1) * B], conds[i % len(conds)], eps)
        ve.train_step_resident(False)

    def vae_resident(i):
        ve.train_step_resident(False)

    res["vae_loader"] = timed(vae_loader)
    res["vae_feed"] = timed(vae_feed)
    res["vae_resident_only"] = timed(vae_resident)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op-child", action="store_true")
    ap.add_argument("--out", default="voxel_bench.json")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--skip-op", action="store_true")
    ap.add_argument("--skip-loop", action="store_true")
    a = ap.parse_args()
    if a.op_child:
        op_child()
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    res = {}
    if not a.skip_op:
        res["op"] = op_measure(os.path.dirname(os.path.abspath(a.out)), a.timeout)
        print(json.dumps(res["op"], indent=1), flush=True)
    if not a.skip_loop:
        tmp = tempfile.mkdtemp(prefix="voxel_bench_")
        try:
            res["train_loop"] = loop_measure(a.steps, a.warmup, tmp)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        print(json.dumps(res["train_loop"], indent=1), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
