"""Cost of rotating inside the pack step: not the contract bench.

  pack     the pack kernel alone at B = 32, d = 32, 1 + 3 float64 parts, float64 ids (59.8 MB moved per launch): kernel
           time from `rocprofv3 --kernel-trace` over a child process of its own, for the un-rotated kernel and for one
           rotation table of each of the six access classes (which source axis feeds the output's fastest axis, and
           with which sign).
  loops    fed class-level loops over the dataset scripts/loop_bench.py writes, U-Net C = 4 and DFC-VAE C = 4: plain
           generators over 512 files, and augmented generators over 128 base files with 3 rotations each (the same 16
           batches an epoch); grids/s, --repeats times.

A tree without the rotating pack (an older commit: copy this file into its scripts/) measures what it has -- the
un-rotated kernel and the plain loops -- and `--parent that.json` puts those figures next to this tree's:

    python scripts/augment_bench.py --out profiles/feed_augment.json [--parent parent.json]
"""
import argparse
import csv
import glob
import inspect
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

D, B, REPS = 32, 32, 20


def table_class(rot):
    """(source axis that feeds the output's fastest axis, forward?)"""
    from icsg3d_amd.augment import rotate_host
    src = rotate_host(np.arange(27).reshape(3, 3, 3), rot)
    delta = int(src[1, 1, 2]) - int(src[1, 1, 1])
    return {9: 0, 3: 1, 1: 2}[abs(delta)], delta > 0


def class_tables():
    """name -> table, one per access class, found by composing (not trusted from a list)"""
    names = {(2, True): "A forward", (2, False): "A reversed", (0, True): "B from axis 0 forward",
             (0, False): "B from axis 0 reversed", (1, True): "B from axis 1 forward", (1, False): "B from axis 1 reversed"}
    out = {}
    for a in range(2, -2, -1):
        for b in range(2, -2, -1):
            for c in range(2, -2, -1):
                if (a, b, c) != (-1, -1, -1):
                    out.setdefault(names[table_class((a, b, c))], (a, b, c))
    return out


def has_rotations():
    from icsg3d_amd.engine import feed_pack
    return "rotations" in inspect.signature(feed_pack).parameters


def pack_child():
    from icsg3d_amd.engine import feed_pack
    rng = np.random.default_rng(0)
    parts = [rng.random((B, D, D, D, 1)), rng.random((B, D, D, D, 3))]
    lab = rng.integers(0, 95, (B, D, D, D)).astype(np.float64)
    runs = [("unrotated", None)] + (sorted(class_tables().items()) if has_rotations() else [])
    for name, rot in runs:
        for _ in range(REPS):
            if rot is None:
                feed_pack(parts, lab, "f64")
            else:
                feed_pack(parts, lab, "f64", rotations=np.tile(np.array(rot, np.int32), (B, 1)))
        print("ran %s %s" % (name, rot), flush=True)


def pack_measure(timeout):
    prof = tempfile.mkdtemp(prefix="icsg3d_augment_trace_")
    cmd = ["timeout", "-k", "10", str(timeout), "rocprofv3", "--kernel-trace", "-f", "csv", "-d", prof, "-o", "pack", "--",
           sys.executable, os.path.abspath(__file__), "--pack-child"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("profiled pack run failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-3000:]))
    traces = glob.glob(os.path.join(prof, "**", "*kernel_trace.csv"), recursive=True)
    rows = [row for f in traces for row in csv.DictReader(open(f)) if "feed_pack" in row["Kernel_Name"]]
    rows.sort(key=lambda x: int(x["Start_Timestamp"]))
    shutil.rmtree(prof, ignore_errors=True)
    names = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("ran ")]
    if len(rows) != REPS * len(names):
        raise SystemExit("expected %d pack launches, the trace has %d" % (REPS * len(names), len(rows)))
    moved = B * D ** 3 * (40 + 17)
    out = {}
    for k, name in enumerate(names):
        us = sorted((int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) * 1e-3 for x in rows[k * REPS + 2:(k + 1) * REPS])
        med = us[len(us) // 2]
        out[name] = {"kernel": rows[k * REPS]["Kernel_Name"].split("(")[0], "median_us": med, "min_us": us[0], "max_us": us[-1],
                     "launches": len(us), "tb_per_s": moved / med * 1e-6}
    return {"bytes_moved": moved, "classes": out}


def loops(samples, epochs, repeats, tmp_root, plain_only=False):
    import loop_bench as LB
    from icsg3d_amd.unet.data import UnetDataGenerator
    from icsg3d_amd.unet.unet import AtomUnet
    from icsg3d_amd.vae.data import VAEDataGenerator
    from icsg3d_amd.vae.lattice_vae import LatticeDFCVAE
    import contextlib
    import io
    import re
    C, NROT = 4, 3
    tmp = tempfile.mkdtemp(prefix="icsg3d_augment_bench_", dir=tmp_root)
    out = {}
    try:
        root = os.path.join(tmp, "matrices")
        ids, csvf = LB.write_dataset(root, samples)
        base = ids[:samples // (NROT + 1)]
        aug = has_rotations() and not plain_only
        np.random.seed(0)
        unet = AtomUnet(input_shape=(D, D, D, C), lr=1e-6, max_batch=B)
        kw = dict(batch_size=B, dim=(D, D, D), n_channels=C)
        gens = {"fed": UnetDataGenerator(ids, root, **kw)}
        if aug:
            gens["fed_augment"] = UnetDataGenerator(base, root, augment=dict(n_rot=NROT, seed=28), **kw)

        def uloop(g, n):
            t0 = time.perf_counter()
            unet.model.fit_generator(g, epochs=n, verbose=0, feed=True)
            unet._eng.sync()
            return n * len(g) * B / (time.perf_counter() - t0)

        rates = {k: [] for k in gens}
        for g in gens.values():
            uloop(g, 1)
        for _ in range(repeats):                                # alternating: both see the same machine
            for k, g in gens.items():
                rates[k].append(uloop(g, epochs))
        out["unet_c4"] = {k: {"grids_per_s": float(np.median(v)), "min": min(v), "max": max(v), "repeats": len(v),
                              "steps_per_figure": epochs * len(gens[k])} for k, v in rates.items()}
        pm = unet._get_weights()
        unet._eng.close()

        vkw = dict(data_path=root, dim=(D, D, D), n_channels=C, property_csv=csvf, n_bins=LB.NCOND, batch_size=B)
        val = VAEDataGenerator(ids[:B], **vkw)
        gens = {"fed": VAEDataGenerator(ids, **vkw)}
        if aug:
            gens["fed_augment"] = VAEDataGenerator(base, augment=dict(n_rot=NROT, seed=28), **vkw)
        np.random.seed(0)
        vae = LatticeDFCVAE(input_shape=(D, D, D, C), perceptual_model=pm, cond_shape=LB.NCOND, output_dir=tmp)

        def vloop(g, n):
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                vae.train(g, val, epochs=1 + n, weights=os.path.join(tmp, "vae.best.hdf5"), feed=True)
            secs = [float(s) for s in re.findall(r"Time: ([0-9.]+) s", buf.getvalue())][1:]
            return n * (len(g) + 1) * B / sum(secs)

        rates = {k: [] for k in gens}
        for _ in range(repeats):
            for k, g in gens.items():
                rates[k].append(vloop(g, epochs))
        out["vae_c4"] = {k: {"grids_per_s": float(np.median(v)), "min": min(v), "max": max(v), "repeats": len(v),
                             "steps_per_figure": epochs * (len(gens[k]) + 1)} for k, v in rates.items()}
        vae._eng.close(); vae._pm_eng.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed_augment.json"))
    ap.add_argument("--parent", default=None, help="JSON this script wrote on the parent commit: merged in as \"parent\"")
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tmp", default="/dev/shm")
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--no-loops", action="store_true")
    ap.add_argument("--no-pack", action="store_true")
    ap.add_argument("--plain-only", action="store_true",
                    help="loops: the plain generators only, the sequence a tree without the rotating pack runs")
    ap.add_argument("--pack-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.pack_child:
        return pack_child()
    from icsg3d_amd import _lib
    doc = {"d": D, "batch": B, "version": _lib.load().ics_version().decode(), "rotating_pack": has_rotations()}
    if not a.no_pack:
        doc["pack"] = pack_measure(a.timeout)
        print("pack:", json.dumps(doc["pack"]), flush=True)
    if not a.no_loops:
        doc["loops"] = loops(a.samples, a.epochs, a.repeats, a.tmp, a.plain_only)
        print("loops:", json.dumps(doc["loops"]), flush=True)
    if a.parent:
        with open(a.parent) as fh:
            doc["parent"] = json.load(fh)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
