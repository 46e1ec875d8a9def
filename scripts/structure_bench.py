#!/usr/bin/env python3
"""generate.py's structure stage on one MI355X -> profiles/structure_bench.json (or --out).

  op      ics_op_structure_screen (icsg3d_amd.structures.screen_packed: one upload, the kernels, one download) on 100,
          1 024 and 16 384 structures of 5 - 40 atoms (cells 3 - 12 A, every second one skewed, angles 60 - 120) and on
          one 2048-atom structure, against a vectorised numpy host loop doing the same arithmetic per structure
          (fractional coordinates, wrapped differences, the exact image search over the range the cell asks for, the
          minimum pair, the count under tol, the nearest neighbours, the histogram).  The two are compared on every
          output before they are timed.
  tail    generate.py's per-batch tail (B = 100 samples of 5 - 40 atoms, d = 32: the coordinate shift and the five .npy
          files per sample) without and with the new stage (one screen per batch, formula, CIF, results row, results.json
          record).  The networks are not part of it.

Every time is the host clock around calls that end in a device synchronise; median of --reps after --warmup.
"""
import argparse
import itertools
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchutil import timeit  # noqa: E402


def draw(rng, n, lo, hi, S):
    """n structures of lo..hi atoms: (species, xyz, abc, angles)."""
    out = []
    for k in range(n):
        abc = rng.uniform(3, 12, 3) if hi <= 64 else rng.uniform(40, 60, 3)
        ang = np.array([90.0, 90.0, 90.0])
        while k % 2:
            ang = rng.integers(60, 121, 3).astype(np.float64)
            try:
                if S.cell(abc, ang)[1] >= 0.3 * abc.prod():
                    break
            except ValueError:
                pass
        na = int(rng.integers(lo, hi + 1))
        out.append((rng.integers(1, 95, na).astype(np.int32), rng.uniform(-0.1, 1.1, (na, 3)) * abc, abc, ang))
    return out


def pack(structs):
    off = np.zeros(len(structs) + 1, np.int32)
    off[1:] = np.cumsum([len(s[0]) for s in structs])
    return (off, np.concatenate([s[0] for s in structs]), np.concatenate([s[1] for s in structs]),
            np.array([s[2] for s in structs]), np.array([s[3] for s in structs]))


def host_screen(structs, S, tol=0.5):
    """The op's arithmetic in numpy, one structure at a time, pairs vectorised."""
    res = []
    for sp, xyz, abc, ang in structs:
        M, vol, g = S.cell(abc, ang)
        n = len(sp)
        frac = xyz / abc
        hist = np.bincount(sp[(sp >= 1) & (sp < 95)], minlength=95)
        if n < 2:
            res.append((np.inf, (-1, -1), 0, np.full(n, np.inf), hist))
            continue
        w = frac - np.floor(frac)
        iu = np.triu_indices(n, 1)
        df = w[iu[1]] - w[iu[0]]
        df -= np.rint(df)
        d0 = np.sqrt(((df @ M) ** 2).sum(-1))
        R = np.floor(d0.max() * g + 0.5 + 1e-9).astype(int)
        best = np.full(len(d0), np.inf)
        for im in itertools.product(*(range(-r, r + 1) for r in R)):
            v = (df + np.array(im, np.float64)) @ M
            np.minimum(best, (v * v).sum(-1), out=best)
        d = np.sqrt(best)
        k = int(np.argmin(d))
        near = np.full(n, np.inf)
        np.minimum.at(near, iu[0], d)
        np.minimum.at(near, iu[1], d)
        res.append((float(d[k]), (int(iu[0][k]), int(iu[1][k])), int((d <= tol).sum()), near, hist))
    return res


def same(o, off, host):
    for k, (dmin, pair, ncl, near, hist) in enumerate(host):
        ok = (np.isclose(o["min_dist"][k], dmin, rtol=1e-12) and tuple(o["min_pair"][k]) == pair and o["n_close"][k] == ncl
              and np.allclose(o["nearest"][off[k]:off[k + 1]], near, rtol=1e-12) and np.array_equal(o["hist"][k], hist))
        if not ok:
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structure_bench.json"))
    a = ap.parse_args()
    from icsg3d_amd import _lib as L
    from icsg3d_amd import structures as S
    from icsg3d_amd.evaluate import predicted_coordinates
    assert L.device_count() >= 1, "no HIP device visible"
    rng = np.random.default_rng(0)
    res = {"reps": a.reps, "warmup": a.warmup}

    op = {}
    for name, n, lo, hi in (("5-40_x100", 100, 5, 40), ("5-40_x1024", 1024, 5, 40), ("5-40_x16384", 16384, 5, 40),
                            ("2048_x1", 1, 2048, 2048)):
        structs = draw(rng, n, lo, hi, S)
        off, sp, xyz, abc, ang = pack(structs)
        o = S.screen_packed(off, sp, xyz, abc, ang)
        reps = max(3, a.reps // (4 if n > 1000 else 1))
        row = {"structures": n, "atoms": int(off[-1]), "pairs": int(sum(len(s[0]) * (len(s[0]) - 1) // 2 for s in structs)),
               "device_op": timeit(lambda: S.screen_packed(off, sp, xyz, abc, ang), reps, a.warmup)}
        hn = min(n, 1024)                           # the host loop is timed on at most 1 024 structures and scaled
        t0 = time.perf_counter()
        host = host_screen(structs[:hn], S)
        row["host_equal"] = bool(same(o, off, host))
        hreps = 1 if n >= 1024 or hi > 64 else 3
        ht = timeit(lambda: host_screen(structs[:hn], S), hreps, 0)
        row["host_loop"] = dict(ht, structures_timed=hn, median_ms_scaled=ht["median_ms"] * n / hn)
        row["host_over_device"] = row["host_loop"]["median_ms_scaled"] / row["device_op"]["median_ms"]
        op[name] = row
        print(name, json.dumps(row), flush=True)
    res["op"] = op

    # generate.py's per-batch tail on constructed samples
    B, d, eps = 100, 32, 0.25
    structs = draw(rng, B, 5, 40, S)
    l_prime = np.array([s[2] for s in structs])
    dv = (l_prime + 2 * l_prime * 0.25) / d
    mus = [(s[1] + eps * s[2] - dv[i] / 2.0) / dv[i] for i, s in enumerate(structs)]          # voxel-frame centroids
    minmax = np.stack([np.zeros_like(l_prime), 1.5 * l_prime], -1)           # coordinate channels that read back as l_prime
    vol = {"density": rng.random((B, d, d, d)).astype(np.float32), "species": rng.integers(0, 95, (B, d, d, d)).astype(np.uint8),
           "mask": rng.integers(0, 2, (B, d, d, d)).astype(np.uint8)}
    tmp = tempfile.mkdtemp(prefix="structure_bench_")

    def tail(stage):
        out_dir = os.path.join(tmp, "with" if stage else "without")
        for sub in ("densities", "species", "binary", "voxel_params", "coords"):
            os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
        writer = S.ResultsWriter(out_dir, 90, 90, 120) if stage else None
        atoms = [None] * B
        xyz = predicted_coordinates([(s[0], mu) for s, mu in zip(structs, mus)], minmax, eps, d)
        for i in range(B):
            species_sample, mu = structs[i][0], xyz[i]
            coords = np.concatenate([np.array(species_sample, np.float64).reshape(-1, 1), mu], axis=-1)
            np.save(os.path.join(out_dir, "densities", "%d.npy" % i), vol["density"][i])
            np.save(os.path.join(out_dir, "species", "%d.npy" % i), vol["species"][i])
            np.save(os.path.join(out_dir, "binary", "%d.npy" % i), vol["mask"][i])
            np.save(os.path.join(out_dir, "voxel_params", "%d.npy" % i), dv[i])
            np.save(os.path.join(out_dir, "coords", "%d.npy" % i), coords)
            atoms[i] = (species_sample, mu)
        if stage:
            writer.add_batch(range(B), l_prime, atoms)
            return writer.finish()
        return None

    try:
        counts = tail(True)
        # alternate the two arms
        t_without, t_with = [], []
        for _ in range(a.warmup + a.reps):
            for stage, ts in ((False, t_without), (True, t_with)):
                t0 = time.perf_counter()
                tail(stage)
                ts.append(time.perf_counter() - t0)
        tw, ts_ = np.array(t_without[a.warmup:]), np.array(t_with[a.warmup:])
        res["tail"] = {"B": B, "d": d, "counts": counts,
                       "without_stage": {"median_ms": 1e3 * float(np.median(tw)), "min_ms": 1e3 * float(tw.min()), "reps": a.reps},
                       "with_stage": {"median_ms": 1e3 * float(np.median(ts_)), "min_ms": 1e3 * float(ts_.min()), "reps": a.reps},
                       "with_over_without": float(np.median(ts_) / np.median(tw)),
                       "note": "files go to the temporary directory of the box; the networks are not part of the tail"}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
