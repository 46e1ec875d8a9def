"""The atom score without a GPU: the rule's two forms against each other (sorted greedy = mutual-best rounds), the
restated tallies on cases small enough to do by hand, icsg3d_amd/atomreport.py against the explicit-loop restatement in
tests/atom_score_ref.py, its files read back, the rank sum with gloo at world size 2 and eval_unet.py's new flags.
Counts compare with array_equal; the derived ratios are a few fp64 operations and are held to rtol 1e-12."""
import csv
import json
import os
import socket
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import atom_score_cases as AC
import atom_score_ref as AR
from icsg3d_amd import atomreport, atomscore

RTOL = 1e-12


# ----------------------------------------------------------------------------------------------------------------------
# 1. the rule: sorted greedy equals mutual-best rounds
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol2", [1.0, 2.25, 4.0, 9.0])
@pytest.mark.parametrize("kind", ["generic", "lattice"])
def test_sorted_greedy_equals_mutual_best_rounds(kind, tol2):
    rng = np.random.default_rng(int(tol2 * 100) + (kind == "lattice"))
    matched = rounds_seen = 0
    for n in range(13):
        for m in (0, 1, 5, 12, (n * 7) % 13):
            if kind == "generic":
                t, p = rng.uniform(0, 2, (n, 3)), rng.uniform(0, 2, (m, 3))        # dense: picks collide
            else:
                t, p = AC.lattice_sample(n, m, rng, box=3)             # 27 sites: coincident points on both sides
            a = AR.greedy_sorted(t, p, tol2)
            b, rounds = AR.mutual_best(t, p, tol2)
            np.testing.assert_array_equal(a, b)
            used = a[a >= 0]
            assert len(set(used.tolist())) == len(used) and rounds <= min(n, m)
            matched += len(used)
            rounds_seen = max(rounds_seen, rounds)
    assert matched > 50 and rounds_seen >= 2


def test_the_chain_takes_one_round_per_pair():
    t, p = AC.chain(64)
    match, rounds = AR.mutual_best(t, p, 1.5 * 1.5)
    assert rounds == 64 and (match >= 0).all()
    np.testing.assert_array_equal(match, AR.greedy_sorted(t, p, 1.5 * 1.5))


def test_strictness_and_planted_tallies_of_the_restatement():
    t, p = np.zeros((1, 3)), np.array([[3.0, 4.0, 0.0]])
    assert AR.greedy_sorted(t, p, 25.0)[0] == -1                        # d2 == tol2 exactly: not admissible
    assert AR.greedy_sorted(t, p, np.nextafter(5.0, 6.0) ** 2)[0] == 0
    # two predictions next to one true atom: the nearer one is matched, the other is a dup; and the reverse
    o, match, st, ds = AR.score_sample([[0, 0, 0]], [4], [[1, 0, 0], [0.5, 0, 0]], [4, 2], 6, 2.0)
    assert match.tolist() == [1] and st.tolist() == [1, 2, 1, 0, 1, 0] and ds == 0.5
    assert o["matrix"][4, 2] == 1 and o["matrix"][6, 4] == 1 and o["matrix"].sum() == 2 and o["dup"].tolist() == [0, 0, 0, 0, 1, 0]
    assert o["dist_q"][4] == 1 << 19 and o["dist2_q"][4] == 1 << 18 and o["hist"][4] == 1
    assert o["totals"].tolist() == [1, 0, 0, 1, 2, 1, 1, 0]
    o, match, st, _ = AR.score_sample([[1, 0, 0], [0.5, 0, 0]], [1, 3], [[0, 0, 0]], [3], 6, 2.0)
    assert match.tolist() == [-1, 0] and st.tolist() == [2, 1, 1, 1, 0, 1]
    assert o["matrix"][1, 6] == 1 and o["matrix"][3, 3] == 1 and o["shadowed"].tolist() == [0, 1, 0, 0, 0, 0]
    o, _, st, ds = AR.score_sample(np.zeros((0, 3)), [], np.zeros((0, 3)), [], 2, 2.0)
    assert o["totals"].tolist() == [1, 0, 1, 0, 0, 0, 0, 1] and st.tolist() == [0] * 6 and ds == 0.0     # empty: perfect
    o, _, st, ds = AR.score_sample([[0, 0, 0]], [1], np.zeros((0, 3)), [], 2, 2.0, failed=True)
    assert o["totals"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0] and o["matrix"].sum() == 0 and np.isnan(ds)


# ----------------------------------------------------------------------------------------------------------------------
# 2. the report
# ----------------------------------------------------------------------------------------------------------------------
def _tallies():
    rng = np.random.default_rng(23)
    rand = AC.random_tallies(17, rng)
    holes = AC.random_tallies(9, rng)
    holes["matrix"][3, :] = 0                                           # no true atom of species 3
    holes["matrix"][:, 5] = 0                                           # species 5 never predicted
    holes["matrix"][7, :] = 0
    holes["matrix"][:, 7] = 0                                           # neither
    for k in ("dist_q", "dist2_q", "shadowed"):
        holes[k][[3, 7]] = 0
    perfect = atomscore.empty_tallies(5)
    perfect["matrix"][np.arange(5), np.arange(5)] = [4, 0, 9, 1, 2]
    perfect["totals"][:] = [6, 0, 6, 16, 16, 16, 0, 1]
    missed = atomscore.empty_tallies(4)
    missed["matrix"][:4, 4] = [3, 1, 0, 8]
    missed["totals"][:] = [5, 0, 0, 12, 0, 0, 12, 0]
    return {"random17": rand, "holes": holes, "all_perfect": perfect, "all_missed": missed}


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    np.testing.assert_allclose(a[~np.isnan(a)], b[~np.isnan(b)], rtol=RTOL, atol=0)


@pytest.mark.parametrize("name", sorted(_tallies()))
def test_report_equals_the_explicit_loops(name):
    t = _tallies()[name]
    r, ref = atomreport.report(t, tol=2.0, top=7), AR.report_ref(t)
    for key in ("true_atoms", "pred_atoms", "detected", "typed"):
        assert r[key].dtype == np.int64
        np.testing.assert_array_equal(r[key], ref[key])
        assert r["overall"][key] == ref["overall"][key]
    for key in atomreport.RATIOS:
        _same(r[key], ref[key])
        _same(r["overall"][key], ref["overall"][key])
    for key in ("perfect_share", "mean_abs_dn"):
        _same(r["overall"][key], ref["overall"][key])
    for key in ("failed", "samples", "missed", "spurious", "dup", "shadowed"):
        assert r["overall"][key] == ref["overall"][key]
    assert [(e["true"], e["predicted"], e["count"]) for e in r["top_confusions"]] == ref["top_confusions"][:7]
    np.testing.assert_array_equal(r["hist"], t["hist"])
    np.testing.assert_array_equal(r["hist_edges"], np.arange(17) * 0.125)
    assert "worst typed recall" in atomreport.table(r) and "top atom confusions" in atomreport.table(r)


def test_zero_denominators_and_the_two_extremes():
    T = _tallies()
    h = atomreport.report(T["holes"])
    assert np.isnan(h["typed_recall"][3]) and np.isnan(h["precision"][5]) and h["typed_recall"][5] == 0.0
    assert all(np.isnan(h[k][7]) for k in atomreport.RATIOS)
    p = atomreport.report(T["all_perfect"])
    assert p["overall"]["typed_recall"] == 1.0 and p["overall"]["precision"] == 1.0 and p["overall"]["perfect_share"] == 1.0
    assert p["overall"]["mean_error"] == 0.0 and p["top_confusions"] == [] and np.isnan(p["typed_recall"][1])
    m = atomreport.report(T["all_missed"])
    assert m["overall"]["detection_recall"] == 0.0 and np.isnan(m["overall"]["precision"]) and np.isnan(m["overall"]["mean_error"])
    assert m["overall"]["missed"] == 12 and m["overall"]["mean_abs_dn"] == 12 / 5 and m["top_confusions"][0]["predicted"] == 4
    for bad in ({}, dict(T["all_missed"], matrix=np.zeros((3, 4), np.int64)), dict(T["all_missed"], dup=np.zeros(3, np.int64)),
                dict(T["all_missed"], matrix=-np.ones((5, 5), np.int64)), dict(T["all_missed"], hist=np.zeros(16))):
        with pytest.raises(ValueError):
            atomreport.report(bad)


def test_write_and_read_back(tmp_path):
    t = _tallies()["holes"]
    names = ["none0"] + ["El%d" % i for i in range(1, 9)]
    r = atomreport.write(str(tmp_path), t, tol=2.0, names=names, top=5, extra={"thresh": 0.8})
    assert sorted(os.listdir(str(tmp_path))) == ["atom_confusion.npy", "atom_report.csv", "atom_report.json"]
    back = np.load(str(tmp_path / "atom_confusion.npy"))
    assert back.dtype == np.int64
    np.testing.assert_array_equal(back, t["matrix"])
    text = open(str(tmp_path / "atom_report.json")).read()
    assert "NaN" not in text and "Infinity" not in text
    js = json.loads(text)
    assert js["thresh"] == 0.8 and js["names"] == names and js["true_atoms"] == r["true_atoms"].tolist()
    assert js["tallies"]["dist_q"] == t["dist_q"].tolist() and js["tallies"]["totals"] == t["totals"].tolist()
    assert js["typed_recall"][3] is None and js["precision"][5] is None and len(js["top_confusions"]) == 5
    assert js["overall"]["failed"] == 3 and js["hist"] == t["hist"].tolist() and len(js["hist_edges"]) == 17
    rows = list(csv.reader(open(str(tmp_path / "atom_report.csv"), newline="")))
    assert rows[0] == ["class", "name"] + list(atomreport.COUNTS) + list(atomreport.RATIOS) and len(rows) == 10
    for c, row in enumerate(rows[1:]):
        assert row[:2] == [str(c), names[c]] and [int(v) for v in row[2:8]] == [int(r[k][c]) for k in atomreport.COUNTS]
        for key, cell in zip(atomreport.RATIOS, row[8:]):
            assert (cell == "") == bool(np.isnan(r[key][c]))
            assert cell == "" or float(cell) == r[key][c]
    assert rows[8][8:] == [""] * 6


# ----------------------------------------------------------------------------------------------------------------------
# 3. the rank sum and the flags
# ----------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_tallies(rank):
    t = AC.random_tallies(6, np.random.default_rng(200 + rank), scale=2 ** 34)
    return [t[k] for k in atomscore.TALLIES]


def _reduce_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        out = atomreport.reduce_over_ranks(dist, _rank_tallies(rank))
        np.savez(os.path.join(out_dir, "sum%d.npz" % rank), *out)
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_tallies_sum_over_ranks_with_gloo(tmp_path):
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    mp.spawn(_reduce_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    want = [a + b for a, b in zip(_rank_tallies(0), _rank_tallies(1))]
    for rank in range(world):
        got = np.load(str(tmp_path / ("sum%d.npz" % rank)))
        for k, w in enumerate(want):
            assert got["arr_%d" % k].dtype == np.int64 and got["arr_%d" % k].shape == w.shape
            np.testing.assert_array_equal(got["arr_%d" % k], w)
    summed = dict(zip(atomscore.TALLIES, want))
    assert atomreport.report(summed)["overall"]["true_atoms"] == int(want[0][:6].sum())


def test_eval_unet_atom_flags():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import eval_unet
    a = eval_unet.parser().parse_args([])
    assert (a.atoms, a.atom_tol, a.min_voxels, a.max_atoms) == (False, 2.0, 3, 512)
    b = eval_unet.parser().parse_args(["--atoms", "--atom_tol", "1.5", "--min_voxels", "0", "--max_atoms", "64"])
    assert (b.atoms, b.atom_tol, b.min_voxels, b.max_atoms) == (True, 1.5, 0, 64)
    assert set(eval_unet.ATOM_FLAGS) == {"atoms", "atom_tol", "min_voxels", "max_atoms"}
