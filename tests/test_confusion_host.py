"""icsg3d_amd/classreport.py against the plain-loop restatement in tests/confusion_ref.py, its files read back, the sum
over ranks with gloo at world size 2, and eval_unet.py's parser -- no GPU.  Counts compare with array_equal; the derived
ratios are a few fp64 operations and are held to rtol 1e-12."""
import csv
import json
import math
import os
import socket
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from confusion_ref import confusion_ref, report_ref
from icsg3d_amd import classreport

RTOL = 1e-12


def _cases():
    rng = np.random.default_rng(17)
    rand = rng.integers(0, 1000, size=(17, 17))
    rand[0, 0] = 10 ** 7                                                  # a dominant background
    holes = rng.integers(1, 50, size=(9, 9))
    holes[3, :] = 0                                                       # an empty row: no support
    holes[:, 5] = 0                                                       # an empty column: never predicted
    holes[7, :] = 0
    holes[:, 7] = 0                                                       # neither
    return {"random17": rand.astype(np.int64), "holes": holes.astype(np.int64),
            "diagonal": np.diag(np.arange(1, 12)).astype(np.int64), "two": np.array([[5, 2], [1, 0]], np.int64),
            "background_only": np.diag([9, 0, 0]).astype(np.int64)}


def _same(a, b):
    """equal, NaN where and only where the reference is NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    np.testing.assert_allclose(a[~np.isnan(a)], b[~np.isnan(b)], rtol=RTOL, atol=0)


@pytest.mark.parametrize("name", sorted(_cases()))
def test_report_equals_the_plain_loops(name):
    M = _cases()[name]
    occ = np.array([[M[0, 0], 3], [2, M.sum() - M[0, 0]]], np.int64)
    r, ref = classreport.report(M, occ, top=7), report_ref(M, occ, top=7)
    for key in ("support", "predicted", "tp"):
        assert r[key].dtype == np.int64
        np.testing.assert_array_equal(r[key], [c[key] for c in ref["per_class"]])
    for key in ("precision", "recall", "f1", "iou"):
        _same(r[key], [c[key] for c in ref["per_class"]])
        _same(r["macro_" + key], ref["macro_" + key])
        _same(r["weighted_" + key], ref["weighted_" + key])
    _same(r["accuracy"], ref["accuracy"])
    _same(r["accuracy_non_background"], ref["accuracy_non_background"])
    assert r["voxels"] == ref["voxels"] == int(M.sum())
    assert [(e["true"], e["predicted"], e["count"]) for e in r["top_confusions"]] == \
           [(e["true"], e["predicted"], e["count"]) for e in ref["top_confusions"]]
    _same([e["share_of_row"] for e in r["top_confusions"]], [e["share_of_row"] for e in ref["top_confusions"]])
    assert len(r["top_confusions"]) <= 7 and all(e["count"] > 0 and e["true"] != e["predicted"] for e in r["top_confusions"])
    for key in ("tn", "fp", "fn", "tp"):
        assert r["occupancy"][key] == ref["occupancy"][key]
    for key in ("precision", "recall", "f1"):
        _same(r["occupancy"][key], ref["occupancy"][key])


def test_zero_denominators_are_nan():
    r = classreport.report(_cases()["holes"])
    assert np.isnan(r["recall"][3]) and np.isnan(r["precision"][5]) and not np.isnan(r["recall"][5])
    assert all(np.isnan(r[k][7]) for k in ("precision", "recall", "f1", "iou"))
    assert r["support"][3] == 0 and r["predicted"][5] == 0
    b = classreport.report(_cases()["background_only"], np.zeros((2, 2), np.int64))
    assert np.isnan(b["accuracy_non_background"]) and b["accuracy"] == 1.0 and b["top_confusions"] == []
    assert all(np.isnan(b["occupancy"][k]) for k in ("precision", "recall", "f1"))


def test_macro_averages_skip_classes_without_support():
    M = _cases()["holes"]
    r = classreport.report(M)
    have = [c for c in range(9) if M[c].sum() > 0]
    assert len(have) == 7
    assert math.isclose(r["macro_recall"], sum(M[c, c] / M[c].sum() for c in have) / len(have), rel_tol=RTOL)
    # a class that is predicted but never true (column 3 is not empty) drags no average down
    assert M[:, 3].sum() > 0 and r["precision"][3] == 0.0
    grown = np.zeros((10, 10), np.int64)
    grown[:9, :9] = M                                                     # one more class that never occurs
    g = classreport.report(grown)
    for key in ("macro_precision", "macro_recall", "macro_f1", "macro_iou", "weighted_recall", "weighted_f1"):
        assert g[key] == r[key], key
    # class 5 has support and no prediction: out of the precision mean, in the recall mean with a recall of 0
    assert math.isclose(r["macro_precision"], np.nanmean([r["precision"][c] for c in have]), rel_tol=RTOL)
    assert r["recall"][5] == 0.0


def test_bad_matrices_are_refused():
    for bad in (np.zeros((3, 4), np.int64), np.zeros((1, 1), np.int64), np.zeros((3, 3)), -np.eye(3, dtype=np.int64)):
        with pytest.raises(ValueError):
            classreport.report(bad)
    with pytest.raises(ValueError):
        classreport.report(np.eye(3, dtype=np.int64), names=["a", "b"])


def test_write_and_read_back(tmp_path):
    M = _cases()["holes"]
    occ = np.array([[100, 0], [0, 0]], np.int64)
    names = ["bg"] + ["El%d" % i for i in range(1, 9)]
    r = classreport.write(str(tmp_path), M, occ, names=names, top=5, extra={"thresh": 0.8})
    assert sorted(os.listdir(str(tmp_path))) == ["confusion.npy", "report.csv", "report.json"]
    back = np.load(str(tmp_path / "confusion.npy"))
    assert back.dtype == np.int64
    np.testing.assert_array_equal(back, M)
    text = open(str(tmp_path / "report.json")).read()
    assert "NaN" not in text and "Infinity" not in text
    js = json.loads(text)
    assert js["thresh"] == 0.8 and js["names"] == names and js["support"] == r["support"].tolist()
    assert js["recall"][3] is None and js["precision"][5] is None and js["occupancy"]["precision"] is None
    for key in ("precision", "recall", "f1", "iou"):
        for c in range(9):
            assert (js[key][c] is None) == bool(np.isnan(r[key][c]))
            assert js[key][c] is None or js[key][c] == r[key][c]
    assert js["top_confusions"][0]["count"] == r["top_confusions"][0]["count"] and len(js["top_confusions"]) == 5
    rows = list(csv.reader(open(str(tmp_path / "report.csv"), newline="")))
    assert rows[0] == ["class", "name", "support", "predicted", "tp", "precision", "recall", "f1", "iou"] and len(rows) == 10
    for c, row in enumerate(rows[1:]):
        assert row[:2] == [str(c), names[c]] and [int(v) for v in row[2:5]] == [r["support"][c], r["predicted"][c], r["tp"][c]]
        for key, cell in zip(("precision", "recall", "f1", "iou"), row[5:]):
            assert (cell == "") == bool(np.isnan(r[key][c]))
            assert cell == "" or float(cell) == r[key][c]                 # repr round-trips an fp64
    assert rows[4][5:] == ["0.0", "", "0.0", "0.0"] and rows[8][5:] == ["", "", "", ""]
    classreport.write(str(tmp_path), M, stem="_best", report_name="class_report")
    assert {"confusion_best.npy", "class_report_best.csv", "class_report_best.json"} <= set(os.listdir(str(tmp_path)))
    assert "worst recall" in classreport.table(r) and "El1" in classreport.table(r)


def test_reference_counts_what_it_says():
    """the brute-force count itself, on a case small enough to do by hand"""
    t = np.array([0, 1, 2, np.nan, -1.0, 2.5, 3.0, 1, 0], np.float32)
    p = np.array([0, 1, 1, 0, 0, 0, 0, 3, 255], np.uint8)
    m = np.array([0, 9, 0, 1, 1, 1, 1, 1, 1], np.uint8)
    M, occ, oor = confusion_ref(t, p, m, 3)
    np.testing.assert_array_equal(M, [[1, 0, 0], [0, 1, 0], [0, 1, 0]])
    assert oor == 6
    np.testing.assert_array_equal(occ, [[1, 1], [1, 2]])                  # over t in {0, 1, 2, 1, 0}: the valid true labels


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_arrays(rank):
    rng = np.random.default_rng(100 + rank)
    return [rng.integers(0, 2 ** 40, size=(5, 5)), rng.integers(0, 2 ** 40, size=(2, 2)), np.array([rank + 1, 7])]


def _reduce_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        mine = _rank_arrays(rank)
        keep = [a.copy() for a in mine]
        out = classreport.reduce_over_ranks(dist, mine)
        assert all(np.array_equal(a, b) for a, b in zip(mine, keep))       # the inputs are left alone
        np.savez(os.path.join(out_dir, "sum%d.npz" % rank), *out)
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_reduce_over_ranks_with_gloo(tmp_path):
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    mp.spawn(_reduce_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    want = [a + b for a, b in zip(_rank_arrays(0), _rank_arrays(1))]
    for rank in range(world):
        got = np.load(str(tmp_path / ("sum%d.npz" % rank)))
        for k, w in enumerate(want):
            assert got["arr_%d" % k].dtype == np.int64 and got["arr_%d" % k].shape == w.shape
            np.testing.assert_array_equal(got["arr_%d" % k], w)           # sums above 2^32: nothing went through fp32
    alone = classreport.reduce_over_ranks(None, _rank_arrays(0))
    assert all(np.array_equal(a, b) and a.dtype == np.int64 for a, b in zip(alone, _rank_arrays(0)))


def test_eval_unet_parser_defaults():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import eval_unet
    a = eval_unet.parser().parse_args([])
    assert (a.which, a.thresh, a.top) == ("val", 0.8, 20)
    # the shared flags keep train_unet.py's defaults
    assert (a.name, a.samples, a.d, a.batch_size, a.nrot, a.nclasses, a.split, a.channels, a.synthetic, a.gpus) == \
           (None, 20000, 32, 10, 10, 95, 0.8, 4, 0, 0)
    b = eval_unet.parser().parse_args(["--which", "train", "--dim", "16", "--thresh", "0.5", "--top", "3"])
    assert (b.which, b.d, b.thresh, b.top) == ("train", 16, 0.5, 3)
    with pytest.raises(SystemExit):
        eval_unet.parser().parse_args(["--which", "test"])
