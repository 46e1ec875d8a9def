"""The confusion matrix on the device: confusion_kernel against a brute-force count, the engine's
accumulator against the running sum of that count over the engine's own predict_labels, and the scripts on top of it.

Every count is an integer: every comparison of counts is array_equal, and no tolerance appears in this file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import confusion_cases as CC
from confusion_ref import confusion_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("u8", "f32", "f64")


def _grid_pairs():
    """pairs after which every lane has made one whole grid-stride pass: threads * pairs per lane * the grid cap"""
    from icsg3d_amd.engine import confusion_grid
    threads, lane_pairs, max_blocks = confusion_grid()
    assert threads % 64 == 0 and lane_pairs == 16 and max_blocks >= 1
    return threads * lane_pairs * max_blocks


def _check_op(t, p, m, ncls):
    from icsg3d_amd.engine import confusion, label_counts
    n = t.size
    ref_m, ref_o, ref_oor = confusion_ref(t, p, m, ncls)
    matrix, occ, oor = confusion(t, p, ncls, mask=m)
    assert matrix.dtype == np.int64 and matrix.shape == (ncls, ncls) and occ.shape == (2, 2)
    np.testing.assert_array_equal(matrix, ref_m)
    np.testing.assert_array_equal(occ, ref_o)
    assert oor == ref_oor and matrix.sum() + oor == n
    # rows against the label counts of the true labels whose prediction is a class id; columns likewise
    p_ok = p < ncls
    rows, rows_oor = label_counts(t[p_ok], ncls)
    np.testing.assert_array_equal(matrix.sum(1), rows)
    t_ok = np.isin(t, np.arange(ncls).astype(t.dtype))
    cols, cols_oor = label_counts(p[t_ok], ncls)
    np.testing.assert_array_equal(matrix.sum(0), cols)
    assert occ.sum() == t_ok.sum() and oor == (~p_ok).sum() + rows_oor == (~t_ok).sum() + cols_oor
    # without a mask: the same matrix from the other instantiation, and no occupancy table
    m2, o2, oor2 = confusion(t, p, ncls)
    np.testing.assert_array_equal(m2, ref_m)
    assert o2 is None and oor2 == ref_oor
    return matrix, oor


# ----------------------------------------------------------------------------------------------------------------------
# 1. the op against the reference
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4099, "two_passes"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ncls", [2, 17, 95, 127])
def test_op_equals_reference(ncls, kind, n):
    if n == "two_passes":
        n = 2 * _grid_pairs() + 3 * 16 + 7           # every lane passes twice, 3 lanes a third time, 7 pairs of ragged tail
    t, p, m = CC.pairs(n, ncls, kind, seed=1000 * ncls + n % 997)
    matrix, oor = _check_op(t, p, m, ncls)
    if n >= 4099:
        assert oor >= 5 and matrix[0, 0] > 0.8 * n and np.count_nonzero(matrix) > min(ncls * ncls, 40) // 2


# ----------------------------------------------------------------------------------------------------------------------
# 2. contention and coverage
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_one_hot_bin(kind):
    """2^22 pairs in ONE bin -- the first and the last of the table: every add of every wave is the ballot's."""
    from icsg3d_amd.engine import confusion
    n, ncls = 1 << 22, 95
    for c in (0, ncls - 1):
        t = np.full(n, c, CC.DTYPES[kind])
        p = np.full(n, c, np.uint8)
        m = np.full(n, 1 if c else 0, np.uint8)
        matrix, occ, oor = confusion(t, p, ncls, mask=m)
        want = np.zeros((ncls, ncls), np.int64)
        want[c, c] = n
        np.testing.assert_array_equal(matrix, want)
        np.testing.assert_array_equal(occ.reshape(-1), [n if k == (3 if c else 0) else 0 for k in range(4)])
        assert oor == 0


@pytest.mark.parametrize("kind", ["u8", "f64"])
def test_every_bin_of_the_largest_table(kind):
    ncls = 127
    n = 4 * ncls * ncls + 5
    i = np.arange(n)
    t = ((i // ncls) % ncls).astype(CC.DTYPES[kind])
    p = (i % ncls).astype(np.uint8)
    m = (i % 3 == 0).astype(np.uint8)
    ref_m, _, _ = confusion_ref(t, p, m, ncls)
    assert ref_m.min() >= 4 and ref_m.shape == (ncls, ncls)             # no zero: all 16 129 bins are hit
    _check_op(t, p, m, ncls)


# ----------------------------------------------------------------------------------------------------------------------
# 3. the engine's accumulator
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncls", [95, 17], ids=["fused_head", "generic_head"])
def test_engine_accumulator(ncls):
    assert CC.check_engine(ncls) == 9 * CC.D ** 3


def test_engine_accumulator_without_the_fused_head():
    """num_classes 95 through GEMM + softmax + labels_kernel, in a fresh process (the switch is read at creation)."""
    script = ("import sys; sys.path[:0] = [%r, %r]; import confusion_cases as CC; print('counted', CC.check_engine(95))"
              % (ROOT, os.path.join(ROOT, "tests")))
    out = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ICSG3D_NO_FUSED_HEAD="1"))
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    assert out.stdout.strip().splitlines()[-1] == "counted %d" % (9 * CC.D ** 3)


@pytest.mark.parametrize("ncls", [95, 17])
def test_accumulator_has_guard_bytes_and_nothing_writes_them(ncls, monkeypatch):
    """ICSG3D_DEBUG_CANARY (read when the engine is created): the accumulator comes from the engine's allocator, so it is
    followed by guard bytes like every buffer, and neither the count nor the forward pass in front of it touches any."""
    monkeypatch.setenv("ICSG3D_DEBUG_CANARY", "1")
    case = CC.engine_case(ncls)
    eng = CC.make_engine(ncls)
    assert eng.check_canaries()[0] == 0
    eng.confusion_open()
    eng.confusion_batch(case["X"], case["lab"], CC.THRESH)
    eng.confusion_step(CC.THRESH)
    r = eng.confusion_read()
    assert r["voxels"] == 2 * case["lab"].size == r["matrix"].sum()
    assert eng.check_canaries() == (0, "")
    eng.close()


# ----------------------------------------------------------------------------------------------------------------------
# 4. nothing is trained
# ----------------------------------------------------------------------------------------------------------------------
def _state(eng):
    return eng.get_weights(), eng.get_optimizer_state()              # every tensor: weights AND BatchNorm moving statistics


def _assert_same_state(a, b):
    (wa, (ma, va, ta)), (wb, (mb, vb, tb)) = a, b
    assert sorted(wa) == sorted(wb) and any(k.endswith("moving_variance") or k.endswith("var") for k in wa)
    for k in wa:
        np.testing.assert_array_equal(wa[k], wb[k], err_msg=k)
    np.testing.assert_array_equal(ma, mb); np.testing.assert_array_equal(va, vb)
    assert ta == tb


@pytest.mark.parametrize("route", ["plain", "class_weights", "communicator"])
def test_nothing_is_trained(route):
    from icsg3d_amd.engine import comm_unique_id
    ncls = 95
    case = CC.engine_case(ncls)
    X, lab = case["X"][:3], case["lab"][:3]
    eng, twin = CC.make_engine(ncls), CC.make_engine(ncls)
    if route == "communicator":
        # The twin stays a plain engine: a single-rank communicator trains to the plain engine's bits
        # (tests/test_gpu_class_weights.py::test_single_rank_communicator_with_the_table), and one RCCL start-up is seconds.
        eng.comm_init(0, 1, comm_unique_id())
        eng.broadcast_state(0)
    for e in (eng, twin):
        if route == "class_weights":
            e.set_class_weights(CC.K.weight_vector(ncls))
        e.train_step(X, lab)                                            # moving statistics and Adam moments worth comparing
    before = _state(eng)
    cw = eng.get_class_weights()
    eng.confusion_open()
    for _ in range(3):
        eng.confusion_batch(X, lab, CC.THRESH)
    r = eng.confusion_read()
    assert r["voxels"] == 3 * lab.size and r["matrix"].sum() == 3 * lab.size
    _assert_same_state(before, _state(eng))
    _assert_same_state(before, _state(twin))
    assert (cw is None) == (route != "class_weights")
    if cw is not None:
        np.testing.assert_array_equal(eng.get_class_weights(), cw)
    m_e, m_t = eng.train_step(X, lab), twin.train_step(X, lab)
    np.testing.assert_array_equal(m_e, m_t)
    assert np.isfinite(m_e).all() and m_e[0] > 0
    _assert_same_state(_state(eng), _state(twin))


# ----------------------------------------------------------------------------------------------------------------------
# 5. train_generator(class_report=True)
# ----------------------------------------------------------------------------------------------------------------------
def test_train_generator_class_report(tmp_path):
    from icsg3d_amd import classreport
    from icsg3d_amd.unet.data import SyntheticUnetGenerator
    from icsg3d_amd.unet.unet import AtomUnet
    d, ncls, bs = 16, 95, 2
    P = CC.engine_case(ncls)["weights"]
    weights = {}
    for flag in (False, True):
        out = tmp_path / ("with" if flag else "without")
        train = SyntheticUnetGenerator(4, bs, (d, d, d), 1, ncls, seed=0)
        val = SyntheticUnetGenerator(4, bs, (d, d, d), 1, ncls, seed=10 ** 6)
        unet = AtomUnet(num_classes=ncls, input_shape=(d, d, d, 1), lr=1e-3, max_batch=bs,
                        weights=str(out / "w" / "unet.best.hdf5"))
        os.makedirs(str(out / "w"))
        unet._set_weights(P)
        unet.train_generator(train, val, epochs=2, output_dir=str(out), class_report=flag)
        weights[flag] = unet._get_weights()
        files = sorted(f for f in os.listdir(str(out)) if "class_report" in f or "confusion" in f)
        if not flag:
            assert files == []
            continue
        assert files == ["class_report_best.csv", "class_report_best.json", "confusion_best.npy"]
        M = np.load(str(out / "confusion_best.npy"))
        assert M.dtype == np.int64 and M.shape == (ncls, ncls) and M.sum() == 4 * d ** 3       # every validation voxel
        counts = sum(np.bincount(val[i][1][0].reshape(-1), minlength=ncls) for i in range(len(val)))
        np.testing.assert_array_equal(M.sum(1), counts)
        rep = json.load(open(str(out / "class_report_best.json")))
        assert rep["support"] == counts.tolist() and rep["voxels"] == 4 * d ** 3 and rep["out_of_range"] == 0
        assert rep["support"] == classreport.report(M)["support"].tolist()
    assert sorted(weights[True]) == sorted(weights[False])
    for k in weights[False]:
        np.testing.assert_array_equal(weights[True][k], weights[False][k], err_msg=k)


# ----------------------------------------------------------------------------------------------------------------------
# 6. eval_unet.py --synthetic, end to end in a child process
# ----------------------------------------------------------------------------------------------------------------------
def test_eval_unet_synthetic(tmp_path):
    sys.path.insert(0, ROOT)
    import eval_unet
    argv = ["--name", "conf_demo", "--synthetic", "14", "--channels", "1", "--d", "16", "--batch_size", "4", "--nclasses", "95"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "eval_unet.py")] + argv, capture_output=True, text=True,
                         timeout=600, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    sdir = tmp_path / "output" / "eval_unet" / "conf_demo"
    assert sorted(os.listdir(str(sdir))) == ["confusion.npy", "report.csv", "report.json", "run.json"]
    # the validation split of 14 grids at 0.8 is 3: no whole batch of 4, one short batch -- and it is counted
    gens = eval_unet.generators(eval_unet.parser().parse_args(argv))
    assert [len(g) * g.batch_size for g in gens] == [0, 3]
    counts = sum(np.bincount(g[i][1][0].reshape(-1), minlength=95) for g in gens for i in range(len(g)))
    assert counts.sum() == 3 * 16 ** 3 and (counts > 0).sum() >= 4
    rep, run = json.load(open(str(sdir / "report.json"))), json.load(open(str(sdir / "run.json")))
    assert rep["support"] == counts.tolist()
    M = np.load(str(sdir / "confusion.npy"))
    np.testing.assert_array_equal(M.sum(1), counts)
    assert run["samples"] == 3 and run["voxels"] == 3 * 16 ** 3 and run["out_of_range"] == 0 and run["ranks"] == 1
    assert "worst recall" in out.stdout and "top confusions" in out.stdout


# ----------------------------------------------------------------------------------------------------------------------
# 7. refusals: an error that names the entry point, and nothing written
# ----------------------------------------------------------------------------------------------------------------------
def _raw_op(t, kind, p, m, n, ncls, matrix, occ, oor, offset=0):
    import ctypes as C
    from icsg3d_amd import _lib as L
    tp = None if t is None else C.c_void_p(t.ctypes.data + offset)
    return L.load().ics_op_confusion(tp, kind, L.u8ptr(p), L.u8ptr(m), n, ncls, L.i64ptr(matrix), L.i64ptr(occ), L.i64ptr(oor))


def test_op_refusals():
    from icsg3d_amd import _lib as L
    from icsg3d_amd._lib import IcsError
    from icsg3d_amd.engine import confusion
    n, ncls = 64, 17
    t, p, m = CC.pairs(n, ncls, "f32", seed=5)
    matrix, occ, oor = np.full((ncls, ncls), -7, np.int64), np.full(4, -7, np.int64), np.full(1, -7, np.int64)
    big = np.full((128, 128), -7, np.int64)
    calls = [("one-hot", (t, 4, p, m, n, ncls, matrix, occ, oor)),
             ("label_kind", (t, 0, p, m, n, ncls, matrix, occ, oor)),
             ("label_kind", (t, 5, p, m, n, ncls, matrix, occ, oor)),
             ("num_classes", (t, 3, p, m, n, 1, big, occ, oor)),
             ("num_classes", (t, 3, p, m, n, 128, big, occ, oor)),
             ("null", (None, 3, p, m, n, ncls, matrix, occ, oor)),
             ("null", (t, 3, None, m, n, ncls, matrix, occ, oor)),
             ("null", (t, 3, p, m, n, ncls, None, occ, oor)),
             ("null", (t, 3, p, m, n, ncls, matrix, occ, None)),
             ("both or neither", (t, 3, p, m, n, ncls, matrix, None, oor)),
             ("both or neither", (t, 3, p, None, n, ncls, matrix, occ, oor))]
    for word, args in calls:
        assert _raw_op(*args) != 0, word
        msg = L.load().ics_last_error().decode()
        assert "ics_op_confusion" in msg and word in msg, (word, msg)
    assert _raw_op(t, 3, p, m, n - 1, ncls, matrix, occ, oor, offset=2) != 0      # float32 labels at an odd half-word
    assert "ics_op_confusion" in L.load().ics_last_error().decode() and "unaligned" in L.load().ics_last_error().decode()
    t64 = t.astype(np.float64)
    assert _raw_op(t64, 2, p, m, n - 1, ncls, matrix, occ, oor, offset=4) != 0
    assert "unaligned" in L.load().ics_last_error().decode()
    for a in (matrix, occ, oor, big):
        assert (a == -7).all()                                          # nothing was written by any refused call
    with pytest.raises(IcsError, match="one-hot"):
        confusion(np.zeros((64, 17), np.float32), np.zeros(64, np.uint8), 17, label_kind="onehot")
    with pytest.raises(ValueError):
        confusion(t, p[:-1], ncls)
    m_ok, o_ok, oor_ok = confusion(t, p, ncls, mask=m)                   # ... and the op still works
    np.testing.assert_array_equal(m_ok, confusion_ref(t, p, m, ncls)[0])


def test_engine_refusals():
    import ctypes as C
    from icsg3d_amd import _lib as L
    from icsg3d_amd._lib import IcsError
    from icsg3d_amd.engine import VaeEngine
    ncls = 17
    case = CC.engine_case(ncls)
    X, lab = case["X"][:2], case["lab"][:2]
    eng = CC.make_engine(ncls)
    lib = L.load()
    for name, call in (("ics_unet_confusion_step", lambda: eng.confusion_step()),
                       ("ics_unet_confusion_batch", lambda: eng.confusion_batch(X, lab)),
                       ("ics_unet_confusion_read", lambda: eng.confusion_read()),
                       ("ics_unet_confusion_reset", lambda: eng.confusion_reset())):
        with pytest.raises(IcsError, match=name + ".*no open accumulator"):
            call()
    eng.confusion_open()
    with pytest.raises(IcsError, match="ics_unet_confusion_step.*no resident batch"):
        eng.confusion_step()
    eng.predict_labels(X)                                               # a resident batch WITHOUT labels
    with pytest.raises(IcsError, match="ics_unet_confusion_step.*without labels"):
        eng.confusion_step()
    eng.confusion_batch(X, lab)
    good = eng.confusion_read()
    assert good["voxels"] == lab.size
    for args in ((None, L.u8ptr(lab)), (L.fptr(X), None)):
        assert lib.ics_unet_confusion_batch(eng._h, args[0], args[1], 2, 0.8) != 0
        assert "ics_unet_confusion_batch" in lib.ics_last_error().decode() and "null" in lib.ics_last_error().decode()
    for batch in (0, CC.MAX_BATCH + 1):
        assert lib.ics_unet_confusion_batch(eng._h, L.fptr(X), L.u8ptr(lab), batch, 0.8) != 0
        assert "ics_unet_confusion_batch" in lib.ics_last_error().decode()
    matrix, occ, one = np.full((ncls, ncls), -7, np.int64), np.full(4, -7, np.int64), np.full(2, -7, np.int64)
    ptr = [L.i64ptr(matrix), L.i64ptr(occ), L.i64ptr(one[:1]), L.i64ptr(one[1:])]
    for k in range(4):
        args = list(ptr)
        args[k] = None
        assert lib.ics_unet_confusion_read(eng._h, *args) != 0
        assert "ics_unet_confusion_read" in lib.ics_last_error().decode() and "null" in lib.ics_last_error().decode()
    assert (matrix == -7).all() and (occ == -7).all() and (one == -7).all()
    for fn in (lib.ics_unet_confusion_open, lib.ics_unet_confusion_reset):
        assert fn(None) != 0 and "null handle" in lib.ics_last_error().decode()
    unet = CC.make_engine(95)
    vae = VaeEngine(unet, in_channels=1, d=CC.D, max_batch=2)
    for name, fn in (("ics_unet_confusion_open", lambda: lib.ics_unet_confusion_open(vae._h)),
                     ("ics_unet_confusion_reset", lambda: lib.ics_unet_confusion_reset(vae._h)),
                     ("ics_unet_confusion_step", lambda: lib.ics_unet_confusion_step(vae._h, 0.8)),
                     ("ics_unet_confusion_batch", lambda: lib.ics_unet_confusion_batch(vae._h, L.fptr(X), L.u8ptr(lab), 2, 0.8)),
                     ("ics_unet_confusion_read", lambda: lib.ics_unet_confusion_read(vae._h, *ptr))):
        assert fn() != 0
        assert name in lib.ics_last_error().decode() and "U-Net engine is required" in lib.ics_last_error().decode()
    assert (matrix == -7).all() and (occ == -7).all() and (one == -7).all()
    after = eng.confusion_read()                                        # the accumulator is what it was
    np.testing.assert_array_equal(after["matrix"], good["matrix"])
    np.testing.assert_array_equal(after["occupancy"], good["occupancy"])
    assert after["voxels"] == good["voxels"] and after["out_of_range"] == good["out_of_range"]
