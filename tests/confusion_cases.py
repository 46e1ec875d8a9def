"""Shared builders of the confusion tests (tests/test_gpu_confusion.py, in its own process and in a child process with
another head route): (true, predicted, mask) arrays with planted invalid values, and the engine case -- a U-Net with a
confident head whose predictions spread over many classes.  Builders cache; nothing is modified after it is built."""
import numpy as np

import class_weight_cases as K
from confusion_ref import confusion_ref
from oracle import numpy_ref as R
from oracle.confident_head import saturate_head

DTYPES = {"u8": np.uint8, "f32": np.float32, "f64": np.float64}
D, MAX_BATCH, THRESH = 16, 5, 0.8
BATCHES = ((0, 3), (0, 5), (4, 5))            # sample ranges: batches of 3, 5 and 1


def pairs(n, ncls, kind, seed):
    """98 % background in the true labels, predictions right nine times in ten, a mask that mostly follows the labels;
    then values that are no class id: NaN, -1, 2.5 and ncls in float labels (ncls, 255, 128 in uint8 ones), ncls and 255
    in the predictions -- as many of them as fit into half of the array."""
    rng = np.random.default_rng(seed)
    dtype = DTYPES[kind]
    t = np.where(rng.uniform(size=n) < 0.98, 0, rng.integers(0, ncls, size=n))
    p = np.where(rng.uniform(size=n) < 0.9, t, rng.integers(0, ncls, size=n)).astype(np.uint8)
    m = np.where(rng.uniform(size=n) < 0.95, t != 0, t == 0).astype(np.uint8) * rng.integers(1, 256, size=n).astype(np.uint8)
    t = t.astype(dtype)
    bad_t = [ncls, 255, 128] if kind == "u8" else [np.nan, -1.0, 2.5, float(ncls)]
    bad_p = [ncls, 255]
    at = rng.permutation(n)[:min(n // 2, len(bad_t) + len(bad_p) + 1)]
    for k, pos in enumerate(at):
        if k < len(bad_t):
            t[pos] = bad_t[k]
        elif k < len(bad_t) + len(bad_p):
            p[pos] = bad_p[k - len(bad_t)]
        else:
            t[pos], p[pos] = bad_t[0], bad_p[0]                          # both invalid: still one pair out of range
    return t, p, m


_engine_cases = {}


def engine_case(ncls):
    """dict(weights, X float32 (5, 16, 16, 16, 1), lab uint8): an oracle U-Net (Glorot trunk, seed 1) with the confident
    head of oracle/confident_head.py fitted to the batch.  Asserted here, on the CPU in fp64: the argmax of the oracle's
    forward takes at least 8 classes on at least 4 voxels each with a gap of 1e-3 to the runner-up (fp32 cannot turn
    those), the true labels hold at least 8 classes, and the sigmoid crosses the threshold somewhere but not everywhere."""
    if ncls in _engine_cases:
        return _engine_cases[ncls]
    X, lab = K.unet_batch(MAX_BATCH, D, ncls)
    orc = R.UnetOracle(in_ch=1, num_classes=ncls, seed=1)
    saturate_head(orc, X, lab, training=False)
    soft, sig = orc.forward(X, training=False)
    top2 = np.sort(soft, -1)[..., -2:]
    firm = (top2[..., 1] - top2[..., 0]) > 1e-3
    _, counts = np.unique(soft.argmax(-1)[firm], return_counts=True)
    assert (counts >= 4).sum() >= 8, counts
    assert np.unique(lab).size >= 8
    mask = sig[..., 0] >= THRESH
    assert 0.005 < mask.mean() < 0.5
    case = dict(weights={**orc.P, **orc.S}, X=X.astype(np.float32), lab=lab)
    _engine_cases[ncls] = case
    return case


def make_engine(ncls, **kw):
    from icsg3d_amd.engine import UnetEngine
    eng = UnetEngine(in_channels=1, num_classes=ncls, d=D, max_batch=MAX_BATCH, lr=1e-3, **kw)
    eng.set_weights(engine_case(ncls)["weights"])                        # set_tensor per tensor, the head's included
    return eng


def _acc_equal(r, matrix, occ, oor, voxels):
    np.testing.assert_array_equal(r["matrix"], matrix)
    np.testing.assert_array_equal(r["occupancy"], occ)
    assert r["out_of_range"] == oor and r["voxels"] == voxels


def check_engine(ncls):
    """Section 3 of the GPU tests for one class count on whatever head route the process's environment selects."""
    from icsg3d_amd.monitor import resident_slices
    case = engine_case(ncls)
    X, lab = case["X"], case["lab"]
    eng = make_engine(ncls)
    pred = [eng.predict_labels(X[a:b], THRESH) for a, b in BATCHES]
    # preconditions, before any comparison: a degenerate prediction would compare zeros with zeros
    sp_all = np.concatenate([sp.reshape(-1) for sp, _ in pred])
    mk_all = np.concatenate([mk.reshape(-1) for _, mk in pred])
    assert np.unique(pred[1][0]).size >= 8, np.unique(pred[1][0])
    assert np.unique(lab).size >= 8 and sp_all.max() < ncls
    assert 0 < mk_all.mean() < 1 and set(np.unique(mk_all)) <= {0, 1}
    eng.confusion_open()
    _acc_equal(eng.confusion_read(), np.zeros((ncls, ncls), np.int64), np.zeros((2, 2), np.int64), 0, 0)
    tot_m, tot_o, vox = np.zeros((ncls, ncls), np.int64), np.zeros((2, 2), np.int64), 0
    for (a, b), (sp, mk) in zip(BATCHES, pred):
        m, o, oor = confusion_ref(lab[a:b], sp, mk, ncls)
        assert oor == 0
        tot_m, tot_o, vox = tot_m + m, tot_o + o, vox + lab[a:b].size
        eng.confusion_batch(X[a:b], lab[a:b], THRESH)
        _acc_equal(eng.confusion_read(), tot_m, tot_o, 0, vox)
    assert (tot_m > 0).sum() >= 16 and np.count_nonzero(tot_m - np.diag(np.diag(tot_m))) >= 4      # off-diagonal entries too
    _acc_equal(eng.confusion_read(), tot_m, tot_o, 0, vox)                # read twice: the same, nothing reset
    # the step on a resident batch equals the batch call
    a, b = BATCHES[0]
    m, o, _ = confusion_ref(lab[a:b], pred[0][0], pred[0][1], ncls)
    eng.upload_batch(X[a:b], lab[a:b])
    eng.confusion_step(THRESH)
    _acc_equal(eng.confusion_read(), tot_m + m, tot_o + o, 0, vox + lab[a:b].size)
    # ... and leaves the species where the slice renderer finds them
    drawn = resident_slices(eng, 1, b - a)
    assert drawn.shape == (b - a, D, D, 4) and np.isfinite(drawn).all()
    eng.predict_resident(labels_only=True, thresh=THRESH)
    np.testing.assert_array_equal(resident_slices(eng, 1, b - a), drawn)
    eng.confusion_reset()
    _acc_equal(eng.confusion_read(), np.zeros((ncls, ncls), np.int64), np.zeros((2, 2), np.int64), 0, 0)
    eng.confusion_step(THRESH)                                            # after a reset it counts from zero
    _acc_equal(eng.confusion_read(), m, o, 0, lab[a:b].size)
    eng.close()
    return int(tot_m.sum())
