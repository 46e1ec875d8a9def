"""Per-class loss weights on the device: the CW instantiations of head_kernel / head_fused_kernel
against the fp64 oracle with a weight VECTOR, the table through every step route of the engine, and label_counts_kernel.

Weight vectors (class_weight_cases.weight_vector): multiples of 1/64 in [0.25, 8], w[0] = 0 and one further present class at
0.  Bounds: those of tests/test_gpu_widths.py, whose derivations carry over with w[label] in place of w."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import class_weight_cases as K
from oracle import numpy_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_KEYS = ("tp", "predicted", "wr_tp", "wr_possible", "voxels")
HEAD_M = 1037                  # not a multiple of 4: a ragged last four-voxel wave
FUSED_M = 16 * 2085            # 2085 tiles > 4 * 512: some waves walk two tiles, some one (grid stride + x prefetch)


def _check_head(case, fused):
    """Losses, the seven sums and dz of the weighted call against the fp64 reference; returns (dz, metrics, sums)."""
    from icsg3d_amd.engine import unet_head
    head, w, lab = K.head_args(case), case["w"], case["lab"]
    M, ncls = lab.size, w.size
    _, m, sums = unet_head(*head, mode=1, fused=fused, class_weights=w)
    print("ncls %d M %d fused %s: device %s, reference lsoft %.6f lsig %.6f" % (ncls, M, fused, m, case["lsoft"], case["lsig"]))
    np.testing.assert_allclose(m[1], case["lsoft"], rtol=1e-5)
    np.testing.assert_allclose(m[2], case["lsig"], rtol=1e-5)
    np.testing.assert_allclose(m[0], case["lsoft"] + case["lsig"], rtol=1e-5)
    np.testing.assert_allclose(sums["sum_lsoft"], case["lsoft"] * M, rtol=1e-5)
    np.testing.assert_allclose(sums["sum_lsig"], case["lsig"] * M, rtol=1e-5)
    # the weights touch neither the sigmoid loss nor a count: the unweighted call on the same inputs gives the same
    _, m_u, sums_u = unet_head(*head, mode=1, fused=fused)
    assert sums["sum_lsig"] == sums_u["sum_lsig"] and m[2] == m_u[2]
    for k in COUNT_KEYS:
        assert sums[k] == sums_u[k], (k, sums[k], sums_u[k])
    assert sums["voxels"] == M and sums["tp"] > 100 and sums["wr_tp"] > 0
    assert m[3] == m_u[3] and m[4] == m_u[4]
    assert abs(m_u[1] - m[1]) > 0.1 * m[1]                               # ... and they do touch the softmax loss
    dz, m2, _ = unet_head(*head, mode=2, fused=fused, class_weights=w)
    np.testing.assert_array_equal(m2, m)
    # dz = w[lab] (p - y) / M: the bound of test_head_kernel_at_other_class_counts (2e-6 of the probabilities + three
    # fp32 roundings < 2.5e-6 of the tensor's maximum)
    err = np.abs(dz[:, :ncls] - case["dzs"]).max() / np.abs(case["dzs"]).max()
    err_g = np.abs(dz[:, ncls] - case["dzg"]).max() / np.abs(case["dzg"]).max()
    print("  dz error %.2e (soft) %.2e (sig) of the tensor's maximum" % (err, err_g))
    assert err <= 2.5e-6 and err_g <= 2.5e-6
    # a class with weight 0: an exactly zero soft row, whatever the probabilities
    assert case["zero_rows"].sum() > 0 and not dz[case["zero_rows"], :ncls].any()
    assert np.abs(dz[~case["zero_rows"], :ncls]).max(-1).min() > 0
    return dz, m, sums


@pytest.mark.parametrize("ncls", [2, 17, 95, 127])
def test_weighted_head_generic_kernel(ncls):
    """1. GEMM + head_kernel<true> at four class counts."""
    _check_head(K.head_case(ncls, HEAD_M), fused=False)


def test_weighted_head_fused_kernel():
    """2. head_fused_kernel<true> on more tiles than waves; fused and generic agree."""
    case = K.head_case(95, FUSED_M)
    dz_f, m_f, s_f = _check_head(case, fused=True)
    dz_g, m_g, s_g = _check_head(case, fused=False)
    # each is within 2.5e-6 of the tensor's maximum / 1e-5 of the losses from the fp64 reference (above): twice that between them
    assert np.abs(dz_f - dz_g).max() <= 5e-6 * np.abs(case["dzs"]).max()
    np.testing.assert_allclose(m_f[:3], m_g[:3], rtol=2e-5)
    for k in COUNT_KEYS:
        assert s_f[k] == s_g[k], k


@pytest.mark.parametrize("c", [95.0, 3.5])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "generic"])
def test_constant_table_equals_scalar_op_level(fused, c):
    """3a. class_weights = full(ncls, c) against loss_weight = c: the same bits out of both instantiations."""
    from icsg3d_amd.engine import unet_head
    case = K.head_case(95, FUSED_M if fused else HEAD_M)
    head = K.head_args(case)
    for mode in (1, 2):
        out_s, m_s, sums_s = unet_head(*head, mode=mode, fused=fused, loss_weight=c)
        out_t, m_t, sums_t = unet_head(*head, mode=mode, fused=fused, class_weights=np.full(95, c))
        np.testing.assert_array_equal(m_t, m_s)
        assert sums_t == sums_s
        if mode == 2:
            np.testing.assert_array_equal(out_t, out_s)
            assert np.abs(out_s).max() > 0


def _engine(ncls, B, w=None, d=16, lr=1e-3, loss_weight=0.0, seed=1):
    from icsg3d_amd.engine import UnetEngine
    orc = R.UnetOracle(in_ch=1, num_classes=ncls, seed=seed, lr=lr)
    eng = UnetEngine(in_channels=1, num_classes=ncls, d=d, max_batch=B, lr=lr, loss_weight=loss_weight)
    eng.set_weights(orc.P)
    if w is not None:
        eng.set_class_weights(w)
    return eng


def _same_state(a, b, grads=True):
    """every gradient and every tensor (weights after Adam, moving statistics) equal bit for bit"""
    for name, shape, trainable in a.tensor_infos():
        np.testing.assert_array_equal(a.get_tensor(name, shape), b.get_tensor(name, shape), err_msg=name)
        if trainable and grads:
            np.testing.assert_array_equal(a.get_grad(name, shape), b.get_grad(name, shape), err_msg=name)


@pytest.mark.parametrize("c", [95.0, 3.5])
def test_constant_table_equals_scalar_train_step(c):
    """3b. one whole train step, d = 16, B = 2 (fused head, head -> c18 BatchNorm-backward fusion)."""
    X, lab = K.unet_batch(2, 16, 95)
    scalar = _engine(95, 2, loss_weight=c)
    table = _engine(95, 2, w=np.full(95, c))
    m_s, m_t = scalar.train_step(X, lab), table.train_step(X, lab)
    print("c = %.1f: %s" % (c, m_s))
    np.testing.assert_array_equal(m_t, m_s)
    _same_state(table, scalar)


@pytest.mark.parametrize("ncls,B", [(95, 2), (95, 3), (17, 2)])
def test_weighted_train_step_matches_oracle(ncls, B):
    """4. UnetOracle(loss_weight=w) against set_class_weights(w): metrics, every gradient, moving statistics, Adam."""
    K.check_step_report(K.oracle_step_report(ncls, B))


def test_weighted_train_step_matches_oracle_on_the_other_head_routes():
    """4. (95, 2) again in a fresh process without the fused head and without the head -> c18 fusion: GEMM + head_kernel<true>,
    and the separate BatchNorm backward of c18 fed by the weighted dz."""
    script = ("import json, sys; sys.path[:0] = [%r, %r]; import class_weight_cases as K; "
              "print(json.dumps(K.oracle_step_report(95, 2)))" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, ICSG3D_NO_HEAD_BNFUSE="1", ICSG3D_NO_FUSED_HEAD="1")
    out = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    K.check_step_report(json.loads(out.stdout.strip().splitlines()[-1]))


def test_weighted_test_step():
    """5. test_step with the table: the oracle's eval-mode loss, nothing updated; NULL gives the scalar step back."""
    ncls, B, d = 95, 2, 16
    w = K.weight_vector(ncls)
    X, lab = K.unet_batch(B, d, ncls)
    orc = R.UnetOracle(in_ch=1, num_classes=ncls, seed=1, loss_weight=w)
    eng = _engine(ncls, B)
    rng = np.random.default_rng(3)
    for k in list(orc.S):                                                  # non-trivial moving statistics
        orc.S[k] = (rng.uniform(0.5, 1.5, orc.S[k].shape) if k.endswith("var") else rng.uniform(-0.2, 0.2, orc.S[k].shape))
        eng.set_tensor(k, orc.S[k])
    m_scalar = eng.test_step(X, lab)
    assert eng.get_class_weights() is None
    before, opt = eng.get_weights(), eng.get_optimizer_state()
    eng.set_class_weights(w)
    np.testing.assert_array_equal(eng.get_class_weights(), w.astype(np.float32))
    m, m_ref = eng.test_step(X, lab), orc.test_on_batch(X, lab)
    print("test_step %s vs %s (scalar %s)" % (m, m_ref, m_scalar))
    assert m_ref[1] > 1e-3 and abs(m_scalar[1] - m_ref[1]) > 0.1 * m_ref[1]
    np.testing.assert_allclose(m[:3], m_ref[:3], rtol=K.METRIC_RTOL)
    np.testing.assert_allclose(m[3:], m_ref[3:], rtol=1e-4, atol=1e-6)
    np.testing.assert_array_equal(m[2:], m_scalar[2:])                     # lsig, f1, wr: no weight in them
    after, opt2 = eng.get_weights(), eng.get_optimizer_state()
    assert sorted(after) == sorted(before)
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg=k)
    np.testing.assert_array_equal(opt2[0], opt[0]); np.testing.assert_array_equal(opt2[1], opt[1])
    assert opt2[2] == opt[2]
    eng.set_class_weights(None)
    assert eng.get_class_weights() is None
    np.testing.assert_array_equal(eng.test_step(X, lab), m_scalar)


def test_fed_and_resident_steps_take_the_table():
    """6a. train_step_fed and train_step_resident with the table equal the synchronous step bit for bit."""
    ncls, B = 95, 2
    w = K.weight_vector(ncls)
    X, lab = K.unet_batch(B, 16, ncls)
    sync = _engine(ncls, B, w=w)
    m_sync = sync.train_step(X, lab)
    res = _engine(ncls, B, w=w)
    res.upload_batch(X, lab)
    m_res = res.train_step_resident(want_metrics=True)
    np.testing.assert_array_equal(m_res, m_sync)
    _same_state(res, sync)
    fed = _engine(ncls, B, w=w)
    fed.feed_open((1,), (np.float32,), "u8", 2)
    slot = fed.feed_slot(0)
    slot["x"][0][:B] = X.astype(np.float32)
    slot["labels"][:B] = lab
    fed.feed_submit(0, B)
    m_fed = fed.feed_metrics(fed.train_step_fed(0)).copy()
    fed.feed_close()
    np.testing.assert_array_equal(m_fed, m_sync)
    _same_state(fed, sync)
    plain = _engine(ncls, B)                                               # ... and the table is what they all took
    assert abs(plain.train_step(X, lab)[1] - m_sync[1]) > 0.1 * m_sync[1]


def test_engine_growth_keeps_the_table():
    """6b. AtomUnet(weighted_loss=True): a batch of 2, then one of 3 (the engine is re-created) equals a model whose engine
    was created at max_batch = 3."""
    from icsg3d_amd.unet.unet import AtomUnet
    ncls, d = 95, 16
    w = K.weight_vector(ncls)
    X3, lab3 = K.unet_batch(3, d, ncls)
    P = R.UnetOracle(in_ch=1, num_classes=ncls, seed=1).P
    kw = dict(num_classes=ncls, class_weights=w, input_shape=(d, d, d, 1), lr=1e-3, weighted_loss=True)
    grown, fixed = AtomUnet(**kw), AtomUnet(max_batch=3, **kw)
    unweighted = AtomUnet(**dict(kw, weighted_loss=False))
    for u in (grown, fixed, unweighted):
        u._set_weights(P)
    steps = [(X3[:2], lab3[:2]), (X3, lab3)]
    m_grown = [grown.model.train_on_batch(X, y) for X, y in steps]
    assert grown._eng.max_batch == 3
    np.testing.assert_array_equal(grown._eng.get_class_weights(), w.astype(np.float32))
    m_fixed = [fixed.model.train_on_batch(X, y) for X, y in steps]
    assert m_grown == m_fixed, (m_grown, m_fixed)
    wg, wf = grown._get_weights(), fixed._get_weights()
    for k in wf:
        np.testing.assert_array_equal(wg[k], wf[k], err_msg=k)
    assert unweighted.model.train_on_batch(*steps[0])[1] != m_grown[0][1] and unweighted._eng.get_class_weights() is None


def test_single_rank_communicator_with_the_table():
    """7. the communicator path (metric all-reduce, bucketed gradients) with the table: the plain engine's bits, and the
    table survives comm_broadcast_state."""
    from icsg3d_amd.engine import comm_unique_id
    ncls, B = 95, 2
    w = K.weight_vector(ncls)
    X, lab = K.unet_batch(B, 16, ncls)
    plain, dp = _engine(ncls, B, w=w), _engine(ncls, B, w=w)
    dp.comm_init(0, 1, comm_unique_id())
    dp.broadcast_state(0)
    np.testing.assert_array_equal(dp.get_class_weights(), w.astype(np.float32))
    m_p, m_d = plain.train_step(X, lab), dp.train_step(X, lab)
    np.testing.assert_array_equal(m_d, m_p)
    _same_state(dp, plain)
    dp.set_class_weights(None)
    dp.broadcast_state(0)
    assert dp.get_class_weights() is None


# ----------------------------------------------------------------------------------------------------------------------
# 8. label_counts
# ----------------------------------------------------------------------------------------------------------------------
def _labels(n, ncls, dtype, seed):
    """98 % background, the rest spread over every class; then planted values that are no class id."""
    rng = np.random.default_rng(seed)
    lab = np.where(rng.uniform(size=n) < 0.98, 0, rng.integers(0, ncls, size=n)).astype(dtype)
    lab[-ncls:] = np.arange(ncls)                                          # every class, and the ragged tail of the array
    ref = np.bincount(lab.astype(np.int64), minlength=ncls)
    at = rng.choice(n - ncls, size=12, replace=False)
    bad = [ncls, 255, 128, 200] if dtype == np.uint8 else [float(ncls), 255.0, -1.0, 3.5, 0.5, np.nan, 1e9, -0.25, np.inf]
    for i, pos in enumerate(at[:len(bad)]):
        ref[int(lab[pos])] -= 1
        lab[pos] = bad[i]
    return lab, ref, len(bad)


@pytest.mark.parametrize("ncls", [2, 95, 127])
@pytest.mark.parametrize("n,dtype", [(5_000_011, np.uint8), (100_003, np.float32), (100_003, np.float64)],
                         ids=["u8", "f32", "f64"])
def test_label_counts_equal_bincount(n, dtype, ncls):
    from icsg3d_amd.engine import label_counts
    lab, ref, nbad = _labels(n, ncls, dtype, seed=n % 1000 + ncls)
    half = lab[:n // 2 + 3]
    clean = half[np.isin(half, np.arange(ncls))]                           # a valid array of another length
    counts, oor = label_counts(lab, ncls)
    assert counts.dtype == np.int64 and counts.shape == (ncls,)
    np.testing.assert_array_equal(counts, ref)
    assert oor == nbad and counts.sum() + oor == n and counts[0] > 0.97 * n and counts.min() >= 1
    c2, oor2 = label_counts(clean, ncls)                                   # counts are overwritten, not accumulated
    np.testing.assert_array_equal(c2, np.bincount(clean.astype(np.int64), minlength=ncls))
    assert oor2 == 0


def test_get_weights_on_the_device_equals_the_host_loop(tmp_path):
    from icsg3d_amd.unet.get_weights import get_weights
    folder = tmp_path / "species_matrices"
    folder.mkdir()
    rng = np.random.default_rng(12)
    names = ["mat_%02d.npy" % i for i in range(8)] + ["mat_%02d_rot_1.npy" % i for i in range(2)] + ["other_0.npy", "other_1.npy"]
    for k, name in enumerate(names):
        S = np.where(rng.uniform(size=(16, 16, 16)) < 0.9, 0, rng.integers(1, 60, size=(16, 16, 16))).astype(np.float64)
        if k >= 8:
            S[0, 0, 0] = 94.0                                              # would show up if the file were counted
        np.save(str(folder / name), S)
    ids = names[:8] + names[8:10] + ["missing.npy"]                        # rotated files are listed and still ignored
    host = get_weights(str(tmp_path), ids, 95)
    dev = get_weights(str(tmp_path), ids, 95, device=True)
    assert host[94] == 0 and (host > 0).sum() >= 50 and host[0] < 2
    np.testing.assert_array_equal(dev, host)
    np.save(str(folder / names[3]), np.full((16, 16, 16), 95.0))            # no class id: the host loop's IndexError
    with pytest.raises(IndexError):
        get_weights(str(tmp_path), ids, 95)
    with pytest.raises(IndexError):
        get_weights(str(tmp_path), ids, 95, device=True)


# ----------------------------------------------------------------------------------------------------------------------
# 9. argument errors: return codes, no fault
# ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from icsg3d_amd._lib import IcsError
    from icsg3d_amd.engine import label_counts, unet_head
    eng = _engine(17, 1)
    w = K.weight_vector(17)
    for bad, word in ((w[:16], "count"), (np.append(w, 1.0), "count"), (np.where(np.arange(17) == 3, -0.5, w), "finite"),
                      (np.where(np.arange(17) == 3, np.nan, w), "finite"), (np.where(np.arange(17) == 3, np.inf, w), "finite")):
        with pytest.raises(IcsError, match=word):
            eng.set_class_weights(bad)
        assert eng.get_class_weights() is None                             # a refused table is not half set
    eng.set_class_weights(w)
    with pytest.raises(IcsError, match="finite"):
        eng.set_class_weights(-w)
    np.testing.assert_array_equal(eng.get_class_weights(), w.astype(np.float32))
    case = K.head_case(17, HEAD_M)
    with pytest.raises(IcsError, match="finite"):
        unet_head(*K.head_args(case), mode=1, fused=False, class_weights=np.where(np.arange(17) == 2, np.nan, w))
    with pytest.raises(IcsError, match="loss modes"):
        unet_head(*K.head_args(case), mode=0, fused=False, class_weights=w)
    with pytest.raises(IcsError, match="one-hot"):
        label_counts(np.zeros((64, 17), np.float32), 17, label_kind="onehot")
    with pytest.raises(IcsError, match="num_classes"):
        label_counts(np.zeros(64, np.uint8), 128)
    X, lab = K.unet_batch(1, 16, 17)                                        # ... and the engine still works
    assert np.isfinite(eng.train_step(X, lab)).all()
