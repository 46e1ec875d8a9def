"""Shared case builders of the per-class loss weight tests (tests/test_gpu_class_weights.py on the device,
tests/test_class_weights_host.py for the builders' own assertions): weight vectors, head-op inputs with their fp64
reference, network batches with enough classes, and the one-train-step-against-the-oracle report that the GPU test runs in
its own process and in a child process with other head routes.

Nothing here is modified after it is built: the builders cache and the tests only read."""
import numpy as np

from oracle import numpy_ref as R

METRIC_RTOL = 2e-5
GRAD_TOL = 1e-4       # the constants of tests/test_gpu_widths.py::test_unet_train_step_at_other_class_counts, unchanged
BN_TOL = 1e-5
MAX_KINK_FLIPS = 64

UNET_LAYERS = ["c1", "c2", "c3", "c4", "c5", "c6", "c9", "c10", "c13", "c14", "c15", "c16", "c17", "c18"]


def layer_shape(name, B, d):
    res = {"c1": 1, "c2": 1, "c3": 2, "c4": 2, "c5": 4, "c6": 4, "c9": 8, "c10": 8, "c13": 4, "c14": 4,
           "c15": 2, "c16": 2, "c17": 1, "c18": 1}[name]
    cout = dict((n, c) for n, _, c in R.UNET_CONVS)[name]
    S = d // res
    return (B, S, S, S, cout)


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ----------------------------------------------------------------------------------------------------------------------
# weight vectors
# ----------------------------------------------------------------------------------------------------------------------
def second_zero_class(ncls):
    """The further class with weight 0 (besides the background).  With two classes there is none to spare: zeroing class 1
    as well would make the loss identically zero, and a test of 0 == 0 checks nothing."""
    return None if ncls < 3 else min(5, ncls - 1)


def weight_vector(ncls):
    """Multiples of 1/64 in [0.25, 8] (exact in fp32, products with 1 / M round once), non-uniform, w[0] = 0 and
    w[second_zero_class] = 0."""
    rng = np.random.default_rng(7700 + ncls)
    w = rng.integers(16, 513, size=ncls).astype(np.float64) / 64.0
    assert w.min() >= 0.25 and w.max() <= 8.0 and np.unique(w).size > min(ncls, 8) // 2
    w[0] = 0.0
    if second_zero_class(ncls) is not None:
        w[second_zero_class(ncls)] = 0.0
    return w


# ----------------------------------------------------------------------------------------------------------------------
# head op: inputs whose logits are exact in fp32, and the fp64 reference with the vector
# ----------------------------------------------------------------------------------------------------------------------
_head_cache = {}


def head_case(ncls, M):
    """tests/test_gpu_widths.py::_head_case at any row count, plus the weighted reference.

    Every input is a multiple of 2^-8 below 8 in magnitude and every weight one of {0, +-1/4, 1}: the 128-term dot products
    of the 1x1x1 GEMM are exact in fp32 in any summation order (the MFMA's included), so the logits both head kernels see
    are the reference's to the bit."""
    if (ncls, M) in _head_cache:
        return _head_cache[(ncls, M)]
    rng = np.random.default_rng(1000 + ncls + 7 * M)
    lab = rng.integers(0, ncls, size=M).astype(np.uint8)
    wrong = (lab.astype(np.int64) + 1 + rng.integers(0, ncls - 1, size=M)) % ncls
    target = np.where(rng.uniform(size=M) < 0.7, lab, wrong)
    x = np.round(rng.normal(size=(M, 128)) * 0.5 * 256) / 256
    boost = np.round((np.log(ncls) + 3.0) * 256) / 256
    x[np.arange(M), target] += boost
    x = np.clip(x, -7.5, 7.5).astype(np.float32)
    pick = lambda shape: rng.choice([-0.25, 0.0, 0.25], size=shape, p=[0.1, 0.8, 0.1])
    ws = pick((128, ncls))
    ws[np.arange(ncls), np.arange(ncls)] = 1.0
    wg = pick(128)
    bs = np.round(rng.normal(size=ncls) * 0.25 * 64) / 64
    bg = np.round(rng.normal(size=1) * 0.25 * 64) / 64
    ws, wg, bs, bg = (a.astype(np.float32) for a in (ws, wg, bs, bg))
    f8 = lambda a: a.astype(np.float64)
    z = f8(x) @ f8(ws) + f8(bs)
    zg = f8(x) @ f8(wg) + f8(bg)[0]
    assert np.array_equal((x @ ws + bs).astype(np.float64), z)          # exact in fp32, as claimed
    p, ps = R.softmax(z), R.sigmoid(zg)
    y = R.one_hot(lab, ncls)
    qt = (p * y).sum(-1)
    # no clip kink of either loss in play: the gradient reference needs no pinned decisions
    assert qt.min() > 1e-6 and qt.max() < 1 - 1e-6 and ps.min() > 1e-6 and ps.max() < 1 - 1e-6
    w = weight_vector(ncls)
    t = (lab != 0).astype(np.float64)
    p5, y5 = p.reshape(1, M, 1, 1, ncls), y.reshape(1, M, 1, 1, ncls)
    lsoft = float(R.wcce_loss(y5, p5, w).mean())
    lsig = float(R.bce_loss(t[:, None], ps[:, None]).mean())
    dzs = R.softmax_bwd(p5, R.wcce_bwd(y5, p5, w, np.ones(1))).reshape(M, ncls)
    dsig = R.bce_bwd(t[:, None], ps[:, None], np.full(M, 1.0 / M))
    dzg = (dsig * ps[:, None] * (1 - ps[:, None]))[:, 0]
    zero_rows = w[lab] == 0
    # every class occurs (the second zero-weight class among them), and the reference is not in a 0 == 0 regime: weighted
    # voxels carry the loss and a gradient, the zero-weight rows carry exactly none
    assert np.unique(lab).size == ncls and zero_rows.any() and not zero_rows.all()
    assert lsoft > 1e-2 and np.abs(dzs[~zero_rows]).max(-1).min() > 0 and not dzs[zero_rows].any()
    assert float(R.wcce_loss(y5, p5, (w == 0).astype(np.float64)).mean()) > 1e-4         # ... which a weight of 1 would not
    case = dict(x=x, ws=ws, bs=bs, wg=wg, bg=bg, lab=lab, w=w, lsoft=lsoft, lsig=lsig, dzs=dzs, dzg=dzg, zero_rows=zero_rows)
    _head_cache[(ncls, M)] = case
    return case


def head_args(case):
    return case["x"], case["ws"], case["bs"], case["wg"], case["bg"], case["lab"]


# ----------------------------------------------------------------------------------------------------------------------
# network batches
# ----------------------------------------------------------------------------------------------------------------------
_batch_cache = {}


def unet_batch(B, d, ncls):
    """R.synthetic_batch's densities with its non-zero voxels remapped over the classes.  Unchanged, the synthetic labels hit
    8 classes; here the class of an atom voxel follows its position, so that (asserted) at least 40 classes occur at
    ncls = 95 (every class at ncls <= 40), the background share stays between 50 % and 99 %, and the second zero-weight
    class occurs."""
    if (B, d, ncls) in _batch_cache:
        return _batch_cache[(B, d, ncls)]
    X, lab, _ = R.synthetic_batch(B, d, 1, seed=0, dtype=np.float64)
    X = X + 1e-3 * np.random.default_rng(5).uniform(size=X.shape)
    zz, yy, xx = np.meshgrid(np.arange(d), np.arange(d), np.arange(d), indexing="ij")
    pos = (zz * 31 + yy * 17 + xx * 7)[None] + 11 * np.arange(B)[:, None, None, None]
    new = 1 + (lab.astype(np.int64) * 13 + pos) % (ncls - 1)
    lab = np.where(lab != 0, new, 0).astype(np.uint8)
    check_batch(lab, ncls)
    _batch_cache[(B, d, ncls)] = (X, lab)
    return X, lab


def check_batch(lab, ncls):
    bg = float((lab == 0).mean())
    assert np.unique(lab).size >= min(40, ncls), np.unique(lab).size
    assert 0.5 <= bg <= 0.99, bg
    z = second_zero_class(ncls)
    assert z is None or (lab == z).any()
    assert lab.max() < ncls


# ----------------------------------------------------------------------------------------------------------------------
# one train step against the oracle (runs on the GPU; called in-process and from a child process with other head routes)
# ----------------------------------------------------------------------------------------------------------------------
def oracle_step_report(ncls, B, d=16, lr=1e-3):
    """UnetOracle(loss_weight=w) against an engine with set_class_weights(w): the procedure of
    tests/test_gpu_widths.py::test_unet_train_step_at_other_class_counts.  Returns plain numbers (JSON-able); the caller
    asserts with the constants above."""
    from icsg3d_amd.engine import UnetEngine
    w = weight_vector(ncls)
    orc = R.UnetOracle(in_ch=1, num_classes=ncls, seed=1, lr=lr, loss_weight=w)
    eng = UnetEngine(in_channels=1, num_classes=ncls, d=d, max_batch=B, lr=lr)
    eng.set_weights(orc.P)
    eng.set_class_weights(w)
    X, lab = unet_batch(B, d, ncls)
    p0 = {k: v.copy() for k, v in orc.P.items()}
    # the same forward pass under the reference's scalar weight: the table must matter for the comparison to mean anything
    soft0, _ = orc.forward(X, training=True)
    lsoft_scalar = float(R.wcce_loss(R.one_hot(lab, ncls), soft0, float(ncls)).mean())
    m = eng.train_step(X, lab)
    kink = {n: eng.get_activation(n, layer_shape(n, B, d)) for n in UNET_LAYERS}
    affine = {n: eng.get_bn_affine(n, layer_shape(n, B, d)[-1]) for n in ("c2", "c4", "c6")}
    m_ref = orc.train_on_batch(X, lab, kink=kink, affine=affine)
    grad_err, adam_err, bn_err = {}, {}, {}
    for name, shape, trainable in eng.tensor_infos():
        if trainable:
            g = eng.get_grad(name, shape)
            grad_err[name] = rel_err(g, orc.last_grads[name])
            p_exp, _, _ = R.adam_update(p0[name], g.astype(np.float64), 0.0, 0.0, 1, lr)
            adam_err[name] = rel_err(eng.get_tensor(name, shape), p_exp)
        else:
            bn_err[name] = rel_err(eng.get_tensor(name, shape), orc.S[name])
    return dict(metrics=[float(v) for v in m], metrics_ref=[float(v) for v in m_ref], lsoft_scalar=lsoft_scalar,
                flips=int(sum(orc.kink_flips.values())), grad_err=grad_err, adam_err=adam_err, bn_err=bn_err)


def check_step_report(r):
    print("kink_flips %d, metrics %s vs %s (scalar-weight lsoft %.4f)" % (r["flips"], r["metrics"], r["metrics_ref"], r["lsoft_scalar"]))
    worst = max(r["grad_err"], key=r["grad_err"].get)
    print("worst gradient error %.2e (%s)" % (r["grad_err"][worst], worst))
    m, m_ref = np.array(r["metrics"]), np.array(r["metrics_ref"])
    assert r["flips"] <= MAX_KINK_FLIPS, r["flips"]
    assert m_ref[1] > 1e-3 and abs(m_ref[1] - r["lsoft_scalar"]) > 0.1 * r["lsoft_scalar"]     # neither 0 == 0 nor the scalar loss
    np.testing.assert_allclose(m[:3], m_ref[:3], rtol=METRIC_RTOL)
    np.testing.assert_allclose(m[3:], m_ref[3:], rtol=1e-4, atol=1e-6)
    for name, e in r["grad_err"].items():
        assert e <= GRAD_TOL, (name, e)
    for name, e in r["adam_err"].items():
        assert e <= 2e-5, (name, e)
    for name, e in r["bn_err"].items():
        assert e <= BN_TOL, (name, e)
