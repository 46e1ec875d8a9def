"""The yardsticks of tests/test_gpu_head_link.py, proven on the CPU before any GPU is involved:

  * the reference of tests/head_link_ref.py equals UnetOracle's own last block (Block "c18"), head, loss, metrics and their
    gradients at 1e-12;
  * the algebra of the head's BatchNorm-backward fusion -- Q = xhat^T dz, dW = gamma Q + beta sum(dz), c1 = W . sum(dz) / n,
    c2 = sum_cls W Q / n, dy = relu' scale (d - c1 - xhat c2) -- equals the plain BatchNorm backward at 1e-12 in every regime;
  * the same algebra in float32 numpy stays inside the GPU file's gradient bound max(1e-5, 2 e32) in every case and regime
    (its share of the bound is printed: the calibration test_conv_link_host.py does for the 3x3x3 folds);
  * the reference alone, fp64 against its float32 twin, stays within the decision caps of the GPU file for every input that
    file runs: <= 8 ReLU sides of P's y, <= 8 clip sides of the losses, <= 8 probabilities within 2e-5 of the 0.5 threshold
    of f1 / wr; and the sharp head puts the stated share of voxels at the probability clip."""
import numpy as np
import pytest

import head_link_ref as HR
from oracle import numpy_ref as R

CAP = 8
TOL = 1e-5


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("kw", [{}, {"bce_from_logits": True, "loss_weight": 7.5}, {"class_weights": True}], ids=str)
def test_reference_equals_the_oracles_last_block_head_and_loss(kw):
    d = HR.make_head_link(2, 4, 16, 95, seed=3, **kw)
    fP, fh, t, _ = HR.reference(d, eps=R.BN_EPS)
    w = d["class_weights"].astype(np.float64) if d["class_weights"] is not None else (d["loss_weight"] or None)
    orc = R.UnetOracle(in_ch=1, num_classes=95, loss_weight=w, bce_from_logits=d["bce_from_logits"])
    P = {"c18/" + k2: d["P"][k].astype(np.float64) for k, k2 in (("w", "kernel"), ("bias", "bias"), ("gamma", "gamma"), ("beta", "beta"))}
    P.update({"soft/kernel": d["head"]["wsoft"].astype(np.float64).reshape(1, 1, 1, 128, 95), "soft/bias": d["head"]["bsoft"].astype(np.float64),
              "sig/kernel": d["head"]["wsig"].astype(np.float64).reshape(1, 1, 1, 128, 1), "sig/bias": d["head"]["bsig"].astype(np.float64)})
    orc.P = P
    orc._trunk = lambda x, training, cache, upto=None: orc.blocks["c18"].fwd(x, orc.P, orc.S, training, cache)
    cache = {}
    lab = d["labels"].astype(np.int64)
    soft, sig = orc.forward(d["x0"], training=True, cache=cache)
    m = orc.loss_and_metrics(soft, sig, lab, cache["_head"]["zg"])
    met, _, _ = HR.head_metrics(d, fh)
    np.testing.assert_allclose(met[0], m, rtol=1e-12, atol=1e-15)
    # the head of UnetOracle.backward, then its c18 block
    B = soft.shape[0]
    y1, tt = R.one_hot(lab, 95), (lab != 0).astype(np.float64)[..., None]
    dzs = R.softmax_bwd(soft, R.wcce_bwd(y1, soft, orc.loss_weight, np.full(B, 1.0 / B)))
    if d["bce_from_logits"]:
        dzg = R.bce_logits_bwd(tt, cache["_head"]["zg"], np.full(sig.shape[:-1], 1.0 / sig[..., 0].size))
    else:
        dzg = R.bce_bwd(tt, sig, np.full(sig.shape[:-1], 1.0 / sig[..., 0].size)) * sig * (1 - sig)
    g = {}
    d1, g["soft/kernel"], g["soft/bias"] = R.conv3d_bwd(cache["_head"]["c18"], P["soft/kernel"], dzs)
    d2, g["sig/kernel"], g["sig/bias"] = R.conv3d_bwd(cache["_head"]["c18"], P["sig/kernel"], dzg)
    dx0 = orc.blocks["c18"].bwd(d1 + d2, P, orc.S, cache, g)
    want = {"dz": np.concatenate([dzs, dzg], -1), "dwsoft": g["soft/kernel"].reshape(128, 95), "dwsig": g["sig/kernel"].reshape(128),
            "dbias_head": np.concatenate([g["soft/bias"], g["sig/bias"]]), "dw": g["c18/kernel"], "dbias": g["c18/bias"],
            "dgamma": g["c18/gamma"], "dbeta": g["c18/beta"], "dx0": dx0}
    for k, v in want.items():
        assert _rel(t[k], v) <= 1e-12, (k, _rel(t[k], v))


FUSED_KEYS = ("dwsoft", "dwsig", "dgamma", "dbeta", "dy_p")


@pytest.mark.parametrize("regime", list(HR.REGIMES))
def test_fusion_algebra_equals_plain_batchnorm_backward(regime):
    d = HR.case_data("blocks3", regime)
    fP, fh, t, _ = HR.reference(d)
    fu = HR.fused_route(d, fP, fh, t["dz"])
    for k in FUSED_KEYS:
        e = _rel(fu[k], t[k])
        assert e <= 1e-12, (regime, k, e)


SHARE = {}


# every input on which the GPU file runs the fusion: each ncls = 95 shape with rows in sixteens, and every regime on the two
# regime shapes.  Not the 8-row and ncls != 95 shapes (no fusion there), and not the ranks cases: under SyncBN the fused
# route differs from this one only in where c1 / c2 are formed (the two per-rank sums added in fp64, bn_bwd_sync_c_kernel),
# which conv_layer_ref's sharded route covers in tests/test_syncbn_host.py
FUSED_CASES = [(s, "ordinary") for s in HR.SHAPES if HR.SHAPES[s][3] == 95 and HR.SHAPES[s][0] * HR.SHAPES[s][1] ** 3 % 16 == 0]
FUSED_CASES += [(s, g) for s in HR.REGIME_SHAPES for g in HR.REGIMES if g != "ordinary"]


@pytest.mark.parametrize("shape,regime", FUSED_CASES, ids=lambda v: str(v))
def test_float32_fusion_stays_inside_the_gradient_bound(shape, regime):
    """the fused formulas in float32 numpy (GEMMs, xhat and the apply in float32; the class sums through fp64, as the kernels)
    against the fp64 reference, with the reference's decisions, measured against max(1e-5, 2 e32) of the plain formulas"""
    d = HR.case_data(shape, regime)
    fP, fh, t, _ = HR.reference(d)
    e32 = HR.e32_of(d, fP, fh, t)
    fP32, fh32 = HR.forward(d, np.float32)
    hb = HR.head_backward(d, fh32, fP32["o"], HR.own_pins(fP, fh))
    fP32 = dict(fP32, s=np.where(fP["y"] > 0, fP32["s"], 0).astype(np.float32))        # the reference's ReLU sides
    fu = HR.fused_route(d, fP32, fh32, hb["dz"], np.float32)
    err = HR.rel_errors(dict(t, **{k: fu[k] for k in FUSED_KEYS}), t, fP)
    for k in FUSED_KEYS:
        lim = max(TOL, 2 * e32[k])
        if err[k] / lim > SHARE.get(k, (0, ""))[0]:
            SHARE[k] = err[k] / lim, "%s/%s" % (shape, regime)
        print("  %s %s %-7s fused32 %.3g  e32 %.3g  bound %.3g  share %.2f" % (shape, regime, k, err[k], e32[k], lim, err[k] / lim))
        assert err[k] <= lim, (shape, regime, k, err[k], e32[k])


def test_zz_report_share_of_the_bound():
    for k, v in sorted(SHARE.items()):
        print("  float32 fusion, worst share of max(1e-5, 2 e32): %-7s %.2f  (%s)" % (k, v[0], v[1]))


@pytest.mark.parametrize("cid,make", HR.all_cases(), ids=[c for c, _ in HR.all_cases()])
def test_reference_alone_stays_within_the_decision_caps(cid, make):
    d = make()
    fP, fh = HR.forward(d)
    fP32, fh32 = HR.forward(d, np.float32)
    relu = int(((fP32["y"] > 0) != (fP["y"] > 0)).sum())
    clip = int((fh32["soft_inside"] != fh["soft_inside"]).sum())
    if not d["bce_from_logits"]:
        clip += int((fh32["sig_inside"] != fh["sig_inside"]).sum())
    _, _, near = HR.head_metrics(d, fh, d["ranks"])
    print("  %s: ReLU sides %d, clip sides %d, probabilities within 2e-5 of 0.5: %d" % (cid, relu, clip, int(near.sum())))
    assert relu <= CAP and clip <= CAP and near.sum() <= CAP, (cid, relu, clip, near)
    # one voxel across the threshold moves tp / predicted by one: |d f1| <= 3 / voxels, |d wr| <= 1 / (voxels with a label != 0)
    if "sharp" in cid:
        share = 1.0 - float(fh["soft_inside"].mean())
        share_sig = 1.0 - float(fh["sig_inside"].mean())
        print("  %s: voxels at the softmax clip %.2f, at the sigmoid clip %.2f" % (cid, share, share_sig))
        assert share >= 0.25 and share_sig >= 0.25, (cid, share, share_sig)
    if "dead" in cid:
        assert (fP["y"][..., HR.DEAD_CH] == 0).all() and fP["var"][HR.DEAD_CH] == 0


@pytest.mark.parametrize("shape", HR.REGIME_SHAPES)
def test_reference_at_the_clip_against_numpy_ref(shape):
    """The sharp regime, where the ordinary-input equality with UnetOracle says nothing: the reference's per-voxel losses and
    its dz against numpy_ref's clipped formulas.  They agree at 1e-8 (float32(1e-7) against 1e-7 in the lower bound) except
    where the two upper bounds differ, and there by exactly the known amount: a sigmoid above 1 - 2^-23 with target 0 costs
    -log(2^-23) = 15.94 here (float32 arithmetic) and -log(1e-7) = 16.12 in numpy_ref; a sigmoid in (1 - 2^-23, 1 - 1e-7]
    is outside the clip here (dz = 0) and inside it there."""
    d = HR.case_data(shape, "sharp")
    fP, fh, t, _ = HR.reference(d)
    lab = d["labels"].astype(np.int64)
    o = fP["o"]
    soft = fh["p"].reshape(lab.shape + (95,))
    sig = fh["ps"].reshape(lab.shape + (1,))
    y1, tt = R.one_hot(lab, 95), (lab != 0).astype(np.float64)[..., None]
    n = lab.size
    # softmax: loss per voxel and dz
    ls = -(y1 * np.log(np.clip(soft / soft.sum(-1, keepdims=True), R.K_EPSILON, 1 - R.K_EPSILON)) * 95.0).sum(-1).reshape(-1)
    assert (~fh["soft_inside"]).mean() >= 0.25
    np.testing.assert_allclose(fh["lsoft"], ls, rtol=1e-8, atol=1e-13)
    B = lab.shape[0]
    dzs = R.softmax_bwd(soft, R.wcce_bwd(y1, soft, 95.0, np.full(B, 1.0 / B)))
    assert _rel(t["dz"][..., :95], dzs) <= 1e-12
    # sigmoid
    lg = R.bce_loss(tt, sig).reshape(-1)
    ps, tf = fh["ps"], fh["t"]
    high = ps > HR.CLIP_HI
    assert high.sum() >= 8 and ((tf == 0) & high).sum() >= 4
    np.testing.assert_allclose(fh["lsig"][~high], lg[~high], rtol=1e-8, atol=1e-13)     # (1e-7-sized terms: -log(1 - lo))
    hz = high & (tf == 0)
    np.testing.assert_allclose(fh["lsig"][hz], -np.log(2.0 ** -23), rtol=1e-12)           # 15.942
    assert (lg[hz & (ps > 1 - R.K_EPSILON)] == -np.log(1 - (1 - R.K_EPSILON))).all()     # 16.118
    assert abs(-np.log(2.0 ** -23) - 15.942) < 1e-3 and abs(-np.log(1e-7) - 16.118) < 1e-3
    dzg = (R.bce_bwd(tt, sig, np.full(sig.shape[:-1], 1.0 / n)) * sig * (1 - sig)).reshape(-1)
    between = high & (ps <= 1 - R.K_EPSILON)
    mine = t["dz"][..., 95].reshape(-1)
    assert (mine[between] == 0).all()
    scale = np.abs(dzg).max()
    assert np.abs(mine[~between] - dzg[~between]).max() <= 1e-12 * scale
    print("  %s: %d sigmoids above 1 - 2^-23, %d of them below 1 - 1e-7" % (shape, int(high.sum()), int(between.sum())))
