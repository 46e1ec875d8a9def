"""The two engines away from their default widths and loss constants, against the fp64 oracle (oracle/numpy_ref.py).

Every other whole-network test builds UnetEngine at num_classes = 95 and VaeEngine at filters (16, 32, 64, 128), latent 256,
alpha 0.5, beta 3e-4, unit tap weights, bn_unbias = True.  The kernels pick their code path from exactly these numbers
(head_fused_ok / head_dgrad_ok: ncls == 95; elementwise.hip: C % 4, C / 4 a power of two; engine.hip: the condition fold at
filters[0] in {16, 32}, padded_cin, enable_split_up), so other values land on code nothing else runs:

  1. head_kernel behind the generic 1x1x1 GEMM at ncls in {2, 15, 16, 17, 33, 96, 127} (16 lanes per voxel, nj = ceil(ncls / 16)
     columns per lane, ldz = ncls + 1), op level, M = 1037 rows (ragged last four-voxel wave);
  2. one U-Net train step at num_classes in {2, 17, 96, 127}, with loss_weight = 3.5, bn_unbias = False and B = 3 among them;
  3. one DFC-VAE train step (and the eval-mode calls) at eleven other width / latent / condition / loss-constant sets;
  4. the class API's checkpoint round trip at such shapes;
  5. what ics_unet_create / ics_vae_create / ics_op_unet_head refuse, and that the smallest accepted sizes run.

Bounds are the project's own: forward tensors 1e-5 tensor-relative, metrics rtol 2e-5, gradients 1e-4
with the activation decisions pinned (at most 64 of them flipped by the pinning, as tests/test_gpu_switches.py), BatchNorm
statistics 1e-5."""
import re

import numpy as np
import pytest

from oracle import numpy_ref as R
from test_gpu_metrics import _check_counts
from test_gpu_unet import UNET_LAYERS, _layer_shape
from test_gpu_vae import _pm_layer_shapes

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5
METRIC_RTOL = 2e-5
GRAD_TOL = 1e-4       # ORACLE_GRAD_TOL of tests/test_gpu_switches.py
BN_TOL = 1e-5
MAX_KINK_FLIPS = 64   # the cap of tests/test_gpu_switches.py: the pinning must not be able to absorb a wrong activation


# ------------------------------------------------------------------------------------------------------------------
# 1. head kernels at other class counts, op level
# ------------------------------------------------------------------------------------------------------------------
HEAD_M = 1037
HEAD_NCLS = [2, 15, 16, 17, 33, 96, 127]
_head_cache = {}


def _head_case(ncls):
    """Inputs and the fp64 reference of one class count (computed once, shared by the loss_weight cases, never modified).

    Every input is a multiple of 2^-8 below 8 in magnitude and every weight one of {0, +-1/4, 1}: the 128-term dot
    products of the 1x1x1 GEMM are then exact in fp32 in any summation order, so the logits the head kernel reads are the
    reference's to the bit and test_gpu_metrics.py's probability bound (written for an identity head) carries over -- while
    the weights are dense enough that a dropped or shifted class column changes every row."""
    if ncls in _head_cache:
        return _head_cache[ncls]
    rng = np.random.default_rng(1000 + ncls)
    M = HEAD_M
    lab = rng.integers(0, ncls, size=M).astype(np.uint8)
    # the voxel's "intended" class: its label for 70 % of the voxels, another class for the rest
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
    case = dict(x=x, ws=ws, bs=bs, wg=wg, bg=bg, lab=lab, p=p, ps=ps, y=y, t=(lab != 0).astype(np.float64))
    _head_cache[ncls] = case
    return case


@pytest.mark.parametrize("loss_weight", [0.0, 3.5], ids=["w_default", "w3.5"])
@pytest.mark.parametrize("ncls", HEAD_NCLS)
def test_head_kernel_at_other_class_counts(ncls, loss_weight):
    """GEMM (Cout = ncls + 1) + head_kernel: probabilities, losses / metrics / the seven sums, dLoss/dlogits against
    R.softmax / R.wcce_loss / R.bce_loss / R.wcce_bwd and the count formulas, bounds of tests/test_gpu_metrics.py."""
    from icsg3d_amd.engine import unet_head
    c = _head_case(ncls)
    M, lab, p, ps, y, t = HEAD_M, c["lab"], c["p"], c["ps"], c["y"], c["t"]
    head = (c["x"], c["ws"], c["bs"], c["wg"], c["bg"], lab)
    w = float(ncls) if loss_weight == 0.0 else loss_weight              # unet/unet.py:253: the integer num_classes
    p5 = p.reshape(1, M, 1, 1, ncls)
    y5 = y.reshape(1, M, 1, 1, ncls)
    # the reference itself is not in the 0 == 0 regime
    ref_tp = np.round(np.clip(y * p, 0, 1)).sum()
    ref_pred = np.round(np.clip(p, 0, 1)).sum()
    assert ref_tp > 100 and ref_pred > ref_tp and (lab != 0).sum() > 0, (ref_tp, ref_pred)

    probs, _, _ = unet_head(*head, mode=0, fused=False, loss_weight=loss_weight)
    assert probs.shape == (M, ncls + 1)
    np.testing.assert_allclose(probs[:, :ncls], p, rtol=2e-6, atol=1e-9)
    np.testing.assert_allclose(probs[:, ncls], ps, rtol=2e-6, atol=1e-9)

    _, m, sums = unet_head(*head, mode=1, fused=False, loss_weight=loss_weight)
    lsoft = R.wcce_loss(y5, p5, w).mean()
    lsig = R.bce_loss(t[:, None], ps[:, None]).mean()
    print("ncls %d w %.1f: device %s, reference lsoft %.6f lsig %.6f" % (ncls, w, m, lsoft, lsig))
    np.testing.assert_allclose(m[1], lsoft, rtol=1e-5)
    np.testing.assert_allclose(m[2], lsig, rtol=1e-5)
    np.testing.assert_allclose(m[0], lsoft + lsig, rtol=1e-5)
    ref, exact = _check_counts(sums, lab, p)                           # counts equal; <= 3 voxels within 2e-5 of one half
    assert ref["tp"] == ref_tp and ref["wr_possible"] == (lab != 0).sum() and ref["wr_tp"] > 0
    np.testing.assert_allclose(m[3], R.f1_m(y, p), rtol=1e-5 if exact else 1e-3)
    np.testing.assert_allclose(m[4], R.wr_m(y, p), rtol=1e-5 if exact else 1e-3)
    np.testing.assert_allclose(sums["sum_lsoft"], lsoft * M, rtol=1e-5)
    np.testing.assert_allclose(sums["sum_lsig"], lsig * M, rtol=1e-5)

    dz, m2, _ = unet_head(*head, mode=2, fused=False, loss_weight=loss_weight)
    np.testing.assert_array_equal(m2, m)
    dzs = R.softmax_bwd(p5, R.wcce_bwd(y5, p5, w, np.ones(1))).reshape(M, ncls)
    dsig = R.bce_bwd(t[:, None], ps[:, None], np.full(M, 1.0 / M))
    dzg = (dsig * ps[:, None] * (1 - ps[:, None]))[:, 0]
    # dz = w (p - y) / M: p carries the 2e-6 of the probability bound, |p - y| <= 1 = the scale of the largest element,
    # plus three fp32 roundings (subtraction, two products): 2e-6 + 3 * 2^-24 < 2.5e-6 of the tensor's maximum
    assert np.abs(dz[:, :ncls] - dzs).max() <= 2.5e-6 * np.abs(dzs).max()
    assert np.abs(dz[:, ncls] - dzg).max() <= 2.5e-6 * np.abs(dzg).max()


# ------------------------------------------------------------------------------------------------------------------
# 2. U-Net train step at other class counts
# ------------------------------------------------------------------------------------------------------------------
def _unet_batch(B, d, ncls):
    X, lab, _ = R.synthetic_batch(B, d, 1, seed=0, dtype=np.float64)
    X = X + 1e-3 * np.random.default_rng(5).uniform(size=X.shape)
    return X, (lab % ncls).astype(np.uint8)


#                                       ncls  B  loss_weight  bn_unbias
@pytest.mark.parametrize("ncls,B,lw,unbias", [(2, 2, 3.5, True), (17, 2, None, False), (96, 3, None, True),
                                              (127, 2, None, True)])
def test_unet_train_step_at_other_class_counts(ncls, B, lw, unbias, relerr):
    """Metrics, every gradient, the BatchNorm moving statistics and the Adam update of one train step; then predict /
    predict_labels from the oracle's updated state.  The head takes the generic GEMM + head_kernel + split_cols path."""
    from icsg3d_amd.engine import UnetEngine
    d, lr = 16, 1e-3
    orc = R.UnetOracle(in_ch=1, num_classes=ncls, seed=1, lr=lr, loss_weight=lw, bn_unbias=unbias)
    eng = UnetEngine(in_channels=1, num_classes=ncls, d=d, max_batch=B, lr=lr, loss_weight=lw or 0.0, bn_unbias=unbias)
    eng.set_weights(orc.P)
    X, lab = _unet_batch(B, d, ncls)
    p0 = {k: v.copy() for k, v in orc.P.items()}
    m = eng.train_step(X, lab)
    kink = {n: eng.get_activation(n, _layer_shape(n, B, d)) for n in UNET_LAYERS}
    affine = {n: eng.get_bn_affine(n, _layer_shape(n, B, d)[-1]) for n in ("c2", "c4", "c6")}
    m_ref = orc.train_on_batch(X, lab, kink=kink, affine=affine)
    flips = sum(orc.kink_flips.values())
    print("ncls %d: kink_flips %d, metrics %s vs %s" % (ncls, flips, m, m_ref))
    assert flips <= MAX_KINK_FLIPS, orc.kink_flips
    np.testing.assert_allclose(m[:3], m_ref[:3], rtol=METRIC_RTOL)
    np.testing.assert_allclose(m[3:], m_ref[3:], rtol=1e-4, atol=1e-6)
    worst = 0.0
    for name, shape, trainable in eng.tensor_infos():
        if trainable:
            g = eng.get_grad(name, shape)
            e = relerr(g, orc.last_grads[name])
            worst = max(worst, e)
            assert e <= GRAD_TOL, (name, e)
            # Adam (keras 2.3.1 formula) applied to the engine's own gradient, in fp64
            p_exp, _, _ = R.adam_update(p0[name], g.astype(np.float64), 0.0, 0.0, 1, lr)
            assert relerr(eng.get_tensor(name, shape), p_exp) <= 2e-5, name
        else:
            assert relerr(eng.get_tensor(name, shape), orc.S[name]) <= BN_TOL, name
    print("ncls %d: worst gradient error %.2e" % (ncls, worst))
    # inference from one common state (the oracle's weights after its step, non-trivial moving statistics)
    eng.set_weights(orc.P)
    rng = np.random.default_rng(3)
    for k in list(orc.S):
        orc.S[k] = (rng.uniform(0.5, 1.5, orc.S[k].shape) if k.endswith("var") else rng.uniform(-0.2, 0.2, orc.S[k].shape))
        eng.set_tensor(k, orc.S[k])
    soft_ref, sig_ref = orc.forward(X, training=False)
    soft, sig = eng.predict(X)
    assert soft.shape == (B, d, d, d, ncls) and sig.shape == (B, d, d, d, 1)
    assert relerr(soft, soft_ref) <= FWD_TOL and relerr(sig, sig_ref) <= FWD_TOL
    thresh = float(np.median(sig_ref))                                 # a threshold that separates something
    sp, mk = eng.predict_labels(X, thresh)
    srt = np.sort(soft_ref, -1)
    clear = (srt[..., -1] - srt[..., -2]) > 1e-4
    assert clear.mean() > 0.5 and np.array_equal(sp[clear], soft_ref.argmax(-1)[clear])
    clear_s = np.abs(sig_ref[..., 0] - thresh) > 1e-4
    want = sig_ref[..., 0] >= thresh
    assert want[clear_s].any() and not want[clear_s].all()
    assert np.array_equal(mk[clear_s].astype(bool), want[clear_s])


# ------------------------------------------------------------------------------------------------------------------
# 3. DFC-VAE at other widths and loss constants
# ------------------------------------------------------------------------------------------------------------------
DEFAULT_FILTERS = (16, 32, 64, 128)
VAE_CASES = {
    # condition fold at the other admitted width; Winograd e1 32 -> 32
    "A": dict(filters=(32, 32, 64, 64), latent=64, cond=10, C=1, B=2),
    # no fold: 11-channel e0 with a broadcast source
    "B": dict(filters=(8, 16, 32, 64), latent=256, cond=10, C=1, B=3),
    # multiples of 4 that are not powers of two: fusion predicates false, padded Cin
    "C": dict(filters=(12, 20, 36, 68), latent=100, cond=1, C=1, B=2),
    # C % 4 != 0 everywhere: the scalar VW = 1 paths
    "D": dict(filters=(6, 10, 18, 34), latent=20, cond=3, C=1, B=3),
    # the same widths behind a 4-channel input (e0 Cin = 16)
    "E": dict(filters=(6, 10, 18, 34), latent=20, cond=3, C=4, B=2),
    "F": dict(filters=DEFAULT_FILTERS, latent=256, cond=10, C=1, B=2, alpha=0.25, beta=1e-2, pm_w=(0.5, 0.0, 2.0, 1.0),
              unbias=False),
    "G": dict(filters=DEFAULT_FILTERS, latent=256, cond=10, C=1, B=2, alpha=0.0),
    # d2 is 32 -> 10 over an upsampled source: 32 input channels qualify for the up-split, 10 outputs do not
    # (launch_pool27 moves four channels per thread), so the layer keeps the direct kernels
    "H": dict(filters=(6, 10, 32, 64), latent=20, cond=3, C=1, B=2),
    # widths past the 256 column groups one block of the generic BatchNorm-backward kernels holds (elementwise.hip
    # bn_bwd_reduce_kernel / bn_bwd_apply_kernel): 260 = 65 float4 groups, which do not divide the 256 threads; 257 scalar
    # columns and 1028 = 257 float4 groups, whose second pass over the columns is ragged (one group of 256)
    "I": dict(filters=(16, 32, 64, 260), latent=32, cond=3, C=1, B=2),
    "J": dict(filters=(16, 32, 64, 257), latent=32, cond=3, C=1, B=3),
    "K": dict(filters=(16, 32, 64, 1028), latent=32, cond=3, C=1, B=2),
}


def _nonzero_biases(vo):
    """The initialisers leave every bias at zero, and a term that is multiplied by or added from a zero cannot be seen to
    be missing (e0's bias enters the folded layer through the condition's bias table): small non-zero biases, as fp32
    holds them.  In front of a BatchNorm a bias moves the batch mean, i.e. the moving statistics that are compared."""
    rng = np.random.default_rng(11)
    for k in vo.P:
        if k.endswith("/bias"):
            vo.P[k] = (rng.normal(size=vo.P[k].shape) * 0.1).astype(np.float32).astype(vo.P[k].dtype)


def _vae_setup(case, d=16, lr=5e-4):
    from icsg3d_amd.engine import UnetEngine, VaeEngine
    c = dict(alpha=0.5, beta=3e-4, pm_w=(1.0, 1.0, 1.0, 1.0), unbias=True)
    c.update(VAE_CASES[case])
    B, C = c["B"], c["C"]
    uo = R.UnetOracle(in_ch=C, seed=1)                                  # the frozen perceptual U-Net: default 95 classes
    opts = dict(in_ch=C, cond=c["cond"], filters=c["filters"], latent=c["latent"], d=d, alpha=c["alpha"], beta=c["beta"],
                lr=lr, seed=3, pm_layer_weights=c["pm_w"], bn_unbias=c["unbias"])
    vo = R.VaeOracle(uo, **opts)
    ue = UnetEngine(in_channels=C, d=d, max_batch=B)
    ue.set_weights(uo.P)
    ve = VaeEngine(ue, in_channels=C, cond_shape=c["cond"], latent_dim=c["latent"], filters=c["filters"], d=d, max_batch=B,
                   lr=lr, alpha=c["alpha"], beta=c["beta"], pm_layer_weights=c["pm_w"], bn_unbias=c["unbias"])
    assert sorted((n, s) for n, s, _ in ve.tensor_infos() if n in vo.P) == sorted((n, tuple(s)) for n, s in vo.shapes)
    _nonzero_biases(vo)
    ve.set_weights(vo.P)
    X, _, _ = R.synthetic_batch(B, d, C, seed=0, dtype=np.float64)
    X = X + 1e-3 * np.random.default_rng(5).uniform(size=X.shape)
    rng = np.random.default_rng(2)
    eps = rng.standard_normal((B, c["latent"]))
    # real-valued conditions (a one-hot row would leave most condition weights without input); what fp32 holds
    cond = rng.uniform(0.0, 1.0, (B, c["cond"])).astype(np.float32).astype(np.float64)
    return c, opts, uo, vo, ue, ve, X, cond, eps


def _vae_layer_shapes(B, d, C, filters, latent):
    sh, S = {}, d
    for i in range(4):
        sh["e%d" % i] = (B, S, S, S, filters[i]); S //= 2
    sh["e4"] = (B, S, S, S, 4)
    sh["enc_dense"] = (B, latent)
    S = d // 8
    for i in range(4):
        sh["d%d" % i] = (B, S, S, S, filters[3 - i])
        if i < 3:
            S *= 2
    sh["dout"] = (B, d, d, d, C)
    return sh


class _WithoutTap(R.VaeOracle):
    """The oracle with one perceptual tap taken out of the loss altogether (not multiplied by anything)."""
    drop = 1

    def losses(self, x, recon, zm, zlv, training, pm_cache=None):
        x = np.asarray(x, self.dtype)
        h1 = self.unet.pm_forward(x, training, {})
        h2 = self.unet.pm_forward(recon, training, {} if pm_cache is None else pm_cache)
        keep = [i for i in range(4) if i != self.drop]
        pm = R.perceptual_from_taps([h1[i] for i in keep], [h2[i] for i in keep], [self.pm_w[i] for i in keep])
        loss = R.vae_dfc_loss(R.mse_loss(x, recon), pm, R.kld_loss(zm, zlv), self.alpha, self.beta)
        return np.array([loss, pm.mean(), R.mse_loss(x, recon), R.kld_loss(zm, zlv).mean()]), h1, h2


@pytest.mark.parametrize("case", sorted(VAE_CASES))
def test_vae_train_step_at_other_widths(case, relerr):
    """One DFC-VAE train step: [Loss, PM, MSE, KLD], every gradient, the BatchNorm moving statistics, the frozen U-Net --
    the assertions of test_gpu_vae.py::test_vae_train_step_matches_oracle at the configuration VAE_CASES[case]."""
    d = 16
    c, opts, uo, vo, ue, ve, X, cond, eps = _vae_setup(case, d)
    B, C = c["B"], c["C"]
    P0 = {k: v.copy() for k, v in vo.P.items()}                         # the weights of this step (the oracle's own step updates vo.P)
    m = ve.train_step(X, cond, eps)
    shapes = _vae_layer_shapes(B, d, C, c["filters"], c["latent"])
    kink = {n: ve.get_activation(n, s) for n, s in shapes.items()}
    kink_pm = {n: ue.get_activation(n, s) for n, s in _pm_layer_shapes(B, d).items()}
    aff = {n: ve.get_bn_affine(n, shapes[n][-1]) for n in ("e0", "e1", "e2", "e3", "d0", "d1", "d2", "d3", "dout")}
    aff_pm = {n: ue.get_bn_affine(n, _pm_layer_shapes(B, d)[n][-1]) for n in ("c2", "c4", "c6")}
    m_ref = vo.train_on_batch(X, cond, eps, kink=kink, kink_pm=kink_pm, affine=aff, affine_pm=aff_pm)
    flips = sum(vo.kink_flips.values())
    print("case %s: kink_flips %d %s" % (case, flips, {k: v for k, v in vo.kink_flips.items() if v}))
    print("case %s: metrics %s vs %s" % (case, m, m_ref))
    assert flips <= MAX_KINK_FLIPS, vo.kink_flips
    np.testing.assert_allclose(m, m_ref, rtol=METRIC_RTOL)
    if case in ("F", "G"):
        # Loss == MSE + alpha PM + beta KLD (vae/lattice_vae.py:241-255) with the configured constants
        assert abs(m[0] - (m[2] + c["alpha"] * m[1] + c["beta"] * m[3])) <= 2e-5 * abs(m[0])
        assert m[1] > 0 and m[3] > 0
    if case == "F":
        # the tap with weight 0 contributes nothing: the oracle without that tap gives the oracle's numbers with it (true of
        # the oracle by construction).  What holds the ENGINE is the comparison with the run that includes the tap: PM above,
        # and the gradient loop below -- a zero-weight tap leaking into d(recon) would move every decoder and encoder gradient
        without, unit = _WithoutTap(uo, **opts), R.VaeOracle(uo, **dict(opts, pm_layer_weights=(1.0, 1.0, 1.0, 1.0)))
        without.P, unit.P = dict(P0), dict(P0)
        m_without = without.forward_losses(X, cond, eps, True)[0]
        np.testing.assert_allclose(m_without, m_ref, rtol=1e-12)
        np.testing.assert_allclose(m, m_without, rtol=METRIC_RTOL)
        # ... and it is not that the taps are all negligible: unit weights give another PM
        m_unit = unit.forward_losses(X, cond, eps, True)[0]
        assert abs(m_unit[1] - m_ref[1]) > 1e-2 * abs(m_ref[1])
    gscale = max(np.abs(g).max() for g in vo.last_grads.values())
    worst = 0.0
    for name, shape, trainable in ve.tensor_infos():
        if trainable:
            g = ve.get_grad(name, shape)
            # conv biases in front of BatchNorm have exactly-zero true gradient: compare on the scale of the same layer's
            # kernel gradient instead of their own (rounding-noise) scale, as tests/test_gpu_vae.py does
            scale = np.abs(vo.last_grads[name]).max()
            if name.endswith("/bias"):
                scale = max(scale, np.abs(vo.last_grads[name[:-4] + "kernel"]).max())
            err = np.abs(g - vo.last_grads[name]).max() / max(scale, 1e-6 * gscale)
            worst = max(worst, err)
            assert err <= GRAD_TOL, (name, err)
        else:
            assert relerr(ve.get_tensor(name, shape), vo.S[name]) <= BN_TOL, name
    print("case %s: worst gradient error %.2e" % (case, worst))
    # the frozen perceptual U-Net must be untouched (weights AND moving statistics)
    for name, shape, _ in ue.tensor_infos():
        ref = uo.P[name] if name in uo.P else uo.S[name]
        assert relerr(ue.get_tensor(name, shape), ref) <= 1e-7, name


@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E", "H", "I", "J", "K"])
def test_vae_encode_decode_at_other_widths(case, relerr):
    """encode / decode / test_step in eval mode (non-trivial moving statistics): test_gpu_vae.py's
    test_vae_encode_decode_match_oracle at the other widths."""
    c, opts, uo, vo, ue, ve, X, cond, eps = _vae_setup(case)
    rng = np.random.default_rng(3)
    for k in list(vo.S):
        vo.S[k] = (rng.uniform(0.5, 1.5, vo.S[k].shape) if k.endswith("var") else rng.uniform(-0.2, 0.2, vo.S[k].shape))
        if k == "dout/moving_mean":
            # the single output channel ends in a ReLU: a moving mean well below its pre-activations keeps the reference
            # reconstruction from being all zeros (asserted below), whichever way the draw above fell
            vo.S[k] = vo.S[k] - 1.0
        ve.set_tensor(k, vo.S[k])
    zm_r, zlv_r, z_r = vo.predict_encoder(X, cond, eps)
    zm, zlv, z = ve.encode(X, cond, eps)
    assert zm.shape == (c["B"], c["latent"])
    assert relerr(zm, zm_r) <= FWD_TOL and relerr(zlv, zlv_r) <= FWD_TOL and relerr(z, z_r) <= FWD_TOL
    rec_r = vo.predict_decoder(z_r, cond)
    rec = ve.decode(z_r, cond)
    assert rec_r.max() > 0                                             # the ReLU tail lets something through
    assert relerr(rec, rec_r) <= FWD_TOL
    m_r = vo.test_on_batch(X, cond, eps)
    m = ve.test_step(X, cond, eps)
    np.testing.assert_allclose(m, m_r, rtol=METRIC_RTOL)


# ------------------------------------------------------------------------------------------------------------------
# 4. class API round trip
# ------------------------------------------------------------------------------------------------------------------
def test_class_api_checkpoint_round_trip_at_other_shapes(tmp_path):
    """AtomUnet(num_classes=17) and LatticeDFCVAE(filters=(12, 20, 36, 68), latent_dim=100, cond_shape=3): weights saved,
    loaded into a fresh object (vae_param_shapes / unet_param_shapes validate the file), same bits predicted."""
    from icsg3d_amd.unet.unet import AtomUnet
    from icsg3d_amd.vae.lattice_vae import LatticeDFCVAE
    d, B = 16, 2
    X, _, _ = R.synthetic_batch(B, d, 1, seed=0, dtype=np.float32)
    np.random.seed(7)
    unet = AtomUnet(num_classes=17, input_shape=(d, d, d, 1))
    soft, sig = unet.model.predict(X)
    assert soft.shape == (B, d, d, d, 17) and np.all(np.isfinite(soft))
    upath = str(tmp_path / "unet17.h5")
    unet.model.save_weights(upath)
    unet2 = AtomUnet(num_classes=17, weights=upath, input_shape=(d, d, d, 1))
    soft2, sig2 = unet2.model.predict(X)
    assert np.array_equal(soft, soft2) and np.array_equal(sig, sig2)
    with pytest.raises(Exception):                                     # a 17-class file does not fit the default model
        AtomUnet(weights=upath, input_shape=(d, d, d, 1))

    pm = AtomUnet(input_shape=(d, d, d, 1))                            # perceptual U-Net: default 95 classes
    kw = dict(input_shape=(d, d, d, 1), filters=(12, 20, 36, 68), latent_dim=100, cond_shape=3, perceptual_model=pm,
              output_dir=str(tmp_path))
    vae = LatticeDFCVAE(**kw)
    vae._set_model(None, batch_size=B)
    rng = np.random.default_rng(4)
    cond = rng.uniform(size=(B, 3)).astype(np.float32)
    eps = rng.standard_normal((B, 100)).astype(np.float32)
    zm, zlv, z = vae.encoder.predict([X, cond], eps=eps)
    rec = vae.decoder.predict([z, cond])
    assert zm.shape == (B, 100) and rec.shape == (B, d, d, d, 1) and np.all(np.isfinite(rec))
    vpath = str(tmp_path / "vae_odd.h5")
    vae.model.save_weights(vpath)
    vae2 = LatticeDFCVAE(**kw)
    vae2._set_model(vpath, batch_size=B)
    zm2, zlv2, z2 = vae2.encoder.predict([X, cond], eps=eps)
    assert np.array_equal(zm, zm2) and np.array_equal(zlv, zlv2) and np.array_equal(z, z2)
    assert np.array_equal(vae2.decoder.predict([z, cond]), rec)


# ------------------------------------------------------------------------------------------------------------------
# 5. refusals (host-side checks of the create calls) and the smallest accepted sizes
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,word", [({"filters": (16, 0, 64, 128)}, "filters[1]"), ({"filters": (-4, 32, 64, 128)}, "filters[0]"),
                                     ({"filters": (16, 32, 64, 0)}, "filters[3]"), ({"latent_dim": 0}, "latent_dim"),
                                     ({"latent_dim": -256}, "latent_dim"), ({"cond_shape": 0}, "cond_shape"),
                                     ({"in_channels": 0}, "in_channels"), ({"max_batch": 0}, "max_batch"),
                                     # wider than any layer input the convolution launchers read (16384 channels)
                                     ({"filters": (16, 32, 64, 16385)}, "filters[3]"), ({"filters": (20000, 32, 64, 128)}, "filters[0]"),
                                     ({"latent_dim": 16384}, "latent_dim + cond_shape"), ({"latent_dim": 20000}, "latent_dim"),
                                     ({"cond_shape": 16384}, "cond_shape"), ({"in_channels": 4, "cond_shape": 4096}, "cond_shape")])
def test_vae_create_refuses_sizes_out_of_range(kw, word):
    from icsg3d_amd._lib import IcsError
    from icsg3d_amd.engine import VaeEngine
    args = dict(d=16, max_batch=2)
    args.update(kw)
    with pytest.raises(IcsError, match=re.escape(word)):
        VaeEngine(None, **args)


def test_vae_smallest_accepted_sizes_match_the_oracle():
    """The other side of the lower rules above: one filter per stage, latent_dim = cond_shape = max_batch = 1 is accepted,
    and what the create call accepts computes: test_step and train_step metrics against the oracle.  (The upper ends --
    16384 filters, a 16374 x 16374 z_mean kernel -- are gigabytes of parameters and are not built here; the widest layers
    tested are the default engines'.)"""
    from icsg3d_amd.engine import UnetEngine, VaeEngine
    d = 16
    uo = R.UnetOracle(in_ch=1, seed=1)
    ue = UnetEngine(in_channels=1, d=d, max_batch=1)
    ue.set_weights(uo.P)
    vo = R.VaeOracle(uo, in_ch=1, cond=1, filters=(1, 1, 1, 1), latent=1, d=d, seed=3)
    _nonzero_biases(vo)
    ve = VaeEngine(ue, in_channels=1, cond_shape=1, latent_dim=1, filters=(1, 1, 1, 1), d=d, max_batch=1)
    ve.set_weights(vo.P)
    X, _, _ = R.synthetic_batch(1, d, 1, seed=0, dtype=np.float32)
    X = X.astype(np.float64)
    cond, eps = np.ones((1, 1)), np.full((1, 1), 0.5)
    # (the oracle's fp32 restatement of these two calls is within 3.4e-6 of its fp64 one: narrow layers need no wider bound)
    m_t = ve.test_step(X, cond, eps)
    np.testing.assert_allclose(m_t, vo.test_on_batch(X, cond, eps), rtol=METRIC_RTOL)
    m = ve.train_step(X, cond, eps)
    m_ref = vo.train_on_batch(X, cond, eps)
    print("smallest sizes: %s vs %s" % (m, m_ref))
    assert m_ref[1] > 0 and m_ref[2] > 0 and m_ref[3] > 0
    np.testing.assert_allclose(m, m_ref, rtol=METRIC_RTOL)


@pytest.mark.parametrize("ncls", [1, 128])
def test_unet_create_and_head_op_agree_on_the_class_range(ncls):
    """2 .. 127 on both entry points (127 and 2 are trained above): ics_unet_create and ics_op_unet_head refuse the same
    counts, naming the option."""
    from icsg3d_amd._lib import IcsError
    from icsg3d_amd.engine import UnetEngine, unet_head
    with pytest.raises(IcsError, match="num_classes"):
        UnetEngine(in_channels=1, num_classes=ncls, d=16, max_batch=1)
    z = np.zeros
    with pytest.raises(IcsError, match="ncls"):
        unet_head(z((16, 128), np.float32), z((128, ncls), np.float32), z(ncls, np.float32), z(128, np.float32),
                  z(1, np.float32), z(16, np.uint8), mode=0, fused=False)


@pytest.mark.parametrize("kw,word", [({"in_channels": 0}, "in_channels"), ({"max_batch": 0}, "max_batch")])
def test_unet_create_refuses_sizes_below_one(kw, word):
    from icsg3d_amd._lib import IcsError
    from icsg3d_amd.engine import UnetEngine
    args = dict(in_channels=1, d=16, max_batch=1)
    args.update(kw)
    with pytest.raises(IcsError, match=re.escape(word)):
        UnetEngine(**args)
