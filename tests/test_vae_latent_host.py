"""tests/vae_latent_ref.py on the CPU: its KL gradient against central finite differences of numpy_ref.kld_loss, its
backward pass against finite differences of the whole link, the yardsticks e32 and the per-element bounds at every case of
tests/test_gpu_vae_latent.py, and the documented error of float32 numpy's exp that the bounds' floors are built on."""
import numpy as np
import pytest

import vae_latent_ref as VR
from oracle import numpy_ref as R

CASES = [(c, b, r) for c in VR.CASES for b in VR.BETAS for r in VR.LV_REGIMES]


def test_kl_gradient_equals_central_differences_of_kld_loss():
    rng = np.random.default_rng(0)
    B, lat, beta = 3, 5, 0.7
    mu, lv = rng.standard_normal((B, lat)), rng.uniform(-3, 2, (B, lat))
    loss = lambda m, l: beta * R.kld_loss(m, l).mean()
    gmu, glv = VR.kl_grad(mu, lv, beta, B)
    h = 1e-6
    for g, which in ((gmu, 0), (glv, 1)):
        fd = np.zeros_like(mu)
        for i in np.ndindex(B, lat):
            d = np.zeros_like(mu)
            d[i] = h
            fd[i] = (loss(mu + d * (which == 0), lv + d * (which == 1)) - loss(mu - d * (which == 0), lv - d * (which == 1))) / (2 * h)
        assert np.abs(fd - g).max() <= 1e-8 * max(np.abs(g).max(), 1.0), which


def test_backward_equals_central_differences_of_the_link():
    """L = sum(zc * G) + beta mean_b KLD_b with a fixed G: dh, dW, dbias of the reference against finite differences"""
    c = VR.make_case(2, 4, 3, "spread", seed=1)
    c = {k: np.asarray(v, np.float64) for k, v in c.items()}
    c["b_lv"] = np.array([-2.0, 0.5, 1.0, -0.3])
    beta, G = 0.4, c["dzc"]

    def loss(cc):
        f = VR.forward(cc)
        return (f["zc"] * G).sum() + beta * R.kld_loss(f["mulv"][:, :4], f["mulv"][:, 4:]).mean()

    b = VR.backward(VR.forward(c), c, beta)
    db = np.concatenate([b["dbias"][:4], b["dbias"][4:]])
    for name, got in (("h", b["dh"]), ("w_mean", b["dw_mean"]), ("w_lv", b["dw_lv"]), ("b_mean", db[:4]), ("b_lv", db[4:])):
        fd = np.zeros_like(c[name])
        for i in np.ndindex(*c[name].shape):
            p, m = dict(c), dict(c)
            d = np.zeros_like(c[name])
            d[i] = 1e-6
            p[name], m[name] = c[name] + d, c[name] - d
            fd[i] = (loss(p) - loss(m)) / 2e-6
        assert np.abs(fd - got).max() <= 1e-7 * max(np.abs(got).max(), 1.0), name


def test_float32_exp_is_within_its_documented_error():
    """the floors of the per-element bounds rest on EXP_ULPS; measured here: 2.35 ulps over [-10, 4] and its halves"""
    x = np.linspace(-10.0, 4.0, 400001).astype(np.float32)
    for s in (np.float32(1.0), np.float32(0.5)):
        got, ref = np.exp(s * x), np.exp(np.float64(s) * x.astype(np.float64))
        err = (np.abs(got.astype(np.float64) - ref) / np.spacing(ref.astype(np.float32))).max()
        print("float32 exp: %.3f ulps" % err)
        assert err <= VR.EXP_ULPS


@pytest.mark.parametrize("case,beta,regime", CASES, ids=lambda v: str(v))
def test_yardsticks_are_finite_and_nonzero(case, beta, regime):
    B, lat, nc = case
    c = VR.make_case(B, lat, nc, regime, seed=VR.CASES.index(case))
    ref, e32 = VR.reference(c, beta)
    lv = ref["mulv"][:, lat:]
    if regime == "small":
        assert np.abs(lv).max() <= 0.2
    elif lat > 1:
        assert lv.min() < -9 and lv.max() > 3
    for k, e in e32.items():
        # (1, 1, 1): h is one relu output; where it is zero every product with it is exact in any format
        assert np.isfinite(e) and (e > 0 or lat == 1) and e < 1e-4, (k, e)
    assert ref["zc"].shape == (B, lat + nc) and np.array_equal(ref["zc"][:, lat:], c["cond"].astype(np.float64))
    # the per-element bounds on the float32 evaluation's own mulv: finite, positive, and the float32 formulas sit inside
    mulv32 = VR.forward(c, np.float32)["mulv"]
    for k, (val, bound) in VR.elementwise(mulv32, c["eps"], c["dzc"][:, :lat], beta).items():
        assert np.isfinite(val).all() and np.isfinite(bound).all() and (bound > 0).all(), k
