"""tests/conv_link_ref.py on the CPU: (1) it reproduces sub-chains of numpy_ref.UnetOracle / VaeOracle, forward and
backward, to 1e-12: c3 -> c4 (same), c2 -> {c3, c17} (pool_skip), e0 -> e1 (pool, VAE form), d1 -> up -> d2 (up, VAE
form); (2) the folds' algebra -- 26 class sums -> S_t, sum W S_t, sum W G, gamma G + beta S_t, and the pool share sum k g,
sum g (ssum - k mean) rstd -- equals the plain formulas in fp64 to 1e-12, also at S = 4 where the interior is two planes;
(3) e32, the PLAIN formulas in float32 against the fp64 reference with the reference's decisions, and a float32 emulation
of the folded path (G and the class partials in float32, the constants through fp64, the apply relu'(s) fma(a, d, fma(b, s,
c)) in float32) next to max(1e-5, 2 e32) in every regime test_gpu_conv_link.py runs; (4) that the decisions a float32
evaluation takes differ from the fp64 reference's at no more than 8 activation sides and 8 pool windows per tensor, for the
seeds of the GPU cases.

Measured here (test_fold_emulation_against_the_yardstick, -s prints the table; (2, 8, 16 -> 64 -> 64), U-Net form; L.dw, dy_p,
P.dgamma, P.dbeta): the fold emulation is within 3 % of e32 in every regime, i.e. at 0.39 .. 0.51 of max(1e-5, 2 e32):
    P ordinary, dout normal   5.3e-6, 4.7e-6, 3.9e-6, 6.3e-6      dout mean 30   1.1e-4, 1.6e-5, 3.2e-5, 3.0e-4
    P mean/std 30             3.3e-5, 9.8e-6, 8.1e-6, 3.0e-5                     2.6e-4, 1.5e-5, 2.3e-5, 3.6e-4
    P mean/std 1000           8.6e-4, 4.5e-4, 4.7e-4, 1.2e-3                     8.3e-4, 4.5e-4, 4.8e-4, 1.2e-3
Decisions of a float32 numpy evaluation against the fp64 reference, data of the GPU cases: <= 2 sides per layer and 0 pool
windows in the ordinary and mean/std = 30 regimes; up to 27 consumer sides at mean/std = 1000 (printed, not asserted)."""
import numpy as np
import pytest

import conv_layer_ref as CR
import conv_link_ref as LR
from oracle import numpy_ref as R

TOL = 1e-12


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def _params(P, name):
    return {"w": P[name + "/kernel"], "bias": P[name + "/bias"], "gamma": P[name + "/gamma"], "beta": P[name + "/beta"]}


def _check_layer(b, grads, name):
    for k, suffix in (("dw", "/kernel"), ("dbias", "/bias"), ("dgamma", "/gamma"), ("dbeta", "/beta")):
        assert _rel(b[k], grads[name + suffix]) <= TOL, (name, k)


@pytest.fixture(scope="module")
def unet_cache():
    o = R.UnetOracle(in_ch=1, num_classes=95, seed=1)
    x, _, _ = R.synthetic_batch(1, 16, 1, seed=0)
    cache = {}
    o._trunk(np.asarray(x, np.float64), True, cache)
    return o, cache


def test_reference_reproduces_unet_c3_c4(unet_cache):
    o, cache = unet_cache
    rng = np.random.default_rng(0)
    d = {"link": "same", "form": "unet", "x0": cache["c3"]["x"], "layers": {"P": _params(o.P, "c3"), "L": _params(o.P, "c4")}}
    d["dout"] = rng.standard_normal(cache["c4"]["bn"].shape)
    f = LR.link_forward(d, eps=R.BN_EPS)
    assert _rel(f["P"]["y"], cache["c3"]["s"]) <= TOL and _rel(f["L"]["y"], cache["c4"]["s"]) <= TOL
    assert _rel(f["L"]["bn"], cache["c4"]["bn"]) <= TOL
    b = LR.link_backward(d, f)
    grads = {}
    dx = o.blocks["c3"].bwd(o.blocks["c4"].bwd(d["dout"], o.P, {}, cache, grads), o.P, {}, cache, grads)
    _check_layer(b["P"], grads, "c3")
    _check_layer(b["L"], grads, "c4")
    assert _rel(b["dx0"], dx) <= TOL and b["pinned"] == {"P": 0, "L": 0}


@pytest.mark.parametrize("ties", ["tf_cpu", "first"])
def test_reference_reproduces_unet_c2_to_c3_and_c17(unet_cache, ties):
    o, cache = unet_cache
    rng = np.random.default_rng(1)
    d = {"link": "pool_skip", "form": "unet", "x0": cache["c2"]["x"], "q": cache["c16"]["bn"],
         "layers": {"P": _params(o.P, "c2"), "K": _params(o.P, "c3"), "L": _params(o.P, "c17")}}
    d["dout"] = rng.standard_normal(cache["c3"]["bn"].shape)
    d["dout_l"] = rng.standard_normal(cache["c17"]["bn"].shape)
    f = LR.link_forward(d, eps=R.BN_EPS)
    for n, name in (("P", "c2"), ("K", "c3"), ("L", "c17")):
        assert _rel(f[n]["y"], cache[name]["s"]) <= TOL and _rel(f[n]["bn"], cache[name]["bn"]) <= TOL
    assert _rel(f["pooled"], cache["_o"]["p1"]) <= TOL
    b = LR.link_backward(d, f, ties=ties)
    grads = {}
    d17 = o.blocks["c17"].bwd(d["dout_l"], o.P, {}, cache, grads)
    d3 = o.blocks["c3"].bwd(d["dout"], o.P, {}, cache, grads)
    dO = R.maxpool_bwd(cache["_o"]["c2"], cache["_o"]["p1"], d3, ties) + d17[..., :64]
    dx = o.blocks["c2"].bwd(dO, o.P, {}, cache, grads)
    for n, name in (("P", "c2"), ("K", "c3"), ("L", "c17")):
        _check_layer(b[n], grads, name)
    assert _rel(b["dO_P"], dO) <= TOL and _rel(b["dx0"], dx) <= TOL and b["rerouted"] == 0


@pytest.fixture(scope="module")
def vae_oracle():
    return R.VaeOracle(None, d=16)


def test_reference_reproduces_vae_e0_e1(vae_oracle):
    v = vae_oracle
    rng = np.random.default_rng(2)
    cache = {}
    x, _, _ = R.synthetic_batch(2, 16, 1, seed=1)
    v.encode(np.asarray(x, np.float64), rng.standard_normal((2, 10)), rng.standard_normal((2, 256)), True, cache)
    d = {"link": "pool", "form": "vae", "x0": cache["e0"]["x"], "layers": {"P": _params(v.P, "e0"), "K": _params(v.P, "e1")}}
    d["dout"] = rng.standard_normal(cache["e1"]["bn"].shape)
    f = LR.link_forward(d, eps=R.BN_EPS)
    assert _rel(f["P"]["y"], cache["e0"]["s"]) <= TOL and _rel(f["K"]["bn"], cache["e1"]["bn"]) <= TOL
    o0, p0 = cache["_pool"][0]
    assert _rel(f["pooled"], p0) <= TOL
    b = LR.link_backward(d, f)
    grads = {}
    d1 = v.enc[1].bwd(d["dout"], v.P, {}, cache, grads)
    dx = v.enc[0].bwd(R.maxpool_bwd(o0, p0, d1, "tf_cpu"), v.P, {}, cache, grads)
    _check_layer(b["P"], grads, "e0")
    _check_layer(b["K"], grads, "e1")
    assert _rel(b["dx0"], dx) <= TOL


def test_reference_reproduces_vae_d1_up_d2(vae_oracle):
    v = vae_oracle
    rng = np.random.default_rng(3)
    cache = {}
    v.decode(rng.standard_normal((2, 256)), rng.standard_normal((2, 10)), True, cache)
    d = {"link": "up", "form": "vae", "x0": cache["d1"]["x"], "layers": {"P": _params(v.P, "d1"), "L": _params(v.P, "d2")}}
    d["dout"] = rng.standard_normal(cache["d2"]["bn"].shape)
    f = LR.link_forward(d, eps=R.BN_EPS)
    assert _rel(f["L"]["V"], cache["d2"]["x"]) <= TOL and _rel(f["L"]["bn"], cache["d2"]["bn"]) <= TOL
    b = LR.link_backward(d, f)
    grads = {}
    d2 = v.dec[2].bwd(d["dout"], v.P, {}, cache, grads)
    dx = v.dec[1].bwd(R.upsample_bwd(d2), v.P, {}, cache, grads)
    _check_layer(b["P"], grads, "d1")
    _check_layer(b["L"], grads, "d2")
    assert _rel(b["dx0"], dx) <= TOL


@pytest.mark.parametrize("S", [4, 8])
def test_fold_algebra_equals_the_plain_formulas(S):
    """the linear fold of a same-resolution consumer and the pool share, in fp64, against link_backward"""
    d = LR.make_link("pool_skip", "unet", 2, S, 8, 16, Ck=8, Cl=12, Cq=8, seed=S, dout_regime="mean30")
    f, b, _ = LR.reference(d)
    dyL = LR._dy_of(f["L"], d["layers"]["L"], d["dout_l"], "unet", None)
    Rc = LR.class_sums(dyL)
    assert _rel(LR.tap_sums(Rc), LR.tap_sums_direct(dyL)) <= TOL
    wL = d["layers"]["L"]["w"][..., :16, :]
    fo = LR.fold_same(f["P"], d["layers"]["P"], wL, dyL)
    dL = b["L"]["dx"][0]
    xhat = (f["P"]["s"] - f["P"]["mean"]) * f["P"]["rstd"]
    assert _rel(fo["d"], dL) <= TOL
    assert _rel(fo["sum_d"], dL.sum(axis=(0, 1, 2, 3))) <= TOL
    assert _rel(fo["sum_dxhat"], (dL * xhat).sum(axis=(0, 1, 2, 3))) <= TOL
    assert _rel(fo["dW_L"], b["L"]["dw"][..., :16, :]) <= TOL          # gamma G + beta S_t, gamma < 0, = 0 and << beta included
    # the pool share on the pooled grid, both tie rules; channel 1 (gamma = 0) ties in all eight elements
    for ties in ("tf_cpu", "first"):
        mask = LR._routing_mask(f["P"]["o"], ties)
        assert ties == "first" or mask[..., 1].all()
        g = b["K"]["dx"][0]
        dpool = R.maxpool_bwd(f["P"]["o"], f["pooled"], g, ties)
        sd, sq = LR.pool_share(f["P"], g, mask)
        assert _rel(sd, dpool.sum(axis=(0, 1, 2, 3))) <= TOL
        assert _rel(sq, (dpool * xhat).sum(axis=(0, 1, 2, 3))) <= TOL
        # both consumers together: P's dbeta and dgamma
        bt = LR.link_backward(d, f, ties=ties)
        assert _rel(fo["sum_d"] + sd, bt["P"]["dbeta"]) <= TOL and _rel(fo["sum_dxhat"] + sq, bt["P"]["dgamma"]) <= TOL
    # same link: the apply from the constants equals the plain dy
    d2 = LR.make_link("same", "unet", 2, S, 8, 16, Cl=12, seed=S + 1)
    f2, b2, _ = LR.reference(d2)
    dy2 = LR._dy_of(f2["L"], d2["layers"]["L"], d2["dout"], "unet", None)
    fo2 = LR.fold_same(f2["P"], d2["layers"]["P"], d2["layers"]["L"]["w"], dy2)
    assert _rel(fo2["dy_p"], b2["dy_p"]) <= TOL and _rel(fo2["dW_L"], b2["L"]["dw"]) <= TOL
    assert _rel(fo2["sum_d"], b2["P"]["dbeta"]) <= TOL and _rel(fo2["sum_dxhat"], b2["P"]["dgamma"]) <= TOL


EMU = {}


@pytest.mark.parametrize("dout_regime", LR.DOUT_REGIMES)
@pytest.mark.parametrize("p_regime", LR.P_REGIMES, ids=str)
def test_fold_emulation_against_the_yardstick(p_regime, dout_regime):
    """e32 (plain formulas, float32) and the float32 emulation of the fold, both against the fp64 reference with its own
    decisions.  Asserted: the emulation is inside max(1e-5, 2 e32) in all three regimes of P's output and both of dout
    (mean/std = 1000 included), so the GPU bound is reachable by a correct float32 fold everywhere it is applied."""
    d = LR.make_link("same", "unet", 2, 8, 16, 64, Cl=64, seed=11, p_regime=p_regime, dout_regime=dout_regime)
    f64, b64, t64 = LR.reference(d)
    e32 = LR.e32_of(d, f64, t64)
    f32 = LR.link_forward(d, np.float32)
    pins = LR.pins_of_forward(f64, "unet")
    dyL = LR._dy_of(f32["L"], d["layers"]["L"], d["dout"], "unet", pins["L"])
    fP = dict(f32["P"], s=f32["P"]["s"])
    fo = LR.fold_same(fP, d["layers"]["P"], d["layers"]["L"]["w"], dyL, np.float32)
    fo["dy_p"] = fo["dy_p"] * ((f64["P"]["y"] > 0) == (f32["P"]["y"] > 0))      # the reference's decisions
    got = {"L.dw": fo["dW_L"], "dy_p": fo["dy_p"], "P.dgamma": fo["sum_dxhat"], "P.dbeta": fo["sum_d"]}
    ref = {k: t64[k] for k in got}
    err = LR.rel_errors(got, ref, "unet")
    worst = 0.0
    for k in sorted(err):
        lim = max(1e-5, 2 * e32[k])
        worst = max(worst, err[k] / lim)
        print("  P %-9s dout %-6s %-8s fold emulation %.3g  e32 %.3g  bound %.3g" % (p_regime, dout_regime, k, err[k], e32[k], lim))
        EMU[(str(p_regime), dout_regime, k)] = (err[k], e32[k])
    assert worst <= 1.0, (p_regime, dout_regime, err, e32)


def test_float32_decisions_stay_inside_the_caps():
    """the data of test_gpu_conv_link.py's cases (same seeds): a float32 evaluation of the plain formulas decides at most 8
    activation sides per layer and routes at most 8 pool windows differently from the fp64 reference, in every regime"""
    import test_gpu_conv_link as G
    worst_p = worst_r = 0
    for name, form, ties in G.VARIANTS:
        for p_regime, dout_regime in G.REGIMES:
            if dout_regime != "normal" and G.CASES[name]["link"] in ("same", "up"):
                continue                                    # the decisions do not depend on dout
            d = G._data(name, form, p_regime, dout_regime)
            f64 = LR.link_forward(d)
            f32 = LR.link_forward(d, np.float32)
            pins = LR.pins_of_forward(f32, form)
            kw = LR.FORM_KW[form]                           # the sides that matter: y behind a pre-activation, bn in front of a post-activation
            pinned = {n: int(((pins[n]["y"] > 0) != (f64[n]["y"] > 0)).sum() * bool(kw["pre_act"])
                             + ((pins[n]["bn"] > 0) != (f64[n]["bn"] > 0)).sum() * bool(kw["post_act"]))
                      for n in LR.layer_names(d["link"])}
            rerouted = 0
            if "K" in d["layers"]:
                t = "tf_cpu" if ties else "first"
                rerouted = int((LR._routing_mask(pins["P"]["route"], t) != LR._routing_mask(f64["P"]["o"], t)).any(axis=4).sum())
            if p_regime == "ratio1000":
                # a consumer's y next to zero: numpy's float32 convolution of P (running sums at magnitude 1000) moves
                # o_P by several 1e-5 and flips a few dozen of them -- printed, not asserted; the GPU test asserts the cap
                # on the engine's own decisions in this regime too (its P.y carries one rounding, not a sum's worth)
                print("  %s %s ties=%d mean/std 1000: float32 numpy decides %s sides, %d windows differently"
                      % (name, form, ties, pinned, rerouted))
                continue
            worst_p, worst_r = max(worst_p, max(pinned.values())), max(worst_r, rerouted)
            assert max(pinned.values()) <= G.CAP and rerouted <= G.CAP, (name, form, ties, p_regime, pinned, rerouted)
    print("  ordinary and mean/std 30, worst: %d pinned activation sides in a layer, %d rerouted pool windows" % (worst_p, worst_r))
