"""BatchNorm backward ACROSS layer links (ics_op_conv_link) against the fp64 reference of tests/conv_link_ref.py: the
consumer-side folds of the producer's BatchNorm backward (BwdStat in conv_wino / conv_wino64 / conv_fwd_kernel and the
up-split dxl launch; conv_bnfuse_kernel + FOLD = 2; pool_bnfuse_kernel + FOLD = 3), the pool / upsample gradient sources of
the BatchNorm-backward kernels, launch_pool_presum and pool_fwd4_kernel's tie masks.  Every case asserts the
profiler rows the op returns (launch sites and the kernel id of every conv launch), so a dispatch change cannot turn it
into a test of another path.

link -> what conv_backward gets, as unet_backward gives it (DESIGN.md section 22 has the same tables):
  same       P -> L                  L: gs_direct(dout), next = P;  P: gs_direct(L.dA)
  up         P -> up -> L            L up-split: next = P, P: gs_direct(L.dxl);  ICSG3D_NO_UPSPLIT: P: gs_up(L.dA)
  pool       P -> MaxPool -> K       K: gs_direct(dout);  P: gs_pool(K.dA), gs_none()
  pool_skip  P -> MaxPool -> K, L = [P | up(q)], L.skip_prod = P     L, K, then P: gs_pool(K.dA), g_skip(L)
Cases: CASES below (B, S of P, C0 -> P -> consumers); expected rows per case and switch: expected_sites, written from the
predicates of engine.hip.  Deviations from the planned table, each because a predicate decides otherwise:
  * (2, 8, 40 -> 24) does not take conv_fwd_kernel's FOLD = true: the fold needs vector loads of the backward-data source,
    dy, i.e. 24 % 32 == 0.  It stays, asserting ", false>" and the separate pass; (2, 8, 72 -> 32) is added and asserts
    ", true>" (dy 32 wide; the Winograd kernels refuse 72 input channels; Npad = 96 keeps the 128-row tile: no split-K).
  * (2, 8, P 96 -> L 32) IS accepted by conv_bnfuse_ok (its width limits are on N = 32, the consumer's outputs): the case
    asserts conv_wino_kernel<false, true, 1> by default and bnfuse:L + <false, true, 2> under ICSG3D_DGRAD_BNFUSE_MIN=0.
  * up (2, 8 <- 4, 64 -> 64): the dxl GEMM (K = 27 x 64) splits K at this size and refuses the fold (", false>");
    up (32 -> 16) takes it (", true>").
  * The VAE engine's own backward pass hands no `next` to conv_backward and vae_build does not enable the Winograd kernels:
    the op builds both forms the U-Net's way, so the VAE-form same / up cases run the post_act' branches of the FOLD = 1
    epilogues, which no train step reaches today.  pool in the VAE form is the encoder's e(i) -> e(i+1) as it is.
  * conv_layer_ref.check_bn_affine recovers the mean from the affine, which gamma = 0 and |beta| >> |gamma| do not allow:
    its bounds (MEAN_ULPS, var_bound, 1 ulp on scale and shift) are applied to the returned mean / rstd of every layer.
P's gamma / beta (conv_link_ref.make_link): channel 0 gamma < 0, channel 1 gamma = 0, channel 2 gamma = 0.01 and beta = 3,
a quarter of the rest negative.  Regimes: P's output ordinary / every channel at mean/std ~ 30 / ~ 1000, times dout standard
normal / columns with mean 30x their std.  Switches: each on top of ICSG3D_DGRAD_BNFUSE_MIN=0, in two regimes.

Bounds (none taken from what the kernels give):
  y            P against the fp64 reference, K / L against the fp64 convolution of what they read (the op's own fp32
               affine, activation and pool of P's stored y): tensor-relative 1e-5
  statistics   mean 4 float32 ulps of max(|mean|, std), var + eps conv_layer_ref.var_bound, scale / shift 1 ulp, per channel,
               against fp64 statistics of the layer's own stored y
  pooled       1 float32 ulp of the window maximum of post_act(fmaf(y, scale, shift)) of the op's own numbers
  gradients    dy_p, dx0 and dw / dbias / dgamma / dbeta of every layer: tensor-relative max(1e-5, 2 e32), e32 = the PLAIN
               formulas in float32 numpy against the fp64 reference with the reference's decisions, per case and regime;
               asserted in all six regimes (tests/test_conv_link_host.py: a float32 emulation of the fold sits at 0.39 ..
               0.51 of this bound in each, mean/std = 1000 included)
  decisions    <= 8 pinned activation sides per layer, <= 8 pool windows routed differently from the fp64 reference

Measured on the MI355X, worst over all cases, regimes and switches (engine | bound there):
  y P 7.2e-7, K 8.6e-7, L 1.5e-6 | 1e-5        mean 1.61 ulps | 4        var + eps 0.157 of its bound
  dy_p 2.99e-6 | 1e-5    dx0 6.3e-5 | 3.0e-4 (mean/std 1000)    P.dw 2.8e-6 | 1e-5    P.dbias 2.1e-5 | 2.9e-5 (dout mean 30)
  P.dgamma 9.5e-5 | 3.4e-4 (1000)    P.dbeta 4.0e-6 | 1.5e-5    K.dw 3.5e-6 | 1e-5    K.dbias 2.8e-4 | 8.0e-4 (1000, mean 30)
  K.dgamma 1.6e-5 | 7.4e-5    L.dw 3.75e-6 | 1e-5    L.dbias 2.2e-6 | 1e-5    L.dgamma 3.3e-6 | 1.03e-5    L.dbeta 1.5e-7 | 1e-5
  ordinary regime, normal dout: every tensor <= 6.8e-6.  Pinned sides <= 5 in a layer, rerouted pool windows 0.
  No kernel was wrong.
Mutations, each in a scratch copy, the whole file against the mutated library (483 tests):
  * tap_valid_for_class with the last-plane test on the centre tap: 93 fail -- same 64 -> 128, 128 -> 128, 96 -> 32 (U-Net
    form) and both pool_skip cases wherever a linear fold runs (test_link_with_the_linear_folds_on in all six regimes,
    test_link_under_switch under every switch but ICSG3D_NO_DGRAD_BNFUSE, the canary runs with the folds): L.dw off by
    0.43, dy_p 5.5e-3, dx0 1.1e-2.  The 390 others pass (default switches, VAE form, refused folds).
  * pool_sums_kernel with k = 1: 47 fail -- pool 64 (the pre-sum, also by default) and both pool_skip cases with the folds
    on, under the tie rule "all" only: P.dbeta off by 0.875 (7/8 of the gamma = 0 channel), dy_p 1.3e-2.  436 pass, among
    them the same cases under "first" (k = 1 there) and pool 64 under ICSG3D_NO_POOL_PRESUM.
  * conv_wino64's FOLD = 1 epilogue without post_act': 42 fail -- same 64 -> 128 and 128 -> 128 in the VAE form wherever
    the fold is taken: P.dbeta off by 0.75, dy_p 2.2e-2.  441 pass, among them those cases under ICSG3D_NO_BWD_FOLD.
  * conv_bnfuse_kernel writing gamma G without beta S_t: the 93 tests of the first mutation fail, by L.dw alone (0.58).
Run time of this file on the MI355X machine: 18.6 s (483 tests; the slowest 0.34 s; the fp64 references take 13 s of it)."""
import contextlib
import functools
import os

import numpy as np
import pytest

import conv_layer_ref as CR
import conv_link_ref as LR
from oracle import numpy_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-5
CAP = 8                    # pinned activation decisions per layer, rerouted pool windows per tensor
FUSED = "ICSG3D_DGRAD_BNFUSE_MIN"


def case(link, forms, B, S, C0, Cp, Ck=0, Cl=0, Cq=0, ties=(1,)):
    """S: P's grid (the consumer of an "up" link works on 2S)"""
    return dict(link=link, forms=forms, kw=dict(B=B, S=S, C0=C0, Cp=Cp, Ck=Ck, Cl=Cl, Cq=Cq), ties=ties)


BOTH, UNET, VAE = ("unet", "vae"), ("unet",), ("vae",)
CASES = {
    "same_64_128": case("same", BOTH, 3, 8, 16, 64, Cl=128),          # c4 -> c3
    "same_128_128": case("same", BOTH, 2, 8, 16, 128, Cl=128),        # c18 -> c17
    "same_96_32": case("same", UNET, 2, 8, 16, 96, Cl=32),            # conv_wino_kernel, the 32-channel tile
    "same_winog": case("same", UNET, 4, 4, 16, 64, Cl=64),            # conv_winog: no fold, the separate pass
    "same_igemm": case("same", UNET, 2, 8, 16, 40, Cl=24),            # conv_fwd_kernel, dy 24 wide: no vector loads, no fold
    "same_splitk": case("same", UNET, 3, 4, 16, 128, Cl=40),          # split-K refuses the fold
    "up_64_64": case("up", BOTH, 2, 4, 16, 64, Cl=64),
    "up_32_16": case("up", BOTH, 2, 4, 16, 32, Cl=16),
    "pool_64": case("pool", UNET, 3, 8, 16, 64, Ck=64, ties=(1, 0)),  # launch_pool_presum
    "pool_16": case("pool", VAE, 2, 8, 16, 16, Ck=32, ties=(1, 0)),   # post_act LeakyReLU: the reduce kernels
    "pool_skip_64": case("pool_skip", UNET, 2, 8, 16, 64, Ck=64, Cl=128, Cq=128, ties=(1, 0)),     # c2 -> {c3, c17}
    "pool_skip_c4": case("pool_skip", UNET, 1, 8, 16, 128, Ck=128, Cl=256, Cq=256, ties=(1, 0)),   # c4 -> {c5, c15}
    "same_igemm_fold": case("same", UNET, 2, 8, 16, 72, Cl=32),       # conv_fwd_kernel FOLD = true (added, see the header)
}
VARIANTS = [(n, f, t) for n, c in CASES.items() for f in c["forms"] for t in c["ties"]]
REGIMES = [(p, g) for p in LR.P_REGIMES for g in LR.DOUT_REGIMES]
SWITCHES = ("ICSG3D_NO_DGRAD_BNFUSE", "ICSG3D_NO_BWD_FOLD", "ICSG3D_NO_FAST_BNBWD", "ICSG3D_NO_POOL_PRESUM", "ICSG3D_NO_UPSPLIT")

W64 = "conv_wino64_kernel<false, true, %d>"
W32 = "conv_wino_kernel<false, true, %d>"


# conv_fwd_kernel<.., FOLD> as the backward-data launch that could carry the producer's sums: does it (default switches)?
IGEMM_FOLD = {"same_igemm": False, "same_igemm_fold": True, "same_splitk": False, "up_64_64": False, "up_32_16": True}


def _dgrad_kernel(name):
    """the backward-data kernel of the consumer whose epilogue carries the fold, by case: fragment with the FOLD slot open"""
    return {"same_64_128": W64, "same_128_128": W64, "same_96_32": W32, "pool_skip_64": W64, "pool_skip_c4": W64}.get(name)


def expected_sites(name, form, env):
    """(present, absent): fragments of profiler rows.  Derived from the predicates of engine.hip (dgrad_bnfuse_ok,
    skip_bnfuse_ok, bwd_stat_for, the presum condition of conv_backward, enable_split_up), not from a run."""
    c = CASES[name]
    link = c["link"]
    fused = FUSED in env and "ICSG3D_NO_DGRAD_BNFUSE" not in env and form == "unet"
    fold = "ICSG3D_NO_BWD_FOLD" not in env
    have, lack = ["conv_fwd:P|", "conv_wgrad:P|", "conv_dgrad:P|"], []
    if link == "same":
        k = _dgrad_kernel(name)
        if k is not None and fused:
            have += ["bnfuse:L", "conv_dgrad:L|" + k % 2]
            lack += ["bn_act_bwd:P"]
        else:
            lack += ["bnfuse:"]
            have += ["bn_act_bwd:P"]
            if k is not None:
                have += ["conv_dgrad:L|" + k % (1 if fold else 0)]
            elif name == "same_winog":
                have += ["conv_dgrad:L|conv_winog"]
            else:
                have += ["conv_dgrad:L|conv_fwd_kernel<"]
                (have if IGEMM_FOLD[name] and fold else lack).append("true>")
    elif link == "up":
        have += ["bn_act_bwd:P"]
        if "ICSG3D_NO_UPSPLIT" in env:
            have += ["conv_dgrad:L|"]
            lack += ["conv_dgrad:L.up|"]
        else:
            have += ["conv_dgrad:L.up|conv_fwd_kernel<"]
            (have if IGEMM_FOLD[name] and fold else lack).append("true>")
    elif link == "pool":
        have += ["pool_fwd", "bn_act_bwd:P"]
        if form == "unet" and "ICSG3D_NO_POOL_PRESUM" not in env:
            have += ["pool_presum:P"]
        else:
            lack += ["pool_presum:"]
    else:
        have += ["pool_fwd"]
        lack += ["pool_presum:"]
        if "ICSG3D_NO_UPSPLIT" in env:
            have += ["conv_dgrad:L|", "bn_act_bwd:P"]
            lack += ["bnfuse:", "conv_dgrad:L.skip|"]
        elif fused:
            have += ["bnfuse:L.skip", "bnfuse:P.pool", "conv_dgrad:L.skip|" + W64 % 3]
            lack += ["bn_act_bwd:P"]
        else:
            have += ["conv_dgrad:L.skip|" + W64 % 0, "bn_act_bwd:P"]
            lack += ["bnfuse:"]
    return have, lack


def _seed(name):
    return list(CASES).index(name)


@functools.lru_cache(maxsize=None)
def _data(name, form, p_regime, dout_regime, B=None):
    c = CASES[name]
    kw = dict(c["kw"], B=B or c["kw"]["B"])
    return LR.make_link(c["link"], form, seed=_seed(name), p_regime=p_regime, dout_regime=dout_regime, **kw)


@functools.lru_cache(maxsize=None)
def _reference(name, form, p_regime, dout_regime, ties, B=None):
    """fp64 forward / backward with the reference's own decisions, its gradient tensors, and e32 -- once per case and regime"""
    d = _data(name, form, p_regime, dout_regime, B)
    t = "tf_cpu" if ties else "first"
    f, b, t64 = LR.reference(d, ties=t)
    return f, b, t64, LR.e32_of(d, f, t64, ties=t)


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _envdict(names):
    return {n: ("0" if n == FUSED else "1") for n in names}


def _run(name, form, ties, env=(), p_regime=None, dout_regime="normal", B=None, max_batch=None):
    from icsg3d_amd import engine as E
    d = _data(name, form, p_regime, dout_regime, B)
    with _env(_envdict(env)):
        return E.conv_link(d["link"], d["x0"], d["layers"], d["dout"], form=form, q=d.get("q"), dout_l=d.get("dout_l"),
                           pool_ties_all=bool(ties), max_batch=max_batch)


WORST = {}


def _note(key, err, yard, what):
    if key not in WORST or err / max(yard, 1e-300) > WORST[key][0] / max(WORST[key][1], 1e-300):
        WORST[key] = (err, yard, what)


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(np.abs(b).max(), 1e-300))


def _check_sites(r, name, form, env, what):
    text = "\n".join(r["sites"])
    have, lack = expected_sites(name, form, env)
    for frag in have:
        if frag == "true>":
            assert any(ln.startswith("conv_dgrad:L") and ln.endswith(frag) for ln in r["sites"]), (what, "no FOLD launch", r["sites"])
            continue
        assert frag in text, (what, "missing", frag, r["sites"])
    for frag in lack:
        rows = [ln for ln in r["sites"] if frag in ln and (frag != "true>" or ln.startswith("conv_dgrad:L"))]
        assert not rows, (what, "unexpected", frag, rows)


def _check_stats(o, p, what):
    """statistics and affine of one layer against fp64 statistics of its OWN stored y, with conv_layer_ref's bounds (the
    checks of conv_layer_ref.check_bn_affine, on the returned mean / rstd: P's gamma = 0 and |beta| >> |gamma| channels do not
    let the mean be recovered from the affine)"""
    m64, v64 = CR.channel_stats(o["y"])
    mu = CR.ulps32(o["mean"], m64, at=np.maximum(np.abs(m64), np.sqrt(v64)))
    ve = CR.var_error(1.0 / o["rstd"].astype(np.float64) ** 2, v64)
    bound = CR.var_bound(m64, v64)
    _note("mean ulps", float(mu.max()), CR.MEAN_ULPS, what)
    _note("var+eps / bound", float((ve / bound).max()), 1.0, what)
    assert (mu <= CR.MEAN_ULPS).all(), (what, "mean", mu.max(), int(mu.argmax()))
    assert (ve <= bound).all(), (what, "var + eps", ve.max(), int((ve / bound).argmax()))
    u = CR.ulps32(o["scale"], p["gamma"] * o["rstd"])
    assert (u <= 1).all(), (what, "scale", u.max())
    prod = o["mean"].astype(np.float64) * o["scale"].astype(np.float64)
    sh = p["beta"].astype(np.float64) - prod
    u = CR.ulps32(o["shift"], sh, at=np.maximum(np.abs(sh), np.maximum(np.abs(prod), np.abs(p["beta"]))))
    assert (u <= 1).all(), (what, "shift", u.max())


def _check_forward(r, d, f64, what):
    """P's y against the fp64 reference; the consumers' y against the fp64 convolution of what they READ, the op's own
    fp32 affine (+ activation, pool) of P's stored y -- as test_gpu_conv_layer.py feeds its sources"""
    form = d["form"]
    post = LR.FORM_KW[form]["post_act"]
    e = _rel(r["P"]["y"], f64["P"]["y"])
    _note("y P", e, TOL, what)
    assert e <= TOL, (what, "P.y", e)
    oP = R.act_fwd(LR.fp32_affine(r["P"]["y"], r["P"]["scale"], r["P"]["shift"]), CR.ACT[post])
    pooled = None
    if "K" in d["layers"]:
        pooled = R.maxpool_fwd(oP)
        u = CR.ulps32(r["pooled"], pooled)
        assert (u <= 1).all(), (what, "pooled", u.max())
    src = LR.consumer_sources(d, oP, r.get("pooled"))
    for n in ("K", "L"):
        if n in d["layers"]:
            p = d["layers"][n]
            f = CR.layer_forward(src[n], p["w"], p["bias"], p["gamma"], p["beta"], **LR.FORM_KW[form])
            e = _rel(r[n]["y"], f["y"])
            _note("y " + n, e, TOL, what)
            assert e <= TOL, (what, n + ".y", e)
    for n in LR.layer_names(d["link"]):
        _check_stats(r[n], d["layers"][n], "%s %s" % (what, n))


def _check_grads(r, d, ref, ties, what, show=True):
    f64, b64, t64, e32 = ref
    pins = LR.pins_of(r, d["form"])
    own = LR.pins_of_forward(f64, d["form"])
    same = all(np.array_equal(pins[n]["y"] > 0, own[n]["y"] > 0) and np.array_equal(pins[n]["bn"] > 0, own[n]["bn"] > 0)
               for n in LR.layer_names(d["link"]))
    t = "tf_cpu" if ties else "first"
    if "K" in d["layers"]:
        same = same and np.array_equal(LR._routing_mask(pins["P"]["route"], t), LR._routing_mask(own["P"]["route"], t))
    if same:
        tref, pinned, rerouted = t64, {}, 0
    else:
        b = LR.link_backward(d, f64, pins, t)
        tref = dict(LR.grad_tensors(b, LR.layer_names(d["link"])), **{k: v for k, v in t64.items() if k.startswith("linear:")})
        pinned, rerouted = b["pinned"], b["rerouted"]
    if show:
        print("  %s: pinned %s, rerouted pool windows %d" % (what, pinned, rerouted))
    assert max(list(pinned.values()) + [0]) <= CAP and rerouted <= CAP, (what, pinned, rerouted)
    err = LR.rel_errors(LR.op_grad_tensors(r, LR.layer_names(d["link"])), tref, d["form"])
    bad = []
    for k in sorted(err):
        lim = max(TOL, 2 * e32[k])
        if show:
            print("  %s %-9s engine %.3g  e32 %.3g  bound %.3g" % (what, k, err[k], e32[k], lim))
        _note("grad " + k, err[k], lim, what)
        if not err[k] <= lim:
            bad.append((k, err[k], e32[k]))
    assert not bad, (what, bad)


def _full(name, form, ties, env=(), p_regime=None, dout_regime="normal", B=None, max_batch=None):
    what = "%s %s ties=%d %s P:%s dout:%s" % (name, form, ties, "+".join(env) or "default", p_regime, dout_regime)
    d = _data(name, form, p_regime, dout_regime, B)
    ref = _reference(name, form, p_regime, dout_regime, ties, B)
    r = _run(name, form, ties, env, p_regime, dout_regime, B, max_batch)
    _check_sites(r, name, form, env, what)
    _check_forward(r, d, ref[0], what)
    _check_grads(r, d, ref, ties, what)
    return r


def _fusable(name, form):
    return form == "unet" and (_dgrad_kernel(name) is not None)


@pytest.mark.parametrize("p_regime,dout_regime", REGIMES, ids=lambda v: str(v))
@pytest.mark.parametrize("name,form,ties", VARIANTS, ids=lambda v: str(v))
def test_link_matches_reference(name, form, ties, p_regime, dout_regime):
    """default switches: the BwdStat fold (FOLD = 1 / FOLD = true / the dxl launch) where the consumer's kernel takes it,
    the pooled-grid sums for the pool link, the gather kernels for pool + skip"""
    _full(name, form, ties, (), p_regime, dout_regime)


@pytest.mark.parametrize("p_regime,dout_regime", REGIMES, ids=lambda v: str(v))
@pytest.mark.parametrize("name,form,ties", VARIANTS, ids=lambda v: str(v))
def test_link_with_the_linear_folds_on(name, form, ties, p_regime, dout_regime):
    """ICSG3D_DGRAD_BNFUSE_MIN=0: conv_bnfuse_kernel + FOLD = 2 (same), + pool_bnfuse_kernel and FOLD = 3 (pool_skip) where
    the predicates accept the link; every other case asserts that nothing changed"""
    r = _full(name, form, ties, (FUSED,), p_regime, dout_regime)
    if not _fusable(name, form):
        base = _run(name, form, ties, (), p_regime, dout_regime)
        assert r["sites"] == base["sites"], (name, form, "the threshold changed the launches of a link the fold refuses")
        for k, v in LR.op_grad_tensors(base, LR.layer_names(CASES[name]["link"])).items():
            assert np.array_equal(v, LR.op_grad_tensors(r, LR.layer_names(CASES[name]["link"]))[k]), (name, form, k)


@pytest.mark.parametrize("p_regime,dout_regime", [(None, "normal"), ("ratio30", "mean30")], ids=lambda v: str(v))
@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("name,form,ties", VARIANTS, ids=lambda v: str(v))
def test_link_under_switch(name, form, ties, switch, p_regime, dout_regime):
    """each switch on top of the forced folds (so ICSG3D_NO_DGRAD_BNFUSE has something to switch off): the separate pass
    of the same case, the generic BatchNorm-backward kernels, the reduce pass instead of the pooled-grid sums, gs_up instead
    of the up-split.  expected_sites says what each switch changes; elsewhere the rows must be those without it."""
    r = _full(name, form, ties, (FUSED, switch), p_regime, dout_regime)
    have0, lack0 = expected_sites(name, form, (FUSED,))
    if (have0, lack0) == expected_sites(name, form, (FUSED, switch)) and switch != "ICSG3D_NO_FAST_BNBWD":
        base = _run(name, form, ties, (FUSED,), p_regime, dout_regime)
        if switch != "ICSG3D_NO_UPSPLIT" or CASES[name]["link"] in ("same", "pool"):
            assert r["sites"] == base["sites"], (name, form, switch, "the switch changed a link it cannot reach")


@pytest.mark.parametrize("fused", [False, True], ids=["default", "folds"])
@pytest.mark.parametrize("name,form,ties", [v for v in VARIANTS if v[0] in ("same_64_128", "up_64_64", "pool_64", "pool_16",
                                                                              "pool_skip_64")], ids=lambda v: str(v))
def test_handle_larger_than_batch_with_canaries(name, form, ties, fused, monkeypatch):
    """(B, max_batch) = (3, 5): workspaces sized for 5, the step runs 3, the guard bytes behind every buffer stay clean"""
    monkeypatch.setenv("ICSG3D_DEBUG_CANARY", "1")
    _full(name, form, ties, (FUSED,) if fused else (), B=3, max_batch=5)


def test_zz_report_worst_gaps():
    """prints the worst (engine error, yardstick) pairs of this run: the source of the measured table in the header"""
    for k in sorted(WORST):
        print("  %-18s %.3g  (of %.3g)  %s" % (k, WORST[k][0], WORST[k][1], WORST[k][2]))
