"""SyncBN and the metric reductions at 2 to 4 ranks on ONE GPU: ics_op_conv_layer / ics_op_conv_link with ranks = R run
every rank's body through the engines' own construction, conv_forward and conv_backward, with the SyncBN exchanges of
launch_bn_finalize and launch_layer_bwd going through emulated rank tables instead of RCCL (include/icsg3d.h, "emulated
ranks").  What only runs when nranks > 1 is held to the fp64 reference of the CONCATENATED batch
(tests/conv_layer_ref.py, tests/conv_link_ref.py): bn_local_merge_kernel, bn_sync_finalize_kernel (the rank-order Chan merge
and the global n of the moving variance), bn_bwd_finalize_kernel's raw sums + bn_bwd_sync_c_kernel with the global count,
through each of launch_layer_bwd's three routes (its own reduce pass, the BwdStat partials of a consumer's backward-data
epilogue, launch_pool_presum), and phases 1 and 2 of head_finalize_kernel and vae_loss_kernel.

Cases, regimes and inputs: tests/syncbn_cases.py (B is the per-rank batch).  tests/test_syncbn_host.py shows on the CPU that
the sharded fp64 route equals the whole-batch one to 1e-12 and that a float32 emulation of the two merges sits at <= 1.1
ulps of the mean and <= 0.06 of var_bound in every regime here -- the bounds are the project's, none comes from the engine.

Assertions, per case, regime and R:
  statistics   mean, rstd, scale, shift (and the moving statistics of a layer) BITWISE equal on all R ranks; against fp64
               statistics of the R B stored y: mean 4 float32 ulps of max(|mean|, std), var + eps conv_layer_ref.var_bound,
               scale / shift 1 ulp; moving statistics after one update (fp64) with the GLOBAL n in the unbias factor, 2 ulps
  y, dy_p, dx  each rank's slice against the reference's slice: y 1e-5 tensor-relative, gradients max(1e-5, 2 e32) with e32
               the plain float32 numpy formulas on the whole batch against fp64, per case and regime
  gradients    dw, dbias, dgamma, dbeta of every rank are LOCAL sums: each against the reference's contribution of that
               shard under the global statistics (scale: the whole-batch tensor), and their sum over the ranks against the
               whole-batch gradient -- same bound
  decisions    <= 8 pinned activation sides per layer, <= 8 rerouted pool windows, of the engine's own decisions
  sites        even with ICSG3D_DGRAD_BNFUSE_MIN=0 no "bnfuse:" row under emulated ranks; bn_act_bwd:P present; pool_presum:P
               where test_gpu_conv_link.expected_sites says so; the conv_dgrad:L epilogue still the BwdStat one
  self         ranks = R at B against ranks = 1 at R B: same bounds (the merge order differs); ranks = 1 against ranks = 0
               bitwise
  switches     ICSG3D_NO_FAST_BNBWD, _NO_POOL_PRESUM, _NO_BWD_FOLD, _NO_UPSPLIT, and ICSG3D_DEBUG_CANARY=1 with max_batch > B
  metrics      unet_head on R shards -> sums added in fp64 on the host -> ics_op_unet_metrics_from_sums, against unet_head on
               the whole batch: 2 float32 ulps per metric; the same for ics_op_vae_loss phase 1 / host add / phase 2 against
               phase 0 on the whole batch (log-variances from -20 to 10, one perceptual weight zero).

Two things about the YARDSTICKS came out of the first runs on the MI355X (findings 2 and 3):
  e32   numpy_ref.act_bwd multiplies by a float64 array for the LeakyReLU, so conv_layer_ref.layer_backward in "float32"
        continued in float64 behind it and e32 of the VAE form was the forward pass's error alone (dw 3.6e-6 where the U-Net
        form of the same case has 1.2e-3).  Here e32 is taken with strict_dtype=True, a float32 evaluation throughout
        (asserted on the dtypes).  The case that showed it: layer (2, 8, 16 -> 64), VAE form, R = 2, rank_const with dout
        mean 30 -- dw 2.88e-5, from the float32 storage of c1 = sum d / n at |c1| = 19.5 (fp64 with nothing but c1 rounded:
        3.3e-5), the same at one rank.
  moving variance   the reference was numpy_ref.bn_moving_update in float32, whose own four roundings reach 2.5 ulps where
        0.01 var dominates 0.99 (rank_shift50); it is now fp64 from the kernel's float32 constants, the allowance is unchanged.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

import conv_layer_ref as CR
import conv_link_ref as LR
import syncbn_cases as SC
import test_gpu_conv_link as TL
from oracle import numpy_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-5
CAP = 8
FUSED = "ICSG3D_DGRAD_BNFUSE_MIN"
STAT_KEYS = ("mean", "rstd", "scale", "shift")
WORST = {}


def _note(key, err, yard, what):
    if key not in WORST or err / max(yard, 1e-300) > WORST[key][0] / max(WORST[key][1], 1e-300):
        WORST[key] = (err, yard, what)


def _rel(a, b, scale=None):
    s = np.abs(b).max() if scale is None else scale
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(s, 1e-300))


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


def _check_stats(o, y, gamma, beta, R_, what, moving=None):
    """o: mean / rstd / scale / shift, each (R, C); y: the R B stored activations of the layer"""
    for k in STAT_KEYS + (("moving_mean", "moving_var") if moving else ()):
        for r in range(1, R_):
            assert np.array_equal(o[k][r].view(np.uint32), o[k][0].view(np.uint32)), (what, k, "rank", r, "differs from rank 0")
    mean, rstd, scale, shift = (o[k][0] for k in STAT_KEYS)
    m64, v64 = CR.channel_stats(y)
    mu = CR.ulps32(mean, m64, at=np.maximum(np.abs(m64), np.sqrt(v64)))
    vpe = 1.0 / rstd.astype(np.float64) ** 2
    ve = CR.var_error(vpe, v64)
    bound = CR.var_bound(m64, v64)
    _note("mean ulps", float(mu.max()), CR.MEAN_ULPS, what)
    _note("var+eps / bound", float((ve / bound).max()), 1.0, what)
    print("  %s: mean %.2f ulps (of %d), var + eps %.3g of its bound" % (what, mu.max(), CR.MEAN_ULPS, (ve / bound).max()))
    assert (mu <= CR.MEAN_ULPS).all(), (what, "mean", mu.max(), int(mu.argmax()))
    assert (ve <= bound).all(), (what, "var + eps", ve.max(), int((ve / bound).argmax()))
    u = CR.ulps32(scale, gamma * rstd)
    assert (u <= 1).all(), (what, "scale", u.max())
    prod = mean.astype(np.float64) * scale.astype(np.float64)
    sh = beta.astype(np.float64) - prod
    u = CR.ulps32(shift, sh, at=np.maximum(np.abs(sh), np.maximum(np.abs(prod), np.abs(beta))))
    assert (u <= 1).all(), (what, "shift", u.max())
    if moving:
        # One update from (0, 1) with n the rows of the GLOBAL batch, in fp64 from the float32 constants the kernel holds
        # (momentum 0.99f, 1.f - 0.99f), the returned float32 mean and var = 1 / rstd^2 - eps.  The kernels round (float)v,
        # the product and the sum once each: 1.5 ulps of the result at most, 2 allowed as in test_gpu_conv_layer.py, plus
        # what half an ulp of rstd (2^-23 of var + eps) moves the result by.  The reference is NOT numpy_ref.bn_moving_update
        # in float32: that chain rounds var32, the unbias product, the product with 1 - momentum and the sum itself, which
        # is negligible where 0.01 var << 0.99 (every regime of test_gpu_conv_layer.py but "huge") and up to 2.5 ulps of
        # its own where 0.01 var dominates (rank_shift50: var ~ 625) -- a reference error the allowance never contained.
        C = y.shape[-1]
        n = y.size // C
        m = float(np.float32(0.99))
        om = float(np.float32(1.0) - np.float32(0.99))

        def update(count):
            v = (vpe - CR.EPS) * (count / (count - (1.0 + CR.EPS)))
            return mean.astype(np.float64) * om, m + v * om

        mm, mv = update(n)
        um, uv = CR.ulps32(o["moving_mean"][0], mm), CR.ulps32(o["moving_var"][0], mv)
        dvar = om * n / (n - (1.0 + CR.EPS)) * vpe * 2.0 ** -23
        lim_v = 2 + dvar / np.spacing(np.abs(mv).astype(np.float32)).astype(np.float64)
        _note("moving_var ulps", float((uv / lim_v).max() * 2), 2, what)
        print("  %s: moving mean %.2f ulps (of 2), moving variance %.2f of its bound (2 ulps + rstd's)" % (what, um.max(), (uv / lim_v).max()))
        assert (um <= 2).all() and (uv <= lim_v).all(), (what, "moving", um.max(), uv.max(), int((uv / lim_v).argmax()))
        # ... and that the bound tells the global from the local count where one ulp allows it
        _, mv_local = update(n // R_)
        far = CR.ulps32(mv_local, mv) > 2 * lim_v + 2
        if far.any():
            assert (CR.ulps32(o["moving_var"][0], mv_local)[far] > lim_v[far]).all(), (what, "moving variance with the local n")

def _check_shards(got, shards, whole, e32, R_, what, dbias_scale=None):
    """got[k]: (R, ...) local sums; shards: R dicts of the reference's contributions; whole[k]: the whole-batch gradient"""
    bad = []
    for k in ("dw", "dbias", "dgamma", "dbeta"):
        if k not in whole:
            continue
        lim = max(TOL, 2 * e32[k])
        scale = np.abs(whole[k]).max()
        if k == "dbias" and dbias_scale is not None:
            scale = max(scale, dbias_scale)
        for r in range(R_):
            # a shard's contribution on the scale of the largest contribution (a rank whose dout is zero contributes ~0)
            s_r = max(scale, max(np.abs(g[k]).max() for g in shards))
            e = _rel(got[k][r], shards[r][k], s_r)
            _note("shard " + k, e, lim, what)
            if not e <= lim:
                bad.append((k, "rank %d" % r, e, lim))
        tot = np.add.reduce(np.asarray(got[k], np.float64), 0)
        e = _rel(tot, whole[k], max(scale, max(np.abs(g[k]).max() for g in shards)))
        print("  %s %-7s sum over ranks %.3g  e32 %.3g  bound %.3g" % (what, k, e, e32[k], lim))
        _note("total " + k, e, lim, what)
        if not e <= lim:
            bad.append((k, "sum", e, lim))
    assert not bad, (what, bad)


# ================================================================ one layer
@functools.lru_cache(maxsize=None)
def _layer_reference(name, form, R_, regime, dr, B=None):
    d = SC.layer_data(name, form, R_, regime, dr, B)
    args = (d["sources"], d["w"], d["bias"], d["gamma"], d["beta"])
    f64 = CR.layer_forward(*args, **d["kw"])
    b64 = CR.layer_backward(f64, d["sources"], d["w"], d["gamma"], d["dout"], **d["kw"])
    f32 = CR.layer_forward(*args, dtype=np.float32, **d["kw"])
    b32 = CR.layer_backward(f32, d["sources"], d["w"], d["gamma"], d["dout"], kink_y=f64["y"], kink_bn=f64.get("bn"),
                            strict_dtype=True, **d["kw"])
    assert b32["dw"].dtype == np.float32 and b32["dgamma"].dtype == np.float32, "e32 is not a float32 evaluation"
    linear = bool(d["kw"]["pre_act"]) and bool((f64["y"] > 0).all())
    dbs = np.abs(b64["dw"]).max() if (not d["kw"]["pre_act"] or linear) else None
    e32 = {k: _rel(b32[k], b64[k], max(np.abs(b64[k]).max(), dbs or 0.0) if k == "dbias" else None)
           for k in ("dw", "dbias", "dgamma", "dbeta")}
    for i in range(len(b64["dx"])):
        e32["dx%d" % i] = _rel(b32["dx"][i], b64["dx"][i])
    return f64, b64, e32, dbs


def _run_layer(name, form, R_, regime, dr, env=(), ranks=None, B=None, max_batch=None):
    from icsg3d_amd import engine as E
    c = SC.LAYER_CASES[name]
    d = SC.layer_data(name, form, R_, regime, dr, B)
    with _env(_envdict(env)):
        return E.conv_layer(d["sources"], d["w"], d["bias"], d["gamma"], d["beta"], dout=d["dout"], pad_input=c["pad"],
                            max_batch=max_batch, ranks=R_ if ranks is None else ranks, **d["kw"])


def _lead(r, R_):
    """a ranks = 0 result in the shape of a ranks = R one"""
    out = dict(r)
    for k in STAT_KEYS + ("moving_mean", "moving_var", "dw", "dbias", "dgamma", "dbeta"):
        out[k] = r[k][None]
    return out


def _check_layer(r, name, form, R_, regime, dr, what, B=None):
    d = SC.layer_data(name, form, R_, regime, dr, B)
    f64, b64, e32, dbs = _layer_reference(name, form, R_, regime, dr, B)
    kw = d["kw"]
    e = _rel(r["y"], f64["y"])
    _note("y", e, TOL, what)
    assert e <= TOL, (what, "y", e)
    _check_stats(r, r["y"], d["gamma"], d["beta"], R_, what, moving=True)
    kink_bn = LR.fp32_affine(r["y"], r["scale"][0], r["shift"][0])
    own_y = np.array_equal(r["y"] > 0, f64["y"] > 0) if kw["pre_act"] else True
    own_bn = np.array_equal(kink_bn > 0, f64["bn"] > 0) if kw["post_act"] else True
    b, pinned = b64, 0
    if not (own_y and own_bn):
        b = CR.layer_backward(f64, d["sources"], d["w"], d["gamma"], d["dout"], kink_y=r["y"], kink_bn=kink_bn, **kw)
        pinned = b["pinned"]
    print("  %s: pinned %d" % (what, pinned))
    assert pinned <= CAP, (what, "pinned", pinned)
    for i, dx in enumerate(r["dx"]):
        lim = max(TOL, 2 * e32["dx%d" % i])
        for rk in range(R_):
            e = _rel(SC.rank_slice(dx, rk, R_), SC.rank_slice(b["dx"][i], rk, R_), np.abs(b["dx"][i]).max())
            _note("dx%d" % i, e, lim, what)
            assert e <= lim, (what, "dx%d" % i, "rank", rk, e, lim)
    _check_shards(r, CR.shard_grads(f64, b, d["w"], R_), b, e32, R_, what, dbs)


def _full_layer(name, form, ranks, regime, dr, env=(), max_batch=None):
    what = "%s %s R=%d %s y:%s dout:%s" % (name, form, ranks, "+".join(env) or "default", regime, dr)
    r = _run_layer(name, form, ranks, regime, dr, env, max_batch=max_batch)
    _check_layer(r, name, form, ranks, regime, dr, what)
    for k in r["kernels"][1:]:
        assert k == r["kernels"][0], (what, "the ranks launched different kernels")


@pytest.mark.parametrize("regime,dout_regime", SC.LAYER_REGIMES, ids=str)
@pytest.mark.parametrize("name,form,ranks", SC.LAYER_VARIANTS, ids=str)
def test_layer_at_emulated_ranks(name, form, ranks, regime, dout_regime):
    if (regime, dout_regime) in SC.layer_regimes(name):      # (a one-channel input has no carrier: those regimes run nothing)
        _full_layer(name, form, ranks, regime, dout_regime)


@pytest.mark.parametrize("switch", ["ICSG3D_NO_FAST_BNBWD", "ICSG3D_NO_UPSPLIT"])
@pytest.mark.parametrize("name,form,ranks", [v for v in SC.LAYER_VARIANTS if v[2] == 2], ids=str)
def test_layer_under_switch(name, form, ranks, switch):
    for regime, dr in [(None, "normal"), ("rank_std100" if name in SC.NO_CARRIER else "rank_shift50", "normal")]:
        _full_layer(name, form, ranks, regime, dr, env=(switch,))


@pytest.mark.parametrize("name,form,ranks", [v for v in SC.LAYER_VARIANTS if v[2] == max(SC.LAYER_CASES[v[0]]["ranks"])], ids=str)
def test_layer_ranks_against_one_rank_at_the_whole_batch(name, form, ranks):
    """ranks = R at B against ranks = 1 at R B (one emulated rank: the same kernels, another merge order) within the bounds
    both are held to; ranks = 1 against ranks = 0 (no SyncBN) bitwise"""
    for regime, dr in [(None, "normal"), ("rank_shift50", "normal") if name not in SC.NO_CARRIER else ("rank_std100", "normal")]:
        what = "%s %s R=%d vs 1 y:%s" % (name, form, ranks, regime)
        d = SC.layer_data(name, form, ranks, regime, dr)
        _, b64, e32, dbs = _layer_reference(name, form, ranks, regime, dr)
        rR = _run_layer(name, form, ranks, regime, dr)
        r1 = _run_layer(name, form, ranks, regime, dr, ranks=1)
        r0 = _run_layer(name, form, ranks, regime, dr, ranks=0)
        assert np.array_equal(rR["y"], r1["y"]), what
        m64, v64 = CR.channel_stats(r1["y"])
        mu = CR.ulps32(rR["mean"][0], r1["mean"][0].astype(np.float64), at=np.maximum(np.abs(m64), np.sqrt(v64)))
        assert (mu <= CR.MEAN_ULPS).all(), (what, "mean", mu.max())
        ve = CR.var_error(1.0 / rR["rstd"][0].astype(np.float64) ** 2, 1.0 / r1["rstd"][0].astype(np.float64) ** 2 - CR.EPS)
        assert (ve <= CR.var_bound(m64, v64)).all(), (what, "var + eps", ve.max())
        for k in ("dw", "dbias", "dgamma", "dbeta"):
            lim = max(TOL, 2 * e32[k])
            scale = max(np.abs(b64[k]).max(), dbs or 0.0) if k == "dbias" else np.abs(b64[k]).max()
            e = _rel(np.add.reduce(rR[k].astype(np.float64), 0), r1[k][0], scale)
            assert e <= lim, (what, k, e, lim)
        for i in range(len(rR["dx"])):
            e = _rel(rR["dx"][i], r1["dx"][i], np.abs(b64["dx"][i]).max())
            assert e <= max(TOL, 2 * e32["dx%d" % i]), (what, "dx", e)
        for k in ("y",) + STAT_KEYS + ("moving_mean", "moving_var", "dw", "dbias", "dgamma", "dbeta"):
            a, b = (r1[k][0] if k != "y" else r1[k]), r0[k]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, k, "ranks = 1 differs from ranks = 0", _rel(a, b))
        for a, b in zip(r1["dx"], r0["dx"]):
            assert np.array_equal(a, b), (what, "dx: ranks = 1 differs from ranks = 0")


# ================================================================ links
@functools.lru_cache(maxsize=None)
def _link_reference(name, form, ties, R_, regime, dr, B=None):
    d = SC.link_data(name, form, R_, regime, dr, B)
    t = "tf_cpu" if ties else "first"
    f, b, t64 = LR.reference(d, ties=t)
    return f, b, t64, LR.e32_of(d, f, t64, ties=t, strict_dtype=True)


def _run_link(name, form, ties, R_, regime, dr, env=(), ranks=None, B=None, max_batch=None):
    from icsg3d_amd import engine as E
    d = SC.link_data(name, form, R_, regime, dr, B)
    with _env(_envdict(env)):
        return E.conv_link(d["link"], d["x0"], d["layers"], d["dout"], form=form, q=d.get("q"), dout_l=d.get("dout_l"),
                           pool_ties_all=bool(ties), max_batch=max_batch, ranks=R_ if ranks is None else ranks)


def _flat(r, names):
    """a ranks = R result with rank 0's statistics in the per-layer slots: what conv_link_ref.pins_of reads"""
    out = {k: v for k, v in r.items() if k not in names}
    for n in names:
        out[n] = dict(r[n], **{k: r[n][k][0] for k in STAT_KEYS})
    return out


def _check_sites(r, name, form, env, R_, what):
    """test_gpu_conv_link.expected_sites with the linear folds refused (SyncBN), on every rank"""
    have, lack = TL.expected_sites(name, form, tuple(e for e in env if e != FUSED))
    lack = lack + ["bnfuse:"]
    have = have + ["bn_act_bwd:P"]
    for rk in range(R_):
        TL_r = {"sites": r["sites"][rk]}
        text = "\n".join(TL_r["sites"])
        for frag in have:
            if frag == "true>":
                assert any(ln.startswith("conv_dgrad:L") and ln.endswith(frag) for ln in TL_r["sites"]), (what, rk, "no FOLD launch")
                continue
            assert frag in text, (what, "rank", rk, "missing", frag, TL_r["sites"])
        for frag in lack:
            rows = [ln for ln in TL_r["sites"] if frag in ln and (frag != "true>" or ln.startswith("conv_dgrad:L"))]
            assert not rows, (what, "rank", rk, "unexpected", frag, rows)
        assert TL_r["sites"] == r["sites"][0], (what, "the ranks launched different sites")


def _check_link(r, name, form, ties, R_, regime, dr, env, what, B=None):
    d = SC.link_data(name, form, R_, regime, dr, B)
    f64, b64, t64, e32 = _link_reference(name, form, ties, R_, regime, dr, B)
    names = LR.layer_names(d["link"])
    _check_sites(r, name, form, env, R_, what)
    # forward: P against the reference, the consumers against the fp64 convolution of what they read (as test_gpu_conv_link)
    flat = _flat(r, names)
    post = LR.FORM_KW[form]["post_act"]
    e = _rel(r["P"]["y"], f64["P"]["y"])
    _note("y P", e, TOL, what)
    assert e <= TOL, (what, "P.y", e)
    oP = R.act_fwd(LR.fp32_affine(r["P"]["y"], flat["P"]["scale"], flat["P"]["shift"]), CR.ACT[post])
    if "K" in d["layers"]:
        u = CR.ulps32(r["pooled"], R.maxpool_fwd(oP))
        assert (u <= 1).all(), (what, "pooled", u.max())
    src = LR.consumer_sources(d, oP, r.get("pooled"))
    for n in ("K", "L"):
        if n in d["layers"]:
            p = d["layers"][n]
            f = CR.layer_forward(src[n], p["w"], p["bias"], p["gamma"], p["beta"], **LR.FORM_KW[form])
            e = _rel(r[n]["y"], f["y"])
            _note("y " + n, e, TOL, what)
            assert e <= TOL, (what, n + ".y", e)
    for n in names:
        _check_stats(r[n], r[n]["y"], d["layers"][n]["gamma"], d["layers"][n]["beta"], R_, "%s %s" % (what, n))
    # backward, with the engine's decisions where they differ from the reference's own
    t = "tf_cpu" if ties else "first"
    pins = LR.pins_of(flat, form)
    own = LR.pins_of_forward(f64, form)
    same = all(np.array_equal(pins[n]["y"] > 0, own[n]["y"] > 0) and np.array_equal(pins[n]["bn"] > 0, own[n]["bn"] > 0) for n in names)
    if "K" in d["layers"]:
        same = same and np.array_equal(LR._routing_mask(pins["P"]["route"], t), LR._routing_mask(own["P"]["route"], t))
    b, pinned, rerouted = b64, {}, 0
    if not same:
        b = LR.link_backward(d, f64, pins, t)
        pinned, rerouted = b["pinned"], b["rerouted"]
    print("  %s: pinned %s, rerouted pool windows %d" % (what, pinned, rerouted))
    assert max(list(pinned.values()) + [0]) <= CAP and rerouted <= CAP, (what, pinned, rerouted)
    for k in ("dy_p", "dx0"):
        lim = max(TOL, 2 * e32[k])
        for rk in range(R_):
            e = _rel(SC.rank_slice(r[k], rk, R_), SC.rank_slice(b[k], rk, R_), np.abs(b[k]).max())
            _note("grad " + k, e, lim, what)
            assert e <= lim, (what, k, "rank", rk, e, lim)
        print("  %s %-7s e32 %.3g  bound %.3g" % (what, k, e32[k], lim))
    sh = LR.shard_grads(d, f64, b, R_)
    for n in names:
        lin = form == "vae" or t64.get("linear:" + n, False)
        _check_shards(r[n], sh[n], b[n], {k: e32["%s.%s" % (n, k)] for k in LR.GRAD_KEYS}, R_, "%s %s" % (what, n),
                      np.abs(b[n]["dw"]).max() if lin else None)


def _full_link(name, form, ties, R_, regime, dr, env=(FUSED,), B=None, max_batch=None):
    what = "%s %s ties=%d R=%d %s P:%s dout:%s" % (name, form, ties, R_, "+".join(env), regime, dr)
    r = _run_link(name, form, ties, R_, regime, dr, env, B=B, max_batch=max_batch)
    _check_link(r, name, form, ties, R_, regime, dr, env, what, B)
    return r


@pytest.mark.parametrize("regime,dout_regime", SC.LINK_REGIMES, ids=str)
@pytest.mark.parametrize("name,form,ties,ranks", SC.LINK_VARIANTS, ids=str)
def test_link_at_emulated_ranks(name, form, ties, ranks, regime, dout_regime):
    """with ICSG3D_DGRAD_BNFUSE_MIN=0: the linear folds would be taken at one rank and must be refused here"""
    _full_link(name, form, ties, ranks, regime, dout_regime)


@pytest.mark.parametrize("name,form,ties,ranks", [v for v in SC.LINK_VARIANTS if v[3] == 2 and v[2] == 1], ids=str)
def test_link_ranks_against_one_rank_at_the_whole_batch(name, form, ties, ranks):
    for regime, dr in [(None, "normal"), ("rank_shift50", "normal")]:
        what = "%s %s R=%d vs 1 P:%s" % (name, form, ranks, regime)
        d = SC.link_data(name, form, ranks, regime, dr)
        _, b64, t64, e32 = _link_reference(name, form, ties, ranks, regime, dr)
        names = LR.layer_names(d["link"])
        rR = _run_link(name, form, ties, ranks, regime, dr)
        r1 = _run_link(name, form, ties, ranks, regime, dr, ranks=1)
        r0 = _run_link(name, form, ties, ranks, regime, dr, ranks=0)
        for k in ("dy_p", "dx0"):
            e = _rel(rR[k], r1[k], np.abs(b64[k]).max())
            assert e <= max(TOL, 2 * e32[k]), (what, k, e)
        for n in names:
            for k in LR.GRAD_KEYS:
                scale = max(np.abs(b64[n][k]).max(), np.abs(b64[n]["dw"]).max() if k == "dbias" else 0.0)
                e = _rel(np.add.reduce(rR[n][k].astype(np.float64), 0), r1[n][k][0], scale)
                assert e <= max(TOL, 2 * e32["%s.%s" % (n, k)]), (what, n, k, e)
        # (the launch sites of R ranks at B and of one at R B may differ: dispatch depends on the batch, e.g. conv_winog's
        # backward-weight needs B % 4 == 0)
        assert not [ln for ln in r1["sites"][0] if "bnfuse:" in ln], (what, "a linear fold under one emulated rank")
        for k in ("dy_p", "dx0"):
            assert np.array_equal(r1[k], r0[k]), (what, k, "ranks = 1 differs from ranks = 0")
        for n in names:
            for k in ("y",) + STAT_KEYS + LR.GRAD_KEYS:
                a = r1[n][k] if k == "y" else r1[n][k][0]
                assert np.array_equal(a.view(np.uint32), r0[n][k].view(np.uint32)), (what, n, k, "ranks = 1 differs from ranks = 0", _rel(a, r0[n][k]))


SWITCHES = ("ICSG3D_NO_FAST_BNBWD", "ICSG3D_NO_POOL_PRESUM", "ICSG3D_NO_BWD_FOLD", "ICSG3D_NO_UPSPLIT")


@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("name,form,ties,ranks", [v for v in SC.LINK_VARIANTS if v[3] == 2 and v[2] == 1], ids=str)
def test_link_under_switch(name, form, ties, ranks, switch):
    for regime, dr in [(None, "normal"), ("rank_shift50", "normal")]:
        _full_link(name, form, ties, ranks, regime, dr, env=(FUSED, switch))


@pytest.mark.parametrize("name,form,ties,ranks", [v for v in SC.LINK_VARIANTS if v[3] == 2 and v[2] == 1 and v[0] in
                                                  ("same_64_128", "up_32_16", "pool_64", "pool_skip_64")], ids=str)
def test_link_handle_larger_than_batch_with_canaries(name, form, ties, ranks, monkeypatch):
    """max_batch = B + 2: workspaces sized for it, every rank runs B, the guard bytes behind every buffer stay clean"""
    monkeypatch.setenv("ICSG3D_DEBUG_CANARY", "1")
    B = SC.LINK_CASES[name]["kw"]["B"]
    for regime, dr in [(None, "normal"), ("rank_shift50", "normal")]:
        _full_link(name, form, ties, ranks, regime, dr, max_batch=B + 2)


@pytest.mark.parametrize("name,form,ranks", [v for v in SC.LAYER_VARIANTS if v[2] == 2], ids=str)
def test_layer_handle_larger_than_batch_with_canaries(name, form, ranks, monkeypatch):
    monkeypatch.setenv("ICSG3D_DEBUG_CANARY", "1")
    regime = "rank_std100" if name in SC.NO_CARRIER else "rank_shift50"
    for rg, dr in [(None, "normal"), (regime, "normal")]:
        _full_layer(name, form, ranks, rg, dr, max_batch=SC.LAYER_CASES[name]["B"] + 2)


def test_refusals():
    from icsg3d_amd import engine as E
    d = SC.layer_data("generic_6", "unet", 2, None, "normal")
    for bad in (5, -1):
        with pytest.raises(Exception):
            E.conv_layer(d["sources"], d["w"], d["bias"], d["gamma"], d["beta"], dout=d["dout"], ranks=bad, **d["kw"])
    with pytest.raises(Exception, match="max_batch"):
        E.conv_layer(d["sources"], d["w"], d["bias"], d["gamma"], d["beta"], dout=d["dout"], ranks=2, max_batch=1, **d["kw"])


# ================================================================ metric sums
def _ulps(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("ncls,fused", [(95, True), (95, False), (17, False)])     # the fused head kernel serves ncls = 95 only
@pytest.mark.parametrize("ranks", [2, 3])
def test_unet_metrics_from_shard_sums(ranks, ncls, fused):
    from icsg3d_amd import engine as E
    rng = np.random.default_rng(ncls + ranks)
    M = 512
    x = rng.standard_normal((ranks * M, 128)).astype(np.float32)
    wsoft = (rng.standard_normal((128, ncls)) * 0.5).astype(np.float32)     # confident enough for tp / wr to be non-zero
    bsoft, wsig, bsig = np.zeros(ncls, np.float32), (rng.standard_normal(128) * 0.3).astype(np.float32), np.zeros(1, np.float32)
    lab = (x @ wsoft).argmax(1).astype(np.uint8)
    lab[rng.uniform(size=lab.size) < 0.3] = 0
    lab[(ranks - 1) * M:] = 0                                               # the last shard has no atom voxels at all
    _, m_whole, s_whole = E.unet_head(x, wsoft, bsoft, wsig, bsig, lab, mode=1, fused=fused)
    tot = np.zeros(7)
    for r in range(ranks):
        sl = slice(r * M, (r + 1) * M)
        _, _, s = E.unet_head(x[sl], wsoft, bsoft, wsig, bsig, lab[sl], mode=1, fused=fused)
        tot += np.array([s[k] for k in E.METRIC_SUM_KEYS])
    assert tot[6] == ranks * M and s_whole["voxels"] == ranks * M
    m = E.unet_metrics_from_sums(tot)
    u = _ulps(m, m_whole)
    print("  unet metrics R=%d ncls=%d fused=%s: from sums %s  whole %s  ulps %s" % (ranks, ncls, fused, m, m_whole, u))
    _note("unet metric ulps", float(u.max()), 2, "R=%d ncls=%d" % (ranks, ncls))
    assert m_whole[3] > 0 and m_whole[4] > 0
    assert (u <= 2).all(), (m, m_whole, u)


@pytest.mark.parametrize("latent,B", [(20, 2), (256, 3)])
@pytest.mark.parametrize("ranks", [2, 3])
def test_vae_loss_from_shard_sums(ranks, latent, B):
    from icsg3d_amd import engine as E
    import test_syncbn_host as H
    mulv, sq, pm, per, w = H.vae_inputs(B * ranks, latent, seed=latent + ranks, zero_weight=True)
    kw = dict(pm_per=per, pm_w=w, alpha=0.5, beta=3e-4)
    whole = E.vae_loss(mulv, sq.sum(1), n_elems=sq.size, pm_partials=[p.sum(1) for p in pm], phase=0, **kw)
    tot = np.zeros(5)
    for r in range(ranks):
        sl = slice(r * B, (r + 1) * B)
        tot += E.vae_loss(mulv[sl], sq[sl].sum(1), n_elems=sq[sl].size, pm_partials=[p[sl].sum(1) for p in pm], phase=1, **kw)
    assert tot[3] == B * ranks and tot[4] == sq.size
    m = E.vae_loss(phase=2, sums=tot, alpha=0.5, beta=3e-4)
    ref = H.vae_metrics_from_sums(H.vae_sums(mulv, sq, pm, per, w), 0.5, 3e-4)
    u = _ulps(m, whole)
    print("  vae loss R=%d latent=%d: from sums %s  phase 0 %s  fp64 %s  ulps %s" % (ranks, latent, m, whole, ref, u))
    _note("vae metric ulps", float(u.max()), 2, "R=%d latent=%d" % (ranks, latent))
    assert (u <= 2).all(), (m, whole, u)
    assert (_ulps(whole, ref.astype(np.float32)) <= 2).all(), (whole, ref)


def test_zz_report_worst_gaps():
    """prints the worst (engine error, yardstick) pairs of this run: the source of the table in DESIGN.md section 23"""
    for k in sorted(WORST):
        print("  %-18s %.3g  (of %.3g)  %s" % (k, WORST[k][0], WORST[k][1], WORST[k][2]))
