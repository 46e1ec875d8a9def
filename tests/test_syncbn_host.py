"""SyncBN at 2 to 4 ranks on the CPU: the references and bounds tests/test_gpu_syncbn.py holds the kernels to.

(1) The SHARDED fp64 route of conv_layer_ref / conv_link_ref (per-shard (n, mean, M2), rank-order Chan merge, per-shard
    (sum d, sum d xhat) added over the ranks, dy from the global sums) equals the whole-batch route to 1e-12, forward and
    backward, for R = 2, 3, 4, both network forms and the four links; every rank's local gradients (shard_grads) add up to
    the whole-batch gradients; the moving variance takes the GLOBAL n in its unbias factor.
(2) A float32 emulation of the kernels' two merges (conv_layer_ref.stats_sharded32: float32 block partials, fp64 local
    merge, fp64 rank merge, rstd through float(1 / sqrt(var + eps))) stays inside the statistic bounds of the project --
    MEAN_ULPS, var_bound -- in every regime the GPU test runs, the rank-heterogeneous ones included; the same emulation
    with either cross term left out does not.  This calibrates the bounds against the reference, not against the engine.
(3) The from-sums finalisers in fp64: the U-Net's five metrics and the VAE's four from shard sums added on the host equal
    the whole-batch metrics to 1e-12.
(4) The decision caps of the GPU cases' seeds: a float32 numpy evaluation differs from the fp64 reference at no more than
    8 activation sides per layer and 8 pool windows (printed where a regime exceeds it; test_gpu_syncbn.py asserts the caps
    on the engine's own decisions)."""
import numpy as np
import pytest

import conv_layer_ref as CR
import conv_link_ref as LR
import syncbn_cases as SC
from oracle import numpy_ref as R

TOL = 1e-12


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


# ---------------------------------------------------------------- (1) sharded route = whole-batch route
SMALL_LAYER = dict(B=1, S=4, src=[(6, 0)], Cout=5)


@pytest.mark.parametrize("regime", [None, 0, "rank_shift50", "rank_const", "rank_zero", "rank_std100"], ids=str)
@pytest.mark.parametrize("form", ["unet", "vae"])
@pytest.mark.parametrize("ranks", [2, 3, 4])
def test_sharded_layer_equals_whole_batch(ranks, form, regime):
    c = SMALL_LAYER
    off = regime if regime in (None, 0) else None
    d = CR.make_case(c["B"] * ranks * 2, c["S"], c["src"], c["Cout"], 27, form, True, seed=ranks, regime_off=off)
    if regime in CR.RANK_REGIMES:
        CR.rank_regimes(d, ranks, regime)
    d["dout"] = CR.rank_dout(d["dout"], ranks, "one_rank" if regime == "rank_zero" else "normal")
    args = (d["sources"], d["w"], d["bias"], d["gamma"], d["beta"])
    f0 = CR.layer_forward(*args, **d["kw"])
    f1 = CR.layer_forward(*args, ranks=ranks, **d["kw"])
    # tiny_std / constant channels: the variance itself is at rounding level of the mean; compare what the layer uses
    for k in ("mean", "rstd", "scale", "shift", "o"):
        assert _rel(f1[k], f0[k]) <= TOL, (k, _rel(f1[k], f0[k]))
    assert np.abs(f1["var"] - f0["var"]).max() <= TOL * (f0["var"] + f0["mean"] ** 2 + CR.EPS).max()
    b0 = CR.layer_backward(f0, d["sources"], d["w"], d["gamma"], d["dout"], **d["kw"])
    b1 = CR.layer_backward(f1, d["sources"], d["w"], d["gamma"], d["dout"], ranks=ranks, **d["kw"])
    for k in ("dw", "dbias", "dgamma", "dbeta", "dy"):
        scale = max(np.abs(b0[k]).max(), np.abs(b0["dw"]).max() if k == "dbias" else 0.0)
        assert np.abs(b1[k] - b0[k]).max() <= 1e-11 * scale, (k, np.abs(b1[k] - b0[k]).max() / scale)
    assert _rel(b1["dx"][0], b0["dx"][0]) <= 1e-11
    sh = CR.shard_grads(f0, b0, d["w"], ranks)
    for k in ("dw", "dbias", "dgamma", "dbeta"):
        scale = max(np.abs(b0[k]).max(), np.abs(b0["dw"]).max() if k == "dbias" else 0.0)
        tot = sum(g[k] for g in sh)
        assert np.abs(tot - b0[k]).max() <= 1e-11 * max(scale, max(np.abs(g[k]).max() for g in sh)), k


@pytest.mark.parametrize("link,form", [("same", "unet"), ("same", "vae"), ("up", "unet"), ("up", "vae"), ("pool", "unet"),
                                       ("pool", "vae"), ("pool_skip", "unet")])
@pytest.mark.parametrize("ranks", [2, 3, 4])
def test_sharded_link_equals_whole_batch(ranks, link, form):
    d = LR.make_link(link, form, B=ranks, S=4, C0=4, Cp=6, Ck=5, Cl=7, Cq=3, seed=ranks)
    CR.rank_regimes(LR.link_case_view(d), ranks, "rank_shift50")
    f0, f1 = LR.link_forward(d), LR.link_forward(d, ranks=ranks)
    names = LR.layer_names(link)
    for n in names:
        for k in ("mean", "var", "o"):
            assert _rel(f1[n][k], f0[n][k]) <= TOL, (n, k)
    # both routes with the same decisions (the whole-batch route's): a decision is not what is compared
    pins = LR.pins_of_forward(f0, form)
    b0, b1 = LR.link_backward(d, f0, pins), LR.link_backward(d, f1, pins, ranks=ranks)
    t0, t1 = LR.grad_tensors(b0, names), LR.grad_tensors(b1, names)
    err = LR.rel_errors(t1, dict(t0, **{"linear:" + n: False for n in names}), "vae")
    assert max(err.values()) <= 1e-11, err
    sh = LR.shard_grads(d, f0, b0, ranks)
    for n in names:
        for k in LR.GRAD_KEYS:
            tot = sum(g[k] for g in sh[n])
            scale = max(np.abs(b0[n][k]).max(), np.abs(b0[n]["dw"]).max(), max(np.abs(g[k]).max() for g in sh[n]))
            assert np.abs(tot - b0[n][k]).max() <= 1e-11 * scale, (n, k)


def test_moving_variance_takes_the_global_count():
    rng = np.random.default_rng(0)
    y = rng.standard_normal((6, 2, 2, 2, 3)) + 5.0
    n, mean, var = CR.merge_moments(*CR.shard_moments(y, 3))
    assert (n == 48).all()
    mm, mv = CR.moving_after_one_update(mean, var, n)
    mm0, mv0 = R.bn_moving_update(np.zeros(3), np.ones(3), mean, var, 48, momentum=0.99)
    assert _rel(mm, mm0) <= TOL and _rel(mv, mv0) <= TOL
    _, mv_local = CR.moving_after_one_update(mean, var, 16.0)       # the local count: visibly different at these sizes
    assert (np.abs(mv_local - mv) / mv > 1e-4).all()


# ---------------------------------------------------------------- (2) float32 emulation of the two merges
def _emulate(y, ranks, rows_per_block, what, show):
    m64, v64 = CR.channel_stats(y)
    mean, vpe, _ = CR.stats_sharded32(y, ranks, rows_per_block)
    mu = CR.ulps32(mean, m64, at=np.maximum(np.abs(m64), np.sqrt(v64)))
    ve = CR.var_error(vpe, v64)
    bound = CR.var_bound(m64, v64)
    if show:
        print("  %-44s mean %.2f ulps (of %d)   var + eps %.3g of its bound" % (what, mu.max(), CR.MEAN_ULPS, (ve / bound).max()))
    return mu, ve / bound


@pytest.mark.parametrize("name,form,ranks", SC.LAYER_VARIANTS, ids=str)
def test_merge_emulation_inside_the_statistic_bounds(name, form, ranks):
    """every layer case and regime of the GPU test, on the fp64 reference's y rounded to float32 (what the engine stores to
    within 1e-5); blocks of 64 and 512 rows span the kernels' statistics blocks"""
    for regime, dr in SC.layer_regimes(name):
        d = SC.layer_data(name, form, ranks, regime, dr)
        f = CR.layer_forward(d["sources"], d["w"], d["bias"], d["gamma"], d["beta"], **d["kw"])
        y = f["y"].astype(np.float32)
        for rpb in (64, 512):
            mu, vr = _emulate(y, ranks, rpb, "%s %s R=%d %s rpb %d" % (name, form, ranks, regime, rpb), True)
            assert (mu <= CR.MEAN_ULPS).all() and (vr <= 1).all(), (name, form, ranks, regime, rpb, mu.max(), vr.max())


@pytest.mark.parametrize("regime", ["rank_shift50", "rank_const"])
def test_a_merge_without_its_cross_term_is_outside_the_bounds(regime):
    """the bounds tell: the rank merge without d^2 n nb / nt, in fp64, on the heterogeneous regimes"""
    d = SC.layer_data("fast_64", "unet", 2, regime, "normal")
    y = CR.layer_forward(d["sources"], d["w"], d["bias"], d["gamma"], d["beta"], **d["kw"])["y"]
    n, mean, M2 = CR.shard_moments(y, 2)
    _, v64 = CR.channel_stats(y)
    wrong = M2.sum(0) / n.sum(0)
    ve = CR.var_error(wrong + CR.EPS, v64) / CR.var_bound(*CR.channel_stats(y))
    assert (ve > 100).all(), ve.min()


# ---------------------------------------------------------------- (3) metrics from sums, fp64
def unet_metrics_from_sums(s):
    """head_finalize_kernel's formulas: s = [sum lsoft, sum lsig, tp, predicted, wr tp, wr possible, voxels]"""
    eps = 1e-7
    M = s[6]
    lsoft, lsig = s[0] / M, s[1] / M
    precision, recall = s[2] / (s[3] + eps), s[2] / (M + eps)
    f1 = 2.0 * (precision * recall / (precision + recall + eps))
    return np.array([lsoft + lsig, lsoft, lsig, f1, s[4] / (s[5] + eps)])


def vae_sums(mulv, sq, pm, per, w):
    """vae_loss_kernel phase 1: {KL, squared error, weighted PM, B, n_elems}; sq (B, elems), pm: four (B, per[l]) arrays"""
    latent = mulv.shape[1] // 2
    mu, lv = mulv[:, :latent].astype(np.float64), mulv[:, latent:].astype(np.float64)
    kl = (-0.5 * (1.0 + lv - mu * mu - np.exp(lv))).sum()
    return np.array([kl, sq.sum(), sum(w[l] * pm[l].sum() / per[l] for l in range(4)), float(mulv.shape[0]), float(sq.size)])


def vae_metrics_from_sums(s, alpha, beta):
    mse, pm, kl = s[1] / s[4], s[2] / s[3], s[0] / s[3]
    return np.array([mse + alpha * pm + beta * kl, pm, mse, kl])


def vae_inputs(B, latent, seed, zero_weight=False):
    rng = np.random.default_rng(seed)
    mulv = np.concatenate([rng.standard_normal((B, latent)), rng.uniform(-20, 10, (B, latent))], 1).astype(np.float32)
    mulv[0, latent], mulv[-1, -1] = -20.0, 10.0
    per = (64.0, 32.0, 16.0, 8.0)
    sq = rng.uniform(0, 1, (B, 128))
    pm = [rng.uniform(0, 4, (B, int(p))) for p in per]
    w = np.array([1.0, 0.0, 0.5, 2.0] if zero_weight else [1.0, 0.75, 0.5, 2.0], np.float32)
    return mulv, sq, pm, per, w


@pytest.mark.parametrize("ranks", [2, 3, 4])
def test_unet_metrics_from_shard_sums(ranks):
    rng = np.random.default_rng(ranks)
    M = 512
    s = np.stack([np.concatenate([rng.uniform(0, 5 * M, 2), rng.integers(0, M, 4), [M]]) for _ in range(ranks)]).astype(np.float64)
    whole = unet_metrics_from_sums(s.sum(0))
    # the ratios are NOT the means of the per-shard ratios (f1 and wr are not linear): the sums must be what is added
    assert _rel(unet_metrics_from_sums(np.add.reduce(s, 0)), whole) <= TOL
    per_shard = np.mean([unet_metrics_from_sums(v) for v in s], 0)
    assert abs(per_shard[3] - whole[3]) > 1e-6 or abs(per_shard[4] - whole[4]) > 1e-6


@pytest.mark.parametrize("latent,B", [(20, 2), (256, 3)])
@pytest.mark.parametrize("ranks", [2, 3])
def test_vae_metrics_from_shard_sums(ranks, latent, B):
    mulv, sq, pm, per, w = vae_inputs(B * ranks, latent, seed=latent + ranks, zero_weight=True)
    whole = vae_metrics_from_sums(vae_sums(mulv, sq, pm, per, w), 0.5, 3e-4)
    tot = 0.0
    for r in range(ranks):
        sl = slice(r * B, (r + 1) * B)
        tot = tot + vae_sums(mulv[sl], sq[sl], [p[sl] for p in pm], per, w)
    assert _rel(vae_metrics_from_sums(tot, 0.5, 3e-4), whole) <= TOL


# ---------------------------------------------------------------- (4) decision caps of the GPU cases' seeds
CAP = 8


@pytest.mark.parametrize("name,form,ties,ranks", [v for v in SC.LINK_VARIANTS if v[3] == 2], ids=str)
def test_float32_decisions_of_the_link_seeds_stay_inside_the_caps(name, form, ties, ranks):
    t = "tf_cpu" if ties else "first"
    for regime, dr in SC.LINK_REGIMES:
        d = SC.link_data(name, form, ranks, regime, dr)
        f64 = LR.link_forward(d)
        f32 = LR.link_forward(d, np.float32)
        b = LR.link_backward(d, f64, LR.pins_of_forward(f32, form), t)
        worst = max(list(b["pinned"].values()) + [b["rerouted"]])
        print("  %-16s %-4s ties=%d P:%-12s dout:%-8s pinned %s rerouted %d" % (name, form, ties, regime, dr, b["pinned"], b["rerouted"]))
        if regime == "ratio1000":
            continue        # printed, not asserted: a float32 evaluation of the consumers flips up to 27 sides there
                            # (tests/test_conv_link_host.py); the engine's own decisions are asserted on the GPU
        assert worst <= CAP, (name, form, regime, dr, b["pinned"], b["rerouted"])
