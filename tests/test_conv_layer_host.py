"""tests/conv_layer_ref.py on the CPU: (1) it reproduces single layers of numpy_ref.UnetOracle / VaeOracle, forward and
backward, from the oracles' caches to 1e-12; (2) calibration of the statistic bounds test_gpu_conv_layer.py and the
train-step tests apply (conv_layer_ref.var_bound, MEAN_ULPS) on every value regime: a float32 two-pass statistic within
blocks (what the kernels do) must sit >= 10x inside the bound, and where mean/std >= 100 a float32 one-pass
E[x^2] - E[x]^2 (what a wrong kernel would do) >= 10x outside it.

Calibration measured here (4 seeds, 192 / 1024 / 1536 rows, blocks of 64 / 128 / 256 / 512 rows, both network forms; relative
error of var + eps against fp64 statistics of the same float32 values; x = |mean| std / (var + eps), ~ mean/std for var >> eps):
    two-pass emulation   <= 3.7e-7 where x < 100 (ratio0, ratio30, constant, tiny_std, huge): 27x inside 1e-5
                         <= 1.03e-8 x where x >= 100 (ratio1000; dead in the VAE form): 1.0e-5 at mean/std = 1000, NOT 10x
                         inside 1e-5 -> the bound there is 10x the emulation, 1.1e-7 x (conv_layer_ref.var_bound)
    one-pass emulation   >= 1.66e-6 x where x >= 100: 15x outside that bound (2e-3 .. 4e-1 at mean/std = 1000)
    mean                 <= 1.5 float32 ulps of max(|mean|, std) (bound 4)
The exact figures are printed by test_statistic_bounds_are_calibrated (run with -s)."""
import numpy as np
import pytest

import conv_layer_ref as CR
from oracle import numpy_ref as R

TOL = 1e-12


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def _affine_source(c, P, name, up=0, act=0):
    """a producer block's stored s with its training-mode BatchNorm affine, as the engines hand it to the consumer"""
    inv = P[name + "/gamma"] / np.sqrt(c["var"] + R.BN_EPS)
    return {"x": c["s"], "scale": inv, "shift": P[name + "/beta"] - c["mean"] * inv, "up": up, "act": act}


def _check_block(blk, P, cache, sources, pre, post, rng):
    c = cache[blk.name]
    w, b, g, bt = (P[blk.name + k] for k in ("/kernel", "/bias", "/gamma", "/beta"))
    f = CR.layer_forward(sources, w, b, g, bt, pre, True, post, eps=R.BN_EPS)    # the oracles' epsilon: the double 1e-3
    assert _rel(f["V"], c["x"]) <= TOL and _rel(f["y"], c["s"]) <= TOL
    assert _rel(f["mean"], c["mean"]) <= TOL and _rel(f["var"], c["var"]) <= TOL
    assert _rel(f["bn"], c["bn"]) <= TOL
    do = rng.standard_normal(f["o"].shape)
    grads = {}
    dx_ref = blk.bwd(do, P, {}, cache, grads)
    bw = CR.layer_backward(f, sources, w, g, do, pre, True, post)
    assert bw["pinned"] == 0
    for k, name in (("dw", "/kernel"), ("dbias", "/bias"), ("dgamma", "/gamma"), ("dbeta", "/beta")):
        assert _rel(bw[k], grads[blk.name + name]) <= TOL, k
    return bw, dx_ref


@pytest.fixture(scope="module")
def unet_cache():
    o = R.UnetOracle(in_ch=1, num_classes=95, seed=1)
    x, _, _ = R.synthetic_batch(1, 16, 1, seed=0)
    cache = {}
    o._trunk(np.asarray(x, np.float64), True, cache)
    return o, cache


def test_reference_reproduces_unet_c2_plain_source(unet_cache):
    o, cache = unet_cache
    rng = np.random.default_rng(0)
    src = [{"x": cache["c2"]["x"]}]
    bw, dx_ref = _check_block(o.blocks["c2"], o.P, cache, src, 1, 0, rng)
    assert _rel(bw["dx"][0], dx_ref) <= TOL


def test_reference_reproduces_unet_c17_skip_up_affine_sources(unet_cache):
    o, cache = unet_cache
    rng = np.random.default_rng(1)
    src = [_affine_source(cache["c2"], o.P, "c2"), _affine_source(cache["c16"], o.P, "c16", up=1)]
    bw, dx_ref = _check_block(o.blocks["c17"], o.P, cache, src, 1, 0, rng)
    assert _rel(bw["dx"][0], dx_ref[..., :64]) <= TOL
    assert _rel(bw["dx"][1], R.upsample_bwd(dx_ref[..., 64:])) <= TOL


def test_reference_reproduces_vae_d2_upsampled_lrelu_source():
    v = R.VaeOracle(None, d=16)
    rng = np.random.default_rng(2)
    cache = {}
    v.decode(rng.standard_normal((2, 256)), rng.standard_normal((2, 10)), True, cache)
    src = [_affine_source(cache["d1"], v.P, "d1", up=1, act=2)]
    bw, dx_ref = _check_block(v.dec[2], v.P, cache, src, 0, 2, rng)
    assert _rel(bw["dx"][0], R.upsample_bwd(dx_ref)) <= TOL


def test_float32_evaluation_is_close_and_kinks_pin():
    """the float32 evaluation (e32's source) runs the same formulas, and a pinned decision is counted"""
    c = CR.make_case(2, 4, [(8, 0), (8, 1)], 8, form="vae", seed=3)
    f64 = CR.layer_forward(c["sources"], c["w"], c["bias"], c["gamma"], c["beta"], **c["kw"])
    f32 = CR.layer_forward(c["sources"], c["w"], c["bias"], c["gamma"], c["beta"], dtype=np.float32, **c["kw"])
    assert f32["y"].dtype == np.float32 and 0 < _rel(f32["y"], f64["y"]) < 1e-5
    b64 = CR.layer_backward(f64, c["sources"], c["w"], c["gamma"], c["dout"], **c["kw"])
    b32 = CR.layer_backward(f32, c["sources"], c["w"], c["gamma"], c["dout"], **c["kw"])
    assert b32["dw"].dtype == np.float32 and _rel(b32["dw"], b64["dw"]) < 1e-4
    flipped = f64["bn"].copy()
    flipped.flat[0] = -flipped.flat[0]
    assert CR.layer_backward(f64, c["sources"], c["w"], c["gamma"], c["dout"], kink_bn=flipped, **c["kw"])["pinned"] == 1
    assert b64["dx"][1].shape == c["sources"][1]["x"].shape


def test_stored_y_mode_takes_statistics_from_the_stored_values():
    c = CR.make_case(3, 4, [(8, 0)], 7, form="unet", seed=4, regime_off=0)
    f = CR.layer_forward(c["sources"], c["w"], c["bias"], c["gamma"], c["beta"], **c["kw"])
    y32 = f["y"].astype(np.float32)
    g = CR.layer_forward(c["sources"], c["w"], c["bias"], c["gamma"], c["beta"], stored_y=y32, **c["kw"])
    m, v = CR.channel_stats(y32)
    assert np.array_equal(g["mean"], m) and np.allclose(g["var"], v, rtol=1e-13, atol=0)
    assert np.array_equal(g["y"], f["y"])


def test_statistic_bounds_are_calibrated():
    """the calibration table of the module docstring"""
    print("\nregime     form  rows  rpb   mean/std  x=|m|s/(v+eps)  two-pass(var)  one-pass(var)      bound  mean ulps")
    k_in = other_in = 0.0
    k_out = np.inf
    for form in ("unet", "vae"):
        for B, S in ((3, 4), (3, 8), (2, 8)):          # 192 rows (ragged on 128), 1536, 1024
            for seed in range(4):
                c = CR.make_case(B, S, [(16, 0)], 14, form=form, seed=seed, regime_off=0)
                f = CR.layer_forward(c["sources"], c["w"], c["bias"], c["gamma"], c["beta"], **c["kw"])
                y32 = f["y"].astype(np.float32)
                m64, v64 = CR.channel_stats(y32)
                std = np.sqrt(v64)
                x = np.abs(m64) * std / (v64 + CR.EPS)
                bound = CR.var_bound(m64, v64)
                _, v1 = CR.stats_one_pass32(y32)
                e1 = CR.var_error(v1 + CR.EPS, v64)
                for rpb in (64, 128, 256, 512):
                    m2, v2 = CR.stats_two_pass32(y32, rpb)
                    e2 = CR.var_error(v2 + CR.EPS, v64)
                    u2 = CR.ulps32(np.float32(m2), m64, at=np.maximum(np.abs(m64), std))
                    for ch in range(14):
                        r = CR.regime_of(ch)
                        ratio = abs(m64[ch]) / std[ch] if std[ch] > 0 else np.inf
                        if seed == 0 and rpb == 128 and ch < 7:
                            print("%-9s  %-4s  %4d  %3d  %9.3g  %14.3g  %13.3g  %13.3g  %9.3g  %6.2f"
                                  % (r, form, y32.size // 14, rpb, ratio, x[ch], e2[ch], e1[ch], bound[ch], u2[ch]))
                        assert e2[ch] * 10 <= bound[ch], (r, form, rpb, e2[ch], bound[ch])
                        assert u2[ch] * 2 <= CR.MEAN_ULPS, (r, form, rpb, u2[ch])
                        if x[ch] >= 100:
                            k_in = max(k_in, e2[ch] / x[ch])
                            # a one-pass statistic must be caught wherever mean/std >= 100 (and var is visible next to eps)
                            assert e1[ch] >= 10 * bound[ch], (r, form, e1[ch], bound[ch])
                            k_out = min(k_out, e1[ch] / x[ch])
                        else:
                            other_in = max(other_in, e2[ch])
    print("two-pass: %.3g x at x >= 100, %.3g elsewhere; one-pass: >= %.3g x; bound max(%g, %g x)"
          % (k_in, other_in, k_out, CR.VAR_BOUND, CR.VAR_BOUND_SLOPE))
    assert 10 * k_in <= CR.VAR_BOUND_SLOPE <= k_out / 10 and 10 * other_in <= CR.VAR_BOUND


def test_two_pass_emulation_handles_a_ragged_last_block():
    rng = np.random.default_rng(5)
    y = (1000.0 + rng.standard_normal((3, 4, 4, 4, 5))).astype(np.float32)     # 192 rows on 128-row blocks
    m64, v64 = CR.channel_stats(y)
    m2, v2 = CR.stats_two_pass32(y, 128)
    assert (CR.var_error(v2 + CR.EPS, v64) * 10 <= CR.var_bound(m64, v64)).all()
    # ... and a merge that takes the ragged block for a full one is far outside the bound
    yf = y.reshape(-1, 5)
    mb = [yf[:128].mean(0), yf[128:].mean(0)]
    wrong_mean = (mb[0] + mb[1]) / 2
    assert CR.ulps32(wrong_mean, m64, at=np.maximum(np.abs(m64), np.sqrt(v64))).max() > 10 * CR.MEAN_ULPS


def test_a_named_regime_fills_every_channel():
    """regime_off = "ratio30" (the backward runs of test_gpu_conv_layer.py): every output channel of the reference sits
    at mean/std ~ 30, the U-Net form's ReLU is open at every voxel, and |BN(y)| < 1e-4 -- where a float32 affine could
    decide a LeakyReLU the other way -- holds for fewer than 8 voxels"""
    for form in ("unet", "vae"):
        c = CR.make_case(3, 4, [(8, 0), (8, 1)], 9, form=form, seed=6, regime_off="ratio30")
        f = CR.layer_forward(c["sources"], c["w"], c["bias"], c["gamma"], c["beta"], **c["kw"])
        m64, v64 = CR.channel_stats(f["y"])
        ratio = np.abs(m64) / np.sqrt(v64)
        assert all(CR.regime_of(ch, "ratio30") == "ratio30" for ch in range(9))
        assert (ratio > 15).all() and (ratio < 100).all(), ratio       # bias 30, conv part of std 0.45 .. 1.5 (LeakyReLU sources: less)
        assert form == "vae" or (f["y"] > 0).all()
        assert int((np.abs(f["bn"]) < 1e-4).sum()) < 8


# ---- condition sources (the VAE's e0): the reference is the plain one on the materialised input; the fold's formulas are
# written out here, and only here, to show on the CPU that the fold is an exact reassociation of that convolution
def _valid(t, c):
    """tap offset t - 1 from a voxel of class c (0 first plane, 1 interior, 2 last plane) stays inside the grid"""
    return not ((t == 0 and c == 0) or (t == 2 and c == 2))


def fold_forward(x, cond, w, bias):
    """cond_bias_table_kernel + the pos_bias epilogue: the convolution of the x channels alone plus a bias that depends on
    the sample and on the voxel's border class (first / interior / last plane per axis: 27 classes)"""
    B, S, C = x.shape[0], x.shape[1], x.shape[-1]
    ncond, Cout = cond.shape[1], w.shape[-1]
    nfold = w.shape[3] - C
    cv = np.tile(cond, (1, nfold // ncond))                                  # (B, nfold): channel j = cond[b][j % ncond]
    y = R.conv3d_fwd(x, w[..., :C, :], np.zeros(Cout))
    cls = np.where(np.arange(S) == 0, 0, np.where(np.arange(S) == S - 1, 2, 1))
    T = np.zeros((B, 3, 3, 3, Cout)) + bias
    for cz, cy, cx, tz, ty, tx in np.ndindex(3, 3, 3, 3, 3, 3):
        if _valid(tz, cz) and _valid(ty, cy) and _valid(tx, cx):
            T[:, cz, cy, cx] += cv @ w[tz, ty, tx, C:, :]
    return y + T[:, cls[:, None, None], cls[None, :, None], cls[None, None, :]]


def fold_dw_cond(dy, cond, nfold):
    """sample_colsum / border_region_sums / cond_wgrad_kernel: the 26 border regions of dy summed directly, the interior one
    as total - border, D[b][tap] = the sum of the regions the tap is valid for, dw[tap][C + j] = sum_b cond[b][j % ncond] D"""
    B, S, Cout = dy.shape[0], dy.shape[1], dy.shape[-1]
    sl = lambda c: slice(0, 1) if c == 0 else (slice(1, S - 1) if c == 1 else slice(S - 1, S))
    Rg = np.zeros((B, 3, 3, 3, Cout))
    for cz, cy, cx in np.ndindex(3, 3, 3):
        if (cz, cy, cx) != (1, 1, 1):
            Rg[:, cz, cy, cx] = dy[:, sl(cz), sl(cy), sl(cx)].sum((1, 2, 3))
    Rg[:, 1, 1, 1] = dy.sum((1, 2, 3)) - Rg.sum((1, 2, 3))
    cv = np.tile(cond, (1, nfold // cond.shape[1]))
    dw = np.zeros((3, 3, 3, nfold, Cout))
    for tz, ty, tx in np.ndindex(3, 3, 3):
        D = sum(Rg[:, cz, cy, cx] for cz, cy, cx in np.ndindex(3, 3, 3) if _valid(tz, cz) and _valid(ty, cy) and _valid(tx, cx))
        dw[tz, ty, tx] = cv.T @ D
    return dw


@pytest.mark.parametrize("S", (4, 8))
@pytest.mark.parametrize("C,ncond", ((1, 1), (1, 3), (1, 10), (3, 1)))
def test_condition_fold_is_an_exact_reassociation(S, C, ncond):
    """fp64, forward and dw, S = 4 and 8, C * ncond in {1, 3, 10} (and 3 = 3 x channels x 1): the fold's formulas equal the
    convolution over the materialised input to rounding.  dy has a per-channel mean of ~1: the totals do not cancel."""
    rng = np.random.default_rng(10 * S + C + ncond)
    B, Cout, nfold = 3, 5, C * ncond
    x, cond = rng.standard_normal((B, S, S, S, C)), rng.standard_normal((B, ncond))
    w, bias = rng.standard_normal((3, 3, 3, C + nfold, Cout)), rng.standard_normal(Cout)
    dy = rng.standard_normal((B, S, S, S, Cout)) + 1.0
    src = [{"x": x}, {"x": cond, "bcast": ncond, "C": nfold}]
    f = CR.layer_forward(src, w, bias, has_bn=False)
    assert f["V"].shape == (B, S, S, S, C + nfold)
    assert _rel(fold_forward(x, cond, w, bias), f["y"]) <= TOL
    b = CR.layer_backward(f, src, w, None, dy, has_bn=False)
    assert b["dx"][1] is None and b["dx"][0].shape == x.shape
    assert _rel(fold_dw_cond(dy, cond, nfold), b["dw"][..., C:, :]) <= TOL
    g = CR.dw_row_groups(b["dw"], C)
    assert g["dw_x"].shape == (3, 3, 3, C, Cout) and g["dw_cond_other"].shape == (26, nfold, Cout)
    assert np.array_equal(g["dw_cond_centre"], b["dw"][1, 1, 1, C:, :])


def test_condition_channels_are_tiled_not_repeated():
    """at C = 4 np.tile and np.repeat differ; the reference's channel order is numpy_ref.VaeOracle's own e0 input"""
    rng = np.random.default_rng(11)
    B, d, C, ncond = 2, 4, 4, 3
    v = R.VaeOracle(None, in_ch=C, cond=ncond, d=16)
    cond = rng.standard_normal((B, ncond))
    x = rng.standard_normal((B, d, d, d, C))
    V = CR.virtual_input([{"x": x}, {"x": cond, "bcast": ncond, "C": C * ncond}])
    want = np.concatenate([x, v.tile_cond(cond, d)], -1)
    assert np.array_equal(V, want)
    rep = np.broadcast_to(np.repeat(cond, C, axis=1)[:, None, None, None, :], (B, d, d, d, C * ncond))
    assert not np.array_equal(V[..., C:], rep)
    for c in range(C * ncond):
        assert np.array_equal(V[:, 1, 2, 3, C + c], cond[:, c % ncond])


def _cond_variants():
    out = []
    for name, cases in (("cond_fold", CR.COND_FOLD_CASES), ("cond_bcast", CR.COND_BCAST_CASES)):
        for i, c in enumerate(cases):
            out += [(name, i, c, form, None) for form in ("unet", "vae")]
        out += [(name, 1, cases[1], form, reg) for form in ("unet", "vae") for reg in CR.COND_REGIMES]
    return out


@pytest.mark.parametrize("name,idx,case,form,regime", _cond_variants(), ids=lambda v: str(v) if not isinstance(v, tuple) else "c")
def test_condition_cases_pin_few_decisions_and_have_a_yardstick(name, idx, case, form, regime):
    """every condition case of test_gpu_conv_layer.py (seeds as there), the reference alone: the float32 evaluation's
    activation decisions differ from the fp64 reference's at no more than 8 voxels per tensor -- the cap the GPU test puts
    on pinned decisions -- and its gradients (with the fp64 decisions: rounding alone) are finite, non-zero yardsticks."""
    B, S, src, Cout = case
    seed = {"cond_fold": 90, "cond_bcast": 100}[name] + idx
    c = CR.make_case(B, S, src, Cout, 27, form, False, seed, cond_regime=regime)
    args = (c["sources"], c["w"], c["bias"], c["gamma"], c["beta"])
    f64 = CR.layer_forward(*args, **c["kw"])
    f32 = CR.layer_forward(*args, dtype=np.float32, **c["kw"])
    pins = CR.layer_backward(f64, c["sources"], c["w"], c["gamma"], c["dout"], kink_y=f32["y"], kink_bn=f32["bn"], **c["kw"])
    assert pins["pinned"] <= 8, pins["pinned"]
    b64 = CR.layer_backward(f64, c["sources"], c["w"], c["gamma"], c["dout"], **c["kw"])
    b32 = CR.layer_backward(f32, c["sources"], c["w"], c["gamma"], c["dout"], kink_y=f64["y"], kink_bn=f64["bn"], **c["kw"])
    for k, e in CR.row_group_errors(b32["dw"], b64["dw"], c["sources"], c["kw"]).items():
        assert np.isfinite(e) and 0 < e < 1e-3, (k, e)
