"""Reference of ONE convolution layer as the engines run it (ics_op_conv_layer), from oracle/numpy_ref.py's pieces.

    virtual input V = channel concat over the sources of act(x * scale + shift), nearest-upsampled where flagged
                      (zero "same" padding is conv3d_fwd's, i.e. AFTER the affine)
    y = pre_act(conv(V, w) + bias)
    o = post_act(BN_train(y))                       (has_bn; biased batch variance, eps = 1e-3)

layer_forward / layer_backward evaluate this in any dtype: float64 is the reference, float32 gives e32, the error the
same formulas make in float32 numpy on the same inputs (the yardstick of the gradient bound in test_gpu_conv_layer.py).

Two modes of the statistics: from the reference's own y, or -- stored_y -- from the values the implementation under
test stored (fp64 statistics of those fp32 numbers), which isolates the statistics epilogue and the finalize kernel
from the convolution's own rounding.

Also here: the value regimes the statistics are tested in (regime_params), two float32 emulations of the statistic
(two-pass within blocks, merged in fp64, as the kernels do; and the one-pass sum a wrong kernel would do), and the
per-channel bounds (test_conv_layer_host.py calibrates them on the CPU)."""
import numpy as np

from oracle import numpy_ref as R

ACT = {0: None, 1: "relu", 2: "lrelu"}
EPS = float(np.float32(1e-3))            # kBnEps as the kernels hold it

# ---- the value regimes of y, one per output channel (channel c takes regime (c + off) % 7), set through bias and a
# per-channel weight scale; with unit-variance virtual inputs and w ~ N(0, 1 / fan_in) the conv part has std ~ 1
REGIMES = ("ratio0", "ratio30", "ratio1000", "constant", "dead", "tiny_std", "huge")
#           bias, weight scale
_REGIME = {"ratio0": (0.0, 1.0), "ratio30": (30.0, 1.0), "ratio1000": (1000.0, 1.0), "constant": (3.0, 0.0),
           "dead": (-1e3, 1.0), "tiny_std": (1.0, 1e-4), "huge": (1e4, 1e4)}
# var + eps recovered from rstd, relative to fp64 statistics of the stored values: 1e-5, except where mean >> std.  There
# the float32 block mean is off by d ~ ulp(mean) and a block's M2 about it enters the merged variance with an error of
# 2 d |mean_block - mean|, i.e. relative to var + eps proportional to x = |mean| std / (var + eps).  The two-pass float32
# emulation below (tree sums, blocks of 64..512 rows, 192..1536 rows, 4 seeds, both network forms) reaches 1.03e-8 x at
# x >= 100 and 3.7e-7 elsewhere (test_conv_layer_host.py prints both), so it lacks the 10x room inside 1e-5 from x ~ 100
# on and the bound there is 10x its error: 1.1e-7 x (1.1e-4 at mean/std = 1000, var ~ 1).  The one-pass emulation is at
# >= 1.66e-6 x there, 15x outside.
VAR_BOUND, VAR_BOUND_SLOPE = 1e-5, 1.1e-7


def var_bound(mean64, var64):
    mean64, var64 = np.asarray(mean64, np.float64), np.asarray(var64, np.float64)
    return np.maximum(VAR_BOUND, VAR_BOUND_SLOPE * np.abs(mean64) * np.sqrt(var64) / (var64 + EPS))


MEAN_ULPS = 4


def regime_of(c, off=0):
    """the regime of output channel c: (c + off) % 7 down the list, or -- off a regime's name -- that one in every channel"""
    return off if isinstance(off, str) else REGIMES[(c + off) % len(REGIMES)]


def regime_params(w, rng, off=0):
    """(w', bias): w rescaled per output channel and the bias that put channel c into regime_of(c, off)."""
    Cout = w.shape[-1]
    bias = np.array([_REGIME[regime_of(c, off)][0] for c in range(Cout)], np.float32)
    ws = np.array([_REGIME[regime_of(c, off)][1] for c in range(Cout)], np.float32)
    bias = bias * (1 + 0.01 * rng.standard_normal(Cout)).astype(np.float32)
    return (w * ws).astype(np.float32), bias.astype(np.float32)


def border_mask(S):
    """(S,S,S) bool: voxels with a zero-padded neighbour."""
    i = np.arange(S)
    e = (i == 0) | (i == S - 1)
    return e[:, None, None] | e[None, :, None] | e[None, None, :]


def virtual_input(sources, dtype=np.float64):
    parts = []
    for s in sources:
        v = np.asarray(s["x"], dtype)
        if s.get("scale") is not None:
            v = v * np.asarray(s["scale"], dtype) + np.asarray(s["shift"], dtype)
        v = R.act_fwd(v, ACT[int(s.get("act", 0))])
        if s.get("up"):
            v = R.upsample_fwd(v)
        parts.append(v)
    return np.concatenate(parts, -1) if len(parts) > 1 else parts[0]


def channel_stats(y):
    """fp64 (mean, biased var) per channel of any-dtype y."""
    yf = np.asarray(y, np.float64).reshape(-1, y.shape[-1])
    mean = yf.mean(0)
    return mean, ((yf - mean) ** 2).mean(0)


def layer_forward(sources, w, bias, gamma=None, beta=None, pre_act=0, has_bn=True, post_act=0, stored_y=None,
                  dtype=np.float64, eps=EPS):
    """Returns a dict: V, y (this evaluation's own), s (the y everything behind it is computed from: stored_y if given),
    and with has_bn mean, var, rstd, scale, shift, bn, o.  eps: the kernels' float32 1e-3 (numpy_ref.BN_EPS is the double)."""
    V = virtual_input(sources, dtype)
    w = np.asarray(w, dtype)
    b = np.zeros(w.shape[-1], dtype) if bias is None else np.asarray(bias, dtype)
    y = R.act_fwd(R.conv3d_fwd(V, w, b), ACT[pre_act])
    f = {"V": V, "y": y, "s": y if stored_y is None else np.asarray(stored_y, dtype), "eps": dtype(eps)}
    if has_bn:
        g, bt = np.asarray(gamma, dtype), np.asarray(beta, dtype)
        bn, mean, var = R.bn_train_fwd(f["s"], g, bt, eps=f["eps"])
        rstd = 1.0 / np.sqrt(var + f["eps"])
        f.update(mean=mean, var=var, rstd=rstd, scale=g * rstd, shift=bt - mean * g * rstd, bn=bn,
                 o=R.act_fwd(bn, ACT[post_act]))
    else:
        f["o"] = f["s"]
    return f


def layer_backward(f, sources, w, gamma, dout, pre_act=0, has_bn=True, post_act=0, kink_y=None, kink_bn=None):
    """Gradients of the layer given dout = dLoss/do, in the dtype of f.  kink_y / kink_bn: the implementation's stored y /
    its own fp32 BatchNorm output; they decide act'(.) (numpy_ref.apply_kink's rule).  Returns dw, dbias, dgamma, dbeta, dx
    (one per source: the gradient w.r.t. its part of V, summed over the 8 children where it is upsampled) and `pinned`,
    the number of decisions that differ from this evaluation's own."""
    dtype = f["y"].dtype.type
    w = np.asarray(w, dtype)
    d = np.asarray(dout, dtype)
    out = {"pinned": 0}
    if has_bn:
        dec = f["bn"] if kink_bn is None else np.asarray(kink_bn, dtype)
        if ACT[post_act] is not None:
            out["pinned"] += int(((dec > 0) != (f["bn"] > 0)).sum())
        d = R.act_bwd(dec, d, ACT[post_act])
        d, out["dgamma"], out["dbeta"] = R.bn_train_bwd(f["s"], np.asarray(gamma, dtype), f["mean"], f["var"], d, eps=f["eps"])
    dec = f["s"] if kink_y is None else np.asarray(kink_y, dtype)
    if ACT[pre_act] is not None:
        out["pinned"] += int(((dec > 0) != (f["y"] > 0)).sum())
    dy = R.act_bwd(dec, d, ACT[pre_act])
    dV, out["dw"], out["dbias"] = R.conv3d_bwd(f["V"], w, dy)
    out["dx"], c0 = [], 0
    for s in sources:
        C = np.asarray(s["x"]).shape[-1]
        g = dV[..., c0:c0 + C]
        out["dx"].append(R.upsample_bwd(g) if s.get("up") else g)
        c0 += C
    return out


# ---- float32 emulations of the per-channel statistic of stored values y (any shape, channels last)
def _tree_sum32(a):
    """float32 sum over axis 0 as a binary tree of adjacent pairs (a lane / wave / LDS reduction), not numpy's running sum"""
    a = np.asarray(a, np.float32)
    while a.shape[0] > 1:
        if a.shape[0] & 1:
            a = np.concatenate([a, np.zeros_like(a[:1])], 0)
        a = a[0::2] + a[1::2]
    return a[0]


def stats_two_pass32(y, rows_per_block):
    """What the kernels do: float32 mean, then float32 sum of squared deviations, within blocks of rows_per_block rows
    (a ragged last block keeps its own count); the blocks merged in fp64 as bn_finalize_kernel merges them."""
    yf = np.asarray(y, np.float32).reshape(-1, y.shape[-1])
    n = s = q = 0.0
    for r0 in range(0, yf.shape[0], rows_per_block):
        blk = yf[r0:r0 + rows_per_block]
        nb = np.float32(blk.shape[0])
        mb = (_tree_sum32(blk) / nb).astype(np.float32)
        m2 = _tree_sum32((blk - mb) ** 2)
        n = n + float(nb)
        s = s + float(nb) * mb.astype(np.float64)
        q = q + m2.astype(np.float64) + float(nb) * mb.astype(np.float64) ** 2
    mean = s / n
    return mean, np.maximum(q - n * mean * mean, 0.0) / n


def stats_one_pass32(y):
    """What a wrong kernel would do: E[x^2] - E[x]^2 with float32 sums."""
    yf = np.asarray(y, np.float32).reshape(-1, y.shape[-1])
    n = np.float32(yf.shape[0])
    mean = _tree_sum32(yf) / n
    ex2 = _tree_sum32(yf * yf) / n
    return mean.astype(np.float64), np.maximum(ex2 - mean * mean, np.float32(0)).astype(np.float64)


def ulps32(a, b, at=None):
    """|a - b| in float32 ulps at the magnitude `at` (default |b|)."""
    at = np.abs(np.asarray(b, np.float64)) if at is None else np.asarray(at, np.float64)
    sp = np.spacing(np.maximum(at, np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / sp


def var_error(var_plus_eps, var64):
    """relative error of a recovered var + eps against fp64 statistics"""
    return np.abs(np.asarray(var_plus_eps, np.float64) - (var64 + EPS)) / (var64 + EPS)


def check_bn_affine(name, stored, scale, shift, gamma, beta):
    """The engine's BatchNorm affine of a layer (scale = gamma rstd, shift = beta - mean scale) against fp64 statistics of
    the layer's own stored activations, per channel, with the bounds above.  mean and rstd are recovered in fp64 from the
    float32 affine: rstd carries scale's rounding (2.4e-7 of var + eps at most, far inside 1e-5), the mean shift's and
    scale's (1.5 ulps of |mean| at most while |beta| <= |mean scale|, as with the initial beta = 0 of these steps)."""
    m64, v64 = channel_stats(stored)
    g = np.asarray(gamma, np.float32).astype(np.float64)
    b = np.asarray(beta, np.float32).astype(np.float64)
    sc, sh = np.asarray(scale, np.float64), np.asarray(shift, np.float64)
    assert (g != 0).all() and (sc != 0).all(), name
    mean, rstd = (b - sh) / sc, sc / g
    mu = ulps32(mean, m64, at=np.maximum(np.abs(m64), np.sqrt(v64)))
    ve = var_error(1.0 / rstd ** 2, v64)
    bound = var_bound(m64, v64)
    assert (mu <= MEAN_ULPS).all(), (name, "mean", float(mu.max()), int(mu.argmax()))
    assert (ve <= bound).all(), (name, "var + eps", float(ve.max()), int((ve / bound).argmax()))
    return float(mu.max()), float((ve / bound).max())


# ---- the inputs of a case, shared by the host and the GPU tests
def make_case(B, S, src_spec, Cout, taps=27, form="unet", aff=True, seed=0, regime_off=None):
    """src_spec: [(C, up), ...].  form "unet": ReLU, BN, none; sources affine, no activation.  "vae": none, BN,
    LeakyReLU; sources affine + LeakyReLU.  "plain": no BatchNorm, plain sources, no activation.
    Source affines have scale in [0.5, 1.5] and |shift| in [0.5, 1] in every channel (a loader that pads before the affine
    is then wrong by act(shift) * sum of the border taps).  regime_off: None = ordinary values (bias ~ N(0, 1)); an int or a
    regime's name: see regime_of."""
    rng = np.random.default_rng(1000 + seed)
    k = 3 if taps == 27 else 1
    Cin = sum(c for c, _ in src_spec)
    sources = []
    for C, up in src_spec:
        s = S // 2 if up else S
        d = {"x": rng.standard_normal((B, s, s, s, C)).astype(np.float32), "up": int(up), "act": 0}
        if aff and form != "plain":
            d["scale"] = rng.uniform(0.5, 1.5, C).astype(np.float32)
            d["shift"] = (rng.uniform(0.5, 1.0, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
            d["act"] = 2 if form == "vae" else 0
        sources.append(d)
    w = (rng.standard_normal((k, k, k, Cin, Cout)) / np.sqrt(taps * Cin)).astype(np.float32)
    bias = rng.standard_normal(Cout).astype(np.float32)
    if regime_off is not None:
        w, bias = regime_params(w, rng, regime_off)
    kw = {"pre_act": 1 if form == "unet" else 0, "has_bn": form != "plain", "post_act": 2 if form == "vae" else 0}
    gamma = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    beta = rng.uniform(-0.5, 0.5, Cout).astype(np.float32)
    dout = rng.standard_normal((B, S, S, S, Cout)).astype(np.float32)
    return {"sources": sources, "w": w, "bias": bias, "gamma": gamma, "beta": beta, "dout": dout, "kw": kw}
