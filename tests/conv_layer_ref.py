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
per-channel bounds (test_conv_layer_host.py calibrates them on the CPU).

Data-parallel ranks with SyncBN (ics_conv_layer.ranks): the reference of R ranks at B samples each IS this reference on
the concatenated batch of R B.  ranks = R in layer_forward / layer_backward evaluates the same thing by the SHARDED route
instead -- per-shard (n, mean, M2) merged in rank order, per-shard (sum d, sum d xhat) added over the ranks, dy from the
global sums -- which tests/test_syncbn_host.py shows equal to the whole-batch route at 1e-12; shard_grads gives each
rank's local parameter gradients (its shard's contribution under the global statistics).  rank_regimes builds the
rank-heterogeneous inputs, stats_sharded32 the float32 emulation of the kernels' two merges."""
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


def materialised_condition(cond, C, shape, dtype=np.float64):
    """The VAE encoder's Reshape -> K.tile -> Concatenate (lattice_vae.py:167-169; numpy_ref.VaeOracle.tile_cond): cond
    (B, ncond) becomes C spatially constant channels, channel c = cond[b][c % ncond] -- np.tile, NOT np.repeat (the two
    differ as soon as C > ncond, i.e. with more than one x channel).  shape: (B, S, S, S) of the layer's input."""
    cond = np.asarray(cond, dtype)
    B, ncond = cond.shape
    assert C % ncond == 0 and shape[0] == B
    return np.broadcast_to(np.tile(cond, (1, C // ncond))[:, None, None, None, :], tuple(shape) + (C,)).copy()


def virtual_input(sources, dtype=np.float64):
    """A condition source ("bcast": ncond, "C", "x": (B, ncond)) is materialised: the reference of such a layer IS the plain
    reference applied to [x | tile(cond) broadcast over space], nothing cleverer."""
    parts = []
    for s in sources:
        if s.get("bcast"):
            parts.append(materialised_condition(s["x"], int(s["C"]), parts[0].shape[:4], dtype))
            continue
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


def shard_moments(s, R):
    """(n, mean, M2), each (R, C): the moments of the R equal shards of s (R B, ..., C), rank-major"""
    xs = np.asarray(s).reshape(R, -1, s.shape[-1])
    mean = xs.mean(1)
    return np.full(mean.shape, float(xs.shape[1])), mean, ((xs - mean[:, None]) ** 2).sum(1)


def merge_moments(n, mean, M2):
    """Chan et al., in rank order, as bn_sync_finalize_kernel: (n, mean, biased variance) of the global batch"""
    nt, mt, qt = np.zeros_like(mean[0]), np.zeros_like(mean[0]), np.zeros_like(mean[0])
    for nb, mb, qb in zip(n, mean, M2):
        tot, d = nt + nb, mb - mt
        qt = qt + qb + d * d * nt * nb / tot
        mt = mt + d * nb / tot
        nt = tot
    return nt, mt, qt / nt


def moving_after_one_update(mean, var, n, unbias=True, momentum=0.99):
    """the moving statistics after one update from (0, 1): the variance fed to the average is rescaled by n / (n - (1 + eps))
    with n the number of rows of the GLOBAL batch (numpy_ref's note on the Keras 2.3 quirk)"""
    v = var * (n / (n - (1.0 + EPS))) if unbias else var
    return mean * (1 - momentum), momentum + v * (1 - momentum)


def bn_bwd_sharded(s, gamma, mean, var, d, R, eps):
    """numpy_ref.bn_train_bwd by the SyncBN route: every shard's (sum d, sum d xhat), added in rank order, divided by the
    global count.  Returns dx and the PER-SHARD dgamma, dbeta, each (R, C)."""
    C = s.shape[-1]
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (s - mean) * rstd
    s1r = d.reshape(R, -1, C).sum(1)
    s2r = (d * xhat).reshape(R, -1, C).sum(1)
    s1, s2 = 0.0, 0.0
    for r in range(R):
        s1, s2 = s1 + s1r[r], s2 + s2r[r]
    n = s.size // C
    return (gamma * rstd) * (d - s1 / n - xhat * (s2 / n)), s2r, s1r


def layer_forward(sources, w, bias, gamma=None, beta=None, pre_act=0, has_bn=True, post_act=0, stored_y=None,
                  dtype=np.float64, eps=EPS, ranks=0):
    """Returns a dict: V, y (this evaluation's own), s (the y everything behind it is computed from: stored_y if given),
    and with has_bn mean, var, rstd, scale, shift, bn, o.  eps: the kernels' float32 1e-3 (numpy_ref.BN_EPS is the double)."""
    V = virtual_input(sources, dtype)
    w = np.asarray(w, dtype)
    b = np.zeros(w.shape[-1], dtype) if bias is None else np.asarray(bias, dtype)
    y = R.act_fwd(R.conv3d_fwd(V, w, b), ACT[pre_act])
    f = {"V": V, "y": y, "s": y if stored_y is None else np.asarray(stored_y, dtype), "eps": dtype(eps)}
    if has_bn:
        g, bt = np.asarray(gamma, dtype), np.asarray(beta, dtype)
        mom = None if ranks < 2 else (lambda x: merge_moments(*shard_moments(x, ranks))[1:])
        bn, mean, var = R.bn_train_fwd(f["s"], g, bt, eps=f["eps"], moments=mom)
        rstd = 1.0 / np.sqrt(var + f["eps"])
        f.update(mean=mean, var=var, rstd=rstd, scale=g * rstd, shift=bt - mean * g * rstd, bn=bn,
                 o=R.act_fwd(bn, ACT[post_act]))
    else:
        f["o"] = f["s"]
    return f


def layer_backward(f, sources, w, gamma, dout, pre_act=0, has_bn=True, post_act=0, kink_y=None, kink_bn=None, ranks=0,
                   strict_dtype=False):
    """Gradients of the layer given dout = dLoss/do, in the dtype of f.  kink_y / kink_bn: the implementation's stored y /
    its own fp32 BatchNorm output; they decide act'(.) (numpy_ref.apply_kink's rule).  Returns dw, dbias, dgamma, dbeta, dx
    (one per source: the gradient w.r.t. its part of V, summed over the 8 children where it is upsampled) and `pinned`,
    the number of decisions that differ from this evaluation's own.
    strict_dtype: numpy_ref.act_bwd multiplies by np.where(x > 0, 1.0, 0.3) for the LeakyReLU, a float64 array, so behind
    it a float32 evaluation silently continues in float64 (sums, c1 / c2, dy, the convolution's gradients) and its error
    against fp64 is that of the forward pass alone; True casts back to the evaluation's dtype after each activation, which
    is what "the plain formulas in float32" means.  tests/test_gpu_syncbn.py takes e32 this way; the older tests keep
    the yardstick they were calibrated with (in the LeakyReLU form a smaller, i.e. stricter, one)."""
    dtype = f["y"].dtype.type
    w = np.asarray(w, dtype)
    d = np.asarray(dout, dtype)
    out = {"pinned": 0}
    if has_bn:
        dec = f["bn"] if kink_bn is None else np.asarray(kink_bn, dtype)
        if ACT[post_act] is not None:
            out["pinned"] += int(((dec > 0) != (f["bn"] > 0)).sum())
        d = R.act_bwd(dec, d, ACT[post_act])
        if strict_dtype:
            d = np.asarray(d, dtype)
        out["d_bn"] = d
        if ranks < 2:
            d, out["dgamma"], out["dbeta"] = R.bn_train_bwd(f["s"], np.asarray(gamma, dtype), f["mean"], f["var"], d, eps=f["eps"])
        else:
            d, dg, db = bn_bwd_sharded(f["s"], np.asarray(gamma, dtype), f["mean"], f["var"], d, ranks, f["eps"])
            out["dgamma"], out["dbeta"] = dg.sum(0), db.sum(0)
    dec = f["s"] if kink_y is None else np.asarray(kink_y, dtype)
    if ACT[pre_act] is not None:
        out["pinned"] += int(((dec > 0) != (f["y"] > 0)).sum())
    dy = R.act_bwd(dec, d, ACT[pre_act])
    if strict_dtype:
        dy = np.asarray(dy, dtype)
    out["dy"] = dy
    dV, out["dw"], out["dbias"] = R.conv3d_bwd(f["V"], w, dy)
    out["dx"], c0 = [], 0
    for s in sources:
        if s.get("bcast"):               # no gradient w.r.t. the condition: the engines never take it
            out["dx"].append(None)
            continue
        C = np.asarray(s["x"]).shape[-1]
        g = dV[..., c0:c0 + C]
        out["dx"].append(R.upsample_bwd(g) if s.get("up") else g)
        c0 += C
    return out


def dw_row_groups(dw, C):
    """The row groups of a condition layer's kernel gradient (k, k, k, Cin, Cout) -- they come from different kernels (the x
    rows [0, C) from a stencil or GEMM reduction, the condition rows [C, Cin) from region sums of dy) and differ in scale
    by the ratio |cond| / |x|; inside the condition rows the centre tap is the only one whose sum is total - border alone."""
    dw = np.asarray(dw)
    k = dw.shape[0] // 2
    other = np.ones(dw.shape[:3], bool)
    other[k, k, k] = False
    return {"dw_x": dw[..., :C, :], "dw_cond": dw[..., C:, :], "dw_cond_centre": dw[k, k, k, C:, :],
            "dw_cond_other": dw[other][:, C:, :]}


def row_group_errors(got_dw, ref_dw, sources, kw, linear=False):
    """name -> error of each row group of got_dw, relative to the largest entry of the same group of ref_dw.
    One exception, decided from the inputs alone: behind a batch-statistics BatchNorm that follows the convolution directly
    (no pre-activation, or a ReLU the reference finds open everywhere) dy sums to zero per channel over the batch, and the
    centre tap -- valid for every voxel -- multiplies each condition by that sum's per-sample parts: when every sample has
    the SAME condition its gradient is exactly zero and the reference holds rounding noise there.  It is then measured on
    the scale of the condition rows (as the bias gradient of such a layer is measured on the kernel gradient's)."""
    C = np.asarray(sources[0]["x"]).shape[-1]
    cond = np.asarray(sources[1]["x"])
    zero_centre = bool(kw["has_bn"]) and (not kw["pre_act"] or linear) and bool((cond == cond[0]).all())
    g, r = dw_row_groups(got_dw, C), dw_row_groups(ref_dw, C)
    out = {}
    for k in r:
        scale = np.abs(r[k]).max()
        if k == "dw_cond_centre" and zero_centre:
            scale = max(scale, np.abs(r["dw_cond"]).max())
        out[k] = float(np.abs(np.asarray(g[k], np.float64) - r[k]).max() / max(scale, 1e-300))
    return out


def shard_grads(f, b, w, R, has_bn=True):
    """Each rank's LOCAL parameter gradients given the layer's forward f and backward b (of the global batch): the
    contribution of its shard, with the global statistics.  A list of R dicts dw, dbias, (dgamma, dbeta)."""
    dtype = f["y"].dtype.type
    w = np.asarray(w, dtype)
    B = f["V"].shape[0] // R
    out = []
    if has_bn:
        xhat = (f["s"] - f["mean"]) * f["rstd"]
        C = xhat.shape[-1]
        dg = (b["d_bn"] * xhat).reshape(R, -1, C).sum(1)
        db = b["d_bn"].reshape(R, -1, C).sum(1)
    for r in range(R):
        sl = slice(r * B, (r + 1) * B)
        _, dw, dbias = R_conv3d_bwd(f["V"][sl], w, b["dy"][sl])
        g = {"dw": dw, "dbias": dbias}
        if has_bn:
            g.update(dgamma=dg[r], dbeta=db[r])
        out.append(g)
    return out


def R_conv3d_bwd(V, w, dy):
    return R.conv3d_bwd(V, w, dy)


# ---- rank-heterogeneous value regimes of y: input channel 0 is the CARRIER, constant within a rank; an output channel in
# one of these regimes reads it through its centre tap only (which never meets the zero padding), so its y is the
# ordinary conv part (std ~ 1) plus a per-rank constant, or -- "rank_const", "rank_zero" -- that constant alone
RANK_REGIMES = ("rank_shift50", "rank_const", "rank_zero", "rank_std100")


def rank_regimes(case, R, regime):
    """`case` (make_case's dict, or link_case_view of a make_link dict) rewritten IN PLACE for R ranks, every output channel:
      rank_shift50  shard r shifted by 50 r conv-part standard deviations (d^2 n nb / nt carries nearly all the variance)
      rank_const    constant within every rank, 3 + 2 r on rank r (every local M2 is 0)
      rank_zero     identically zero on rank R - 1, ordinary elsewhere (that rank's virtual input and the bias are zero)
      rank_std100   the virtual inputs of the even ranks divided by 100, bias 0: shards with std in the ratio 1 : 100
    The carrier regimes need a first source that is not upsampled and at least 2 channels wide."""
    srcs, w = case["sources"], case["w"]
    R_B = srcs[0]["x"].shape[0]
    B = R_B // R
    if regime in ("rank_zero", "rank_std100"):
        case["bias"][:] = 0
        for src in srcs:
            x = src["x"]
            if regime == "rank_zero":
                if "shift" in src:
                    src["shift"][:] = 0
                x[(R - 1) * B:] = 0
                continue
            sc = np.asarray(src.get("scale", np.ones(x.shape[-1])), np.float64)
            sh = np.asarray(src.get("shift", np.zeros(x.shape[-1])), np.float64)
            for r in range(0, R, 2):      # x' with x' sc + sh = (x sc + sh) / 100 (an activation in between is positively homogeneous)
                xs = x[r * B:(r + 1) * B].astype(np.float64)
                x[r * B:(r + 1) * B] = (((xs * sc + sh) / 100.0 - sh) / sc).astype(np.float32)
        return case
    src = srcs[0]
    x = src["x"]
    assert x.shape[-1] >= 2 and not src.get("up"), "no carrier channel"     # (the values are >= 0: an activation keeps them)
    sc0 = float(src["scale"][0]) if "scale" in src else 1.0
    sh0 = float(src["shift"][0]) if "shift" in src else 0.0
    value = {"rank_shift50": lambda r: 50.0 * r, "rank_const": lambda r: 3.0 + 2.0 * r}[regime]
    for r in range(R):          # the carrier's VIRTUAL value on rank r is value(r)
        x[r * B:(r + 1) * B, ..., 0] = np.float32((value(r) - sh0) / sc0)
    k = w.shape[0] // 2
    w[..., 0, :] = 0
    w[k, k, k, 0, :] = 1
    if regime == "rank_const":
        w[..., 1:, :] = 0
        case["bias"][:] = 0
    return case


def rank_dout(dout, R, regime, seed=0):
    """the output gradient's regimes: "normal" as it is, "mean30" every column with a mean of 30x its std, "one_rank" zero
    on every rank but the last"""
    g = np.array(dout, np.float32)
    if regime == "mean30":
        g += (30.0 * np.random.default_rng(seed).choice([-1.0, 1.0], g.shape[-1])).astype(np.float32)
    elif regime == "one_rank":
        g[:g.shape[0] // R * (R - 1)] = 0
    else:
        assert regime == "normal"
    return g


def stats_sharded32(y, R, rows_per_block):
    """What the SyncBN kernels do: float32 two-pass block partials (as stats_two_pass32), bn_local_merge_kernel's fp64 merge
    to the shard's (n, mean, M2) about the SHARD's mean, bn_sync_finalize_kernel's fp64 merge in rank order, and rstd
    through float(1 / sqrt(var + eps)).  Returns (mean fp64, var + eps recovered from the float32 rstd, float32 mean)."""
    yf = np.asarray(y, np.float32).reshape(R, -1, y.shape[-1])
    n, mean, M2 = [], [], []
    for r in range(R):
        nb, mb, qb = [], [], []
        for r0 in range(0, yf.shape[1], rows_per_block):
            blk = yf[r, r0:r0 + rows_per_block]
            c = np.float32(blk.shape[0])
            m = (_tree_sum32(blk) / c).astype(np.float32)
            nb.append(float(c)); mb.append(m.astype(np.float64)); qb.append(_tree_sum32((blk - m) ** 2).astype(np.float64))
        nb, mb, qb = np.array(nb)[:, None], np.array(mb), np.array(qb)
        nr = nb.sum(0)
        mr = (nb * mb).sum(0) / nr
        n.append(nr); mean.append(mr); M2.append((qb + nb * (mb - mr) ** 2).sum(0))
    _, mt, var = merge_moments(n, mean, M2)
    rstd = (1.0 / np.sqrt(var + EPS)).astype(np.float32)
    return mt, 1.0 / rstd.astype(np.float64) ** 2, mt.astype(np.float32)


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
COND_REGIMES = ("same", "zero_sample", "huge")


def make_case(B, S, src_spec, Cout, taps=27, form="unet", aff=True, seed=0, regime_off=None, cond_regime=None,
              dout_mean=None):
    """src_spec: [(C, up), ...], the last of two possibly (C, 0, ncond): a condition source (virtual_input), always plain.
    form "unet": ReLU, BN, none; sources affine, no activation.  "vae": none, BN,
    LeakyReLU; sources affine + LeakyReLU.  "plain": no BatchNorm, plain sources, no activation.
    Source affines have scale in [0.5, 1.5] and |shift| in [0.5, 1] in every channel (a loader that pads before the affine
    is then wrong by act(shift) * sum of the border taps).  regime_off: None = ordinary values (bias ~ N(0, 1)); an int or a
    regime's name: see regime_of.
    cond_regime (condition N(0, 1) otherwise): "same" every sample the same condition; "zero_sample" the last sample's all
    zero; "huge" conditions of magnitude 1e3 next to x of magnitude 1.  dout_mean: added to dout per channel, +-dout_mean
    (1 + 0.1 N(0, 1)) -- with has_bn = 0 dout is dy and its per-sample totals then do not cancel."""
    rng = np.random.default_rng(1000 + seed)
    k = 3 if taps == 27 else 1
    Cin = sum(sp[0] for sp in src_spec)
    sources = []
    for sp in src_spec:
        C, up = sp[0], sp[1]
        if len(sp) > 2 and sp[2]:
            cond = rng.standard_normal((B, sp[2])).astype(np.float32)
            if cond_regime == "same":
                cond[:] = cond[0]
            elif cond_regime == "zero_sample":
                cond[-1] = 0
            elif cond_regime == "huge":
                cond = (1e3 * rng.choice([-1.0, 1.0], cond.shape) * rng.uniform(0.5, 1.5, cond.shape)).astype(np.float32)
            else:
                assert cond_regime is None
            sources.append({"x": cond, "bcast": int(sp[2]), "C": int(C), "up": 0, "act": 0})
            continue
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
    if dout_mean is not None:
        dout += (dout_mean * rng.choice([-1.0, 1.0], Cout) * (1 + 0.1 * rng.standard_normal(Cout))).astype(np.float32)
    return {"sources": sources, "w": w, "bias": bias, "gamma": gamma, "beta": beta, "dout": dout, "kw": kw}


# ---- the condition cases of tests/test_gpu_conv_layer.py, here so that tests/test_conv_layer_host.py checks the reference
# alone on the same inputs: (B, S, [(C, 0), (C * ncond, 0, ncond)], Cout)
def _cond(B, S, C, ncond, Cout):
    return (B, S, ((C, 0), (C * ncond, 0, ncond)), Cout)


COND_FOLD_CASES = (_cond(2, 4, 1, 10, 16), _cond(3, 8, 1, 10, 16), _cond(5, 8, 1, 3, 32), _cond(2, 16, 1, 10, 16),
                   _cond(2, 8, 1, 1, 16), _cond(2, 8, 1, 7, 32))
COND_BCAST_CASES = (_cond(2, 8, 4, 10, 16), _cond(3, 4, 4, 3, 16), _cond(2, 8, 4, 1, 12))
