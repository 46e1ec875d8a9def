"""Reference of the U-Net's last link as the engine runs it (ics_op_head_link): a producer P in c18's place -- Conv 3x3x3
C0 -> 128, ReLU, BatchNorm, conv_layer_ref.layer_forward / layer_backward -- the 1x1x1 head 128 -> ncls + 1 and its losses,
in fp64 numpy.

    o = gamma xhat + beta            z = o [wsoft | wsig] + [bsoft | bsig]          soft = softmax(z[:ncls]), sig = sigmoid(z[ncls])
    Loss = mean_v wcce(soft, label; weight) + mean_v bce(sig, label != 0)           (numpy_ref.wcce_loss / bce_loss / bce_logits_loss)
    dz = dLoss / dz,  head dW = o^T dz,  head dbias = sum_v dz,  d = dz [wsoft | wsig]^T,  then P's BatchNorm and ReLU backward

head_forward / head_backward evaluate the head in any dtype (numpy_ref's own functions build float64 one-hot arrays and so
continue in float64 whatever they are given): float64 is the reference -- tests/test_head_link_host.py shows it equal to
UnetOracle's own c18 block, head and loss at 1e-12 -- and float32, with the fp64 reference's decisions, gives e32, the error
of the PLAIN formulas in float32 (the yardstick of test_gpu_head_link.py; it never comes from the fused formulas under test).

Decisions are discontinuities: the ReLU side of P's y, K.clip's zero-gradient region of the true class's probability and of
the sigmoid, and the 0.5 threshold of f1 / wr.  `pins` = {"y": the op's stored y, "soft_inside", "sig_inside": bool per
voxel} replaces the evaluation's own; the counts of those that differ come back as "pinned".

Emulated ranks (ranks = R): the batch is R equal shards; P's statistics are those of the whole batch (layer_forward's sharded
route), every rank's loss is the mean over its OWN voxels, and the parameter gradients are each rank's local sums.

Also here: the algebra of the head's BatchNorm-backward fusion (head_bnfuse_kernel, head_dgrad_kernel<true>) in plain numpy of
either dtype, for the host test."""
import numpy as np

import conv_layer_ref as CR
from oracle import numpy_ref as R

KW = {"pre_act": 1, "has_bn": True, "post_act": 0}
KEPS = R.K_EPSILON
# K.clip's bounds as float32 arithmetic holds them -- the kernels' kKEps and 1.f - kKEps, and Keras' own float32 graph:
# 1 - 1e-7 is not a float32, the nearest one is 1 - 2^-23 = 0.99999988, so a saturated sigmoid costs -log(1.19e-7) = 15.94,
# not 16.12 (the ordinary cases never reach a bound: there this reference equals numpy_ref's fp64 clip exactly)
CLIP_LO = float(np.float32(KEPS))
CLIP_HI = float(np.float32(1) - np.float32(KEPS))
P_REGIMES = (None, "ratio30", "ratio1000", "dead")
HEAD_REGIMES = ("ordinary", "sharp")
LABEL_REGIMES = ("mixed", "background", "missing", "one_class")
DEAD_CH = 5
SHARP_SOFT, SHARP_SIG = 6.0, 40.0     # the sharp head's weight scales: about half of the voxels have their true class below
                                      # the clip's 1e-7 and two thirds a saturated sigmoid (test_head_link_host.py prints both)
MISSING = 7


def make_head_link(B, S, C0, ncls=95, seed=0, p_regime=None, head_regime="ordinary", label_regime="mixed", loss_weight=0.0,
                   class_weights=False, bce_from_logits=False, ranks=0, rank_regime=None):
    """The inputs of a case; B per rank.  P's gamma / beta as conv_link_ref.make_link: channel 0 gamma < 0, channel 1 gamma = 0,
    channel 2 gamma = 0.01 with beta = 3, a quarter of the rest negative.  p_regime "ratio30" / "ratio1000": every channel at
    that mean/std (conv_layer_ref.regime_params); "dead": channel DEAD_CH all zeros behind the ReLU (var = 0, xhat = 0).
    head_regime "sharp": the head's weights times SHARP_SOFT / SHARP_SIG.  class_weights: a table with zeros and one weight of 1e3."""
    rng = np.random.default_rng(9000 + seed)
    NB = B * max(ranks, 1)
    x0 = rng.standard_normal((NB, S, S, S, C0)).astype(np.float32)
    w = (rng.standard_normal((3, 3, 3, C0, 128)) / np.sqrt(27 * C0)).astype(np.float32)
    P = {"w": w, "bias": rng.standard_normal(128).astype(np.float32),
         "gamma": rng.uniform(0.5, 1.5, 128).astype(np.float32), "beta": rng.uniform(-0.5, 0.5, 128).astype(np.float32)}
    if p_regime in ("ratio30", "ratio1000"):
        P["w"], P["bias"] = CR.regime_params(P["w"], rng, p_regime)
    elif p_regime == "dead":
        P["w"][..., DEAD_CH] = 0
        P["bias"][DEAD_CH] = -1.0
    else:
        assert p_regime is None
    P["gamma"] = (P["gamma"] * np.where(rng.uniform(size=128) < 0.25, -1.0, 1.0)).astype(np.float32)
    P["gamma"][0] = -abs(P["gamma"][0])
    P["gamma"][1] = 0.0
    P["gamma"][2], P["beta"][2] = 0.01, 3.0
    k, kg = (SHARP_SOFT, SHARP_SIG) if head_regime == "sharp" else (1.0, 1.0)
    head = {"wsoft": (k * rng.standard_normal((128, ncls)) / np.sqrt(128)).astype(np.float32),
            "bsoft": (0.1 * rng.standard_normal(ncls)).astype(np.float32),
            "wsig": (kg * rng.standard_normal(128) / np.sqrt(128)).astype(np.float32),
            "bsig": (0.1 * rng.standard_normal(1)).astype(np.float32)}
    lab = rng.integers(1, ncls, size=(NB, S, S, S))
    if label_regime == "mixed":
        lab = np.where(rng.uniform(size=lab.shape) < 0.5, 0, lab)
    elif label_regime == "background":
        lab[:] = 0
    elif label_regime == "missing":
        lab = np.where(lab == MISSING % ncls, (MISSING + 1) % ncls, lab)
    elif label_regime == "one_class":
        lab[:] = 3 % ncls
    else:
        raise ValueError(label_regime)
    d = {"B": B, "S": S, "C0": C0, "ncls": ncls, "ranks": ranks, "x0": x0, "P": P, "head": head, "labels": lab.astype(np.uint8),
         "loss_weight": float(loss_weight), "class_weights": None, "bce_from_logits": bool(bce_from_logits)}
    if class_weights:
        cw = rng.uniform(0.5, 2.0, ncls).astype(np.float32)
        cw[[1, ncls // 2]] = 0.0
        cw[ncls // 3] = 1e3
        d["class_weights"] = cw
    if rank_regime is not None:
        CR.rank_regimes({"sources": [{"x": x0}], "w": P["w"], "bias": P["bias"]}, ranks, rank_regime)
    return d


def loss_weights(d, dtype=np.float64):
    """per-voxel weight of the softmax loss: the table's entry of the voxel's label, or the scalar (<= 0: ncls)"""
    lab = d["labels"].reshape(-1)
    if d["class_weights"] is not None:
        return np.asarray(d["class_weights"], dtype)[lab]
    lw = d["loss_weight"] if d["loss_weight"] > 0 else float(d["ncls"])
    return np.full(lab.shape, lw, dtype)


def head_forward(d, o, dtype=np.float64):
    """softmax / sigmoid of the head on o (rows, 128) and the per-voxel losses, in dtype"""
    h, ncls = d["head"], d["ncls"]
    o = np.asarray(o, dtype).reshape(-1, 128)
    zs = o @ np.asarray(h["wsoft"], dtype) + np.asarray(h["bsoft"], dtype)
    zg = o @ np.asarray(h["wsig"], dtype).reshape(128) + np.asarray(h["bsig"], dtype).reshape(())
    e = np.exp(zs - zs.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    with np.errstate(over="ignore"):               # exp(-z) = inf at a saturated logit: the sigmoid is then exactly 0
        ps = dtype(1) / (dtype(1) + np.exp(-zg))
    lab = d["labels"].reshape(-1).astype(np.int64)
    rows = np.arange(lab.size)
    S = p.sum(-1)
    pt = p[rows, lab]
    qt = pt / S
    lo, hi = dtype(CLIP_LO), dtype(CLIP_HI)
    wv = loss_weights(d, dtype)
    t = (lab != 0).astype(dtype)
    f = {"zs": zs, "zg": zg, "p": p, "ps": ps, "S": S, "pt": pt, "qt": qt, "wv": wv, "t": t, "lab": lab,
         "soft_inside": (qt >= lo) & (qt <= hi), "sig_inside": (ps >= lo) & (ps <= hi)}
    f["lsoft"] = -wv * np.log(np.clip(qt, lo, hi))
    if d["bce_from_logits"]:
        f["lsig"] = np.maximum(zg, 0) - zg * t + np.log1p(np.exp(-np.abs(zg)))
    else:
        pc = np.clip(ps, lo, hi)
        f["lsig"] = -(t * np.log(pc) + (dtype(1) - t) * np.log(dtype(1) - pc))
    return f


def head_metrics(d, f, ranks=0):
    """(metrics (R, 5) = [Loss, lsoft, lsig, f1, wr], sums (R, 7) in engine.METRIC_SUM_KEYS order, near (R,)): every rank's
    LOCAL ones, as numpy_ref.f1_m / wr_m form them from the counts.  near: probabilities within 2e-5 of the 0.5 threshold
    (tests/saturated.metric_counts' margin) -- each may round either way in float32."""
    Rr = max(ranks, 1)
    n = f["lab"].size // Rr
    met, sums, near = np.zeros((Rr, 5)), np.zeros((Rr, 7)), np.zeros(Rr, int)
    for r in range(Rr):
        sl = slice(r * n, (r + 1) * n)
        p, pt, lab = np.asarray(f["p"][sl], np.float64), np.asarray(f["pt"][sl], np.float64), f["lab"][sl]
        hit = pt > 0.5
        tp, pred, wtp, wpos = hit.sum(), (p > 0.5).sum(), (hit & (lab != 0)).sum(), (lab != 0).sum()
        ls, lg = float(np.asarray(f["lsoft"][sl], np.float64).sum()), float(np.asarray(f["lsig"][sl], np.float64).sum())
        sums[r] = [ls, lg, tp, pred, wtp, wpos, n]
        met[r] = metrics_from_sums(sums[r])
        near[r] = int((np.abs(p - 0.5) <= 2e-5).sum())
    return met, sums, near


def metrics_from_sums(s):
    ls, lg, tp, pred, wtp, wpos, n = [float(v) for v in s]
    prec, rec = tp / (pred + KEPS), tp / (n + KEPS)
    return np.array([(ls + lg) / n, ls / n, lg / n, 2 * prec * rec / (prec + rec + KEPS), wtp / (wpos + KEPS)])


def head_backward(d, f, o, pins=None, ranks=0):
    """dz (rows, ncls + 1), the head's parameter gradients per rank, d = dLoss/do, in the dtype of f; `pinned`: clip
    decisions of `pins` that differ from this evaluation's own."""
    dtype = f["p"].dtype.type
    h, ncls = d["head"], d["ncls"]
    Rr = max(ranks, 1)
    n = f["lab"].size // Rr
    inv = dtype(1.0 / n)
    lo, hi = dtype(CLIP_LO), dtype(CLIP_HI)
    si = f["soft_inside"] if pins is None else np.asarray(pins["soft_inside"], bool).reshape(-1)
    gi = f["sig_inside"] if pins is None else np.asarray(pins["sig_inside"], bool).reshape(-1)
    pinned = int((si != f["soft_inside"]).sum()) + (0 if d["bce_from_logits"] else int((gi != f["sig_inside"]).sum()))
    p, S = f["p"], f["S"]
    rows = np.arange(f["lab"].size)
    # numpy_ref.wcce_bwd: q = p / S, dq_t = -w / clip(q_t) inside, dp_j = dq_j / S - sum_i dq_i p_i / S^2; softmax_bwd
    # a voxel decided "inside" takes the inside branch's derivative, -w / q_t itself: where `pins` overrules this evaluation
    # (q_t within rounding of a bound) the clipped value is not q_t, and -w / clip(q_t) would be neither branch
    dqt = -f["wv"] / np.where(si, f["qt"], np.clip(f["qt"], lo, hi)) * si.astype(dtype) * inv
    dp = -(dqt * f["pt"] / (S * S))[:, None] * np.ones_like(p)
    dp[rows, f["lab"]] += dqt / S
    dzs = p * (dp - (dp * p).sum(-1, keepdims=True))
    ps, t = f["ps"], f["t"]
    if d["bce_from_logits"]:
        dzg = (ps - t) * inv
    else:
        pc = np.where(gi, ps, np.clip(ps, lo, hi))          # as above: the inside branch reads the probability itself
        with np.errstate(divide="ignore", invalid="ignore"):
            dl = np.where(gi, -(t / pc) + (dtype(1) - t) / (dtype(1) - pc), dtype(0))
        dzg = dl * inv * ps * (dtype(1) - ps)
    dz = np.concatenate([dzs, dzg[:, None]], -1).astype(dtype)
    o = np.asarray(o, dtype).reshape(-1, 128)
    W = np.concatenate([np.asarray(h["wsoft"], dtype), np.asarray(h["wsig"], dtype).reshape(128, 1)], -1)
    dW = np.stack([o[r * n:(r + 1) * n].T @ dz[r * n:(r + 1) * n] for r in range(Rr)])
    db = np.stack([dz[r * n:(r + 1) * n].sum(0) for r in range(Rr)])
    return {"dz": dz, "dwsoft": dW[..., :ncls], "dwsig": dW[..., ncls], "dbias_head": db, "d": dz @ W.T, "pinned": pinned}


def forward(d, dtype=np.float64, eps=CR.EPS):
    P = d["P"]
    fP = CR.layer_forward([{"x": d["x0"]}], P["w"], P["bias"], P["gamma"], P["beta"], dtype=dtype, eps=eps, ranks=d["ranks"], **KW)
    return fP, head_forward(d, fP["o"], dtype)


def backward(d, fP, fh, pins=None, strict_dtype=False):
    """every gradient tensor the op returns, flat, with leading (R,) under ranks as the op has them"""
    P, Rr = d["P"], d["ranks"]
    hb = head_backward(d, fh, fP["o"], pins, Rr)
    dout = hb["d"].reshape(fP["o"].shape)
    b = CR.layer_backward(fP, [{"x": d["x0"]}], P["w"], P["gamma"], dout, kink_y=None if pins is None else pins["y"], ranks=Rr,
                          strict_dtype=strict_dtype, **KW)
    t = {"dz": hb["dz"].reshape(d["labels"].shape + (d["ncls"] + 1,)), "dy_p": b["dy"], "dx0": b["dx"][0]}
    if Rr:
        sg = CR.shard_grads(fP, b, P["w"], Rr)
        for k in ("dw", "dbias", "dgamma", "dbeta"):
            t[k] = np.stack([g[k] for g in sg])
        for k in ("dwsoft", "dwsig", "dbias_head"):
            t[k] = hb[k]
    else:
        for k in ("dw", "dbias", "dgamma", "dbeta"):
            t[k] = b[k]
        for k in ("dwsoft", "dwsig", "dbias_head"):
            t[k] = hb[k][0]
    return t, {"relu": b["pinned"], "clip": hb["pinned"]}


GRAD_KEYS = ("dz", "dwsoft", "dwsig", "dbias_head", "dw", "dbias", "dgamma", "dbeta", "dy_p", "dx0")


def own_pins(fP, fh):
    return {"y": fP["y"], "soft_inside": fh["soft_inside"], "sig_inside": fh["sig_inside"]}


def _lead(v, y):
    """per-rank (R, 128) statistics broadcast over the rank-major batch of y"""
    v = np.asarray(v, np.float64)
    if v.ndim == 1:
        return v
    return np.repeat(v, y.shape[0] // v.shape[0], axis=0)[:, None, None, None, :]


def affine_of(d, r):
    """the op's own float32 BatchNorm output fmaf(y, scale, shift): what the head kernels read (rounded once)"""
    y = np.asarray(r["y"], np.float64)
    return (y * _lead(r["scale"], y) + _lead(r["shift"], y)).astype(np.float32)


def reference(d, pins=None, eps=CR.EPS):
    """(fP, fh, tensors, pinned): fp64 forward and backward, every gradient tensor the op returns, and the metrics"""
    fP, fh = forward(d, np.float64, eps)
    t, pinned = backward(d, fP, fh, pins)
    return fP, fh, t, pinned


def e32_of(d, fP64, fh64, t64):
    """the PLAIN formulas in float32 numpy against the fp64 reference, with the fp64 reference's decisions, per tensor"""
    fP32, fh32 = forward(d, np.float32)
    t32, _ = backward(d, fP32, fh32, own_pins(fP64, fh64), strict_dtype=True)
    # (under ranks conv_layer_ref's merged moments are float64 whatever they are given, and P's dgamma continues in float64
    # behind them: a smaller e32, i.e. a stricter bound)
    assert d["ranks"] or all(np.asarray(v).dtype == np.float32 for v in t32.values()), {k: np.asarray(v).dtype for k, v in t32.items()}
    return rel_errors(t32, t64, fP64)


def rel_errors(got, ref, fP64):
    """tensor-relative error per gradient tensor.  P's bias sits in front of a ReLU and a batch-statistics BatchNorm: once
    every voxel of a channel is open its gradient is exactly zero and the reference holds rounding noise there (the mean/std
    >= 30 regimes): dbias is then measured on the scale of the kernel gradient, as conv_link_ref.rel_errors does."""
    linear = bool((fP64["y"] > 0).all())
    out = {}
    for k in GRAD_KEYS:
        scale = np.abs(ref[k]).max()
        if k == "dbias" and linear:
            scale = max(scale, np.abs(ref["dw"]).max())
        out[k] = float(np.abs(np.asarray(got[k], np.float64) - np.asarray(ref[k], np.float64)).max() / max(scale, 1e-300))
    return out


# ---- the fusion's algebra (head_bnfuse_kernel + head_dgrad_kernel<true>), plain numpy of either dtype
def fused_route(d, fP, fh, dz, dtype=np.float64):
    """From dz alone, single process: Q = xhat^T dz, zs = sum_v dz, head dW = gamma Q + beta zs, sum_v d = W . zs,
    sum_v d xhat = sum_cls W Q, and dy = relu'(s) scale (d - c1 - xhat c2).  dtype float32: the GEMMs, xhat and the apply in
    float32, the per-channel class sums through fp64 as head_bnfuse_kernel; xhat from the float32 affine (rstd, -mean rstd)."""
    P, h, ncls = d["P"], d["head"], d["ncls"]
    s = np.asarray(fP["s"], dtype).reshape(-1, 128)
    mean, rstd = np.asarray(fP["mean"], dtype), np.asarray(fP["rstd"], dtype)
    gamma, beta = np.asarray(P["gamma"], dtype), np.asarray(P["beta"], dtype)
    xs1 = (-mean.astype(np.float64) * rstd.astype(np.float64)).astype(dtype)
    # the weight-gradient GEMM reads xhat as an affine of s (rstd, -mean rstd): a rounding matter, so in float32 only -- the
    # fp64 evaluation is the algebra itself
    xhat_w = s * rstd + xs1 if dtype == np.float32 else (s - mean) * rstd
    dz = np.asarray(dz, dtype).reshape(-1, ncls + 1)
    W = np.concatenate([np.asarray(h["wsoft"], dtype), np.asarray(h["wsig"], dtype).reshape(128, 1)], -1)
    Q = xhat_w.T @ dz
    zs = dz.sum(0, dtype=dtype)
    dW = (gamma[:, None] * Q + beta[:, None] * zs[None, :]).astype(dtype)
    W64 = W.astype(np.float64)
    sd = (W64 * zs.astype(np.float64)[None, :]).sum(1)
    sq = (W64 * Q.astype(np.float64)).sum(1)
    n = float(s.shape[0])
    c1, c2 = (sd / n).astype(dtype), (sq / n).astype(dtype)
    dd = dz @ W.T
    xhat = (s - mean) * rstd                        # the apply's own xhat
    scale = (gamma * rstd).astype(dtype)
    dy = np.where(s > 0, scale * (dd - c1 - xhat * c2), dtype(0)).astype(dtype)
    return {"dwsoft": dW[:, :ncls], "dwsig": dW[:, ncls], "dgamma": sq.astype(dtype), "dbeta": sd.astype(dtype),
            "dy_p": dy.reshape(fP["s"].shape), "Q": Q, "zs": zs}


# ---- the cases of tests/test_gpu_head_link.py, here so that tests/test_head_link_host.py checks the reference alone on the
# same inputs.  name -> (B, S, C0, ncls, max_batch)
SHAPES = {
    "one_tile": (2, 2, 16, 95, None),        # 16 rows: one tile, three of four waves idle
    "ragged": (6, 2, 16, 95, None),          # 48 rows: 3 tiles, a ragged block
    "blocks1": (1, 4, 16, 95, None),         # 64 rows: one whole block
    "blocks3": (3, 4, 16, 95, None),         # 192 rows
    "blocks5": (5, 4, 8, 95, None),          # 320 rows
    "big_handle": (2, 8, 16, 95, 5),         # 1024 rows on a handle sized for 5 grids
    "waves": (9, 16, 8, 95, None),           # 36 864 rows: 2304 tiles over 2048 waves, 256 waves take a second tile
    "rows8": (1, 2, 16, 95, None),           # 8 rows: both fused kernels refuse
    "ncls31": (2, 4, 16, 31, None),          # ncls + 1 = 32: the generic route with vector loads of dz
    "ncls20": (2, 4, 16, 20, None),          # 21 columns
    "ncls127": (2, 4, 16, 127, None),        # 128 columns: the column-buffer limit
}
REGIMES = {
    "ordinary": {},
    "ratio30": {"p_regime": "ratio30"},
    "ratio1000": {"p_regime": "ratio1000"},
    "dead": {"p_regime": "dead"},
    "sharp": {"head_regime": "sharp"},
    "sharp_logits": {"head_regime": "sharp", "bce_from_logits": True},
    "logits": {"bce_from_logits": True},
    "lw7.5": {"loss_weight": 7.5},
    "cw": {"class_weights": True},
    "cw_sharp_dead": {"class_weights": True, "head_regime": "sharp", "p_regime": "dead"},
    "background": {"label_regime": "background"},
    "missing": {"label_regime": "missing"},
    "one_class": {"label_regime": "one_class"},
    "one_class_ratio1000_cw": {"label_regime": "one_class", "p_regime": "ratio1000", "class_weights": True},
}
REGIME_SHAPES = ("blocks3", "big_handle")
RANK_SHAPES = {"r_s4": (2, 4, 16), "r_s8": (1, 8, 16)}       # per rank
RANK_REGIME = "rank_shift50"


def case_data(shape, regime="ordinary"):
    B, S, C0, ncls, _ = SHAPES[shape]
    return make_head_link(B, S, C0, ncls, seed=list(SHAPES).index(shape), **REGIMES[regime])


def rank_case_data(shape, ranks, rank_regime=None):
    B, S, C0 = RANK_SHAPES[shape]
    return make_head_link(B, S, C0, 95, seed=50 + list(RANK_SHAPES).index(shape), ranks=ranks, rank_regime=rank_regime)


def all_cases():
    """(id, data factory) of every input the GPU file runs"""
    out = [("%s" % s, (lambda s=s: case_data(s))) for s in SHAPES]
    out += [("%s/%s" % (s, g), (lambda s=s, g=g: case_data(s, g))) for s in REGIME_SHAPES for g in REGIMES if g != "ordinary"]
    out += [("%s/R%d" % (s, r), (lambda s=s, r=r: rank_case_data(s, r))) for s in RANK_SHAPES for r in (1, 2, 3, 4)]
    out += [("%s/R%d/%s" % (s, r, RANK_REGIME), (lambda s=s, r=r: rank_case_data(s, r, RANK_REGIME))) for s in RANK_SHAPES for r in (2, 4)]
    return out
