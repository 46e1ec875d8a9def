"""Reference of a producer layer P and its consumer(s) as the engines link them (ics_op_conv_link), in fp64 numpy from
conv_layer_ref.layer_forward / layer_backward and numpy_ref.maxpool_bwd / upsample_bwd.

    same       P -> L                     dO_P = dV_L
    up         P -> up -> L               dO_P = upsample_bwd(dV_L)
    pool       P -> MaxPool -> K          dO_P = maxpool_bwd(o_P, dV_K)
    pool_skip  P -> MaxPool -> K,  L = [P | up(q)]        dO_P = maxpool_bwd(o_P, dV_K) + dV_L[..., :Cp]

o_P = post_act(BN(P.y)) is what every consumer reads.  link_forward / link_backward evaluate the chain in any dtype: float64
is the reference, float32 -- with the fp64 reference's decisions -- gives e32, the error of the PLAIN formulas in float32
(the yardstick of test_gpu_conv_link.py: it never comes from the folded formulas under test).

Decisions (ReLU / LeakyReLU sides, pool routing) are discontinuities: link_backward takes them from `pins`, the op's stored
y per layer and its own fp32 affine (what the kernels decide from), and counts how many differ from the evaluation's own.

Also here: the algebra of the folds in plain numpy (class sums -> S_t, sum W S_t, sum W G, gamma G + beta S_t, the pool
share on the pooled grid) and a float32 emulation of the folded path, for tests/test_conv_link_host.py."""
import numpy as np

import conv_layer_ref as CR
from oracle import numpy_ref as R

LINKS = ("same", "up", "pool", "pool_skip")
FORM_KW = {"unet": {"pre_act": 1, "has_bn": True, "post_act": 0}, "vae": {"pre_act": 0, "has_bn": True, "post_act": 2}}
P_REGIMES = (None, "ratio30", "ratio1000")      # conv_layer_ref.regime_params: ordinary, every channel at mean/std 30, 1000
DOUT_REGIMES = ("normal", "mean30")


def layer_names(link):
    return {"same": ("P", "L"), "up": ("P", "L"), "pool": ("P", "K"), "pool_skip": ("P", "K", "L")}[link]


def make_link(link, form, B, S, C0, Cp, Ck=0, Cl=0, Cq=0, seed=0, p_regime=None, dout_regime="normal"):
    """The inputs of a case.  S: P's grid.  P's gamma / beta: channel 0 has gamma < 0 (the pool picks the minimum of s),
    channel 1 gamma = 0 (all eight elements of a window tie; dy = 0, dgamma is not), channel 2 |beta| = 300 |gamma| (beta S_t
    dominates the rebuilt dW); a quarter of the others are negative.  dout_regime "mean30": every column of the output
    gradients has a mean of 30x its std (total-minus-border and c1 cancel)."""
    rng = np.random.default_rng(7000 + seed)

    def layer(Cin, Cout):
        w = (rng.standard_normal((3, 3, 3, Cin, Cout)) / np.sqrt(27 * Cin)).astype(np.float32)
        return {"w": w, "bias": rng.standard_normal(Cout).astype(np.float32),
                "gamma": rng.uniform(0.5, 1.5, Cout).astype(np.float32), "beta": rng.uniform(-0.5, 0.5, Cout).astype(np.float32)}

    def grad(shape):
        g = rng.standard_normal(shape).astype(np.float32)
        if dout_regime == "mean30":
            g = g + (30.0 * rng.choice([-1.0, 1.0], shape[-1])).astype(np.float32)
        return g

    d = {"link": link, "form": form, "x0": rng.standard_normal((B, S, S, S, C0)).astype(np.float32), "layers": {}}
    P = layer(C0, Cp)
    if p_regime is not None:
        P["w"], P["bias"] = CR.regime_params(P["w"], rng, p_regime)
    P["gamma"] = (P["gamma"] * np.where(rng.uniform(size=Cp) < 0.25, -1.0, 1.0)).astype(np.float32)
    P["gamma"][0] = -abs(P["gamma"][0])
    P["gamma"][1] = 0.0
    P["gamma"][2], P["beta"][2] = 0.01, 3.0
    d["layers"]["P"] = P
    if link in ("pool", "pool_skip"):
        d["layers"]["K"] = layer(Cp, Ck)
        d["dout"] = grad((B, S // 2, S // 2, S // 2, Ck))
    if link == "pool_skip":
        d["q"] = rng.standard_normal((B, S // 2, S // 2, S // 2, Cq)).astype(np.float32)
        d["layers"]["L"] = layer(Cp + Cq, Cl)
        d["dout_l"] = grad((B, S, S, S, Cl))
    elif link in ("same", "up"):
        SL = 2 * S if link == "up" else S
        d["layers"]["L"] = layer(Cp, Cl)
        d["dout"] = grad((B, SL, SL, SL, Cl))
    return d


def _lf(sources, p, form, dtype, eps, ranks=0):
    return CR.layer_forward(sources, p["w"], p["bias"], p["gamma"], p["beta"], dtype=dtype, eps=eps, ranks=ranks, **FORM_KW[form])


def consumer_sources(d, oP, pooled):
    """the virtual-input description of K and L given P's output"""
    link = d["link"]
    src = {}
    if link in ("pool", "pool_skip"):
        src["K"] = [{"x": pooled}]
    if link == "same":
        src["L"] = [{"x": oP}]
    elif link == "up":
        src["L"] = [{"x": oP, "up": 1}]
    elif link == "pool_skip":
        src["L"] = [{"x": oP}, {"x": d["q"], "up": 1}]
    return src


def link_forward(d, dtype=np.float64, eps=CR.EPS, ranks=0):
    """{"P": f, "K": f, "L": f, "pooled": .., "src": ..} with f as conv_layer_ref.layer_forward returns it.  ranks >= 2: the
    statistics of every layer by the sharded (SyncBN) route of conv_layer_ref, the batch being `ranks` equal shards."""
    form = d["form"]
    out = {"P": _lf([{"x": d["x0"]}], d["layers"]["P"], form, dtype, eps, ranks)}
    oP = out["P"]["o"]
    pooled = R.maxpool_fwd(oP) if "K" in d["layers"] else None
    out["pooled"] = pooled
    out["src"] = consumer_sources(d, oP, pooled)
    for name in ("K", "L"):
        if name in d["layers"]:
            out[name] = _lf(out["src"][name], d["layers"][name], form, dtype, eps, ranks)
    return out


def fp32_affine(y, scale, shift):
    """the kernels' fmaf(s, scale, shift): the exact product-sum rounded once"""
    return (np.asarray(y, np.float64) * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)).astype(np.float32)


def pins_of(r, form):
    """the decision inputs of an op result (or of a float32 link_forward, see pins_of_forward): per layer the stored y and
    the fp32 BatchNorm output; for P also `route`, the fp32 pool input post_act(BN(y))"""
    pins = {}
    for name in ("P", "K", "L"):
        if name in r:
            bn = fp32_affine(r[name]["y"], r[name]["scale"], r[name]["shift"])
            pins[name] = {"y": r[name]["y"], "bn": bn}
    pins["P"]["route"] = R.act_fwd(pins["P"]["bn"], CR.ACT[FORM_KW[form]["post_act"]])
    return pins


def pins_of_forward(f, form):
    """the same from a link_forward result: its own decisions in its own dtype (float32: what a float32 evaluation of the
    plain formulas decides; float64: the reference's own)"""
    pins = {n: {"y": f[n]["y"], "bn": f[n]["bn"]} for n in ("P", "K", "L") if n in f}
    pins["P"]["route"] = f["P"]["o"]
    return pins


def _routing_mask(route, ties):
    xw = R._windows(np.asarray(route))
    if ties == "tf_cpu":
        return np.abs(xw - xw.max(axis=4)[..., None, :]) < R.POOL_TIE_TOL
    return np.arange(8).reshape(1, 1, 1, 1, 8, 1) == xw.argmax(axis=4)[..., None, :]


def _lb(f, sources, p, dout, form, pin, ranks=0, strict_dtype=False):
    kw = FORM_KW[form]
    b = CR.layer_backward(f, sources, p["w"], p["gamma"], dout, kink_y=None if pin is None else pin["y"],
                          kink_bn=None if pin is None else pin["bn"], ranks=ranks, strict_dtype=strict_dtype, **kw)
    return b


def _dy_of(f, p, dout, form, pin):
    """gradient w.r.t. the convolution's output (behind the pre-activation): layer_backward's intermediate"""
    kw = FORM_KW[form]
    dtype = f["y"].dtype.type
    d = np.asarray(dout, dtype)
    d = R.act_bwd(np.asarray(f["bn"] if pin is None else pin["bn"], dtype), d, CR.ACT[kw["post_act"]])
    d, _, _ = R.bn_train_bwd(f["s"], np.asarray(p["gamma"], dtype), f["mean"], f["var"], d, eps=f["eps"])
    return R.act_bwd(np.asarray(f["s"] if pin is None else pin["y"], dtype), d, CR.ACT[kw["pre_act"]])


def link_backward(d, f, pins=None, ties="tf_cpu", ranks=0, strict_dtype=False):
    """Gradients of the whole link in the dtype of f.  Returns {"P": b, "K": b, "L": b, "dO_P", "dy_p", "dx0",
    "pinned": {layer: count}, "rerouted": pool windows whose routing under `pins` differs from this evaluation's own}."""
    link, form, lay = d["link"], d["form"], d["layers"]
    dtype = f["P"]["y"].dtype.type
    pin = (lambda n: None) if pins is None else (lambda n: pins[n])
    out = {"pinned": {}, "rerouted": 0}
    dO = 0
    if "K" in lay:
        out["K"] = _lb(f["K"], f["src"]["K"], lay["K"], d["dout"], form, pin("K"), ranks, strict_dtype)
        oP = f["P"]["o"]
        route = None if pins is None else np.asarray(pins["P"]["route"], dtype)
        dO = R.maxpool_bwd(oP, f["pooled"], out["K"]["dx"][0], ties=ties, route=route)
        if route is not None:
            diff = _routing_mask(route, ties) != _routing_mask(oP, ties)
            out["rerouted"] = int(diff.any(axis=4).sum())
    if "L" in lay:
        out["L"] = _lb(f["L"], f["src"]["L"], lay["L"], d["dout_l"] if link == "pool_skip" else d["dout"], form, pin("L"), ranks, strict_dtype)
        dO = dO + out["L"]["dx"][0]
    out["dO_P"] = dO
    srcP = [{"x": d["x0"]}]
    out["P"] = _lb(f["P"], srcP, lay["P"], dO, form, pin("P"), ranks, strict_dtype)
    out["dy_p"] = out["P"]["dy"]
    out["dx0"] = out["P"]["dx"][0]
    for n in ("P", "K", "L"):
        if n in out:
            out["pinned"][n] = out[n]["pinned"]
    return out


GRAD_KEYS = ("dw", "dbias", "dgamma", "dbeta")


def grad_tensors(b, names):
    """name -> array, every gradient tensor the op returns"""
    t = {"dy_p": b["dy_p"], "dx0": b["dx0"]}
    for n in names:
        for k in GRAD_KEYS:
            t["%s.%s" % (n, k)] = b[n][k]
    return t


def op_grad_tensors(r, names):
    t = {"dy_p": r["dy_p"], "dx0": r["dx0"]}
    for n in names:
        for k in GRAD_KEYS:
            t["%s.%s" % (n, k)] = r[n][k]
    return t


def rel_errors(got, ref, form):
    """tensor-relative error per gradient tensor.  A bias in front of a BatchNorm without an activation in between (VAE
    form) has a gradient of exactly zero; the reference holds rounding noise there: measured on the scale of the same
    layer's kernel gradient (as tests/test_gpu_conv_layer.py does).  In the U-Net form the same holds once every voxel of a
    layer is open, which the mean/std >= 30 regimes bring about for P: decided from the reference's own y, see `linear`."""
    out = {}
    for k, v in ref.items():
        scale = np.abs(v).max()
        if k.endswith(".dbias") and (form == "vae" or ref.get("linear:" + k[0], False)):
            scale = max(scale, np.abs(ref[k[0] + ".dw"]).max())
        if k.startswith("linear:"):
            continue
        out[k] = float(np.abs(np.asarray(got[k], np.float64) - np.asarray(v, np.float64)).max() / max(scale, 1e-300))
    return out


def link_case_view(d):
    """P of a make_link dict in the shape conv_layer_ref.rank_regimes rewrites (the arrays are shared)"""
    P = d["layers"]["P"]
    return {"sources": [{"x": d["x0"]}], "w": P["w"], "bias": P["bias"]}


def shard_grads(d, f, b, R):
    """{layer: [per-rank dict dw, dbias, dgamma, dbeta]}: every rank's local parameter gradients (conv_layer_ref.shard_grads)"""
    return {n: CR.shard_grads(f[n], b[n], d["layers"][n]["w"], R) for n in layer_names(d["link"])}


def reference(d, pins=None, ties="tf_cpu"):
    """fp64 forward + backward, and the flat dict of gradient tensors (with the `linear:<layer>` flags rel_errors reads)"""
    f = link_forward(d)
    b = link_backward(d, f, pins, ties)
    names = layer_names(d["link"])
    t = grad_tensors(b, names)
    for n in names:
        t["linear:" + n] = d["form"] == "unet" and bool((f[n]["y"] > 0).all())
    return f, b, t


def e32_of(d, f64, t64, ties="tf_cpu", strict_dtype=False):
    """the PLAIN formulas in float32 numpy against the fp64 reference, with the fp64 reference's decisions
    (strict_dtype: conv_layer_ref.layer_backward)"""
    f32 = link_forward(d, np.float32)
    b32 = link_backward(d, f32, pins_of_forward(f64, d["form"]), ties, strict_dtype=strict_dtype)
    if strict_dtype:
        assert all(v.dtype == np.float32 for v in grad_tensors(b32, layer_names(d["link"])).values())
    return rel_errors(grad_tensors(b32, layer_names(d["link"])), t64, d["form"])


# ---- the folds' algebra, in plain numpy of any dtype
def tap_valid_for_class(tapd, cls):
    """tap offset tapd - 1 in {-1, 0, +1} applied to a voxel of plane class cls (0 first, 1 interior, 2 last) stays inside"""
    return not ((cls == 0 and tapd == 0) or (cls == 2 and tapd == 2))


def class_sums(dy, sum_dtype=None):
    """R[27][N]: the sum of dy over the voxels of each class {first plane, interior, last plane}^3; the 26 border classes
    directly, the interior (class 13) as total minus border -- as class_sums_kernel / conv_bnfuse_kernel do"""
    S = dy.shape[1]
    sl = (slice(0, 1), slice(1, S - 1), slice(S - 1, S))
    acc = dy.dtype if sum_dtype is None else sum_dtype
    Rc = np.zeros((27, dy.shape[-1]), np.float64)
    for cls in range(27):
        if cls != 13:
            Rc[cls] = dy[:, sl[cls // 9], sl[(cls // 3) % 3], sl[cls % 3]].sum(axis=(0, 1, 2, 3), dtype=acc)
    total = dy.sum(axis=(0, 1, 2, 3), dtype=acc).astype(np.float64)
    Rc[13] = total - (Rc.sum(0) - Rc[13])
    return Rc


def tap_sums(Rc):
    """S_t[27][N]: the sum of dy over the voxels v with v + t inside the grid"""
    St = np.zeros_like(Rc)
    for t in range(27):
        for cls in range(27):
            if (tap_valid_for_class(t // 9, cls // 9) and tap_valid_for_class((t // 3) % 3, (cls // 3) % 3)
                    and tap_valid_for_class(t % 3, cls % 3)):
                St[t] += Rc[cls]
    return St


def tap_sums_direct(dy):
    """the same by definition: for each tap, the sum over the voxels whose shifted position is inside"""
    S = dy.shape[1]
    rng = (slice(1, S), slice(0, S), slice(0, S - 1))      # tap offset -1: v >= 1; 0: all; +1: v <= S - 2
    return np.stack([dy[:, rng[t // 9], rng[(t // 3) % 3], rng[t % 3]].sum(axis=(0, 1, 2, 3)) for t in range(27)])


def fold_same(fP, pP, wL, dyL, dtype=np.float64):
    """The linear fold of a same-resolution 3x3x3 consumer L (U-Net form of P): from L's dy, its weights and P's xhat
        G = wgrad(xhat, dy),  S_t,  dW_L = gamma G + beta S_t,  sum d = sum W S_t,  sum d xhat = sum W G
    and the apply dy_P = relu'(s) fma(a, d, fma(b, s, c)).  dtype float32: G, the class partials (64-row blocks summed in
    fp64, as the kernels) and the apply in float32, the per-channel constants through fp64, as conv_bnfuse_kernel."""
    s = np.asarray(fP["s"], dtype)
    mean, rstd = np.asarray(fP["mean"], dtype), np.asarray(fP["rstd"], dtype)
    gamma, beta = np.asarray(pP["gamma"], dtype), np.asarray(pP["beta"], dtype)
    xs0, xs1 = rstd, (-mean.astype(np.float64) * rstd.astype(np.float64)).astype(dtype)
    xhat = s * xs0 + xs1
    dy = np.asarray(dyL, dtype)
    w = np.asarray(wL, dtype)
    d, G, _ = R.conv3d_bwd(xhat, w, dy)
    if dtype == np.float32:
        Rc = class_sums32(dy)
    else:
        Rc = class_sums(dy)
    St = tap_sums(Rc).reshape(3, 3, 3, 1, -1)
    G64, w64 = G.astype(np.float64), w.astype(np.float64)
    g64, b64 = gamma.astype(np.float64)[:, None], beta.astype(np.float64)[:, None]
    dW = (g64 * G64 + b64 * St).astype(dtype)
    sd = (w64 * St).sum(axis=(0, 1, 2, 4))
    sq = (w64 * G64).sum(axis=(0, 1, 2, 4))
    n = float(s.size // s.shape[-1])
    sc = (gamma * rstd).astype(dtype).astype(np.float64)
    k1, k2, rs, mu = sd / n, sq / n, rstd.astype(np.float64), mean.astype(np.float64)
    a, b, c = sc.astype(dtype), (-sc * k2 * rs).astype(dtype), (sc * (k2 * rs * mu - k1)).astype(dtype)
    dyP = (s > 0) * (a * d + (b * s + c))
    return {"dW_L": dW, "sum_d": sd, "sum_dxhat": sq, "dy_p": dyP, "d": d, "G": G, "St": St}


def class_sums32(dy):
    """class sums with float32 partials over 64-row blocks, merged in fp64 (class_sums_kernel + class_reduce_kernel); the
    total from float32 partials over 128-row blocks (the bias-gradient partials of L's BatchNorm-backward apply)"""
    S = dy.shape[1]
    sl = (slice(0, 1), slice(1, S - 1), slice(S - 1, S))

    def blocks(rows, n):
        tot = np.zeros(rows.shape[-1], np.float64)
        for r0 in range(0, rows.shape[0], n):
            tot += CR._tree_sum32(rows[r0:r0 + n]).astype(np.float64)
        return tot

    N = dy.shape[-1]
    Rc = np.zeros((27, N), np.float64)
    for cls in range(27):
        if cls != 13:
            Rc[cls] = blocks(dy[:, sl[cls // 9], sl[(cls // 3) % 3], sl[cls % 3]].reshape(-1, N), 64)
    Rc[13] = blocks(dy.reshape(-1, N), 128) - (Rc.sum(0) - Rc[13])
    return Rc


def pool_share(fP, g, mask, dtype=np.float64):
    """The MaxPool consumer's share of P's two sums on the pooled grid: sum k g and sum g (ssum - k mean) rstd, with k the
    number of routed elements of a window and ssum the sum of their stored activations (pool_sums_kernel).  mask: bool
    (B, S/2, S/2, S/2, 8, C).  dtype float32: the per-window terms in float32, the sums in fp64."""
    sw = R._windows(np.asarray(fP["s"], dtype))
    k = mask.sum(axis=4).astype(dtype)
    ssum = (sw * mask).sum(axis=4, dtype=dtype)
    mean, rstd = np.asarray(fP["mean"], dtype), np.asarray(fP["rstd"], dtype)
    g = np.asarray(g, dtype)
    xs = (ssum - k * mean) * rstd
    return (g * k).astype(np.float64).sum(axis=(0, 1, 2, 3)), (g * xs).astype(np.float64).sum(axis=(0, 1, 2, 3))
