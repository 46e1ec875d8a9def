"""The U-Net's last link, c18 -> head, op by op (ics_op_head_link) against the fp64 reference of tests/head_link_ref.py:
head_fused_kernel (the GEMM on the producer's BatchNorm output, the affine applied in registers; the logits never reach
memory), the head's weight-gradient GEMM on xhat, head_bnfuse_kernel (dW = gamma Q + beta sum(dz); c1, c2, dgamma, dbeta of the producer from W . sum(dz) and W . Q),
head_dgrad_kernel<true> (writes the producer's dy and its bias-gradient partials), head_dgrad_kernel<false> with the folded
BwdStat sums, the generic GEMM + head_kernel + implicit-GEMM route, and under emulated ranks xhat_affine_kernel, the 256-double
exchange and bn_bwd_sync_c_kernel.  Every case asserts its profiler rows, so a dispatch change cannot turn it into a test of
another kernel.

Expected rows (expected_sites), from the predicates of engine.hip / elementwise.hip, with rows = B S^3:
  head_fused_ok      ncls == 95, rows % 16 == 0, not ICSG3D_NO_FUSED_HEAD: "head_fused"; else "conv_fwd:head|" + "head_softmax_loss"
  head_dgrad_ok      the same condition: "conv_dgrad:head|head_dgrad_kernel..."; else "conv_dgrad:head|conv_fwd_kernel<"
  bnfuse             head_dgrad_ok and not ICSG3D_NO_HEAD_BNFUSE: "...head_dgrad_kernel<true>", no "bn_act_bwd:P", and under ranks
                     "xhat_affine:head" + "head_bnfuse_exchange"; else "bn_act_bwd:P" (and "...head_dgrad_kernel" is the <false> one)
Where a predicate decides otherwise than the planned table:
  * ICSG3D_NO_FAST_BNBWD cannot reach a fused-route case (the route has no BatchNorm-backward pass at all): those cases assert that
    nothing changed, rows and bits.  ICSG3D_NO_BWD_FOLD changes no row (the fold is an argument of the same launch): the case
    asserts bits against the default route only.
  * (1, 2, 16), 8 rows: neither ICSG3D_NO_HEAD_BNFUSE nor ICSG3D_NO_FUSED_HEAD can reach it (asserted: nothing changed); whether
    the implicit-GEMM launch folds the sums at 8 rows, and whether the generic BatchNorm-backward kernels differ in bits there,
    is not asserted.
  * The profiler had no row for xhat_affine_kernel and the exchange: unet_head_backward now brackets them, under SyncBN only
    ("xhat_affine:head", "head_bnfuse_exchange"), so the rows of a single-process step are unchanged.

Cases: head_link_ref.SHAPES (rows 16, 48, 64, 192, 320, 1024 on a 5-grid handle, 36 864, 8; ncls 31, 20, 127), each ncls = 95 case
on the five routes ROUTES (36 864 rows: the first two); head_link_ref.REGIMES on (3, 4, 16) and (2, 8, 16), first two routes;
ranks 1 .. 4 on (2, 4, 16) and (1, 8, 16) per rank, plus conv_layer_ref's rank_shift50 at 2 and 4 ranks.

Bounds (none taken from what the kernels give):
  y            tensor-relative 1e-5 against the fp64 convolution
  statistics   mean 4 float32 ulps of max(|mean|, std), var + eps conv_layer_ref.var_bound, scale / shift 1 ulp (test_gpu_conv_link.py)
  metrics      against the fp64 reference evaluated on the op's OWN stored y and float32 affine, with the tolerances
               tests/test_gpu_metrics.py holds ics_op_unet_head to: Loss, lsoft, lsig rtol 1e-5 (the clipped sigmoid loss at
               saturation: 2e-5 of the float32 formula and 5e-3 of fp64, as that file's lines 196-202); the counts equal as integers up to
               the number of probabilities within 2e-5 of 0.5 (<= 8, 0 in every case here: test_head_link_host.py); f1, wr rtol 1e-5
               against numpy_ref's formulas on the op's own counts.  One voxel across the threshold moves f1 by <= 3 / rows, wr by
               <= 1 / (rows with a label != 0).
  gradients    dz, dwsoft, dwsig, head dbias, P's dw / dbias / dgamma / dbeta, dy_p, dx0: tensor-relative max(1e-5, 2 e32), e32 = the
               PLAIN formulas in float32 numpy against the same fp64 reference with the reference's decisions, per case and regime
  decisions    <= 8 pinned ReLU sides (the op's stored y), <= 8 pinned clip sides (read off the op's dz: a clipped voxel's row is zero)

Measured on the MI355X, worst over the 114 tests (engine | bound there; printed by test_zz_report_worst_gaps):
  y 1.8e-6 | 1e-5    mean 1.53 ulps | 4    var + eps 0.157 of its bound    Loss, lsoft, lsig <= 1.3e-7 | 1e-5
  lsig under the sharp head in the clipped form 9.6e-5 | 5e-3 of fp64 and LSIG32 | 2e-5 of the float32 formula (see _check_metrics)
  dz 8.2e-6 | 2.6e-5 (sharp)    dwsoft 2.9e-6 | 1e-5    dwsig 4.0e-6 | 1.6e-5    head dbias 5.4e-6 | 6.6e-5 (mean/std 1000)
  P: dw 2.9e-6, dbias 3.2e-6, dgamma 2.0e-6, dbeta 2.2e-6, dy_p 3.6e-6, dx0 3.2e-6, each | 1e-5.  Pinned: 0 ReLU, <= 6 clip sides.
Found: head_fused_kernel's affine folded into the weights biased the loss by 1.2e-5 .. 1.5e-5 at mean/std 1000 (1.5e-4 with one
class and a 1e3 weight); the affine is now applied in registers (5e-6).  Nothing in the backward kernels.
Mutations, each in a scratch copy, the whole file against the mutated library:
  1 head_bnfuse dw = g * q: 51 fail (every fused-route case, by dwsoft / dwsig), 63 pass (the other routes)
  2 c1c2[128 + ch] from sd: 39 fail (single-process fused route: dy_p, dx0, P.dw), 75 pass (ranks, other routes)
  3 head_dgrad<true> sv >= 0: 45 fail (fused route with a closed ReLU side, the dead channel), 69 pass (mean/std 30, 1000; other routes)
  4 second tile reuses the first tile's dz: 2 fail (36 864 rows, both routes), 112 pass
  5 xhat_affine +mean * rstd: 12 fail (exactly the ranks cases), 102 pass
  6 head_fused (x + shift) * scale: 90 fail (every case on the fused head), 24 pass (NO_FUSED_HEAD, 8 rows, ncls 31 / 20 / 127)
A train step launches what it launched: the 73 profiler rows of one U-Net train step at d = 16 (labels and launch counts) are
identical to the parent's.  Its head forward rounds differently (the affine above), so results are not bit-identical to the
parent's: that step's Loss 448.98322 against 448.98328.  bench.py --gpus 1 --steps 20 --warmup 5, same visit, alternating:
parent 26.979, 26.989 ms per U-Net step, this tree 27.034, 27.030 ms (+0.05 ms: the affine's 32 FMAs per lane and tile).
Run time of this file on the MI355X machine: 5.1 s (114 tests; the slowest 0.6 s, the 36 864-row reference)."""
import contextlib
import functools
import os

import numpy as np
import pytest

import conv_layer_ref as CR
import head_link_ref as HR

pytestmark = pytest.mark.gpu

TOL = 1e-5
CAP = 8
BNFUSE, FOLD, FUSED, FAST = "ICSG3D_NO_HEAD_BNFUSE", "ICSG3D_NO_BWD_FOLD", "ICSG3D_NO_FUSED_HEAD", "ICSG3D_NO_FAST_BNBWD"
ROUTES = {"default": (), "no_bnfuse": (BNFUSE,), "no_bnfuse_no_fold": (BNFUSE, FOLD), "no_fused_head": (FUSED,), "no_fast_bnbwd": (FAST,)}
NCLS95 = [s for s, v in HR.SHAPES.items() if v[3] == 95]
ROUTE_CASES = [(s, r) for s in NCLS95 for r in ROUTES if s != "waves" or r in ("default", "no_bnfuse")]
T, F, G = "conv_dgrad:head|head_dgrad_kernel<true>", "conv_dgrad:head|head_dgrad_kernel", "conv_dgrad:head|conv_fwd_kernel<"


def _rows(d):
    return d["B"] * d["S"] ** 3


def _fusable(d, env):
    return d["ncls"] == 95 and _rows(d) % 16 == 0 and FUSED not in env


def expected_sites(d, env):
    """(rows that must be there -- a trailing '$' asks for the whole row --, fragments that must not)"""
    have, lack = ["conv_fwd:P|", "conv_wgrad:head|", "conv_wgrad:P|", "conv_dgrad:P|"], []
    if _fusable(d, env):
        have += ["head_fused"]
        lack += ["head_softmax_loss", "conv_fwd:head|"]
        if BNFUSE not in env:
            have += [T]
            lack += ["bn_act_bwd:P"]
            if d["ranks"]:
                have += ["xhat_affine:head", "head_bnfuse_exchange"]
        else:
            have += [F + "$", "bn_act_bwd:P"]
            lack += ["<true>", "xhat_affine", "head_bnfuse_exchange"]
    else:
        have += ["conv_fwd:head|", "head_softmax_loss", G, "bn_act_bwd:P"]
        lack += ["head_fused", "head_dgrad_kernel", "xhat_affine", "head_bnfuse_exchange"]
    return have, lack


def reaches(d, env):
    """does the switch set change the arithmetic of this case?  True / False / None (not asserted, see the header)"""
    if not env:
        return False
    if _fusable(d, ()):
        return env != (FAST,)
    return False if env in ((BNFUSE,), (FUSED,)) else None


@functools.lru_cache(maxsize=None)
def _data(shape, regime="ordinary", ranks=0, rank_regime=None):
    return HR.rank_case_data(shape, ranks, rank_regime) if ranks else HR.case_data(shape, regime)


@functools.lru_cache(maxsize=None)
def _reference(shape, regime="ordinary", ranks=0, rank_regime=None):
    """fp64 forward / backward with the reference's own decisions, and e32 -- once per input, never modified"""
    d = _data(shape, regime, ranks, rank_regime)
    fP, fh, t, _ = HR.reference(d)
    return fP, fh, t, HR.e32_of(d, fP, fh, t)


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: "1" for k in env})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _run(shape, env=(), regime="ordinary", ranks=0, rank_regime=None):
    from icsg3d_amd import engine as E
    d = _data(shape, regime, ranks, rank_regime)
    mb = None if ranks else HR.SHAPES[shape][4]
    with _env(env):
        return E.head_link(d["x0"], d["P"], d["head"], d["labels"], loss_weight=d["loss_weight"], class_weights=d["class_weights"],
                           bce_from_logits=d["bce_from_logits"], max_batch=mb, ranks=ranks)


WORST = {}


def _note(key, err, yard, what):
    if key not in WORST or err / max(yard, 1e-300) > WORST[key][0] / max(WORST[key][1], 1e-300):
        WORST[key] = (err, yard, what)


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(np.abs(b).max(), 1e-300))


def _check_sites(r, d, env, what):
    for sites in (r["sites"] if d["ranks"] else [r["sites"]]):
        have, lack = expected_sites(d, env)
        for frag in have:
            ok = (frag[:-1] in sites) if frag.endswith("$") else any(frag in ln for ln in sites)
            assert ok, (what, "missing", frag, sites)
        for frag in lack:
            rows = [ln for ln in sites if frag in ln]
            assert not rows, (what, "unexpected", frag, rows)
    assert r["dy_in_place"] == (_fusable(d, env) and BNFUSE not in env), what


def _check_forward(r, d, fP, what):
    e = _rel(r["y"], fP["y"])
    _note("y", e, TOL, what)
    assert e <= TOL, (what, "P.y", e)
    m64, v64 = CR.channel_stats(r["y"])           # of the whole batch: under ranks every rank holds the global statistics
    P = d["P"]
    for k in range(max(d["ranks"], 1)):
        o = {n: (r[n][k] if d["ranks"] else r[n]) for n in ("mean", "rstd", "scale", "shift")}
        mu = CR.ulps32(o["mean"], m64, at=np.maximum(np.abs(m64), np.sqrt(v64)))
        ve = CR.var_error(1.0 / o["rstd"].astype(np.float64) ** 2, v64)
        bound = CR.var_bound(m64, v64)
        _note("mean ulps", float(mu.max()), CR.MEAN_ULPS, what)
        _note("var+eps / bound", float((ve / bound).max()), 1.0, what)
        assert (mu <= CR.MEAN_ULPS).all(), (what, "mean", mu.max(), int(mu.argmax()))
        assert (ve <= bound).all(), (what, "var + eps", ve.max(), int((ve / bound).argmax()))
        u = CR.ulps32(o["scale"], P["gamma"] * o["rstd"])
        assert (u <= 1).all(), (what, "scale", u.max())
        prod = o["mean"].astype(np.float64) * o["scale"].astype(np.float64)
        sh = P["beta"].astype(np.float64) - prod
        u = CR.ulps32(o["shift"], sh, at=np.maximum(np.abs(sh), np.maximum(np.abs(prod), np.abs(P["beta"]))))
        assert (u <= 1).all(), (what, "shift", u.max())


def _check_metrics(r, d, what):
    """the fp64 reference on the op's OWN stored y and float32 affine; tolerances of tests/test_gpu_metrics.py"""
    fh = HR.head_forward(d, HR.affine_of(d, r))
    met, sums, near = HR.head_metrics(d, fh, d["ranks"])
    assert near.sum() <= CAP, (what, near)
    for k in range(max(d["ranks"], 1)):
        m = r["metrics"][k] if d["ranks"] else r["metrics"]
        s = r["sums"][k] if d["ranks"] else r["sums"]
        got = np.array([s[n] for n in ("sum_lsoft", "sum_lsig", "tp", "predicted", "wr_tp", "wr_possible", "voxels")])
        print("  %s rank %d: metrics %s | reference %s; counts %s | %s; near 0.5: %d" % (what, k, m, met[k], got[2:], sums[k][2:], near[k]))
        for i, n in ((0, "Loss"), (1, "lsoft"), (2, "lsig")):
            e = abs(float(m[i]) - met[k][i]) / max(abs(met[k][i]), 1e-300)
            _note("metric " + n + (" (saturated sigmoid, clipped form)" if i != 1 and not d["bce_from_logits"]
                                   and (fh["ps"] > 1 - 2.0 ** -12).any() else ""), e, 1e-5, what)
        # the clipped-probability form AT saturation is a float32 statement (tests/test_gpu_metrics.py,
        # test_bce_from_logits_switch_on_the_device: 1 - p has a handful of bits left, the kernels mirror a float32 Keras
        # graph): that file holds it to 5e-3 of the fp64 value, and so does this one -- where the REFERENCE finds a sigmoid
        # above 1 - 2^-12 in that form (the sharp head); everywhere else 1e-5
        sat = not d["bce_from_logits"] and bool((fh["ps"] > 1 - 2.0 ** -12).any())
        tol_sig = 5e-3 if sat else 1e-5
        np.testing.assert_allclose(m[1], met[k][1], rtol=1e-5, err_msg=what)
        np.testing.assert_allclose(m[2], met[k][2], rtol=tol_sig, err_msg=what)
        if sat:
            # ... and, as tests/test_gpu_metrics.py:196-201, to 2e-5 of the SAME formula evaluated in float32 numpy, on
            # the float32 logit of the op's own affine
            f = np.float32
            n = fh["lab"].size // max(d["ranks"], 1)
            z32 = fh["zg"][k * n:(k + 1) * n].astype(f)
            with np.errstate(over="ignore"):
                p32 = (f(1) / (f(1) + np.exp(-z32))).astype(f)
            pc = np.clip(p32, f(1e-7), f(1) - f(1e-7))
            t32 = fh["t"][k * n:(k + 1) * n].astype(f)
            ref32 = float((-(t32 * np.log(pc) + (f(1) - t32) * np.log(f(1) - pc))).astype(np.float64).mean())
            e = abs(float(m[2]) - ref32) / ref32
            print("  %s lsig against the float32 formula: %.3g (of 2e-5)" % (what, e))
            _note("metric lsig vs float32 formula (saturated)", e, 2e-5, what)
            np.testing.assert_allclose(m[2], ref32, rtol=2e-5, err_msg=what)
        np.testing.assert_allclose(m[0], met[k][0], rtol=0, atol=1e-5 * met[k][1] + tol_sig * met[k][2], err_msg=what)
        np.testing.assert_allclose(m[0], float(m[1]) + float(m[2]), rtol=1e-6, err_msg=what)
        np.testing.assert_allclose(got[0], sums[k][0], rtol=1e-5, err_msg=what)
        np.testing.assert_allclose(got[1], sums[k][1], rtol=tol_sig, err_msg=what)
        assert (np.abs(got[2:5] - sums[k][2:5]) <= near[k]).all() and got[5] == sums[k][5] and got[6] == sums[k][6], (what, got, sums[k])
        own = HR.metrics_from_sums(got)
        np.testing.assert_allclose(m[3:], own[3:], rtol=1e-5, atol=1e-12, err_msg=what)
        if near[k] == 0:
            np.testing.assert_allclose(m[3:], met[k][3:], rtol=1e-5, atol=1e-12, err_msg=what)


def _op_pins(r, d, fh64):
    """the op's decisions: its stored y, and the clip sides read off its dz (a clipped voxel's part of the row is exactly
    zero; where the loss weight is zero the row says nothing and the reference's own side stands)"""
    ncls = d["ncls"]
    dz = r["dz"].reshape(-1, ncls + 1)
    wv = HR.loss_weights(d)
    si = np.where(wv > 0, (dz[:, :ncls] != 0).any(-1), fh64["soft_inside"])
    gi = fh64["sig_inside"] if d["bce_from_logits"] else dz[:, ncls] != 0
    return {"y": r["y"], "soft_inside": si, "sig_inside": gi}


def _check_grads(r, d, ref, what, show=True):
    fP, fh, t64, e32 = ref
    pins = _op_pins(r, d, fh)
    same = (np.array_equal(pins["y"] > 0, fP["y"] > 0) and np.array_equal(pins["soft_inside"], fh["soft_inside"])
            and np.array_equal(pins["sig_inside"], fh["sig_inside"]))
    tref, pinned = (t64, {"relu": 0, "clip": 0}) if same else HR.backward(d, fP, fh, pins)
    assert pinned["relu"] <= CAP and pinned["clip"] <= CAP, (what, pinned)
    err = HR.rel_errors(r, tref, fP)
    bad = []
    for k in HR.GRAD_KEYS:
        lim = max(TOL, 2 * e32[k])
        if show:
            print("  %s %-10s engine %.3g  e32 %.3g  bound %.3g  pinned %s" % (what, k, err[k], e32[k], lim, pinned))
        _note("grad " + k, err[k], lim, what)
        if not err[k] <= lim:
            bad.append((k, err[k], e32[k], lim))
    assert not bad, (what, bad)


def _full(shape, env=(), regime="ordinary", ranks=0, rank_regime=None):
    what = "%s %s %s R%d %s" % (shape, "+".join(e[7:] for e in env) or "default", regime, ranks, rank_regime or "")
    d = _data(shape, regime, ranks, rank_regime)
    ref = _reference(shape, regime, ranks, rank_regime)
    r = _run(shape, env, regime, ranks, rank_regime)
    _check_sites(r, d, env, what)
    _check_forward(r, d, ref[0], what)
    _check_metrics(r, d, what)
    _check_grads(r, d, ref, what)
    return r


def _check_against_default(r, shape, env, regime="ordinary"):
    d = _data(shape, regime)
    base = _run(shape, (), regime)
    hit = reaches(d, env)
    if hit is True:
        assert not np.array_equal(r["dy_p"], base["dy_p"]), (shape, env, "dy_p equals the default route's bit for bit")
    elif hit is False:
        assert r["sites"] == base["sites"], (shape, env, "the switch changed the launches of a case it cannot reach")
        for k in HR.GRAD_KEYS:
            assert np.array_equal(r[k], base[k]), (shape, env, k, "the switch changed a case it cannot reach")


@pytest.mark.parametrize("shape,route", ROUTE_CASES, ids=lambda v: str(v))
def test_head_link_route(shape, route):
    """every ncls = 95 shape on the five routes: one tile (three idle waves), a ragged block, whole blocks, a handle larger
    than the batch, 2304 tiles over 2048 waves (a second, prefetched tile for 256 of them), and 8 rows, which both fused
    kernels refuse"""
    env = ROUTES[route]
    r = _full(shape, env)
    _check_against_default(r, shape, env)


@pytest.mark.parametrize("shape", ["ncls31", "ncls20", "ncls127"])
def test_head_link_other_class_counts(shape):
    """the generic route at ncls + 1 = 32 (vector loads of dz), 21 and 128 (the column-buffer limit)"""
    _full(shape)


@pytest.mark.parametrize("route", ["default", "no_bnfuse"])
@pytest.mark.parametrize("regime", [g for g in HR.REGIMES if g != "ordinary"])
@pytest.mark.parametrize("shape", HR.REGIME_SHAPES)
def test_head_link_value_regimes(shape, regime, route):
    """P at mean/std 30 and 1000, a dead channel, a sharp head at the clip, the logits form of the sigmoid loss, a scalar
    weight other than ncls, a class-weight table with zeros and 1e3 (the kernels' CW instantiation), degenerate label sets"""
    env = ROUTES[route]
    r = _full(shape, env, regime)
    _check_against_default(r, shape, env, regime)


@pytest.mark.parametrize("ranks", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", list(HR.RANK_SHAPES))
def test_head_link_syncbn_ranks(shape, ranks):
    """emulated ranks on the default route: xhat_affine_kernel, the 256-double exchange, bn_bwd_sync_c_kernel, against the
    reference with global-batch statistics; parameter gradients per rank"""
    _full(shape, (), "ordinary", ranks)


@pytest.mark.parametrize("ranks", [2, 4])
@pytest.mark.parametrize("shape", list(HR.RANK_SHAPES))
def test_head_link_syncbn_shards_that_differ_in_mean(shape, ranks):
    _full(shape, (), "ordinary", ranks, HR.RANK_REGIME)


@pytest.mark.parametrize("route", ["default", "no_bnfuse", "no_fused_head"])
@pytest.mark.parametrize("shape", ["one_tile", "rows8", "big_handle"])
def test_head_link_leaves_the_guard_bytes_clean(shape, route, monkeypatch):
    """ICSG3D_DEBUG_CANARY: the op fails, naming the buffers, if anything was written behind a buffer of the handle -- the
    bias-gradient partials of a one-block launch, dz column partials, the handle sized for 5 grids running 2"""
    monkeypatch.setenv("ICSG3D_DEBUG_CANARY", "1")
    from icsg3d_amd import engine as E
    d = _data(shape)
    with _env(ROUTES[route]):
        r = E.head_link(d["x0"], d["P"], d["head"], d["labels"], max_batch=HR.SHAPES[shape][4])
    base = _run(shape, ROUTES[route])
    for k in HR.GRAD_KEYS:
        assert np.array_equal(r[k], base[k]), (shape, route, k)


def test_zz_report_worst_gaps():
    """prints the worst (engine error, yardstick) pairs of this run: the source of the measured table"""
    for k in sorted(WORST):
        print("  %-18s %.3g  (of %.3g)  %s" % (k, WORST[k][0], WORST[k][1], WORST[k][2]))
