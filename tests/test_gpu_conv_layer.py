"""The conv kernels in the form the ENGINES launch them, one layer at a time (ics_op_conv_layer), against the fp64
reference of tests/conv_layer_ref.py: BatchNorm-affine / activated / upsampled sources (zero padding after the affine),
[skip | up] pairs with accumulate, the per-block (count, mean, M2) statistics epilogue of every kernel family and
bn_finalize, handles larger than the batch, and the value regimes (mean >> std, constant, all-zero, var << eps, 1e4) in
which a one-pass sum or an equal-count merge of a ragged block would show.  Every case asserts the kernel ids the op
returns, so a dispatch change cannot turn it into a test of another kernel.

path -> cases (B, S, sources -> Cout) -> kernel ids: the PATHS table below (DESIGN.md section 21 has the same list).
Deviations from the planned table, each because the path's own predicate decides otherwise:
  * thin-C serves PLAIN single-channel sources only (conv_thin_c_ok refuses an affine): its cases run with plain sources,
    as U-Net c1 / VAE e0 see their input; the pad_input case (2, 8, 4 -> 32) is served by conv_fwd_kernel's thin loader.
    The condition fold, which puts the K.tile'd condition of VAE e0 through the same stencil, has the paths cond_fold /
    cond_bcast below.
  * split-K forward: the smallest S <= 4 geometry whose training plan splits K is (3, 4, 128 -> 40) (64 x 64 tile needs
    Npad % 64 == 0, conv_winog takes Cout % 64 == 0): 12 splits.  The kernel id is conv_fwd_kernel with and without the
    split; the case asserts that ICSG3D_NO_FWD_SPLITK changes the bits of y.
  * ICSG3D_NO_REUSE / _NO_WGRAD3 / _NO_WGRAD3S do not change the kernels of the three planned implicit-GEMM shapes: the
    dx-reuse forward / backward-data pipeline needs Cin % 32 == 0 of the convolution it runs, conv_wgrad3_kernel
    Cin % 64 == 0 and Cout % 128 == 0 (wgrad3_ok), conv_wgrad3s_kernel S >= 16 on top.  Two shapes are added:
    (2, 8, 64 -> 24), whose forward takes the dx-reuse instantiation, and (1, 16, 64 -> 128) under ICSG3D_NO_WINO (the
    Winograd kernels take it otherwise), which runs conv_fwd_kernel<.., REUSE = true, ..> in both directions and
    conv_wgrad3s_kernel.  Each case asserts the template parameter or kernel name the switch changes: REUSE true -> false,
    conv_wgrad3s_kernel -> conv_wgrad3_kernel -> conv_wgrad_kernel; at the shapes a switch cannot reach, that nothing changed.
  * [skip | up] asserts conv_up3_kernel<.., STATS = false, 1> (the statistics are the accumulating skip launch's) and
    <.., 2>, the 32-voxel tile, under ICSG3D_UP3_BIG_MIN_WG=1.  An up-only layer with Cout % 64 == 0 (VAE d1) is served by
    conv_up3_kernel<.., STATS = true, ..>, not conv_up3n: (2, 8, up 64 -> 64) is added for that instantiation.
  * The op runs with the handle's profiler on (that is where the kernel ids come from), and a profiled handle keeps the
    backward-weight launches on the main stream where a train step puts them on its side stream: same kernels, same
    instantiations, same arguments, one stream.

Bounds (none taken from what the kernels give):
  y            tensor-relative 1e-5, separately on border and interior voxels
  mean         4 float32 ulps of max(|mean|, std), against fp64 statistics of the op's own stored y
  var + eps    from rstd, relative: conv_layer_ref.var_bound = max(1e-5, 1.1e-7 |mean| std / (var + eps)), calibrated in
               tests/test_conv_layer_host.py (two-pass float32 >= 10x inside, one-pass >= 10x outside at mean/std >= 100)
  constant / all-zero channels: rstd within 2 ulps of 1/sqrt(eps)
  scale        gamma * rstd in float32: 1 ulp
  shift        beta - mean * scale in float32 (fused or not): 1 ulp AT THE LARGER OPERAND, max(|shift|, |mean scale|, |beta|),
               not at the result -- looser than "to 1 ulp" reads where the subtraction cancels, and all a float32
               subtraction of two rounded operands can promise there
  moving_*     numpy_ref.bn_moving_update of the op's own (mean, 1/rstd^2 - eps), evaluated in float32 with the kernel's
               float32 momentum 0.99f: 2 ulps -- for moving_var plus what the rounding of rstd leaves open in the
               REFERENCE's input (the op returns rstd, not var: 2^-23 of var + eps, through 0.01 n / (n - 1 - eps)):
               +0.02 ulps where var ~ 1, up to +2 in the 1e4 regime, where the kernel -- which updates from its fp64
               variance -- is 3 ulps from the update of the recovered one
  gradients    tensor-relative max(1e-5, 2 e32) per tensor, in the ordinary regime and with every channel at
               mean/std = 30; e32 = the same formulas in float32 numpy against the same fp64 reference (with the fp64
               reference's activation decisions: rounding alone, no flipped voxel inflates the yardstick); the fp64
               reference's decisions pinned to the op's stored y / its own fp32 affine (<= 8 per tensor)
  The value regimes run in every case whose forward kernel differs from the path's first: all three thin-N cases (Cout = 1 is
  thin1_gather_kernel's own 256-row epilogue; seven launches put every regime through its one channel), thin-C's 4-channel
  case, up-only's conv_up3 case.

Measured on the MI355X, worst over all cases (engine error | yardstick):
  y border 1.42e-6, interior 1.89e-6 | 1e-5
  mean 3.0 ulps | 4        var + eps 0.256 of its bound (1.24e-5 at mean/std = 871 through conv_up3n, bound 9.6e-5; 1.16e-5 at
                           1620 through conv_wino64, bound 1.8e-4: the kernels do exceed a flat 1e-5 there, as the emulation)
  moving_mean 0 ulps | 2   moving_var 3 ulps | 2 + 1.85 (up-only conv_up3, 1e4 regime; <= 2 of 2.02 elsewhere)
  scale, shift <= 1 ulp | 1
  ordinary regime, engine (e32 of that case): dw 1.39e-6 (1.6e-6), dbias 8.81e-6 (3.3e-6), dgamma 2.59e-6 (5.1e-7),
  dbeta 4.67e-7 (0), dx0 1.40e-6 (3.2e-7), dx1 1.06e-6 (2.3e-7) | max(1e-5, 2 e32)
  every channel at mean/std = 30 (22 .. 64 as measured on the reference's y), worst per tensor over the 13 cases x 2 forms:
  dw 1.94e-6 (1.4e-5, conv_wino), dbias 1.71e-6 (1.3e-5), dgamma 3.91e-6 (4.1e-5, conv_wino64), dbeta 7.45e-7 (0, thin1),
  dx0 1.37e-6 (1.3e-6, split-K), dx1 4.29e-7 (2.6e-6): the float32 formulas lose 1e-5 .. 6e-5 there, the engines stay
  below 4e-6 -- every one inside the flat 1e-5
  pinned activation decisions: 1 in (1, 16, 64 -> 128), U-Net form; 0 in every other case
  In the train steps of test_gpu_unet.py / test_gpu_vae.py (conv_layer_ref.check_bn_affine): mean <= 2.66 ulps, var + eps <=
  0.063 of its bound.
Mutations tried in a scratch copy of conv_wino64.hip, run against the wino64 and skip_up cases (30 tests):
  * its statistics epilogue as a one-pass sum (pair sum of squares, M2 = sum x^2 - n mean^2 in float32):
    test_statistics_in_every_value_regime[wino64-*] and [skip_up-*] fail with var + eps off by 6.7e-2 / 1.5e-1 (channel 2,
    mean/std = 1000; bound 1.1e-4); the other 26 tests, all in the ordinary regime, still pass -- which is why the regimes
    are there.
  * its loader zeroing the halo BEFORE the affine (sstore / hstore): every wino64 and skip_up case fails its border check
    with 0.49 / 0.34 / 0.33 / 0.29 (bound 1e-5; 16 tests, the assertion in front of the interior's), the four regime tests
    fail their per-channel y check; the 10 tests that pass are the plain-source ones (no affine) and the switches that
    route around the kernel.
  * thin1_gather_kernel's statistics epilogue as a one-pass sum (M2 = max(sum x^2 - n mu^2, 0) in float32), run against
    the thin-N cases (27 tests): the four tests of (2, 8, 16 -> 1) that leave the ordinary regime fail --
    test_statistics_in_every_value_regime[thin_n-2-*] with var + eps off by 3.2e-5 / 1.2e-4 already at mean/std = 30
    (bound 1e-5; the launch in front of the mean/std = 1000 one) and test_gradients_at_mean_over_std_30[thin_n-2-*] with
    3.2e-5 / 2.8e-5 -- and the 23 others pass.
Condition sources (VAE e0: x | K.tile'd condition, a source dict with "bcast"; the reference is conv_layer_ref's plain one on
the materialised input, np.tile order): path cond_fold -- one x channel, 16 / 32 filters, (2, 4, 1+10 -> 16), (3, 8, 1+10 -> 16),
(5, 8, 1+3 -> 32), (2, 16, 1+10 -> 16), (2, 8, 1+1 -> 16), (2, 8, 1+7 -> 32) -- asserts "cond_bias_table_kernel +
conv_thin_c_fwd_kernel<1, N>" and "conv_thin_c_wgrad_kernel<N> + cond_wgrad_kernel" (the fold's two launch sites name both of
their kernels), and under ICSG3D_NO_COND_FOLD / _NO_THIN_C conv_fwd_kernel / conv_wgrad_kernel with y AND dw required to
differ in bits from the fold's; path cond_bcast -- four x channels, (2, 8, 4+40 -> 16) through the materialised input,
(3, 4, 4+12 -> 16) and (2, 8, 4+4 -> 12) through the loader's broadcast branch.  On top of every check above: dw per row group
(x rows | condition rows | their centre tap | their 26 other taps), each on its own scale at max(1e-5, 2 e32) (rule for the one
group that can be exactly zero: conv_layer_ref.row_group_errors); test_condition_regimes (same condition in every sample, one
sample's all zero, conditions of 1e3) on each of the four routes; test_condition_without_batchnorm (has_bn = 0, mean(dy) ~ 1).
  Measured, worst over the condition cases (engine | e32): dw_x 1.11e-6 (5.1e-7), dw_cond 2.14e-6 (8.1e-6), centre tap
  3.55e-6 (1.3e-5), other taps 1.85e-6 (7.9e-6) | max(1e-5, 2 e32); 0 pinned decisions in every condition case.
  Mutations, each one line in a scratch copy, run against the 71 condition tests and against test_gpu_vae.py:
  (a) cond_bias_table_kernel with the first and last class swapped on x: 31 fail, first at the border check of y with 0.35 ..
      0.59 (bound 1e-5) -- every cond_fold test on the fold route; the switched routes and cond_bcast pass.
  (b) cond_wgrad_kernel's interior as `tot` without `- border`: 29 fail with dw off by 0.62 .. 0.82 -- every backward test on
      the fold route (the two forward-only regime tests pass).
  (c) the loader's `cl % bcast` as `cl / C`: 19 fail, y border off by 0.41 .. 0.98 -- all of cond_bcast; cond_fold passes
      even under its switches (with one x channel the two orders coincide), which is why the C = 4 path is there.
  The whole-step test would have caught each of them too: test_gpu_vae.py fails under (a) ("activation signs of e0 differ",
  6182 .. 12990 elements, C = 1), (b) (e0/kernel off by 0.44 .. 0.59, C = 1) and (c) (activation signs, C = 4 only).  What
  the cases here add is the route (which kernel, which row group), shapes down to S = 4 and the regimes no step reaches.
Run time of this file on the MI355X machine: 9.6 s (243 tests; the fp64 references take most of it on the host)."""
import contextlib
import functools
import os
import re

import numpy as np
import pytest

import conv_layer_ref as CR
from oracle import numpy_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-5
FORMS = ("unet", "vae")

# kernel-id fragments
W64F, W64B = "conv_wino64_kernel<true", "conv_wino64_kernel<false"
W32F, W32B = "conv_wino_kernel<true", "conv_wino_kernel<false"
WW, WG, IG, IGW = "conv_wino_wgrad_kernel", "conv_winog", "conv_fwd_kernel<", "conv_wgrad_kernel<"


def K(fwd, dgrad, wgrad):
    return {"fwd": fwd, "dgrad": dgrad, "wgrad": wgrad}


def _tf(v):
    return r"(true|false)" if v is None else "true" if v else "false"


def IGR(reuse):
    """conv_fwd_kernel<WM, WN, TM, TN, VEC, ABL, AFF, UP, THIN, REUSE, ..> with the given dx-reuse parameter"""
    return re.compile(r"conv_fwd_kernel<\d, \d, \d, \d, %s, 0, %s, %s, %s, %s, " % (_tf(None), _tf(None), _tf(None), _tf(None), _tf(reuse)))


def UP3(stats, tile=r"\d"):
    """conv_up3_kernel<AFF, NOACT, STATS, tile>: tile 1 = 16-voxel workgroups, 2 = 32-voxel ones"""
    return re.compile(r"conv_up3_kernel<%s, %s, %s, %s>" % (_tf(None), _tf(None), _tf(stats), tile))


def case(B, S, src, Cout, taps=27, pad=False, aff=True, env=()):
    """env: switches the case always runs under (they route it to the kernel the path is about).  src: (C, up) per source;
    (C, 0, ncond) is a condition source (conv_layer_ref.make_case)"""
    return {"B": B, "S": S, "src": tuple(src), "Cout": Cout, "taps": taps, "pad": pad, "aff": aff, "env": tuple(env)}


IGEMM_CASES = [case(2, 8, [(40, 0)], 24), case(3, 4, [(48, 0)], 40), case(3, 4, [(96, 0)], 48, taps=1),
               case(2, 8, [(64, 0)], 24), case(1, 16, [(64, 0)], 128, env=("ICSG3D_NO_WINO",))]


def _igemm_ids(idx, env, plain):
    """the dx-reuse forward / backward-data pipeline needs vector loads (the convolution's Cin % 32 == 0; backward-data
    convolves Cout -> Cin) and 27 taps: (2, 8, 64 -> 24) forward, (1, 16, 64 -> 128) both.  The dx-reuse backward-weight
    kernels need Cin % 64 == 0 and Cout % 128 == 0, their wave-uniform variant S >= 16 on top: the last case only."""
    c = IGEMM_CASES[idx]
    on = env != "ICSG3D_NO_REUSE" and c["taps"] == 27
    wg = IGW
    if idx == 4:
        wg = {"ICSG3D_NO_WGRAD3": IGW, "ICSG3D_NO_WGRAD3S": "conv_wgrad3_kernel<"}.get(env, "conv_wgrad3s_kernel<")
    return K([IGR(on and c["src"][0][0] % 32 == 0)], [IGR(on and c["Cout"] % 32 == 0)], [wg])


UP_ONLY_CASES = [case(2, 8, [(32, 1)], 16), case(3, 8, [(64, 1)], 32), case(2, 8, [(64, 1)], 64)]


def _up_only_ids(idx, env, plain):
    """Cout % 64 == 0 goes to conv_up3_kernel, which then carries bias, activation and the statistics itself (VAE d1)"""
    if env == "ICSG3D_NO_UPSPLIT":
        return K([IG], None, ["conv_wgrad"])
    if idx == 2:
        return K([UP3(not plain)], [IG], [IGW])
    return K([IG] if env == "ICSG3D_NO_UP3N" else ["conv_up3n_kernel"], [IG], [IGW])


# path -> cases, expected kernel ids per launch site (in launch order), and the switches it also runs under with the ids
# expected then.  None: the site's kernel differs from case to case and is not what the path is about (the backward-data
# launch of a narrow layer is itself a thin / Winograd convolution Cout -> Cin); "conv_wgrad": conv_wgrad_kernel or the
# dx-reuse conv_wgrad3_kernel, by size.
PATHS = {
    "wino64": dict(
        cases=[case(3, 8, [(64, 0)], 64), case(1, 16, [(128, 0)], 64)], ids=K([W64F], [W64B], [WW]),
        env={"ICSG3D_NO_WINO64": K([W32F], [W32B], [WW]), "ICSG3D_NO_WINO": K([IG], [IG], [IGW])}),
    "wino32": dict(
        cases=[case(2, 8, [(32, 0)], 96), case(3, 8, [(96, 0)], 32)], ids=K([W32F], [W32B], [WW]),
        env={"ICSG3D_NO_WINO": K([IG], [IG], [IGW])}),
    "winog": dict(      # B % 4 != 0: backward-weight leaves the Winograd domain
        cases=[case(4, 4, [(64, 0)], 64), case(3, 4, [(128, 0)], 64)], ids=K([WG], [WG], [WG]),
        ids_by_case={1: K([WG], [WG], [IGW])}, env={"ICSG3D_NO_WINOG": K([IG], [IG], [IGW])}),
    "igemm": dict(
        cases=IGEMM_CASES, ids_fn=_igemm_ids, env=("ICSG3D_NO_REUSE", "ICSG3D_NO_WGRAD3", "ICSG3D_NO_WGRAD3S")),
    "splitk": dict(
        cases=[case(3, 4, [(128, 0)], 40)], ids=K([IG], [IG], [IGW]), env={"ICSG3D_NO_FWD_SPLITK": K([IG], [IG], [IGW])},
        must_differ=("ICSG3D_NO_FWD_SPLITK",)),
    "thin_n": dict(
        cases=[case(2, 8, [(16, 0)], 4), case(2, 8, [(16, 0)], 2), case(2, 8, [(16, 0)], 1)],
        ids=K(["conv_thin_n_fwd_kernel"], None, ["conv_thin_n_wgrad_kernel"]),
        ids_by_case={2: K(["thin1_taps_kernel + thin1_gather_kernel"], None, ["thin1_wgrad_kernel"])}, regimes=(0, 1, 2),
        env={"ICSG3D_NO_THIN_N": K([IG], None, [IGW]),
             "ICSG3D_NO_THIN1_2STAGE": K(["conv_thin_n_fwd_kernel"], None, ["conv_thin_n_wgrad_kernel"])}),
    "thin_c": dict(
        cases=[case(2, 8, [(1, 0)], 16, pad=True, aff=False), case(3, 16, [(1, 0)], 32, pad=True, aff=False),
               case(2, 8, [(4, 0)], 32, pad=True)],
        ids=K(["conv_thin_c_fwd_kernel<1, "], None, ["conv_thin_c_wgrad_kernel"]),
        ids_by_case={2: K([IG], None, [IGW])}, env={"ICSG3D_NO_THIN_C": K([IG], None, [IGW])}, regimes=(0, 2)),
    "skip_up": dict(
        cases=[case(2, 8, [(32, 0), (64, 1)], 64), case(1, 16, [(64, 0), (128, 1)], 128)],
        ids=K([UP3(False, 1), W64F], None, [WW, IGW]),      # the statistics are the accumulating skip launch's
        env={"ICSG3D_UP3_BIG_MIN_WG": K([UP3(False, 2), W64F], None, [WW, IGW]),
             "ICSG3D_NO_UP3": K([IG, W64F], None, [WW, IGW]), "ICSG3D_NO_UPSPLIT": K([IG], None, ["conv_wgrad"])}),
    "up_only": dict(
        cases=UP_ONLY_CASES, ids_fn=_up_only_ids, env=("ICSG3D_NO_UP3N", "ICSG3D_NO_UPSPLIT"), regimes=(0, 2)),
    # the VAE's e0: x | K.tile'd condition, padded input, plain sources.  One x channel and 16 / 32 filters: the fold
    # (cond_bias_table_kernel + the stencil's pos_bias epilogue; the stencil reduction + sample_colsum / border_region_sums /
    # cond_wgrad_kernel in ONE launch site); with either switch the same layers through the implicit-GEMM kernels -- the
    # materialised padded input (1 + 10 -> 16, 1 + 1 -> 4 channels) or the loader's broadcast branch (1 + 3, 1 + 7: no padding)
    "cond_fold": dict(
        cases=[case(B, S, src, Cout, pad=True, aff=False) for B, S, src, Cout in CR.COND_FOLD_CASES],
        ids=K(["cond_bias_table_kernel + conv_thin_c_fwd_kernel<1, "], None,
              [re.compile(r"conv_thin_c_wgrad_kernel<\d+>.* \+ .*cond_wgrad_kernel")]),
        env={"ICSG3D_NO_COND_FOLD": K([IG], None, [IGW]), "ICSG3D_NO_THIN_C": K([IG], None, [IGW])},
        must_differ=("ICSG3D_NO_COND_FOLD", "ICSG3D_NO_THIN_C"), differ_dw=True),
    # four x channels: never folded.  4 + 40 -> 64 materialised, 4 + 12 = 16 and 4 + 4 = 8 through the broadcast branch
    "cond_bcast": dict(
        cases=[case(B, S, src, Cout, pad=True, aff=False) for B, S, src, Cout in CR.COND_BCAST_CASES],
        ids=K([IG], None, [IGW]), env={}),
}
COND_PATHS = ("cond_fold", "cond_bcast")
ORDER = tuple(PATHS)
ALL = [(p, i) for p, d in PATHS.items() for i in range(len(d["cases"]))]


def _case(path, idx):
    """idx "big": the path's handle-size case -- its first case with B = 3, or its first case at B = 3"""
    cases = PATHS[path]["cases"]
    if idx != "big":
        return cases[idx]
    return dict(cases[_big_idx(path)], B=3)


def _big_idx(path):
    return next((i for i, c in enumerate(PATHS[path]["cases"]) if c["B"] == 3), 0)


ALL_ENV = [(p, e) for p, d in PATHS.items() for e in d["env"]]
WORST = {}          # name -> (engine error, yardstick): printed at the end of the module


def _note(name, err, yard):
    if name not in WORST or err / max(yard, 1e-300) > WORST[name][0] / max(WORST[name][1], 1e-300):
        WORST[name] = (err, yard)


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(np.abs(b).max(), 1e-300))


def _rel_grad(k, got, ref, kw, linear=False):
    """tensor-relative error of gradient tensor k.  The bias of a layer whose BatchNorm follows the convolution directly
    (no pre-activation, or -- linear -- a ReLU that the fp64 reference finds open at every voxel, as at mean/std = 30) has a
    gradient of exactly zero -- the batch mean removes it -- and the reference holds only its own rounding noise there:
    measured on the scale of the same layer's kernel gradient instead (as tests/test_gpu_vae.py does)."""
    scale = np.abs(ref[k]).max()
    if k == "dbias" and kw["has_bn"] and (not kw["pre_act"] or linear):
        scale = max(scale, np.abs(ref["dw"]).max())
    return float(np.abs(np.asarray(got[k], np.float64) - ref[k]).max() / max(scale, 1e-300))


def _well_conditioned(d):
    """dgamma and dbeta of a layer with one to four output channels are one to four sums of N = B S^3 terms of either sign.
    Such a sum is typically sqrt(N) times smaller than the sum of its terms' magnitudes; a draw where it is very much
    smaller than that (the first seed of (2, 8, 16 -> 1) in the VAE form: 1460x at N = 1024) cannot be reproduced to 1e-5 by
    ANYTHING that stores y in float32 -- the fp64 formulas on the float32-rounded reference y are then off by 2e-5 -- and
    e32, one sample of that rounding, does not tell.  Decided from the fp64 reference alone: such a draw is not used."""
    kw = d["kw"]
    f = CR.layer_forward(d["sources"], d["w"], d["bias"], d["gamma"], d["beta"], **kw)
    dbn = R.act_bwd(f["bn"], d["dout"].astype(np.float64), CR.ACT[kw["post_act"]]).reshape(-1, f["bn"].shape[-1])
    xhat = ((f["s"] - f["mean"]) * f["rstd"]).reshape(dbn.shape)
    for t in (dbn, dbn * xhat):
        if np.abs(t).sum(0).max() > 2 * np.sqrt(t.shape[0]) * np.abs(t.sum(0)).max():
            return False
    return True


def _variant_kw(variant):
    """variant: None, a condition regime of conv_layer_ref.COND_REGIMES, or "dy_mean1" (dout with a per-channel mean of ~1)"""
    if variant is None:
        return {}
    return {"dout_mean": 1.0} if variant == "dy_mean1" else {"cond_regime": variant}


@functools.lru_cache(maxsize=None)
def _data(path, idx, form, regime_off=None, variant=None):
    c = _case(path, idx)
    seed = ORDER.index(path) * 10 + (9 if idx == "big" else idx)
    d = CR.make_case(c["B"], c["S"], c["src"], c["Cout"], c["taps"], form, c["aff"], seed, regime_off, **_variant_kw(variant))
    while c["Cout"] <= 4 and form != "plain" and regime_off in (None, "ratio30") and not _well_conditioned(d):
        seed += 100
        d = CR.make_case(c["B"], c["S"], c["src"], c["Cout"], c["taps"], form, c["aff"], seed, regime_off)
    return d


@functools.lru_cache(maxsize=None)
def _reference(path, idx, form, regime_off=None, variant=None):
    """fp64 forward and backward (own decisions) and e32 per tensor, computed once per case, form and regime"""
    d = _data(path, idx, form, regime_off, variant)
    args = (d["sources"], d["w"], d["bias"], d["gamma"], d["beta"])
    f64 = CR.layer_forward(*args, **d["kw"])
    b64 = CR.layer_backward(f64, d["sources"], d["w"], d["gamma"], d["dout"], **d["kw"])
    f32 = CR.layer_forward(*args, dtype=np.float32, **d["kw"])
    # e32 is rounding alone: the float32 evaluation takes the fp64 reference's activation decisions (its own differ at a
    # few voxels next to a kink, most at mean/std = 30, and one flipped voxel is worth 1e-3 of a small tensor)
    b32 = CR.layer_backward(f32, d["sources"], d["w"], d["gamma"], d["dout"], kink_y=f64["y"], kink_bn=f64.get("bn"), **d["kw"])
    linear = bool(d["kw"]["pre_act"]) and bool((f64["y"] > 0).all())
    e32 = {k: _rel_grad(k, b32, b64, d["kw"], linear) for k in b64 if k not in ("dx", "pinned")}
    for i in range(len(b64["dx"])):
        if b64["dx"][i] is not None:
            e32["dx%d" % i] = _rel(b32["dx"][i], b64["dx"][i])
    if path in COND_PATHS:
        e32.update(CR.row_group_errors(b32["dw"], b64["dw"], d["sources"], d["kw"], linear))
    return f64, b64, e32, linear


@contextlib.contextmanager
def _env(names):
    """the switches are read when a handle is made: set around one call of an op"""
    added = [n for n in names if n not in os.environ]
    for n in added:
        os.environ[n] = "1"
    try:
        yield
    finally:
        for n in added:
            del os.environ[n]


def _run(path, idx, form, max_batch=None, regime_off=None, backward=True, variant=None):
    from icsg3d_amd import engine as E
    c = _case(path, idx)
    d = _data(path, idx, form, regime_off, variant)
    with _env(c["env"]):
        return E.conv_layer(d["sources"], d["w"], d["bias"], d["gamma"], d["beta"], dout=d["dout"] if backward else None,
                            pad_input=c["pad"], max_batch=max_batch, **d["kw"])


def _check_ids(got, want, what, plain=False):
    """plain: the same kernels in their no-affine instantiation (first template parameter of the Winograd kernels)"""
    for site in ("fwd", "dgrad", "wgrad"):
        if want[site] is None:
            continue
        assert len(got[site]) == len(want[site]), (what, site, got[site])
        for line, frag in zip(got[site], want[site]):
            kid = line.split("|", 1)[1]
            if hasattr(frag, "search"):
                assert frag.search(kid), (what, site, line, frag.pattern)
            else:
                assert (frag.replace("<true", "<false") if plain else frag) in kid, (what, site, line, frag)


def _check_y(r, f64, S, what):
    y, ref = r["y"], f64["y"]
    bm = CR.border_mask(S)
    for name, m in (("border", bm), ("interior", ~bm)):
        if m.any():
            e = _rel(y[:, m], ref[:, m])
            _note("y " + name, e, TOL)
            assert e <= TOL, (what, name, e)


def _check_stats(r, d, what, regime_off=None, show=False):
    """the statistics epilogue + bn_finalize against fp64 statistics of the op's OWN stored y, per channel"""
    y = r["y"]
    Cout = y.shape[-1]
    m64, v64 = CR.channel_stats(y)
    std = np.sqrt(v64)
    mu = CR.ulps32(r["mean"], m64, at=np.maximum(np.abs(m64), std))
    vpe = 1.0 / r["rstd"].astype(np.float64) ** 2
    ve = CR.var_error(vpe, v64)
    bound = CR.var_bound(m64, v64)
    if show:
        for c in range(min(Cout, 7)):
            print("  %s ch %d %-9s mean/std %9.3g  mean %.2f ulps  var+eps %.3g (bound %.3g)"
                  % (what, c, CR.regime_of(c, regime_off), abs(m64[c]) / max(std[c], 1e-300), mu[c], ve[c], bound[c]))
    _note("mean ulps", float(mu.max()), CR.MEAN_ULPS)
    _note("var+eps / bound", float((ve / bound).max()), 1.0)
    assert (mu <= CR.MEAN_ULPS).all(), (what, "mean", mu.max(), int(mu.argmax()))
    assert (ve <= bound).all(), (what, "var + eps", ve.max(), int((ve / bound).argmax()))
    assert (vpe >= CR.EPS * (1 - 2.0 ** -22)).all(), (what, "negative variance")
    flat = v64 == 0                      # constant and all-zero channels: by name where the regimes are set, and flat
    if regime_off is not None:
        names = ("constant", "dead") if d["kw"]["pre_act"] == 1 else ("constant",)     # "dead" is dead behind a ReLU only
        named = np.array([CR.regime_of(c, regime_off) in names for c in range(Cout)])
        assert (v64[named] == 0).all(), (what, "a constant channel is not stored constant", v64[named])
        flat = flat | named
    if flat.any():
        u = CR.ulps32(r["rstd"][flat], np.full(int(flat.sum()), 1.0 / np.sqrt(CR.EPS)))
        assert (u <= 2).all(), (what, "rstd of a constant channel", u.max())
    # the affine, in float32 from the op's own mean / rstd: one rounding per operation, the product fused or not
    sc = d["gamma"] * r["rstd"]
    u = CR.ulps32(r["scale"], sc)
    assert (u <= 1).all(), (what, "scale", u.max())
    prod = r["mean"].astype(np.float64) * r["scale"].astype(np.float64)
    sh = d["beta"].astype(np.float64) - prod
    u = CR.ulps32(r["shift"], sh, at=np.maximum(np.abs(sh), np.maximum(np.abs(prod), np.abs(d["beta"]))))
    assert (u <= 1).all(), (what, "shift", u.max())
    # moving statistics after one update from (0, 1): bn_moving_update in float32, the momentum as the kernel holds it
    n = y.size // Cout
    var32 = (vpe - CR.EPS).astype(np.float32)
    mm, mv = R.bn_moving_update(np.zeros(Cout, np.float32), np.ones(Cout, np.float32), r["mean"], var32, n,
                                momentum=np.float32(0.99))
    um = CR.ulps32(r["moving_mean"], mm)
    uv = CR.ulps32(r["moving_var"], mv)
    # the op hands out rstd, not the variance: var + eps = 1 / rstd^2 is known only to the rounding of rstd (half an ulp,
    # 2^-24 relative; twice that in the square).  That uncertainty of the REFERENCE's input, carried through the update
    # (d moving_var / d var = 0.01 n / (n - 1 - eps)), is added to the 2 ulps: 0.02 ulps where var ~ 1, up to 2 where
    # 0.01 var >> 0.99 (the 1e4 regime)
    dvar = (1.0 - float(np.float32(0.99))) * n / (n - (1.0 + CR.EPS)) * vpe * 2.0 ** -23
    lim_v = 2 + dvar / np.spacing(np.abs(mv).astype(np.float32)).astype(np.float64)
    _note("moving_mean ulps", float(um.max()), 2)
    _note("moving_var ulps", float((uv / lim_v).max() * 2), 2)
    assert (um <= 2).all() and (uv <= lim_v).all(), (what, "moving", um.max(), uv.max(), int((uv / lim_v).argmax()))
    assert r["blocks"] >= 1 and (r["rows_per_block"] == 0 or (n + r["rows_per_block"] - 1) // r["rows_per_block"] == r["blocks"])


def _check_grads(r, d, ref, what):
    f64, b64, e32, linear = ref
    kw = d["kw"]
    kink_bn = None
    if kw["has_bn"]:
        kink_bn = (r["y"].astype(np.float64) * r["scale"].astype(np.float64) + r["shift"].astype(np.float64)).astype(np.float32)
    own_y = (r["y"] > 0) == (f64["y"] > 0) if kw["pre_act"] else True
    own_bn = (kink_bn > 0) == (f64["bn"] > 0) if (kw["has_bn"] and kw["post_act"]) else True
    if np.all(own_y) and np.all(own_bn):
        b, pinned = b64, 0
    else:
        b = CR.layer_backward(f64, d["sources"], d["w"], d["gamma"], d["dout"], kink_y=r["y"], kink_bn=kink_bn, **kw)
        pinned = b["pinned"]
    print("  %s: %d pinned activation decisions" % (what, pinned))
    assert pinned <= 8, (what, pinned)
    pairs = [(k, _rel_grad(k, r, b, kw, linear)) for k in ("dw", "dbias", "dgamma", "dbeta") if k in b]
    pairs += [("dx%d" % i, _rel(r["dx"][i], b["dx"][i])) for i in range(len(b["dx"])) if b["dx"][i] is not None]
    if len(d["sources"]) == 2 and d["sources"][1].get("bcast"):
        # the x rows and the condition rows come from different kernels and differ in scale: each on its own, and inside
        # the condition rows the centre tap (the whole-sample totals) apart from the 26 others
        pairs += sorted(CR.row_group_errors(r["dw"], b["dw"], d["sources"], kw, linear).items())
    for k, e in pairs:
        lim = max(TOL, 2 * e32[k])
        print("  %s %-6s engine %.3g  e32 %.3g" % (what, k, e, e32[k]))
        _note("grad " + k, e, lim)
        assert e <= lim, (what, k, e, e32[k])


def _full(path, idx, form, ids, what, max_batch=None, regime_off=None, variant=None):
    c = _case(path, idx)
    d = _data(path, idx, form, regime_off, variant)
    ref = _reference(path, idx, form, regime_off, variant)
    r = _run(path, idx, form, max_batch=max_batch, regime_off=regime_off, variant=variant)
    _check_ids(r["kernels"], ids, what)
    _check_y(r, ref[0], c["S"], what)
    _check_stats(r, d, what, regime_off=regime_off)
    _check_grads(r, d, ref, what)
    return r


def _ids(path, idx, env=None, plain=False):
    p = PATHS[path]
    if "ids_fn" in p:
        return p["ids_fn"](idx, env, plain)
    if env is not None:
        return p["env"][env]
    return p.get("ids_by_case", {}).get(idx, p["ids"])


# the cases of a path that launch another forward kernel than its first: each has a statistics epilogue of its own
REGIME_CASES = [(p, i) for p, d in PATHS.items() for i in d.get("regimes", (0,))]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("path,idx", ALL, ids=lambda v: str(v))
def test_layer_matches_reference(path, idx, form):
    _full(path, idx, form, _ids(path, idx), "%s[%d] %s" % (path, idx, form))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("path,env", ALL_ENV, ids=lambda v: str(v))
def test_layer_under_switch(path, env, form, monkeypatch):
    """the same cases with the path's fast kernel switched off (or forced): the general kernels' loaders and epilogues"""
    for idx in range(len(PATHS[path]["cases"])):
        base = _run(path, idx, form) if env in PATHS[path].get("must_differ", ()) else None
        monkeypatch.setenv(env, "1")
        ids = _ids(path, idx, env)
        if env == "ICSG3D_NO_THIN1_2STAGE" and PATHS[path]["cases"][idx]["Cout"] != 1:
            ids = _ids(path, idx)
        if env == "ICSG3D_NO_THIN_C" and PATHS[path]["cases"][idx]["src"][0][0] != 1:
            ids = _ids(path, idx)
        r = _full(path, idx, form, ids, "%s[%d] %s %s" % (path, idx, form, env))
        monkeypatch.delenv(env)
        if base is not None:
            assert not np.array_equal(base["y"], r["y"]), (path, env, "the switch did not change the summation")
            if PATHS[path].get("differ_dw"):
                assert not np.array_equal(base["dw"], r["dw"]), (path, env, "the switch did not change backward-weight")


@pytest.mark.parametrize("path,idx", ALL, ids=lambda v: str(v))
def test_plain_form_equals_single_op_entry_points(path, idx, monkeypatch):
    """has_bn = 0, plain sources, against ics_op_conv3d_forward / _backward.  Those two run conv_forward / conv_backward on
    the same one-layer handle with split-K off, so under ICSG3D_NO_FWD_SPLITK the train-step form and the old entry points
    are the same launches: the same kernels in the same instantiation, the same bits.  An upsampled source has no
    counterpart there.  Three comparisons are to the reference only, as before the old entry points went through the handle
    (they then handed the launchers no workspace): the two-stage single-channel kernels (forward at Cout = 1, backward-data
    at Cin = 1), and backward-weight of a padded thin single-channel input, which the old entry points never pad."""
    from icsg3d_amd import engine as E
    c = _case(path, idx)
    d = _data(path, idx, "plain")
    monkeypatch.setenv("ICSG3D_NO_FWD_SPLITK", "1")
    r = _run(path, idx, "plain")
    _check_ids(r["kernels"], _ids(path, idx, plain=True), "%s[%d] plain" % (path, idx), plain=True)
    f64 = CR.layer_forward(d["sources"], d["w"], d["bias"], **d["kw"])
    _check_y(r, f64, c["S"], "%s[%d] plain" % (path, idx))
    b64 = CR.layer_backward(f64, d["sources"], d["w"], None, d["dout"], **d["kw"])
    assert _rel(r["dw"], b64["dw"]) <= TOL and _rel(r["dbias"], b64["dbias"]) <= TOL
    for got, want in zip(r["dx"], b64["dx"]):
        assert want is None or _rel(got, want) <= TOL
    if any(s[1] for s in c["src"]) or path in COND_PATHS:     # (a condition source has no counterpart there either)
        return
    x = d["sources"][0]["x"]
    with _env(c["env"]):
        y = E.conv3d_forward(x, d["w"], d["bias"], pre_act=0)
        dx, dw = E.conv3d_backward(x, d["w"], d["dout"])
    if c["Cout"] != 1:
        assert np.array_equal(y, r["y"]), (path, idx, "forward bits differ from ics_op_conv3d_forward")
    if c["src"][0][0] != 1:
        assert np.array_equal(dx, r["dx"][0]), (path, idx, "backward-data bits differ from ics_op_conv3d_backward")
    if not (c["pad"] and c["src"][0][0] == 1):      # 4 channels are their own padded width: nothing is padded
        assert np.array_equal(dw, r["dw"]), (path, idx, "backward-weight bits differ from ics_op_conv3d_backward")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("path", list(PATHS))
def test_handle_larger_than_batch_with_canaries(path, form, monkeypatch):
    """(B, max_batch) = (3, 5) -- (3, 7) on the 16- and 32-channel outputs: every workspace is sized for max_batch, the step
    runs 3 samples, the guard bytes behind every buffer stay clean (the op fails by name otherwise)."""
    monkeypatch.setenv("ICSG3D_DEBUG_CANARY", "1")
    big = 7 if _case(path, "big")["Cout"] in (16, 32) else 5
    _full(path, "big", form, _ids(path, _big_idx(path)), "%s B=3 max_batch=%d %s" % (path, big, form), max_batch=big)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("path,idx", REGIME_CASES, ids=lambda v: str(v))
def test_statistics_in_every_value_regime(path, idx, form):
    """forward and statistics only: channel c of one launch sits in regime (c + off) % 7 -- mean/std ~ 0, 30, 1000, a constant
    channel, an all-zero channel behind ReLU (mean/std = 1000 without), std 1e-4 around 1.0, magnitudes of 1e4.  A layer
    with fewer than seven output channels is launched until every regime has been through it (Cout = 1: seven times)."""
    c = _case(path, idx)
    for off in range(0, 7, min(c["Cout"], 7)):
        d = _data(path, idx, form, off)
        r = _run(path, idx, form, regime_off=off, backward=False)
        what = "%s[%d] regimes+%d %s" % (path, idx, off, form)
        _check_ids(r["kernels"], dict(_ids(path, idx), dgrad=None, wgrad=None), what)
        f64 = CR.layer_forward(d["sources"], d["w"], d["bias"], d["gamma"], d["beta"], **d["kw"])
        # y per channel: the regimes differ by 1e8 in magnitude, a tensor-relative bound would only see the largest
        for ch in range(c["Cout"]):
            ref = f64["y"][..., ch]
            scale = max(np.abs(ref).max(), 1e-30)
            assert np.abs(r["y"][..., ch] - ref).max() <= TOL * scale, (what, ch, CR.regime_of(ch, off))
        _check_stats(r, d, what, regime_off=off, show=True)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("path,idx", REGIME_CASES, ids=lambda v: str(v))
def test_gradients_at_mean_over_std_30(path, idx, form):
    """forward, statistics AND backward with every output channel at mean/std ~ 30 (bias 30, conv part of std ~ 1): the
    c1 / c2 sums of BatchNorm backward, dgamma / dbeta and the inputs of backward-weight cancel there.  Same bounds, same
    pinned decisions and e32 as in the ordinary regime; behind the U-Net form's ReLU every voxel is open."""
    _full(path, idx, form, _ids(path, idx), "%s[%d] mean/std 30 %s" % (path, idx, form), regime_off="ratio30")


# ---- condition sources: the regimes only they have.  One case per route: the B = 3 one of each path
COND_ROUTES = [("cond_fold", None), ("cond_fold", "ICSG3D_NO_COND_FOLD"), ("cond_fold", "ICSG3D_NO_THIN_C"), ("cond_bcast", None)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("regime", CR.COND_REGIMES)
@pytest.mark.parametrize("path,env", COND_ROUTES, ids=lambda v: str(v))
def test_condition_regimes(path, env, regime, form, monkeypatch):
    """every sample the same condition (behind BatchNorm the centre tap's condition rows are then exactly zero: see
    conv_layer_ref.row_group_errors), one sample's condition all zero, conditions of 1e3 next to x of 1 (y nearly constant per
    sample and border class: the mean >> std statistics bounds apply unchanged; the condition rows of dw are 1e3 x the x
    rows, which only the per-group comparison sees).  Every check of the file, ids included."""
    if env:
        monkeypatch.setenv(env, "1")
    idx = _big_idx(path)
    _full(path, idx, form, _ids(path, idx, env), "%s[%d] %s cond %s %s" % (path, idx, env, regime, form), variant=regime)


@pytest.mark.parametrize("path,env", COND_ROUTES, ids=lambda v: str(v))
def test_condition_without_batchnorm(path, env, monkeypatch):
    """has_bn = 0 and dout = dy with a per-channel mean of ~1: the per-sample totals and the interior = total - border sums
    of cond_wgrad_kernel without BatchNorm's zero sum.  No engine runs e0 this way; it is the only regime in which the region
    sums do not cancel over the batch.  Every case of the path."""
    if env:
        monkeypatch.setenv(env, "1")
    for idx in range(len(PATHS[path]["cases"])):
        what = "%s[%d] %s no BatchNorm, mean(dy) ~ 1" % (path, idx, env)
        d = _data(path, idx, "plain", None, "dy_mean1")
        ref = _reference(path, idx, "plain", None, "dy_mean1")
        r = _run(path, idx, "plain", variant="dy_mean1")
        _check_ids(r["kernels"], _ids(path, idx, env), what, plain=True)
        _check_y(r, ref[0], _case(path, idx)["S"], what)
        _check_grads(r, d, ref, what)


def test_zz_report_worst_gaps():
    """prints the worst (engine error, yardstick) pairs of this run: the source of the MEASURED table in the header"""
    for k in sorted(WORST):
        print("  %-16s %.3g  (of %.3g)" % (k, WORST[k][0], WORST[k][1]))
