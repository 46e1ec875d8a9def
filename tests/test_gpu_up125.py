"""The 125-product form of the up-split backward (icsg3d_amd/csrc/up125.h: pool125_kernel, the z-batched class GEMMs both
ways, the x-class, combine and contraction kernels) against the fp64 reference of tests/conv_layer_ref.py, one layer at a
time through engine.conv_layer under ICSG3D_FORCE_UP125 (the default predicate asks for Cout and Cu multiples of 128 and
2048 tile rows B (S/4)^3; the switch engages the form wherever its layout serves).

The form is a reassociation: 125 block products per 2x2x2 coarse tile instead of 216, with +-1 coefficients only
(tests/test_up125_host.py).  Every gradient -- dw, dbias, dgamma, dbeta and every dx -- is held to the per-tensor bound of
tests/test_gpu_conv_layer.py, max(1e-5, 2 e32), e32 the error of an fp32 run of the reference itself.

Shapes, (B, S, sources, Cout):
  (2, 8, [64 | up 128], 128)   two tiles per axis: every tile touches a border on every axis
  (1, 16, up 64, 64)           no skip channels
  (3, 16, [32 | up 64], 32)    sample boundaries, 192 tile rows, partial GEMM tiles
  (3, 16, [32 | up 64], 64)    max_batch 5, under ICSG3D_DEBUG_CANARY: the scratch set laid out for the batch at hand
The default predicate: (4, 32, [64 | up 128], 128), the smallest shape it accepts, against the same call under
ICSG3D_NO_UP125 (an fp64 reference would take minutes on the host at that size): 1e-5 tensor-relative per gradient, the
forward output bit for bit."""
import functools

import numpy as np
import pytest

import conv_layer_ref as CR
import test_gpu_conv_layer as T

pytestmark = pytest.mark.gpu

SKIP32, SKIP64, UP64 = ((32, 0), (64, 1)), ((64, 0), (128, 1)), ((64, 1),)
#        B, S, sources, Cout, max_batch
CASES = [(2, 8, SKIP64, 128, None), (1, 16, UP64, 64, None), (3, 16, SKIP32, 32, None), (3, 16, SKIP32, 64, 5)]
DEFAULT = (4, 32, SKIP64, 128, None)
GRADS = ("dw", "dbias", "dgamma", "dbeta")
FORCE = ("ICSG3D_FORCE_UP125",)


def _name(c):
    return "%d-%d-%s-%d%s" % (c[0], c[1], "+".join("%s%d" % ("up" if u else "", n) for n, u in c[2]), c[3],
                              "-max%d" % c[4] if c[4] else "")


@functools.lru_cache(maxsize=None)
def _data(c):
    B, S, src, Cout, _ = c
    return CR.make_case(B, S, src, Cout, 27, "unet", True, seed=900 + 10 * B + S + Cout)


@functools.lru_cache(maxsize=None)
def _reference(c):
    """fp64 forward and backward and e32 per tensor, as test_gpu_conv_layer._reference"""
    d = _data(c)
    args = (d["sources"], d["w"], d["bias"], d["gamma"], d["beta"])
    f64 = CR.layer_forward(*args, **d["kw"])
    b64 = CR.layer_backward(f64, d["sources"], d["w"], d["gamma"], d["dout"], **d["kw"])
    f32 = CR.layer_forward(*args, dtype=np.float32, **d["kw"])
    b32 = CR.layer_backward(f32, d["sources"], d["w"], d["gamma"], d["dout"], kink_y=f64["y"], kink_bn=f64.get("bn"), **d["kw"])
    linear = bool(d["kw"]["pre_act"]) and bool((f64["y"] > 0).all())
    e32 = {k: T._rel_grad(k, b32, b64, d["kw"], linear) for k in b64 if k not in ("dx", "pinned")}
    for i in range(len(b64["dx"])):
        e32["dx%d" % i] = T._rel(b32["dx"][i], b64["dx"][i])
    return f64, b64, e32, linear


def _run(c, env=()):
    from icsg3d_amd import engine as E
    d = _data(c)
    with T._env(env):
        return E.conv_layer(d["sources"], d["w"], d["bias"], d["gamma"], d["beta"], dout=d["dout"], max_batch=c[4], **d["kw"])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _up_sites(r):
    return ([ln for ln in r["kernels"]["dgrad"] if ".up|" in ln], [ln for ln in r["kernels"]["wgrad"] if ".up|" in ln])


def _took_up125(r, what):
    assert len(r["kernels"]["pool"]) == 1 and r["kernels"]["pool"][0].startswith("pool125:"), (what, r["kernels"]["pool"])
    dg, wg = _up_sites(r)
    assert len(dg) == 1 and "conv_fwd_kernel<" in dg[0] and dg[0].endswith("UP125"), (what, dg)
    assert len(wg) == 1 and "conv_wgrad_kernel<" in wg[0] and "ZB>" in wg[0] and wg[0].endswith("UP125"), (what, wg)


def _took_up8(r, what):
    assert len(r["kernels"]["pool"]) == 1 and r["kernels"]["pool"][0].startswith("pool8:"), (what, r["kernels"]["pool"])
    dg, wg = _up_sites(r)
    assert len(dg) == 1 and "UP8" in dg[0] and "UP125" not in dg[0], (what, dg)
    assert len(wg) == 1 and "UP8" in wg[0] and "UP125" not in wg[0], (what, wg)


@pytest.mark.parametrize("c", CASES, ids=_name)
def test_up125_against_fp64(c):
    what = _name(c)
    canary = ("ICSG3D_DEBUG_CANARY",) if c[4] else ()     # the op fails if a guard behind any buffer is written
    new = _run(c, canary + FORCE)
    _took_up125(new, what)
    T._check_grads(new, _data(c), _reference(c), what)


@pytest.mark.parametrize("c", CASES[:1] + CASES[3:], ids=_name)
def test_switches(c):
    """ICSG3D_NO_UP125 wins over the force switch; without either, these small shapes stay on pool8"""
    what = _name(c)
    off = _run(c, FORCE + ("ICSG3D_NO_UP125",))
    _took_up8(off, what)
    plain = _run(c)
    _took_up8(plain, what)
    for k in GRADS:
        assert np.array_equal(_bits(off[k]), _bits(plain[k])), (what, k)
    new = _run(c, FORCE)
    assert np.array_equal(_bits(new["y"]), _bits(plain["y"])), what     # the forward pass is untouched


def test_default_predicate():
    c = DEFAULT
    what = _name(c)
    new, old = _run(c), _run(c, ("ICSG3D_NO_UP125",))
    _took_up125(new, what)
    _took_up8(old, what)
    assert np.array_equal(_bits(new["y"]), _bits(old["y"])), what
    pairs = [(k, T._rel(new[k], old[k])) for k in GRADS]
    assert len(new["dx"]) == len(old["dx"]) == 2
    pairs += [("dx%d" % i, T._rel(a, b)) for i, (a, b) in enumerate(zip(new["dx"], old["dx"]))]
    for k, e in pairs:
        print("  %s %-6s up125 against up8 %.3g" % (what, k, e))
    for k, e in pairs:
        assert e <= 1e-5, (what, k, e)
