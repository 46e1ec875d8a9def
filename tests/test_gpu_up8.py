"""The up-split backward over the 8 pooled volumes of dy (icsg3d_amd/csrc/up8.h: pool8_kernel and the UP8 loaders of the
two coarse-grid GEMMs) against the same call over pool27's 27 tap copies (ICSG3D_NO_UP8=1) and against the fp64
reference of tests/conv_layer_ref.py, one layer at a time through engine.conv_layer.

The 8 volumes hold the same floats as the tap copies (tests/test_up8_host.py), the GEMMs keep their tiles, split-K plans
and K order, so the same products are added in the same order: every gradient is required EQUAL BIT FOR BIT to the tap-copy
path's, and within the per-tensor bound of tests/test_gpu_conv_layer.py (max(1e-5, 2 e32)) of the fp64 reference.

Shapes: the smallest at which each piece of the address logic can go wrong --
  (2, 8)            Sh = 4: a 32-row chunk spans two z planes, a 64-row sample ends inside a 128-row tile
  (1, 16), (3, 16)  a chunk is two x lines; B = 3 has sample boundaries
  Cout 32, 64, 128  tap boundaries inside a backward-weight N tile (32, 64) and between tiles (128); 27 * 32 = 864 columns
                    leave a partial last N tile
  sources           [32 | up 64], [64 | up 128], up-only 64
  max_batch 5, B 3  volumes laid out for the batch at hand inside an allocation for 5, under ICSG3D_DEBUG_CANARY=1
Layers the layout does not serve keep pool27 in both runs: (3, 4, up 64 -> 32) (S = 4) and (2, 8, up 32 -> 16) (Cout = 16).
LARGE: the 128 x 64 and 128 x 128 backward-data tiles at the smallest batch that picks them, and an up-192 layer whose
96-wide tile has no UP8 form (see there)."""
import functools

import numpy as np
import pytest

import conv_layer_ref as CR
import test_gpu_conv_layer as T

pytestmark = pytest.mark.gpu

SKIP32, SKIP64, UP64 = ((32, 0), (64, 1)), ((64, 0), (128, 1)), ((64, 1),)
#        B, S, sources, Cout, max_batch
CASES = [(2, 8, SKIP32, 64, None), (2, 8, SKIP64, 128, None), (2, 8, UP64, 32, None),
         (1, 16, SKIP64, 128, None), (1, 16, UP64, 64, None), (1, 16, SKIP32, 32, None),
         (3, 16, SKIP32, 32, None), (3, 16, UP64, 128, None), (3, 16, SKIP32, 64, 5)]
FALLBACK = [(3, 4, UP64, 32, None), (2, 8, ((32, 1),), 16, None)]
GRADS = ("dw", "dbias", "dgamma", "dbeta")


def _name(c):
    return "%d-%d-%s-%d%s" % (c[0], c[1], "+".join("%s%d" % ("up" if u else "", n) for n, u in c[2]), c[3],
                              "-max%d" % c[4] if c[4] else "")


@functools.lru_cache(maxsize=None)
def _data(c):
    B, S, src, Cout, _ = c
    return CR.make_case(B, S, src, Cout, 27, "unet", True, seed=700 + 10 * B + S + Cout)


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


def _same_bits(new, old, what):
    for k in GRADS:
        assert np.array_equal(_bits(new[k]), _bits(old[k])), (what, k, T._rel(new[k], old[k]))
    assert len(new["dx"]) == len(old["dx"])
    for i, (a, b) in enumerate(zip(new["dx"], old["dx"])):      # dA_skip where there is one, and dxl
        assert np.array_equal(_bits(a), _bits(b)), (what, "dx%d" % i, T._rel(a, b))


def _up_sites(r):
    return ([ln for ln in r["kernels"]["dgrad"] if ".up|" in ln], [ln for ln in r["kernels"]["wgrad"] if ".up|" in ln])


@pytest.mark.parametrize("c", CASES, ids=_name)
def test_up8_equals_tap_copies_bit_for_bit(c):
    what = _name(c)
    canary = ("ICSG3D_DEBUG_CANARY",) if c[4] else ()     # the op fails if a guard behind any buffer is written
    new = _run(c, canary)
    old = _run(c, canary + ("ICSG3D_NO_UP8",))
    # the pooling each run took, and the loader variant (the UP8 mark in the kernel id) of the two coarse-grid GEMMs
    assert len(new["kernels"]["pool"]) == 1 and new["kernels"]["pool"][0].startswith("pool8:"), (what, new["kernels"]["pool"])
    assert len(old["kernels"]["pool"]) == 1 and old["kernels"]["pool"][0].startswith("pool27:"), (what, old["kernels"]["pool"])
    for r, up8 in ((new, True), (old, False)):
        dg, wg = _up_sites(r)
        assert len(dg) == 1 and "conv_fwd_kernel<" in dg[0] and ("UP8" in dg[0]) == up8, (what, dg)
        assert len(wg) == 1 and "conv_wgrad_kernel<" in wg[0] and ("UP8" in wg[0]) == up8, (what, wg)
    _same_bits(new, old, what)
    assert np.array_equal(_bits(new["y"]), _bits(old["y"])), what
    T._check_grads(new, _data(c), _reference(c), what)


# The backward-data GEMM picks its tile by the number of blocks: every shape above runs the 64 x 64 tile.  From
# B (S/2)^3 = 49152 coarse rows on it takes the 128-row tiles, 128 x 64 at Cu = 64 and 128 x 128 at Cu = 128 -- the smallest
# shapes that launch those two UP8 instantiations.  Cu = 192 takes the 96-wide tile from 24576 rows on, which has no UP8
# form: a handle that can run such a batch keeps pool27.  At these sizes an fp64 reference would take minutes on the
# host; the cases compare the two paths bit for bit (the reference bound is asserted at the small shapes above, on the
# same kernels' other tile).
LARGE = [((12, 32, UP64, 32, None), "conv_fwd_kernel<2, 2, 2, 1, ", True), ((12, 32, ((128, 1),), 32, None), "conv_fwd_kernel<2, 2, 2, 2, ", True),
         ((6, 32, ((192, 1),), 32, None), "conv_fwd_kernel<4, 1, 1, 3, ", False)]


@pytest.mark.parametrize("c,tile,up8", LARGE, ids=lambda v: _name(v) if isinstance(v, tuple) else None)
def test_large_tiles(c, tile, up8):
    what = _name(c)
    new, old = _run(c), _run(c, ("ICSG3D_NO_UP8",))
    assert len(new["kernels"]["pool"]) == 1 and new["kernels"]["pool"][0].startswith("pool8:" if up8 else "pool27:"), (what, new["kernels"]["pool"])
    assert len(old["kernels"]["pool"]) == 1 and old["kernels"]["pool"][0].startswith("pool27:"), (what, old["kernels"]["pool"])
    for r, want in ((new, up8), (old, False)):
        dg, wg = _up_sites(r)
        assert len(dg) == 1 and tile in dg[0] and ("UP8" in dg[0]) == want, (what, dg)
        assert len(wg) == 1 and "conv_wgrad_kernel<" in wg[0] and ("UP8" in wg[0]) == want, (what, wg)
    _same_bits(new, old, what)
    assert np.isfinite(new["dx"][0]).all() and np.abs(new["dx"][0]).max() > 0 and np.abs(new["dw"]).max() > 0, what


@pytest.mark.parametrize("c", FALLBACK, ids=_name)
def test_layers_outside_the_layout_keep_pool27(c):
    what = _name(c)
    new, old = _run(c), _run(c, ("ICSG3D_NO_UP8",))
    for r in (new, old):
        assert len(r["kernels"]["pool"]) == 1 and r["kernels"]["pool"][0].startswith("pool27:"), (what, r["kernels"]["pool"])
        dg, wg = _up_sites(r)
        assert dg and wg and not any("UP8" in ln for ln in dg + wg), (what, dg, wg)
    _same_bits(new, old, what)
    T._check_grads(new, _data(c), _reference(c), what)
