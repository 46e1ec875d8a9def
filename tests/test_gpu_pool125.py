"""The pooling pass of the 125-product up-split backward (icsg3d_amd/csrc/up125.hip), both kernels: pool125_kernel (one
wave per z type, `variant 0`, ICSG3D_POOL125_V1 in the engine) and pool125_planes_kernel (one wave per fine plane, every
plane of a tile's 6x6x6 window loaded, x-transformed and (y, x)-accumulated once, the z combination last through LDS;
`variant 1`, the engine's default).

1. Exactness, through ics_op_up125_pool on integer dy in [-8, 8] (every sum is exact in fp32): variant 1 equals variant 0
   bit for bit, and both equal the numpy definition  sum coef(tz,fz) coef(ty,fy) coef(tx,fx) dy  (test_up125_host.COEF).
   Shapes (B, S, N): (2, 8, 32) eight tiles per wave, every tile on a border of every axis; (1, 16, 64) interior tiles on
   every axis; (3, 8, 256) one tile per wave, sample boundaries; (1, 8, 512) two channel groups in blockIdx.y.  (A wave
   covers 64 >> lgc <= 8 whole tiles and B (S/4)^3 is a multiple of 8: no launch has a partial group of tiles.)
2. General data, float dy ~ N(0, 1) at (2, 8, 128) and (1, 16, 64): variant 1 against the definition in fp64.  Bound per
   element, none excluded: 64 * 2^-24 * sum |coef dy| over its at most 64 samples -- at most 63 additions, one rounding
   of at most 2^-24 relative each, each partial sum at most sum |coef dy| in magnitude.
3. Through the layer under ICSG3D_FORCE_UP125: the four CASES of tests/test_gpu_up125.py (imported) through
   test_gpu_conv_layer._check_grads with the new kernel, bound max(1e-5, 2 e32) as there; the max_batch 5 case also under
   ICSG3D_DEBUG_CANARY and under ICSG3D_POOL125_V1 (the old kernel; the launch site's label is "pool125:<layer>" for
   both, so which kernel ran does not show in the rows -- part 1 holds the two kernels against each other directly),
   whose gradients equal the new kernel's within the same bound; the forward output is bit-identical in all three runs.
4. Refusals: S = 4, N = 48, N = 16 return an error and launch nothing."""
import functools

import numpy as np
import pytest

import test_gpu_conv_layer as T
import test_gpu_up125 as U
import test_up125_host as H

pytestmark = pytest.mark.gpu

EXACT = [(2, 8, 32), (1, 16, 64), (3, 8, 256), (1, 8, 512)]
GENERAL = [(2, 8, 128), (1, 16, 64)]
FORCE = U.FORCE
V1 = ("ICSG3D_POOL125_V1",)


def _definition(dy, coef):
    """the 125 blocks in the layout of up125.h from dy (B,S,S,S,N), in fp64; coef: H.COEF or its magnitudes"""
    B, S, N = dy.shape[0], dy.shape[1], dy.shape[4]
    Tn = S // 4
    rows = B * Tn ** 3
    p = np.zeros((B, S + 2, S + 2, S + 2, N), np.float64)
    p[:, 1:-1, 1:-1, 1:-1] = dy
    idx = 4 * np.arange(Tn)[:, None] + np.arange(6)[None, :]          # padded coordinate of sample f of tile j
    win = p[:, idx[:, :, None, None, None, None], idx[None, None, :, :, None, None], idx[None, None, None, None, :, :]]
    c = coef.astype(np.float64)                                        # win: (B, jz, fz, jy, fy, jx, fx, N)
    blocks = np.einsum("af,bg,ch,nzfygxhk->nzyxabck", c, c, c, win, optimize=True).reshape(rows, 5, 5, 5, N)
    out = np.empty(125 * rows * N, np.float64)
    for tz, ty, tx in H.TYPES:
        q = H.class_of(tz, ty, tx)
        v = out[H.bbase(q) * rows * N:(H.bbase(q) + H.nb(q)) * rows * N].reshape(rows, H.nb(q), N)
        v[:, H.block(q, tz, ty, tx)] = blocks[:, tz, ty, tx]
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("shape", EXACT, ids=lambda s: "%d-%d-%d" % s)
def test_exact_on_integers(shape):
    from icsg3d_amd import engine as E
    B, S, N = shape
    dy = np.random.Generator(np.random.PCG64(1250 + S + N)).integers(-8, 9, (B, S, S, S, N)).astype(np.float32)
    ref = _definition(dy, H.COEF)
    assert np.abs(ref).max() <= 64 * 8                     # integers far below 2^24: exact in fp32
    old, new = E.up125_pool(dy, 0), E.up125_pool(dy, 1)
    assert old.shape == new.shape == ref.shape
    print("  %s: variant 0 differs from the definition at %d, variant 1 at %d, from each other (bits) at %d of %d" %
          (shape, int((old != ref).sum()), int((new != ref).sum()), int((_bits(old) != _bits(new)).sum()), ref.size))
    assert np.array_equal(old.astype(np.float64), ref), shape
    assert np.array_equal(new.astype(np.float64), ref), shape
    assert np.array_equal(_bits(new), _bits(old)), shape


@pytest.mark.parametrize("shape", GENERAL, ids=lambda s: "%d-%d-%d" % s)
def test_general_data(shape):
    from icsg3d_amd import engine as E
    B, S, N = shape
    dy = np.random.Generator(np.random.PCG64(77 + S + N)).standard_normal((B, S, S, S, N)).astype(np.float32)
    ref = _definition(dy, H.COEF)
    bound = 64 * 2.0 ** -24 * _definition(np.abs(dy), np.abs(H.COEF))
    err = np.abs(E.up125_pool(dy, 1).astype(np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("  %s: largest error / bound %.3g, largest error %.3g" % (shape, worst, float(err.max())))
    assert np.all(err <= bound), (shape, worst)


@pytest.mark.parametrize("c", U.CASES, ids=U._name)
def test_layer_against_fp64(c):
    what = U._name(c)
    new = U._run(c, FORCE)
    U._took_up125(new, what)
    T._check_grads(new, U._data(c), U._reference(c), what)


def test_layer_canary_and_old_kernel():
    c = U.CASES[3]
    assert c[:2] == (3, 16) and c[3:] == (64, 5)
    what = U._name(c)
    e32 = U._reference(c)[2]
    new = U._run(c, FORCE)
    guarded = U._run(c, ("ICSG3D_DEBUG_CANARY",) + FORCE)     # the op fails if a guard behind any buffer is written
    old = U._run(c, FORCE + V1)
    for r in (new, guarded, old):
        U._took_up125(r, what)
    T._check_grads(guarded, U._data(c), U._reference(c), what + " canary")
    T._check_grads(old, U._data(c), U._reference(c), what + " v1")
    assert np.array_equal(_bits(guarded["y"]), _bits(new["y"])) and np.array_equal(_bits(old["y"]), _bits(new["y"])), what
    pairs = [(k, T._rel(old[k], new[k])) for k in U.GRADS]
    pairs += [("dx%d" % i, T._rel(a, b)) for i, (a, b) in enumerate(zip(old["dx"], new["dx"]))]
    for k, e in pairs:
        print("  %s %-6s old pooling kernel against new %.3g  e32 %.3g" % (what, k, e, e32[k]))
    for k, e in pairs:
        assert e <= max(T.TOL, 2 * e32[k]), (what, k, e)


@pytest.mark.parametrize("shape", [(1, 4, 32), (1, 8, 48), (1, 8, 16)], ids=lambda s: "%d-%d-%d" % s)
def test_refusals(shape):
    from icsg3d_amd import _lib
    from icsg3d_amd import engine as E
    lib = _lib.load()
    B, S, N = shape
    dy = np.zeros((B, S, S, S, N), np.float32)
    for variant in (0, 1):
        before = lib.ics_kernel_launches()
        with pytest.raises(_lib.IcsError):
            E.up125_pool(dy, variant)
        assert lib.ics_kernel_launches() == before, shape
