"""The 125-product form of the up-split backward (icsg3d_amd/csrc/up125.h) in numpy, without the library: the identities
against brute-force gradients of conv3(upsample(x)), and the layout arithmetic through a Python twin of the header
(hoststub/up125_check.cpp checks the header itself under the sanitizers).

Per axis, tile j covers the coarse pair (2j, 2j+1) and the fine samples f0..f5 = dy[4j-1 .. 4j+4] (0 outside the grid):

    D1 = f0+f1-f2-f3   R0 = f1+f2   Q1 = f2+f3   D2 = f2+f3-f4-f5   R1 = f3+f4
    dx[2j]   = wp D1 + (wp+wm) Q1 + wc R0            (wp / wc / wm: tap index 2 / 1 / 0, offsets +1 / 0 / -1)
    dx[2j+1] = (wp+wm) Q1 - wm D2 + wc R1
    dwp = xA D1 + xB Q1    dwc = xA R0 + xC R1    dwm = xB Q1 - xC D2,    xA = x[2j], xB = x[2j]+x[2j+1], xC = x[2j+1]

five products per axis for two outputs, 125 per 2x2x2 coarse tile in three dimensions where the 27-tap form does 216."""
import itertools

import numpy as np
import pytest

D1, R0, Q1, D2, R1 = range(5)
COEF = np.array([[1, 1, -1, -1, 0, 0], [0, 1, 1, 0, 0, 0], [0, 0, 1, 1, 0, 0], [0, 0, 1, 1, -1, -1], [0, 0, 0, 1, 1, 0]])
WCOEF = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 1], [-1, 0, 0], [0, 1, 0]])     # [type][tap index]
XCLS = np.array([[1, 0], [1, 1], [0, 1]])                                      # [class][x[2j], x[2j+1]]


# ---- twin of up125.h
def cls(t): return 0 if t < 2 else (1 if t == 2 else 2)
def eidx(t): return t if t < 2 else (0 if t == 2 else t - 3)
def nax(c): return 1 if c == 1 else 2
def n_b(q): return (q // 9 == 1) + ((q // 3) % 3 == 1) + (q % 3 == 1)
def nb(q): return 8 >> n_b(q)


SLOT0, BLOCK0, CLASSES = (0, 8, 20, 26), (0, 64, 112, 124), (8, 12, 6, 1)


def slot(q):
    g = n_b(q)
    return SLOT0[g] + sum(1 for p in range(q) if n_b(p) == g)


def bbase(q):
    g = n_b(q)
    return BLOCK0[g] + (slot(q) - SLOT0[g]) * (8 >> g)


def block(q, tz, ty, tx):
    return (eidx(tz) * nax((q // 3) % 3) + eidx(ty)) * nax(q % 3) + eidx(tx)


def class_of(tz, ty, tx):
    return cls(tz) * 9 + cls(ty) * 3 + cls(tx)


def pooled_off(rows, N, q, row, b, n):
    return (bbase(q) * rows + row * nb(q) + b) * N + n


def class_off(rows, Cu, q, row, c):
    return (slot(q) * rows + row) * Cu + c


TYPES = list(itertools.product(range(5), repeat=3))


def test_classes_and_slots():
    assert sorted(slot(q) for q in range(27)) == list(range(27))
    assert sum(nb(q) for q in range(27)) == 125
    for g in range(4):
        qs = [q for q in range(27) if n_b(q) == g]
        assert len(qs) == CLASSES[g] and [slot(q) for q in qs] == list(range(SLOT0[g], SLOT0[g] + CLASSES[g]))
        assert [bbase(q) for q in qs] == [BLOCK0[g] + z * (8 >> g) for z in range(len(qs))]     # uniform z strides
    per_class = {}
    for t in TYPES:
        per_class.setdefault(class_of(*t), []).append(block(class_of(*t), *t))
    assert all(sorted(v) == list(range(nb(q))) for q, v in per_class.items()) and len(per_class) == 27


@pytest.mark.parametrize("rows,N,Cu", [(16, 32, 64), (192, 32, 64), (24, 64, 128)])
def test_offsets_are_dense_and_disjoint(rows, N, Cu):
    hit = np.zeros(125 * rows * N // 4, np.int32)
    r = np.arange(rows)[:, None]
    n = np.arange(0, N, 4)[None, :]
    for t in TYPES:
        q = class_of(*t)
        off = pooled_off(rows, N, q, r, block(q, *t), n)
        assert (off % 4 == 0).all()
        np.add.at(hit, (off // 4).ravel(), 1)
    assert (hit == 1).all()
    hit = np.zeros(27 * rows * Cu, np.int32)
    c = np.arange(Cu)[None, :]
    for q in range(27):
        np.add.at(hit, class_off(rows, Cu, q, r, c).ravel(), 1)
        assert pooled_off(rows, N, q, 0, 0, 0) == bbase(q) * rows * N and class_off(rows, Cu, q, 0, 0) == slot(q) * rows * Cu
    assert (hit == 1).all()


# ---- brute force: y = conv3(upsample(x)) with Keras' cross-correlation, "same" zero padding
def _brute(x, w, dy):
    """dxl (B, Sh, Sh, Sh, Cu) and dw (3, 3, 3, Cu, N) of sum(y * dy)"""
    B, Sh, _, _, Cu = x.shape
    S = 2 * Sh
    xu = x.repeat(2, 1).repeat(2, 2).repeat(2, 3)
    xp = np.pad(xu, ((0, 0), (1, 1), (1, 1), (1, 1), (0, 0)))
    dxp = np.zeros_like(xp)
    dw = np.zeros_like(w)
    for dz, dyy, dx in itertools.product(range(3), repeat=3):
        win = (slice(None), slice(dz, dz + S), slice(dyy, dyy + S), slice(dx, dx + S))
        dw[dz, dyy, dx] = np.einsum("bzyxc,bzyxn->cn", xp[win], dy)
        dxp[win] += dy @ w[dz, dyy, dx].T
    dxu = dxp[:, 1:-1, 1:-1, 1:-1]
    return dxu.reshape(B, Sh, 2, Sh, 2, Sh, 2, Cu).sum((2, 4, 6)), dw


def _up125(x, w, dy):
    """the 125-product form through the twin's blocks, classes and signs"""
    B, Sh, _, _, Cu = x.shape
    S, T, N = 2 * Sh, Sh // 2, dy.shape[-1]
    p = np.pad(dy, ((0, 0), (1, 1), (1, 1), (1, 1), (0, 0)))     # coordinate c at c + 1: 4j - 1 + f at 4j + f
    idx = (4 * np.arange(T)[:, None] + np.arange(6)[None, :])    # [tile][f]
    fine = p[:, idx][:, :, :, idx][:, :, :, :, :, idx]           # (B, jz, fz, jy, fy, jx, fx, N)
    co = COEF.astype(dy.dtype)
    P = np.einsum("af,bg,ch,izfygxhn->abcizyxn", co, co, co, fine, optimize=True)     # (tz, ty, tx, B, jz, jy, jx, N)
    xt = x.reshape(B, T, 2, T, 2, T, 2, Cu)
    xc = XCLS.astype(x.dtype)
    X = np.einsum("ae,bf,dg,izeyfxgk->abdizyxk", xc, xc, xc, xt)     # (cz, cy, cx, B, jz, jy, jx, Cu)
    wu = w                                                           # (3, 3, 3, Cu, N)
    O = np.zeros((3, 3, 3, B, T, T, T, Cu), dy.dtype)
    dw = np.zeros_like(w)
    for tz, ty, tx in TYPES:
        Wb = np.einsum("i,j,k,ijkcn->cn", WCOEF[tz].astype(w.dtype), WCOEF[ty].astype(w.dtype), WCOEF[tx].astype(w.dtype), wu)
        O[cls(tz), cls(ty), cls(tx)] += P[tz, ty, tx] @ Wb.T
        G = np.einsum("izyxc,izyxn->cn", X[cls(tz), cls(ty), cls(tx)], P[tz, ty, tx])
        for iz, iy, ix in itertools.product(range(3), repeat=3):
            s = WCOEF[tz, iz] * WCOEF[ty, iy] * WCOEF[tx, ix]
            if s:
                dw[iz, iy, ix] += s * G
    dxl = np.zeros((B, T, 2, T, 2, T, 2, Cu), dy.dtype)
    for ez, ey, ex in itertools.product(range(2), repeat=3):     # out0 = A + B, out1 = B + C per axis
        dxl[:, :, ez, :, ey, :, ex] = sum(O[ez + a, ey + b, ex + c] for a, b, c in itertools.product(range(2), repeat=3))
    return dxl.reshape(B, Sh, Sh, Sh, Cu), dw


def _case(B, S, Cu, N, seed, dtype):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, S // 2, S // 2, S // 2, Cu)).astype(dtype)
    w = (rng.standard_normal((3, 3, 3, Cu, N)) / np.sqrt(27 * Cu)).astype(dtype)
    dy = rng.standard_normal((B, S, S, S, N)).astype(dtype)
    return x, w, dy


def _rel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())


@pytest.mark.parametrize("B,S", [(2, 8), (1, 16)])
def test_identities_fp64(B, S):
    x, w, dy = _case(B, S, 3, 2, 10 * B + S, np.float64)
    dx_ref, dw_ref = _brute(x, w, dy)
    dx, dw = _up125(x, w, dy)
    assert _rel(dx, dx_ref) <= 1e-12 and _rel(dw, dw_ref) <= 1e-12, (_rel(dx, dx_ref), _rel(dw, dw_ref))


def test_fp32_rounding_class():
    """fp32 against fp64 at S = 8, 16 -> 16 channels: the form stays inside the project's 1e-5 tensor-relative bound, like
    the 27-tap sums it reassociates (coefficients +-1: no Winograd-style loss)"""
    x, w, dy = _case(2, 8, 16, 16, 7, np.float64)
    dx_ref, dw_ref = _brute(x, w, dy)
    dx, dw = _up125(x.astype(np.float32), w.astype(np.float32), dy.astype(np.float32))
    assert dx.dtype == np.float32 and dw.dtype == np.float32
    assert _rel(dx, dx_ref) <= 1e-5 and _rel(dw, dw_ref) <= 1e-5, (_rel(dx, dx_ref), _rel(dw, dw_ref))


def test_product_count():
    assert len(TYPES) == 125 and 8 * 27 == 216
    # every tap gradient is the signed sum of 8 block products, every coarse voxel the sum of 8 class outputs
    for tap in itertools.product(range(3), repeat=3):
        assert sum(1 for t in TYPES if all(WCOEF[t[i], tap[i]] for i in range(3))) == 8
