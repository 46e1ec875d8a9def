"""The identities behind the 8-volume form of the up-split backward's pooled dy (icsg3d_amd/csrc/up8.h), in float32
numpy, without the library.

pool27 sums dy over the <= 8 fine voxels that tap (dz, dy, dx) maps onto a coarse voxel.  Per axis, with a the coarse
coordinate, Sh = S / 2 and out-of-range dy = 0:

    d =  0:  dy[2a]   + dy[2a+1]  =  R[a]        a = 0 .. Sh-1
    d = +1:  dy[2a-1] + dy[2a]    =  Q[a]
    d = -1:  dy[2a+1] + dy[2a+2]  =  Q[a+1]      Q has Sh + 1 entries, Q[Sh] = dy[S-1]

so the 27 tap copies are 2 x 2 x 2 volumes read at 27 shifts.  Both sides keep pool27_kernel's order of additions (x pair
with the lower coordinate first, then the y pair, then 0 + first z plane + second z plane), so the comparison is bit for
bit, signed zeros included."""
import numpy as np
import pytest

BATCHES = (1, 2, 3, 5)
SIZES = (8, 16, 32, 64)


def _padded(dy):
    """dy (B, S, S, S, N) with one zero plane in front of every spatial axis and two behind: coordinate c sits at c + 1"""
    return np.pad(dy, ((0, 0), (1, 2), (1, 2), (1, 2), (0, 0)))


def _slot(p, axis, s, Sh):
    """coordinate 2a - 1 + s for a = 0 .. Sh-1 along `axis` of the padded array"""
    idx = [slice(None)] * p.ndim
    idx[axis] = slice(s, s + 2 * Sh, 2)
    return p[tuple(idx)]


def _pair_taps(p, axis, Sh, zsum=False):
    """pool27's three pair sums along one axis, {d: array}: slots {0,1} for d = +1, {1,2} for d = 0, {2,3} for d = -1"""
    v = [_slot(p, axis, s, Sh) for s in range(4)]
    out = {}
    for d, (i, j) in {+1: (0, 1), 0: (1, 2), -1: (2, 3)}.items():
        out[d] = (np.float32(0) + v[i]) + v[j] if zsum else v[i] + v[j]
    return out


def pool27(dy):
    """{(dz, dy, dx): (B, Sh, Sh, Sh, N)} with pool27_kernel's association"""
    Sh = dy.shape[1] // 2
    taps = {}
    for dx, ax in _pair_taps(_padded(dy), 3, Sh).items():
        for dyy, ay in _pair_taps(ax, 2, Sh).items():
            for dz, az in _pair_taps(ay, 1, Sh, zsum=True).items():
                taps[(dz, dyy, dx)] = az
    return taps


def _rq(p, axis, Sh, zsum=False):
    """(R, Q) along one axis of the padded array: R[a] = c[2a] + c[2a+1], a < Sh; Q[a] = c[2a-1] + c[2a], a <= Sh"""
    def at(off, n):      # coordinate 2a + off, a = 0 .. n-1
        idx = [slice(None)] * p.ndim
        idx[axis] = slice(off + 1, off + 1 + 2 * n, 2)
        return p[tuple(idx)]
    z = np.float32(0)
    r = (z + at(0, Sh)) + at(1, Sh) if zsum else at(0, Sh) + at(1, Sh)
    q = (z + at(-1, Sh + 1)) + at(0, Sh + 1) if zsum else at(-1, Sh + 1) + at(0, Sh + 1)
    return r, q


def pool8(dy):
    """{(kz, ky, kx): volume}, 0 = R (Sh entries on that axis), 1 = Q (Sh + 1 entries)"""
    Sh = dy.shape[1] // 2
    vols = {}
    for kx, ax in enumerate(_rq(_padded(dy), 3, Sh)):
        for ky, ay in enumerate(_rq(ax, 2, Sh)):
            for kz, az in enumerate(_rq(ay, 1, Sh, zsum=True)):
                vols[(kz, ky, kx)] = az
    return vols


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dy(B, S, N, seed):
    rng = np.random.default_rng(seed)
    dy = rng.standard_normal((B, S, S, S, N)).astype(np.float32)
    dy[rng.random(dy.shape) < 0.02] = -0.0       # signed zeros: 0 + (-0) and (-0) + 0 must come out alike on both sides
    return dy


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("B", BATCHES)
def test_27_tap_copies_are_8_volumes_at_27_shifts(B, S):
    Sh = S // 2
    dy = _dy(B, S, 2 if S < 64 else 1, 100 * B + S)
    taps, vols = pool27(dy), pool8(dy)
    assert len(taps) == 27 and len(vols) == 8
    for (dz, dyy, dx), want in taps.items():
        vol = vols[(int(dz != 0), int(dyy != 0), int(dx != 0))]
        sz, sy, sx = int(dz < 0), int(dyy < 0), int(dx < 0)       # d = -1 reads Q one coarse voxel further on
        got = vol[:, sz:sz + Sh, sy:sy + Sh, sx:sx + Sh]
        assert got.shape == want.shape
        assert np.array_equal(_bits(got), _bits(want)), (B, S, (dz, dyy, dx))


@pytest.mark.parametrize("S", SIZES)
def test_per_axis_identities(S):
    """the three identities on one axis, and Q's last entry"""
    Sh = S // 2
    c = _dy(1, S, 1, S)[0, :, 0, 0, 0]
    p = np.pad(c, (1, 2))
    at = lambda k: p[k + 1]
    r = np.array([at(2 * a) + at(2 * a + 1) for a in range(Sh)], np.float32)
    q = np.array([at(2 * a - 1) + at(2 * a) for a in range(Sh + 1)], np.float32)
    for a in range(Sh):
        assert _bits(at(2 * a) + at(2 * a + 1)) == _bits(r[a])              # d = 0
        assert _bits(at(2 * a - 1) + at(2 * a)) == _bits(q[a])              # d = +1
        assert _bits(at(2 * a + 1) + at(2 * a + 2)) == _bits(q[a + 1])      # d = -1
    assert _bits(q[Sh]) == _bits(c[S - 1] + np.float32(0))
    assert _bits(q[0]) == _bits(np.float32(0) + c[0])


def test_sizes():
    """8 P^3 against 27 Sh^3 floats per sample and channel: the ratios the change is sized by"""
    ratio = {S: 27 * (S // 2) ** 3 / (8 * (S // 2 + 1) ** 3) for S in (4, 8, 16, 32)}
    assert ratio[4] == 1.0
    assert abs(ratio[8] - 1.73) < 0.01 and abs(ratio[16] - 2.37) < 0.01 and abs(ratio[32] - 2.81) < 0.01
