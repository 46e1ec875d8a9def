"""interpolate.py on the MI355X: latent_path_kernel held bit for bit to the reference's own interpolate
(tests/golden/interp_golden.npz) and to its arithmetic restated in numpy; slerp to a float64 restatement under a derived
bound; the chains ics_vae_interpolate / ics_vae_interpolate_to_unet_atoms held bit for bit to the composed calls they
replace; interpolate() against the fp64 oracle; the refusals; the script end to end.

The whole file also passes under ICSG3D_DEBUG_CANARY=1 (guard bytes behind every device buffer; the last test checks the
guards of the handles it drove)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import numpy_ref as R
from saturated import saturate_head

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "interp_golden.npz")


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _lerp(za, zb, alpha):
    """"Semantics": fl32( fl64(za) + alpha * fl64( fl32(zb - za) ) ), product and sum rounded separately in float64"""
    with np.errstate(all="ignore"):
        diff = (zb - za).astype(np.float64)                       # float32 subtraction first
        assert (zb - za).dtype == np.float32
        return (za.astype(np.float64)[:, None, :] + alpha[None, :, None] * diff[:, None, :]).astype(np.float32)


# ---------------------------------------------------------------- 1. the kernel, lerp
def test_latent_path_lerp_equals_the_reference_bit_for_bit():
    from icsg3d_amd.engine import latent_path
    g = np.load(GOLDEN)
    n = len(g["num_interps"])
    assert n >= 10
    for k in range(n):
        got = latent_path(g["za_%d" % k], g["zb_%d" % k], g["alpha_%d" % k])
        assert got.dtype == np.float32 and got.shape == (1,) + g["dec_z_%d" % k].shape
        assert np.array_equal(_bits(got[0]), _bits(g["dec_z_%d" % k])), k


def test_latent_path_lerp_sweep_bit_for_bit():
    from icsg3d_amd.engine import latent_path
    rng = np.random.default_rng(41)
    checked = 0
    for latent in (1, 7, 63, 64, 65, 256, 300):
        for steps in (1, 2, 8, 33):
            for pairs in (1, 3, 50):
                with np.errstate(all="ignore"):
                    za = (rng.standard_normal((pairs, latent)) * 10.0 ** rng.uniform(-42, 30, (pairs, latent))).astype(np.float32)
                    zb = (rng.standard_normal((pairs, latent)) * 10.0 ** rng.uniform(-42, 30, (pairs, latent))).astype(np.float32)
                za.flat[0], zb.flat[0] = np.float32(1e-40), np.float32(-2e-41)          # denormals
                za.flat[-1], zb.flat[-1] = np.float32(1e30), np.float32(-1e30)           # 1e30 magnitudes
                if latent > 4:
                    zb[:, 2] = za[:, 2]
                    za[:, 3], zb[:, 3] = 0.0, -0.0
                alpha = np.linspace(0, rng.choice([1.0, 0.5, 2.0, -1.5, 3.25]), steps)
                if steps >= 2:
                    alpha[1] = -0.75                                                       # outside [0, 1], unsorted
                assert np.isfinite(za).all() and np.isfinite(zb).all()
                got = latent_path(za, zb, alpha)
                ref = _lerp(za, zb, alpha)
                assert np.array_equal(_bits(got), _bits(ref)), (latent, steps, pairs)
                checked += 1
    assert checked == 7 * 4 * 3


# ---------------------------------------------------------------- 2. the kernel, slerp
def _slerp_ref(a32, b32, t):
    """float64 restatement: (coefficient a, coefficient b, fallback) per pair"""
    a, b = a32.astype(np.float64), b32.astype(np.float64)
    aa, bb, ab = (a * a).sum(), (b * b).sum(), (a * b).sum()
    if not (aa > 0 and bb > 0):
        return None
    c = min(1.0, max(-1.0, ab / (np.sqrt(aa) * np.sqrt(bb))))
    w, s = np.arccos(c), np.sqrt(1.0 - c * c)
    if s < 1e-3:
        return None
    return np.sin((1.0 - t) * w) / s, np.sin(t * w) / s


def _pair_with_sin(rng, latent, s):
    """unit-scale codes a, b with sin(angle) = s (float32 rounding moves it by ~1e-7 relative)"""
    a = rng.standard_normal(latent)
    u = rng.standard_normal(latent)
    u -= a * (u @ a) / (a @ a)
    a /= np.linalg.norm(a); u /= np.linalg.norm(u)
    b = 1.7 * (np.sqrt(1 - s * s) * a + s * u)
    return a.astype(np.float32), b.astype(np.float32)


def test_latent_path_slerp_bound_fallbacks_and_determinism():
    from icsg3d_amd.engine import latent_path
    rng = np.random.default_rng(43)
    alpha = np.array([0.0, 0.125, 0.5, 1.0, 1.5, 2.0, -0.5, -2.0])
    za, zb = [], []
    for latent in (256,):
        for _ in range(20):
            za.append(rng.standard_normal(latent).astype(np.float32)); zb.append(rng.standard_normal(latent).astype(np.float32))
        for s in (0.9, 0.1, 1e-2, 2e-3):                                   # down to the slerp side of the threshold
            a, b = _pair_with_sin(rng, latent, s)
            za.append(a); zb.append(b)
            za.append(a); zb.append((-b).astype(np.float32))              # near-antiparallel: the terms cancel
    za, zb = np.stack(za), np.stack(zb)
    got = latent_path(za, zb, alpha, "slerp")
    lerp = latent_path(za, zb, alpha, "lerp")
    worst = 0.0
    for p in range(len(za)):
        co = _slerp_ref(za[p], zb[p], alpha)
        assert co is not None, p
        assert not np.array_equal(_bits(got[p]), _bits(lerp[p])), p        # took the slerp side
        ca, cb = co
        a, b = za[p].astype(np.float64), zb[p].astype(np.float64)
        ref = ca[:, None] * a[None] + cb[:, None] * b[None]
        bound = 2.0 ** -22 * (np.abs(ca[:, None] * a[None]) + np.abs(cb[:, None] * b[None]))
        err = np.abs(got[p].astype(np.float64) - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (p, float((err / np.maximum(bound, 1e-300)).max()))
    print("slerp: worst error / bound = %.3f" % worst)
    # other latent sizes (partial waves, several strides)
    for latent in (1, 7, 63, 64, 65, 300):
        a = rng.standard_normal((4, latent)).astype(np.float32); b = rng.standard_normal((4, latent)).astype(np.float32)
        out = latent_path(a, b, alpha, "slerp")
        for p in range(4):
            co = _slerp_ref(a[p], b[p], alpha)
            if co is None:                                                 # latent 1: always (anti)parallel
                assert np.array_equal(_bits(out[p]), _bits(_lerp(a[p:p + 1], b[p:p + 1], alpha)[0]))
                continue
            ca, cb = co
            x, y = a[p].astype(np.float64), b[p].astype(np.float64)
            ref = ca[:, None] * x[None] + cb[:, None] * y[None]
            bound = 2.0 ** -22 * (np.abs(ca[:, None] * x[None]) + np.abs(cb[:, None] * y[None]))
            assert (np.abs(out[p].astype(np.float64) - ref) <= bound).all(), (latent, p)
    # fallback pairs equal the lerp of the same pair bit for bit
    a = rng.standard_normal((1, 256)).astype(np.float32)
    lo_a, lo_b = _pair_with_sin(rng, 256, 5e-4)                           # the lerp side of the threshold
    fa = np.concatenate([a, a, a, a, np.zeros_like(a), lo_a[None]])
    fb = np.concatenate([a, -a, 2 * a, np.zeros_like(a), a, lo_b[None]])
    assert np.array_equal(_bits(latent_path(fa, fb, alpha, "slerp")), _bits(latent_path(fa, fb, alpha, "lerp")))
    assert np.array_equal(_bits(latent_path(fa, fb, alpha, "lerp")), _bits(_lerp(fa, fb, alpha)))
    # two runs give identical bits
    assert np.array_equal(_bits(latent_path(za, zb, alpha, "slerp")), _bits(got))


# ---------------------------------------------------------------- engines
def _weights(C, d, seed):
    from icsg3d_amd.synthetic import random_weights
    rng = np.random.default_rng(seed)
    uw, vw = random_weights(d, C, seed)
    for w in (uw, vw):                       # non-trivial moving statistics: eval-mode BatchNorm everywhere
        for k in list(w):
            if k.endswith("moving_var"):
                w[k] = rng.uniform(0.5, 1.5, w[k].shape).astype(np.float32)
            elif k.endswith("moving_mean"):
                w[k] = rng.uniform(-0.2, 0.2, w[k].shape).astype(np.float32)
    assert any(k.endswith("moving_var") for k in vw) and any(k.endswith("moving_mean") for k in vw)
    return uw, vw


def _vae(C, d, mb, seed):
    from icsg3d_amd.synthetic import random_engines
    return random_engines(d, C, mb, unet=False, weights=_weights(C, d, seed))[0]


def _pairs(rng, P, d, C):
    from icsg3d_amd.synthetic import synthetic_batch
    X = synthetic_batch(2 * P, d, C, seed=int(rng.integers(1 << 30)), noise=1e-3)[0].astype(np.float32)
    cond = np.eye(10, dtype=np.float32)[rng.integers(0, 10, P)]
    eps = rng.standard_normal((P, 2, 256)).astype(np.float32)
    return X[0::2].copy(), X[1::2].copy(), cond, eps


def _interleave(a, b):
    return np.stack([a, b], axis=1).reshape((2 * len(a),) + a.shape[1:])


# ---------------------------------------------------------------- 3. one group == the composed calls
@pytest.mark.parametrize("d,C", [(16, 1), (16, 4), (32, 1), (32, 4)])
@pytest.mark.parametrize("mode", ["lerp", "slerp"])
def test_chain_equals_encode_path_decode(d, C, mode):
    from icsg3d_amd.engine import latent_path
    rng = np.random.default_rng(100 * d + C)
    P, S = 3, 5
    ve = _vae(C, d, 16, seed=d + C)                       # 2 P <= 16, P S <= 16: one group
    a, b, cond, eps = _pairs(rng, P, d, C)
    alpha = np.linspace(0, 1.25, S)
    z_ends, z_path, recon = ve.interpolate(a, b, cond, eps[:, 0], eps[:, 1], alpha, mode)
    _, _, z = ve.encode(_interleave(a, b), np.repeat(cond, 2, axis=0), eps.reshape(2 * P, 256))
    assert _same_bits(z_ends.reshape(2 * P, 256), z)
    assert _same_bits(z_path, latent_path(z_ends[:, 0], z_ends[:, 1], alpha, mode))
    ref = ve.decode(z_path.reshape(P * S, 256), np.repeat(cond, S, axis=0))
    assert recon.shape == (P, S, d, d, d, C) and _same_bits(recon.reshape(ref.shape), ref)
    assert np.abs(recon).max() > 0
    if mode == "slerp":
        assert not np.array_equal(z_path, latent_path(z_ends[:, 0], z_ends[:, 1], alpha, "lerp"))


# ---------------------------------------------------------------- 4. grouping
def test_chain_grouping(relerr):
    from icsg3d_amd.engine import latent_path
    rel_err = relerr
    rng = np.random.default_rng(7)
    d, C, P, S = 16, 4, 11, 3                          # P S = 33 frames through a handle of 8: groups of 2 pairs, 8 % 3 != 0
    a, b, cond, eps = _pairs(rng, P, d, C)
    alpha = np.linspace(0, 1, S)
    small, big = _vae(C, d, 8, seed=9), _vae(C, d, 40, seed=9)
    ze1, zp1, r1 = small.interpolate(a, b, cond, eps[:, 0], eps[:, 1], alpha)
    ze2, zp2, r2 = big.interpolate(a, b, cond, eps[:, 0], eps[:, 1], alpha)     # 22 <= 40, 33 <= 40: one group
    assert _same_bits(zp1, latent_path(ze1[:, 0], ze1[:, 1], alpha))
    assert _same_bits(zp2, latent_path(ze2[:, 0], ze2[:, 1], alpha))
    e = rel_err(r1, r2)
    print("grouping: recon rel err %.3g vs one group, bit-identical: %s; z_ends bit-identical: %s"
          % (e, np.array_equal(_bits(r1), _bits(r2)), np.array_equal(_bits(ze1), _bits(ze2))))
    assert e <= 1e-5


# ---------------------------------------------------------------- 5. the atoms chain
def _oracles(C, d, seed):
    uo = R.UnetOracle(in_ch=C, seed=1)
    vo = R.VaeOracle(uo, in_ch=C, d=d, seed=3)
    rng = np.random.default_rng(seed)
    for o in (uo, vo):
        for k in list(o.S):
            o.S[k] = rng.uniform(0.5, 1.5, o.S[k].shape) if k.endswith("var") else rng.uniform(-0.2, 0.2, o.S[k].shape)
    return uo, vo


def _same_atoms(o1, o2):
    for k in ("species", "mask", "density", "coord_minmax", "regions", "n_components", "n_atoms", "stats", "bounds", "failed"):
        x, y = o1[k], o2[k]
        assert (x is None) == (y is None), k
        if x is not None:
            assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), k
    assert len(o1["atoms"]) == len(o2["atoms"])
    for (s1, m1), (s2, m2) in zip(o1["atoms"], o2["atoms"]):
        assert np.array_equal(np.asarray(s1), np.asarray(s2))
        assert np.array_equal(np.asarray(m1, np.float64), np.asarray(m2, np.float64))


def test_atoms_chain_equals_decode_to_atoms():
    """full-width U-Net with a confident head (as tests/test_gpu_chain.py: with Glorot heads sig never reaches 0.8 and the
    comparison would be all-zeros == all-zeros), fitted on the oracle's decodings of the frames the chain decodes"""
    from icsg3d_amd.engine import UnetEngine, VaeEngine
    d, C, P, S = 16, 4, 2, 3
    uo, vo = _oracles(C, d, 3)
    rng = np.random.default_rng(11)
    pm = UnetEngine(in_channels=C, d=d, max_batch=8); pm.set_weights({**uo.P, **uo.S})
    ve = VaeEngine(pm, in_channels=C, d=d, max_batch=8); ve.set_weights({**vo.P, **vo.S})
    a, b, cond, eps = _pairs(rng, P, d, C)
    alpha = np.linspace(0, 1, S)
    ze, zp, _ = ve.interpolate(a, b, cond, eps[:, 0], eps[:, 1], alpha, want_recon=False)
    rec0 = vo.predict_decoder(zp.reshape(P * S, 256).astype(np.float64), np.repeat(cond, S, axis=0).astype(np.float64))
    dens = rec0[..., 0]
    lab = np.zeros(dens.shape, np.uint8)
    for i in range(P * S):
        lab[i][dens[i] > np.quantile(dens[i], 0.97)] = 1 + 13 * i
    saturate_head(uo, rec0, lab, training=False)
    seg = UnetEngine(in_channels=C, d=d, max_batch=8); seg.set_weights({**uo.P, **uo.S})
    kw = dict(thresh=0.8, min_voxels=3, max_atoms=512, want_regions=True)
    got = ve.interpolate_to_atoms(seg, a, b, cond, eps[:, 0], eps[:, 1], alpha, **kw)
    assert _same_bits(got["z_ends"], ze) and _same_bits(got["z_path"], zp)
    ref = ve.decode_to_atoms(seg, zp.reshape(P * S, 256), np.repeat(cond, S, axis=0), **kw)
    _same_atoms(got, ref)
    assert got["mask"].any() and got["n_atoms"].sum() > 0
    # several groups (a U-Net handle of 4: one pair per group) give the same frames
    seg4 = UnetEngine(in_channels=C, d=d, max_batch=4); seg4.set_weights({**uo.P, **uo.S})
    got4 = ve.interpolate_to_atoms(seg4, a, b, cond, eps[:, 0], eps[:, 1], alpha, **kw)
    from icsg3d_amd.engine import latent_path
    assert _same_bits(got4["z_path"], latent_path(got4["z_ends"][:, 0], got4["z_ends"][:, 1], alpha))
    assert got4["mask"].shape == got["mask"].shape and got4["mask"].any()
    print("atoms chain, groups of one pair vs one group: masks identical %s, stats identical %s"
          % (np.array_equal(got4["mask"], got["mask"]), np.array_equal(got4["stats"], got["stats"])))


# ---------------------------------------------------------------- 6. interpolate() against the fp64 oracle
def test_interpolate_against_the_oracle(relerr):
    from icsg3d_amd.interpolate import interpolate, interpolate_pairs
    from icsg3d_amd.vae.lattice_vae import LatticeDFCVAE
    rel_err = relerr
    d, C, n = 16, 4, 6
    uo = R.UnetOracle(in_ch=C, seed=1)
    vo = R.VaeOracle(uo, in_ch=C, d=d, seed=3)
    rng = np.random.default_rng(5)
    for k in list(vo.S):
        vo.S[k] = rng.uniform(0.5, 1.5, vo.S[k].shape) if k.endswith("var") else rng.uniform(-0.2, 0.2, vo.S[k].shape)
    vae = LatticeDFCVAE(input_shape=(d, d, d, C), perceptual_model={**uo.P, **uo.S})
    vae._set_model(batch_size=20)
    vae._set_weights({**vo.P, **vo.S})
    A, B, cond, eps = _pairs(rng, 2, d, C)
    out, zs = interpolate(A[:1], B[:1], cond[:1], vae, n, True, 1.5, eps=eps[0])
    assert vae.batch_size == n
    assert out.dtype == np.float32 and out.shape == (n + 2, d, d, d, C) and zs.shape == (n + 2, 256)
    assert np.array_equal(out[0], A[0]) and np.array_equal(out[-1], B[0])
    c64 = cond[:1].astype(np.float64)
    z_a = vo.predict_encoder(A[:1].astype(np.float64), c64, eps[0, :1].astype(np.float64))[2]
    z_b = vo.predict_encoder(B[:1].astype(np.float64), c64, eps[0, 1:].astype(np.float64))[2]
    alpha = np.linspace(0, 1.5, n)
    line = z_a + alpha[:, None] * (z_b - z_a)
    ref = vo.predict_decoder(line, np.tile(c64, (n, 1)))
    assert rel_err(zs[0], z_a[0]) <= 1e-5 and rel_err(zs[-1], z_b[0]) <= 1e-5 and rel_err(zs[1:-1], line) <= 1e-5
    for k in range(n):
        assert rel_err(out[1 + k], ref[k]) <= 1e-5, k
    assert interpolate(A[:1], B[:1], cond[:1], vae, n, eps=eps[0]).shape == (n + 2, d, d, d, C)
    # without eps: a fresh draw per call (the sampled z, F8)
    o1 = interpolate(A[:1], B[:1], cond[:1], vae, 2)
    o2 = interpolate(A[:1], B[:1], cond[:1], vae, 2)
    assert not np.array_equal(o1[1:-1], o2[1:-1])
    rows, zz = interpolate_pairs(A, B, cond, vae, n, True, 1.5, eps=eps)
    assert rows.shape == (2, n + 2, d, d, d, C) and _same_bits(zz[0], zs) and rel_err(rows[0], out) <= 1e-5


# ---------------------------------------------------------------- 7. refusals
def test_refusals_write_nothing_and_leave_the_handle_usable():
    from icsg3d_amd import _lib as L
    from icsg3d_amd.engine import UnetEngine, VaeEngine, latent_path
    lib = L.load()
    d, C, P, S, mb = 16, 1, 2, 3, 6
    rng = np.random.default_rng(1)
    ve = _vae(C, d, mb, seed=2)
    a, b, cond, eps = _pairs(rng, P, d, C)
    ea, eb = np.ascontiguousarray(eps[:, 0]), np.ascontiguousarray(eps[:, 1])
    alpha = np.linspace(0, 1, S)
    ze = np.full((P, 2, 256), -7.0, np.float32)
    zp = np.full((P, S, 256), -7.0, np.float32)
    rec = np.full((P * S, d, d, d, C), -7.0, np.float32)

    def untouched():
        return (ze == -7.0).all() and (zp == -7.0).all() and (rec == -7.0).all()

    def call(h=None, a_=a, b_=b, c_=cond, ea_=ea, eb_=eb, p_=P, al_=alpha, s_=S, m_=0):
        return lib.ics_vae_interpolate(ve._h if h is None else h, L.fptr(a_), L.fptr(b_), L.fptr(c_), L.fptr(ea_), L.fptr(eb_),
                                       p_, L.f64ptr(al_), s_, m_, L.fptr(ze), L.fptr(zp), L.fptr(rec))
    bad_alpha = alpha.copy(); bad_alpha[1] = np.nan
    inf_alpha = alpha.copy(); inf_alpha[2] = np.inf
    many = np.zeros(mb + 1)
    cases = [(dict(p_=0), "pairs"), (dict(s_=0), "steps"), (dict(al_=many, s_=mb + 1), "steps exceeds max_batch"),
             (dict(al_=bad_alpha), "alpha[1]"), (dict(al_=inf_alpha), "alpha[2]"), (dict(m_=2), "mode"), (dict(m_=-1), "mode"),
             (dict(a_=None), "null"), (dict(b_=None), "null"), (dict(c_=None), "null"), (dict(ea_=None), "null"),
             (dict(eb_=None), "null"), (dict(al_=None), "alpha"), (dict(h=ve.unet._h), "not a VAE")]
    for kw, msg in cases:
        assert call(**kw) != 0, msg
        err = lib.ics_last_error().decode()
        assert msg in err, (msg, err)
        assert untouched(), msg
    one = _vae(C, d, 1, seed=2)                                    # max_batch < 2
    assert call(h=one._h, p_=1, s_=1) != 0 and "max_batch" in lib.ics_last_error().decode() and untouched()
    # the atoms variant: U-Net of another C / another d, null counts / stats, steps above the U-Net's max_batch
    counts = np.full((P * S, 2), -7, np.int32)
    stats = np.full((P * S, 8, 11), -7, np.int32)

    def atoms(un, cn=counts, st=stats, ma=8):
        return lib.ics_vae_interpolate_to_unet_atoms(ve._h, un._h, L.fptr(a), L.fptr(b), L.fptr(cond), L.fptr(ea), L.fptr(eb), P,
                                                     L.f64ptr(alpha), S, 0, 0.8, 3, ma, L.fptr(ze), L.fptr(zp), None, None, None,
                                                     None, None, L.i32ptr(cn), L.i32ptr(st), None)
    ok_un = UnetEngine(in_channels=C, d=d, max_batch=mb)
    for un, kw, msg in [(UnetEngine(in_channels=4, d=d, max_batch=mb), {}, "do not match"),
                        (UnetEngine(in_channels=C, d=32, max_batch=mb), {}, "do not match"),
                        (UnetEngine(in_channels=C, d=d, max_batch=S - 1), {}, "steps exceeds max_batch"),
                        (ok_un, dict(cn=None), "null"), (ok_un, dict(st=None), "null"), (ok_un, dict(ma=0), "max_atoms"),
                        (ve, {}, "not a U-Net")]:
        assert atoms(un, **kw) != 0, msg
        err = lib.ics_last_error().decode()
        assert msg in err, (msg, err)
        assert untouched() and (counts == -7).all() and (stats == -7).all(), msg
    # the op
    path = np.full((P, S, 256), -7.0, np.float32)
    za, zb = np.ascontiguousarray(eps[:, 0]), np.ascontiguousarray(eps[:, 1])

    def op(za_=za, zb_=zb, p_=P, l_=256, al_=alpha, s_=S, m_=0, out=path):
        return lib.ics_op_latent_path(L.fptr(za_), L.fptr(zb_), p_, l_, L.f64ptr(al_), s_, m_, L.fptr(out))
    for kw, msg in [(dict(p_=0), "pairs"), (dict(l_=0), "latent"), (dict(s_=0), "steps"), (dict(m_=5), "mode"),
                    (dict(al_=bad_alpha), "alpha[1]"), (dict(al_=None), "alpha"), (dict(za_=None), "null"),
                    (dict(zb_=None), "null")]:
        assert op(**kw) != 0, msg
        assert msg in lib.ics_last_error().decode(), msg
        assert (path == -7.0).all(), msg
    assert lib.ics_op_latent_path(L.fptr(za), L.fptr(zb), P, 256, L.f64ptr(alpha), S, 0, None) != 0
    with pytest.raises(ValueError):
        latent_path(za, zb, alpha, "cubic")
    # the next valid calls succeed
    assert op() == 0 and np.array_equal(_bits(path), _bits(_lerp(za, zb, alpha)))
    ve.upload_batch(a, cond, ea)
    assert ve.train_step_resident(True) is not None               # a resident batch: the resident step runs
    ve.upload_batch(a, cond, ea)
    assert call() == 0 and not (ze == -7.0).any() and not (zp == -7.0).any() and not (rec == -7.0).any()
    # ... and the chain cleared the resident batch: the resident step and the resident reconstruction are refused
    m = np.zeros(4, np.float32)
    assert lib.ics_vae_train_step_resident(ve._h, L.fptr(m)) != 0
    assert "no resident batch" in lib.ics_last_error().decode()
    assert lib.ics_vae_reconstruct_resident_to_unet_atoms(ve._h, ok_un._h, 0.8, 3, 8, None, None, None, None, None,
                                                          L.i32ptr(counts), L.i32ptr(stats), None) != 0
    assert "no resident batch" in lib.ics_last_error().decode()
    assert atoms(ok_un) == 0 and (counts >= 0).all()
    assert lib.ics_vae_train_step_resident(ve._h, L.fptr(m)) != 0
    ve.upload_batch(a, cond, ea)
    assert ve.train_step_resident(True) is not None
    for h in (ve, one):
        dirty = L.C.c_int(-1)
        L.check(lib.ics_net_check_canaries(h._h, L.C.byref(dirty)))
        assert dirty.value == 0, lib.ics_last_error().decode()


def test_cond_shape_3_single_channel_matches_the_oracle():
    """interpolate.py --ncond 3 --channels 1: 1 + 3 input channels need no padding, and the condition-folded first encoder
    layer was left without its sources there (every forward was refused).  Encoder, decoder and one train step against the
    fp64 oracle at cond_shape 3."""
    from icsg3d_amd.engine import UnetEngine, VaeEngine
    B, d, C, nc = 2, 16, 1, 3
    X, _, _ = R.synthetic_batch(B, d, C, seed=0, dtype=np.float64)
    X = X + 1e-3 * np.random.default_rng(5).uniform(size=X.shape)
    cond = np.eye(nc)[[2, 0]]
    uo = R.UnetOracle(in_ch=C, seed=1)
    vo = R.VaeOracle(uo, in_ch=C, cond=nc, d=d, seed=3)
    pm = UnetEngine(in_channels=C, d=d, max_batch=B); pm.set_weights(uo.P)
    ve = VaeEngine(pm, in_channels=C, cond_shape=nc, d=d, max_batch=B); ve.set_weights(vo.P)
    eps = np.random.default_rng(2).standard_normal((B, 256))
    zm, zlv, z = ve.encode(X, cond, eps)
    zm_ref, zlv_ref, z_ref = vo.predict_encoder(X, cond, eps)
    for got, ref in ((zm, zm_ref), (zlv, zlv_ref), (z, z_ref)):
        assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
    rec, rec_ref = ve.decode(z_ref, cond), vo.predict_decoder(z_ref, cond)
    assert np.abs(rec - rec_ref).max() <= 1e-5 * np.abs(rec_ref).max()
    np.testing.assert_allclose(ve.train_step(X, cond, eps), vo.train_on_batch(X, cond, eps), rtol=2e-5)


# ---------------------------------------------------------------- 8. the script
def test_script_end_to_end(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "interpolate.py"), "--name", "t", "--synthetic", "--ninterps", "4",
                        "--ncond", "3", "--d", "16", "--channels", "1", "--atoms", "--seed", "5"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    out = tmp_path / "output" / "interpolation"
    g = np.load(out / "t_rows.npz")
    assert g["rows"].shape == (3, 6, 16, 16, 16, 1) and g["rows"].dtype == np.float32
    assert g["zs"].shape == (3, 6, 256) and g["ids"].shape == (3, 2) and g["formulae"].shape == (3, 2)
    assert np.array_equal(g["alpha"], np.linspace(0, 1, 4)) and str(g["mode"]) == "lerp"
    assert g["frame_emd"].shape == (3, 3) and g["n_atoms"].shape == (3, 4) and g["failed"].shape == (3, 4)
    run = json.load(open(out / "run.json"))
    assert run["enda"] == "CeCrO3" and run["endb"] == "YbCrO3" and run["ninterps"] == 4 and run["rows_shape"] == [3, 6, 16, 16, 16, 1]
    # the rows are interpolate_pairs' with the same seed
    spec = importlib.util.spec_from_file_location("interpolate_script", os.path.join(ROOT, "interpolate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from icsg3d_amd.cli import load_models
    from icsg3d_amd.interpolate import interpolate_pairs
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        vae, _ = load_models("t", 16, 1, 3, 20, True, 5, True)
    finally:
        os.chdir(cwd)
    A, B, ids, _ = mod.synthetic_pairs(3, 16, 1, 5)
    rows, zs = interpolate_pairs(A, B, np.eye(3, dtype=np.float32), vae, 4, True, eps=mod.draw_eps(5, 3, 256))
    assert np.array_equal(_bits(rows), _bits(g["rows"])) and np.array_equal(_bits(zs), _bits(g["zs"]))
    assert [list(i) for i in ids] == g["ids"].tolist()
