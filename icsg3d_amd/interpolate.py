"""interpolate() of the reference's interpolate.py (interpolate.py:47-64) on the MI355X engine: encode two crystals
under one condition, walk a line between their sampled latent codes, decode every point.

- interpolate        the reference's function, same positional signature and return values; one device-resident chain
                     (VaeEngine.interpolate -> ics_vae_interpolate) instead of two encoder.predict round trips, numpy
                     arithmetic and a decoder.predict.
- interpolate_pairs  the same for P pairs in one call (what the interpolate.py script uses: every condition bin at once).
- lerp_path / slerp_path / latent_path_numpy
                     the walk itself in numpy -- the arithmetic the kernel is held to, and the path a `vae` WITHOUT an
                     engine takes (any object with encoder.predict / decoder.predict).

The reference's line is not a float32 lerp: `z_b - z_a` is a float32 subtraction, `alpha = np.linspace(...)` is float64, so
`z_a + alpha[:, None] * z_a2b` is evaluated in float64 and Keras rounds it to float32 when it feeds the decoder:
    step k, element j = fl32( fl64(z_a[j]) + alpha[k] * fl64( fl32(z_b[j] - z_a[j]) ) ).
Both paths reproduce that bit for bit.  `zs` (return_zs) holds these float32 codes -- what the decoder received; the
reference returns the float64 line before Keras' rounding, whose float32 cast equals it.
z_a, z_b are the SAMPLED codes (the encoder's third output): without `eps` every call draws a fresh N(0,1)
pair, as the reference's encoder.predict does.
mode="slerp" (new, opt-in) is spherical interpolation in float64, rounded once; (anti)parallel or zero codes fall back to
the lerp -- include/icsg3d.h has the formula.
"""
from __future__ import annotations

import numpy as np

SLERP_MIN_SIN = 1e-3


def lerp_path(z_a, z_b, alpha):
    """(P, latent) float32 codes, (S,) float64 steps -> (P, S, latent) float32, the reference's arithmetic."""
    z_a, z_b = np.asarray(z_a, np.float32), np.asarray(z_b, np.float32)
    alpha = np.asarray(alpha, np.float64).reshape(-1)
    z_a2b = z_b - z_a                                                  # float32 (interpolate.py:54)
    with np.errstate(all="ignore"):
        line = z_a[:, None, :].astype(np.float64) + alpha[None, :, None] * z_a2b[:, None, :].astype(np.float64)
        return line.astype(np.float32)                                 # Keras' cast at the decoder's input


def slerp_path(z_a, z_b, alpha):
    """Spherical interpolation in float64 from the float32 codes; pairs with a zero code or sin(angle) < 1e-3 lerp."""
    z_a, z_b = np.asarray(z_a, np.float32), np.asarray(z_b, np.float32)
    alpha = np.asarray(alpha, np.float64).reshape(-1)
    out = lerp_path(z_a, z_b, alpha)
    a, b = z_a.astype(np.float64), z_b.astype(np.float64)
    with np.errstate(all="ignore"):
        for p in range(len(a)):
            aa, bb, ab = a[p] @ a[p], b[p] @ b[p], a[p] @ b[p]
            if not (aa > 0.0 and bb > 0.0):
                continue
            c = min(1.0, max(-1.0, ab / (np.sqrt(aa) * np.sqrt(bb))))
            w, s = np.arccos(c), np.sqrt(1.0 - c * c)
            if not s >= SLERP_MIN_SIN:
                continue
            ca, cb = np.sin((1.0 - alpha) * w) / s, np.sin(alpha * w) / s
            out[p] = (ca[:, None] * a[p][None, :] + cb[:, None] * b[p][None, :]).astype(np.float32)
    return out


def latent_path_numpy(z_a, z_b, alpha, mode="lerp"):
    if mode in ("lerp", 0):
        return lerp_path(z_a, z_b, alpha)
    if mode in ("slerp", 1):
        return slerp_path(z_a, z_b, alpha)
    raise ValueError("mode must be 'lerp' or 'slerp', not %r" % (mode,))


def _predict_z(vae, M, cond, eps):
    if eps is None:
        return vae.encoder.predict([M, cond])[2]
    return vae.encoder.predict([M, cond], eps=eps)[2]


def interpolate_pairs(A, B, conds, vae, num_interps=8, return_zs=False, max_alpha=1, *, mode="lerp", eps=None):
    """interpolate() for P pairs at once: A, B (P, d, d, d, C), conds (P, cond_shape), eps None or (P, 2, latent) (the
    draws of pair p's two encoder calls).  Returns rows (P, num_interps + 2, d, d, d, C) float32 -- row p is
    interpolate(A[p:p+1], B[p:p+1], conds[p:p+1], ...) -- and with return_zs also zs (P, num_interps + 2, latent)."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    conds = np.asarray(conds, np.float32)
    P = len(A)
    if A.shape != B.shape or A.ndim != 5 or conds.shape[:1] != (P,) or conds.ndim != 2:
        raise ValueError("bad shapes: A %s, B %s, conds %s" % (A.shape, B.shape, conds.shape))
    num_interps = int(num_interps)
    alpha = np.linspace(0, max_alpha, num_interps)                     # float64 (interpolate.py:55)
    latent_path_numpy(np.zeros((1, 1), np.float32), np.zeros((1, 1), np.float32), alpha[:0], mode)   # mode check
    vae.batch_size = num_interps                                       # the reference's side effect (interpolate.py:52)
    if hasattr(vae, "_engine"):
        if eps is None:
            eps = np.random.normal(size=(P, 2, vae.latent_dim))
        eps = np.asarray(eps, np.float32).reshape(P, 2, vae.latent_dim)
        eng = vae._engine(max(2, num_interps), grow=True)
        z_ends, z_path, recon = eng.interpolate(A, B, conds, eps[:, 0], eps[:, 1], alpha, mode)
    else:                                                              # no engine: predict calls + the numpy walk
        eps = None if eps is None else np.asarray(eps).reshape(P, 2, -1)
        z_ends, z_path, recon = [], [], []
        for p in range(P):
            cond = conds[p:p + 1]
            z_a = np.asarray(_predict_z(vae, A[p:p + 1], cond, None if eps is None else eps[p, 0:1]), np.float32)
            z_b = np.asarray(_predict_z(vae, B[p:p + 1], cond, None if eps is None else eps[p, 1:2]), np.float32)
            z_int = latent_path_numpy(z_a, z_b, alpha, mode)[0]
            z_ends.append(np.concatenate([z_a, z_b]))
            z_path.append(z_int)
            recon.append(np.asarray(vae.decoder.predict([z_int, np.tile(cond, (num_interps, 1))]), np.float32))
        z_ends, z_path, recon = np.stack(z_ends), np.stack(z_path), np.stack(recon)
    rows = np.concatenate([A[:, None], recon, B[:, None]], axis=1)     # [a, M_interps, b] (interpolate.py:60-61)
    if return_zs:
        return rows, np.concatenate([z_ends[:, :1], z_path, z_ends[:, 1:]], axis=1)
    return rows


def interpolate(a, b, cond, vae, num_interps=8, return_zs=False, max_alpha=1, *, mode="lerp", eps=None):
    """Linearly interpolate between two M's a and b (1, d, d, d, C) under cond (1, cond_shape), num_interps points from
    alpha = 0 to max_alpha (interpolate.py:47-64).  Returns concatenate([a, M_interps, b]) (num_interps + 2, d, d, d, C)
    float32 -- steps 0 and num_interps - 1 are DECODINGS of z_a / z_b(max_alpha), so the endpoints appear twice in
    different form, as in the reference -- and with return_zs also concatenate([z_a, z_interps, z_b]).
    eps: None (a fresh draw per encoder call) or (2, latent)."""
    if eps is not None:
        eps = np.asarray(eps)[None]
    out = interpolate_pairs(a, b, cond, vae, num_interps, return_zs, max_alpha, mode=mode, eps=eps)
    if return_zs:
        return out[0][0], out[1][0]
    return out[0]
