"""fp64 numpy restatement of the three renderers of icsg3d_amd/csrc/render.hip, written for clarity.

It follows the camera formula and the compositing rule written down in icsg3d_amd/csrc/render.h:

    eye   = ( cos(el) cos(az),  cos(el) sin(az), sin(el))
    right = (-sin(az),          cos(az),         0      )
    up    = (-sin(el) cos(az), -sin(el) sin(az), cos(el))
    p = d sqrt(3) / min(W, H);  u = (i + 0.5 - W/2) p;  v = (H/2 - (j + 0.5)) p
    o = (d/2, d/2, d/2) + u right + v up;   ray(t) = o - t eye

(sine and cosine exact at multiples of 90 degrees).  The volume walk does not step a DDA: it collects every plane crossing
of the ray, sorts them, and finds the voxel of each [t0, t1] segment from its MIDPOINT, so it cannot mis-step on a tie.
One Python loop over the ray's segments, all rays at once.  No early exit.
"""
import math

import numpy as np


def sincos_deg(deg):
    r = math.fmod(float(deg), 360.0)
    q = r / 90.0
    if q == math.floor(q):
        k = int(q) % 4
        return (0.0, 1.0, 0.0, -1.0)[k], (1.0, 0.0, -1.0, 0.0)[k]
    return math.sin(math.radians(r)), math.cos(math.radians(r))


def basis(elev=30.0, azim=-60.0):
    se, ce = sincos_deg(elev)
    sa, ca = sincos_deg(azim)
    eye = np.array([ce * ca, ce * sa, se])
    right = np.array([-sa, ca, 0.0])
    up = np.array([-se * ca, -se * sa, ce])
    return right, up, eye


def pixel_origins(cam, d, W, H):
    """o of every pixel, (H, W, 3), and the eye vector."""
    right, up, eye = basis(*cam)
    p = d * math.sqrt(3.0) / min(W, H)
    u = (np.arange(W) + 0.5 - W / 2.0) * p
    v = (H / 2.0 - (np.arange(H) + 0.5)) * p
    o = d / 2.0 + u[None, :, None] * right + v[:, None, None] * up
    return o, eye


def _walk(o, eye, d, shade):
    """Composite along every ray.  shade(ix, iy, iz) -> (opacity (N,), rgb (N, 3)) for voxel indices (N,)."""
    N = o.shape[0]
    D = -eye
    tmin = np.full(N, -np.inf)
    tmax = np.full(N, np.inf)
    hit = np.ones(N, bool)
    cross = []
    for a in range(3):
        if D[a] != 0.0:
            t = (np.arange(d + 1)[None, :] - o[:, a:a + 1]) / D[a]
            tmin = np.maximum(tmin, t.min(axis=1))
            tmax = np.minimum(tmax, t.max(axis=1))
            cross.append(t)
        else:
            hit &= (o[:, a] >= 0.0) & (o[:, a] < d)
    hit &= tmin < tmax
    ts = np.concatenate(cross, axis=1)
    ts = np.sort(np.clip(ts, np.where(hit, tmin, 0.0)[:, None], np.where(hit, tmax, 0.0)[:, None]), axis=1)
    C = np.zeros((N, 3))
    A = np.zeros(N)
    T = np.ones(N)
    for s in range(ts.shape[1] - 1):
        t0, t1 = ts[:, s], ts[:, s + 1]
        ln = t1 - t0
        mid = o + (0.5 * (t0 + t1))[:, None] * D
        idx = np.clip(np.floor(mid).astype(np.int64), 0, d - 1)
        a, rgb = shade(idx[:, 0], idx[:, 1], idx[:, 2])
        live = hit & (ln > 0.0) & (a > 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            a_eff = np.where(live, 1.0 - np.power(1.0 - np.minimum(a, 1.0), np.where(live, ln, 1.0)), 0.0)
        w = T * a_eff
        C += w[:, None] * rgb
        A += w
        T = T * (1.0 - a_eff)
    return np.concatenate([C, A[:, None]], axis=1)


def lut_index(v):
    """matplotlib's rule for floats: int(v * 256); v == 1 -> 255; v < 0 -> 0; v > 1 -> 255."""
    v = np.asarray(v, np.float64)
    idx = np.floor(v * 256.0)
    idx = np.where(v >= 1.0, 255, idx)
    idx = np.where(v < 0.0, 0, idx)
    return np.nan_to_num(idx).astype(np.int64)


def density(vol, lut, cam=(30.0, -60.0), W=64, H=64, channel=0, mode=0, alpha=0.2, floor=-1.0):
    """vol (B, d, d, d, C) float32 -> (B, H, W, 4) float64."""
    vol = np.asarray(vol)
    B, d = vol.shape[0], vol.shape[1]
    lut = np.asarray(lut, np.float64)
    alpha = float(np.float32(alpha))
    floor = float(np.float32(floor))
    o, eye = pixel_origins(cam, d, W, H)
    out = np.zeros((B, H, W, 4))
    for b in range(B):
        g = vol[b, ..., channel].astype(np.float64)

        def shade(ix, iy, iz, g=g):
            v = g[ix, iy, iz]
            if mode == 0:
                a = np.where(v > floor, alpha, 0.0)
            else:
                a = alpha * np.clip(np.nan_to_num(v), 0.0, 1.0)
            return a, lut[lut_index(v)]

        out[b] = _walk(o.reshape(-1, 3), eye, d, shade).reshape(H, W, 4)
    return out


def labels(lab, palette, cam=(30.0, -60.0), W=64, H=64, alpha=0.5):
    """lab (B, d, d, d) int -> (B, H, W, 4) float64."""
    lab = np.asarray(lab)
    B, d = lab.shape[0], lab.shape[1]
    palette = np.asarray(palette, np.float64)
    alpha = float(np.float32(alpha))
    o, eye = pixel_origins(cam, d, W, H)
    out = np.zeros((B, H, W, 4))
    for b in range(B):
        g = lab[b]

        def shade(ix, iy, iz, g=g):
            k = g[ix, iy, iz]
            return np.where(k > 0, alpha, 0.0), palette[(np.maximum(k, 1) - 1) % len(palette)]

        out[b] = _walk(o.reshape(-1, 3), eye, d, shade).reshape(H, W, 4)
    return out


def atoms(atom_sets, palette, d, cam=(30.0, -60.0), W=64, H=64, radius=1.5):
    """atom_sets: one (species (n,), xyz (n, 3) in voxel units) per sample -> (B, H, W, 4) float64."""
    palette = np.asarray(palette, np.float64)
    o, eye = pixel_origins(cam, d, W, H)
    o = o.reshape(-1, 3)
    out = np.zeros((len(atom_sets), H * W, 4))
    for b, (species, xyz) in enumerate(atom_sets):
        best_t = np.full(len(o), np.inf)
        for sp, c in zip(np.asarray(species).reshape(-1), np.asarray(xyz, np.float64).reshape(-1, 3)):
            q = o - c
            # |q - t eye|^2 = R^2:  t^2 - 2 t (q . eye) + |q|^2 - R^2 = 0, the smaller root is the near hit
            qe = q @ eye
            disc = qe * qe - ((q * q).sum(axis=1) - radius * radius)
            ok = disc > 0.0
            t = qe - np.sqrt(np.where(ok, disc, 0.0))
            win = ok & (t < best_t)
            normal = (q - t[:, None] * eye) / radius
            lambert = np.maximum(0.0, normal @ eye)
            col = palette[int(sp) % len(palette)]
            out[b][win, :3] = lambert[win, None] * col
            out[b][win, 3] = 1.0
            best_t = np.where(win, t, best_t)
    return out.reshape(len(atom_sets), H, W, 4)
