"""numpy restatement of the three formulas of icsg3d_amd/csrc/monitor.h: the slice colour index in float32, the
per-dimension Gaussian KDE and the polyline plot in float64.  The formulas are written down there; this file repeats them
so that the GPU tests have something to compare with."""
import numpy as np


def slice_plane(vol, channel, axis, index):
    """vol (B, d, d, d, C) -> the planes (B, d, d): row and column are the two remaining axes in array order."""
    v = np.asarray(vol)[..., channel]
    return np.take(v, index, axis=axis + 1)


def slice_index(plane, vrange=None):
    """One plane (d, d) -> (colour index int (d, d), finite mask, t * 256 as float32) by the SLICE rule, in float32."""
    v = np.asarray(plane).astype(np.float32)
    fin = np.isfinite(v)
    if vrange is None:
        if not fin.any():
            return np.zeros(v.shape, np.int64), fin, np.zeros(v.shape, np.float32)
        vmin, vmax = v[fin].min(), v[fin].max()
    else:
        vmin, vmax = np.float32(vrange[0]), np.float32(vrange[1])
    if vmax == vmin:
        return np.zeros(v.shape, np.int64), fin, np.zeros(v.shape, np.float32)
    with np.errstate(all="ignore"):
        t = (np.where(fin, v, vmin) - vmin) / (vmax - vmin)
        t256 = (t * np.float32(256.0)).astype(np.float32)
        idx = np.where(~(t >= 0), 0, np.where(t >= 1, 255, np.minimum(255, np.clip(t256, 0, 300).astype(np.int64))))
    assert t.dtype == np.float32
    return idx, fin, t256


def slice_rgba(vol, channel, axis, index, zoom, lut, vrange=None):
    """The op's picture: float32 premultiplied RGBA (B, d zoom, d zoom, 4)."""
    planes = slice_plane(vol, channel, axis, index)
    lut = np.asarray(lut, np.float32)
    out = []
    for p in planes:
        idx, fin, _ = slice_index(p, vrange)
        rgba = np.concatenate([lut[idx], np.ones(idx.shape + (1,), np.float32)], axis=-1) * fin[..., None]
        out.append(np.repeat(np.repeat(rgba, zoom, axis=0), zoom, axis=1))
    return np.stack(out).astype(np.float32)


def kde(z, x):
    """z (n, dim) float32 codes, x (npts,) -> density (dim, npts), bandwidth (dim,), status (dim,), all by the KDE rule
    in float64: two-pass variance, Scott's factor n^(-1/5), status 1 and a NaN row where h2 == 0 or is not finite."""
    z = np.asarray(z, np.float32).astype(np.float64)
    x = np.asarray(x, np.float64)
    n, dim = z.shape
    mean = z.sum(axis=0) / n
    var = ((z - mean) ** 2).sum(axis=0) / (n - 1)
    f = float(n) ** (-1.0 / 5.0)
    h2 = var * (f * f)
    status = ((h2 == 0) | ~np.isfinite(h2)).astype(np.int32)
    dens = np.full((dim, len(x)), np.nan)
    for j in np.nonzero(status == 0)[0]:
        dv = x[:, None] - z[None, :, j]
        dens[j] = np.exp(-(dv * dv) / (2.0 * h2[j])).sum(axis=1) / (n * np.sqrt(2.0 * np.pi * h2[j]))
    with np.errstate(invalid="ignore"):
        return dens, np.sqrt(h2), status


def lines(xy, window, palette, width_px, alpha, width, height):
    """xy (ncurves, npts, 2) -> float32 premultiplied RGBA (height, width, 4) by the LINES rule in float64."""
    xy = np.asarray(xy, np.float64)
    x0, x1, y0, y1 = (float(v) for v in window)
    pal = np.asarray(palette, np.float32).astype(np.float64).reshape(-1, 3)
    reach = width_px / 2.0 + 0.5
    a_ = float(np.float32(alpha))
    with np.errstate(all="ignore"):
        px = (xy[..., 0] - x0) / (x1 - x0) * width
        py = (1.0 - (xy[..., 1] - y0) / (y1 - y0)) * height
    cx = (np.arange(width) + 0.5)[None, :]
    cy = (np.arange(height) + 0.5)[:, None]
    C = np.zeros((height, width, 3))
    A = np.zeros((height, width))
    for c in range(len(xy)):
        ax, ay, bx, by = px[c, :-1], py[c, :-1], px[c, 1:], py[c, 1:]
        ok = np.isfinite(ax) & np.isfinite(ay) & np.isfinite(bx) & np.isfinite(by)
        cov = np.zeros((height, width))
        for s in np.nonzero(ok)[0]:
            ex, ey = bx[s] - ax[s], by[s] - ay[s]
            ee = ex * ex + ey * ey
            if ee != 0.0:
                t = np.clip(((cx - ax[s]) * ex + (cy - ay[s]) * ey) / ee, 0.0, 1.0)
            else:
                t = np.zeros((height, width))
            qx, qy = cx - (ax[s] + t * ex), cy - (ay[s] + t * ey)
            cov = np.maximum(cov, np.clip(reach - np.sqrt(qx * qx + qy * qy), 0.0, 1.0))
        w = a_ * cov
        C = w[..., None] * pal[c % len(pal)] + (1.0 - w[..., None]) * C
        A = w + (1.0 - w) * A
    return np.concatenate([C, A[..., None]], axis=-1).astype(np.float32)
