"""The pictures the reference's two train loops draw when the validation loss improves, on the GPU.

U-Net (reference unet/unet.py:39-157, TrainingPlot): plot_segmentations, plot_binary, plot_losses.  VAE (reference
vae/lattice_vae.py:327-337, 359-436): plot_reconstructions, plot_samples, plot_kde, plot_losses.  Three C entry points do
the drawing (include/icsg3d.h, "training monitors"): a colour-mapped slice of a volume where it lies in device memory, the
Gaussian KDE of every latent dimension, and a polyline plot; their formulas are written down in icsg3d_amd/csrc/monitor.h
and `slices`, `Kde` and `line_plot` below are thin wrappers.  Backgrounds, sheets and PNG files are icsg3d_amd.render's.
No text is drawn: every PNG gets a .json sidecar with what a caption would say (ids, value ranges, axis windows).

The monitors run eval-mode inference passes only, none of which runs a collective, and draw their random numbers from
their own np.random.RandomState: weights, BatchNorm moving statistics, the Adam state and training's np.random stream
are left as they were.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os

import numpy as np

from . import _lib as L
from . import render as R

# matplotlib's default colour cycle (tab10), written out
CYCLE = np.array([(31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75),
                  (227, 119, 194), (127, 127, 127), (188, 189, 34), (23, 190, 207)], np.float64) / 255.0
BLACK = np.zeros((1, 3), np.float64)
DTYPES = {np.dtype(np.float32): 0, np.dtype(np.uint8): 1, np.dtype(np.int32): 2}


def _lut(lut):
    lut = np.ascontiguousarray(R.VIRIDIS if lut is None else lut, np.float32)
    if lut.shape != (256, 3):
        raise ValueError("lut must be (256, 3)")
    return lut


def _range(vrange):
    return None if vrange is None else np.ascontiguousarray(vrange, np.float32).reshape(2)


def slices(vol, channel=0, axis=2, index=None, zoom=1, vrange=None, lut=None):
    """imshow(vol[b, :, :, index, channel]) for every b: vol (B, d, d, d[, C]) float32, uint8 or int32 (anything else is
    taken as float32) -> float32 premultiplied RGBA (B, d * zoom, d * zoom, 4).  vrange None: each image's own minimum
    and maximum over its finite values (monitor.h has the colour rule)."""
    vol = np.asarray(vol)
    if vol.dtype not in DTYPES:
        vol = vol.astype(np.float32)
    vol = np.ascontiguousarray(vol)
    if vol.ndim == 4:
        vol = vol[..., None]
    if vol.ndim != 5 or not (vol.shape[1] == vol.shape[2] == vol.shape[3]):
        raise ValueError("vol must be (B, d, d, d[, C]), got %s" % (vol.shape,))
    B, d, nc = vol.shape[0], vol.shape[1], vol.shape[4]
    index = d // 2 if index is None else int(index)
    out = np.empty((B, d * int(zoom), d * int(zoom), 4), np.float32)
    rng = _range(vrange)
    L.check(L.load().ics_op_render_slice(vol.ctypes.data_as(C.c_void_p), DTYPES[vol.dtype], B, d, nc, int(channel),
                                         int(axis), index, L.fptr(_lut(lut)), L.fptr(rng), int(zoom), L.fptr(out)))
    return out


def resident_slices(engine, which, count, channel=0, axis=2, index=None, zoom=1, vrange=None, lut=None):
    """`slices` of the first `count` samples of what a UnetEngine or VaeEngine holds, read where it lies (which: see
    ics_vae_render_slice_resident / ics_unet_render_slice_resident); the bits `slices` gives for the same values."""
    from .engine import VaeEngine
    d = engine.d
    index = d // 2 if index is None else int(index)
    out = np.empty((int(count), d * int(zoom), d * int(zoom), 4), np.float32)
    lib = L.load()
    fn = lib.ics_vae_render_slice_resident if isinstance(engine, VaeEngine) else lib.ics_unet_render_slice_resident
    L.check(fn(engine._h, int(which), int(channel), int(count), int(axis), index, L.fptr(_lut(lut)),
               L.fptr(_range(vrange)), int(zoom), L.fptr(out)))
    return out


class Kde:
    """scipy.stats.gaussian_kde of every column of the appended codes at once (ics_op_kde_*): Scott's bandwidth, fp64."""

    def __init__(self, dim, capacity):
        self._lib = L.load()
        self._h = C.c_void_p()
        self.dim, self.capacity = int(dim), int(capacity)
        L.check(self._lib.ics_op_kde_create(self.dim, self.capacity, C.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.ics_op_kde_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def append(self, codes):
        codes = np.ascontiguousarray(codes, np.float32)
        if codes.ndim != 2 or codes.shape[1] != self.dim:
            raise ValueError("codes must be (rows, %d), got %s" % (self.dim, codes.shape))
        L.check(self._lib.ics_op_kde_append(self._h, L.fptr(codes), codes.shape[0]))

    def append_vae(self, engine, batch, which="z"):
        """`batch` rows of what the VaeEngine's last encoder pass left, device to device: which "z_mean" or "z" (sampled)."""
        if which not in ("z_mean", "z"):
            raise ValueError("which must be 'z_mean' or 'z'")
        L.check(self._lib.ics_op_kde_append_vae(self._h, engine._h, int(batch), 1 if which == "z" else 0))

    def evaluate(self, x):
        """x (npts,) -> density (dim, npts) float64, bandwidth (dim,), status (dim,) int32 (1: a collapsed dimension,
        its row NaN), count."""
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
        dens = np.empty((self.dim, len(x)), np.float64)
        bw = np.empty(self.dim, np.float64)
        status = np.empty(self.dim, np.int32)
        n = C.c_int(0)
        L.check(self._lib.ics_op_kde_evaluate(self._h, L.f64ptr(x), len(x), L.f64ptr(dens), L.f64ptr(bw), L.i32ptr(status),
                                              C.byref(n)))
        return dens, bw, status, n.value


def line_plot(curves, window, size=(640, 480), width_px=1.5, alpha=1.0, palette=None):
    """curves (ncurves, npts, 2) float64 in data units, NaN breaks a line -> float32 premultiplied RGBA (height, width,
    4); window (x0, x1, y0, y1) maps onto the picture, curve k in palette[k % len(palette)] (monitor.h)."""
    xy = np.ascontiguousarray(curves, np.float64)
    if xy.ndim != 3 or xy.shape[2] != 2:
        raise ValueError("curves must be (ncurves, npts, 2), got %s" % (xy.shape,))
    w, h = R._size(size)
    win = np.ascontiguousarray(window, np.float64).reshape(4)
    pal = np.ascontiguousarray(CYCLE if palette is None else palette, np.float32).reshape(-1, 3)
    out = np.empty((h, w, 4), np.float32)
    L.check(L.load().ics_op_render_lines(L.f64ptr(xy), xy.shape[0], xy.shape[1], L.f64ptr(win), L.fptr(pal), len(pal),
                                         float(width_px), float(alpha), w, h, L.fptr(out)))
    return out


# ---------------------------------------------------------------- axes without text
def ticks_125(lo, hi, nticks=5):
    """Tick positions in [lo, hi] at a step of 1, 2 or 5 times a power of ten: the smallest such step that gives at most
    `nticks` intervals."""
    lo, hi = float(min(lo, hi)), float(max(lo, hi))
    if not (math.isfinite(lo) and math.isfinite(hi)) or hi == lo or nticks < 1:
        return []
    raw = (hi - lo) / nticks
    e = math.floor(math.log10(raw))
    m = next((m for m in (1, 2, 5, 10) if m * 10.0 ** e >= raw * (1 - 1e-12)), 10)
    if m == 10:
        m, e = 1, e + 1

    def at(k):      # k * m * 10^e, the power applied as a division where e < 0 so that 0.1 steps come out as 0.1, 0.2, ...
        return k * m * 10.0 ** e if e >= 0 else k * m / 10.0 ** (-e)
    k0, k1 = math.ceil(lo / at(1) - 1e-9), math.floor(hi / at(1) + 1e-9)
    return [at(k) for k in range(k0, k1 + 1)]


def pad_curves(curves, npts=None):
    """Polylines of different lengths [(n_k, 2)] -> one (ncurves, npts, 2) array, NaN-padded (a NaN point draws nothing)."""
    curves = [np.asarray(c, np.float64).reshape(-1, 2) for c in curves]
    npts = max([2, npts or 0] + [len(c) for c in curves])
    out = np.full((len(curves), npts, 2), np.nan)
    for k, c in enumerate(curves):
        out[k, :len(c)] = c
    return out


def axes_curves(window, nticks=5, tick_frac=0.015):
    """The frame of `window` = (x0, x1, y0, y1) and its tick marks as NaN-padded polylines (1 + ticks, 5, 2): the frame
    first, then one short stroke per 1-2-5 tick, inwards from the bottom and the left edge.  Returns (curves, xticks,
    yticks)."""
    x0, x1, y0, y1 = (float(v) for v in window)
    frame = [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]
    xt, yt = ticks_125(x0, x1, nticks), ticks_125(y0, y1, nticks)
    lx, ly = tick_frac * (x1 - x0), tick_frac * (y1 - y0)
    strokes = [[(t, y0), (t, y0 + ly)] for t in xt] + [[(x0, t), (x0 + lx, t)] for t in yt]
    return pad_curves([frame] + strokes, 5), xt, yt


def plot_with_axes(curves, window, size=(640, 480), width_px=1.5, alpha=1.0, palette=None, nticks=5, margin=24):
    """line_plot of `curves` with a black frame and tick marks, over white, with `margin` white pixels around the plot
    area -> uint8 (height, width, 3), and (xticks, yticks) for the sidecar."""
    w, h = R._size(size)
    pw, ph = w - 2 * margin, h - 2 * margin
    if pw < 1 or ph < 1:
        raise ValueError("size %s leaves no room inside a margin of %d" % ((w, h), margin))
    data = line_plot(curves, window, (pw, ph), width_px, alpha, palette).astype(np.float64)
    ax, xt, yt = axes_curves(window, nticks)
    frame = line_plot(ax, window, (pw, ph), 1.0, 1.0, BLACK).astype(np.float64)
    rgba = frame + (1.0 - frame[..., 3:4]) * data                 # the frame over the curves
    out = np.full((h, w, 3), 255, np.uint8)
    out[margin:margin + ph, margin:margin + pw] = R.over(rgba)
    return out, xt, yt


def _window(xs, ys, pad=0.05):
    """An axis window around finite data, `pad` of the span on every side; a flat range is widened to be drawable."""
    xs, ys = np.asarray(xs, np.float64), np.asarray(ys, np.float64)
    xs, ys = xs[np.isfinite(xs)], ys[np.isfinite(ys)]
    out = []
    for v in (xs, ys):
        lo, hi = (float(v.min()), float(v.max())) if len(v) else (0.0, 1.0)
        if hi == lo:
            lo, hi = lo - 0.5, hi + 0.5
        out += [lo - pad * (hi - lo), hi + pad * (hi - lo)]
    return tuple(out)


def _write(sdir, stem, rgb, meta):
    os.makedirs(sdir, exist_ok=True)
    R.write_png(os.path.join(sdir, stem + ".png"), rgb)
    with open(os.path.join(sdir, stem + ".json"), "w") as f:
        json.dump(meta, f, indent=1)


def _ids(gen, n):
    ids = getattr(gen, "list_IDs_temp", None)
    return [str(i) for i in list(ids)[:n]] if ids is not None else []


def _finite_range(a):
    a = np.asarray(a, np.float64)
    a = a[np.isfinite(a)]
    return [float(a.min()), float(a.max())] if a.size else [None, None]


def loss_plot(sdir, stem, series, names, size=(640, 480)):
    """plot_losses: the named series against the epoch index, one PNG and its sidecar."""
    series = [np.asarray([np.nan if v is None else v for v in s], np.float64) for s in series]
    n = max(len(s) for s in series)
    curves = pad_curves([np.stack([np.arange(len(s), dtype=np.float64), s], axis=1) for s in series], n)
    win = _window([0.0, max(n - 1, 1)], np.concatenate(series), pad=0.05)
    rgb, xt, yt = plot_with_axes(curves, win, size)
    _write(sdir, stem, rgb, {"series": names, "epochs": n, "window": list(win), "xticks": xt, "yticks": yt,
                             "colours": [[float(c) for c in CYCLE[k % len(CYCLE)]] for k in range(len(series))],
                             "last": [None if not len(s) or not np.isfinite(s[-1]) else float(s[-1]) for s in series]})


class UnetMonitor:
    """TrainingPlot's pictures (unet/unet.py:39-157) as a fit_generator callback.  On a new best val_loss:
    segmentations_best.png (true species slice | argmax species slice) and segmentations_binary_best.png (occupancy
    target | sigmoid output), each 10 rows x 2 columns: the first sample of each of the first 10 validation batches at
    plane d // 2 of axis 2, true on the left.  Every epoch: unet_loss.png.  `model` is the AtomUnet."""

    rows = 10

    def __init__(self, val_gen, sdir, model=None, zoom=4):
        self.val_gen, self.sdir, self.model, self.zoom = val_gen, sdir, model, int(zoom)
        self.min_val_loss = np.inf
        self.losses, self.val_losses = [], []

    def set_model(self, model):
        self.model = model

    def on_epoch_end(self, epoch, logs=None):
        logs = logs or {}
        self.losses.append(logs.get("loss"))
        self.val_losses.append(logs.get("val_loss"))
        v = self.val_losses[-1]
        if v is not None and v < self.min_val_loss:
            self.min_val_loss = v
            self.draw_sheets(epoch)
        loss_plot(self.sdir, "unet_loss", [self.losses, self.val_losses], ["train_loss", "val_loss"])

    def draw_sheets(self, epoch=None):
        from .unet.unet import _to_labels
        seg, binary, ids, ranges = [], [], [], []
        nc = self.model.num_classes
        for i in range(min(self.rows, len(self.val_gen))):
            X, y = self.val_gen[i]
            X = np.asarray(X, np.float32)[:1]                        # the batch's first sample (eval mode: its output
            lab = _to_labels(y[0] if isinstance(y, (list, tuple)) else y, nc)[:1]   # does not depend on the batch)
            eng = self.model._engine(1)
            eng.upload_batch(X, lab)
            true = resident_slices(eng, 3, 1, zoom=self.zoom)[0]
            # the occupancy target is labels != 0 (unet/data.py:87): the same slice with every class above 0 at the top
            occ = resident_slices(eng, 3, 1, zoom=self.zoom, vrange=(0.0, 1.0))[0]
            eng.predict_resident(labels_only=True)
            pred = resident_slices(eng, 1, 1, zoom=self.zoom)[0]
            eng.predict_resident(labels_only=False)
            prob = resident_slices(eng, 2, 1, zoom=self.zoom)[0]
            seg += [true, pred]
            binary += [occ, prob]
            ids += _ids(self.val_gen, 1)
            d = X.shape[1]
            ranges.append(_finite_range(lab[0, :, :, d // 2]))
        if not seg:
            return
        n = len(seg) // 2
        meta = {"epoch": epoch, "val_loss": None if not np.isfinite(self.min_val_loss) else float(self.min_val_loss),
                "rows": n, "columns": ["true", "predicted"], "ids": ids, "axis": 2, "plane": "d // 2", "zoom": self.zoom,
                "colour_range": "each slice's own minimum and maximum"}
        _write(self.sdir, "segmentations_best", R.sheet([R.over(p) for p in seg], n, 2),
               dict(meta, true_label_range=ranges))
        _write(self.sdir, "segmentations_binary_best", R.sheet([R.over(p) for p in binary], n, 2),
               dict(meta, columns=["occupancy target (labels != 0)", "sigmoid output"]))


class VaeMonitor:
    """The VAE train loop's pictures (vae/lattice_vae.py:327-337, 359-436).  `best()` on a new best validation loss:
    vae_reconstructions.png (input | reconstruction, batch_size // 2 rows, mid slice of channel 0), vae_samples.png
    (decoded prior samples in pairs, at most 10 rows) and vae_kde.png / .svg / .json (the KDE of every latent dimension
    over the SAMPLED z of validation batches until >= maxz codes, on linspace(-3, 3, 50): the picture that shows
    posterior collapse).  `losses()` every 10 epochs: vae_losses.png.  All random draws come from RandomState(seed)."""

    maxz, npts = 1000, 50

    def __init__(self, vae, val_gen, sdir, seed=0, zoom=4):
        self.vae, self.val_gen, self.sdir, self.zoom = vae, val_gen, sdir, int(zoom)
        self.rng = np.random.RandomState(seed)

    def best(self, epoch=None):
        self.reconstructions(epoch)
        self.samples(epoch)
        self.kde(epoch)

    def reconstructions(self, epoch=None):
        vae = self.vae
        M, cond = self.val_gen[0][:2]
        eng = vae._engine(len(M))
        M, cond = np.asarray(M, np.float32)[:eng.max_batch], np.asarray(cond, np.float32)[:eng.max_batch]
        eps = self.rng.normal(size=(len(M), vae.latent_dim))
        _, _, z = eng.encode(M, cond, eps)
        eng.decode(z, cond)                                         # leaves the reconstruction where it is drawn from
        n = max(len(M) // 2, 1)
        left = resident_slices(eng, 0, n, zoom=self.zoom)
        right = resident_slices(eng, 1, n, zoom=self.zoom)
        panels = [p for pair in zip(left, right) for p in pair]
        _write(self.sdir, "vae_reconstructions", R.sheet([R.over(p) for p in panels], n, 2),
               {"epoch": epoch, "rows": n, "columns": ["input", "reconstruction"], "ids": _ids(self.val_gen, n), "axis": 2,
                "plane": "d // 2", "channel": 0, "zoom": self.zoom, "colour_range": "each slice's own minimum and maximum",
                "input_range": [_finite_range(M[i, :, :, M.shape[1] // 2, 0]) for i in range(n)]})

    def samples(self, epoch=None):
        """sample_vae(batch_size) with this monitor's own draws (training's np.random stream is not touched)."""
        vae = self.vae
        bs = int(vae.batch_size or self.val_gen.batch_size)
        cond = self.rng.randint(low=0, high=vae.cond_shape, size=bs)
        onehot = np.zeros((bs, vae.cond_shape), np.float32)
        onehot[np.arange(bs), cond] = 1.0
        z = self.rng.normal(0, 1.0, size=(bs, vae.latent_dim))
        vol = vae.decoder.predict([z, onehot])
        n = min(max(bs // 2, 1), 10)
        pics = slices(vol[:2 * n] if bs >= 2 else vol, channel=0, zoom=self.zoom)
        cols = 2 if len(pics) >= 2 * n and bs >= 2 else 1
        _write(self.sdir, "vae_samples", R.sheet([R.over(p) for p in pics[:n * cols]], n, cols),
               {"epoch": epoch, "rows": n, "columns": cols, "cond_bins": [int(c) for c in cond[:n * cols]], "axis": 2,
                "plane": "d // 2", "channel": 0, "zoom": self.zoom, "colour_range": "each slice's own minimum and maximum"})

    def kde(self, epoch=None):
        vae = self.vae
        bs = int(self.val_gen.batch_size)
        steps = len(self.val_gen.list_IDs) // bs
        if getattr(self.val_gen, "augment", None) is not None:      # an augmented generator's epoch is its plan
            steps = len(self.val_gen)
        if steps < 1:
            return
        need = -(-self.maxz // bs)                                  # batches until >= maxz codes, wrapping as the reference
        kde = Kde(vae.latent_dim, need * bs)
        try:
            for k in range(need):
                M, cond = self.val_gen[k % steps][:2]
                eng = vae._engine(len(M))
                eps = self.rng.normal(size=(len(M), vae.latent_dim))
                for i in range(0, len(M), eng.max_batch):           # one encoder pass per resident batch
                    s = slice(i, i + eng.max_batch)
                    eng.encode(M[s], cond[s], eps[s])
                    kde.append_vae(eng, len(M[s]), "z")
            x = np.linspace(-3, 3, self.npts)
            dens, bw, status, count = kde.evaluate(x)
        finally:
            kde.close()
        ok = status == 0
        top = float(dens[ok].max()) if ok.any() and np.isfinite(dens[ok]).any() else 1.0
        win = (-3.0, 3.0, 0.0, 1.05 * top if top > 0 else 1.0)
        curves = np.stack([np.broadcast_to(x, dens.shape), dens], axis=2)
        rgb, xt, yt = plot_with_axes(curves, win, alpha=0.6)
        meta = {"epoch": epoch, "x": [float(v) for v in x], "count": int(count), "bandwidth": [float(v) for v in bw],
                "status": [int(s) for s in status], "collapsed": int((status != 0).sum()), "window": list(win),
                "y_range": [win[2], win[3]], "xticks": xt, "yticks": yt}
        _write(self.sdir, "vae_kde", rgb, meta)
        with open(os.path.join(self.sdir, "vae_kde.svg"), "w") as f:
            f.write(kde_svg(x, dens, status, win))

    def losses(self, losses, epochs_done):
        arr = np.asarray(losses, np.float64)[:epochs_done]
        loss_plot(self.sdir, "vae_losses", [arr[:, 0], arr[:, 1]], ["train_loss", "val_loss"])


def kde_svg(x, dens, status, window, size=(640, 480)):
    """The KDE curves as an SVG of polylines in the colour cycle (no text), window as `line_plot` maps it."""
    w, h = size
    x0, x1, y0, y1 = window
    parts = ['<svg xmlns="http://www.w3.org/2000/svg" width="%d" height="%d" viewBox="0 0 %d %d">' % (w, h, w, h),
             '<rect width="%d" height="%d" fill="white" stroke="black"/>' % (w, h)]
    px = (np.asarray(x, np.float64) - x0) / (x1 - x0) * w
    for j in range(len(dens)):
        if status[j]:
            continue
        py = (1.0 - (dens[j] - y0) / (y1 - y0)) * h
        c = (CYCLE[j % len(CYCLE)] * 255).astype(int)
        pts = " ".join("%.2f,%.2f" % (a, b) for a, b in zip(px, py))
        parts.append('<polyline fill="none" stroke="rgb(%d,%d,%d)" stroke-opacity="0.6" stroke-width="1.5" points="%s"/>'
                     % (c[0], c[1], c[2], pts))
    parts.append("</svg>")
    return "\n".join(parts)
