"""Pictures of the pipeline's volumes (reference view_results.py:152-183, viz.py:43-66, 184-233), ray cast on the GPU.

The three renderers are C entry points (include/icsg3d.h: ics_op_render_density / _labels / _atoms); the camera and the
compositing rule are written down in icsg3d_amd/csrc/render.h, and `basis` / `pixel_origins` below restate the camera
for callers that want to place something in a picture.  Everything after the float RGBA -- the background, the sheet of
panels, the PNG file -- is plain numpy, zlib and struct: matplotlib and PIL are not needed at run time.
"""
from __future__ import annotations

import ctypes as C
import math
import struct
import zlib

import numpy as np

from . import _lib as L
from ._viridis import VIRIDIS_DATA

VIRIDIS = np.array(VIRIDIS_DATA, np.float64)             # cm.viridis(np.arange(256))[:, :3]
TAB10 = np.array([(31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75),
                  (227, 119, 194), (127, 127, 127), (188, 189, 34), (23, 190, 207)], np.float64) / 255.0
MODES = {"flat": 0, "value": 1}


def camera(elev=30.0, azim=-60.0):
    """(elev, azim) in degrees as matplotlib's 3-D axes define them: what every renderer takes as `cam`."""
    cam = np.array([elev, azim], np.float64)
    if not np.isfinite(cam).all():
        raise ValueError("camera angles must be finite")
    return cam


def _sincos_deg(deg):
    r = math.fmod(float(deg), 360.0)
    q = r / 90.0
    if q == math.floor(q):                 # exact at the multiples of 90 degrees (render.h)
        k = int(q) % 4
        return (0.0, 1.0, 0.0, -1.0)[k], (1.0, 0.0, -1.0, 0.0)[k]
    return math.sin(math.radians(r)), math.cos(math.radians(r))


def basis(cam):
    """right, up, eye of the camera (render.h): image x, image y, and the direction from the grid centre to the viewer."""
    se, ce = _sincos_deg(cam[0])
    sa, ca = _sincos_deg(cam[1])
    return (np.array([-sa, ca, 0.0]), np.array([-se * ca, -se * sa, ce]), np.array([ce * ca, ce * sa, se]))


def pixel_origins(cam, d, width, height):
    """o of every pixel centre, (height, width, 3) in voxel units; the pixel's ray is o - t eye (render.h)."""
    right, up, _ = basis(cam)
    p = d * math.sqrt(3.0) / min(width, height)
    u = (np.arange(width) + 0.5 - width / 2.0) * p
    v = (height / 2.0 - (np.arange(height) + 0.5)) * p
    return d / 2.0 + u[None, :, None] * right + v[:, None, None] * up


def _mode(mode):
    if mode in MODES:
        return MODES[mode]
    if mode in (0, 1):
        return int(mode)
    raise ValueError("mode must be 'flat' (0) or 'value' (1), got %r" % (mode,))


def _size(size):
    w, h = (size, size) if np.isscalar(size) else size
    return int(w), int(h)


def _cam(cam):
    return camera() if cam is None else camera(*cam)


def density(vol, channel=0, cam=None, size=256, mode="value", alpha=0.2, floor=-1.0, lut=None):
    """vol (B, d, d, d[, C]) float -> float32 premultiplied RGBA (B, height, width, 4).  mode 'flat': every voxel above
    `floor` at opacity alpha (floor < 0: the reference's picture); 'value': opacity alpha * clip(v, 0, 1)."""
    vol = np.ascontiguousarray(vol, np.float32)
    if vol.ndim == 4:
        vol = vol[..., None]
    if vol.ndim != 5 or not (vol.shape[1] == vol.shape[2] == vol.shape[3]):
        raise ValueError("vol must be (B, d, d, d[, C]), got %s" % (vol.shape,))
    B, d, nc = vol.shape[0], vol.shape[1], vol.shape[4]
    w, h = _size(size)
    cam = _cam(cam)
    lut = np.ascontiguousarray(VIRIDIS if lut is None else lut, np.float32)
    if lut.shape != (256, 3):
        raise ValueError("lut must be (256, 3)")
    out = np.empty((B, h, w, 4), np.float32)
    L.check(L.load().ics_op_render_density(L.fptr(vol), B, d, nc, int(channel), L.fptr(lut), _mode(mode), float(alpha),
                                           float(floor), L.f64ptr(cam), w, h, L.fptr(out)))
    return out


def labels(vol, cam=None, size=256, alpha=0.5, palette=None):
    """vol (B, d, d, d) integer labels, 0 empty -> RGBA; label k in palette[(k - 1) % len(palette)] at opacity alpha."""
    vol = np.ascontiguousarray(vol, np.int32)                 # uint8 species / mask volumes are widened here
    if vol.ndim != 4 or not (vol.shape[1] == vol.shape[2] == vol.shape[3]):
        raise ValueError("labels must be (B, d, d, d), got %s" % (vol.shape,))
    B, d = vol.shape[0], vol.shape[1]
    w, h = _size(size)
    cam = _cam(cam)
    pal = np.ascontiguousarray(TAB10 if palette is None else palette, np.float32).reshape(-1, 3)
    out = np.empty((B, h, w, 4), np.float32)
    L.check(L.load().ics_op_render_labels(L.i32ptr(vol), B, d, L.fptr(pal), len(pal), float(alpha), L.f64ptr(cam), w, h,
                                          L.fptr(out)))
    return out


def pack_atoms(atom_sets):
    """[(species (n,), xyz (n, 3))] -> offsets (B + 1,) int32, species int32, xyz float64: ics_op_structure_screen's layout."""
    offsets = np.zeros(len(atom_sets) + 1, np.int32)
    sp, xyz = [], []
    for b, (s, x) in enumerate(atom_sets):
        s = np.asarray(s, np.int32).reshape(-1)
        x = np.asarray(x, np.float64).reshape(-1, 3)
        if len(s) != len(x):
            raise ValueError("sample %d: %d species for %d positions" % (b, len(s), len(x)))
        offsets[b + 1] = offsets[b] + len(s)
        sp.append(s)
        xyz.append(x)
    sp = np.ascontiguousarray(np.concatenate(sp) if sp else np.zeros(0), np.int32)
    xyz = np.ascontiguousarray(np.concatenate(xyz) if xyz else np.zeros((0, 3)), np.float64)
    return offsets, sp, xyz


def atoms(atom_sets, d, cam=None, size=256, radius=1.5, palette=None):
    """atom_sets [(species, xyz in voxel units)] -> RGBA: one Lambert-shaded sphere of `radius` voxels per atom."""
    offsets, sp, xyz = pack_atoms(atom_sets)
    w, h = _size(size)
    cam = _cam(cam)
    pal = np.ascontiguousarray(TAB10 if palette is None else palette, np.float32).reshape(-1, 3)
    out = np.empty((len(atom_sets), h, w, 4), np.float32)
    L.check(L.load().ics_op_render_atoms(L.i32ptr(offsets), L.i32ptr(sp), L.f64ptr(xyz), len(atom_sets), int(d),
                                         float(radius), L.fptr(pal), len(pal), L.f64ptr(cam), w, h, L.fptr(out)))
    return out


# ---------------------------------------------------------------- after the GPU: background, sheet, file
def over(rgba, background=1.0):
    """Premultiplied float RGBA (..., H, W, 4) over a flat background -> uint8 (..., H, W, 3)."""
    rgba = np.asarray(rgba, np.float64)
    rgb = rgba[..., :3] + (1.0 - rgba[..., 3:4]) * np.asarray(background, np.float64)
    return np.clip(np.rint(rgb * 255.0), 0, 255).astype(np.uint8)


def sheet(panels, rows, cols, pad=4, background=255):
    """uint8 (H, W, 3) panels of one size, row-major, into one rows x cols image with `pad` pixels around each."""
    panels = [np.asarray(p, np.uint8) for p in panels]
    if not panels or len(panels) > rows * cols:
        raise ValueError("%d panels do not fit %d x %d" % (len(panels), rows, cols))
    h, w = panels[0].shape[:2]
    if any(p.shape != (h, w, 3) for p in panels):
        raise ValueError("panels must share one (H, W, 3) shape")
    out = np.full((rows * (h + pad) + pad, cols * (w + pad) + pad, 3), background, np.uint8)
    for k, p in enumerate(panels):
        r, c = divmod(k, cols)
        y, x = pad + r * (h + pad), pad + c * (w + pad)
        out[y:y + h, x:x + w] = p
    return out


def png_bytes(rgb):
    """uint8 (H, W, 3) as an 8-bit RGB PNG: filter 0 on every row, one IDAT."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("rgb must be (H, W, 3) uint8")
    h, w = rgb.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rgb.reshape(h, w * 3)], axis=1).tobytes()

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def write_png(path, rgb):
    with open(path, "wb") as f:
        f.write(png_bytes(rgb))
