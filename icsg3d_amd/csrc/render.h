// Declarations for render.hip: pictures of the volumes the pipeline already holds (reference viz.py:43-66 plot_points_3d,
// viz.py:184-233 the voxel panels, view_results.py:152-183 the eight-panel sheet), ray cast at full resolution instead of
// one matplotlib polygon set per voxel.  Three renderers -- density, labels, atoms -- share ONE camera and, for the two
// volume renderers, ONE compositing rule; both are written down here once and nowhere else.  icsg3d_amd/render.py and
// tests/render_ref.py restate them and say so.
//
// CAMERA.  Orthographic, W x H pixels, looking at the grid centre c = (d/2, d/2, d/2).  Array axis 0 is x, axis 1 is y,
// axis 2 is z; z is up.  With elev and azim in degrees as matplotlib's 3-D axes define them (defaults 30, -60):
//     eye   = ( cos(el) cos(az),  cos(el) sin(az), sin(el))      from the centre towards the viewer
//     right = (-sin(az),          cos(az),         0      )      image x
//     up    = (-sin(el) cos(az), -sin(el) sin(az), cos(el))      image y;  right x up = eye
// The sine and cosine of a multiple of 90 degrees are taken as exactly 0 and +-1, so an axis-aligned view has exact zeros
// in its ray direction.  The image plane is a square of side d sqrt(3) (the cube's diagonal: the cube fits at any angle)
// mapped onto the SHORTER image side; pixels are square, so the longer side sees a padding strip beyond the square:
//     p = d sqrt(3) / min(W, H)                                  pixel size in voxel units
//     u = (i + 0.5 - W/2) p,   v = (H/2 - (j + 0.5)) p           pixel (column i, row j), row 0 at the top
//     o = c + u right + v up,  ray(t) = o - t eye,  t in (-inf, +inf)
// t is a length in voxel units (|eye| = 1); t = 0 is the plane through the centre, so |t| <= d sqrt(3) / 2 inside the cube.
//
// COMPOSITING (density, labels).  The ray's voxels are visited in order: slab entry / exit of [0, d]^3, then a 3-D DDA whose
// next crossing per axis is (plane - o) / dir from the integer plane index (no accumulated step).  A crossing of length l
// through a voxel of opacity a and colour rgb adds
//     a_eff = 1 - (1 - a)^l,   C += T a_eff rgb,   A += T a_eff,   T *= 1 - a_eff        (T starts at 1)
// Path-length weighting makes the image continuous in the ray position: a ray that grazes a voxel contributes almost
// nothing, so a walk that rounds a corner crossing differently (fp32 here, fp64 in the test reference) differs by the
// rounding, not by a voxel.  The walk may stop once T < 1e-5.  Output: float32 premultiplied RGBA in [0, 1].
#pragma once
#include "common.h"

#include <cmath>

namespace ics {

constexpr int kRenderMaxGrid = 256;
constexpr int kRenderMaxImage = 4096;
constexpr int kRenderMaxBatch = 65535;   // one grid z-slice per image
constexpr float kRenderMinT = 1e-5f;     // early exit below this transmittance
constexpr int kRenderLutRows = 256;

// The camera of one launch in the arithmetic type of its renderer (float: the volume walks; double: the spheres).
template <typename T>
struct RenderView {
  T right[3], up[3], eye[3];
  T pix, half_w, half_h, centre;
};

// o of pixel (i, j): the formula above
template <typename T>
__host__ __device__ inline void render_pixel_origin(const RenderView<T>& V, int i, int j, T o[3]) {
  const T u = ((T)i + (T)0.5 - V.half_w) * V.pix;
  const T v = (V.half_h - ((T)j + (T)0.5)) * V.pix;
  for (int a = 0; a < 3; ++a) o[a] = V.centre + u * V.right[a] + v * V.up[a];
}

// One voxel's contribution; log1m_a = log(1 - a) (-inf for an opaque voxel), len > 0.
__host__ __device__ inline void render_composite(float len, float log1m_a, const float rgb[3], float& T, float C[3],
                                                 float& A) {
  const float a_eff = -expm1f(len * log1m_a);
  const float w = T * a_eff;
  C[0] += w * rgb[0]; C[1] += w * rgb[1]; C[2] += w * rgb[2];
  A += w;
  T *= 1.f - a_eff;
}

// The walk of pixel (i, j) through a d^3 grid.  shade(x, y, z, &log1m_a, rgb) returns false for an empty voxel.
template <typename Shade>
__host__ __device__ inline void render_walk(const RenderView<float>& V, int d, int i, int j, const Shade& shade,
                                            float out[4]) {
  const float kInf = __builtin_huge_valf();
  float o[3];
  render_pixel_origin(V, i, j, o);
  const float fd = (float)d;
  const float dx = -V.eye[0], dy = -V.eye[1], dz = -V.eye[2];
  const float D[3] = {dx, dy, dz};
  float inv[3], tmin = -kInf, tmax = kInf;
  bool hit = true;
  for (int a = 0; a < 3; ++a) {
    if (D[a] != 0.f) {
      inv[a] = 1.f / D[a];
      const float t0 = (0.f - o[a]) * inv[a], t1 = (fd - o[a]) * inv[a];
      tmin = fmaxf(tmin, fminf(t0, t1));
      tmax = fminf(tmax, fmaxf(t0, t1));
    } else {
      inv[a] = 0.f;
      if (o[a] < 0.f || o[a] >= fd) hit = false;
    }
  }
  out[0] = out[1] = out[2] = out[3] = 0.f;
  if (!hit || !(tmin < tmax)) return;
  // entry voxel: a coordinate that rounding put on the wrong side of a plane costs a crossing of rounding length
  int x = min(max((int)floorf(o[0] + tmin * dx), 0), d - 1);
  int y = min(max((int)floorf(o[1] + tmin * dy), 0), d - 1);
  int z = min(max((int)floorf(o[2] + tmin * dz), 0), d - 1);
  const int sx = dx > 0.f ? 1 : (dx < 0.f ? -1 : 0), sy = dy > 0.f ? 1 : (dy < 0.f ? -1 : 0),
            sz = dz > 0.f ? 1 : (dz < 0.f ? -1 : 0);
  float t = tmin, T = 1.f, A = 0.f, C[3] = {0.f, 0.f, 0.f};
  for (int it = 0; it < 3 * d + 3; ++it) {
    const float tx = sx ? ((float)(x + (sx > 0)) - o[0]) * inv[0] : kInf;
    const float ty = sy ? ((float)(y + (sy > 0)) - o[1]) * inv[1] : kInf;
    const float tz = sz ? ((float)(z + (sz > 0)) - o[2]) * inv[2] : kInf;
    const float tn = fminf(tx, fminf(ty, tz));
    const float te = fminf(tn, tmax);
    const float len = te - t;
    if (len > 0.f) {
      float log1m_a, rgb[3];
      if (shade(x, y, z, &log1m_a, rgb)) render_composite(len, log1m_a, rgb, T, C, A);
      t = te;
    }
    if (tn >= tmax || T < kRenderMinT) break;
    if (tx == tn) { x += sx; if (x < 0 || x >= d) break; }
    else if (ty == tn) { y += sy; if (y < 0 || y >= d) break; }
    else { z += sz; if (z < 0 || z >= d) break; }
  }
  out[0] = C[0]; out[1] = C[1]; out[2] = C[2]; out[3] = A;
}

// Density voxel: colour lut[idx] with matplotlib's index rule for floats (idx = int(v 256); v == 1 -> 255; v < 0 -> 0;
// v > 1 -> 255; NaN is empty).  mode 0: opacity alpha where v > floor;  mode 1: opacity alpha clip(v, 0, 1).
__host__ __device__ inline int render_lut_index(float v) {
  return v < 0.f ? 0 : (v >= 1.f ? kRenderLutRows - 1 : (int)(v * (float)kRenderLutRows));
}
struct DensityShade {
  const float* vol;       // sample base + channel
  size_t sx, sy, sz;      // element strides of the three array axes
  const float* lut;       // [256][3]
  int mode;
  float alpha, floor_v, log1m_alpha;
  __host__ __device__ bool operator()(int x, int y, int z, float* log1m_a, float rgb[3]) const {
    const float v = vol[x * sx + y * sy + z * sz];
    if (mode == 0) {
      if (!(v > floor_v)) return false;
      *log1m_a = log1m_alpha;
    } else {
      const float c = fminf(fmaxf(v, 0.f), 1.f);
      if (!(c > 0.f)) return false;
      *log1m_a = log1pf(-(alpha * c));
    }
    const float* q = lut + 3 * render_lut_index(v);
    rgb[0] = q[0]; rgb[1] = q[1]; rgb[2] = q[2];
    return true;
  }
};
// Label voxel: 0 (or below) is empty, label k takes palette[(k - 1) % npal] at opacity alpha.
struct LabelShade {
  const int* lab;
  size_t sx, sy, sz;
  const float* palette;   // [npal][3]
  int npal;
  float log1m_alpha;
  __host__ __device__ bool operator()(int x, int y, int z, float* log1m_a, float rgb[3]) const {
    const int k = lab[x * sx + y * sy + z * sz];
    if (k <= 0) return false;
    const float* q = palette + 3 * ((k - 1) % npal);
    rgb[0] = q[0]; rgb[1] = q[1]; rgb[2] = q[2];
    *log1m_a = log1m_alpha;
    return true;
  }
};

// Atoms of one sample as spheres of `radius` voxels: analytic ray-sphere intersection in fp64, the nearest hit wins (the
// lower atom index on an exact tie), colour palette[species mod npal] times the Lambert term max(0, n . eye), alpha 1; a
// miss is transparent.
__host__ __device__ inline void render_spheres(const RenderView<double>& V, int i, int j, const int* species,
                                               const double* xyz, int n, double radius, const float* palette, int npal,
                                               float out[4]) {
  double o[3];
  render_pixel_origin(V, i, j, o);
  double best_t = __builtin_huge_val(), best_h = 0.0;
  int best = -1;
  for (int k = 0; k < n; ++k) {
    const double qx = o[0] - xyz[3 * k], qy = o[1] - xyz[3 * k + 1], qz = o[2] - xyz[3 * k + 2];
    // ray(t) = o - t eye: the foot of the centre on the ray is at t0 = q . eye, at distance |q - t0 eye| from it
    const double t0 = qx * V.eye[0] + qy * V.eye[1] + qz * V.eye[2];
    const double px = qx - t0 * V.eye[0], py = qy - t0 * V.eye[1], pz = qz - t0 * V.eye[2];
    const double disc = radius * radius - (px * px + py * py + pz * pz);
    if (!(disc > 0.0)) continue;
    const double h = sqrt(disc), t = t0 - h;
    if (t < best_t) { best_t = t; best_h = h; best = k; }
  }
  out[0] = out[1] = out[2] = out[3] = 0.f;
  if (best < 0) return;
  // n = (ray(t) - centre) / radius = (p + h eye) / radius with p perpendicular to eye: n . eye = h / radius
  const double lambert = fmax(0.0, best_h / radius);
  const int s = species[best] % npal, c = s < 0 ? s + npal : s;
  out[0] = (float)(palette[3 * c] * lambert);
  out[1] = (float)(palette[3 * c + 1] * lambert);
  out[2] = (float)(palette[3 * c + 2] * lambert);
  out[3] = 1.f;
}

// camera = (elev, azim) in degrees -> the view of a W x H picture of a d^3 grid, in double; -1 if not finite
int render_view(const double camera[2], int d, int W, int H, RenderView<double>* out);

// Argument rules shared by the four entry points (include/icsg3d.h): 0, or -1 with the error set naming `op`.
int render_check(const char* op, int B, int d, const double* camera, int W, int H, const float* out);
int render_density_check(const char* op, int stride_c, int channel, const float* lut, int mode, float alpha, float floor_v);

// The density picture of DEVICE volumes vol [B][d][d][d][stride_c] and a DEVICE lut into DEVICE out [B][H][W][4]; arguments
// checked by the caller.  Asynchronous on st.  The one launch site of the density kernel: the host-pointer op and
// ics_vae_render_resident both come here, which is why their images are the same bits.
int render_density_device(hipStream_t st, const float* vol, int B, int d, int stride_c, int channel, const float* lut,
                          int mode, float alpha, float floor_v, const RenderView<double>& view, int W, int H, float* out);

}  // namespace ics
