// Declarations for monitor.hip: the pictures the reference's two train loops draw whenever the validation loss improves
// (unet/unet.py:39-157 TrainingPlot: plot_segmentations, plot_binary, plot_losses; vae/lattice_vae.py:327-337, 359-436:
// plot_reconstructions, plot_samples, plot_kde, plot_losses).  Three small operations -- a colour-mapped slice, a
// per-dimension Gaussian KDE, a polyline plot -- whose formulas are written down here once and nowhere else.
// icsg3d_amd/monitor.py and tests/monitor_ref.py restate them and say so.
//
// SLICE  (imshow(V[b, :, :, index, c]) with vmin / vmax the slice's own minimum and maximum).  Source: a volume
// [batch][d][d][d][stride_c] of float32, uint8 or int32, channel `channel`, plane `index` of array axis `axis`.  The
// picture's row and column are the two remaining axes in array order (axis 2: row = axis 0, column = axis 1; axis 1:
// row = axis 0, column = axis 2; axis 0: row = axis 1, column = axis 2), row 0 at the top as imshow draws with origin
// upper; every source pixel becomes zoom x zoom output pixels (nearest neighbour).  Everything below is fp32; an integer
// source is converted to float first.
//     range  given (vmin, vmax), or the minimum and maximum over the FINITE values of the image (one per image)
//     t      = (v - vmin) / (vmax - vmin)                  one IEEE subtraction each, one IEEE division
//     idx    = 0 where !(t >= 0);  255 where t >= 1;  else min(255, (int)(t * 256.0f))
//     vmax == vmin -> idx = 0 for every finite value (matplotlib's Normalize)
//     a non-finite value is left out of the range and drawn transparent (0, 0, 0, 0); an image without a finite value
//     is transparent everywhere
// This is the index rule ics_op_render_density documents, after the normalisation.  Output: float32 premultiplied RGBA
// (lut[idx], 1), [count][d zoom][d zoom][4].
//
// KDE  (scipy.stats.gaussian_kde(z[:, j]) evaluated on a grid, for every latent dimension j at once).  Entirely fp64;
// the float32 codes z [n][dim] are widened exactly.
//     mean_j = sum_i z_ij / n                              first pass
//     var_j  = sum_i (z_ij - mean_j)^2 / (n - 1)           second pass (never E[z^2] - E[z]^2)
//     h2_j   = var_j * f^2,  f = n^(-1/5)                  Scott's rule in one dimension (f^2 = n^(-2/5))
//     density[j][k] = sum_i exp(-(x_k - z_ij)^2 / (2 h2_j)) / (n sqrt(2 pi h2_j))
//     bandwidth[j] = sqrt(h2_j);  status[j] = 1 and a NaN row where h2_j == 0 or is not finite (scipy raises LinAlgError
//     there; a collapsed dimension is what the plot is for), else 0.
//
// LINES  (plt.plot of ncurves curves of npts points, xy [ncurves][npts][2] in data units).  Entirely fp64.
//     a point with a non-finite coordinate breaks the line: the segments on both sides of it are not drawn
//     px = (x - x0) / (x1 - x0) width,   py = (1 - (y - y0) / (y1 - y0)) height        window (x0, x1, y0, y1)
//     dist(pixel, segment p -> q): c = (col + 0.5, row + 0.5), e = q - p, t = clamp(((c - p) . e) / (e . e), 0, 1)
//         (t = 0 where e . e == 0: a zero-length segment is a point), dist = |c - (p + t e)|
//     coverage of a pixel by a curve = max over its segments of clamp(width_px / 2 + 0.5 - dist, 0, 1)
//     curves are composited "over" in index order: a = alpha coverage, rgb = palette[curve % npal],
//         C = a rgb + (1 - a) C,  A = a + (1 - a) A        (C, A start at 0)
//     one rounding to float32 at the end.  Output: premultiplied RGBA [height][width][4].
#pragma once
#include "common.h"

#include <cmath>

struct ics_kde;

namespace ics {

constexpr int kMonitorMaxGrid = 256;
constexpr int kMonitorMaxZoom = 64;
constexpr int kMonitorMaxImage = 4096;
constexpr int kMonitorMaxBatch = 65535;
constexpr int kMonitorLutRows = 256;
constexpr int kKdeMaxDim = 4096, kKdeMaxPoints = 4096, kKdeMaxCodes = 1 << 20;
constexpr int kLinesMaxPoints = 4096, kLinesMaxCurves = 65535;

// the colour index of a finite value v under (vmin, vmax): the SLICE rule above
__host__ __device__ inline int monitor_lut_index(float v, float vmin, float vmax) {
  if (vmax == vmin) return 0;
  const float t = (v - vmin) / (vmax - vmin);
  if (!(t >= 0.f)) return 0;
  if (t >= 1.f) return kMonitorLutRows - 1;
  const int i = (int)(t * 256.0f);
  return i < kMonitorLutRows - 1 ? i : kMonitorLutRows - 1;
}

// coverage of the pixel centre (cx, cy) by the segment (x0, y0) -> (x1, y1), reach = width_px / 2 + 0.5: the LINES rule
__host__ __device__ inline double monitor_segment_coverage(double cx, double cy, double x0, double y0, double x1, double y1,
                                                           double reach) {
  const double ex = x1 - x0, ey = y1 - y0;
  const double ee = ex * ex + ey * ey;
  double t = 0.0;
  if (ee != 0.0) {
    t = ((cx - x0) * ex + (cy - y0) * ey) / ee;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  }
  const double qx = cx - (x0 + t * ex), qy = cy - (y0 + t * ey);
  const double c = reach - sqrt(qx * qx + qy * qy);
  return c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c);
}

// Where a slice's values lie: element (image b, row r, column c) is at base[b img + r row + c col], in elements of the
// source type.  slice_layout fills it for a [batch][d][d][d][stride_c] volume.
struct SliceLayout {
  size_t img, row, col, offset;
};
SliceLayout slice_layout(int d, int stride_c, int channel, int axis, int index);

// Argument rules of the slice entry points (include/icsg3d.h): 0, or -1 with the error set naming `op`.
int slice_check(const char* op, int dtype, int count, int d, int stride_c, int channel, int axis, int index,
                const float* lut, const float* range_or_null, int zoom, const float* out);

// The slice picture of DEVICE values (dtype 0 float32, 1 uint8, 2 int32) under `lay` and a DEVICE lut into DEVICE out
// [count][d zoom][d zoom][4].  d_range: DEVICE [count][2] scratch; with own_range the range kernel fills it, without, the
// caller has uploaded the given (vmin, vmax) to its first row.  Asynchronous on st.  The one launch site of the slice kernels: the
// host-pointer op and the two resident entries all come here, which is why their images are the same bits.
int slice_device(hipStream_t st, const void* src, int dtype, const SliceLayout& lay, int count, int d, const float* d_lut,
                 bool own_range, float* d_range, int zoom, float* d_out);

// ---- the KDE handle (struct ics_kde, defined in monitor.hip): codes resident on the device
// rows of `dim` floats, `stride_floats` apart, already on the handle's device; ordered after the work on src_stream
int kde_append_device(ics_kde* h, const float* src, size_t stride_floats, int rows, hipStream_t src_stream);
int kde_device(const ics_kde* h);
int kde_dim(const ics_kde* h);

}  // namespace ics
