// The training monitors' pictures (reference unet/unet.py:39-157, vae/lattice_vae.py:327-337, 359-436) on the device: a
// colour-mapped slice of a resident volume, the Gaussian KDE of every latent dimension, and a polyline plot.  The formulas
// are in monitor.h.
//
// All three are small.  Slice: one workgroup per image reduces the plane's range (wave-64 shuffles, four partials through
// LDS), then one thread per output pixel maps it.  KDE: one workgroup per latent dimension; the column of z, strided by dim
// in memory, is staged through LDS in chunks of 2048 codes and every pass (mean, squared deviations, densities) reads the
// staged copy; a wave owns a grid point, its lanes stride over the staged codes and a shuffle tree folds them.  Lines: one
// workgroup per 16 x 16 pixel tile, one thread per pixel; the segments stream through LDS 256 at a time, each wave loads 64
// of them and leaves their bounding box, and a tile skips a group of 64 whose box, grown by the line's reach, misses it.
//
// No contraction anywhere in this file, monitor.h's inline colour and coverage rules included: the pragma comes first.
#pragma clang fp contract(off)

#include "monitor.h"
#include "scratch.h"
#include "../../include/icsg3d.h"

#include <algorithm>
#include <cmath>
#include <cstring>

struct ics_kde {
  int dim = 0, capacity = 0, device = 0;
  hipStream_t st = nullptr;
  float* codes = nullptr;   // [capacity][dim]
  int count = 0;
};

namespace ics {
namespace {

constexpr size_t kMonitorBudget = (size_t)256 << 20;   // device bytes per chunk of slice pictures
constexpr int kKdeThreads = 256, kKdeChunk = 2048;
constexpr int kLineThreads = 256, kLineTile = 16;


template <typename V>
__device__ __forceinline__ V wave_min(V v) {
  for (int o = 32; o > 0; o >>= 1) { const V w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
  return v;
}
template <typename V>
__device__ __forceinline__ V wave_max(V v) {
  for (int o = 32; o > 0; o >>= 1) { const V w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------- slice
template <typename T>
__global__ __launch_bounds__(256) void slice_range_kernel(const T* __restrict__ src, SliceLayout lay, int d,
                                                          float* __restrict__ range) {
  __shared__ float s_lo[4], s_hi[4];
  const int tid = threadIdx.x, b = blockIdx.x;
  const T* img = src + lay.offset + (size_t)b * lay.img;
  float lo = __builtin_huge_valf(), hi = -__builtin_huge_valf();
  for (int p = tid; p < d * d; p += 256) {
    const float v = (float)img[(size_t)(p / d) * lay.row + (size_t)(p % d) * lay.col];
    if (isfinite(v)) { lo = fminf(lo, v); hi = fmaxf(hi, v); }
  }
  lo = wave_min(lo); hi = wave_max(hi);
  if ((tid & 63) == 0) { s_lo[tid >> 6] = lo; s_hi[tid >> 6] = hi; }
  __syncthreads();
  if (tid == 0) {
    range[2 * b] = fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3]));
    range[2 * b + 1] = fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3]));
  }
}

template <typename T>
__global__ __launch_bounds__(256) void slice_map_kernel(const T* __restrict__ src, SliceLayout lay, int d, int zoom,
                                                        const float* __restrict__ lut, const float* __restrict__ range,
                                                        int range_stride, float* __restrict__ out) {
  const int side = d * zoom, b = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= side * side) return;
  const int r = (p / side) / zoom, c = (p % side) / zoom;
  const float v = (float)src[lay.offset + (size_t)b * lay.img + (size_t)r * lay.row + (size_t)c * lay.col];
  float4 px = make_float4(0.f, 0.f, 0.f, 0.f);
  if (isfinite(v)) {
    const float* q = lut + 3 * monitor_lut_index(v, range[(size_t)b * range_stride], range[(size_t)b * range_stride + 1]);
    px = make_float4(q[0], q[1], q[2], 1.f);
  }
  reinterpret_cast<float4*>(out)[(size_t)b * side * side + p] = px;
}

template <typename T>
int slice_launch(hipStream_t st, const void* src, const SliceLayout& lay, int count, int d, const float* d_lut,
                 bool own_range, float* d_range, int zoom, float* d_out) {
  const T* s = static_cast<const T*>(src);
  if (own_range) ICS_LAUNCH(slice_range_kernel<T>, dim3((unsigned)count), dim3(256), 0, st, s, lay, d, d_range);
  const int side = d * zoom;
  ICS_LAUNCH(slice_map_kernel<T>, dim3((unsigned)((side * side + 255) / 256), (unsigned)count), dim3(256), 0, st, s, lay, d,
             zoom, d_lut, (const float*)d_range, own_range ? 2 : 0, d_out);
  ICS_HIP(hipGetLastError());
  return 0;
}

size_t slice_elem_bytes(int dtype) { return dtype == 1 ? 1 : 4; }

// ---------------------------------------------------------------- KDE
// sum over the workgroup in a fixed order; every thread gets the result
__device__ __forceinline__ double kde_block_sum(double v, double* s_red) {
  v = wave_sum(v);
  __syncthreads();                       // the previous result has been read
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__global__ __launch_bounds__(kKdeThreads) void kde_kernel(const float* __restrict__ z, int n, int dim,
                                                          const double* __restrict__ x, int npts, double fac2,
                                                          double* __restrict__ density, double* __restrict__ bandwidth,
                                                          int* __restrict__ status) {
  __shared__ double s_z[kKdeChunk];
  __shared__ double s_acc[kKdeMaxPoints];
  __shared__ double s_red[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = blockIdx.x;
  const bool one_chunk = n <= kKdeChunk;       // the usual case: the column is read from memory once
  auto stage = [&](int i0, int cnt) {
    __syncthreads();                           // the previous chunk has been consumed
    for (int i = tid; i < cnt; i += kKdeThreads) s_z[i] = (double)z[(size_t)(i0 + i) * dim + j];
    __syncthreads();
  };
  if (one_chunk) stage(0, n);
  double part = 0.0;
  for (int i0 = 0; i0 < n; i0 += kKdeChunk) {
    const int cnt = min(kKdeChunk, n - i0);
    if (!one_chunk) stage(i0, cnt);
    for (int i = tid; i < cnt; i += kKdeThreads) part += s_z[i];
  }
  const double mean = kde_block_sum(part, s_red) / (double)n;
  part = 0.0;
  for (int i0 = 0; i0 < n; i0 += kKdeChunk) {
    const int cnt = min(kKdeChunk, n - i0);
    if (!one_chunk) stage(i0, cnt);
    for (int i = tid; i < cnt; i += kKdeThreads) { const double dv = s_z[i] - mean; part += dv * dv; }
  }
  const double var = kde_block_sum(part, s_red) / (double)(n - 1);
  const double h2 = var * fac2;
  const bool bad = h2 == 0.0 || !isfinite(h2);
  if (tid == 0) { bandwidth[j] = sqrt(h2); status[j] = bad ? 1 : 0; }
  double* row = density + (size_t)j * npts;
  if (bad) {
    for (int k = tid; k < npts; k += kKdeThreads) row[k] = __builtin_nan("");
    return;
  }
  for (int k = tid; k < npts; k += kKdeThreads) s_acc[k] = 0.0;
  const double two_h2 = 2.0 * h2;
  for (int i0 = 0; i0 < n; i0 += kKdeChunk) {
    const int cnt = min(kKdeChunk, n - i0);
    if (!one_chunk) stage(i0, cnt); else __syncthreads();
    for (int k = wave; k < npts; k += kKdeThreads / 64) {     // only this wave touches s_acc[k]
      const double xk = x[k];
      double p = 0.0;
      for (int i = lane; i < cnt; i += 64) { const double dv = xk - s_z[i]; p += exp(-(dv * dv) / two_h2); }
      p = wave_sum(p);
      if (lane == 0) s_acc[k] += p;
    }
  }
  __syncthreads();
  const double norm = (double)n * sqrt(2.0 * M_PI * h2);
  for (int k = tid; k < npts; k += kKdeThreads) row[k] = s_acc[k] / norm;
}

int kde_enter(ics_kde* h, const char* who) {
  ICS_CHECK(h != nullptr, std::string(who) + ": null KDE handle");
  ICS_HIP(hipSetDevice(h->device));
  return 0;
}

// ---------------------------------------------------------------- lines
struct LineArgs {
  double x0, x1, y0, y1;     // window
  double reach, alpha;       // width_px / 2 + 0.5; opacity
  int ncurves, npts, width, height, npal;
};

__global__ __launch_bounds__(kLineThreads) void lines_kernel(const double* __restrict__ xy, LineArgs a,
                                                             const float* __restrict__ palette, float* __restrict__ out) {
  __shared__ double s_seg[kLineThreads][4];     // pixel coordinates of a segment's ends; [0] NaN: not drawn
  __shared__ double s_box[kLineThreads / 64][4];   // xmin, xmax, ymin, ymax of each wave's 64 segments
  const int tid = threadIdx.x, wave = tid >> 6;
  const int col = blockIdx.x * kLineTile + (tid & (kLineTile - 1)), row = blockIdx.y * kLineTile + tid / kLineTile;
  const double cx = (double)col + 0.5, cy = (double)row + 0.5;
  // the tile's pixel centres
  const double tx0 = (double)(blockIdx.x * kLineTile) + 0.5, tx1 = tx0 + (double)(kLineTile - 1);
  const double ty0 = (double)(blockIdx.y * kLineTile) + 0.5, ty1 = ty0 + (double)(kLineTile - 1);
  const int nseg = a.npts - 1;
  const long long total = (long long)a.ncurves * nseg;
  const double kInf = __builtin_huge_val();
  double C[3] = {0.0, 0.0, 0.0}, A = 0.0, cov = 0.0;
  int cur = 0;
  auto flush = [&]() {
    if (cov > 0.0) {
      const double w = a.alpha * cov;
      const float* q = palette + 3 * (cur % a.npal);
      for (int k = 0; k < 3; ++k) C[k] = w * (double)q[k] + (1.0 - w) * C[k];
      A = w + (1.0 - w) * A;
    }
    cov = 0.0;
  };
  for (long long s0 = 0; s0 < total; s0 += kLineThreads) {
    __syncthreads();                          // the previous chunk has been consumed
    {
      const long long s = s0 + tid;
      double p[4] = {__builtin_nan(""), 0.0, 0.0, 0.0};
      double bx0 = kInf, bx1 = -kInf, by0 = kInf, by1 = -kInf;
      if (s < total) {
        const long long c = s / nseg;
        const double* q = xy + 2 * (c * a.npts + (s - c * nseg));
        const double ax = (q[0] - a.x0) / (a.x1 - a.x0) * (double)a.width;
        const double ay = (1.0 - (q[1] - a.y0) / (a.y1 - a.y0)) * (double)a.height;
        const double bx = (q[2] - a.x0) / (a.x1 - a.x0) * (double)a.width;
        const double by = (1.0 - (q[3] - a.y0) / (a.y1 - a.y0)) * (double)a.height;
        if (isfinite(ax) && isfinite(ay) && isfinite(bx) && isfinite(by)) {
          p[0] = ax; p[1] = ay; p[2] = bx; p[3] = by;
          bx0 = fmin(ax, bx); bx1 = fmax(ax, bx); by0 = fmin(ay, by); by1 = fmax(ay, by);
        }
      }
      for (int k = 0; k < 4; ++k) s_seg[tid][k] = p[k];
      bx0 = wave_min(bx0); bx1 = wave_max(bx1); by0 = wave_min(by0); by1 = wave_max(by1);
      if ((tid & 63) == 0) { s_box[wave][0] = bx0; s_box[wave][1] = bx1; s_box[wave][2] = by0; s_box[wave][3] = by1; }
    }
    __syncthreads();
    const int cnt = (int)(total - s0 < kLineThreads ? total - s0 : kLineThreads);
    for (int g = 0; g * 64 < cnt; ++g) {
      // a group none of whose segments can reach a pixel centre of this tile adds coverage 0: skipped, same result
      if (s_box[g][0] - a.reach > tx1 || s_box[g][1] + a.reach < tx0 || s_box[g][2] - a.reach > ty1 ||
          s_box[g][3] + a.reach < ty0)
        continue;
      const int i1 = min(cnt, g * 64 + 64);
      long long s = s0 + g * 64;
      int c = (int)(s / nseg), k = (int)(s - (long long)c * nseg);
      for (int i = g * 64; i < i1; ++i) {
        if (c != cur) { flush(); cur = c; }
        const double ax = s_seg[i][0];
        if (ax == ax) cov = fmax(cov, monitor_segment_coverage(cx, cy, ax, s_seg[i][1], s_seg[i][2], s_seg[i][3], a.reach));
        if (++k == nseg) { k = 0; ++c; }
      }
    }
  }
  flush();
  if (col < a.width && row < a.height)
    reinterpret_cast<float4*>(out)[(size_t)row * a.width + col] = make_float4((float)C[0], (float)C[1], (float)C[2], (float)A);
}

}  // namespace

// ---------------------------------------------------------------- slice: host side
SliceLayout slice_layout(int d, int stride_c, int channel, int axis, int index) {
  const size_t s2 = (size_t)stride_c, s1 = s2 * d, s0 = s1 * d;
  const size_t st[3] = {s0, s1, s2};
  SliceLayout l;
  l.img = s0 * d;
  l.row = st[axis == 0 ? 1 : 0];
  l.col = st[axis == 2 ? 1 : 2];
  l.offset = (size_t)index * st[axis] + (size_t)channel;
  return l;
}

int slice_check(const char* who, int dtype, int count, int d, int stride_c, int channel, int axis, int index,
                const float* lut, const float* range, int zoom, const float* out) {
  const std::string op = std::string(who) + ": ";
  ICS_CHECK(lut && out, op + "null argument (lut, out)");
  ICS_CHECK(dtype >= 0 && dtype <= 2, op + "dtype must be 0 (float32), 1 (uint8) or 2 (int32)");
  ICS_CHECK(count >= 1 && count <= kMonitorMaxBatch, op + "batch must be in [1, 65535]");
  ICS_CHECK(d >= 1 && d <= kMonitorMaxGrid, op + "grid must be in [1, 256]");
  ICS_CHECK(stride_c >= 1 && channel >= 0 && channel < stride_c, op + "channel must be in [0, stride_c)");
  ICS_CHECK(axis >= 0 && axis <= 2, op + "axis must be 0, 1 or 2");
  ICS_CHECK(index >= 0 && index < d, op + "index must be in [0, d)");
  ICS_CHECK(zoom >= 1 && zoom <= kMonitorMaxZoom, op + "zoom must be in [1, 64]");
  ICS_CHECK(d * zoom <= kMonitorMaxImage, op + "image side d * zoom must not exceed 4096");
  if (range)
    ICS_CHECK(std::isfinite(range[0]) && std::isfinite(range[1]) && range[1] >= range[0],
              op + "range must be finite with vmax >= vmin");
  return 0;
}

int slice_device(hipStream_t st, const void* src, int dtype, const SliceLayout& lay, int count, int d, const float* d_lut,
                 bool own_range, float* d_range, int zoom, float* d_out) {
  if (dtype == 0) return slice_launch<float>(st, src, lay, count, d, d_lut, own_range, d_range, zoom, d_out);
  if (dtype == 1) return slice_launch<unsigned char>(st, src, lay, count, d, d_lut, own_range, d_range, zoom, d_out);
  return slice_launch<int32_t>(st, src, lay, count, d, d_lut, own_range, d_range, zoom, d_out);
}

// ---------------------------------------------------------------- KDE: the handle
int kde_device(const ics_kde* h) { return h->device; }
int kde_dim(const ics_kde* h) { return h->dim; }

int kde_append_device(ics_kde* h, const float* src, size_t stride_floats, int rows, hipStream_t src_stream) {
  ICS_TRY(kde_enter(h, "ics_op_kde_append_vae"));
  ICS_CHECK(src != nullptr, "ics_op_kde_append_vae: null source");
  ICS_CHECK(rows >= 1 && rows <= h->capacity - h->count, "ics_op_kde_append_vae: rows exceed the handle's capacity");
  const size_t w = (size_t)h->dim * 4;
  ICS_HIP(hipMemcpy2DAsync(h->codes + (size_t)h->count * h->dim, w, src, stride_floats * 4, w, (size_t)rows,
                           hipMemcpyDeviceToDevice, src_stream));
  ICS_HIP(hipStreamSynchronize(src_stream));
  h->count += rows;
  return 0;
}

}  // namespace ics

using namespace ics;

extern "C" {

// The planes are gathered on the host, uploaded, drawn and downloaded in chunks under a device-memory budget through the
// calling thread's scratch (scratch.h); synchronous on the calling thread's stream.
int ics_op_render_slice(const void* vol, int dtype, int batch, int d, int stride_c, int channel, int axis, int index,
                        const float* lut, const float* range, int zoom, float* out) {
  ICS_TRY(slice_check("ics_op_render_slice", dtype, batch, d, stride_c, channel, axis, index, lut, range, zoom, out));
  ICS_CHECK(vol != nullptr, "ics_op_render_slice: null vol");
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  const size_t es = slice_elem_bytes(dtype), side = (size_t)d * zoom;
  const size_t plane_b = (size_t)d * d * es, img_b = side * side * 16;
  const int nb = (int)std::min<size_t>((size_t)batch, std::max<size_t>(1, kMonitorBudget / (plane_b + img_b)));
  Layout L;
  const auto s_lut = L.add<float>(3 * kMonitorLutRows);
  const auto s_rng = L.add<float>(2 * (size_t)nb);
  const auto s_src = L.add<unsigned char>(plane_b * nb);
  const auto s_out = L.add<float>(img_b / 4 * nb);
  float *d_lut, *d_rng, *d_out;
  unsigned char* d_src;
  ICS_TRY(L.reserve(s_lut, &d_lut, s_rng, &d_rng, s_src, &d_src, s_out, &d_out));
  ICS_TRY(L.upload(s_lut, lut, s_lut.count, st));
  const SliceLayout src_l = slice_layout(d, stride_c, channel, axis, index);
  const SliceLayout dev_l = {(size_t)d * d, (size_t)d, 1, 0};
  std::vector<unsigned char> planes(plane_b * nb);
  const unsigned char* v = static_cast<const unsigned char*>(vol);
  for (int b0 = 0; b0 < batch; b0 += nb) {
    const int n = std::min(nb, batch - b0);
    for (int b = 0; b < n; ++b)
      for (int r = 0; r < d; ++r)
        for (int c = 0; c < d; ++c)
          std::memcpy(&planes[(((size_t)b * d + r) * d + c) * es],
                      v + (src_l.offset + (size_t)(b0 + b) * src_l.img + (size_t)r * src_l.row + (size_t)c * src_l.col) * es, es);
    ICS_TRY(L.upload(s_src, planes.data(), plane_b * n, st));
    if (range) ICS_TRY(L.upload(s_rng, range, 2, st));
    ICS_TRY(slice_device(st, d_src, dtype, dev_l, n, d, d_lut, range == nullptr, d_rng, zoom, d_out));
    ICS_TRY(L.download(reinterpret_cast<unsigned char*>(out) + img_b * b0, s_out, img_b / 4 * n, st));
    ICS_HIP(hipStreamSynchronize(st));   // planes is refilled by the next chunk
  }
  return 0;
}

// ---------------------------------------------------------------- KDE: the handle
int ics_op_kde_create(int dim, int capacity, ics_kde** out) {
  ICS_CHECK(out != nullptr, "ics_op_kde_create: null argument");
  ICS_CHECK(dim >= 1 && dim <= kKdeMaxDim, "ics_op_kde_create: dim must be in [1, 4096]");
  ICS_CHECK(capacity >= 2 && capacity <= kKdeMaxCodes, "ics_op_kde_create: capacity must be in [2, 2^20]");
  ics_kde* h = new ics_kde();
  h->dim = dim; h->capacity = capacity;
  auto fail = [&]() { (void)ics_op_kde_destroy(h); return -1; };
  if (hipGetDevice(&h->device) != hipSuccess) { set_error("ics_op_kde_create: hipGetDevice failed"); return fail(); }
  if (hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) != hipSuccess) {
    h->st = nullptr;
    set_error("ics_op_kde_create: hipStreamCreateWithFlags failed");
    return fail();
  }
  void* p = nullptr;
  if (hipMalloc(&p, (size_t)capacity * dim * 4) != hipSuccess) {
    set_error("ics_op_kde_create: out of device memory for " + std::to_string(capacity) + " codes");
    return fail();
  }
  h->codes = static_cast<float*>(p);
  *out = h;
  return 0;
}

int ics_op_kde_destroy(ics_kde* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  if (h->st) (void)hipStreamSynchronize(h->st);
  if (h->codes) (void)hipFree(h->codes);
  if (h->st) (void)hipStreamDestroy(h->st);
  delete h;
  return 0;
}

int ics_op_kde_append(ics_kde* h, const float* codes, int rows) {
  ICS_TRY(kde_enter(h, "ics_op_kde_append"));
  ICS_CHECK(codes != nullptr, "ics_op_kde_append: null codes");
  ICS_CHECK(rows >= 1 && rows <= h->capacity - h->count, "ics_op_kde_append: rows exceed the handle's capacity");
  const size_t cnt = (size_t)rows * h->dim;
  for (size_t i = 0; i < cnt; ++i) ICS_CHECK(std::isfinite(codes[i]), "ics_op_kde_append: codes are not finite");
  ICS_HIP(hipMemcpyAsync(h->codes + (size_t)h->count * h->dim, codes, cnt * 4, hipMemcpyHostToDevice, h->st));
  ICS_HIP(hipStreamSynchronize(h->st));
  h->count += rows;
  return 0;
}

int ics_op_kde_evaluate(ics_kde* h, const double* x, int npts, double* density, double* bandwidth, int32_t* status,
                        int* count) {
  ICS_TRY(kde_enter(h, "ics_op_kde_evaluate"));
  ICS_CHECK(x && density, "ics_op_kde_evaluate: null argument (x, density)");
  ICS_CHECK(npts >= 1 && npts <= kKdeMaxPoints, "ics_op_kde_evaluate: npts must be in [1, 4096]");
  ICS_CHECK(h->count >= 2, "ics_op_kde_evaluate: at least 2 codes are needed, the handle has " + std::to_string(h->count));
  for (int k = 0; k < npts; ++k) ICS_CHECK(!std::isnan(x[k]), "ics_op_kde_evaluate: x must not be NaN");
  const int n = h->count, dim = h->dim;
  Layout L;
  const auto s_x = L.add<double>(npts);
  const auto s_dens = L.add<double>((size_t)dim * npts);
  const auto s_bw = L.add<double>(dim);
  const auto s_st = L.add<int>(dim);
  double *d_x, *d_dens, *d_bw;
  int* d_st;
  ICS_TRY(L.reserve(s_x, &d_x, s_dens, &d_dens, s_bw, &d_bw, s_st, &d_st));
  ICS_TRY(L.upload(s_x, x, npts, h->st));
  const double fac = std::pow((double)n, -1.0 / 5.0);
  ICS_LAUNCH(kde_kernel, dim3((unsigned)dim), dim3(kKdeThreads), 0, h->st, (const float*)h->codes, n, dim,
             (const double*)d_x, npts, fac * fac, d_dens, d_bw, d_st);
  ICS_HIP(hipGetLastError());
  ICS_TRY(L.download(density, s_dens, s_dens.count, h->st));
  if (bandwidth) ICS_TRY(L.download(bandwidth, s_bw, dim, h->st));
  if (status) ICS_TRY(L.download(status, s_st, dim, h->st));
  ICS_HIP(hipStreamSynchronize(h->st));
  if (count) *count = n;
  return 0;
}

// ---------------------------------------------------------------- lines
int ics_op_render_lines(const double* xy, int ncurves, int npts, const double window[4], const float* palette, int npal,
                        double width_px, float alpha, int width, int height, float* out) {
  const std::string op = "ics_op_render_lines: ";
  ICS_CHECK(xy && window && palette && out, op + "null argument (xy, window, palette, out)");
  ICS_CHECK(npts >= 2 && npts <= kLinesMaxPoints, op + "npts must be in [2, 4096]");
  ICS_CHECK(ncurves >= 1 && ncurves <= kLinesMaxCurves, op + "ncurves must be in [1, 65535]");
  ICS_CHECK(width >= 1 && width <= kMonitorMaxImage && height >= 1 && height <= kMonitorMaxImage,
            op + "image sides must be in [1, 4096]");
  ICS_CHECK(std::isfinite(window[0]) && std::isfinite(window[1]) && std::isfinite(window[2]) && std::isfinite(window[3]) &&
                window[0] != window[1] && window[2] != window[3] && std::isfinite(window[1] - window[0]) &&
                std::isfinite(window[3] - window[2]),
            op + "window (x0, x1, y0, y1) must be finite with x0 != x1 and y0 != y1");
  ICS_CHECK(std::isfinite(width_px) && width_px > 0.0, op + "width_px must be finite and > 0");
  ICS_CHECK(alpha >= 0.f && alpha <= 1.f, op + "alpha must be in [0, 1]");
  ICS_CHECK(npal >= 1, op + "npal must be >= 1");
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  Layout L;
  const auto s_xy = L.add<double>((size_t)ncurves * npts * 2);
  const auto s_pal = L.add<float>((size_t)npal * 3);
  const auto s_out = L.add<float>((size_t)width * height * 4);
  double* d_xy;
  float *d_pal, *d_out;
  ICS_TRY(L.reserve(s_xy, &d_xy, s_pal, &d_pal, s_out, &d_out));
  ICS_TRY(L.upload(s_xy, xy, s_xy.count, st));
  ICS_TRY(L.upload(s_pal, palette, s_pal.count, st));
  LineArgs a;
  a.x0 = window[0]; a.x1 = window[1]; a.y0 = window[2]; a.y1 = window[3];
  a.reach = width_px / 2.0 + 0.5; a.alpha = (double)alpha;
  a.ncurves = ncurves; a.npts = npts; a.width = width; a.height = height; a.npal = npal;
  ICS_LAUNCH(lines_kernel, dim3((unsigned)((width + kLineTile - 1) / kLineTile), (unsigned)((height + kLineTile - 1) / kLineTile)),
             dim3(kLineThreads), 0, st, (const double*)d_xy, a, (const float*)d_pal, d_out);
  ICS_HIP(hipGetLastError());
  ICS_TRY(L.download(out, s_out, s_out.count, st));
  ICS_HIP(hipStreamSynchronize(st));
  return 0;
}

}  // extern "C"
