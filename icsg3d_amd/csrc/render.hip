// view_results.py's pictures (reference viz.py:43-66, 184-233; view_results.py:152-183) on the device: ray casts of the
// density, label and atom volumes at full resolution.  The camera and the compositing rule are in render.h.
//
// One thread per pixel, one wave per 8x8 pixel tile: the 64 rays of a wave are parallel and at most 8 pixel sizes apart, so
// at every step they read voxels a few cells from each other -- neighbouring addresses along z, neighbouring lines along y.
// A workgroup is 2x2 tiles (16x16 pixels, 256 threads).  The volume is read straight from global memory: a 32^3 fp32
// volume is 128 KiB, the 32 volumes of a batch 4 MiB, one XCD's L2.  The 3 KiB colour table is copied into LDS once per
// workgroup, since every step indexes it by value.
// Staging the whole volume in LDS instead (128 KiB at d = 32, 32x32 pixels per 1024-thread workgroup) was built and measured:
// 1.4 - 1.6x slower than these global reads, so it is not kept.
#include "render.h"
#include "scratch.h"
#include "../../include/icsg3d.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace ics {
namespace {

constexpr size_t kRenderBudget = (size_t)256 << 20;   // device bytes per chunk (volumes + pictures)


RenderView<float> view_f32(const RenderView<double>& v) {
  RenderView<float> f;
  for (int a = 0; a < 3; ++a) { f.right[a] = (float)v.right[a]; f.up[a] = (float)v.up[a]; f.eye[a] = (float)v.eye[a]; }
  f.pix = (float)v.pix; f.half_w = (float)v.half_w; f.half_h = (float)v.half_h; f.centre = (float)v.centre;
  return f;
}

// pixel of thread tid in a 256-thread workgroup: 2 x 2 wave tiles of 8 x 8 pixels
__device__ __forceinline__ void tile_pixel(int tid, int* i, int* j) {
  const int wave = tid >> 6, lane = tid & 63;
  *i = (blockIdx.x * 2 + (wave & 1)) * 8 + (lane & 7);
  *j = (blockIdx.y * 2 + (wave >> 1)) * 8 + (lane >> 3);
}

__device__ __forceinline__ void store_pixel(float* out, int b, int W, int H, int i, int j, const float px[4]) {
  *reinterpret_cast<float4*>(out + (((size_t)b * H + j) * W + i) * 4) = make_float4(px[0], px[1], px[2], px[3]);
}

__global__ __launch_bounds__(256) void render_density_kernel(const float* __restrict__ vol, int d, int stride_c, int channel,
                                                             const float* __restrict__ lut, int mode, float alpha,
                                                             float floor_v, RenderView<float> V, int W, int H,
                                                             float* __restrict__ out) {
  __shared__ float s_lut[3 * kRenderLutRows];
  const int tid = threadIdx.x, b = blockIdx.z;
  for (int k = tid; k < 3 * kRenderLutRows; k += 256) s_lut[k] = lut[k];
  __syncthreads();
  DensityShade sh;
  sh.vol = vol + (size_t)b * d * d * d * stride_c + channel;
  sh.sz = (size_t)stride_c; sh.sy = sh.sz * d; sh.sx = sh.sy * d;
  sh.lut = s_lut; sh.mode = mode; sh.alpha = alpha; sh.floor_v = floor_v; sh.log1m_alpha = log1pf(-alpha);
  int i, j;
  tile_pixel(tid, &i, &j);
  if (i >= W || j >= H) return;
  float px[4];
  render_walk(V, d, i, j, sh, px);
  store_pixel(out, b, W, H, i, j, px);
}

__global__ __launch_bounds__(256) void render_labels_kernel(const int* __restrict__ labels, int d,
                                                            const float* __restrict__ palette, int npal, float alpha,
                                                            RenderView<float> V, int W, int H, float* __restrict__ out) {
  const int b = blockIdx.z;
  int i, j;
  tile_pixel(threadIdx.x, &i, &j);
  if (i >= W || j >= H) return;
  LabelShade sh;
  sh.lab = labels + (size_t)b * d * d * d;
  sh.sz = 1; sh.sy = (size_t)d; sh.sx = (size_t)d * d;
  sh.palette = palette; sh.npal = npal; sh.log1m_alpha = log1pf(-alpha);
  float px[4];
  render_walk(V, d, i, j, sh, px);
  store_pixel(out, b, W, H, i, j, px);
}

__global__ __launch_bounds__(256) void render_atoms_kernel(const int* __restrict__ off, const int* __restrict__ species,
                                                           const double* __restrict__ xyz, double radius,
                                                           const float* __restrict__ palette, int npal,
                                                           RenderView<double> V, int W, int H, float* __restrict__ out) {
  const int b = blockIdx.z;
  int i, j;
  tile_pixel(threadIdx.x, &i, &j);
  if (i >= W || j >= H) return;
  const int a0 = off[b], n = off[b + 1] - a0;
  float px[4];
  render_spheres(V, i, j, species + a0, xyz + 3 * (size_t)a0, n, radius, palette, npal, px);
  store_pixel(out, b, W, H, i, j, px);
}

dim3 tile_grid(int W, int H, int B) {
  return dim3((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16), (unsigned)B);
}

// exact sine and cosine at the multiples of 90 degrees
void sincos_deg(double deg, double* s, double* c) {
  const double r = std::fmod(deg, 360.0), q = r / 90.0;
  if (q == std::floor(q)) {
    const int k = (((int)q) % 4 + 4) % 4;
    *s = k == 1 ? 1.0 : (k == 3 ? -1.0 : 0.0);
    *c = k == 0 ? 1.0 : (k == 2 ? -1.0 : 0.0);
    return;
  }
  const double rad = r * M_PI / 180.0;
  *s = std::sin(rad); *c = std::cos(rad);
}

// pictures per chunk for `per` device bytes each
int chunk_images(size_t per, int B) {
  const size_t n = std::max<size_t>(1, kRenderBudget / std::max<size_t>(per, 1));
  return (int)std::min<size_t>({n, (size_t)B, (size_t)kRenderMaxBatch});
}

}  // namespace

int render_view(const double camera[2], int d, int W, int H, RenderView<double>* out) {
  if (!std::isfinite(camera[0]) || !std::isfinite(camera[1])) return -1;
  double se, ce, sa, ca;
  sincos_deg(camera[0], &se, &ce);
  sincos_deg(camera[1], &sa, &ca);
  RenderView<double>& v = *out;
  v.eye[0] = ce * ca; v.eye[1] = ce * sa; v.eye[2] = se;
  v.right[0] = -sa; v.right[1] = ca; v.right[2] = 0.0;
  v.up[0] = -se * ca; v.up[1] = -se * sa; v.up[2] = ce;
  v.pix = (double)d * std::sqrt(3.0) / (double)std::min(W, H);
  v.half_w = 0.5 * W; v.half_h = 0.5 * H; v.centre = 0.5 * d;
  return 0;
}

int render_check(const char* who, int B, int d, const double* camera, int W, int H, const float* out) {
  const std::string op = std::string(who) + ": ";
  ICS_CHECK(B >= 1 && B <= kRenderMaxBatch, op + "batch must be in [1, 65535]");
  ICS_CHECK(d >= 1 && d <= kRenderMaxGrid, op + "grid must be in [1, 256]");
  ICS_CHECK(W >= 1 && W <= kRenderMaxImage && H >= 1 && H <= kRenderMaxImage, op + "image sides must be in [1, 4096]");
  ICS_CHECK(camera && out, op + "null argument (camera, out)");
  ICS_CHECK(std::isfinite(camera[0]) && std::isfinite(camera[1]), op + "camera (elev, azim) must be finite");
  return 0;
}

int render_density_check(const char* who, int stride_c, int channel, const float* lut, int mode, float alpha,
                         float floor_v) {
  const std::string op = std::string(who) + ": ";
  ICS_CHECK(lut != nullptr, op + "null lut");
  ICS_CHECK(stride_c >= 1 && channel >= 0 && channel < stride_c, op + "channel must be in [0, stride_c)");
  ICS_CHECK(mode == 0 || mode == 1, op + "mode must be 0 (flat) or 1 (opacity from the value)");
  ICS_CHECK(alpha >= 0.f && alpha <= 1.f, op + "alpha must be in [0, 1]");
  ICS_CHECK(!std::isnan(floor_v), op + "floor must not be NaN");
  return 0;
}

int render_density_device(hipStream_t st, const float* vol, int B, int d, int stride_c, int channel, const float* lut,
                          int mode, float alpha, float floor_v, const RenderView<double>& view, int W, int H, float* out) {
  ICS_LAUNCH(render_density_kernel, tile_grid(W, H, B), dim3(256), 0, st, vol, d, stride_c, channel, lut, mode, alpha,
             floor_v, view_f32(view), W, H, out);
  ICS_HIP(hipGetLastError());
  return 0;
}

}  // namespace ics

using namespace ics;

extern "C" {

// Each of the three is chunked over the batch under a device-memory budget through the calling thread's scratch
// (scratch.h), one upload, one launch and one download per chunk; synchronous on the calling thread's stream.
int ics_op_render_density(const float* vol, int B, int d, int stride_c, int channel, const float* lut, int mode, float alpha,
                          float floor_v, const double* camera, int W, int H, float* out) {
  ICS_TRY(render_check("ics_op_render_density", B, d, camera, W, H, out));
  ICS_TRY(render_density_check("ics_op_render_density", stride_c, channel, lut, mode, alpha, floor_v));
  ICS_CHECK(vol != nullptr, "ics_op_render_density: null vol");
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  RenderView<double> view;
  ICS_CHECK(render_view(camera, d, W, H, &view) == 0, "ics_op_render_density: camera must be finite");
  const size_t vol_b = (size_t)d * d * d * stride_c * sizeof(float), img_b = (size_t)W * H * 16;
  const int nb = chunk_images(vol_b + img_b, B);
  Layout L;
  const auto s_lut = L.add<float>(3 * kRenderLutRows);
  const auto s_vol = L.add<float>(vol_b / 4 * nb);
  const auto s_out = L.add<float>(img_b / 4 * nb);
  float *d_lut, *d_vol, *d_out;
  ICS_TRY(L.reserve(s_lut, &d_lut, s_vol, &d_vol, s_out, &d_out));
  ICS_TRY(L.upload(s_lut, lut, s_lut.count, st));
  for (int b0 = 0; b0 < B; b0 += nb) {
    const int n = std::min(nb, B - b0);
    ICS_TRY(L.upload(s_vol, reinterpret_cast<const unsigned char*>(vol) + vol_b * b0, vol_b / 4 * n, st));
    ICS_TRY(render_density_device(st, d_vol, n, d, stride_c, channel, d_lut, mode, alpha, floor_v, view, W, H, d_out));
    ICS_TRY(L.download(reinterpret_cast<unsigned char*>(out) + img_b * b0, s_out, img_b / 4 * n, st));
    ICS_HIP(hipStreamSynchronize(st));
  }
  return 0;
}

int ics_op_render_labels(const int32_t* labels, int B, int d, const float* palette, int npal, float alpha,
                         const double* camera, int W, int H, float* out) {
  ICS_TRY(render_check("ics_op_render_labels", B, d, camera, W, H, out));
  ICS_CHECK(labels && palette, "ics_op_render_labels: null argument (labels, palette)");
  ICS_CHECK(npal >= 1, "ics_op_render_labels: npal must be >= 1");
  ICS_CHECK(alpha >= 0.f && alpha <= 1.f, "ics_op_render_labels: alpha must be in [0, 1]");
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  RenderView<double> view;
  ICS_CHECK(render_view(camera, d, W, H, &view) == 0, "ics_op_render_labels: camera must be finite");
  const RenderView<float> V = view_f32(view);
  const size_t vol_b = (size_t)d * d * d * sizeof(int32_t), img_b = (size_t)W * H * 16;
  const int nb = chunk_images(vol_b + img_b, B);
  Layout L;
  const auto s_pal = L.add<float>((size_t)npal * 3);
  const auto s_lab = L.add<int>(vol_b / 4 * nb);
  const auto s_out = L.add<float>(img_b / 4 * nb);
  float *d_pal, *d_out;
  int* d_lab;
  ICS_TRY(L.reserve(s_pal, &d_pal, s_lab, &d_lab, s_out, &d_out));
  ICS_TRY(L.upload(s_pal, palette, s_pal.count, st));
  for (int b0 = 0; b0 < B; b0 += nb) {
    const int n = std::min(nb, B - b0);
    ICS_TRY(L.upload(s_lab, reinterpret_cast<const unsigned char*>(labels) + vol_b * b0, vol_b / 4 * n, st));
    ICS_LAUNCH(render_labels_kernel, tile_grid(W, H, n), dim3(256), 0, st, d_lab, d, d_pal, npal, alpha, V, W, H, d_out);
    ICS_HIP(hipGetLastError());
    ICS_TRY(L.download(reinterpret_cast<unsigned char*>(out) + img_b * b0, s_out, img_b / 4 * n, st));
    ICS_HIP(hipStreamSynchronize(st));
  }
  return 0;
}

int ics_op_render_atoms(const int32_t* offsets, const int32_t* species, const double* xyz, int B, int d, double radius,
                        const float* palette, int npal, const double* camera, int W, int H, float* out) {
  const std::string op = "ics_op_render_atoms: ";
  ICS_TRY(render_check("ics_op_render_atoms", B, d, camera, W, H, out));
  ICS_CHECK(offsets && palette, op + "null argument (offsets, palette)");
  ICS_CHECK(npal >= 1, op + "npal must be >= 1");
  ICS_CHECK(std::isfinite(radius) && radius > 0.0, op + "radius must be finite and > 0");
  ICS_CHECK(offsets[0] == 0, op + "offsets[0] must be 0");
  for (int b = 0; b < B; ++b)
    ICS_CHECK(offsets[b + 1] >= offsets[b], op + "offsets decrease at sample " + std::to_string(b));
  ICS_CHECK((species && xyz) || offsets[B] == 0, op + "null species or xyz");
  for (long long k = 0; k < 3LL * offsets[B]; ++k)
    ICS_CHECK(std::isfinite(xyz[k]), op + "non-finite coordinate");
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  RenderView<double> view;
  ICS_CHECK(render_view(camera, d, W, H, &view) == 0, "ics_op_render_atoms: camera must be finite");
  const size_t img_b = (size_t)W * H * 16;
  const int nb = chunk_images(img_b, B);
  std::vector<int32_t> off(nb + 1);
  for (int b0 = 0; b0 < B; b0 += nb) {
    const int n = std::min(nb, B - b0);
    const int A0 = offsets[b0];
    const size_t N = (size_t)(offsets[b0 + n] - A0);
    for (int k = 0; k <= n; ++k) off[k] = offsets[b0 + k] - A0;
    Layout L;
    const auto s_pal = L.add<float>((size_t)npal * 3);
    const auto s_off = L.add<int>(n + 1);
    const auto s_sp = L.add<int>(N + 1);          // one spare element each: never empty
    const auto s_xyz = L.add<double>(3 * N + 1);
    const auto s_out = L.add<float>(img_b / 4 * n);
    float *d_pal, *d_out;
    int *d_off, *d_sp;
    double* d_xyz;
    ICS_TRY(L.reserve(s_pal, &d_pal, s_off, &d_off, s_sp, &d_sp, s_xyz, &d_xyz, s_out, &d_out));
    ICS_TRY(L.upload(s_pal, palette, s_pal.count, st));
    ICS_TRY(L.upload(s_off, off.data(), n + 1, st));
    if (N) {
      ICS_TRY(L.upload(s_sp, species + A0, N, st));
      ICS_TRY(L.upload(s_xyz, xyz + 3 * (size_t)A0, 3 * N, st));
    }
    ICS_LAUNCH(render_atoms_kernel, tile_grid(W, H, n), dim3(256), 0, st, d_off, d_sp, d_xyz, radius, d_pal, npal, view, W,
               H, d_out);
    ICS_HIP(hipGetLastError());
    ICS_TRY(L.download(reinterpret_cast<unsigned char*>(out) + img_b * b0, s_out, img_b / 4 * n, st));
    ICS_HIP(hipStreamSynchronize(st));   // off is reused by the next chunk
  }
  return 0;
}

}  // extern "C"
