// interpolate.py's walk between two latent codes (reference interpolate.py:54-59) on the device, written straight into
// the decoder's dense input zc = [z | cond] (the tiled condition of interpolate.py:58 in the same pass).
//
// lerp, element j of step k:  fl32( fl64(a_j) + alpha_k * fl64( fl32(b_j - a_j) ) ) -- the reference subtracts two
// float32 arrays, multiplies by a float64 linspace (so product and sum are float64, rounded separately) and Keras rounds
// to float32 once when it feeds the decoder.  Bit for bit: contraction is off for this file.
// slerp (opt-in), in float64 from the float32 codes: c = a.b / (|a||b|), w = acos(clamp(c)), s = sqrt(1 - c c),
// out = fl32( sin((1-t) w)/s a_j + sin(t w)/s b_j ); pairs with a zero code or s < 1e-3 take the lerp, every step.
//
// One workgroup per pair.  The three dot products are summed in a fixed order -- per-thread strided partial sums, a
// wave64 butterfly, then the wave sums from LDS in wave order -- so results are the same run to run.  Latency-sized
// (256 x 8 values per pair at the defaults): the only care taken is that a row is written by consecutive threads.
#include "latent.h"
#include "scratch.h"
#include "../../include/icsg3d.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace ics {
namespace {

constexpr int kLatentThreads = 256;
constexpr size_t kLatentChunkFloats = (size_t)16 << 20;   // path floats per chunk of the host-pointer op (64 MB)

__global__ __launch_bounds__(kLatentThreads) void latent_path_kernel(
    const float* __restrict__ za, const float* __restrict__ zb, size_t z_stride, const float* __restrict__ cond,
    size_t cond_stride, int ncond, int latent, const double* __restrict__ alpha, int steps, int mode,
    float* __restrict__ zc, float* __restrict__ path) {
  constexpr int NW = kLatentThreads / 64;
  __shared__ double red[3][NW];
  __shared__ double bc[2];      // w, s
  __shared__ int use_slerp;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* a = za + (size_t)p * z_stride;
  const float* b = zb + (size_t)p * z_stride;
  const float* cp = ncond > 0 ? cond + (size_t)p * cond_stride : nullptr;
  const int W = latent + ncond;

  bool slerp = false;
  double w = 0.0, s = 1.0;
  if (mode == LATENT_SLERP) {                   // uniform over the workgroup
    double aa = 0.0, bb = 0.0, ab = 0.0;
    for (int j = tid; j < latent; j += kLatentThreads) {
      const double x = (double)a[j], y = (double)b[j];
      aa += x * x; bb += y * y; ab += x * y;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      aa += __shfl_xor(aa, o, 64); bb += __shfl_xor(bb, o, 64); ab += __shfl_xor(ab, o, 64);
    }
    if (lane == 0) { red[0][wave] = aa; red[1][wave] = bb; red[2][wave] = ab; }
    __syncthreads();
    if (tid == 0) {
      double saa = red[0][0], sbb = red[1][0], sab = red[2][0];
      for (int v = 1; v < NW; ++v) { saa += red[0][v]; sbb += red[1][v]; sab += red[2][v]; }
      int ok = 0;
      double ww = 0.0, ss = 1.0;
      if (saa > 0.0 && sbb > 0.0) {
        double c = sab / (sqrt(saa) * sqrt(sbb));
        c = fmin(1.0, fmax(-1.0, c));
        ww = acos(c);
        ss = sqrt(1.0 - c * c);
        ok = ss >= kSlerpMinSin;     // false for NaN too (non-finite codes): the lerp carries them through
      }
      bc[0] = ww; bc[1] = ss; use_slerp = ok;
    }
    __syncthreads();
    slerp = use_slerp != 0;
    w = bc[0]; s = bc[1];
  }

  for (int k = 0; k < steps; ++k) {
    const double t = alpha[k];
    const size_t row = (size_t)p * steps + k;
    double ca = 0.0, cb = 0.0;
    if (slerp) { ca = sin((1.0 - t) * w) / s; cb = sin(t * w) / s; }
    for (int j = tid; j < W; j += kLatentThreads) {
      float v;
      if (j < latent) {
        const float x = a[j], y = b[j];
        if (slerp) {
          v = (float)(ca * (double)x + cb * (double)y);
        } else {
          const float d = y - x;                          // float32, as z_b - z_a of two float32 arrays
          v = (float)((double)x + t * (double)d);         // float64 product, float64 sum, one rounding to float32
        }
        if (path) path[row * latent + j] = v;
      } else {
        v = cp[j - latent];
      }
      if (zc) zc[row * W + j] = v;
    }
  }
}

}  // namespace

int latent_path_check(const char* who, int pairs, int latent, const double* alpha, int steps, int mode) {
  const std::string p = std::string(who) + ": ";
  ICS_CHECK(pairs >= 1, p + "pairs must be >= 1");
  ICS_CHECK(latent >= 1, p + "latent must be >= 1");
  ICS_CHECK(steps >= 1, p + "steps must be >= 1");
  ICS_CHECK(mode == LATENT_LERP || mode == LATENT_SLERP, p + "unknown mode (0 = lerp, 1 = slerp)");
  ICS_CHECK(alpha != nullptr, p + "null alpha");
  for (int k = 0; k < steps; ++k)
    ICS_CHECK(std::isfinite(alpha[k]), p + "alpha[" + std::to_string(k) + "] is not finite");
  return 0;
}

int launch_latent_path(hipStream_t st, const float* za, const float* zb, size_t z_stride, const float* cond,
                       size_t cond_stride, int ncond, int pairs, int latent, const double* d_alpha, int steps, int mode,
                       float* zc, float* path) {
  ICS_CHECK(za && zb && d_alpha && (cond || ncond == 0) && (zc || path), "latent path: null device pointer");
  ICS_CHECK(pairs >= 1 && latent >= 1 && steps >= 1 && ncond >= 0, "latent path: bad extents");
  ICS_LAUNCH(latent_path_kernel, dim3((unsigned)pairs), dim3(kLatentThreads), 0, st, za, zb, z_stride, cond,
             cond_stride, ncond, latent, d_alpha, steps, mode, zc, path);
  ICS_HIP(hipGetLastError());
  return 0;
}

}  // namespace ics

using namespace ics;

// The pairs in chunks through the calling thread's scratch; synchronous on its stream.
extern "C" int ics_op_latent_path(const float* za, const float* zb, int pairs, int latent, const double* alpha, int steps,
                                  int mode, float* path) {
  ICS_TRY(latent_path_check("ics_op_latent_path", pairs, latent, alpha, steps, mode));
  ICS_CHECK(za && zb && path, "ics_op_latent_path: null argument (za, zb, path are required)");
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  const size_t per_pair = (size_t)steps * latent;
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)pairs, kLatentChunkFloats / per_pair));
  Layout L;
  const auto s_alpha = L.add<double>(steps);
  const auto s_a = L.add<float>((size_t)chunk * latent), s_b = L.add<float>((size_t)chunk * latent);
  const auto s_path = L.add<float>((size_t)chunk * per_pair);
  double* d_alpha;
  float *da, *db, *dp;
  ICS_TRY(L.reserve(s_alpha, &d_alpha, s_a, &da, s_b, &db, s_path, &dp));
  ICS_TRY(L.upload(s_alpha, alpha, steps, st));
  for (int p0 = 0; p0 < pairs; p0 += chunk) {
    const int n = std::min(chunk, pairs - p0);
    ICS_TRY(L.upload(s_a, za + (size_t)p0 * latent, (size_t)n * latent, st));
    ICS_TRY(L.upload(s_b, zb + (size_t)p0 * latent, (size_t)n * latent, st));
    ICS_TRY(launch_latent_path(st, da, db, (size_t)latent, nullptr, 0, 0, n, latent, d_alpha, steps, mode, nullptr, dp));
    ICS_TRY(L.download(path + (size_t)p0 * per_pair, s_path, (size_t)n * per_pair, st));
    ICS_HIP(hipStreamSynchronize(st));
  }
  return 0;
}
