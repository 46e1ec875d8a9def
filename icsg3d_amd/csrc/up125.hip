// The bandwidth passes of the 125-product up-split backward (up125.h): pooling of dy into the 125 blocks, the 27
// x-class volumes, the combine of the 27 class outputs into dxl and the contraction of the 125 block gradients to the
// 27 taps.  The GEMMs between them are launch_gemm_zbatch and launch_wgrad_zbatch (conv_igemm.hip).
#include "common.h"
#include "elementwise.h"
#include "up125.h"
#include "scratch.h"
#include "icsg3d.h"

#include <algorithm>
#include <string>

namespace ics {

typedef float qf4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------
// pool125, one wave per z type (ICSG3D_POOL125_V1; the default is pool125_planes_kernel below, which reads each plane once):
// one WAVE = one z type (blockDim = 5 waves), one lane = one tile x four channels.  A lane reads the 6 x 6 fine
// samples of the <= 4 planes its z type needs (216 float4 for the five waves of a tile where dy holds 64 per tile; the
// repeats are the same lines in the same workgroup), applies the x transform per line, and accumulates the 25 (y, x)
// types with the +-1 coefficients of up125_coef.  Out-of-range samples are 0 (the borders of up8.h's Q).
// ------------------------------------------------------------------------------------------
template <int TZ>
__device__ __forceinline__ void pool125_body(const float* __restrict__ dy, int S, int N, int b, int jz, int jy, int jx,
                                             unsigned tile, int n, float* __restrict__ out, const Up125Geom& u) {
  qf4 acc[5][5];
#pragma unroll
  for (int k = 0; k < 25; ++k) acc[k / 5][k % 5] = qf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int fz = 0; fz < 6; ++fz) {
    const int cz = up125_coef(TZ, fz);
    if (cz == 0) continue;
    const int z = 4 * jz - 1 + fz;
    if ((unsigned)z >= (unsigned)S) continue;
#pragma unroll
    for (int fy = 0; fy < 6; ++fy) {
      const int y = 4 * jy - 1 + fy;
      if ((unsigned)y >= (unsigned)S) continue;
      const float* line = dy + ((((size_t)b * S + z) * S + y) * S) * (size_t)N + n;
      qf4 v[6];
#pragma unroll
      for (int fx = 0; fx < 6; ++fx) {
        const int x = 4 * jx - 1 + fx;
        const bool ok = (unsigned)x < (unsigned)S;
        v[fx] = ok ? *reinterpret_cast<const qf4*>(line + (size_t)(ok ? x : 0) * N) : qf4{0.f, 0.f, 0.f, 0.f};
      }
      qf4 xr[5];
      const qf4 q0 = v[0] + v[1], q1 = v[2] + v[3], q2 = v[4] + v[5];
      xr[UP125_D1] = q0 - q1; xr[UP125_R0] = v[1] + v[2]; xr[UP125_Q1] = q1; xr[UP125_D2] = q1 - q2; xr[UP125_R1] = v[3] + v[4];
#pragma unroll
      for (int ty = 0; ty < 5; ++ty) {
        const int s = cz * up125_coef(ty, fy);
        if (s == 0) continue;
#pragma unroll
        for (int tx = 0; tx < 5; ++tx) {
          if (s > 0) acc[ty][tx] += xr[tx]; else acc[ty][tx] -= xr[tx];
        }
      }
    }
  }
#pragma unroll
  for (int ty = 0; ty < 5; ++ty)
#pragma unroll
    for (int tx = 0; tx < 5; ++tx) {
      const int q = up125_cls(TZ) * 9 + up125_cls(ty) * 3 + up125_cls(tx);
      *reinterpret_cast<qf4*>(out + up125_pooled_off(u, q, tile, up125_block(q, TZ, ty, tx), n)) = acc[ty][tx];
    }
}
__global__ __launch_bounds__(320) void pool125_kernel(const float* __restrict__ dy, int S, int lgc,
                                                      float* __restrict__ out, Up125Geom u) {
  const int tz = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = (((int)blockIdx.y << lgc) + (lane & ((1 << lgc) - 1))) * 4;
  const unsigned tile = blockIdx.x * (64u >> lgc) + (unsigned)(lane >> lgc);
  if (tile >= u.rows) return;
  const int T = u.T, lg = u.lgT;
  const int jx = tile & (T - 1), jy = (tile >> lg) & (T - 1), jz = (tile >> (2 * lg)) & (T - 1), b = tile >> (3 * lg);
  switch (tz) {
    case 0: pool125_body<0>(dy, S, u.N, b, jz, jy, jx, tile, n, out, u); break;
    case 1: pool125_body<1>(dy, S, u.N, b, jz, jy, jx, tile, n, out, u); break;
    case 2: pool125_body<2>(dy, S, u.N, b, jz, jy, jx, tile, n, out, u); break;
    case 3: pool125_body<3>(dy, S, u.N, b, jz, jy, jx, tile, n, out, u); break;
    default: pool125_body<4>(dy, S, u.N, b, jz, jy, jx, tile, n, out, u); break;
  }
}
// ------------------------------------------------------------------------------------------
// pool125, every fine plane once: one WAVE = one plane fz of the tile's 6 x 6 x 6 window (blockDim = 6 waves), lanes as
// above.  Stage 1 (up125_xline, up125_yacc): the wave loads its plane's 36 float4, and keeps the 25 (ty, tx) sums of
// that plane in registers: 216 float4 loaded per tile and channel quad where the kernel above loads 504.  Stage 2
// (up125_zcomb): the planes meet in LDS in five rounds of one ty each (6 planes x 5 tx x 64 lanes x 16 B = 30 KB, two
// buffers so that a round's stores need not wait for the previous round's loads: one barrier per round); the wave
// that owns z type tz (waves 0..4) reads the <= 4 planes of its type and stores the five blocks of the round.
// EVERY wave reaches EVERY barrier: a plane outside the volume and a tile row past the end only turn loads into zeros
// and switch the global stores off; nothing returns early and no barrier stands inside a condition.
// ------------------------------------------------------------------------------------------
template <int TZ>
__device__ __forceinline__ void pool125_zstore(const qf4* __restrict__ buf, int lane, int ty, bool live, unsigned tile, int n,
                                               float* __restrict__ out, const Up125Geom& u) {
#pragma unroll
  for (int tx = 0; tx < 5; ++tx) {
    qf4 s[6];
#pragma unroll
    for (int fz = 0; fz < 6; ++fz)
      s[fz] = up125_coef(TZ, fz) != 0 ? buf[up125_xch_off(fz, tx, lane)] : qf4{0.f, 0.f, 0.f, 0.f};
    const qf4 v = up125_zcomb(TZ, s);
    const int q = up125_cls(TZ) * 9 + up125_cls(ty) * 3 + up125_cls(tx);
    if (live) *reinterpret_cast<qf4*>(out + up125_pooled_off(u, q, tile, up125_block(q, TZ, ty, tx), n)) = v;
  }
}
__global__ __launch_bounds__(64 * UP125_POOL_WAVES) void pool125_planes_kernel(const float* __restrict__ dy, int S, int lgc,
                                                                               float* __restrict__ out, Up125Geom u) {
  __shared__ qf4 xch[2][UP125_XCH_ELEMS];
  const int fz = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned tile;
  int n;
  up125_pool_lane(lgc, blockIdx.x, blockIdx.y, lane, &tile, &n);
  const bool live = tile < u.rows;   // a tile row past the end: no global access, but every barrier below
  const int T = u.T, lg = u.lgT, N = u.N;
  const int jx = tile & (T - 1), jy = (tile >> lg) & (T - 1), jz = (tile >> (2 * lg)) & (T - 1), b = tile >> (3 * lg);
  // stage 1: this wave's plane
  qf4 Sa[25];
#pragma unroll
  for (int k = 0; k < 25; ++k) Sa[k] = qf4{0.f, 0.f, 0.f, 0.f};
  const int z = 4 * jz - 1 + fz;
  const bool zok = live && (unsigned)z < (unsigned)S;
#pragma unroll
  for (int fy = 0; fy < 6; ++fy) {
    const int y = 4 * jy - 1 + fy;
    const bool yok = zok && (unsigned)y < (unsigned)S;
    const float* line = dy + (yok ? ((((size_t)b * S + z) * S + y) * S) * (size_t)N + n : (size_t)0);
    qf4 v[6];
#pragma unroll
    for (int fx = 0; fx < 6; ++fx) {
      const int x = 4 * jx - 1 + fx;
      const bool ok = yok && (unsigned)x < (unsigned)S;
      v[fx] = ok ? *reinterpret_cast<const qf4*>(line + (size_t)(ok ? x : 0) * N) : qf4{0.f, 0.f, 0.f, 0.f};
    }
    qf4 xr[5];
    up125_xline(v, xr);
    up125_yacc(fy, xr, Sa);
  }
  // stage 2: five rounds of one ty
#pragma unroll
  for (int ty = 0; ty < UP125_POOL_ROUNDS; ++ty) {
    qf4* buf = xch[ty & 1];
#pragma unroll
    for (int tx = 0; tx < 5; ++tx) buf[up125_xch_off(fz, tx, lane)] = Sa[ty * 5 + tx];
    __syncthreads();
    // buf is written again in round ty + 2, behind the barrier of round ty + 1, which every reader of this round has passed
    switch (fz) {   // wave-uniform; wave 5 owns no z type
      case 0: pool125_zstore<0>(buf, lane, ty, live, tile, n, out, u); break;
      case 1: pool125_zstore<1>(buf, lane, ty, live, tile, n, out, u); break;
      case 2: pool125_zstore<2>(buf, lane, ty, live, tile, n, out, u); break;
      case 3: pool125_zstore<3>(buf, lane, ty, live, tile, n, out, u); break;
      case 4: pool125_zstore<4>(buf, lane, ty, live, tile, n, out, u); break;
      default: break;
    }
  }
}
int launch_pool125(hipStream_t st, const float* dy, int B, int S, int N, float* out, const Up125Geom& u, bool v1) {
  ICS_CHECK(up125_shape_ok(S, N, u.Cu, B) && u.T == S / 4 && u.N == N && (1 << u.lgT) == u.T &&
                u.rows == (unsigned)B * (unsigned)(u.T * u.T * u.T),
            "pool125: layout does not match the shape");
  int lgc = 0;
  while ((1 << lgc) < std::min(N / 4, 64)) ++lgc;   // float4 columns of a tile per wave (N = 32 * 2^k: a power of two)
  const unsigned tpw = 64u >> lgc;
  const dim3 grid((u.rows + tpw - 1) / tpw, (unsigned)((N / 4) >> lgc));
  if (v1) ICS_LAUNCH(pool125_kernel, grid, dim3(320), 0, st, dy, S, lgc, out, u);
  else ICS_LAUNCH(pool125_planes_kernel, grid, dim3(64 * UP125_POOL_WAVES), 0, st, dy, S, lgc, out, u);
  ICS_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// x classes: X_q[row][c] with (x[2j], x[2j] + x[2j+1], x[2j+1]) per axis of the low-res source, the producer's affine and
// activation applied first, as the backward-weight loader applies them.  One thread = one tile x four channels.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void up125_xclass_kernel(ConvSrc s, size_t total, float* __restrict__ out, Up125Geom u) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int C4 = u.Cu >> 2, T = u.T, lg = u.lgT, Sh = 2 * T;
  const int c = (int)(i % C4) * 4;
  const unsigned tile = (unsigned)(i / C4);
  const int jx = tile & (T - 1), jy = (tile >> lg) & (T - 1), jz = (tile >> (2 * lg)) & (T - 1), b = tile >> (3 * lg);
  const bool aff = s.scale != nullptr;
  qf4 sc = qf4{1.f, 1.f, 1.f, 1.f}, sh = qf4{0.f, 0.f, 0.f, 0.f};
  if (aff) { sc = *reinterpret_cast<const qf4*>(s.scale + c); sh = *reinterpret_cast<const qf4*>(s.shift + c); }
  const float slope = aff ? (s.act == ACT_RELU ? 0.f : (s.act == ACT_LRELU ? kLeaky : 1.f)) : 1.f;
  qf4 X[3][3][3];
#pragma unroll
  for (int ez = 0; ez < 2; ++ez)
#pragma unroll
    for (int ey = 0; ey < 2; ++ey) {
      qf4 p[2];
#pragma unroll
      for (int ex = 0; ex < 2; ++ex) {
        const size_t vox = (((size_t)b * Sh + 2 * jz + ez) * Sh + 2 * jy + ey) * Sh + 2 * jx + ex;
        qf4 v = *reinterpret_cast<const qf4*>(s.p + vox * (size_t)s.C + c);
        if (aff) {
          v.x = fmaf(v.x, sc.x, sh.x); v.y = fmaf(v.y, sc.y, sh.y); v.z = fmaf(v.z, sc.z, sh.z); v.w = fmaf(v.w, sc.w, sh.w);
          v.x = fmaxf(v.x, v.x * slope); v.y = fmaxf(v.y, v.y * slope); v.z = fmaxf(v.z, v.z * slope); v.w = fmaxf(v.w, v.w * slope);
        }
        p[ex] = v;
      }
      X[2 * ez][2 * ey][0] = p[0]; X[2 * ez][2 * ey][1] = p[0] + p[1]; X[2 * ez][2 * ey][2] = p[1];
    }
#pragma unroll
  for (int ez = 0; ez < 2; ++ez)
#pragma unroll
    for (int cx = 0; cx < 3; ++cx) X[2 * ez][1][cx] = X[2 * ez][0][cx] + X[2 * ez][2][cx];
#pragma unroll
  for (int cy = 0; cy < 3; ++cy)
#pragma unroll
    for (int cx = 0; cx < 3; ++cx) X[1][cy][cx] = X[0][cy][cx] + X[2][cy][cx];
#pragma unroll
  for (int q = 0; q < 27; ++q)
    *reinterpret_cast<qf4*>(out + up125_class_off(u, q, tile, c)) = X[q / 9][(q / 3) % 3][q % 3];
}
int launch_up125_xclass(hipStream_t st, const ConvSrc& s, float* out, const Up125Geom& u) {
  ICS_CHECK(s.C == u.Cu && u.Cu % 4 == 0 && !s.up && !s.bcast && u.rows > 0, "up125 x classes: plain low-res source required");
  const size_t total = (size_t)u.rows * (u.Cu / 4);
  ICS_LAUNCH(up125_xclass_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, s, total, out, u);
  ICS_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// combine: dxl[coarse voxel (2j + e per axis)][c] = sum of the 8 class outputs with digit e or e + 1 per axis
// (dx[2j] = A + B, dx[2j+1] = B + C).  One thread = one tile x four channels: 27 loads, 8 stores.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void up125_combine_kernel(const float* __restrict__ cls, size_t total,
                                                            float* __restrict__ dxl, Up125Geom u) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int C4 = u.Cu >> 2, T = u.T, lg = u.lgT, Sh = 2 * T;
  const int c = (int)(i % C4) * 4;
  const unsigned tile = (unsigned)(i / C4);
  const int jx = tile & (T - 1), jy = (tile >> lg) & (T - 1), jz = (tile >> (2 * lg)) & (T - 1), b = tile >> (3 * lg);
  qf4 O[3][3][3];
#pragma unroll
  for (int q = 0; q < 27; ++q) O[q / 9][(q / 3) % 3][q % 3] = *reinterpret_cast<const qf4*>(cls + up125_class_off(u, q, tile, c));
#pragma unroll
  for (int ez = 0; ez < 2; ++ez)
#pragma unroll
    for (int ey = 0; ey < 2; ++ey)
#pragma unroll
      for (int ex = 0; ex < 2; ++ex) {
        qf4 v = qf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 8; ++k) v += O[ez + (k >> 2)][ey + ((k >> 1) & 1)][ex + (k & 1)];
        const size_t vox = (((size_t)b * Sh + 2 * jz + ez) * Sh + 2 * jy + ey) * Sh + 2 * jx + ex;
        *reinterpret_cast<qf4*>(dxl + vox * (size_t)u.Cu + c) = v;
      }
}
int launch_up125_combine(hipStream_t st, const float* cls, float* dxl, const Up125Geom& u) {
  ICS_CHECK(u.Cu % 4 == 0 && u.rows > 0, "up125 combine: channels must be a multiple of 4");
  const size_t total = (size_t)u.rows * (u.Cu / 4);
  ICS_LAUNCH(up125_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, cls, total, dxl, u);
  ICS_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// contraction: dw_up[cu][tap N + n] = sum over the 8 (class, block) products of the tap, sign from up125_wcoef, each
// summed over its split-K partials in split order (fixed order: the result does not depend on the schedule).
// ws: group g at ws + p.off[g], laid out [class of the group][split][Cu][nb N].
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void up125_contract_kernel(const float* __restrict__ ws, Up125Splits p, size_t total,
                                                             float* __restrict__ dw, Up125Geom u) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int N4 = u.N >> 2;
  const int n = (int)(i % N4) * 4;
  const int tap = (int)((i / N4) % 27);
  const int cu = (int)(i / ((size_t)N4 * 27));
  const int iz = tap / 9, iy = (tap / 3) % 3, ix = tap % 3;
  qf4 v = qf4{0.f, 0.f, 0.f, 0.f};
  for (int tz = 0; tz < 5; ++tz) {
    const int sz = up125_wcoef(tz, iz);
    if (sz == 0) continue;
    for (int ty = 0; ty < 5; ++ty) {
      const int sy = sz * up125_wcoef(ty, iy);
      if (sy == 0) continue;
      for (int tx = 0; tx < 5; ++tx) {
        const int s = sy * up125_wcoef(tx, ix);
        if (s == 0) continue;
        const int q = up125_cls(tz) * 9 + up125_cls(ty) * 3 + up125_cls(tx);
        const int g = up125_nB(q), nb = 8 >> g, ks = p.ks[g];
        const size_t ld = (size_t)nb * u.N;
        const float* base = ws + p.off[g] + ((size_t)(u.slot[q] - up125_group_slot0(g)) * ks * u.Cu + cu) * ld +
                            (size_t)up125_block(q, tz, ty, tx) * u.N + n;
        // four independent partial sums keep four loads in flight (one dependent chain sat at the load latency); the
        // order is fixed by k alone
        const size_t st = (size_t)u.Cu * ld;
        qf4 a0 = qf4{0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
        int k = 0;
        for (; k + 4 <= ks; k += 4) {
          a0 += *reinterpret_cast<const qf4*>(base + (size_t)k * st);
          a1 += *reinterpret_cast<const qf4*>(base + (size_t)(k + 1) * st);
          a2 += *reinterpret_cast<const qf4*>(base + (size_t)(k + 2) * st);
          a3 += *reinterpret_cast<const qf4*>(base + (size_t)(k + 3) * st);
        }
        for (; k < ks; ++k) a0 += *reinterpret_cast<const qf4*>(base + (size_t)k * st);
        const qf4 a = (a0 + a1) + (a2 + a3);
        if (s > 0) v += a; else v -= a;
      }
    }
  }
  *reinterpret_cast<qf4*>(dw + ((size_t)cu * 27 + tap) * u.N + n) = v;
}
int launch_up125_contract(hipStream_t st, const float* ws, const Up125Splits& p, float* dw, const Up125Geom& u) {
  ICS_CHECK(u.N % 4 == 0, "up125 contraction: channels must be a multiple of 4");
  const size_t total = (size_t)u.Cu * 27 * (u.N / 4);
  ICS_LAUNCH(up125_contract_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ws, p, total, dw, u);
  ICS_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// class weight images (up125_pack_piece) outside a pack table
// ------------------------------------------------------------------------------------------
__global__ void pack_up125_kernel(const float* __restrict__ w, int Cin_total, int N, int c_off, int Cu, size_t total,
                                  float* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) up125_pack_piece(i, w, Cin_total, N, c_off, Cu, dst);
}
int launch_pack_up125_pieces(hipStream_t st, const float* w, int Cin_total, int N, int c_off, int Cu, float* dst) {
  const size_t total = up125_pack_pieces(N, Cu);
  ICS_LAUNCH(pack_up125_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w, Cin_total, N, c_off, Cu, total, dst);
  ICS_HIP(hipGetLastError());
  return 0;
}

}  // namespace ics

using namespace ics;

extern "C" {

// the pooling pass alone on a host array (include/icsg3d.h)
int ics_op_up125_pool(const float* dy, int B, int S, int N, int variant, float* out) {
  const std::string op = "ics_op_up125_pool: ";
  ICS_CHECK(dy && out, op + "dy and out are required");
  ICS_CHECK(variant == 0 || variant == 1, op + "variant is 0 (one wave per z type) or 1 (one wave per fine plane)");
  ICS_CHECK(up125_shape_ok(S, N, 64, B), op + "need S a power of two >= 8, N = 32 * 2^k and B (S/4)^3 * 8 N < 2^30");
  const Up125Geom u = up125_geom(B, S, N, 64);
  const size_t cnt = (size_t)B * S * S * S * N, pooled = up125_pooled_floats(u.rows, N);
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  Layout L;
  const auto s_dy = L.add<float>(cnt);
  const auto s_out = L.add<float>(pooled);
  float *d_dy, *d_out;
  ICS_TRY(L.reserve(s_dy, &d_dy, s_out, &d_out));
  ICS_TRY(L.upload(s_dy, dy, cnt, st));
  ICS_TRY(launch_pool125(st, d_dy, B, S, N, d_out, u, variant == 0));
  ICS_TRY(L.download(out, s_out, pooled, st));
  ICS_HIP(hipStreamSynchronize(st));
  return 0;
}

}  // extern "C"
