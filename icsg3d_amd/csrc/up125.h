// Layout of the 125-product form of the up-split backward (the pool125 kernels, the class GEMMs, the combine / contraction
// kernels of up125.hip, engine.hip and hoststub/up125_check.cpp all take their arithmetic from here).
//
// up8.h: per axis, with a the coarse coordinate,  R[a] = dy[2a] + dy[2a+1],  Q[a] = dy[2a-1] + dy[2a]  and
//   dx[a] = wp Q[a] + wc R[a] + wm Q[a+1]          (wp / wc / wm: the taps at offsets +1 / 0 / -1, tap index 2 / 1 / 0).
// For the coarse pair (2j, 2j+1) of TILE j (T = S/4 tiles per axis) five pooled TYPES
//   D1 = Q[2j] - Q[2j+1]   R0 = R[2j]   Q1 = Q[2j+1]   D2 = Q[2j+1] - Q[2j+2]   R1 = R[2j+1]
// give three output CLASSES
//   A = wp D1 + wc R0      B = (wp + wm) Q1      C = -wm D2 + wc R1        dx[2j] = A + B,  dx[2j+1] = B + C:
// five products for two outputs instead of six.  In three dimensions: 5^3 = 125 blocks per tile, accumulated into 27
// classes q = (cz, cy, cx); class q owns nb(q) = 2^(number of A/C digits) blocks, i.e. it is ONE dense GEMM
//   O_q[rows][Cu] = P_q[rows][nb Cout] x W_q[nb Cout][Cu],      rows = B T^3,
// and the transpose, dW_q[Cu][nb Cout] = X_q^T P_q with X = (x[2j], x[2j] + x[2j+1], x[2j+1]) per axis, is the
// backward-weight form.  Classes of equal nb are consecutive ("slots"), so a group of them is one z-batched launch:
//   group g = number of B digits: nb = 8, 4, 2, 1; 8, 12, 6, 1 classes; first slot 0, 8, 20, 26; first block 0, 64, 112, 124.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ICS_UP125_HD __host__ __device__ constexpr inline
#define ICS_UP125_F __host__ __device__ inline
#else
#define ICS_UP125_HD constexpr inline
#define ICS_UP125_F inline
#endif

enum { UP125_D1 = 0, UP125_R0 = 1, UP125_Q1 = 2, UP125_D2 = 3, UP125_R1 = 4 };

// per axis: class of a type (0 = A, 1 = B, 2 = C), index of the type among its class's blocks, blocks of a class
ICS_UP125_HD int up125_cls(int t) { return t < 2 ? 0 : (t == 2 ? 1 : 2); }
ICS_UP125_HD int up125_e(int t) { return t < 2 ? t : (t == 2 ? 0 : t - 3); }
ICS_UP125_HD int up125_n(int c) { return c == 1 ? 1 : 2; }
ICS_UP125_HD int up125_type(int c, int e) { return c == 0 ? e : (c == 1 ? UP125_Q1 : 3 + e); }
// coefficient of fine sample f = 0..5 (coordinate 4j - 1 + f, out-of-range dy = 0) in type t
ICS_UP125_HD int up125_coef(int t, int f) {
  return t == UP125_D1 ? (f < 2 ? 1 : (f < 4 ? -1 : 0))
       : t == UP125_R0 ? (f == 1 || f == 2)
       : t == UP125_Q1 ? (f == 2 || f == 3)
       : t == UP125_D2 ? ((f == 2 || f == 3) ? 1 : (f >= 4 ? -1 : 0))
                       : (f == 3 || f == 4);
}
// coefficient of tap index i (0: offset -1 = wm, 1: wc, 2: offset +1 = wp) in the weight that multiplies type t;
// read along t it is also the sign with which the product x-class x type enters the gradient of tap i
ICS_UP125_HD int up125_wcoef(int t, int i) {
  return t == UP125_D1 ? (i == 2) : t == UP125_Q1 ? (i != 1) : t == UP125_D2 ? -(i == 0) : (i == 1);
}

// 3-d class q = cz*9 + cy*3 + cx
ICS_UP125_HD int up125_nB(int q) { return (q / 9 == 1) + ((q / 3) % 3 == 1) + (q % 3 == 1); }
ICS_UP125_HD int up125_nb(int q) { return 8 >> up125_nB(q); }
ICS_UP125_HD int up125_group_slot0(int g) { return g == 0 ? 0 : (g == 1 ? 8 : (g == 2 ? 20 : 26)); }
ICS_UP125_HD int up125_group_block0(int g) { return g == 0 ? 0 : (g == 1 ? 64 : (g == 2 ? 112 : 124)); }
ICS_UP125_HD int up125_group_classes(int g) { return g == 0 ? 8 : (g == 1 ? 12 : (g == 2 ? 6 : 1)); }
ICS_UP125_HD int up125_slot(int q) {
  const int g = up125_nB(q);
  int r = 0;
  for (int p = 0; p < q; ++p) r += up125_nB(p) == g;
  return up125_group_slot0(g) + r;
}
ICS_UP125_HD int up125_class_of_slot(int s) {
  for (int q = 0; q < 27; ++q)
    if (up125_slot(q) == s) return q;
  return -1;
}
// blocks that precede class q's in the pooled buffer (and in the class weight images)
ICS_UP125_HD int up125_bbase(int q) {
  const int g = up125_nB(q);
  return up125_group_block0(g) + (up125_slot(q) - up125_group_slot0(g)) * (8 >> g);
}
// block of class q that holds the per-axis types (tz, ty, tx) (each of its own axis class)
ICS_UP125_HD int up125_block(int q, int tz, int ty, int tx) {
  return (up125_e(tz) * up125_n((q / 3) % 3) + up125_e(ty)) * up125_n(q % 3) + up125_e(tx);
}

struct Up125Geom {
  int T = 0, lgT = 0;          // tiles per axis (S / 4) and its log2
  int N = 0, Cu = 0;           // channels of dy; channels of the low-res source
  unsigned rows = 0;           // B * T^3 tile rows of the batch at hand
  unsigned char slot[27] = {};   // by class q
  unsigned char bbase[27] = {};
};

inline Up125Geom up125_geom(int B, int S, int N, int Cu) {
  Up125Geom u;
  u.T = S / 4;
  while ((1 << u.lgT) < u.T) ++u.lgT;
  u.N = N; u.Cu = Cu;
  u.rows = (unsigned)B * (unsigned)u.T * (unsigned)u.T * (unsigned)u.T;
  for (int q = 0; q < 27; ++q) { u.slot[q] = (unsigned char)up125_slot(q); u.bbase[q] = (unsigned char)up125_bbase(q); }
  return u;
}

// buffer sizes in floats: the 125 pooled blocks; the 27 x-class volumes or the 27 class outputs
ICS_UP125_HD size_t up125_pooled_floats(size_t rows, int N) { return 125 * rows * (size_t)N; }
ICS_UP125_HD size_t up125_class_floats(size_t rows, int Cu) { return 27 * rows * (size_t)Cu; }
// the class weight images W_q[nb N][Cu] (packed [K/4][Cu][4]), class q at up125_bbase(q) * N * Cu
ICS_UP125_HD size_t up125_weight_floats(int N, int Cu) { return (size_t)125 * N * Cu; }

// float offset of (class q, tile row, block b of the class, channel n): row-major [rows][nb N] per class
ICS_UP125_F size_t up125_pooled_off(const Up125Geom& u, int q, size_t row, int b, int n) {
  return ((size_t)u.bbase[q] * u.rows + row * (size_t)up125_nb(q) + (size_t)b) * (size_t)u.N + (size_t)n;
}
// float offset of (class q, tile row, channel c) in the x-class volumes / class outputs
ICS_UP125_F size_t up125_class_off(const Up125Geom& u, int q, size_t row, int c) {
  return ((size_t)u.slot[q] * u.rows + row) * (size_t)u.Cu + (size_t)c;
}

// Shapes the layout serves.  S: FINE extent of the layer (power of two, S/4 >= 2 tiles per axis); N = 32 * 2^k: K = nb N
// of a class GEMM is whole 32-channel chunks and a wave of pool125_kernel covers whole tiles; Cu % 64: the N tile of the z-batched GEMM; every matrix inside 32-bit offsets
ICS_UP125_HD bool up125_shape_ok(int S, int N, int Cu, int B) {
  if (S < 8 || (S & (S - 1)) != 0 || N < 32 || (N & (N - 1)) != 0 || Cu < 64 || Cu % 64 != 0 || B < 1) return false;
  const size_t rows = (size_t)B * (S / 4) * (S / 4) * (S / 4);
  const size_t w = (size_t)(8 * N > Cu ? 8 * N : Cu);
  return rows * w < ((size_t)1 << 30);
}

// ---- pooling of dy into the 125 blocks, one fine plane at a time (pool125_planes_kernel and hoststub/pool125_check.cpp
// run these same functions; V is a float4 on the device and a float on the host).  The blocks are separable: per axis
// the five types are +-1 combinations of the six window samples, so a plane fz of a tile's window is loaded, x-transformed
// and (y, x)-accumulated ONCE into the 25 partial sums S_fz[ty][tx], and the z combination of the six sets comes last.
enum { UP125_POOL_WAVES = 6, UP125_POOL_ROUNDS = 5, UP125_XCH_ELEMS = 6 * 5 * 64 };
// lane of wave-sized group (bx, by) -> tile row and first channel: 2^lgc float4 columns of N per tile, 64 >> lgc tiles
ICS_UP125_F void up125_pool_lane(int lgc, unsigned bx, unsigned by, int lane, unsigned* tile, int* n) {
  *n = (int)(((by << lgc) + ((unsigned)lane & ((1u << lgc) - 1u))) * 4u);
  *tile = bx * (64u >> lgc) + ((unsigned)lane >> lgc);
}
// element of one exchange round (one ty): plane fz, x type tx, lane -- a wave's 64 lanes adjoin
ICS_UP125_HD int up125_xch_off(int fz, int tx, int lane) { return (fz * 5 + tx) * 64 + lane; }
// stage 1, x transform of one line of six samples
template <class V>
ICS_UP125_F void up125_xline(const V* v, V* xr) {
  const V q0 = v[0] + v[1], q1 = v[2] + v[3], q2 = v[4] + v[5];
  xr[UP125_D1] = q0 - q1; xr[UP125_R0] = v[1] + v[2]; xr[UP125_Q1] = q1; xr[UP125_D2] = q1 - q2; xr[UP125_R1] = v[3] + v[4];
}
// stage 1, line fy of the plane enters the (ty, tx) sums S[ty * 5 + tx] with the sign of up125_coef(ty, fy)
template <class V>
ICS_UP125_F void up125_yacc(int fy, const V* xr, V* S) {
#pragma unroll
  for (int ty = 0; ty < 5; ++ty) {
    const int s = up125_coef(ty, fy);
    if (s == 0) continue;
#pragma unroll
    for (int tx = 0; tx < 5; ++tx) {
      if (s > 0) S[ty * 5 + tx] += xr[tx]; else S[ty * 5 + tx] -= xr[tx];
    }
  }
}
// stage 2, z type tz from the planes' sums s[fz]; only the planes with up125_coef(tz, fz) != 0 are read
template <class V>
ICS_UP125_F V up125_zcomb(int tz, const V* s) {
  return tz == UP125_D1 ? (s[0] + s[1]) - (s[2] + s[3])
       : tz == UP125_R0 ? s[1] + s[2]
       : tz == UP125_Q1 ? s[2] + s[3]
       : tz == UP125_D2 ? (s[2] + s[3]) - (s[4] + s[5])
                        : s[3] + s[4];
}

// ---- class weight images, as the pack jobs build them: piece i = ((tz * 5 + ty) * (N / 4) + n4) * Cu + c  (c fastest:
// the stores of neighbouring threads adjoin) reads the <= 12 taps its (tz, ty) needs at (input channel c, output
// channels 4 n4 .. 4 n4 + 3) and writes the five tx blocks' 16-byte pieces of the packed images [K/4][Cu][4].
// up125_weight_value below defines the same images element by element (the host check compares the two).
ICS_UP125_HD size_t up125_pack_pieces(int N, int Cu) { return (size_t)25 * (N / 4) * Cu; }
ICS_UP125_F void up125_pack_piece(size_t i, const float* w, int Cin_total, int N, int c_off, int Cu, float* dst) {
  const int c = (int)(i % (size_t)Cu);
  size_t r = i / (size_t)Cu;
  const int n = (int)(r % (size_t)(N / 4)) * 4;
  r /= (size_t)(N / 4);
  const int ty = (int)(r % 5), tz = (int)(r / 5);
  float sx[3][4] = {};
  for (int iz = 0; iz < 3; ++iz)
    for (int iy = 0; iy < 3; ++iy) {
      const int s = up125_wcoef(tz, iz) * up125_wcoef(ty, iy);
      if (s == 0) continue;
      for (int ix = 0; ix < 3; ++ix) {
        const float* p = w + ((size_t)((iz * 3 + iy) * 3 + ix) * Cin_total + c_off + c) * N + n;
        for (int k = 0; k < 4; ++k) sx[ix][k] += (float)s * p[k];
      }
    }
  for (int tx = 0; tx < 5; ++tx) {
    const int q = up125_cls(tz) * 9 + up125_cls(ty) * 3 + up125_cls(tx);
    const int k0 = up125_block(q, tz, ty, tx) * N + n;   // row of the class image [nb N][Cu]; k0 % 4 == 0
    float* d = (float*)__builtin_assume_aligned(dst + (size_t)up125_bbase(q) * N * Cu + ((size_t)(k0 / 4) * Cu + c) * 4, 16);
    for (int k = 0; k < 4; ++k) {
      float v = 0.f;
      for (int ix = 0; ix < 3; ++ix) {
        const int s = up125_wcoef(tx, ix);
        if (s != 0) v += (float)s * sx[ix][k];
      }
      d[k] = v;
    }
  }
}

// ---- class weight images: element i of class q's packed image [K/4][Cu][4], K = nb N, from w[27][Cin_total][N]
// (Keras layout; the upsampled channels start at c_off)
ICS_UP125_F float up125_weight_value(size_t i, const float* w, int Cin_total, int N, int c_off, int Cu, int q) {
  const int tq = (int)(i & 3);
  const size_t rest = i >> 2;
  const int c = (int)(rest % (size_t)Cu);
  const int k = (int)(rest / (size_t)Cu) * 4 + tq;
  int b = k / N;
  const int n = k - b * N;
  const int cz = q / 9, cy = (q / 3) % 3, cx = q % 3;
  const int ex = b % up125_n(cx); b /= up125_n(cx);
  const int ey = b % up125_n(cy); b /= up125_n(cy);
  const int tz = up125_type(cz, b), ty = up125_type(cy, ey), tx = up125_type(cx, ex);
  float v = 0.f;
  for (int iz = 0; iz < 3; ++iz)
    for (int iy = 0; iy < 3; ++iy)
      for (int ix = 0; ix < 3; ++ix) {
        const int s = up125_wcoef(tz, iz) * up125_wcoef(ty, iy) * up125_wcoef(tx, ix);
        if (s != 0) v += (float)s * w[((size_t)((iz * 3 + iy) * 3 + ix) * Cin_total + c_off + c) * N + n];
      }
  return v;
}
