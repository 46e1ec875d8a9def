// Layout of the 8 pooled volumes of the up-split backward (pool8_kernel, the two coarse-grid GEMM loaders, engine.hip
// and hoststub/up8_check.cpp all take their address arithmetic from here).
//
// pool27 materialises dyS[vl][tap][n]: dy summed over the <= 8 fine voxels that tap `tap` maps onto coarse voxel vl.
// Per axis, with a the coarse coordinate, Sh = S/2 and out-of-range dy = 0, there are only two distinct pair sums
//   R[a] = dy[2a]   + dy[2a+1]   a = 0..Sh-1    (tap offset d =  0)
//   Q[a] = dy[2a-1] + dy[2a]     a = 0..Sh      (tap offset d = +1 reads Q[a], d = -1 reads Q[a+1])
// so the 27 tap copies are 2 x 2 x 2 = 8 volumes read at 27 row shifts.
//
// A volume has index k = kz*4 + ky*2 + kx (0 = R, 1 = Q per axis).  Every volume has extents P^3 per sample,
// P = Sh + 1, channels innermost with pitch N; volumes are `vstride` floats apart, vstride = B * P^3 * N for the
// batch B AT HAND (a handle runs any batch up to max_batch; the allocation is sized by max_batch and a smaller batch
// uses a prefix of it, so each launch touches a dense range).  Slot Sh of an R-type axis is never written by the pool
// kernel under its own batch's layout and never read by a loader.
// The largest row a loader reads is prow(M-1) + (P*P + P + 1) = B*P^3 - 1: inside the volume by construction.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ICS_UP8_HD __host__ __device__ inline
#else
#define ICS_UP8_HD inline
#endif

struct Up8Geom {
  int P = 0;             // padded extent Sh + 1
  int lgSh = 0;          // log2 of the coarse extent
  int N = 0;             // channels of dy (a power of two times 32)
  int lgcpt = 0;         // log2(N / 32): 32-channel chunks per tap
  unsigned vstride = 0;  // floats between consecutive volumes
  // float offset of tap t's reads from the buffer base: volume base + row shift.  Filled by up8_geom on the host; a
  // kernel indexes it with a wave-uniform tap (one scalar load from its arguments instead of the divisions of up8_tap)
  unsigned tapoff[27] = {};
};

struct Up8Tap {
  int vol;     // volume index 0..7
  int shift;   // row shift in padded rows
};

// tap = (dz+1)*9 + (dy+1)*3 + (dx+1), the numbering of pool27 and w_up.
// Per axis: d = 0 -> (R, shift 0), d = +1 -> (Q, shift 0), d = -1 -> (Q, shift 1).
ICS_UP8_HD Up8Tap up8_tap(int tap, int P) {
  const int dz = tap / 9 - 1, dy = (tap / 3) % 3 - 1, dx = tap % 3 - 1;
  const int vol = (dz != 0 ? 4 : 0) + (dy != 0 ? 2 : 0) + (dx != 0 ? 1 : 0);
  const int shift = ((dz < 0 ? 1 : 0) * P + (dy < 0 ? 1 : 0)) * P + (dx < 0 ? 1 : 0);
  return Up8Tap{vol, shift};
}

// padded row of coarse voxel m = ((b*Sh + z)*Sh + y)*Sh + x
ICS_UP8_HD unsigned up8_prow(unsigned m, int lgSh, int P) {
  const unsigned mask = (1u << lgSh) - 1u;
  const unsigned x = m & mask, y = (m >> lgSh) & mask, z = (m >> (2 * lgSh)) & mask, b = m >> (3 * lgSh);
  return ((b * (unsigned)P + z) * (unsigned)P + y) * (unsigned)P + x;
}

ICS_UP8_HD size_t up8_volume_floats(int B, int Sh, int N) {
  const size_t P = (size_t)Sh + 1;
  return (size_t)B * P * P * P * (size_t)N;
}

ICS_UP8_HD Up8Geom up8_geom(int B, int Sh, int lgSh, int N) {
  Up8Geom u;
  u.P = Sh + 1;
  u.lgSh = lgSh;
  u.N = N;
  int l = 0;
  while ((32 << l) < N) ++l;
  u.lgcpt = l;
  u.vstride = (unsigned)up8_volume_floats(B, Sh, N);
  for (int t = 0; t < 27; ++t) {
    const Up8Tap tp = up8_tap(t, u.P);
    u.tapoff[t] = (unsigned)tp.vol * u.vstride + (unsigned)tp.shift * (unsigned)N;   // < 2^30 floats (up8_shape_ok)
  }
  return u;
}

// Shapes the layout serves.  S: FINE extent of the layer (power of two); M8 = B * (S/2)^3 coarse rows.
//  S >= 8: at Sh >= 4 the 5 low bits of a coarse row are whole (z,y,x) digits, so prow(mbase + r) = prow(mbase) + prow(r)
//  for a 32-aligned mbase (backward-weight chunks); N = 32 * 2^k: a 32-channel K chunk lies inside one tap and the
//  tap of a chunk is a shift; whole 32-row chunks; every byte offset into the 8 volumes fits in 32 bits.
ICS_UP8_HD bool up8_shape_ok(int S, int N, size_t M8, int B) {
  if (S < 8 || (S & (S - 1)) != 0 || N < 32 || (N & (N - 1)) != 0 || M8 % 32 != 0) return false;
  return 8 * up8_volume_floats(B, S / 2, N) * sizeof(float) <= 0xffffffffull;
}

// ---- backward-data loader (conv_fwd_kernel): A[m][k], k = tap*N + channel, 32-channel chunk c.
// wave-uniform float offset of chunk c from the buffer base (volume base + row shift + channel offset)
ICS_UP8_HD size_t up8_chunk_floats(int c, const Up8Geom& u) {
  const int tap = c >> u.lgcpt, cc = c & ((1 << u.lgcpt) - 1);
  return (size_t)(u.tapoff[tap] + (unsigned)cc * 32u);
}
// per-row float offset, fixed for the kernel
ICS_UP8_HD unsigned up8_row_floats(unsigned m, const Up8Geom& u) { return up8_prow(m, u.lgSh, u.P) * (unsigned)u.N; }

// ---- backward-weight loader (conv_wgrad_kernel): dY[m][n], n = tap*N + channel.
// per-thread float offset of column n (volume base + row shift + channel) plus row r of a chunk; fixed for the kernel
ICS_UP8_HD unsigned up8_col_floats(int n, const Up8Geom& u) {
  const int tap = n / u.N, ch = n - tap * u.N;
  return u.tapoff[tap] + (unsigned)ch;
}
// wave-uniform float offset of the 32-row chunk that starts at row mbase (a multiple of 32)
ICS_UP8_HD size_t up8_chunk_base_floats(unsigned mbase, const Up8Geom& u) {
  return (size_t)up8_prow(mbase, u.lgSh, u.P) * (size_t)u.N;
}
