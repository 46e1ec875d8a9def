// Host check of the plane-by-plane pooling of the up-split backward (../up125.h: up125_pool_lane, up125_xline,
// up125_yacc, up125_xch_off, up125_zcomb, the functions pool125_planes_kernel runs); no GPU.  Built with
// -fsanitize=address,undefined by `make asan`.
//
// The workgroup is played through as the kernel walks it: grid (tile groups, channel groups) of six waves of 64 lanes,
// a lane = (tile row, four channels, one at a time here), stage 1 per wave = fine plane, the five exchange rounds through
// two buffers of UP125_XCH_ELEMS elements (heap blocks of exactly that size), stage 2 by the waves 0..4.  A round's
// buffer is poisoned before it is written, so a read of an element no wave of the round wrote shows.  dy holds integers
// in [-8, 8]: every sum is exact, and each of the 125 * rows * N outputs must EQUAL the definition
//   sum over (fz, fy, fx) of coef(tz, fz) coef(ty, fy) coef(tx, fx) dy[4j - 1 + f]      (outside the volume: 0).
#include "../up125.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

static int g_fail = 0;
#define CHECK(cond, ...)                            \
  do {                                              \
    if (!(cond)) {                                  \
      if (g_fail < 20) {                            \
        fprintf(stderr, "pool125_check FAILED: ");  \
        fprintf(stderr, __VA_ARGS__);               \
        fprintf(stderr, "\n");                      \
      }                                             \
      ++g_fail;                                     \
    }                                               \
  } while (0)

static uint32_t g_rng = 2463534242u;
static float irand() {   // integer in [-8, 8]
  g_rng = g_rng * 1664525u + 1013904223u;
  return (float)((int)((g_rng >> 8) % 17u) - 8);
}

// one workgroup of pool125_planes_kernel for channel k (0..3) of every lane's quad
static void workgroup(const float* dy, int S, int lgc, unsigned bx, unsigned by, int k, float* out, const Up125Geom& u,
                      std::vector<unsigned char>& written) {
  const int T = u.T, lg = u.lgT, N = u.N;
  float* xch[2] = {(float*)malloc(UP125_XCH_ELEMS * sizeof(float)), (float*)malloc(UP125_XCH_ELEMS * sizeof(float))};
  std::vector<float> Sa((size_t)UP125_POOL_WAVES * 64 * 25, 0.f);   // the registers of every lane of every wave
  // stage 1
  for (int fz = 0; fz < UP125_POOL_WAVES; ++fz)
    for (int lane = 0; lane < 64; ++lane) {
      unsigned tile;
      int n;
      up125_pool_lane(lgc, bx, by, lane, &tile, &n);
      const bool live = tile < u.rows;
      const int jx = tile & (T - 1), jy = (tile >> lg) & (T - 1), jz = (tile >> (2 * lg)) & (T - 1), b = tile >> (3 * lg);
      const int z = 4 * jz - 1 + fz;
      const bool zok = live && (unsigned)z < (unsigned)S;
      float* Sl = &Sa[((size_t)fz * 64 + lane) * 25];
      for (int fy = 0; fy < 6; ++fy) {
        const int y = 4 * jy - 1 + fy;
        const bool yok = zok && (unsigned)y < (unsigned)S;
        float v[6], xr[5];
        for (int fx = 0; fx < 6; ++fx) {
          const int x = 4 * jx - 1 + fx;
          const bool ok = yok && (unsigned)x < (unsigned)S;
          v[fx] = ok ? dy[((((size_t)b * S + z) * S + y) * S + x) * (size_t)N + n + k] : 0.f;
        }
        up125_xline(v, xr);
        up125_yacc(fy, xr, Sl);
      }
    }
  // stage 2
  for (int ty = 0; ty < UP125_POOL_ROUNDS; ++ty) {
    float* buf = xch[ty & 1];
    for (int i = 0; i < UP125_XCH_ELEMS; ++i) buf[i] = NAN;
    for (int fz = 0; fz < UP125_POOL_WAVES; ++fz)
      for (int lane = 0; lane < 64; ++lane)
        for (int tx = 0; tx < 5; ++tx) buf[up125_xch_off(fz, tx, lane)] = Sa[((size_t)fz * 64 + lane) * 25 + ty * 5 + tx];
    // barrier
    for (int tz = 0; tz < 5; ++tz)   // wave tz; wave 5 owns no type
      for (int lane = 0; lane < 64; ++lane) {
        unsigned tile;
        int n;
        up125_pool_lane(lgc, bx, by, lane, &tile, &n);
        if (tile >= u.rows) continue;
        for (int tx = 0; tx < 5; ++tx) {
          float s[6];
          for (int fz = 0; fz < 6; ++fz) s[fz] = up125_coef(tz, fz) != 0 ? buf[up125_xch_off(fz, tx, lane)] : 0.f;
          const int q = up125_cls(tz) * 9 + up125_cls(ty) * 3 + up125_cls(tx);
          const size_t off = up125_pooled_off(u, q, tile, up125_block(q, tz, ty, tx), n + k);
          CHECK(off < written.size() && !written[off], "offset %zu outside the buffer or written twice", off);
          if (off < written.size()) { out[off] = up125_zcomb(tz, s); written[off] = 1; }
        }
      }
  }
  free(xch[0]); free(xch[1]);
}

static void check(int B, int S, int N) {
  CHECK(up125_shape_ok(S, N, 64, B), "shape (B %d, S %d, N %d) refused", B, S, N);
  const Up125Geom u = up125_geom(B, S, N, 64);
  const int T = u.T;
  std::vector<float> dy((size_t)B * S * S * S * N);
  for (float& v : dy) v = irand();
  const size_t total = up125_pooled_floats(u.rows, N);
  float* P = (float*)malloc(total * sizeof(float));   // exactly the buffer: ASan sees every overrun
  std::vector<unsigned char> written(total, 0);
  // the launch: launch_pool125's grid
  int lgc = 0;
  while ((1 << lgc) < (N / 4 < 64 ? N / 4 : 64)) ++lgc;
  const unsigned tpw = 64u >> lgc, gx = (u.rows + tpw - 1) / tpw, gy = (unsigned)((N / 4) >> lgc);
  for (unsigned by = 0; by < gy; ++by)
    for (unsigned bx = 0; bx < gx; ++bx)
      for (int k = 0; k < 4; ++k) workgroup(dy.data(), S, lgc, bx, by, k, P, u, written);
  size_t missing = 0;
  for (unsigned char w : written) missing += !w;
  CHECK(missing == 0, "%zu of %zu outputs never written (B %d, S %d, N %d)", missing, total, B, S, N);
  // the definition
  size_t wrong = 0;
  for (size_t tile = 0; tile < u.rows; ++tile) {
    const int jx = (int)(tile % T), jy = (int)((tile / T) % T), jz = (int)((tile / ((size_t)T * T)) % T), b = (int)(tile / ((size_t)T * T * T));
    for (int tz = 0; tz < 5; ++tz)
      for (int ty = 0; ty < 5; ++ty)
        for (int tx = 0; tx < 5; ++tx) {
          const int q = up125_cls(tz) * 9 + up125_cls(ty) * 3 + up125_cls(tx);
          for (int n = 0; n < N; ++n) {
            int ref = 0;
            for (int fz = 0; fz < 6; ++fz)
              for (int fy = 0; fy < 6; ++fy)
                for (int fx = 0; fx < 6; ++fx) {
                  const int s = up125_coef(tz, fz) * up125_coef(ty, fy) * up125_coef(tx, fx);
                  const int z = 4 * jz - 1 + fz, y = 4 * jy - 1 + fy, x = 4 * jx - 1 + fx;
                  if (s == 0 || z < 0 || z >= S || y < 0 || y >= S || x < 0 || x >= S) continue;
                  ref += s * (int)dy[((((size_t)b * S + z) * S + y) * S + x) * N + n];
                }
            const float got = P[up125_pooled_off(u, q, tile, up125_block(q, tz, ty, tx), n)];
            if (!(got == (float)ref)) {
              if (wrong < 5) fprintf(stderr, "  tile %zu type (%d, %d, %d) channel %d: %g, definition %d\n", tile, tz, ty, tx, n, got, ref);
              ++wrong;
            }
          }
        }
  }
  CHECK(wrong == 0, "%zu of %zu outputs differ from the definition (B %d, S %d, N %d)", wrong, total, B, S, N);
  free(P);
}

int main() {
  check(1, 8, 32);    // 8 tiles per wave, every tile on a border of every axis
  check(2, 8, 64);    // sample boundary inside a wave
  check(1, 16, 32);   // interior tiles
  if (g_fail) { fprintf(stderr, "pool125_check: %d check(s) failed\n", g_fail); return 1; }
  printf("pool125_check: plane-by-plane pooling equals the definition on 3 shapes\n");
  return 0;
}
