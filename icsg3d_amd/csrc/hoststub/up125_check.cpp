// Host check of the 125-product layout of the up-split backward (../up125.h); no GPU.  Built with
// -fsanitize=address,undefined by `make asan`.
//
//  1. addresses: over max_batch in {1,2,3,5}, every run-time batch up to it and S in {8,16,32}: every (class, tile row,
//     block, channel) offset of the pooled buffer and every (class, tile row, channel) offset of the class volumes lies
//     inside a buffer sized by max_batch, no two of them coincide and together they cover a dense prefix; the classes of
//     a group are whole matrices apart (the z strides of the batched GEMMs); the 27 weight images tile their buffer.
//  2. values (S <= 16): a float port of pool27_kernel's sums (in double) and of pool125_kernel; every block equals the
//     signed combination of tap copies its type stands for (D1 = Q[2j] - Q[2j+1], ...).
//  3. algebra in double: class GEMMs + combine against dxl = sum_tap dyS[tap] W[tap]; x classes + block products +
//     contraction against dW[tap] = xl^T dyS[tap].  The weights are the packed class images as the pack jobs write them
//     (up125_pack_piece), compared element by element with their definition (up125_weight_value).
#include "../up125.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

static int g_fail = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      if (g_fail < 20) {                          \
        fprintf(stderr, "up125_check FAILED: ");  \
        fprintf(stderr, __VA_ARGS__);             \
        fprintf(stderr, "\n");                    \
      }                                           \
      ++g_fail;                                   \
    }                                             \
  } while (0)

static uint32_t g_rng = 12345u;
static float frand() {
  g_rng = g_rng * 1664525u + 1013904223u;
  return (float)((g_rng >> 8) & 0xffff) / 65536.f - 0.5f;
}

static void check_addresses(int maxB, int B, int S, int N, int Cu) {
  CHECK(up125_shape_ok(S, N, Cu, B), "shape (B %d, S %d, N %d, Cu %d) refused", B, S, N, Cu);
  const Up125Geom u = up125_geom(B, S, N, Cu);
  const size_t rows = u.rows, rows_max = up125_geom(maxB, S, N, Cu).rows;
  const size_t allocP = up125_pooled_floats(rows_max, N), allocC = up125_class_floats(rows_max, Cu);
  std::vector<unsigned char> hitP(up125_pooled_floats(rows, N) / 4, 0), hitC(up125_class_floats(rows, Cu) / 4, 0);
  CHECK(up125_pooled_floats(rows, N) <= allocP && up125_class_floats(rows, Cu) <= allocC, "prefix larger than the allocation");
  int blocks = 0;
  for (int tz = 0; tz < 5; ++tz)
    for (int ty = 0; ty < 5; ++ty)
      for (int tx = 0; tx < 5; ++tx) {
        const int q = up125_cls(tz) * 9 + up125_cls(ty) * 3 + up125_cls(tx);
        const int b = up125_block(q, tz, ty, tx);
        CHECK(b >= 0 && b < up125_nb(q), "block %d of class %d", b, q);
        ++blocks;
        for (size_t r = 0; r < rows; ++r)
          for (int n = 0; n < N; n += 4) {
            const size_t off = up125_pooled_off(u, q, r, b, n);
            CHECK(off + 4 <= allocP && off % 4 == 0 && off / 4 < hitP.size(), "pooled offset %zu outside", off);
            if (off / 4 < hitP.size()) { CHECK(!hitP[off / 4], "pooled offset %zu written twice", off); hitP[off / 4] = 1; }
          }
      }
  CHECK(blocks == 125, "block count");
  for (unsigned char h : hitP) if (!h) { CHECK(false, "pooled prefix not dense"); break; }
  for (int q = 0; q < 27; ++q)
    for (size_t r = 0; r < rows; ++r)
      for (int c = 0; c < Cu; c += 4) {
        const size_t off = up125_class_off(u, q, r, c);
        CHECK(off + 4 <= allocC && off / 4 < hitC.size(), "class offset %zu outside", off);
        if (off / 4 < hitC.size()) { CHECK(!hitC[off / 4], "class offset %zu written twice", off); hitC[off / 4] = 1; }
      }
  for (unsigned char h : hitC) if (!h) { CHECK(false, "class prefix not dense"); break; }
  // z strides: class z of group g is a whole matrix [rows][nb N] (pooled), [nb N][Cu] (weights), [rows][Cu] (classes) on
  int seen = 0;
  for (int g = 0; g < 4; ++g)
    for (int z = 0; z < up125_group_classes(g); ++z, ++seen) {
      const int q = up125_class_of_slot(up125_group_slot0(g) + z), nb = 8 >> g;
      CHECK(q >= 0 && up125_nB(q) == g && up125_nb(q) == nb && up125_slot(q) == up125_group_slot0(g) + z, "slot order");
      CHECK(up125_pooled_off(u, q, 0, 0, 0) == ((size_t)up125_group_block0(g) + (size_t)z * nb) * rows * N, "pooled z stride");
      CHECK(up125_class_off(u, q, 0, 0) == ((size_t)up125_group_slot0(g) + z) * rows * Cu, "class z stride");
      CHECK((size_t)up125_bbase(q) * N * Cu == ((size_t)up125_group_block0(g) + (size_t)z * nb) * N * Cu &&
                ((size_t)up125_bbase(q) + nb) * N * Cu <= up125_weight_floats(N, Cu), "weight image");
    }
  CHECK(seen == 27, "27 classes");
}

// dyS[vl][tap][n] of pool27_kernel, in double
static std::vector<double> pool27_host(const std::vector<float>& dy, int B, int S, int N) {
  const int Sh = S / 2;
  std::vector<double> o((size_t)B * Sh * Sh * Sh * 27 * N, 0.0);
  for (int b = 0; b < B; ++b)
    for (int z = 0; z < S; ++z)
      for (int y = 0; y < S; ++y)
        for (int x = 0; x < S; ++x)
          for (int tap = 0; tap < 27; ++tap) {
            const int d[3] = {tap / 9 - 1, (tap / 3) % 3 - 1, tap % 3 - 1};
            const int p[3] = {z + d[0], y + d[1], x + d[2]};
            if (p[0] < 0 || p[0] >= S || p[1] < 0 || p[1] >= S || p[2] < 0 || p[2] >= S) continue;
            const size_t vl = (((size_t)b * Sh + p[0] / 2) * Sh + p[1] / 2) * Sh + p[2] / 2;
            const size_t v = (((size_t)b * S + z) * S + y) * S + x;
            for (int n = 0; n < N; ++n) o[(vl * 27 + tap) * N + n] += dy[v * N + n];
          }
  return o;
}
// the kernel's sums: fine samples 4j-1 .. 4j+4 per axis with up125_coef
static void pool125_host(const std::vector<float>& dy, int B, int S, int N, const Up125Geom& u, float* out) {
  const int T = u.T;
  for (int b = 0; b < B; ++b)
    for (int jz = 0; jz < T; ++jz)
      for (int jy = 0; jy < T; ++jy)
        for (int jx = 0; jx < T; ++jx) {
          const size_t tile = (((size_t)b * T + jz) * T + jy) * T + jx;
          for (int tz = 0; tz < 5; ++tz)
            for (int ty = 0; ty < 5; ++ty)
              for (int tx = 0; tx < 5; ++tx) {
                const int q = up125_cls(tz) * 9 + up125_cls(ty) * 3 + up125_cls(tx);
                for (int n = 0; n < N; ++n) {
                  float acc = 0.f;
                  for (int fz = 0; fz < 6; ++fz)
                    for (int fy = 0; fy < 6; ++fy)
                      for (int fx = 0; fx < 6; ++fx) {
                        const int s = up125_coef(tz, fz) * up125_coef(ty, fy) * up125_coef(tx, fx);
                        const int z = 4 * jz - 1 + fz, y = 4 * jy - 1 + fy, x = 4 * jx - 1 + fx;
                        if (s == 0 || z < 0 || z >= S || y < 0 || y >= S || x < 0 || x >= S) continue;
                        acc += (float)s * dy[((((size_t)b * S + z) * S + y) * S + x) * N + n];
                      }
                  out[up125_pooled_off(u, q, tile, up125_block(q, tz, ty, tx), n)] = acc;
                }
              }
        }
}
// type t of tile j as signed tap copies: (coarse coordinate, tap offset d, sign), two entries at most
struct Term { int a, d, s; };
static int type_terms(int t, int j, Term* o) {
  switch (t) {
    case UP125_D1: o[0] = Term{2 * j, +1, +1}; o[1] = Term{2 * j + 1, +1, -1}; return 2;
    case UP125_R0: o[0] = Term{2 * j, 0, +1}; return 1;
    case UP125_Q1: o[0] = Term{2 * j + 1, +1, +1}; return 1;
    case UP125_D2: o[0] = Term{2 * j + 1, +1, +1}; o[1] = Term{2 * j + 1, -1, -1}; return 2;   // Q[2j+2] is tap -1 at 2j+1
    default: o[0] = Term{2 * j + 1, 0, +1}; return 1;
  }
}

static void check_values(int maxB, int B, int S, int N, int Cu) {
  const int Sh = S / 2, T = S / 4;
  const Up125Geom u = up125_geom(B, S, N, Cu);
  const size_t rows = u.rows;
  std::vector<float> dy((size_t)B * S * S * S * N);
  for (float& v : dy) v = frand();
  const std::vector<double> dyS = pool27_host(dy, B, S, N);
  const size_t alloc = up125_pooled_floats(up125_geom(maxB, S, N, Cu).rows, N);
  float* P = (float*)malloc(alloc * sizeof(float));   // exactly the allocation: ASan sees every overrun
  pool125_host(dy, B, S, N, u, P);
  double worst = 0, scale = 0;
  for (int b = 0; b < B; ++b)
    for (int jz = 0; jz < T; ++jz)
      for (int jy = 0; jy < T; ++jy)
        for (int jx = 0; jx < T; ++jx) {
          const size_t tile = (((size_t)b * T + jz) * T + jy) * T + jx;
          for (int tz = 0; tz < 5; ++tz)
            for (int ty = 0; ty < 5; ++ty)
              for (int tx = 0; tx < 5; ++tx) {
                const int q = up125_cls(tz) * 9 + up125_cls(ty) * 3 + up125_cls(tx);
                Term az[2], ay[2], ax[2];
                const int nz = type_terms(tz, jz, az), ny = type_terms(ty, jy, ay), nx = type_terms(tx, jx, ax);
                for (int n = 0; n < N; ++n) {
                  double ref = 0;
                  for (int i = 0; i < nz; ++i)
                    for (int k = 0; k < ny; ++k)
                      for (int l = 0; l < nx; ++l) {
                        const size_t vl = (((size_t)b * Sh + az[i].a) * Sh + ay[k].a) * Sh + ax[l].a;
                        const int tap = (az[i].d + 1) * 9 + (ay[k].d + 1) * 3 + (ax[l].d + 1);
                        ref += az[i].s * ay[k].s * ax[l].s * dyS[(vl * 27 + tap) * N + n];
                      }
                  const double got = P[up125_pooled_off(u, q, tile, up125_block(q, tz, ty, tx), n)];
                  worst = std::fmax(worst, std::fabs(got - ref));
                  scale = std::fmax(scale, std::fabs(ref));
                }
              }
        }
  CHECK(worst <= 1e-5 * scale, "pooled blocks differ from the tap copies: %g of %g (B %d, S %d)", worst, scale, B, S);

  // ---- the algebra in double, weights through the packed class images
  const int Cin_total = Cu + 32, c_off = 32;
  std::vector<float> w((size_t)27 * Cin_total * N), xl(rows * 8 * Cu);
  for (float& v : w) v = frand();
  for (float& v : xl) v = frand();
  // the images as the pack jobs write them (a heap buffer of exactly the allocated size), against the element-wise definition
  const size_t nW = up125_weight_floats(N, Cu);
  float* W = (float*)aligned_alloc(16, nW * sizeof(float));
  for (size_t i = 0; i < nW; ++i) W[i] = 1e30f;
  for (size_t i = 0; i < up125_pack_pieces(N, Cu); ++i) up125_pack_piece(i, w.data(), Cin_total, N, c_off, Cu, W);
  double wworst = 0;
  for (int q = 0; q < 27; ++q)
    for (size_t i = 0; i < (size_t)up125_nb(q) * N * Cu; ++i)
      wworst = std::fmax(wworst, std::fabs((double)W[(size_t)up125_bbase(q) * N * Cu + i] -
                                           up125_weight_value(i, w.data(), Cin_total, N, c_off, Cu, q)));
  CHECK(wworst <= 1e-6, "packed class images differ from their definition: %g", wworst);
  // backward-data: class outputs, combine
  std::vector<double> O(up125_class_floats(rows, Cu), 0.0);
  for (int q = 0; q < 27; ++q) {
    const int K = up125_nb(q) * N;
    const float* Wq = W + (size_t)up125_bbase(q) * N * Cu;
    for (size_t r = 0; r < rows; ++r)
      for (int k = 0; k < K; ++k) {
        const double p = P[up125_pooled_off(u, q, r, 0, 0) + k];
        for (int c = 0; c < Cu; ++c) O[up125_class_off(u, q, r, c)] += p * Wq[((size_t)(k / 4) * Cu + c) * 4 + k % 4];
      }
  }
  double wdx = 0, sdx = 0;
  for (int b = 0; b < B; ++b)
    for (int z = 0; z < Sh; ++z)
      for (int y = 0; y < Sh; ++y)
        for (int x = 0; x < Sh; ++x) {
          const size_t vl = (((size_t)b * Sh + z) * Sh + y) * Sh + x;
          const size_t tile = (((size_t)b * T + z / 2) * T + y / 2) * T + x / 2;
          for (int c = 0; c < Cu; ++c) {
            double ref = 0, got = 0;
            for (int tap = 0; tap < 27; ++tap)
              for (int n = 0; n < N; ++n) ref += dyS[(vl * 27 + tap) * N + n] * w[((size_t)tap * Cin_total + c_off + c) * N + n];
            for (int k = 0; k < 8; ++k)
              got += O[up125_class_off(u, (z % 2 + (k >> 2)) * 9 + (y % 2 + ((k >> 1) & 1)) * 3 + (x % 2 + (k & 1)), tile, c)];
            wdx = std::fmax(wdx, std::fabs(got - ref));
            sdx = std::fmax(sdx, std::fabs(ref));
          }
        }
  CHECK(wdx <= 1e-5 * sdx, "dxl through the classes differs: %g of %g (B %d, S %d)", wdx, sdx, B, S);
  // backward-weight: x classes, block products, contraction
  std::vector<double> X(up125_class_floats(rows, Cu));
  for (size_t r = 0; r < rows; ++r) {
    const int jx = (int)(r % T), jy = (int)((r / T) % T), jz = (int)((r / ((size_t)T * T)) % T), b = (int)(r / ((size_t)T * T * T));
    for (int q = 0; q < 27; ++q)
      for (int c = 0; c < Cu; ++c) {
        double v = 0;
        for (int k = 0; k < 8; ++k) {
          const int e[3] = {k >> 2, (k >> 1) & 1, k & 1}, cl[3] = {q / 9, (q / 3) % 3, q % 3};
          bool in = true;
          for (int i = 0; i < 3; ++i) in = in && (cl[i] == 1 || cl[i] == 2 * e[i]);   // A: x[2j], B: both, C: x[2j+1]
          if (in) v += xl[((((size_t)b * Sh + 2 * jz + e[0]) * Sh + 2 * jy + e[1]) * Sh + 2 * jx + e[2]) * Cu + c];
        }
        X[up125_class_off(u, q, r, c)] = v;
      }
  }
  double wdw = 0, sdw = 0;
  for (int tap = 0; tap < 27; ++tap)
    for (int c = 0; c < Cu; c += 7)
      for (int n = 0; n < N; n += 5) {
        double ref = 0, got = 0;
        for (size_t vl = 0; vl < rows * 8; ++vl) ref += xl[vl * Cu + c] * dyS[(vl * 27 + tap) * N + n];
        for (int tz = 0; tz < 5; ++tz)
          for (int ty = 0; ty < 5; ++ty)
            for (int tx = 0; tx < 5; ++tx) {
              const int s = up125_wcoef(tz, tap / 9) * up125_wcoef(ty, (tap / 3) % 3) * up125_wcoef(tx, tap % 3);
              if (s == 0) continue;
              const int q = up125_cls(tz) * 9 + up125_cls(ty) * 3 + up125_cls(tx);
              for (size_t r = 0; r < rows; ++r)
                got += s * X[up125_class_off(u, q, r, c)] * P[up125_pooled_off(u, q, r, up125_block(q, tz, ty, tx), n)];
            }
        wdw = std::fmax(wdw, std::fabs(got - ref));
        sdw = std::fmax(sdw, std::fabs(ref));
      }
  CHECK(wdw <= 1e-5 * sdw, "dW through the blocks differs: %g of %g (B %d, S %d)", wdw, sdw, B, S);
  free(P);
  free(W);
}

int main() {
  long cases = 0;
  const int maxBs[4] = {1, 2, 3, 5};
  for (int mb : maxBs)
    for (int B = 1; B <= mb; ++B)
      for (int S = 8; S <= 32; S *= 2) {
        check_addresses(mb, B, S, S == 32 ? 32 : 64, 64);
        ++cases;
      }
  check_values(2, 2, 8, 32, 64);
  check_values(3, 2, 8, 32, 64);
  check_values(1, 1, 16, 32, 64);
  CHECK(!up125_shape_ok(4, 64, 64, 3), "S = 4 accepted");
  CHECK(!up125_shape_ok(16, 96, 64, 1), "N = 96 accepted");
  CHECK(!up125_shape_ok(16, 64, 32, 1), "Cu = 32 accepted");
  CHECK(!up125_shape_ok(64, 512, 512, 64), "a matrix past 2^30 floats accepted");
  if (g_fail) { fprintf(stderr, "up125_check: %d checks FAILED\n", g_fail); return 1; }
  printf("up125_check: %ld (max_batch, batch, S) cases OK\n", cases);
  return 0;
}
