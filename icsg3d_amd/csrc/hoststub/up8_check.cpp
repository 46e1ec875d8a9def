// Host check of the 8-volume layout of the up-split backward (../up8.h); no GPU.  Built with
// -fsanitize=address,undefined by `make asan`.
//
//  1. addresses: over max_batch in {1,2,3,5}, every run-time batch up to it, S in {8,16,32,64}, every coarse row m,
//     every tap and every 32-row chunk, the float offset each GEMM loader forms (backward-data: chunk pointer + row
//     offset; backward-weight: chunk base + per-thread row/column offset) lies inside its volume of a buffer sized
//     by max_batch, fits the 32-bit byte offsets the loaders keep, and equals the padded position derived digit by
//     digit from pool27's slot definition (d = 0 -> R[a], d = +1 -> Q[a], d = -1 -> Q[a+1] per axis).
//  2. values (S <= 16): a float32 port of pool27_kernel and of pool8_kernel on random dy; every (m, tap, channel)
//     read through the loader formulas from a heap buffer of exactly the allocated size equals the tap copy bit for
//     bit, and the slots the layout leaves unused keep their fill pattern.
#include "../up8.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int g_fail = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      if (g_fail < 20) {                         \
        fprintf(stderr, "up8_check FAILED: ");   \
        fprintf(stderr, __VA_ARGS__);            \
        fprintf(stderr, "\n");                   \
      }                                          \
      ++g_fail;                                  \
    }                                            \
  } while (0)

static int ilog2i(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

// padded position of (coarse row m, tap), independent of up8_tap / up8_prow: digits first, then the combination
struct Pos { int vol; size_t row; };
static Pos expected_pos(int m, int tap, int Sh, int P) {
  const int x = m % Sh, y = (m / Sh) % Sh, z = (m / (Sh * Sh)) % Sh, b = m / (Sh * Sh * Sh);
  const int d[3] = {tap / 9 - 1, (tap / 3) % 3 - 1, tap % 3 - 1};   // dz, dy, dx
  const int a[3] = {z, y, x};
  int slot[3], typ[3];
  for (int i = 0; i < 3; ++i) {
    typ[i] = d[i] == 0 ? 0 : 1;                    // 0 = R, 1 = Q
    slot[i] = d[i] < 0 ? a[i] + 1 : a[i];          // d = -1 reads Q one coarse voxel further on
  }
  return Pos{typ[0] * 4 + typ[1] * 2 + typ[2], (((size_t)b * P + slot[0]) * P + slot[1]) * P + slot[2]};
}

static void check_addresses(int maxB, int B, int S, int N) {
  const int Sh = S / 2, lg = ilog2i(Sh), P = Sh + 1;
  const int M8 = B * Sh * Sh * Sh;
  CHECK(up8_shape_ok(S, N, (size_t)M8, B), "shape (B %d, S %d, N %d) refused", B, S, N);
  const Up8Geom u = up8_geom(B, Sh, lg, N);
  const size_t alloc = 8 * up8_volume_floats(maxB, Sh, N);   // what the engine allocates
  const size_t vs = u.vstride;
  CHECK(vs == up8_volume_floats(B, Sh, N) && 8 * vs <= alloc, "volume stride");
  CHECK(8 * vs * 4 <= 0xffffffffull, "byte offsets exceed 32 bits");
  const int cpt = N / 32;
  // backward-data: chunk c = tap * cpt + cc, row m (rows past M8 re-read row M8 - 1), 32 channels
  for (int m = 0; m < M8; ++m) {
    const uint64_t rowb = ((uint64_t)up8_row_floats((unsigned)m, u) + 28) * 4;   // + the last float4 column of a chunk
    CHECK(rowb <= 0xffffffffull, "row byte offset exceeds 32 bits");
    for (int tap = 0; tap < 27; ++tap) {
      const Pos e = expected_pos(m, tap, Sh, P);
      for (int cc = 0; cc < cpt; ++cc) {
        const size_t off = up8_chunk_floats(tap * cpt + cc, u) + up8_row_floats((unsigned)m, u);
        const size_t want = (size_t)e.vol * vs + e.row * N + (size_t)cc * 32;
        CHECK(off == want, "dgrad B %d S %d N %d m %d tap %d cc %d: %zu != %zu", B, S, N, m, tap, cc, off, want);
        CHECK(off >= (size_t)e.vol * vs && off + 32 <= (size_t)(e.vol + 1) * vs && off + 32 <= alloc,
              "dgrad B %d S %d N %d m %d tap %d: outside its volume", B, S, N, m, tap);
      }
    }
  }
  // backward-weight: 32-row chunk at mbase, thread row r, float4 column n
  CHECK(M8 % 32 == 0, "whole chunks");
  for (int mbase = 0; mbase < M8; mbase += 32) {
    const size_t cb = up8_chunk_base_floats((unsigned)mbase, u);
    for (int r = 0; r < 32; ++r) {
      const unsigned pr = up8_prow((unsigned)r, lg, P) * (unsigned)N;
      for (int n = 0; n < 27 * N; n += 4) {
        const uint64_t tb = ((uint64_t)pr + up8_col_floats(n, u)) * 4;   // the per-thread byte offset (doffg)
        CHECK(tb <= 0xffffffffull, "per-thread byte offset exceeds 32 bits");
        const size_t off = cb + pr + up8_col_floats(n, u);
        const int tap = n / N;
        const Pos e = expected_pos(mbase + r, tap, Sh, P);
        const size_t want = (size_t)e.vol * vs + e.row * N + (size_t)(n % N);
        CHECK(off == want, "wgrad B %d S %d N %d m %d n %d: %zu != %zu", B, S, N, mbase + r, n, off, want);
        CHECK(off >= (size_t)e.vol * vs && off + 4 <= (size_t)(e.vol + 1) * vs && off + 4 <= alloc,
              "wgrad B %d S %d N %d m %d n %d: outside its volume", B, S, N, mbase + r, n);
      }
    }
  }
}

// ---- float32 ports of the two pooling kernels (same slots, same order of additions)
static void pool27_host(const std::vector<float>& dy, int B, int S, int N, std::vector<float>& out) {
  const int Sh = S / 2;
  out.assign((size_t)B * Sh * Sh * Sh * 27 * N, 0.f);
  for (int b = 0; b < B; ++b) for (int a = 0; a < Sh; ++a) for (int bq = 0; bq < Sh; ++bq) for (int c = 0; c < Sh; ++c)
  for (int n = 0; n < N; ++n) {
    float o[27];
    for (int k = 0; k < 27; ++k) o[k] = 0.f;
    for (int sz = 0; sz < 4; ++sz) {
      const int z = 2 * a - 1 + sz;
      if (z < 0 || z >= S) continue;
      float lx[4][3];
      for (int sy = 0; sy < 4; ++sy) {
        const int y = 2 * bq - 1 + sy;
        float v[4];
        for (int sx = 0; sx < 4; ++sx) {
          const int x = 2 * c - 1 + sx;
          const bool ok = y >= 0 && y < S && x >= 0 && x < S;
          v[sx] = ok ? dy[((((size_t)b * S + z) * S + y) * S + x) * N + n] : 0.f;
        }
        lx[sy][2] = v[0] + v[1]; lx[sy][1] = v[1] + v[2]; lx[sy][0] = v[2] + v[3];
      }
      float Pq[3][3];
      for (int dx = 0; dx < 3; ++dx) {
        Pq[2][dx] = lx[0][dx] + lx[1][dx]; Pq[1][dx] = lx[1][dx] + lx[2][dx]; Pq[0][dx] = lx[2][dx] + lx[3][dx];
      }
      for (int dyi = 0; dyi < 3; ++dyi) for (int dx = 0; dx < 3; ++dx) {
        if (sz <= 1) o[2 * 9 + dyi * 3 + dx] += Pq[dyi][dx];
        if (sz >= 1 && sz <= 2) o[1 * 9 + dyi * 3 + dx] += Pq[dyi][dx];
        if (sz >= 2) o[0 * 9 + dyi * 3 + dx] += Pq[dyi][dx];
      }
    }
    const size_t vl = (((size_t)b * Sh + a) * Sh + bq) * Sh + c;
    for (int k = 0; k < 27; ++k) out[(vl * 27 + k) * N + n] = o[k];
  }
}
static void pool8_host(const std::vector<float>& dy, int B, int S, int N, const Up8Geom& u, float* out) {
  const int Sh = S / 2, P = u.P;
  for (int b = 0; b < B; ++b) for (int jz = 0; jz < P; ++jz) for (int jy = 0; jy < P; ++jy) for (int jx = 0; jx < P; ++jx)
  for (int n = 0; n < N; ++n) {
    float o[2][2][2] = {};
    for (int sz = 0; sz < 3; ++sz) {
      const int z = 2 * jz - 1 + sz;
      if (z < 0 || z >= S) continue;
      float lx[3][2];
      for (int sy = 0; sy < 3; ++sy) {
        const int y = 2 * jy - 1 + sy;
        float v[3];
        for (int sx = 0; sx < 3; ++sx) {
          const int x = 2 * jx - 1 + sx;
          const bool ok = y >= 0 && y < S && x >= 0 && x < S;
          v[sx] = ok ? dy[((((size_t)b * S + z) * S + y) * S + x) * N + n] : 0.f;
        }
        lx[sy][1] = v[0] + v[1]; lx[sy][0] = v[1] + v[2];
      }
      for (int kx = 0; kx < 2; ++kx) {
        const float q = lx[0][kx] + lx[1][kx], rr = lx[1][kx] + lx[2][kx];
        if (sz <= 1) { o[1][1][kx] += q; o[1][0][kx] += rr; }
        if (sz >= 1) { o[0][1][kx] += q; o[0][0][kx] += rr; }
      }
    }
    const size_t row = (((size_t)b * P + jz) * P + jy) * P + jx;
    for (int k = 0; k < 8; ++k) {
      const int kz = k >> 2, ky = (k >> 1) & 1, kx = k & 1;
      if ((kz == 0 && jz == Sh) || (ky == 0 && jy == Sh) || (kx == 0 && jx == Sh)) continue;
      out[(size_t)k * u.vstride + row * N + n] = o[kz][ky][kx];
    }
  }
}

static void check_values(int maxB, int B, int S, int N) {
  const int Sh = S / 2, lg = ilog2i(Sh), P = Sh + 1, M8 = B * Sh * Sh * Sh;
  const Up8Geom u = up8_geom(B, Sh, lg, N);
  std::vector<float> dy((size_t)B * S * S * S * N);
  uint32_t st = 12345u + (uint32_t)(B * 131 + S * 7 + N);
  for (auto& v : dy) {
    st = st * 1664525u + 1013904223u;
    v = ((int)(st >> 8) % 20001 - 10000) * 1.37e-4f;
    if ((st >> 28) == 0) v = -0.f;               // signed zeros must survive the same way in both forms
  }
  std::vector<float> ref;
  pool27_host(dy, B, S, N, ref);
  const size_t alloc = 8 * up8_volume_floats(maxB, Sh, N);
  float* vol = (float*)malloc(alloc * sizeof(float));   // exactly the allocation: a read past it is an ASan report
  const uint32_t fill = 0x7fc0dead;
  for (size_t i = 0; i < alloc; ++i) memcpy(vol + i, &fill, 4);
  pool8_host(dy, B, S, N, u, vol);
  const int cpt = N / 32;
  for (int m = 0; m < M8; ++m)
    for (int tap = 0; tap < 27; ++tap)
      for (int ch = 0; ch < N; ++ch) {
        const size_t off = up8_chunk_floats(tap * cpt + ch / 32, u) + up8_row_floats((unsigned)m, u) + ch % 32;
        const size_t offw = up8_chunk_base_floats((unsigned)(m & ~31), u) + up8_prow((unsigned)(m & 31), lg, P) * (size_t)N +
                            up8_col_floats(tap * N + ch, u);
        CHECK(off == offw, "value check: the two loaders disagree at m %d tap %d ch %d", m, tap, ch);
        const float a = vol[off], b = ref[((size_t)m * 27 + tap) * N + ch];
        CHECK(memcmp(&a, &b, 4) == 0, "value B %d S %d m %d tap %d ch %d: %.9g != %.9g", B, S, m, tap, ch, a, b);
      }
  // the unused slots (slot Sh of an R-type axis, and everything behind batch B) were not written
  size_t untouched = 0, expect_untouched = alloc - 8 * (size_t)u.vstride;
  for (int k = 0; k < 8; ++k) {
    const int q = (k >> 2) + ((k >> 1) & 1) + (k & 1);             // Q-type axes
    size_t used = (size_t)B * N;
    for (int i = 0; i < 3; ++i) used *= (size_t)(i < q ? P : Sh);
    expect_untouched += (size_t)u.vstride - used;
  }
  for (size_t i = 0; i < alloc; ++i) untouched += memcmp(vol + i, &fill, 4) == 0;
  CHECK(untouched == expect_untouched, "B %d S %d: %zu untouched floats, expected %zu", B, S, untouched, expect_untouched);
  free(vol);
}

int main() {
  const int Bs[4] = {1, 2, 3, 5}, Ss[4] = {8, 16, 32, 64};
  long cases = 0;
  for (int bi = 0; bi < 4; ++bi)
    for (int si = 0; si < 4; ++si)
      for (int B = 1; B <= Bs[bi]; ++B) {
        if (B != Bs[bi] && B != Bs[bi] - 1 && B != 1) continue;   // the maximum, one below it, and 1
        check_addresses(Bs[bi], B, Ss[si], Ss[si] >= 32 ? 32 : 64);
        if (Ss[si] <= 16) { check_addresses(Bs[bi], B, Ss[si], 32); check_values(Bs[bi], B, Ss[si], 32); }
        if (Ss[si] == 8) check_values(Bs[bi], B, Ss[si], 64);
        ++cases;
      }
  // shapes the layout must refuse
  CHECK(!up8_shape_ok(4, 64, 3 * 8, 3), "S = 4 accepted");
  CHECK(!up8_shape_ok(8, 16, 2 * 64, 2), "N = 16 accepted");
  CHECK(!up8_shape_ok(16, 96, 512, 1), "N = 96 accepted");
  CHECK(!up8_shape_ok(64, 512, (size_t)64 * 32768, 64), "a buffer past 4 GiB accepted");
  if (g_fail) { fprintf(stderr, "up8_check: %d checks FAILED\n", g_fail); return 1; }
  printf("up8_check: %ld (max_batch, batch, S) cases OK\n", cases);
  return 0;
}
