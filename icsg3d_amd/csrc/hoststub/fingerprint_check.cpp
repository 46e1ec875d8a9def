// fingerprint.h on the CPU: the pieces of H and their joins, the telescoping sum of a pair's deposits over the bins, the
// shell normalisation, the image range against an exhaustive search over a wider range for skewed cells, and the
// argument checks -- the text the kernels of structure_fingerprint.hip compile.
#include "../fingerprint.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

using namespace ics;

static int fail(const char* what, double a = 0.0, double b = 0.0) {
  std::fprintf(stderr, "fingerprint_check: %s (%.17g, %.17g)\n", what, a, b);
  return 1;
}

// the norms of the columns of inv(M) and the volume, M rows va, vb, vc
static double inverse_column_norms(const double* M, double g[3]) {
  const double* a = M; const double* b = M + 3; const double* c = M + 6;
  const double bc[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
  const double ca[3] = {c[1] * a[2] - c[2] * a[1], c[2] * a[0] - c[0] * a[2], c[0] * a[1] - c[1] * a[0]};
  const double ab[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  const double vol = a[0] * bc[0] + a[1] * bc[1] + a[2] * bc[2];
  g[0] = std::sqrt(bc[0] * bc[0] + bc[1] * bc[1] + bc[2] * bc[2]) / vol;
  g[1] = std::sqrt(ca[0] * ca[0] + ca[1] * ca[1] + ca[2] * ca[2]) / vol;
  g[2] = std::sqrt(ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2]) / vol;
  return vol;
}

int main() {
  const double kInf = std::numeric_limits<double>::infinity(), kNaN = std::numeric_limits<double>::quiet_NaN();
  // ---- H: the four pieces, the joins, symmetry, monotone
  if (fp_H(-1.0) != 0.0 || fp_H(-7.0) != 0.0 || fp_H(-kInf) != 0.0) return fail("H below -1");
  if (fp_H(1.0) != 1.0 || fp_H(7.0) != 1.0 || fp_H(kInf) != 1.0) return fail("H above 1");
  if (fp_H(0.0) != 0.5) return fail("H(0)", fp_H(0.0));
  if (fp_H(-0.5) != 0.125 || fp_H(0.5) != 0.875) return fail("H(+-1/2)", fp_H(-0.5), fp_H(0.5));
  for (double join : {-1.0, 0.0, 1.0}) {
    const double lo = fp_H(std::nextafter(join, -kInf)), hi = fp_H(std::nextafter(join, kInf));
    if (!(lo <= fp_H(join) && fp_H(join) <= hi) || hi - lo > 1e-15) return fail("H jumps at a join", join, hi - lo);
  }
  double prev = 0.0;
  for (int k = -1200; k <= 1200; ++k) {
    const double t = k / 1000.0, h = fp_H(t);
    if (h < prev || h < 0.0 || h > 1.0) return fail("H is not monotone in [0, 1]", t, h);
    if (std::fabs(h + fp_H(-t) - 1.0) > 1e-15) return fail("H(t) + H(-t) != 1", t, h);
    // the derivative is the triangle 1 - |t|
    const double e = 1e-6, slope = (fp_H(t + e) - fp_H(t - e)) / (2 * e), tri = std::fabs(t) < 1.0 ? 1.0 - std::fabs(t) : 0.0;
    if (std::fabs(slope - tri) > 2e-6) return fail("H' is not the triangular kernel", t, slope);
    prev = h;
  }
  // ---- edges and deposits: exact ends, the telescoping sum, exactly 0 outside the support
  for (int nb : {1, 2, 59, 60, 61, 256}) {
    for (double r_max : {6.0, 5.3, 0.7}) {
      if (fp_edge(0, r_max, nb) != 0.0 || fp_edge(nb, r_max, nb) != r_max) return fail("edge ends", nb, r_max);
      for (int k = 0; k < nb; ++k)
        if (!(fp_edge(k, r_max, nb) < fp_edge(k + 1, r_max, nb))) return fail("edges do not ascend", nb, k);
      for (double w : {0.1, 0.013, 0.37, 2.5}) {
        for (int s = 0; s <= 400; ++s) {
          const double d = (r_max + 2 * w) * s / 400.0;
          double sum = 0.0;
          for (int k = 0; k < nb; ++k) {
            const double lo = fp_edge(k, r_max, nb), hi = fp_edge(k + 1, r_max, nb), dep = fp_deposit(lo, hi, d, w);
            if (dep < 0.0 || dep > 1.0) return fail("a deposit outside [0, 1]", d, dep);
            if ((d >= hi + w || d <= lo - w) && dep != 0.0) return fail("a deposit outside the support is not exactly 0", d, dep);
            sum += dep;
          }
          const double want = fp_H((r_max - d) / w) - fp_H(-d / w);
          if (std::fabs(sum - want) > 1e-13) return fail("the deposits do not sum to H((r_max - d) / w) - H(-d / w)", sum, want);
          if (d >= r_max + w && sum != 0.0) return fail("a pair at d >= R deposits", d, sum);
        }
      }
    }
  }
  if (fp_deposit(fp_edge(59, 6.0, 60), fp_edge(60, 6.0, 60), 6.0, 0.1) != 0.5) return fail("the peak on r_max is not halved");
  // ---- the shell normalisation: the shells of [0, r_max] add up to the ball
  {
    double sum = 0.0;
    for (int k = 0; k < 60; ++k) sum += fp_shell_norm(5, 100.0, fp_edge(k, 6.0, 60), fp_edge(k + 1, 6.0, 60));
    const double ball = 5.0 * (5.0 / 100.0) * 4.0 * std::acos(-1.0) / 3.0 * 216.0;
    if (std::fabs(sum - ball) > 1e-12 * ball) return fail("the shells do not add up to the ball", sum, ball);
    if (fp_weight(8, 22, 15.0) != 176.0 / 225.0) return fail("weight");
  }
  // ---- the image range against an exhaustive search two images wider, skewed cells
  std::mt19937_64 rng(5);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  int cells = 0;
  while (cells < 200) {
    double M[9], g[3];
    for (int k = 0; k < 9; ++k) M[k] = (k % 4 == 0 ? 2.0 + 5.0 * U(rng) : 4.0 * (U(rng) - 0.5));
    const double vol = inverse_column_norms(M, g);
    if (!(vol > 5.0)) continue;
    const double w = 0.1, r_max = 1.0 + 5.0 * U(rng), cn_tol = 0.5 * U(rng), reach = fp_reach(r_max, w, cn_tol, M);
    double shortest = kInf;
    for (int r = 0; r < 3; ++r) shortest = std::fmin(shortest, std::sqrt(M[3 * r] * M[3 * r] + M[3 * r + 1] * M[3 * r + 1] + M[3 * r + 2] * M[3 * r + 2]));
    if (reach < r_max + w || reach < (1.0 + cn_tol) * shortest) return fail("reach too short", reach, shortest);
    int T[3];
    if (!fp_image_range(reach, g, T)) continue;
    ++cells;
    for (int pair = 0; pair < 6; ++pair) {
      const double e[3] = {U(rng) - U(rng), U(rng) - U(rng), U(rng) - U(rng)};     // a difference of wrapped coordinates
      for (int a = -T[0] - 2; a <= T[0] + 2; ++a)
        for (int b = -T[1] - 2; b <= T[1] + 2; ++b)
          for (int c = -T[2] - 2; c <= T[2] + 2; ++c) {
            const double x = e[0] + a, y = e[1] + b, z = e[2] + c;
            const double vx = x * M[0] + y * M[3] + z * M[6], vy = x * M[1] + y * M[4] + z * M[7], vz = x * M[2] + y * M[5] + z * M[8];
            const bool inside = std::abs(a) <= T[0] && std::abs(b) <= T[1] && std::abs(c) <= T[2];
            if (!inside && std::sqrt(vx * vx + vy * vy + vz * vz) <= reach) return fail("an image within reach lies outside the range", reach, vol);
          }
    }
  }
  {
    const double thin[3] = {1.0 / 0.18, 1.0 / 0.18, 1.0 / 0.18}, wide[3] = {1.0 / 3.0, 1.0 / 3.0, 0.05};
    int T[3];
    if (fp_image_range(6.1, thin, T)) return fail("34 images per axis accepted");
    if (!fp_image_range(6.1, wide, T) || T[0] != 3 || T[1] != 3 || T[2] != 1) return fail("range of the 3 x 3 x 20 cell", T[0], T[2]);
    const double g32[3] = {31.9 / 6.1, 0.1, 0.1};
    if (!fp_image_range(6.1, g32, T) || T[0] != 32) return fail("32 images per axis refused", T[0]);
  }
  // ---- the argument checks
  if (fp_check_params(6.0, 60, 0.1, 0.1) || fp_check_params(0.5, 1, 3.0, 0.0) || fp_check_params(6.0, 256, 0.1, 0.1)) return fail("good parameters refused");
  if (!fp_check_params(0.0, 60, 0.1, 0.1) || !fp_check_params(-1.0, 60, 0.1, 0.1) || !fp_check_params(kNaN, 60, 0.1, 0.1) ||
      !fp_check_params(kInf, 60, 0.1, 0.1) || !fp_check_params(6.0, 0, 0.1, 0.1) || !fp_check_params(6.0, 257, 0.1, 0.1) ||
      !fp_check_params(6.0, 60, 0.0, 0.1) || !fp_check_params(6.0, 60, kNaN, 0.1) || !fp_check_params(6.0, 60, 0.1, -0.1) ||
      !fp_check_params(6.0, 60, 0.1, kNaN) || !fp_check_params(6.0, 60, 0.1, kInf))
    return fail("a bad parameter accepted");
  if (fp_check_counts(1, 1, 0) || fp_check_counts(120, 5000, 20000)) return fail("good counts refused");
  if (!fp_check_counts(0, 1, 0) || !fp_check_counts(1, 0, 5) || !fp_check_counts(1, 1, -1) || !fp_check_counts(1, 2000000000, 2000000000))
    return fail("bad counts accepted");
  std::puts("fingerprint_check: ok");
  return 0;
}
