// The arithmetic of the structural fingerprint (structure_fingerprint.hip; include/icsg3d.h states the definition in
// full), stated once: the deposit kernel H, the bin edges, a pair's deposit into a bin, the shell normalisation, the
// image range and the parameter limits.  Plain C++ that compiles for host and device; hoststub/fingerprint_check.cpp
// walks it on the CPU, so the stand-alone check tests the text the kernel compiles.
#pragma once

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ICS_FP_HD __host__ __device__ __forceinline__
#else
#define ICS_FP_HD inline
#endif

namespace ics {

constexpr int kFpMaxBins = 256;     // n_bins
constexpr int kFpMaxImage = 32;     // lattice translations per axis the sweep covers

// The integral of the triangular kernel of half-width 1 from -inf to t: 0 below -1, 1 above 1, C1 at the joins.
ICS_FP_HD double fp_H(double t) {
  if (t <= -1.0) return 0.0;
  if (t >= 1.0) return 1.0;
  if (t <= 0.0) return 0.5 * (1.0 + t) * (1.0 + t);
  return 1.0 - 0.5 * (1.0 - t) * (1.0 - t);
}

// edge k of n_bins bins over [0, r_max]: exactly 0 at k = 0 and exactly r_max at k = n_bins
ICS_FP_HD double fp_edge(int k, double r_max, int n_bins) { return ((double)k * r_max) / (double)n_bins; }

// what a pair at distance d adds to the bin [lo, hi) with half-width w.  Outside the kernel's support (d >= hi + w or
// d <= lo - w, tested first, so the answer there is exactly 0 whatever the quotients below would round to) nothing; a lane
// that owns a far bin skips the two divisions.  The sweep takes only pairs with d < r_max + w.
ICS_FP_HD double fp_deposit(double lo, double hi, double d, double w) {
  if (d >= hi + w || d <= lo - w) return 0.0;
  return fp_H((hi - d) / w) - fp_H((lo - d) / w);
}

// the count an ideal gas of n atoms in the volume vol puts into the shell [lo, hi): n (n / vol) 4 pi / 3 (hi^3 - lo^3)
ICS_FP_HD double fp_shell_norm(int n, double vol, double lo, double hi) {
  const double kFourPiOver3 = 4.1887902047863909846168578443727;
  return (double)n * ((double)n / vol) * kFourPiOver3 * (hi * hi * hi - lo * lo * lo);
}

// the weight of the pair (Z_i, Z_j) in countz
ICS_FP_HD double fp_weight(int zi, int zj, double zbar) { return (double)(zi * zj) / (zbar * zbar); }

// The image range that holds every pair within `reach` of wrapped coordinates: |T_k| <= floor(reach g_k + 1), g the norms
// of the columns of inv(M) (a fractional difference of wrapped atoms lies in (-1, 1) and |(v inv(M))_k| <= |v| g_k).
// False when an axis would exceed kFpMaxImage (t is then not usable).
ICS_FP_HD bool fp_image_range(double reach, const double g[3], int t[3]) {
  bool ok = true;
  for (int k = 0; k < 3; ++k) {
    const double v = floor(reach * g[k] + 1.0);
    ok = ok && v <= (double)kFpMaxImage;
    t[k] = ok ? (int)v : 0;
  }
  return ok;
}

// How far the sweep has to reach: R = r_max + w for the deposits, and (1 + cn_tol) times the shortest lattice vector for
// the neighbours -- an atom's own image along that vector bounds its nearest distance, so every (j, T) within
// (1 + cn_tol) nn_dist lies inside.
ICS_FP_HD double fp_reach(double r_max, double w, double cn_tol, const double* M) {
  double shortest = INFINITY;
  for (int r = 0; r < 3; ++r) {
    const double l = sqrt(M[3 * r] * M[3 * r] + M[3 * r + 1] * M[3 * r + 1] + M[3 * r + 2] * M[3 * r + 2]);
    shortest = l < shortest ? l : shortest;
  }
  const double nb = (1.0 + cn_tol) * shortest, R = r_max + w;
  return nb > R ? nb : R;
}

// The parameter limits of ics_op_structure_fingerprint: nullptr, or what is wrong.
inline const char* fp_check_params(double r_max, int n_bins, double w, double cn_tol) {
  if (!(std::isfinite(r_max) && r_max > 0.0)) return "r_max must be finite and > 0";
  if (!(n_bins >= 1 && n_bins <= kFpMaxBins)) return "n_bins must be in 1..256";
  if (!(std::isfinite(w) && w > 0.0)) return "width must be finite and > 0";
  if (!(std::isfinite(cn_tol) && cn_tol >= 0.0)) return "cn_tol must be finite and >= 0";
  return nullptr;
}

// The counts of ics_op_fingerprint_nearest: nullptr, or what is wrong.
inline const char* fp_check_counts(int len, int nq, int nref) {
  if (len < 1) return "len must be >= 1";
  if (nq < 1) return "nq must be >= 1";
  if (nref < 0) return "nref must be >= 0";
  if ((long long)nq + nref > 0x7ffffffeLL) return "too many rows";
  return nullptr;
}

}  // namespace ics
