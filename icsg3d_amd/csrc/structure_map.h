// The atom-mapping test that structure matching (structure_match.hip) and structure symmetry (structure_symmetry.hip)
// both rest on, stated once; include/icsg3d.h gives the predicate in full.  A transformed copy of a structure maps onto a
// target when (a) every atom has a same-species atom of the target within 2 tol, (b) that nearest-atom map is injective,
// (c) with the common shift taken out every residual is within tol; the score is the rms of those residuals.
//
// Device: atoms are stored sorted by (species, index), thread k of the owning group -- one wave (NW = 1, four groups per
// workgroup) or one 256-thread workgroup (NW = 4) -- owns the k-th sorted atom and scans the run [lo, hi) of its species,
// where the lower slot is the lower atom index; the wrapped coordinates live in LDS and lanes of one species read the
// same address.  Sums are wave butterflies combined in wave order: the same bits run to run.
// Host: the cell quantities, the rules every eligible structure must meet, the atom sort with its run words
// (lo | hi << 16) and anchor run, and the environment cap of the chunk sizes.
#pragma once
#include "scratch.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

namespace ics {

constexpr int kMapMaxAtoms = 256;    // atoms per structure: one thread per atom
constexpr int kMapSmall = 64;        // atoms one wave takes
constexpr int kMapMaxSpecies = 94;

// Sums of a, b, c and the maximum of m over the owning group (wave butterfly, then the wave slots in wave order).
template <int NW>
__device__ __forceinline__ void group_reduce(double& a, double& b, double& c, double& m, double (*red)[NW][4], int& ph,
                                             int wave, int lane) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
    c += __shfl_xor(c, o, 64);
    m = fmax(m, __shfl_xor(m, o, 64));
  }
  if (NW > 1) {
    if (lane == 0) { red[ph][wave][0] = a; red[ph][wave][1] = b; red[ph][wave][2] = c; red[ph][wave][3] = m; }
    __syncthreads();
    a = red[ph][0][0]; b = red[ph][0][1]; c = red[ph][0][2]; m = red[ph][0][3];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      a += red[ph][w][0]; b += red[ph][w][1]; c += red[ph][w][2]; m = fmax(m, red[ph][w][3]);
    }
    ph ^= 1;   // the other buffer next: a slot is rewritten only after a barrier every reader of it has passed
  }
}

// The atom of the species run [rlo, rhi) nearest to (x, y, z) by wrapped-image distance with lattice rows m (ties to the
// lower slot = the lower atom index), its squared distance and Cartesian vector.
__device__ __forceinline__ int nearest_in_run(const double* fx, const double* fy, const double* fz, int rlo, int rhi,
                                              double x, double y, double z, const double* m, double& bd2, double& ux,
                                              double& uy, double& uz) {
  int br = rlo;
  bd2 = __builtin_inf(); ux = uy = uz = 0.0;
  for (int r = rlo; r < rhi; ++r) {
    double da = fx[r] - x, db = fy[r] - y, dc = fz[r] - z;
    da -= rint(da); db -= rint(db); dc -= rint(dc);
    const double vx = da * m[0] + db * m[3] + dc * m[6], vy = da * m[1] + db * m[4] + dc * m[7],
                 vz = da * m[2] + db * m[5] + dc * m[8];
    const double d2 = vx * vx + vy * vy + vz * vz;
    if (d2 < bd2) { bd2 = d2; ux = vx; uy = vy; uz = vz; br = r; }
  }
  return br;
}

// The test of one combination, by every thread of the owning group: `have` says the thread owns an atom, (br, bd2, u) is
// its nearest_in_run result, `tag` a number no other combination of this group uses on `mark` (the group's row of
// injectivity marks, zero at the start: a second arrival on a slot reads the tag back, nothing is reset), dn the atom
// count.  Returns whether the combination passes (a), (b) and (c); then rms is its score and (sx, sy, sz) the mean of u,
// the common shift.  When it fails rms is -1 and the mean is whatever the steps reached.
// Barriers: with NW == 1 group_reduce holds none, so the four waves of a workgroup go their own ways and a wave may leave
// at the first ballot that shows an atom beyond 2 tol.  With NW > 1 the whole workgroup is one group and must call this
// together (the caller's loops are uniform over it); there is no ballot exit, and the two returns between and after the
// reductions test values every thread read from the same LDS slots in the same order, so they are uniform and each
// barrier inside group_reduce is reached by all 256 threads or by none.
template <int NW>
__device__ __forceinline__ bool map_test(bool have, int br, double bd2, double ux, double uy, double uz, double tol, int tag,
                                         int* mark, double dn, double (*red)[NW][4], int& ph, int wave, int lane,
                                         double& rms, double& sx, double& sy, double& sz) {
  rms = -1.0; sx = sy = sz = 0.0;
  const bool far = have && !(sqrt(bd2) <= 2.0 * tol);                            // (a)
  if (NW == 1) {
    if (__ballot(far) != 0ull) return false;
  }
  const bool twice = have && atomicExch(&mark[br], tag) == tag;                  // (b): a second atom on the same nb
  sx = have ? ux : 0.0; sy = have ? uy : 0.0; sz = have ? uz : 0.0;
  double bad = (far || twice) ? 1.0 : 0.0;
  group_reduce<NW>(sx, sy, sz, bad, red, ph, wave, lane);
  if (bad != 0.0) return false;
  sx /= dn; sy /= dn; sz /= dn;
  const double rx = ux - sx, ry = uy - sy, rz = uz - sz;
  double r2 = have ? rx * rx + ry * ry + rz * rz : 0.0, z0 = 0.0, z1 = 0.0, mx = r2;
  group_reduce<NW>(r2, z0, z1, mx, red, ph, wave, lane);
  if (!(sqrt(mx) <= tol)) return false;                                          // (c)
  rms = sqrt(r2 / dn);
  return true;
}

// lattice rows -> volume, the norms of the columns of the inverse and, where inv is given, the inverse itself
inline void cell_inverse(const double* M, double* vol, double g[3], double* inv) {
  const double* va = M; const double* vb = M + 3; const double* vc = M + 6;
  auto cross = [](const double* u, const double* v, double* o) {
    o[0] = u[1] * v[2] - u[2] * v[1]; o[1] = u[2] * v[0] - u[0] * v[2]; o[2] = u[0] * v[1] - u[1] * v[0];
  };
  auto norm = [](const double* u) { return std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]); };
  double bc[3], ca[3], ab[3];
  cross(vb, vc, bc); cross(vc, va, ca); cross(va, vb, ab);
  *vol = va[0] * bc[0] + va[1] * bc[1] + va[2] * bc[2];
  g[0] = norm(bc) / *vol; g[1] = norm(ca) / *vol; g[2] = norm(ab) / *vol;
  if (inv)
    for (int r = 0; r < 3; ++r) { inv[3 * r] = bc[r] / *vol; inv[3 * r + 1] = ca[r] / *vol; inv[3 * r + 2] = ab[r] / *vol; }
}

// G = M M^T as its six entries 00 01 02 11 12 22
inline void cell_gram(const double* M, double g6[6]) {
  for (int i = 0, k = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j) g6[k++] = M[3 * i] * M[3 * j] + M[3 * i + 1] * M[3 * j + 1] + M[3 * i + 2] * M[3 * j + 2];
}

// The rules both ops set for their structure arrays, every structure checked before anything is written: 0, or -1 with
// the error set naming the structure.  `op` opens every message ("ics_op_structure_match: ").
inline int check_structures(const std::string& op, const int32_t* offsets, const int32_t* species, const double* frac,
                            const double* lattice, const int32_t* eligible, int ns, double tol) {
  ICS_CHECK(offsets[0] == 0, op + "offsets[0] must be 0");
  for (int s = 0; s < ns; ++s)
    ICS_CHECK(offsets[s + 1] >= offsets[s], op + "offsets decrease at structure " + std::to_string(s));
  ICS_CHECK((species && frac) || offsets[ns] == 0, op + "null species or frac");
  for (int s = 0; s < ns; ++s) {
    if (!eligible[s]) continue;
    const std::string who = op + "eligible structure " + std::to_string(s);
    const long long n = (long long)offsets[s + 1] - offsets[s];
    ICS_CHECK(n >= 1, who + " has no atoms");
    ICS_CHECK(n <= kMapMaxAtoms, who + " has " + std::to_string(n) + " atoms, above the limit of " +
                                     std::to_string(kMapMaxAtoms));
    const double* M = lattice + 9 * (size_t)s;
    for (int k = 0; k < 9; ++k) ICS_CHECK(std::isfinite(M[k]), who + " has a non-finite lattice entry");
    for (long long k = 3LL * offsets[s]; k < 3LL * offsets[s + 1]; ++k)
      ICS_CHECK(std::isfinite(frac[k]) && std::fabs(frac[k]) <= 1e15,
                who + " has a non-finite or out-of-range (> 1e15) fractional coordinate");
    for (long long k = offsets[s]; k < offsets[s + 1]; ++k)
      ICS_CHECK(species[k] >= 1 && species[k] <= kMapMaxSpecies, who + " has a species outside 1..94");
    double vol, g[3];
    cell_inverse(M, &vol, g, nullptr);
    ICS_CHECK(vol > 0.0 && std::isfinite(vol), who + " has a lattice volume <= 0");
    for (int k = 0; k < 3; ++k)
      ICS_CHECK(2.0 * tol * g[k] < 0.5, who + ": the cell is too thin for tol (2 tol times an inverse-column norm "
                                                  "reaches 0.5: another image could lie within 2 tol)");
  }
  return 0;
}

// One structure's n atoms sorted by (species, index): perm[k] is the atom at sorted slot k, z[k] its species and
// run[k] = lo | hi << 16 the slots [lo, hi) of that species.  [*alo, *ahi) is the anchor run: the species of the smallest
// count, ties to the lower Z (= the earlier run).
inline void sort_atoms(const int32_t* species, int n, int* perm, int* z, int* run, int* alo, int* ahi) {
  for (int k = 0; k < n; ++k) perm[k] = k;
  std::stable_sort(perm, perm + n, [&](int a, int b) { return species[a] < species[b]; });
  for (int k = 0; k < n; ++k) z[k] = species[perm[k]];
  *alo = 0; *ahi = n;
  for (int lo = 0; lo < n;) {
    int hi = lo + 1;
    while (hi < n && z[hi] == z[lo]) ++hi;
    for (int i = lo; i < hi; ++i) run[i] = lo | (hi << 16);
    if (lo == 0 || hi - lo < *ahi - *alo) { *alo = lo; *ahi = hi; }
    lo = hi;
  }
}

// The cap `def` of a chunk size, or the positive value below it that the environment variable `name` holds.
inline long long env_cap(const char* name, long long def) {
  const char* e = std::getenv(name);
  const long long r = e ? std::atoll(e) : 0;
  return r >= 1 && r < def ? r : def;
}

}  // namespace ics
