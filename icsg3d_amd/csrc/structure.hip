// generate.py's structure stage (reference generate.py:250-263, utils.py:225-239) on the device: per generated sample,
// the periodic structure to_pymatgen_structure builds and the validity screen structure.is_valid() applies to it.
//
// The cell (Lattice.from_parameters, one per structure) is computed on the host, where the refusals need it before any
// device work.  Everything per atom and per pair runs in the kernel, in fp64:
//   frac = xyz / abc (placement in the 90-degree lattice; kept when the lattice is swapped for the alpha/beta/gamma one),
//   the shortest periodic distance of every pair i < j -- the TRUE minimum over lattice translations: per pair the image
//   range per axis follows from the zero-image distance D0 and the norms g of the columns of inv(M), since an image at
//   distance <= D0 has |df_i + n_i| <= D0 g_i -- the minimum pair as a (distance, i, j) key, the pairs at or under tol,
//   each atom's nearest other atom, and the species histogram.
// A structure is owned by G threads: one wave (four structures per 256-thread workgroup) up to 64 atoms, a whole
// 1024-thread workgroup above.  Wrapped fractional coordinates live in LDS; threads own pairs.  The key is reduced
// through wave shuffles, then one LDS slot per wave combined in wave order; the per-atom minimum is an integer LDS
// atomic min on the bit pattern of the (non-negative) distance and the histogram an integer LDS atomic add, so no result
// depends on arrival order.
#include "scratch.h"
#include "../../include/icsg3d.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace ics {
namespace {

constexpr int kStructMaxAtoms = 2048;   // atoms per structure (generate.py's max_atoms)
constexpr int kStructMaxImage = 32;     // lattice translations searched per axis: |n| <= 32
constexpr int kStructHist = 95;         // histogram row: atomic numbers 0..94 (0 is never counted)
constexpr double kStructMaxCoord = 1e150;

// reason bits of an invalid structure (ics_op_structure_screen's `reason`)
constexpr int kStructReasonClose = 1;     // a pair at or under tol
constexpr int kStructReasonSpecies = 2;   // a species outside 1..94
constexpr int kStructReasonEmpty = 4;     // no atoms

constexpr size_t kStructBudget = (size_t)1 << 20;   // atoms per chunk
constexpr int kStructMaxChunk = 1 << 16;            // structures per chunk
constexpr int kStructSmall = 64;                    // atoms one wave takes
constexpr double kRangeSlack = 1e-9;                // widens every image range: rounding never drops the minimiser
constexpr int kCellStride = 16;                     // doubles per structure: M[9], abc[3], g[3], pad

// dynamic LDS of one group of threads for `cap` atoms (cap even)
__host__ __device__ inline size_t struct_lds_bytes(int cap) {
  return (size_t)cap * 32 + 16 * 8 + 3 * 16 * 4 + 96 * 4 + 16;
}

__device__ __forceinline__ bool key_less(double d1, int i1, int j1, double d2, int i2, int j2) {
  return d1 < d2 || (d1 == d2 && (i1 < i2 || (i1 == i2 && j1 < j2)));
}

template <int NT, int G>
__global__ __launch_bounds__(NT) void structure_screen_kernel(
    const int* __restrict__ ids, int nids, const int* __restrict__ off, const int* __restrict__ species,
    const double* __restrict__ xyz, const double* __restrict__ cells, double tol, int cap, double* __restrict__ frac,
    double* __restrict__ nearest, double* __restrict__ dmin, int* __restrict__ ipair, int* __restrict__ nclose,
    int* __restrict__ valid, int* __restrict__ reason, int* __restrict__ hist) {
  constexpr int NG = NT / G, NW = G / 64;
  static_assert(NW <= 16, "one reduction slot per wave");
  extern __shared__ __align__(16) unsigned char lds[];
  const int tid = threadIdx.x, grp = tid / G, gt = tid % G, wave = gt >> 6;
  const int slot = blockIdx.x * NG + grp;
  const bool active = slot < nids;
  const int s = active ? ids[slot] : 0;
  const int a0 = active ? off[s] : 0;
  const int n = active ? off[s + 1] - a0 : 0;

  unsigned char* base = lds + (size_t)grp * struct_lds_bytes(cap);
  double* fx = reinterpret_cast<double*>(base);
  double* fy = fx + cap;
  double* fz = fy + cap;
  unsigned long long* nbits = reinterpret_cast<unsigned long long*>(fz + cap);
  double* red_d = reinterpret_cast<double*>(nbits + cap);
  int* red_i = reinterpret_cast<int*>(red_d + 16);
  int* red_j = red_i + 16;
  int* red_c = red_j + 16;
  int* h = red_c + 16;
  int* bad = h + 96;

  for (int k = gt; k < 96; k += G) h[k] = 0;
  if (gt == 0) bad[0] = 0;
  __syncthreads();

  const double* c = cells + (size_t)kCellStride * s;
  const double m0 = c[0], m1 = c[1], m2 = c[2], m3 = c[3], m4 = c[4], m5 = c[5], m6 = c[6], m7 = c[7], m8 = c[8];
  const double la = c[9], lb = c[10], lc = c[11], ga = c[12], gb = c[13], gc = c[14];
  const double kInf = __builtin_inf();

  for (int a = gt; a < n; a += G) {
    const size_t q = 3 * (size_t)(a0 + a);
    const double x = xyz[q] / la, y = xyz[q + 1] / lb, z = xyz[q + 2] / lc;
    frac[q] = x; frac[q + 1] = y; frac[q + 2] = z;
    fx[a] = x - floor(x); fy[a] = y - floor(y); fz[a] = z - floor(z);
    nbits[a] = (unsigned long long)__double_as_longlong(kInf);
    const int zz = species[a0 + a];
    if (zz >= 1 && zz < kStructHist) atomicAdd(&h[zz], 1);
    else atomicOr(&bad[0], 1);
  }
  __syncthreads();

  double bd = kInf;
  int bi = -1, bj = -1, cnt = 0;
  const int P = n * (n - 1) / 2;
  const double tn = 2.0 * n - 1.0;
  for (int p = gt; p < P; p += G) {
    // pair p of the row-major upper triangle: row i starts at i (2n - i - 1) / 2
    int i = (int)((tn - sqrt(tn * tn - 8.0 * p)) * 0.5);
    i = min(max(i, 0), n - 2);
    while (i > 0 && i * (2 * n - i - 1) / 2 > p) --i;
    while ((i + 1) * (2 * n - i - 2) / 2 <= p) ++i;
    const int j = p - i * (2 * n - i - 1) / 2 + i + 1;
    double da = fx[j] - fx[i], db = fy[j] - fy[i], dc = fz[j] - fz[i];
    da -= rint(da); db -= rint(db); dc -= rint(dc);
    const double x0 = da * m0 + db * m3 + dc * m6, y0 = da * m1 + db * m4 + dc * m7, z0 = da * m2 + db * m5 + dc * m8;
    const double D0 = sqrt(x0 * x0 + y0 * y0 + z0 * z0);
    const double lim = (double)kStructMaxImage;
    const int loa = (int)fmax(ceil(-da - D0 * ga - kRangeSlack), -lim), hia = (int)fmin(floor(-da + D0 * ga + kRangeSlack), lim);
    const int lob = (int)fmax(ceil(-db - D0 * gb - kRangeSlack), -lim), hib = (int)fmin(floor(-db + D0 * gb + kRangeSlack), lim);
    const int loc = (int)fmax(ceil(-dc - D0 * gc - kRangeSlack), -lim), hic = (int)fmin(floor(-dc + D0 * gc + kRangeSlack), lim);
    double b2 = kInf;
    for (int na = loa; na <= hia; ++na) {
      const double ta = da + (double)na;
      const double ax = ta * m0, ay = ta * m1, az = ta * m2;
      for (int nb = lob; nb <= hib; ++nb) {
        const double tb = db + (double)nb;
        const double bx = fma(tb, m3, ax), by = fma(tb, m4, ay), bz = fma(tb, m5, az);
        for (int nc = loc; nc <= hic; ++nc) {
          const double tc = dc + (double)nc;
          const double x = fma(tc, m6, bx), y = fma(tc, m7, by), z = fma(tc, m8, bz);
          b2 = fmin(b2, x * x + y * y + z * z);
        }
      }
    }
    const double d = sqrt(b2);
    const unsigned long long bits = (unsigned long long)__double_as_longlong(d);
    atomicMin(&nbits[i], bits);
    atomicMin(&nbits[j], bits);
    cnt += d <= tol ? 1 : 0;
    if (key_less(d, i, j, bd, bi, bj) || bi < 0) { bd = d; bi = i; bj = j; }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double od = __shfl_xor(bd, o, 64);
    const int oi = __shfl_xor(bi, o, 64), oj = __shfl_xor(bj, o, 64);
    cnt += __shfl_xor(cnt, o, 64);
    if (oi >= 0 && (bi < 0 || key_less(od, oi, oj, bd, bi, bj))) { bd = od; bi = oi; bj = oj; }
  }
  if (NW > 1) {
    if ((gt & 63) == 0) { red_d[wave] = bd; red_i[wave] = bi; red_j[wave] = bj; red_c[wave] = cnt; }
  }
  __syncthreads();   // the atomic minima and the wave slots are complete
  if (NW > 1 && gt == 0) {
    bd = red_d[0]; bi = red_i[0]; bj = red_j[0]; cnt = red_c[0];
    for (int w = 1; w < NW; ++w) {
      cnt += red_c[w];
      if (red_i[w] >= 0 && (bi < 0 || key_less(red_d[w], red_i[w], red_j[w], bd, bi, bj))) {
        bd = red_d[w]; bi = red_i[w]; bj = red_j[w];
      }
    }
  }
  if (!active) return;
  for (int a = gt; a < n; a += G) nearest[a0 + a] = __longlong_as_double((long long)nbits[a]);
  for (int k = gt; k < kStructHist; k += G) hist[(size_t)kStructHist * s + k] = h[k];
  if (gt == 0) {
    int r = 0;
    if (n == 0) r |= kStructReasonEmpty;
    if (cnt > 0) r |= kStructReasonClose;
    if (bad[0]) r |= kStructReasonSpecies;
    dmin[s] = bi < 0 ? kInf : bd;
    ipair[2 * s] = bi; ipair[2 * s + 1] = bj;
    nclose[s] = cnt;
    reason[s] = r;
    valid[s] = r == 0 ? 1 : 0;
  }
}

template <int NT, int G>
int launch_screen(hipStream_t st, const int* ids, int nids, int cap, const int* off, const int* species,
                  const double* xyz, const double* cells, double tol, double* frac, double* nearest, double* dmin,
                  int* ipair, int* nclose, int* valid, int* reason, int* hist) {
  constexpr int NG = NT / G;
  const size_t lds = NG * struct_lds_bytes(cap);
  auto kern = structure_screen_kernel<NT, G>;
  if (lds > 65536)
    ICS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
  ICS_LAUNCH(kern, dim3((unsigned)((nids + NG - 1) / NG)), dim3(NT), lds, st, ids, nids, off, species, xyz, cells, tol,
             cap, frac, nearest, dmin, ipair, nclose, valid, reason, hist);
  ICS_HIP(hipGetLastError());
  return 0;
}

// Per structure: the lattice of Lattice.from_parameters (rows va, vb, vc), its volume and the norms of the columns of
// its inverse.  0, or -1 where the six parameters make no cell.
int structure_cell(const double abc[3], const double angles[3], double M[9], double* volume, double g[3]) {
  // Lattice.from_parameters; the sine and cosine of exactly 90 degrees are taken as 1 and 0
  double sn[3], cs[3];
  for (int k = 0; k < 3; ++k) {
    if (!(angles[k] > 0.0 && angles[k] < 180.0)) return -1;
    if (angles[k] == 90.0) { sn[k] = 1.0; cs[k] = 0.0; }
    else { const double r = angles[k] * M_PI / 180.0; sn[k] = std::sin(r); cs[k] = std::cos(r); }
  }
  const double val = (cs[0] * cs[1] - cs[2]) / (sn[0] * sn[1]);
  if (!(std::fabs(val) < 1.0)) return -1;
  const double gs = std::acos(val);
  const double a = abc[0], b = abc[1], c = abc[2];
  M[0] = a * sn[1]; M[1] = 0.0; M[2] = a * cs[1];
  M[3] = -b * sn[0] * std::cos(gs); M[4] = b * sn[0] * std::sin(gs); M[5] = b * cs[0];
  M[6] = 0.0; M[7] = 0.0; M[8] = c;
  const double* va = M; const double* vb = M + 3; const double* vc = M + 6;
  auto cross = [](const double* u, const double* v, double* o) {
    o[0] = u[1] * v[2] - u[2] * v[1]; o[1] = u[2] * v[0] - u[0] * v[2]; o[2] = u[0] * v[1] - u[1] * v[0];
  };
  auto norm = [](const double* u) { return std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]); };
  double bc[3], ca[3], ab[3];
  cross(vb, vc, bc); cross(vc, va, ca); cross(va, vb, ab);
  const double vol = va[0] * bc[0] + va[1] * bc[1] + va[2] * bc[2];
  if (!(vol > 0.0) || !std::isfinite(vol)) return -1;
  *volume = vol;
  g[0] = norm(bc) / vol; g[1] = norm(ca) / vol; g[2] = norm(ab) / vol;   // column norms of inv(M)
  return 0;
}

}  // namespace
}  // namespace ics

using namespace ics;

// The argument rules of include/icsg3d.h, every structure checked before anything is written.  Then chunked under a
// device-memory budget through the calling thread's scratch, one upload, at most two launches and one download per chunk;
// synchronous on the calling thread's stream.
extern "C" int ics_op_structure_screen(const int32_t* offsets, const int32_t* species, const double* xyz, const double* abc,
                                       const double* angles, int batch, double tol, double* lattice, double* volume,
                                       double* frac, double* min_dist, int32_t* min_pair, int32_t* n_close, int32_t* valid,
                                       int32_t* reason, double* nearest, int32_t* hist) {
  const std::string op = "ics_op_structure_screen: ";
  ICS_CHECK(batch >= 1, op + "batch must be >= 1");
  ICS_CHECK(offsets && abc && angles, op + "null argument");
  ICS_CHECK(std::isfinite(tol) && tol >= 0.0, op + "tol must be finite and >= 0");
  ICS_CHECK(offsets[0] == 0, op + "offsets[0] must be 0");
  for (int s = 0; s < batch; ++s) {
    const long long n = (long long)offsets[s + 1] - offsets[s];
    ICS_CHECK(n >= 0, op + "offsets decrease at structure " + std::to_string(s));
    ICS_CHECK(n <= kStructMaxAtoms, op + "structure " + std::to_string(s) + " has " + std::to_string(n) +
                                        " atoms, above the limit of " + std::to_string(kStructMaxAtoms));
  }
  ICS_CHECK((species && xyz) || offsets[batch] == 0, op + "null species or xyz");
  for (int s = 0; s < batch; ++s) {
    const std::string who = op + "structure " + std::to_string(s);
    for (int k = 0; k < 3; ++k) {
      const double l = abc[3 * s + k], t = angles[3 * s + k];
      ICS_CHECK(std::isfinite(l) && std::isfinite(t), who + " has a non-finite cell parameter");
      ICS_CHECK(l > 0.0, who + " has a cell length <= 0");
      ICS_CHECK(l >= 1.0 / kStructMaxCoord && l <= kStructMaxCoord, who + " has a cell length out of range");
    }
    double M[9], vol, g[3];
    ICS_CHECK(structure_cell(abc + 3 * s, angles + 3 * s, M, &vol, g) == 0,
              who + ": the angles make no cell (volume <= 0)");
    const double dmax = 0.5 * (abc[3 * s] + abc[3 * s + 1] + abc[3 * s + 2]);
    for (int k = 0; k < 3; ++k)
      ICS_CHECK(dmax * g[k] + 0.5 + kRangeSlack <= (double)kStructMaxImage,
                who + ": the cell is too skewed, its image search exceeds " + std::to_string(kStructMaxImage) +
                    " translations per axis");
    for (long long k = 3LL * offsets[s]; k < 3LL * offsets[s + 1]; ++k)
      ICS_CHECK(std::isfinite(xyz[k]) && std::fabs(xyz[k]) <= kStructMaxCoord,
                who + " has a non-finite or out-of-range (> 1e150) coordinate");
  }
  ICS_CHECK(lattice && volume && min_dist && min_pair && n_close && valid && reason && hist,
            "ics_op_structure_screen: null output");
  ICS_CHECK((frac && nearest) || offsets[batch] == 0, "ics_op_structure_screen: null frac or nearest");
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  std::vector<unsigned char> hin, hout;
  for (int s0 = 0; s0 < batch;) {
    // one chunk: structures [s0, s1) under the atom budget (at least one structure)
    int s1 = s0, nbig = 0, capbig = 2;
    size_t atoms = 0;
    while (s1 < batch && s1 - s0 < kStructMaxChunk) {
      const int n = offsets[s1 + 1] - offsets[s1];
      if (s1 > s0 && atoms + n > kStructBudget) break;
      atoms += n;
      if (n > kStructSmall) { ++nbig; capbig = std::max(capbig, (n + 1) & ~1); }
      ++s1;
    }
    const int ns = s1 - s0, nsmall = ns - nbig;
    const int A0 = offsets[s0];
    const size_t N = atoms;
    // upload: cells | xyz | offsets | species | ids (small first)     download: frac | nearest | dmin | int rows
    Layout in(16), res(16);
    const auto i_cell = in.add<double>((size_t)ns * kCellStride), i_xyz = in.add<double>(3 * N + 1);
    const auto i_off = in.add<int>(ns + 1), i_spec = in.add<int>(N + 1), i_ids = in.add<int>(ns);
    const auto o_frac = res.add<double>(3 * N + 1), o_near = res.add<double>(N + 1), o_dmin = res.add<double>(ns);
    const auto o_pair = res.add<int>(2 * (size_t)ns), o_close = res.add<int>(ns), o_valid = res.add<int>(ns);
    const auto o_reason = res.add<int>(ns), o_hist = res.add<int>((size_t)ns * kStructHist);
    hin.assign(in.bytes(), 0);
    double *hc, *hxyz;
    int *ho, *hspec, *hi;
    ICS_TRY(in.bind(hin.data(), hin.size(), i_cell, &hc, i_xyz, &hxyz, i_off, &ho, i_spec, &hspec, i_ids, &hi));
    int ks = 0, kb = nsmall;
    for (int k = 0; k < ns; ++k) {
      const int s = s0 + k;
      double* c = hc + (size_t)kCellStride * k;
      if (structure_cell(abc + 3 * s, angles + 3 * s, c, &volume[s], c + 12) != 0) {
        set_error("ics_op_structure_screen: cell of structure " + std::to_string(s) + " changed during the call");
        return -1;
      }
      std::memcpy(lattice + 9 * (size_t)s, c, 72);
      std::memcpy(c + 9, abc + 3 * s, 24);
      ho[k] = offsets[s] - A0;
      if (offsets[s + 1] - offsets[s] > kStructSmall) hi[kb++] = k; else hi[ks++] = k;
    }
    ho[ns] = offsets[s1] - A0;
    if (N) {
      std::memcpy(hxyz, xyz + 3 * (size_t)A0, N * 24);
      std::memcpy(hspec, species + A0, N * 4);
    }
    Layout L;
    const auto s_in = L.add<unsigned char>(in.bytes()), s_res = L.add<unsigned char>(res.bytes());
    unsigned char *din, *dres;
    ICS_TRY(L.reserve(s_in, &din, s_res, &dres));
    ICS_TRY(L.upload(s_in, hin.data(), in.bytes(), st));
    double *dcell, *dxyz, *dfrac, *dnear, *ddmin;
    int *doff, *dspec, *dids, *dpair, *dclose, *dvalid, *dreason, *dhist;
    ICS_TRY(in.bind(din, s_in.count, i_cell, &dcell, i_xyz, &dxyz, i_off, &doff, i_spec, &dspec, i_ids, &dids));
    ICS_TRY(res.bind(dres, s_res.count, o_frac, &dfrac, o_near, &dnear, o_dmin, &ddmin, o_pair, &dpair,
                     o_close, &dclose, o_valid, &dvalid, o_reason, &dreason, o_hist, &dhist));
    if (nsmall)
      ICS_TRY((launch_screen<256, 64>(st, dids, nsmall, kStructSmall, doff, dspec, dxyz, dcell, tol, dfrac, dnear, ddmin,
                                      dpair, dclose, dvalid, dreason, dhist)));
    if (nbig)
      ICS_TRY((launch_screen<1024, 1024>(st, dids + nsmall, nbig, capbig, doff, dspec, dxyz, dcell, tol, dfrac, dnear,
                                         ddmin, dpair, dclose, dvalid, dreason, dhist)));
    hout.resize(res.bytes());
    ICS_TRY(L.download(hout.data(), s_res, res.bytes(), st));
    ICS_HIP(hipStreamSynchronize(st));
    // the same layout over the downloaded block
    ICS_TRY(res.bind(hout.data(), hout.size(), o_frac, &dfrac, o_near, &dnear, o_dmin, &ddmin, o_pair, &dpair,
                     o_close, &dclose, o_valid, &dvalid, o_reason, &dreason, o_hist, &dhist));
    if (N) {
      std::memcpy(frac + 3 * (size_t)A0, dfrac, N * 24);
      std::memcpy(nearest + A0, dnear, N * 8);
    }
    std::memcpy(min_dist + s0, ddmin, (size_t)ns * 8);
    std::memcpy(min_pair + 2 * (size_t)s0, dpair, (size_t)ns * 8);
    std::memcpy(n_close + s0, dclose, (size_t)ns * 4);
    std::memcpy(valid + s0, dvalid, (size_t)ns * 4);
    std::memcpy(reason + s0, dreason, (size_t)ns * 4);
    std::memcpy(hist + (size_t)kStructHist * s0, dhist, (size_t)ns * kStructHist * 4);
    s0 = s1;
  }
  return 0;
}
