// Structural fingerprints for generate.py's results: a radial distribution function per crystal (plain and Z-weighted),
// every atom's nearest distance and coordination number, and the nearest partners of fingerprints by rms distance.  The
// descriptor is the project's own (include/icsg3d.h states it in full; no parity with pymatgen's or matminer's
// fingerprints is claimed).  The arithmetic both kernels and the stand-alone check share is fingerprint.h's.
//
// ics_op_structure_fingerprint.  Ownership as in structure_map.h: one wave per structure of up to 64 atoms (four per
// 256-thread workgroup), one workgroup above that; thread k owns atom k as the pair's first atom i.  The wrapped
// coordinates and Z live in LDS.  The sweep is uniform over the owning group: for j ascending, for T in lexicographic
// order (Ta, Tb, Tc ascending), every lane computes d for its own i; the lanes with 0 < d < R are balloted and their
// (d, weight) broadcast one by one, in lane order, to the whole wave, where lane b owns the bins b, b + 64, b + 128,
// b + 192 and adds the pair's deposit to them.  So every bin is summed in the order (j, T, i) by one lane -- no atomics on
// doubles, no scratch list -- and the four waves of a workgroup (atoms 0..63, 64..127, ...) are added in wave order.  The
// same sweep keeps the atom's smallest d; a second one counts the neighbours within (1 + cn_tol) of it.  The image range
// is one per structure, wide enough for both (fp_reach).  Chunks are runs of structures: nothing a structure's result is
// made of depends on which chunk it is in.
//
// ics_op_fingerprint_nearest.  The valid rows are packed on the host; a thread owns a row (read from a transposed copy, so
// a wave's loads are contiguous) and walks a segment of 512 consecutive partners, 16 at a time, staged in LDS 64 components
// at a time and read as broadcasts; the squared differences are summed in ascending k into 16 registers.  A block is 256
// rows x one segment and writes per row the segment's (minimum, partner, sum over partners above the row); a second kernel
// (one thread per row) folds the segments in ascending order into the row's state.  Rows of queries against references,
// references against queries and queries against queries are three such problems -- D is symmetric bit for bit, so the
// nearest query of a reference needs no column minima.  A chunk is a run of segments; the fold is sequential over
// segments, so the chunking does not show.
#include "structure_map.h"
#include "fingerprint.h"
#include "../../include/icsg3d.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <limits>

namespace ics {
namespace {

constexpr long long kFpChunkBytes = 1LL << 26;     // tables and results of one fingerprint chunk
constexpr long long kFpChunkPairs = 1LL << 28;     // row x partner pairs of one nearest chunk
constexpr size_t kFpTableBudget = (size_t)3 << 30; // resident fingerprint rows (both copies)
constexpr int kSeg = 512;                          // partners per segment
constexpr int kSegMax = 32768;                     // segments per launch (gridDim.y)
constexpr int kTP = 16, kKT = 64;                  // partners and components staged at a time

long long fp_chunk_bytes() {
  static const long long v = env_cap("ICSG3D_FINGERPRINT_CHUNK_BYTES", kFpChunkBytes);
  return v;
}
long long fp_chunk_pairs() {
  static const long long v = env_cap("ICSG3D_FINGERPRINT_CHUNK_PAIRS", kFpChunkPairs);
  return v;
}

struct FpRec {
  double m[9], vol, zbar;
  int at, n, t[3], pad;
};
static_assert(sizeof(FpRec) == 112, "FpRec is uploaded as bytes");

template <int G>
__global__ __launch_bounds__(256) void fingerprint_kernel(int ns, const FpRec* __restrict__ recs,
                                                          const double* __restrict__ afrac, const int* __restrict__ az,
                                                          double r_max, int n_bins, double w, double cn_tol,
                                                          double* __restrict__ rdf, double* __restrict__ count,
                                                          long long* __restrict__ npairs, double* __restrict__ nn,
                                                          int* __restrict__ cn) {
  constexpr int NT = 256, NG = NT / G, NW = G / 64, NB = kFpMaxBins / 64;
  __shared__ double fx[NG][G], fy[NG][G], fz[NG][G];
  __shared__ int zs[NG][G];
  __shared__ double red[NW > 1 ? NW : 1][2][NW > 1 ? kFpMaxBins : 1];
  __shared__ long long redn[NW > 1 ? NW : 1];
  const int tid = threadIdx.x, grp = tid / G, gt = tid % G, lane = gt & 63, wave = gt >> 6;
  const int slot = blockIdx.x * NG + grp;
  const bool active = slot < ns;
  const FpRec* rc = recs + (active ? slot : 0);
  const int n = active ? rc->n : 0, at = rc->at;
  const int Ta = rc->t[0], Tb = rc->t[1], Tc = rc->t[2];
  const double zbar = rc->zbar, vol = rc->vol;
  double m[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = rc->m[k];
  const bool have = gt < n;
  if (have) {
    const double x = afrac[3 * (size_t)(at + gt)], y = afrac[3 * (size_t)(at + gt) + 1], z = afrac[3 * (size_t)(at + gt) + 2];
    fx[grp][gt] = x - floor(x); fy[grp][gt] = y - floor(y); fz[grp][gt] = z - floor(z);
    zs[grp][gt] = az[at + gt];
  }
  __syncthreads();

  const double R = r_max + w;
  const double fix = have ? fx[grp][gt] : 0.0, fiy = have ? fy[grp][gt] : 0.0, fiz = have ? fz[grp][gt] : 0.0;
  const int zi = have ? zs[grp][gt] : 1;
  double lo[NB], hi[NB], ac[NB], aw[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int k = lane + 64 * b;
    const bool own = k < n_bins;
    lo[b] = own ? fp_edge(k, r_max, n_bins) : 0.0;       // an unowned slot is the empty bin [0, 0): it deposits 0
    hi[b] = own ? fp_edge(k + 1, r_max, n_bins) : 0.0;
    ac[b] = aw[b] = 0.0;
  }
  long long cnt = 0;
  double mn = __builtin_inf();
  for (int j = 0; j < n; ++j) {
    const double ex = fx[grp][j] - fix, ey = fy[grp][j] - fiy, ez = fz[grp][j] - fiz;
    const double wgt = fp_weight(zi, zs[grp][j], zbar);
    for (int ta = -Ta; ta <= Ta; ++ta)
      for (int tb = -Tb; tb <= Tb; ++tb)
        for (int tc = -Tc; tc <= Tc; ++tc) {
          const double da = ex + (double)ta, db = ey + (double)tb, dc = ez + (double)tc;
          const double vx = da * m[0] + db * m[3] + dc * m[6], vy = da * m[1] + db * m[4] + dc * m[7],
                       vz = da * m[2] + db * m[5] + dc * m[8];
          const double d2 = vx * vx + vy * vy + vz * vz, d = sqrt(d2);
          const bool pos = have && d > 0.0, in = pos && d < R;
          if (pos && d2 < mn) mn = d2;
          cnt += in ? 1 : 0;
          unsigned long long mask = __ballot(in);
          while (mask != 0ull) {                               // uniform over the wave: the pairs in lane order
            const int src = __ffsll((long long)mask) - 1;
            mask &= mask - 1ull;
            const double dd = __shfl(d, src, 64), ww = __shfl(wgt, src, 64);
#pragma unroll
            for (int b = 0; b < NB; ++b)
              if (64 * b < n_bins) {
                const double dep = fp_deposit(lo[b], hi[b], dd, w);
                ac[b] += dep;
                aw[b] += dep * ww;
              }
          }
        }
  }
  const double nnd = sqrt(mn), thr = (1.0 + cn_tol) * nnd;
  int c = 0;
  for (int j = 0; j < n; ++j) {
    const double ex = fx[grp][j] - fix, ey = fy[grp][j] - fiy, ez = fz[grp][j] - fiz;
    for (int ta = -Ta; ta <= Ta; ++ta)
      for (int tb = -Tb; tb <= Tb; ++tb)
        for (int tc = -Tc; tc <= Tc; ++tc) {
          const double da = ex + (double)ta, db = ey + (double)tb, dc = ez + (double)tc;
          const double vx = da * m[0] + db * m[3] + dc * m[6], vy = da * m[1] + db * m[4] + dc * m[7],
                       vz = da * m[2] + db * m[5] + dc * m[8];
          const double d = sqrt(vx * vx + vy * vy + vz * vz);
          c += (d > 0.0 && d <= thr) ? 1 : 0;
        }
  }
  if (have) {
    nn[at + gt] = nnd;
    cn[at + gt] = c;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (NW == 1) {
    if (active) {
      if (lane == 0) npairs[slot] = cnt;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int k = lane + 64 * b;
        if (k < n_bins) {
          const double norm = fp_shell_norm(n, vol, lo[b], hi[b]);
          count[(size_t)slot * n_bins + k] = ac[b];
          rdf[((size_t)slot * 2) * n_bins + k] = ac[b] / norm;
          rdf[((size_t)slot * 2 + 1) * n_bins + k] = aw[b] / norm;
        }
      }
    }
  } else {                                                     // the whole workgroup is one structure: barriers by all
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      red[wave][0][lane + 64 * b] = ac[b];
      red[wave][1][lane + 64 * b] = aw[b];
    }
    if (lane == 0) redn[wave] = cnt;
    __syncthreads();
    if (active && gt < n_bins) {
      double sc = red[0][0][gt], sw = red[0][1][gt];
      for (int v = 1; v < NW; ++v) { sc += red[v][0][gt]; sw += red[v][1][gt]; }
      const double norm = fp_shell_norm(n, vol, fp_edge(gt, r_max, n_bins), fp_edge(gt + 1, r_max, n_bins));
      count[(size_t)slot * n_bins + gt] = sc;
      rdf[((size_t)slot * 2) * n_bins + gt] = sc / norm;
      rdf[((size_t)slot * 2 + 1) * n_bins + gt] = sw / norm;
    }
    if (active && gt == 0) {
      long long t = redn[0];
      for (int v = 1; v < NW; ++v) t += redn[v];
      npairs[slot] = t;
    }
  }
}

template <int G>
int launch_fingerprint(hipStream_t st, int ns, const FpRec* recs, const double* afrac, const int* az, double r_max,
                       int n_bins, double w, double cn_tol, double* rdf, double* count, long long* npairs, double* nn,
                       int* cn) {
  constexpr int NG = 256 / G;
  ICS_LAUNCH(fingerprint_kernel<G>, dim3((unsigned)((ns + NG - 1) / NG)), dim3(256), 0, st, ns, recs, afrac, az, r_max, n_bins,
             w, cn_tol, rdf, count, npairs, nn, cn);
  ICS_HIP(hipGetLastError());
  return 0;
}

// out[k][r] = in[r][k] for n rows of len components
__global__ __launch_bounds__(256) void fp_transpose_kernel(const double* __restrict__ in, int n, int len,
                                                           double* __restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)n * len;
  if (idx >= total) return;
  const size_t r = idx / (size_t)len, k = idx % (size_t)len;
  out[k * (size_t)n + r] = in[idx];
}

// Rows [256 blockIdx.x, +256) of X (transposed: xt[k][nx]) against segment seg0 + blockIdx.y of Y (y[p][len]): per row the
// smallest D and its partner (the lower p on a tie) and, with SELF (X and Y are the same rows: p == row is left out), the
// sum of D over the segment's partners p > row in ascending p.
template <bool SELF>
__global__ __launch_bounds__(256) void fp_nearest_kernel(const double* __restrict__ xt, int nx, const double* __restrict__ y,
                                                         int ny, int len, int seg0, int nsegc, double* __restrict__ pd,
                                                         int* __restrict__ pi, double* __restrict__ ps) {
  __shared__ double yt[kKT][kTP];
  const int tid = threadIdx.x, r = blockIdx.x * 256 + tid;
  const bool have = r < nx;
  const long long pbeg = (long long)(seg0 + (int)blockIdx.y) * kSeg;
  const int p_lo = (int)(pbeg < ny ? pbeg : ny), p_hi = (int)(pbeg + kSeg < ny ? pbeg + kSeg : ny);
  double best = __builtin_inf(), sum = 0.0;
  int bi = -1;
  for (int p0 = p_lo; p0 < p_hi; p0 += kTP) {
    double acc[kTP];
#pragma unroll
    for (int t = 0; t < kTP; ++t) acc[t] = 0.0;
    for (int k0 = 0; k0 < len; k0 += kKT) {
      const int kn = min(kKT, len - k0);
      __syncthreads();
      for (int e = tid; e < kTP * kKT; e += 256) {
        const int t = e / kKT, kk = e % kKT;
        yt[kk][t] = (p0 + t < p_hi && kk < kn) ? y[(size_t)(p0 + t) * len + k0 + kk] : 0.0;
      }
      __syncthreads();
      if (have)
        for (int kk = 0; kk < kn; ++kk) {
          const double a = xt[(size_t)(k0 + kk) * nx + r];
#pragma unroll
          for (int t = 0; t < kTP; ++t) {
            const double df = a - yt[kk][t];
            acc[t] = fma(df, df, acc[t]);
          }
        }
    }
#pragma unroll
    for (int t = 0; t < kTP; ++t) {
      const int p = p0 + t;
      if (!have || p >= p_hi || (SELF && p == r)) continue;
      const double D = sqrt(acc[t] / (double)len);
      if (SELF && p > r) sum += D;
      if (D < best) { best = D; bi = p; }
    }
  }
  if (have) {
    const size_t o = (size_t)r * nsegc + blockIdx.y;
    pd[o] = best; pi[o] = bi; ps[o] = sum;
  }
}

// One thread per row: the chunk's segments folded, in ascending order, into the row's state (first: the state starts here).
__global__ __launch_bounds__(256) void fp_nearest_fold_kernel(int nx, int nsegc, int first, const double* __restrict__ pd,
                                                              const int* __restrict__ pi, const double* __restrict__ ps,
                                                              double* __restrict__ sd, int* __restrict__ si,
                                                              double* __restrict__ ss) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= nx) return;
  double best = first ? __builtin_inf() : sd[r], sum = first ? 0.0 : ss[r];
  int bi = first ? -1 : si[r];
  for (int s = 0; s < nsegc; ++s) {
    const size_t o = (size_t)r * nsegc + s;
    if (pd[o] < best) { best = pd[o]; bi = pi[o]; }             // segments ascend: a tie keeps the lower partner
    sum += ps[o];
  }
  sd[r] = best; si[r] = bi; ss[r] = sum;
}

// segments of one launch for nx rows against ny partners
int nearest_segs_per_chunk(int nx, int ny) {
  const int nseg = (ny + kSeg - 1) / kSeg;
  const long long per = fp_chunk_pairs() / ((long long)std::max(nx, 1) * kSeg);
  return (int)std::max<long long>(1, std::min<long long>({per, (long long)nseg, (long long)kSegMax}));
}

// One problem: every row of X against every row of Y, the row states left in (sd, si, ss).
int nearest_problem(hipStream_t st, bool self, const double* xt, int nx, const double* y, int ny, int len, double* pd, int* pi,
                    double* ps, double* sd, int* si, double* ss) {
  const int nseg = (ny + kSeg - 1) / kSeg, per = nearest_segs_per_chunk(nx, ny);
  const dim3 rows((unsigned)((nx + 255) / 256));
  if (nseg == 0) {                                              // no partner: the empty state
    ICS_LAUNCH(fp_nearest_fold_kernel, rows, dim3(256), 0, st, nx, 0, 1, pd, pi, ps, sd, si, ss);
    ICS_HIP(hipGetLastError());
    return 0;
  }
  for (int s0 = 0; s0 < nseg; s0 += per) {
    const int nc = std::min(per, nseg - s0);
    if (self)
      ICS_LAUNCH(fp_nearest_kernel<true>, dim3(rows.x, (unsigned)nc), dim3(256), 0, st, xt, nx, y, ny, len, s0, nc, pd, pi, ps);
    else
      ICS_LAUNCH(fp_nearest_kernel<false>, dim3(rows.x, (unsigned)nc), dim3(256), 0, st, xt, nx, y, ny, len, s0, nc, pd, pi, ps);
    ICS_HIP(hipGetLastError());
    ICS_LAUNCH(fp_nearest_fold_kernel, rows, dim3(256), 0, st, nx, nc, s0 == 0 ? 1 : 0, pd, pi, ps, sd, si, ss);
    ICS_HIP(hipGetLastError());
  }
  return 0;
}

}  // namespace
}  // namespace ics

using namespace ics;

// Eligible structures whose image range fits are ordered small (one wave) before large (one workgroup), each in index
// order, and cut into chunks under kFpChunkBytes (ICSG3D_FINGERPRINT_CHUNK_BYTES shrinks it); synchronous on the calling
// thread's stream.
extern "C" int ics_op_structure_fingerprint(const int32_t* offsets, const int32_t* species, const double* frac,
                                            const double* lattice, const int32_t* eligible, int ns, double r_max,
                                            int n_bins, double width, double cn_tol, double* rdf, double* count,
                                            int64_t* n_pairs, double* nn_dist, int32_t* cn, int32_t* reason) {
  const std::string op = "ics_op_structure_fingerprint: ";
  ICS_CHECK(ns >= 1, op + "ns must be >= 1");
  ICS_CHECK(ns <= INT_MAX - 1, op + "too many structures");
  ICS_CHECK(offsets && lattice && eligible, op + "null argument");
  if (const char* bad = fp_check_params(r_max, n_bins, width, cn_tol)) {
    set_error(op + bad);
    return -1;
  }
  ICS_TRY(check_structures(op, offsets, species, frac, lattice, eligible, ns, 0.0));   // tol 0: no thin-cell rule here
  ICS_CHECK(rdf && count && n_pairs && nn_dist && cn && reason, op + "null output");
  hipStream_t st;
  ICS_TRY(op_stream(&st));

  const double kNaN = std::numeric_limits<double>::quiet_NaN();
  const size_t nb = (size_t)n_bins;
  std::vector<FpRec> recs((size_t)ns);
  std::vector<int> small, large;
  for (int s = 0; s < ns; ++s) {
    const int a0 = offsets[s], n = offsets[s + 1] - a0;
    int bits = eligible[s] ? 0 : 1;
    if (!bits) {
      FpRec& r = recs[(size_t)s];
      const double* M = lattice + 9 * (size_t)s;
      double g[3];
      std::memcpy(r.m, M, 72);
      cell_inverse(M, &r.vol, g, nullptr);
      long long zsum = 0;
      for (int i = 0; i < n; ++i) zsum += species[a0 + i];
      r.zbar = (double)zsum / (double)n;
      r.n = n; r.at = 0; r.pad = 0;
      if (!fp_image_range(fp_reach(r_max, width, cn_tol, M), g, r.t)) bits |= 2;
    }
    reason[s] = bits;
    if (bits) {
      for (size_t k = 0; k < 2 * nb; ++k) rdf[(size_t)s * 2 * nb + k] = kNaN;
      for (size_t k = 0; k < nb; ++k) count[(size_t)s * nb + k] = kNaN;
      n_pairs[s] = -1;
      for (int i = 0; i < n; ++i) { nn_dist[a0 + i] = kNaN; cn[a0 + i] = -1; }
    } else {
      (n <= kMapSmall ? small : large).push_back(s);
    }
  }
  std::vector<int> order(small);
  order.insert(order.end(), large.begin(), large.end());
  const size_t nsmall = small.size(), ne = order.size();

  auto bytes_of = [&](int s) {
    const size_t n = (size_t)(offsets[s + 1] - offsets[s]);
    return sizeof(FpRec) + n * (24 + 4 + 8 + 4) + 3 * nb * 8 + 8;
  };
  for (size_t c0 = 0; c0 < ne;) {
    // one chunk: structures order[c0, c1) of one kernel kind
    const size_t lim = c0 < nsmall ? nsmall : ne;
    size_t c1 = c0, N = 0, bytes = 0;
    while (c1 < lim && (c1 == c0 || bytes + bytes_of(order[c1]) <= (size_t)fp_chunk_bytes())) {
      bytes += bytes_of(order[c1]);
      N += (size_t)(offsets[order[c1] + 1] - offsets[order[c1]]);
      ++c1;
    }
    const size_t nc = c1 - c0;
    Layout in(16);
    const auto i_rec = in.add<FpRec>(nc);
    const auto i_frac = in.add<double>(3 * N);
    const auto i_z = in.add<int>(N);
    std::vector<unsigned char> hin(in.bytes(), 0);
    FpRec* hrec; double* hf; int* hz;
    ICS_TRY(in.bind(hin.data(), hin.size(), i_rec, &hrec, i_frac, &hf, i_z, &hz));
    size_t at = 0;
    for (size_t k = 0; k < nc; ++k) {
      const int s = order[c0 + k], a0 = offsets[s], n = offsets[s + 1] - a0;
      hrec[k] = recs[(size_t)s];
      hrec[k].at = (int)at;
      std::memcpy(hf + 3 * at, frac + 3 * (size_t)a0, (size_t)n * 24);
      std::memcpy(hz + at, species + a0, (size_t)n * 4);
      at += (size_t)n;
    }
    Layout L;
    const auto s_in = L.add<unsigned char>(in.bytes());
    const auto s_rdf = L.add<double>(2 * nb * nc), s_cnt = L.add<double>(nb * nc), s_nn = L.add<double>(N);
    const auto s_np = L.add<long long>(nc);
    const auto s_cn = L.add<int>(N);
    unsigned char* din;
    double *drdf, *dcnt, *dnn, *dfrac;
    long long* dnp;
    int *dcn, *dz;
    FpRec* drec;
    ICS_TRY(L.reserve(s_in, &din, s_rdf, &drdf, s_cnt, &dcnt, s_nn, &dnn, s_np, &dnp, s_cn, &dcn));
    ICS_TRY(L.upload(s_in, hin.data(), in.bytes(), st));
    ICS_TRY(in.bind(din, s_in.count, i_rec, &drec, i_frac, &dfrac, i_z, &dz));
    if (c0 < nsmall)
      ICS_TRY((launch_fingerprint<64>(st, (int)nc, drec, dfrac, dz, r_max, n_bins, width, cn_tol, drdf, dcnt, dnp, dnn, dcn)));
    else
      ICS_TRY((launch_fingerprint<256>(st, (int)nc, drec, dfrac, dz, r_max, n_bins, width, cn_tol, drdf, dcnt, dnp, dnn, dcn)));
    std::vector<double> ordf(2 * nb * nc), ocnt(nb * nc), onn(N);
    std::vector<long long> onp(nc);
    std::vector<int> ocn(N);
    ICS_TRY(L.download(ordf.data(), s_rdf, ordf.size(), st));
    ICS_TRY(L.download(ocnt.data(), s_cnt, ocnt.size(), st));
    ICS_TRY(L.download(onn.data(), s_nn, onn.size(), st));
    ICS_TRY(L.download(onp.data(), s_np, onp.size(), st));
    ICS_TRY(L.download(ocn.data(), s_cn, ocn.size(), st));
    ICS_HIP(hipStreamSynchronize(st));
    at = 0;
    for (size_t k = 0; k < nc; ++k) {
      const int s = order[c0 + k], a0 = offsets[s], n = offsets[s + 1] - a0;
      std::memcpy(rdf + (size_t)s * 2 * nb, ordf.data() + k * 2 * nb, 2 * nb * 8);
      std::memcpy(count + (size_t)s * nb, ocnt.data() + k * nb, nb * 8);
      n_pairs[s] = onp[k];
      std::memcpy(nn_dist + a0, onn.data() + at, (size_t)n * 8);
      std::memcpy(cn + a0, ocn.data() + at, (size_t)n * 4);
      at += (size_t)n;
    }
    c0 = c1;
  }
  return 0;
}

// The valid rows packed, queries then references; three problems (queries x references, references x queries, queries x
// queries), each chunked under kFpChunkPairs (ICSG3D_FINGERPRINT_CHUNK_PAIRS shrinks it); synchronous on the calling
// thread's stream.
extern "C" int ics_op_fingerprint_nearest(const double* fp, const int32_t* valid, int len, int nq, int nref, int32_t* q_ref,
                                          double* q_ref_d, int32_t* ref_q, double* ref_q_d, int32_t* q_q, double* q_q_d,
                                          double* div_sum, int64_t* div_pairs) {
  const std::string op = "ics_op_fingerprint_nearest: ";
  if (const char* bad = fp_check_counts(len, nq, nref)) {
    set_error(op + bad);
    return -1;
  }
  ICS_CHECK(fp && valid, op + "null argument");
  ICS_CHECK(q_ref && q_ref_d && q_q && q_q_d && div_sum && div_pairs && ((ref_q && ref_q_d) || nref == 0), op + "null output");
  const int nrows = nq + nref;
  std::vector<int> vq, vr;
  for (int r = 0; r < nrows; ++r) {
    if (!valid[r]) continue;
    const double* row = fp + (size_t)r * len;
    for (int k = 0; k < len; ++k)
      ICS_CHECK(std::isfinite(row[k]), op + "valid row " + std::to_string(r) + " has a non-finite entry");
    (r < nq ? vq : vr).push_back(r);
  }
  const int nvq = (int)vq.size(), nvr = (int)vr.size();
  const size_t nv = (size_t)nvq + nvr;
  if (2 * nv * (size_t)len * 8 > kFpTableBudget) {
    set_error(op + "the fingerprint rows (" + std::to_string(2 * nv * (size_t)len * 8) + " bytes) exceed the device budget");
    return -1;
  }
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  const double kInf = std::numeric_limits<double>::infinity();
  for (int q = 0; q < nq; ++q) { q_ref[q] = q_q[q] = -1; q_ref_d[q] = q_q_d[q] = kInf; }
  for (int r = 0; r < nref; ++r) { ref_q[r] = -1; ref_q_d[r] = kInf; }
  *div_sum = 0.0;
  *div_pairs = (int64_t)nvq * (nvq - 1) / 2;
  if (nvq == 0) return 0;

  std::vector<double> rows(nv * (size_t)len);
  for (size_t k = 0; k < nv; ++k)
    std::memcpy(rows.data() + k * len, fp + (size_t)(k < (size_t)nvq ? vq[k] : vr[k - nvq]) * len, (size_t)len * 8);
  const size_t pcap = std::max({(size_t)nvq * nearest_segs_per_chunk(nvq, nvr), (size_t)nvr * nearest_segs_per_chunk(nvr, nvq),
                                (size_t)nvq * nearest_segs_per_chunk(nvq, nvq)});
  Layout L;
  const auto s_y = L.add<double>(nv * len), s_t = L.add<double>(nv * len);
  const auto s_pd = L.add<double>(pcap), s_ps = L.add<double>(pcap);
  const auto s_sd = L.add<double>(nv + nvq), s_ss = L.add<double>(nv + nvq);
  const auto s_pi = L.add<int>(pcap), s_si = L.add<int>(nv + nvq);
  double *dy, *dt, *dpd, *dps, *dsd, *dss;
  int *dpi, *dsi;
  ICS_TRY(L.reserve(s_y, &dy, s_t, &dt, s_pd, &dpd, s_ps, &dps, s_sd, &dsd, s_ss, &dss, s_pi, &dpi, s_si, &dsi));
  ICS_TRY(L.upload(s_y, rows.data(), rows.size(), st));
  const size_t qlen = (size_t)nvq * len;
  ICS_LAUNCH(fp_transpose_kernel, dim3((unsigned)((qlen + 255) / 256)), dim3(256), 0, st, dy, nvq, len, dt);
  ICS_HIP(hipGetLastError());
  if (nvr) {
    ICS_LAUNCH(fp_transpose_kernel, dim3((unsigned)(((size_t)nvr * len + 255) / 256)), dim3(256), 0, st, dy + qlen, nvr, len,
               dt + qlen);
    ICS_HIP(hipGetLastError());
  }
  // states: [0, nvq) queries x references, [nvq, nv) references x queries, [nv, nv + nvq) queries x queries
  ICS_TRY(nearest_problem(st, false, dt, nvq, dy + qlen, nvr, len, dpd, dpi, dps, dsd, dsi, dss));
  if (nvr) ICS_TRY(nearest_problem(st, false, dt + qlen, nvr, dy, nvq, len, dpd, dpi, dps, dsd + nvq, dsi + nvq, dss + nvq));
  ICS_TRY(nearest_problem(st, true, dt, nvq, dy, nvq, len, dpd, dpi, dps, dsd + nv, dsi + nv, dss + nv));
  std::vector<double> osd(nv + nvq), oss(nv + nvq);
  std::vector<int> osi(nv + nvq);
  ICS_TRY(L.download(osd.data(), s_sd, osd.size(), st));
  ICS_TRY(L.download(oss.data(), s_ss, oss.size(), st));
  ICS_TRY(L.download(osi.data(), s_si, osi.size(), st));
  ICS_HIP(hipStreamSynchronize(st));
  for (int k = 0; k < nvq; ++k) {
    const int a = osi[k], b = osi[nv + k];
    if (a < -1 || a >= nvr || b < -1 || b >= nvq) { set_error(op + "the device returned a partner out of range"); return -1; }
  }
  for (int k = 0; k < nvr; ++k)
    if (osi[nvq + k] < -1 || osi[nvq + k] >= nvq) { set_error(op + "the device returned a partner out of range"); return -1; }
  double total = 0.0;
  for (int k = 0; k < nvq; ++k) {
    const int q = vq[k], a = osi[k], b = osi[nv + k];
    if (a >= 0) { q_ref[q] = vr[a] - nq; q_ref_d[q] = osd[k]; }
    if (b >= 0) { q_q[q] = vq[b]; q_q_d[q] = osd[nv + k]; }
    total += oss[nv + k];
  }
  for (int k = 0; k < nvr; ++k)
    if (osi[nvq + k] >= 0) { ref_q[vr[k] - nq] = vq[osi[nvq + k]]; ref_q_d[vr[k] - nq] = osd[nvq + k]; }
  *div_sum = total;
  return 0;
}
