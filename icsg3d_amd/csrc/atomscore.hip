// The atom score of a segmentation (gfx950 / MI355X only): the predicted atoms of a sample matched to its true atoms by
// the project's greedy rule and tallied per species on the device.  atomscore.h has the rule, the accumulator's layout
// and the contract of the launches.
//
// One workgroup per sample.  Both atom sets sit in LDS as planes (x, y, z, species, pick, partner); a round is two
// strided scans -- free true atoms over free predicted ones, and the reverse -- then a pairing pass, with a barrier
// behind the scans and one behind the pairing.  In a scan the lanes of a wave hold different atoms of their own side and
// walk the other side together, so every LDS read of the inner loop is a broadcast.  "Something matched" is ONE LDS word
// that holds the number of the last round that matched a pair: it needs no reset, so a round needs no third barrier.
// The tallies follow the matching in the same launch: at most a handful of 64-bit global atomics per atom, integer sums.
#include "atomscore.h"

#include <cmath>

#include "scratch.h"
#include "segment.h"

// d2 is compared against numpy bit for bit: no FMA may be formed from dx * dx + dy * dy
#pragma clang fp contract(off)

namespace ics {

namespace {

// ragged fp64 positions + int32 species with offsets (the layout of ics_op_match_emd)
struct RaggedSrc {
  const double* xyz; const int* species; const int* off;
  __device__ int count(int b) const { return off[b + 1] - off[b]; }
  __device__ size_t base(int b) const { return (size_t)off[b]; }
  __device__ int rows(int, int n) const { return n; }
  __device__ void load(int b, int a, double* x, double* y, double* z, int* s) const {
    const size_t k = (size_t)off[b] + a;
    *x = xyz[3 * k]; *y = xyz[3 * k + 1]; *z = xyz[3 * k + 2]; *s = species[k];
  }
};
// the statistics rows of launch_segment_atoms
struct StatsSrc {
  const int* stats; const int* counts; int max_atoms;
  __device__ int count(int b) const { return counts[2 * b + 1]; }
  __device__ size_t base(int b) const { return (size_t)b * max_atoms; }
  __device__ int rows(int, int) const { return max_atoms; }
  __device__ void load(int b, int a, double* x, double* y, double* z, int* s) const {
    const int* r = stats + ((size_t)b * max_atoms + a) * kSegStatInts;
    const double v = (double)r[1];
    *x = (double)r[4] / v; *y = (double)r[3] / v; *z = (double)r[2] / v; *s = r[0];
  }
};

__device__ __forceinline__ double atom_d2(double tx, double ty, double tz, double px, double py, double pz) {
  const double dx = tx - px, dy = ty - py, dz = tz - pz;
  return ((dx * dx + dy * dy) + dz * dz);
}
__device__ __forceinline__ void acc_add(unsigned long long* p, unsigned long long v) { atomicAdd(p, v); }

template <class Src>
__global__ __launch_bounds__(kAtomScoreThreads) void atom_score_kernel(Src T, Src P, int ncls, double tol2, double hist_scale,
                                                                      int cap, AtomScoreOut out) {
  constexpr int NT = kAtomScoreThreads;
  extern __shared__ __attribute__((aligned(16))) unsigned char atom_lds[];
  double* tx = reinterpret_cast<double*>(atom_lds);
  double *ty = tx + cap, *tz = ty + cap, *px = tz + cap, *py = px + cap, *pz = py + cap;
  int* tsp = reinterpret_cast<int*>(pz + cap);
  int *tpick = tsp + cap, *tpart = tpick + cap, *psp = tpart + cap, *ppick = psp + cap, *ppart = ppick + cap;
  int* cnt = ppart + cap;      // [0] last round that matched, [1] matched, [2] species agree, [3] dup, [4] shadowed
  const int b = blockIdx.x, tid = threadIdx.x;
  const int K = ncls + 1;
  unsigned long long* acc = out.acc;
  unsigned long long* a_dist = acc + (size_t)K * K;
  unsigned long long *a_dist2 = a_dist + ncls, *a_dup = a_dist2 + ncls, *a_shadow = a_dup + ncls;
  unsigned long long* a_hist = a_shadow + ncls;
  unsigned long long* a_tot = a_hist + kAtomScoreHistBins;
  int n = T.count(b), m = P.count(b);
  n = n < 0 ? 0 : n; m = m < 0 ? 0 : m;
  const size_t mbase = T.base(b);
  if (n > cap || m > cap) {                       // failed: nothing of the sample enters LDS
    if (out.match) {
      const int rows = T.rows(b, n);
      for (int i = tid; i < rows; i += NT) out.match[mbase + i] = -1;
    }
    if (tid == 0) {
      acc_add(a_tot + 0, 1ull); acc_add(a_tot + 1, 1ull);
      if (out.sample_stats) {
        int* s = out.sample_stats + (size_t)b * 6;
        s[0] = n; s[1] = m; s[2] = s[3] = s[4] = s[5] = -1;
      }
      if (out.dist_sum) out.dist_sum[b] = __builtin_nan("");
    }
    return;
  }
  for (int i = tid; i < n; i += NT) {
    int s;
    T.load(b, i, &tx[i], &ty[i], &tz[i], &s);
    tsp[i] = (unsigned)s < (unsigned)ncls ? s : 0;
    tpart[i] = -1;
  }
  for (int j = tid; j < m; j += NT) {
    int s;
    P.load(b, j, &px[j], &py[j], &pz[j], &s);
    psp[j] = (unsigned)s < (unsigned)ncls ? s : 0;
    ppart[j] = -1;
  }
  if (tid < 8) cnt[tid] = 0;
  __syncthreads();
  const int max_rounds = n < m ? n : m;
  for (int r = 1; r <= max_rounds; ++r) {
    for (int i = tid; i < n; i += NT) {
      if (tpart[i] >= 0) continue;
      const double x = tx[i], y = ty[i], z = tz[i];
      double bd = tol2;
      int bj = -1;
      for (int j = 0; j < m; ++j) {
        if (ppart[j] >= 0) continue;
        const double d2 = atom_d2(x, y, z, px[j], py[j], pz[j]);
        if (d2 < bd) { bd = d2; bj = j; }          // ascending j: an equal d2 keeps the smaller j
      }
      tpick[i] = bj;
    }
    for (int j = tid; j < m; j += NT) {
      if (ppart[j] >= 0) continue;
      const double x = px[j], y = py[j], z = pz[j];
      double bd = tol2;
      int bi = -1;
      for (int i = 0; i < n; ++i) {
        if (tpart[i] >= 0) continue;
        const double d2 = atom_d2(tx[i], ty[i], tz[i], x, y, z);
        if (d2 < bd) { bd = d2; bi = i; }
      }
      ppick[j] = bi;
    }
    __syncthreads();
    for (int i = tid; i < n; i += NT) {
      if (tpart[i] >= 0) continue;
      const int j = tpick[i];
      if (j >= 0 && ppick[j] == i) { tpart[i] = j; ppart[j] = i; cnt[0] = r; }
    }
    __syncthreads();
    if (cnt[0] != r) break;                        // uniform: every lane reads it behind the barrier
  }
  // ---- tallies
  for (int i = tid; i < n; i += NT) {
    const int ts = tsp[i], j = tpart[i];
    if (j >= 0) {
      const double d2 = atom_d2(tx[i], ty[i], tz[i], px[j], py[j], pz[j]);
      const double dist = __dsqrt_rn(d2);
      acc_add(acc + (size_t)ts * K + psp[j], 1ull);
      acc_add(a_dist + ts, (unsigned long long)llrint(dist * kAtomScoreFix));
      acc_add(a_dist2 + ts, (unsigned long long)llrint(d2 * kAtomScoreFix));
      const double hb = floor(dist * hist_scale);
      acc_add(a_hist + (hb < (double)(kAtomScoreHistBins - 1) ? (int)hb : kAtomScoreHistBins - 1), 1ull);
      atomicAdd(&cnt[1], 1);
      if (ts == psp[j]) atomicAdd(&cnt[2], 1);
    } else {
      acc_add(acc + (size_t)ts * K + ncls, 1ull);
      bool near = false;
      for (int q = 0; q < m && !near; ++q) near = atom_d2(tx[i], ty[i], tz[i], px[q], py[q], pz[q]) < tol2;
      if (near) { acc_add(a_shadow + ts, 1ull); atomicAdd(&cnt[4], 1); }
    }
  }
  for (int j = tid; j < m; j += NT) {
    if (ppart[j] >= 0) continue;
    const int ps = psp[j];
    acc_add(acc + (size_t)ncls * K + ps, 1ull);
    bool near = false;
    for (int q = 0; q < n && !near; ++q) near = atom_d2(tx[q], ty[q], tz[q], px[j], py[j], pz[j]) < tol2;
    if (near) { acc_add(a_dup + ps, 1ull); atomicAdd(&cnt[3], 1); }
  }
  if (out.match) {
    const int rows = T.rows(b, n);
    for (int i = tid; i < rows; i += NT) out.match[mbase + i] = i < n ? tpart[i] : -1;
  }
  __syncthreads();
  if (tid == 0) {
    const int matched = cnt[1], agree = cnt[2];
    acc_add(a_tot + 0, 1ull);
    if (matched == n && matched == m && agree == matched) acc_add(a_tot + 2, 1ull);
    if (n) acc_add(a_tot + 3, (unsigned long long)n);
    if (m) acc_add(a_tot + 4, (unsigned long long)m);
    if (matched) acc_add(a_tot + 5, (unsigned long long)matched);
    if (n != m) acc_add(a_tot + 6, (unsigned long long)(n > m ? n - m : m - n));
    if (n == 0) acc_add(a_tot + 7, 1ull);
    if (out.sample_stats) {
      int* s = out.sample_stats + (size_t)b * 6;
      s[0] = n; s[1] = m; s[2] = matched; s[3] = agree; s[4] = cnt[3]; s[5] = cnt[4];
    }
    if (out.dist_sum) {
      double sum = 0.0;
      for (int i = 0; i < n; ++i) {
        const int j = tpart[i];
        if (j >= 0) sum += __dsqrt_rn(atom_d2(tx[i], ty[i], tz[i], px[j], py[j], pz[j]));
      }
      out.dist_sum[b] = sum;
    }
  }
}

template <class Src>
int atom_score_launch(hipStream_t st, const Src& T, const Src& P, int batch, int ncls, double tol2, double hist_scale,
                      int cap, const AtomScoreOut& out) {
  ICS_CHECK(batch >= 1 && cap >= 0 && cap <= kAtomScoreMaxAtoms && out.acc != nullptr, "atom score: bad launch arguments");
  ICS_CHECK(ncls >= kAtomScoreMinCls && ncls <= kAtomScoreMaxCls, "atom score: num_classes must be in [2, 127]");
  const int cap_lds = cap < 1 ? 1 : cap;
  const size_t lds = atom_score_lds_bytes(cap_lds);
  auto kern = atom_score_kernel<Src>;
  if (lds > 65536)
    ICS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  ICS_LAUNCH(kern, dim3((unsigned)batch), dim3(kAtomScoreThreads), lds, st, T, P, ncls, tol2, hist_scale, cap_lds, out);
  ICS_HIP(hipGetLastError());
  return 0;
}

}  // namespace

int launch_atom_score_ragged(hipStream_t st, const double* t_xyz, const int* t_species, const int* t_off, const double* p_xyz,
                             const int* p_species, const int* p_off, int batch, int ncls, double tol2, double hist_scale,
                             int cap, const AtomScoreOut& out) {
  ICS_CHECK(t_off && p_off, "atom score: null offsets");
  return atom_score_launch(st, RaggedSrc{t_xyz, t_species, t_off}, RaggedSrc{p_xyz, p_species, p_off}, batch, ncls, tol2,
                           hist_scale, cap, out);
}

int launch_atom_score_stats(hipStream_t st, const int* t_stats, const int* t_counts, const int* p_stats, const int* p_counts,
                            int batch, int max_atoms, int ncls, double tol2, double hist_scale, const AtomScoreOut& out) {
  ICS_CHECK(t_stats && t_counts && p_stats && p_counts, "atom score: null statistics");
  ICS_CHECK(max_atoms >= 1 && max_atoms <= kAtomScoreMaxAtoms, "atom score: max_atoms must be in [1, 1024]");
  return atom_score_launch(st, StatsSrc{t_stats, t_counts, max_atoms}, StatsSrc{p_stats, p_counts, max_atoms}, batch, ncls,
                           tol2, hist_scale, max_atoms, out);
}

int atom_score_params(const std::string& who, int ncls, double tol, double* tol2, double* hist_scale) {
  ICS_CHECK(ncls >= kAtomScoreMinCls && ncls <= kAtomScoreMaxCls, who + ": num_classes must be in [2, 127]");
  ICS_CHECK(std::isfinite(tol) && tol > 0.0, who + ": tol must be finite and > 0");
  ICS_CHECK(tol <= kAtomScoreMaxTol, who + ": tol above 1e6 voxels (the fixed-point sums would overflow)");
  *tol2 = tol * tol;
  *hist_scale = (double)kAtomScoreHistBins / tol;
  return 0;
}

}  // namespace ics

// ==========================================================================================
// C ABI
// ==========================================================================================
using namespace ics;

namespace {

constexpr int kAtomScoreChunkSamples = 4096;       // samples (= workgroups) per launch
constexpr size_t kAtomScoreChunkAtoms = 32768;     // atoms of both sides per launch (at least one sample)
constexpr size_t kAtomScoreChunkVoxels = (size_t)1 << 24;   // voxels per launch of the volumes op (at least one sample)

struct Tallies { int64_t *matrix, *dist_q, *dist2_q, *dup, *shadowed, *hist, *totals; };

int tallies_check(const std::string& who, const Tallies& t) {
  ICS_CHECK(t.matrix && t.dist_q && t.dist2_q && t.dup && t.shadowed && t.hist && t.totals, who + ": null argument");
  return 0;
}
void tallies_out(const std::vector<unsigned long long>& host, int ncls, const Tallies& t) {
  const size_t KK = (size_t)(ncls + 1) * (ncls + 1);
  const unsigned long long* h = host.data();
  for (size_t i = 0; i < KK; ++i) t.matrix[i] = (int64_t)h[i];
  h += KK;
  for (int s = 0; s < ncls; ++s) {
    t.dist_q[s] = (int64_t)h[s]; t.dist2_q[s] = (int64_t)h[ncls + s];
    t.dup[s] = (int64_t)h[2 * ncls + s]; t.shadowed[s] = (int64_t)h[3 * ncls + s];
  }
  h += 4 * (size_t)ncls;
  for (int k = 0; k < kAtomScoreHistBins; ++k) t.hist[k] = (int64_t)h[k];
  for (int k = 0; k < kAtomScoreTotals; ++k) t.totals[k] = (int64_t)h[kAtomScoreHistBins + k];
}

int check_atoms(const double* xyz, const int32_t* species, const int32_t* off, int batch, int ncls, const char* name) {
  const std::string w = std::string("ics_op_atom_score: ");
  ICS_CHECK(off[0] == 0, w + name + "_off[0] must be 0");
  for (int s = 0; s < batch; ++s) {
    const long long n = (long long)off[s + 1] - off[s];
    ICS_CHECK(n >= 0, w + name + "_off decreases at sample " + std::to_string(s));
    ICS_CHECK(n <= kAtomScoreMaxAtoms, w + "sample " + std::to_string(s) + " has " + std::to_string(n) + " atoms in " + name +
                                           ", above the limit of " + std::to_string(kAtomScoreMaxAtoms));
  }
  ICS_CHECK((xyz != nullptr && species != nullptr) || off[batch] == 0, w + "null " + name + "_xyz or " + name + "_species");
  for (int s = 0; s < batch; ++s)
    for (long long a = off[s]; a < off[s + 1]; ++a) {
      ICS_CHECK(species[a] >= 0 && species[a] < ncls,
                w + "sample " + std::to_string(s) + " has a species outside [0, num_classes) in " + name);
      for (int k = 0; k < 3; ++k)
        ICS_CHECK(std::isfinite(xyz[3 * a + k]) && std::fabs(xyz[3 * a + k]) <= kAtomScoreMaxCoord,
                  w + "sample " + std::to_string(s) + " has a non-finite or out-of-range (> 1e150) coordinate in " + name);
    }
  return 0;
}

}  // namespace

extern "C" {

int ics_op_atom_score(const double* t_xyz, const int32_t* t_species, const int32_t* t_off, const double* p_xyz,
                      const int32_t* p_species, const int32_t* p_off, int batch, int ncls, double tol, int64_t* matrix,
                      int64_t* dist_q, int64_t* dist2_q, int64_t* dup, int64_t* shadowed, int64_t* hist, int64_t* totals,
                      int32_t* match, int32_t* sample_stats, double* dist_sum) {
  const std::string who = "ics_op_atom_score";
  const Tallies tl{matrix, dist_q, dist2_q, dup, shadowed, hist, totals};
  ICS_CHECK(batch >= 1, who + ": batch must be >= 1");
  ICS_CHECK(t_off && p_off, who + ": null argument");
  ICS_TRY(tallies_check(who, tl));
  double tol2, hist_scale;
  ICS_TRY(atom_score_params(who, ncls, tol, &tol2, &hist_scale));
  ICS_TRY(check_atoms(t_xyz, t_species, t_off, batch, ncls, "t"));
  ICS_TRY(check_atoms(p_xyz, p_species, p_off, batch, ncls, "p"));
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  const size_t len = atom_acc_len(ncls);
  // the accumulator lives in a block of its own for the whole call; the chunks' segments come and go behind it
  std::vector<int> to, po;
  std::vector<unsigned long long> host(len, 0ull), part(len);
  for (int s0 = 0; s0 < batch;) {
    int s1 = s0, cap = 0;
    size_t atoms = 0;
    while (s1 < batch && s1 - s0 < kAtomScoreChunkSamples) {
      const int n = t_off[s1 + 1] - t_off[s1], m = p_off[s1 + 1] - p_off[s1];
      if (s1 > s0 && atoms + n + m > kAtomScoreChunkAtoms) break;
      atoms += (size_t)n + m;
      cap = std::max(cap, std::max(n, m));
      ++s1;
    }
    const int nb = s1 - s0;
    const int T0 = t_off[s0], NT = t_off[s1] - T0, P0 = p_off[s0], NP = p_off[s1] - P0;
    to.resize(nb + 1); po.resize(nb + 1);
    for (int k = 0; k <= nb; ++k) { to[k] = t_off[s0 + k] - T0; po[k] = p_off[s0 + k] - P0; }
    Layout L;
    const auto s_acc = L.add<unsigned long long>(len);
    const auto s_tx = L.add<double>(3 * (size_t)NT + 1), s_px = L.add<double>(3 * (size_t)NP + 1);   // one spare: never empty
    const auto s_ts = L.add<int>((size_t)NT + 1), s_ps = L.add<int>((size_t)NP + 1);
    const auto s_to = L.add<int>(nb + 1), s_po = L.add<int>(nb + 1);
    const auto s_match = L.add<int>(match ? (size_t)NT + 1 : 0);
    const auto s_stats = L.add<int>(sample_stats ? (size_t)nb * 6 : 0);
    const auto s_sum = L.add<double>(dist_sum ? (size_t)nb : 0);
    unsigned long long* d_acc;
    double *d_tx, *d_px, *d_sum;
    int *d_ts, *d_ps, *d_to, *d_po, *d_match, *d_stats;
    ICS_TRY(L.reserve(s_acc, &d_acc, s_tx, &d_tx, s_px, &d_px, s_ts, &d_ts, s_ps, &d_ps, s_to, &d_to, s_po, &d_po, s_match,
                      &d_match, s_stats, &d_stats, s_sum, &d_sum));
    ICS_TRY(L.fill(s_acc, 0, len, st));
    ICS_TRY(L.upload(s_tx, t_xyz ? t_xyz + 3 * (size_t)T0 : nullptr, 3 * (size_t)NT, st));
    ICS_TRY(L.upload(s_px, p_xyz ? p_xyz + 3 * (size_t)P0 : nullptr, 3 * (size_t)NP, st));
    ICS_TRY(L.upload(s_ts, t_species ? t_species + T0 : nullptr, (size_t)NT, st));
    ICS_TRY(L.upload(s_ps, p_species ? p_species + P0 : nullptr, (size_t)NP, st));
    ICS_TRY(L.upload(s_to, to.data(), nb + 1, st));
    ICS_TRY(L.upload(s_po, po.data(), nb + 1, st));
    ICS_TRY(launch_atom_score_ragged(st, d_tx, d_ts, d_to, d_px, d_ps, d_po, nb, ncls, tol2, hist_scale, cap,
                                     AtomScoreOut{d_acc, d_match, d_stats, d_sum}));
    ICS_TRY(L.download(part.data(), s_acc, len, st));
    if (match) ICS_TRY(L.download(match + T0, s_match, (size_t)NT, st));
    if (sample_stats) ICS_TRY(L.download(sample_stats + (size_t)s0 * 6, s_stats, (size_t)nb * 6, st));
    if (dist_sum) ICS_TRY(L.download(dist_sum + s0, s_sum, (size_t)nb, st));
    ICS_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i < len; ++i) host[i] += part[i];
    s0 = s1;
  }
  tallies_out(host, ncls, tl);
  return 0;
}

int ics_op_atom_score_volumes(const uint8_t* true_labels, const uint8_t* pred_species, const uint8_t* pred_mask, int batch,
                              int d, int min_voxels, int max_atoms, int ncls, double tol, int64_t* matrix, int64_t* dist_q,
                              int64_t* dist2_q, int64_t* dup, int64_t* shadowed, int64_t* hist, int64_t* totals,
                              int32_t* match, int32_t* sample_stats, double* dist_sum) {
  const std::string who = "ics_op_atom_score_volumes";
  const Tallies tl{matrix, dist_q, dist2_q, dup, shadowed, hist, totals};
  ICS_CHECK(true_labels && pred_species && pred_mask, who + ": null argument");
  ICS_TRY(tallies_check(who, tl));
  ICS_CHECK(batch >= 1, who + ": batch must be >= 1");
  ICS_CHECK(d >= 2 && d <= 256 && (d & (d - 1)) == 0, who + ": grid must be a power of two in [2, 256]");
  ICS_CHECK(min_voxels >= 0, who + ": min_voxels must be >= 0");
  ICS_CHECK(max_atoms >= 1 && max_atoms <= kAtomScoreMaxAtoms, who + ": max_atoms must be in [1, 1024]");
  double tol2, hist_scale;
  ICS_TRY(atom_score_params(who, ncls, tol, &tol2, &hist_scale));
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  // The segmentation takes grids from 16 up: a smaller one is laid into the corner of a zeroed 16^3 grid, which changes
  // neither its components nor their coordinates.
  const int dd = d < 16 ? 16 : d;
  const size_t vox = (size_t)d * d * d, vv = (size_t)dd * dd * dd;
  const int per = (int)std::max<size_t>(1, std::min<size_t>((size_t)batch, kAtomScoreChunkVoxels / vv));
  const size_t len = atom_acc_len(ncls);
  std::vector<unsigned long long> host(len, 0ull), part(len);
  std::vector<unsigned char> pad;
  const size_t wsb = segment_workspace_bytes(per, dd, max_atoms, ncls);
  Layout L;
  const auto s_acc = L.add<unsigned long long>(len);
  const auto s_lab = L.add<unsigned char>(per * vv), s_sp = L.add<unsigned char>(per * vv), s_mk = L.add<unsigned char>(per * vv);
  const auto s_wt = L.add<unsigned char>(wsb), s_wp = L.add<unsigned char>(wsb);
  const auto s_match = L.add<int>(match ? (size_t)per * max_atoms : 0);
  const auto s_stats = L.add<int>(sample_stats ? (size_t)per * 6 : 0);
  const auto s_sum = L.add<double>(dist_sum ? (size_t)per : 0);
  unsigned long long* d_acc;
  unsigned char *d_lab, *d_sp, *d_mk, *d_wt, *d_wp;
  int *d_match, *d_stats;
  double* d_sum;
  ICS_TRY(L.reserve(s_acc, &d_acc, s_lab, &d_lab, s_sp, &d_sp, s_mk, &d_mk, s_wt, &d_wt, s_wp, &d_wp, s_match, &d_match,
                    s_stats, &d_stats, s_sum, &d_sum));
  auto up = [&](const Seg<unsigned char>& seg, const uint8_t* src, int nb) -> int {
    if (dd == d) return L.upload(seg, src, (size_t)nb * vox, st);
    pad.assign((size_t)nb * vv, 0);
    for (int b = 0; b < nb; ++b)
      for (int z = 0; z < d; ++z)
        for (int y = 0; y < d; ++y)
          std::copy(src + b * vox + ((size_t)z * d + y) * d, src + b * vox + ((size_t)z * d + y) * d + d,
                    pad.begin() + b * vv + ((size_t)z * dd + y) * dd);
    ICS_TRY(L.upload(seg, pad.data(), (size_t)nb * vv, st));
    ICS_HIP(hipStreamSynchronize(st));          // pad is reused by the next volume
    return 0;
  };
  for (int s0 = 0; s0 < batch; s0 += per) {
    const int nb = std::min(per, batch - s0);
    ICS_TRY(L.fill(s_acc, 0, len, st));
    ICS_TRY(up(s_lab, true_labels + (size_t)s0 * vox, nb));
    ICS_TRY(up(s_sp, pred_species + (size_t)s0 * vox, nb));
    ICS_TRY(up(s_mk, pred_mask + (size_t)s0 * vox, nb));
    int *ct, *stt, *cp, *stp;
    ICS_TRY(launch_segment_atoms(st, d_mk, d_sp, nb, dd, min_voxels, max_atoms, ncls, d_wp, wsb, nullptr, &cp, &stp));
    ICS_TRY(launch_segment_atoms(st, d_lab, d_lab, nb, dd, 0, max_atoms, ncls, d_wt, wsb, nullptr, &ct, &stt));
    ICS_TRY(launch_atom_score_stats(st, stt, ct, stp, cp, nb, max_atoms, ncls, tol2, hist_scale,
                                    AtomScoreOut{d_acc, d_match, d_stats, d_sum}));
    ICS_TRY(L.download(part.data(), s_acc, len, st));
    if (match) ICS_TRY(L.download(match + (size_t)s0 * max_atoms, s_match, (size_t)nb * max_atoms, st));
    if (sample_stats) ICS_TRY(L.download(sample_stats + (size_t)s0 * 6, s_stats, (size_t)nb * 6, st));
    if (dist_sum) ICS_TRY(L.download(dist_sum + s0, s_sum, (size_t)nb, st));
    ICS_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i < len; ++i) host[i] += part[i];
  }
  tallies_out(host, ncls, tl);
  return 0;
}

int ics_op_atom_score_limits(int* threads, int* max_atoms, int* chunk_samples, int* chunk_atoms) {
  ICS_CHECK(threads && max_atoms && chunk_samples && chunk_atoms, "ics_op_atom_score_limits: null argument");
  *threads = kAtomScoreThreads; *max_atoms = kAtomScoreMaxAtoms;
  *chunk_samples = kAtomScoreChunkSamples; *chunk_atoms = (int)kAtomScoreChunkAtoms;
  return 0;
}

}  // extern "C"
