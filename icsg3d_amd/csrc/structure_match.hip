// Structure matching for generate.py's results: which written samples are the same crystal as an earlier sample of the
// run, and which are a structure of the training set.  The predicate is the project's own (include/icsg3d.h states it in
// full; no parity with pymatgen's StructureMatcher is claimed): A and B match when some admissible signed axis
// permutation P and some anchor atom j of B map every atom of A onto its own atom of B within tol after the common
// shift is taken out.  Everything per atom runs in the kernel, in fp64.
//
// Host: the eligible structures are ordered by composition key (atom count, then the sorted species list), queries before
// references inside a bucket, each in index order.  A query at slot s of bucket [b0, b1) with references from r0 has the
// partners  k < s - b0: (A = b0 + k, B = s)  and then  (A = s, B = r0 + k - (s - b0)); a 64-bit prefix sum of the partner
// counts over the sorted queries numbers all pairs, and the device finds a pair's query by bisection of that prefix: no
// pair list is uploaded.  Structures of up to 64 atoms sort first, so pair numbers below a boundary go to the wave kernel
// (four pairs per 256-thread workgroup) and the rest to the workgroup kernel (one pair per 256 threads).
// Kernel: A and B of a compared pair have the same sorted species list, so thread k owns A's k-th sorted atom and scans
// the run of its species in B; the scan and the test of one (op, anchor) combination are structure_map.h's, shared with
// structure_symmetry.hip.  The (op, anchor) loop is uniform over the owning wave / workgroup and keeps the best
// (rms, op, anchor).  Pair results of a chunk are reduced per query by a second kernel (one wave per query) into a
// per-query state that is merged by key -- (partner) for duplicates, (rms, partner) for references -- so neither the
// chunking nor any arrival order shows in the result.
#include "structure_map.h"
#include "../../include/icsg3d.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <limits>

namespace ics {
namespace {

constexpr int kMatchOps = 48;
constexpr long long kMatchChunkPairs = 1 << 20;        // pair results per chunk: 16 B each
constexpr size_t kMatchTableBudget = (size_t)1 << 31;  // resident structure tables
constexpr int kCell = 16;                              // doubles per structure: M[9], G[6] (00 01 02 11 12 22), pad
constexpr int kStateI = 6;                             // ints per query: dup k, op, anchor; ref k, op, anchor

long long chunk_pairs() {
  static const long long v = env_cap("ICSG3D_MATCH_CHUNK_PAIRS", kMatchChunkPairs);
  return v;
}

__device__ __forceinline__ double sel3(double a, double b, double c, int i) { return i == 0 ? a : (i == 1 ? b : c); }
// entry (k, l) of the symmetric matrix stored as 00 01 02 11 12 22
__device__ __forceinline__ double sym3(const double* g, int k, int l) {
  const int lo = min(k, l), hi = max(k, l);
  return g[lo == 0 ? hi : (lo == 1 ? 2 + hi : 5)];
}

template <int G>
__global__ __launch_bounds__(256) void structure_match_kernel(
    long long p0, int npairs, const long long* __restrict__ pref, int nqs, const int4* __restrict__ qrec,
    const int4* __restrict__ sinfo, const double* __restrict__ scell, const double* __restrict__ afrac,
    const int* __restrict__ aperm, const int* __restrict__ arun, const int* __restrict__ ops, int nops, double tol,
    double ltol, double* __restrict__ res_rms, int2* __restrict__ res_oa) {
  constexpr int NT = 256, NG = NT / G, NW = G / 64;
  __shared__ double fa[NG][3][G], fb[NG][3][G];
  __shared__ int mark[NG][G], bidx[NG][G];
  __shared__ double red[2][NW][4];
  const int tid = threadIdx.x, grp = tid / G, gt = tid % G, lane = gt & 63, wave = gt >> 6;
  const int slot = blockIdx.x * NG + grp;
  const bool active = slot < npairs;

  int sa = 0, sb = 0, n = 0, oa = 0, ob = 0, alo = 0, ahi = 0;
  if (active) {
    const long long p = p0 + slot;
    int lo = 0, hi = nqs;                         // the last query whose first pair is <= p
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (pref[mid] <= p) lo = mid; else hi = mid;
    }
    const int4 r = qrec[lo];
    const int k = (int)(p - pref[lo]), ne = r.x - r.y;
    if (k < ne) { sa = r.y + k; sb = r.x; } else { sa = r.x; sb = r.z + (k - ne); }
    const int4 ia = sinfo[sa], ib = sinfo[sb];
    oa = ia.x; ob = ib.x; n = ia.y; alo = ia.z; ahi = ia.w;
  }
  const bool have = gt < n;
  int rlo = 0, rhi = 0;
  if (have) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double x = afrac[3 * (size_t)(oa + gt) + c], y = afrac[3 * (size_t)(ob + gt) + c];
      fa[grp][c][gt] = x - floor(x);
      fb[grp][c][gt] = y - floor(y);
    }
    bidx[grp][gt] = aperm[ob + gt];
    mark[grp][gt] = 0;
    const int run = arun[oa + gt];
    rlo = run & 0xffff; rhi = run >> 16;
  }
  __syncthreads();

  double mb[9], ga[6], gb[6];
#pragma unroll
  for (int k = 0; k < 9; ++k) mb[k] = active ? scell[(size_t)kCell * sb + k] : 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    ga[k] = active ? scell[(size_t)kCell * sa + 9 + k] : 0.0;
    gb[k] = active ? scell[(size_t)kCell * sb + 9 + k] : 0.0;
  }
  const double ax = have ? fa[grp][0][gt] : 0.0, ay = have ? fa[grp][1][gt] : 0.0, az = have ? fa[grp][2][gt] : 0.0;
  const double a0x = active ? fa[grp][0][alo] : 0.0, a0y = active ? fa[grp][1][alo] : 0.0,
               a0z = active ? fa[grp][2][alo] : 0.0;
  const double kInf = __builtin_inf();
  const double dn = (double)n;

  double best = kInf;
  int best_op = -1, best_anchor = -1, ph = 0;
  const int nloop = active ? nops : 0;
  for (int o = 0; o < nloop; ++o) {
    const int code = ops[o];
    const int p0k = code & 3, p1k = (code >> 2) & 3, p2k = (code >> 4) & 3;
    const double s0 = (code >> 6) & 1 ? -1.0 : 1.0, s1 = (code >> 7) & 1 ? -1.0 : 1.0, s2 = (code >> 8) & 1 ? -1.0 : 1.0;
    // admissible: |(P G_A P^T)_kl - G_B,kl| <= ltol sqrt(G_B,kk G_B,ll)
    const int pk[3] = {p0k, p1k, p2k};
    const double sk[3] = {s0, s1, s2};
    const double dg[3] = {gb[0], gb[3], gb[5]};
    bool adm = true;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int l = k; l < 3; ++l) {
        const double gp = sk[k] * sk[l] * sym3(ga, pk[k], pk[l]);
        const double gbkl = gb[k == 0 ? l : (k == 1 ? 2 + l : 5)];
        adm = adm && (fabs(gp - gbkl) <= ltol * sqrt(dg[k] * dg[l]));
      }
    if (!adm) continue;                                           // uniform: the cells are the pair's
    const double qx = s0 * sel3(ax, ay, az, p0k), qy = s1 * sel3(ax, ay, az, p1k), qz = s2 * sel3(ax, ay, az, p2k);
    const double px = s0 * sel3(a0x, a0y, a0z, p0k), py = s1 * sel3(a0x, a0y, a0z, p1k),
                 pz = s2 * sel3(a0x, a0y, a0z, p2k);
    for (int js = alo; js < ahi; ++js) {
      const double tx = fb[grp][0][js] - px, ty = fb[grp][1][js] - py, tz = fb[grp][2][js] - pz;
      double bd2, ux, uy, uz, rms, sx, sy, sz;
      const int br = nearest_in_run(fb[grp][0], fb[grp][1], fb[grp][2], rlo, rhi, qx + tx, qy + ty, qz + tz, mb, bd2, ux,
                                    uy, uz);
      const int tag = o * kMapMaxAtoms + (js - alo) + 1;
      if (map_test<NW>(have, br, bd2, ux, uy, uz, tol, tag, mark[grp], dn, red, ph, wave, lane, rms, sx, sy, sz) &&
          rms < best) {
        best = rms; best_op = o; best_anchor = bidx[grp][js];
      }
    }
  }
  if (active && gt == 0) {
    res_rms[slot] = best;
    res_oa[slot] = make_int2(best_op, best_anchor);
  }
}

// One wave per sorted query of the chunk: its pair results into the per-query state, merged by key.
__global__ __launch_bounds__(256) void structure_match_reduce_kernel(
    long long c0, int npairs, int q0, int nq, const long long* __restrict__ pref, const int4* __restrict__ qrec,
    const double* __restrict__ res_rms, const int2* __restrict__ res_oa, double* __restrict__ st_d,
    int* __restrict__ st_i) {
  const int w = (int)((blockIdx.x * (unsigned)blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (w >= nq) return;
  const int qi = q0 + w;
  const long long first = pref[qi];
  const long long last = pref[qi + 1], lo = first > c0 ? first : c0, hi = last < c0 + npairs ? last : c0 + npairs;
  const int4 r = qrec[qi];
  const int ne = r.x - r.y;
  const double kInf = __builtin_inf();
  int dk = INT_MAX, dop = -1, dan = -1, rk = INT_MAX, rop = -1, ran = -1;
  double drms = kInf, rrms = kInf;
  for (long long p = lo + lane; p < hi; p += 64) {
    const double v = res_rms[p - c0];
    if (!(v < kInf)) continue;
    const int2 oa = res_oa[p - c0];
    const int k = (int)(p - first);
    if (k < ne) {
      if (k < dk) { dk = k; drms = v; dop = oa.x; dan = oa.y; }
    } else if (v < rrms || (v == rrms && k < rk)) { rk = k; rrms = v; rop = oa.x; ran = oa.y; }
  }
  int dmin = dk, kmin = rk;
  double vmin = rrms;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    dmin = min(dmin, __shfl_xor(dmin, o, 64));
    const double ov = __shfl_xor(vmin, o, 64);
    const int ok = __shfl_xor(kmin, o, 64);
    if (ov < vmin || (ov == vmin && ok < kmin)) { vmin = ov; kmin = ok; }
  }
  if (dk == dmin && dk != INT_MAX && dk < st_i[(size_t)kStateI * qi]) {            // partner numbers are distinct: one lane
    st_i[(size_t)kStateI * qi] = dk; st_i[(size_t)kStateI * qi + 1] = dop; st_i[(size_t)kStateI * qi + 2] = dan;
    st_d[2 * (size_t)qi] = drms;
  }
  if (rk == kmin && rk != INT_MAX) {
    const double sv = st_d[2 * (size_t)qi + 1];
    const int sk = st_i[(size_t)kStateI * qi + 3];
    if (rrms < sv || (rrms == sv && rk < sk)) {
      st_i[(size_t)kStateI * qi + 3] = rk; st_i[(size_t)kStateI * qi + 4] = rop; st_i[(size_t)kStateI * qi + 5] = ran;
      st_d[2 * (size_t)qi + 1] = rrms;
    }
  }
}

template <int G>
int launch_match(hipStream_t st, long long p0, int npairs, const long long* pref, int nqs, const int4* qrec,
                 const int4* sinfo, const double* scell, const double* afrac, const int* aperm, const int* arun,
                 const int* ops, int nops, double tol, double ltol, double* res_rms, int2* res_oa) {
  constexpr int NG = 256 / G;
  ICS_LAUNCH(structure_match_kernel<G>, dim3((unsigned)((npairs + NG - 1) / NG)), dim3(256), 0, st, p0, npairs, pref, nqs,
             qrec, sinfo, scell, afrac, aperm, arun, ops, nops, tol, ltol, res_rms, res_oa);
  ICS_HIP(hipGetLastError());
  return 0;
}

// The op list of `ops_mode` (0..2): perm[k][3], sign[k][3] with f'_k = sign_k f[perm_k]; returns the count (1, 24, 48).
// Order: lexicographic over (permutation, sign pattern) -- permutations (0,1,2) (0,2,1) (1,0,2) (1,2,0) (2,0,1) (2,1,0), and
// per permutation the sign patterns (+,+,+) (+,+,-) (+,-,+) (+,-,-) (-,+,+) (-,+,-) (-,-,+) (-,-,-).  Index 0 is the
// identity.  ops_mode 0 keeps index 0, ops_mode 1 the 24 of determinant +1 in that order, ops_mode 2 all 48; a reported
// `op` indexes the mode's own list.
int structure_match_ops(int ops_mode, int perm[][3], int sign[][3]) {
  static const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  static const int parity[6] = {1, -1, -1, 1, 1, -1};
  int n = 0;
  for (int p = 0; p < 6; ++p)
    for (int s = 0; s < 8; ++s) {
      const int sg[3] = {s & 4 ? -1 : 1, s & 2 ? -1 : 1, s & 1 ? -1 : 1};
      const int det = parity[p] * sg[0] * sg[1] * sg[2];
      if ((ops_mode == 0 && (p || s)) || (ops_mode == 1 && det != 1)) continue;
      for (int k = 0; k < 3; ++k) { perm[n][k] = perms[p][k]; sign[n][k] = sg[k]; }
      ++n;
    }
  return n;
}

// The argument rules of ics_op_structure_match for its inputs, every structure checked before anything is written: 0, or
// -1 with the error set naming the structure.
int structure_match_check(const int32_t* offsets, const int32_t* species, const double* frac, const double* lattice,
                          const int32_t* eligible, int nq, int nref, double tol, double ltol, int ops_mode) {
  const std::string op = "ics_op_structure_match: ";
  ICS_CHECK(nq >= 1, op + "nq must be >= 1");
  ICS_CHECK(nref >= 0, op + "nref must be >= 0");
  ICS_CHECK((long long)nq + nref <= INT_MAX - 1, op + "too many structures");
  ICS_CHECK(offsets && lattice && eligible, op + "null argument");
  ICS_CHECK(std::isfinite(tol) && tol > 0.0, op + "tol must be finite and > 0");
  ICS_CHECK(std::isfinite(ltol) && ltol > 0.0, op + "ltol must be finite and > 0");
  ICS_CHECK(ops_mode >= 0 && ops_mode <= 2, op + "ops_mode must be 0 (identity), 1 (rotations) or 2 (all 48)");
  return check_structures(op, offsets, species, frac, lattice, eligible, nq + nref, tol);
}

}  // namespace
}  // namespace ics

using namespace ics;

// Structures ordered by composition key on the host, pairs enumerated on the device from the bucket ranges, pair results
// chunked under kMatchChunkPairs (ICSG3D_MATCH_CHUNK_PAIRS shrinks it); synchronous on the calling thread's stream.
extern "C" int ics_op_structure_match(const int32_t* offsets, const int32_t* species, const double* frac,
                                      const double* lattice, const int32_t* eligible, int nq, int nref, double tol,
                                      double ltol, int ops_mode, int32_t* dup_of, double* dup_rms, int32_t* dup_op,
                                      int32_t* ref_of, double* ref_rms, int32_t* ref_op, int32_t* n_cmp) {
  ICS_TRY(structure_match_check(offsets, species, frac, lattice, eligible, nq, nref, tol, ltol, ops_mode));
  ICS_CHECK(dup_of && dup_rms && dup_op && ref_of && ref_rms && ref_op && n_cmp, "ics_op_structure_match: null output");
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  const int ns = nq + nref;
  const double kInf = std::numeric_limits<double>::infinity();
  for (int q = 0; q < nq; ++q) {
    dup_of[q] = ref_of[q] = -1;
    dup_rms[q] = ref_rms[q] = kInf;
    dup_op[2 * q] = dup_op[2 * q + 1] = ref_op[2 * q] = ref_op[2 * q + 1] = -1;
    n_cmp[2 * q] = n_cmp[2 * q + 1] = 0;
  }
  // ---- composition keys: per eligible structure its atoms sorted by (species, index)
  std::vector<int> order;
  for (int s = 0; s < ns; ++s)
    if (eligible[s]) order.push_back(s);
  const int ne = (int)order.size();
  if (ne == 0) return 0;
  const size_t natoms_all = (size_t)offsets[ns];
  // at the structure's own offsets: sorted atom -> atom, its species, its run word; per structure the anchor run
  std::vector<int> sperm(natoms_all), sz(natoms_all), srun(natoms_all), anchor(2 * (size_t)ns);
  for (int s : order) {
    const int a0 = offsets[s];
    sort_atoms(species + a0, offsets[s + 1] - a0, sperm.data() + a0, sz.data() + a0, srun.data() + a0, &anchor[2 * s],
               &anchor[2 * s + 1]);
  }
  auto key_cmp = [&](int a, int b) {   // <0, 0, >0 on (atom count, sorted species)
    const int na = offsets[a + 1] - offsets[a], nb = offsets[b + 1] - offsets[b];
    if (na != nb) return na < nb ? -1 : 1;
    const int* za = sz.data() + offsets[a]; const int* zb = sz.data() + offsets[b];
    for (int k = 0; k < na; ++k)
      if (za[k] != zb[k]) return za[k] < zb[k] ? -1 : 1;
    return 0;
  };
  std::sort(order.begin(), order.end(), [&](int a, int b) { const int c = key_cmp(a, b); return c ? c < 0 : a < b; });

  // ---- buckets, sorted queries and the pair prefix
  std::vector<int> qrec;          // per sorted query: slot, b0, r0, r1
  std::vector<long long> pref(1, 0);
  long long psmall = 0;           // pairs of structures of up to kMapSmall atoms come first
  for (int b0 = 0; b0 < ne;) {
    int b1 = b0 + 1;
    while (b1 < ne && key_cmp(order[b0], order[b1]) == 0) ++b1;
    int r0 = b0;
    while (r0 < b1 && order[r0] < nq) ++r0;
    for (int s = b0; s < r0; ++s) {
      const int q = order[s];
      n_cmp[2 * q] = s - b0; n_cmp[2 * q + 1] = b1 - r0;
      qrec.insert(qrec.end(), {s, b0, r0, b1});
      pref.push_back(pref.back() + (s - b0) + (b1 - r0));
    }
    if (offsets[order[b0] + 1] - offsets[order[b0]] <= kMapSmall) psmall = pref.back();
    b0 = b1;
  }
  const int nqs = (int)qrec.size() / 4;
  const long long ptotal = pref.back();
  if (nqs == 0 || ptotal == 0) return 0;

  // ---- tables
  size_t N = 0;
  for (int s : order) N += (size_t)(offsets[s + 1] - offsets[s]);
  int perm[kMatchOps][3], sign[kMatchOps][3];
  const int nops = structure_match_ops(ops_mode, perm, sign);
  const long long cp = std::min(chunk_pairs(), ptotal);
  Layout in(16);
  const auto i_cell = in.add<double>((size_t)ne * kCell), i_frac = in.add<double>(3 * N), i_std = in.add<double>(2 * (size_t)nqs);
  const auto i_pref = in.add<long long>(nqs + 1);
  const auto i_info = in.add<int4>(ne), i_qrec = in.add<int4>(nqs);
  const auto i_perm = in.add<int>(N), i_run = in.add<int>(N), i_ops = in.add<int>(kMatchOps);
  const auto i_sti = in.add<int>((size_t)nqs * kStateI);
  if (in.bytes() > kMatchTableBudget) {
    set_error("ics_op_structure_match: the structure tables (" + std::to_string(in.bytes()) + " bytes) exceed the device budget");
    return -1;
  }
  std::vector<unsigned char> hin(in.bytes(), 0);
  double *hc, *hf, *hsd;
  long long* hpref;
  int4 *hinfo, *hqrec;
  int *hperm, *hrun, *hops, *hsti;
  ICS_TRY(in.bind(hin.data(), hin.size(), i_cell, &hc, i_frac, &hf, i_std, &hsd, i_pref, &hpref, i_info, &hinfo,
                  i_qrec, &hqrec, i_perm, &hperm, i_run, &hrun, i_ops, &hops, i_sti, &hsti));
  size_t at = 0;
  for (int k = 0; k < ne; ++k) {
    const int s = order[k], a0 = offsets[s], n = offsets[s + 1] - a0;
    const double* M = lattice + 9 * (size_t)s;
    double* c = hc + (size_t)kCell * k;
    std::memcpy(c, M, 72);
    cell_gram(M, c + 9);
    std::memcpy(hperm + at, sperm.data() + a0, (size_t)n * 4);
    std::memcpy(hrun + at, srun.data() + a0, (size_t)n * 4);
    for (int i = 0; i < n; ++i) std::memcpy(hf + 3 * (at + i), frac + 3 * (size_t)(a0 + sperm[a0 + i]), 24);
    hinfo[k] = make_int4((int)at, n, anchor[2 * s], anchor[2 * s + 1]);
    at += n;
  }
  std::memcpy(hpref, pref.data(), (size_t)(nqs + 1) * 8);
  std::memcpy(hqrec, qrec.data(), (size_t)nqs * 16);
  for (int k = 0; k < nops; ++k)
    hops[k] = perm[k][0] | perm[k][1] << 2 | perm[k][2] << 4 | (sign[k][0] < 0) << 6 | (sign[k][1] < 0) << 7 |
              (sign[k][2] < 0) << 8;
  for (int k = 0; k < nqs; ++k) {
    hsd[2 * k] = hsd[2 * k + 1] = kInf;
    for (int i = 0; i < kStateI; ++i) hsti[kStateI * k + i] = i % 3 == 0 ? INT_MAX : -1;
  }

  Layout L;
  const auto s_in = L.add<unsigned char>(in.bytes());
  const auto s_rms = L.add<double>(cp);
  const auto s_oa = L.add<int2>(cp);
  unsigned char* din;
  double *dcell, *dfrac, *dstd, *drms;
  long long* dpref;
  int4 *dinfo, *dqrec;
  int *dperm, *drun, *dops, *dsti;
  int2* doa;
  ICS_TRY(L.reserve(s_in, &din, s_rms, &drms, s_oa, &doa));
  ICS_TRY(L.upload(s_in, hin.data(), in.bytes(), st));
  ICS_TRY(in.bind(din, s_in.count, i_cell, &dcell, i_frac, &dfrac, i_std, &dstd, i_pref, &dpref, i_info, &dinfo,
                  i_qrec, &dqrec, i_perm, &dperm, i_run, &drun, i_ops, &dops, i_sti, &dsti));

  for (long long c0 = 0; c0 < ptotal;) {
    // one chunk: pairs [c0, c1) of one kernel kind
    const long long lim = c0 < psmall ? psmall : ptotal;
    const long long c1 = std::min(c0 + cp, lim);
    const int np = (int)(c1 - c0);
    if (c0 < psmall)
      ICS_TRY((launch_match<64>(st, c0, np, dpref, nqs, dqrec, dinfo, dcell, dfrac, dperm, drun, dops, nops, tol, ltol,
                                drms, doa)));
    else
      ICS_TRY((launch_match<256>(st, c0, np, dpref, nqs, dqrec, dinfo, dcell, dfrac, dperm, drun, dops, nops, tol, ltol,
                                 drms, doa)));
    // the sorted queries with a pair in the chunk
    const int q0 = (int)(std::upper_bound(pref.begin(), pref.end(), c0) - pref.begin()) - 1;
    const int q1 = (int)(std::upper_bound(pref.begin(), pref.end(), c1 - 1) - pref.begin()) - 1;
    const int nqc = q1 - q0 + 1;
    ICS_LAUNCH(structure_match_reduce_kernel, dim3((unsigned)((nqc + 3) / 4)), dim3(256), 0, st, c0, np, q0, nqc, dpref,
               dqrec, drms, doa, dstd, dsti);
    ICS_HIP(hipGetLastError());
    c0 = c1;
  }
  std::vector<double> osd((size_t)nqs * 2);
  std::vector<int> osi((size_t)nqs * kStateI);
  ICS_TRY(in.download(osd.data(), i_std, osd.size(), st));
  ICS_TRY(in.download(osi.data(), i_sti, osi.size(), st));
  ICS_HIP(hipStreamSynchronize(st));
  for (int k = 0; k < nqs; ++k) {
    const int s = qrec[4 * k], b0 = qrec[4 * k + 1], r0 = qrec[4 * k + 2], r1 = qrec[4 * k + 3], q = order[s];
    const int* si = osi.data() + (size_t)kStateI * k;
    if (si[0] != INT_MAX) {
      if (si[0] < 0 || si[0] >= s - b0) { set_error("ics_op_structure_match: the device returned a partner out of range"); return -1; }
      dup_of[q] = order[b0 + si[0]]; dup_rms[q] = osd[2 * k]; dup_op[2 * q] = si[1]; dup_op[2 * q + 1] = si[2];
    }
    if (si[3] != INT_MAX) {
      const int kr = si[3] - (s - b0);
      if (kr < 0 || kr >= r1 - r0) { set_error("ics_op_structure_match: the device returned a partner out of range"); return -1; }
      ref_of[q] = order[r0 + kr] - nq; ref_rms[q] = osd[2 * k + 1]; ref_op[2 * q] = si[4]; ref_op[2 * q + 1] = si[5];
    }
  }
  return 0;
}
