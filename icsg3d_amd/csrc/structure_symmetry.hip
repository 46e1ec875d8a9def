// Symmetry of generate.py's structures: which operations (W, t) -- W an integer matrix the structure's own lattice admits,
// t a translation -- map the structure onto itself within tol, and the group they form.  The predicate is the project's
// own (include/icsg3d.h states it in full; no parity with spglib or pymatgen's SpacegroupAnalyzer is claimed).
//
// Host: the eligible structures are ordered by atom count (then index), their atoms by (species, index); one packed block
// is uploaded.  Structures of up to 64 atoms sort first, so a launch of the operation kernel is uniform.
// Stage 1 (sym_lattice_kernel, one workgroup per structure): all 3^9 codes in ascending order, 256 at a time; a thread
//   decodes its code, keeps determinant +-1 and tests W^T G W against G in fp64; the admissible codes are compacted in code
//   order by ballot + wave prefix + the four wave totals.
// Stage 2 (sym_ops_kernel<G>, unit = (structure, admissible W)): one wave (G = 64, four units per workgroup) or one
//   256-thread workgroup per unit, lane = atom in sorted order.  The scan of an atom's species run and the test of one
//   (W, anchor) combination are structure_map.h's, shared with structure_match.hip; the anchor loop is uniform over the
//   owning wave / workgroup.  Every (W, anchor) gets one entry of the candidate table (t*, rms or -1).  sym_scan_kernel
//   (one workgroup per structure) walks the table in (code, anchor) order and gives each passing combination its slot by
//   ballot + prefix, so the order of the operation list holds by construction; it also counts n_ops, n_point, n_trans
//   and the rotation types over ALL passing combinations.
// Stage 3 (sym_group_kernel, one workgroup per structure whose reason is still 0): recomputes nb_g per stored operation
//   (one byte per atom, kept in device memory for the closure test), sums the projection in operation order, tests
//   closure over all ordered pairs through a (lattice operation, anchor) -> slot table in LDS, then orbits,
//   multiplicities, sym_G, sym_shift and sym_resid.
// The candidate table, the maps and the operation lists are chunked over structures under a byte cap; no result depends
// on the chunking, and no floating-point atomic is used anywhere: the same bits run to run.
#include "structure_map.h"
#include "../../include/icsg3d.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <limits>

namespace ics {

constexpr int kSymLatCap = 64;         // admissible lattice operations kept per structure
constexpr int kSymMaxOpsLimit = 4096;  // largest max_ops accepted
constexpr int kSymCodes = 19683;       // 3^9 matrices with entries in {-1, 0, 1}
constexpr int kSymIdentityCode = 16484;

// code = sum_k (W[k/3][k%3] + 1) 3^(8-k)  ->  W, row-major
__host__ __device__ inline void sym_decode(int code, int w[9]) {
  for (int k = 8; k >= 0; --k) { w[k] = code % 3 - 1; code /= 3; }
}
__host__ __device__ inline int sym_det(const int w[9]) {
  return w[0] * (w[4] * w[8] - w[5] * w[7]) - w[1] * (w[3] * w[8] - w[5] * w[6]) + w[2] * (w[3] * w[7] - w[4] * w[6]);
}
// index into the rotation-type histogram (-6, -4, -3, -2, -1, 1, 2, 3, 4, 6), or -1 for a (det, trace) in no row of the table
__host__ __device__ inline int sym_type_index(const int w[9]) {
  const int det = sym_det(w), tr = w[0] + w[4] + w[8];
  if (det == 1) return tr == 3 ? 5 : (tr >= -1 && tr <= 2 ? 7 + tr : -1);
  if (det == -1) return tr == -3 ? 4 : (tr >= -2 && tr <= 1 ? 2 + tr : -1);
  return -1;
}

namespace {

constexpr size_t kSymChunkBytes = (size_t)256 << 20;   // candidate table + maps + operation lists of one chunk
constexpr size_t kSymTableBudget = (size_t)1 << 31;    // resident structure tables
constexpr int kCell = 24;     // doubles per structure: M[9], inv(M)[9], G[6] (00 01 02 11 12 22)
constexpr int kCounts = 16;   // ints per structure: n_ops, n_point, n_trans, reason, types[10], pad
constexpr int kOpBytes = 4 + 4 + 4 + 24 + 8;   // code, anchor, (slot | lattice op << 16), t*, rms

size_t chunk_bytes() {
  static const size_t v = (size_t)env_cap("ICSG3D_SYMMETRY_CHUNK_BYTES", (long long)kSymChunkBytes);
  return v;
}

// The maximum of v over a 256-thread workgroup, to every thread.
__device__ __forceinline__ double block_max(double v, double* red4, int tid) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((tid & 63) == 0) red4[tid >> 6] = v;
  __syncthreads();
  return fmax(fmax(red4[0], red4[1]), fmax(red4[2], red4[3]));
}

// W f for an integer matrix held as doubles
__device__ __forceinline__ void apply_w(const double* w, double x, double y, double z, double& ox, double& oy, double& oz) {
  ox = w[0] * x + w[1] * y + w[2] * z;
  oy = w[3] * x + w[4] * y + w[5] * z;
  oz = w[6] * x + w[7] * y + w[8] * z;
}

// ---------------------------------------------------------------- stage 1: the lattice operations
__global__ __launch_bounds__(256) void sym_lattice_kernel(const double* __restrict__ scell, double ltol,
                                                          int* __restrict__ nlat, int* __restrict__ latcode) {
  __shared__ int wtot[4];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* g6 = scell + (size_t)kCell * s + 18;
  const double g[3][3] = {{g6[0], g6[1], g6[2]}, {g6[1], g6[3], g6[4]}, {g6[2], g6[4], g6[5]}};
  double lim[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int l = 0; l < 3; ++l) lim[k][l] = ltol * sqrt(g[k][k] * g[l][l]);
  int run = 0;
  for (int base = 0; base < kSymCodes; base += 256) {
    const int code = base + tid;
    bool adm = false;
    if (code < kSymCodes) {
      int w[9];
      sym_decode(code, w);
      const int det = sym_det(w);
      if (det == 1 || det == -1) {
        adm = true;
        double gw[3][3];   // G W
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int l = 0; l < 3; ++l) gw[a][l] = g[a][0] * w[l] + g[a][1] * w[3 + l] + g[a][2] * w[6 + l];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
          for (int l = 0; l < 3; ++l) {
            const double v = w[k] * gw[0][l] + w[3 + k] * gw[1][l] + w[6 + k] * gw[2][l];   // (W^T G W)_kl
            adm = adm && (fabs(v - g[k][l]) <= lim[k][l]);
          }
      }
    }
    const unsigned long long b = __ballot(adm);
    if (lane == 0) wtot[wave] = __popcll(b);
    __syncthreads();
    int pos = run + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += wtot[w];
    if (adm && pos < kSymLatCap) latcode[(size_t)kSymLatCap * s + pos] = code;
    run += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
  }
  if (tid == 0) nlat[s] = run;
}

// ---------------------------------------------------------------- stage 2: the operations
// The second launch bound is the waves per SIMD the kernel has always had (96 and 108 VGPRs): the wave form sits one
// register off the step from 5 to 4, and the allocator is to stay on this side of it.
template <int G>
__global__ __launch_bounds__(256, G == 64 ? 5 : 4) void sym_ops_kernel(
    int s0, int nsc, const int4* __restrict__ sinfo, const double* __restrict__ scell, const double* __restrict__ afrac,
    const int* __restrict__ arun, const int* __restrict__ nlat, const int* __restrict__ latcode,
    const long long* __restrict__ candoff, double tol, double4* __restrict__ cand) {
  constexpr int NT = 256, NG = NT / G, NW = G / 64;
  __shared__ double fa[NG][3][G];
  __shared__ int mark[NG][G];
  __shared__ double red[2][NW][4];
  const int tid = threadIdx.x, grp = tid / G, gt = tid % G, lane = gt & 63, wave = gt >> 6;
  const int unit = blockIdx.x * NG + grp, sl = unit / kSymLatCap, l = unit % kSymLatCap;
  bool active = sl < nsc;
  const int s = s0 + (active ? sl : 0);
  int n = 0, oa = 0, alo = 0, ahi = 0, code = 0;
  if (active) {
    const int nl = nlat[s];
    active = nl <= kSymLatCap && l < nl;
  }
  if (active) {
    const int4 ia = sinfo[s];
    oa = ia.x; n = ia.y; alo = ia.z; ahi = ia.w;
    code = latcode[(size_t)kSymLatCap * s + l];
  }
  const bool have = gt < n;
  int rlo = 0, rhi = 0;
  if (have) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double x = afrac[3 * (size_t)(oa + gt) + c];
      fa[grp][c][gt] = x - floor(x);
    }
    const int run = arun[oa + gt];
    rlo = run & 0xffff; rhi = run >> 16;
  }
  mark[grp][gt] = 0;
  __syncthreads();

  double m[9], mi[9], w[9];
  int wi[9];
  sym_decode(code, wi);
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    m[k] = active ? scell[(size_t)kCell * s + k] : 0.0;
    mi[k] = active ? scell[(size_t)kCell * s + 9 + k] : 0.0;
    w[k] = (double)wi[k];
  }
  const double ax = have ? fa[grp][0][gt] : 0.0, ay = have ? fa[grp][1][gt] : 0.0, az = have ? fa[grp][2][gt] : 0.0;
  double qx, qy, qz, px, py, pz;
  apply_w(w, ax, ay, az, qx, qy, qz);
  apply_w(w, active ? fa[grp][0][alo] : 0.0, active ? fa[grp][1][alo] : 0.0, active ? fa[grp][2][alo] : 0.0, px, py, pz);
  const double dn = (double)n;
  const int na = ahi - alo;
  double4* out = cand + (active ? candoff[s] - candoff[s0] + (long long)l * na : 0);
  int ph = 0;
  for (int a = 0; a < na; ++a) {            // na = 0 for an idle group
    const int js = alo + a;
    const double tx = fa[grp][0][js] - px, ty = fa[grp][1][js] - py, tz = fa[grp][2][js] - pz;
    double bd2, ux, uy, uz, rms, sx, sy, sz;
    const int br = nearest_in_run(fa[grp][0], fa[grp][1], fa[grp][2], rlo, rhi, qx + tx, qy + ty, qz + tz, m, bd2, ux, uy, uz);
    map_test<NW>(have, br, bd2, ux, uy, uz, tol, a + 1, mark[grp], dn, red, ph, wave, lane, rms, sx, sy, sz);
    if (gt == 0) {
      // t* = t + inv(M)^T ubar; a combination that failed leaves rms = -1 and a t* nobody reads
      const double t0 = tx + (sx * mi[0] + sy * mi[3] + sz * mi[6]), t1 = ty + (sx * mi[1] + sy * mi[4] + sz * mi[7]),
                   t2 = tz + (sx * mi[2] + sy * mi[5] + sz * mi[8]);
      out[a] = make_double4(t0 - floor(t0), t1 - floor(t1), t2 - floor(t2), rms);
    }
  }
}

// One workgroup per structure: the candidate table in (lattice operation, anchor) order -> slots, counts, types.
__global__ __launch_bounds__(256) void sym_scan_kernel(int s0, const int4* __restrict__ sinfo, const int* __restrict__ aperm,
                                                       const int* __restrict__ nlat, const int* __restrict__ latcode,
                                                       const long long* __restrict__ candoff,
                                                       const double4* __restrict__ cand, int max_ops, int* __restrict__ counts,
                                                       int* __restrict__ op_code, int* __restrict__ op_anchor,
                                                       int* __restrict__ op_slot, double* __restrict__ op_t,
                                                       double* __restrict__ op_rms) {
  __shared__ int wtot[4], wtr[4], lflag[kSymLatCap];
  const int sl = blockIdx.x, s = s0 + sl, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int4 ia = sinfo[s];
  const int alo = ia.z, na = ia.w - ia.z, nl = nlat[s];
  int* cnt = counts + (size_t)kCounts * s;
  if (nl > kSymLatCap) {                                   // uniform
    if (tid < kCounts) cnt[tid] = tid == 3 ? 2 : 0;
    return;
  }
  if (tid < kSymLatCap) lflag[tid] = 0;
  __syncthreads();
  const double4* in = cand + (candoff[s] - candoff[s0]);
  const size_t ob = (size_t)sl * max_ops;
  const int total = nl * na;
  int run = 0, ntr = 0;
  for (int base = 0; base < total; base += 256) {
    const int e = base + tid;
    double4 v = make_double4(0.0, 0.0, 0.0, -1.0);
    int l = 0, code = -1;
    if (e < total) {
      v = in[e];
      l = e / na;
      code = latcode[(size_t)kSymLatCap * s + l];
    }
    const bool pass = v.w >= 0.0;
    const unsigned long long b = __ballot(pass), bt = __ballot(pass && code == kSymIdentityCode);
    if (lane == 0) { wtot[wave] = __popcll(b); wtr[wave] = __popcll(bt); }
    __syncthreads();
    int pos = run + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += wtot[w];
    if (pass) {
      lflag[l] = 1;
      if (pos < max_ops) {
        const int a = e - l * na;
        op_code[ob + pos] = code;
        op_anchor[ob + pos] = aperm[ia.x + alo + a];
        op_slot[ob + pos] = (alo + a) | (l << 16);
        op_t[3 * (ob + pos)] = v.x; op_t[3 * (ob + pos) + 1] = v.y; op_t[3 * (ob + pos) + 2] = v.z;
        op_rms[ob + pos] = v.w;
      }
    }
    run += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    ntr += wtr[0] + wtr[1] + wtr[2] + wtr[3];
    __syncthreads();
  }
  if (wave == 0) {
    const bool has = lane < nl && lflag[lane] != 0;
    int ti = -1;
    if (has) {
      int w[9];
      sym_decode(latcode[(size_t)kSymLatCap * s + lane], w);
      ti = sym_type_index(w);
    }
    const int npoint = __popcll(__ballot(has));
    int mine = 0;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      const int c = __popcll(__ballot(has && ti == k));
      if (lane == 4 + k) mine = c;
    }
    if (lane == 0) mine = run;
    if (lane == 1) mine = npoint;
    if (lane == 2) mine = ntr;
    if (lane == 3) mine = run > max_ops ? 4 : 0;
    if (lane < kCounts) cnt[lane] = lane < 14 ? mine : 0;
  }
}

// ---------------------------------------------------------------- stage 3: the group
__global__ __launch_bounds__(256) void sym_group_kernel(
    int s0, const int4* __restrict__ sinfo, const double* __restrict__ scell, const double* __restrict__ afrac,
    const int* __restrict__ aperm, const int* __restrict__ arun, const int* __restrict__ nlat,
    const int* __restrict__ latcode, const long long* __restrict__ mapoff, int max_ops, int* __restrict__ counts,
    const int* __restrict__ op_slot, const double* __restrict__ op_t, unsigned char* __restrict__ maps,
    int* __restrict__ orbit, int* __restrict__ mult, double* __restrict__ sym_frac, double* __restrict__ sres) {
  __shared__ double f[3][kMapMaxAtoms], fh[3][kMapMaxAtoms], tmp[2][3][kMapMaxAtoms];
  __shared__ short slot_tab[kSymLatCap * kMapMaxAtoms];
  __shared__ int wl[kSymLatCap][9], lcode[kSymLatCap], orb[kMapMaxAtoms];
  __shared__ double red4[4];
  const int sl = blockIdx.x, s = s0 + sl, tid = threadIdx.x;
  int* cnt = counts + (size_t)kCounts * s;
  if (cnt[3] != 0) return;                                 // uniform: overflow of either kind
  const int nops = cnt[0], nl = nlat[s];
  const int4 ia = sinfo[s];
  const int oa = ia.x, n = ia.y, alo = ia.z, na = ia.w - ia.z;
  const bool have = tid < n;
  int rlo = 0, rhi = 0;
  if (have) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double x = afrac[3 * (size_t)(oa + tid) + c];
      f[c][tid] = x - floor(x);
    }
    const int run = arun[oa + tid];
    rlo = run & 0xffff; rhi = run >> 16;
  }
  if (tid < nl) {
    lcode[tid] = latcode[(size_t)kSymLatCap * s + tid];
    sym_decode(lcode[tid], wl[tid]);
  }
  for (int k = tid; k < nl * na; k += 256) slot_tab[k] = -1;
  __syncthreads();
  const size_t ob = (size_t)sl * max_ops;
  for (int g = tid; g < nops; g += 256) {
    const int v = op_slot[ob + g];
    slot_tab[(v >> 16) * na + ((v & 0xffff) - alo)] = (short)g;
  }
  double m[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = scell[(size_t)kCell * s + k];
  unsigned char* mp = maps + (mapoff[s] - mapoff[s0]);
  const double ax = have ? f[0][tid] : 0.0, ay = have ? f[1][tid] : 0.0, az = have ? f[2][tid] : 0.0;
  const double a0x = f[0][alo], a0y = f[1][alo], a0z = f[2][alo];

  // ---- nb_g per operation, and the projection sum in operation order
  double accx = 0.0, accy = 0.0, accz = 0.0;
  int ph = 0;
  for (int g = 0; g < nops; ++g) {
    const int v = op_slot[ob + g], js = v & 0xffff;
    double w[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = (double)wl[v >> 16][k];
    if (have) {
      double qx, qy, qz, px, py, pz, bd2, ux, uy, uz;
      apply_w(w, ax, ay, az, qx, qy, qz);
      apply_w(w, a0x, a0y, a0z, px, py, pz);
      const double tx = f[0][js] - px, ty = f[1][js] - py, tz = f[2][js] - pz;
      const int br = nearest_in_run(f[0], f[1], f[2], rlo, rhi, qx + tx, qy + ty, qz + tz, m, bd2, ux, uy, uz);
      mp[(size_t)g * n + tid] = (unsigned char)br;
      double dx = (qx + op_t[3 * (ob + g)]) - f[0][br], dy = (qy + op_t[3 * (ob + g) + 1]) - f[1][br],
             dz = (qz + op_t[3 * (ob + g) + 2]) - f[2][br];
      tmp[ph][0][br] = dx - rint(dx); tmp[ph][1][br] = dy - rint(dy); tmp[ph][2][br] = dz - rint(dz);
    }
    __syncthreads();
    if (have) { accx += tmp[ph][0][tid]; accy += tmp[ph][1][tid]; accz += tmp[ph][2][tid]; }
    ph ^= 1;      // the other buffer next: this one is rewritten only after the next barrier
  }
  __syncthreads();   // the maps and the slot table are complete for every thread

  // ---- closure over all ordered pairs (g, h)
  int open = 0;
  for (int p = tid; p < nops * nops && !open; p += 256) {
    const int g = p / nops, h = p - g * nops;
    const int* wg = wl[op_slot[ob + g] >> 16];
    const int* wh = wl[op_slot[ob + h] >> 16];
    int code = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        code = code * 3 + (wg[3 * r] * wh[c] + wg[3 * r + 1] * wh[3 + c] + wg[3 * r + 2] * wh[6 + c]) + 1;
    int lo = 0, hi = nl;                                   // lcode ascends; a product with an entry outside {-1, 0, 1}
    while (hi - lo > 1) {                                  // gives a number that is no stored code, or another matrix's:
      const int mid = (lo + hi) >> 1;                      // checked entry by entry below
      if (lcode[mid] <= code) lo = mid; else hi = mid;
    }
    bool same = lcode[lo] == code;
    if (same) {
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          same = same && wl[lo][3 * r + c] == wg[3 * r] * wh[c] + wg[3 * r + 1] * wh[3 + c] + wg[3 * r + 2] * wh[6 + c];
    }
    if (!same) { open = 1; break; }
    const unsigned char* mg = mp + (size_t)g * n;
    const unsigned char* mh = mp + (size_t)h * n;
    const int k = slot_tab[lo * na + (mg[mh[alo]] - alo)];
    if (k < 0) { open = 1; break; }
    const unsigned char* mk = mp + (size_t)k * n;
    for (int i = 0; i < n; ++i)
      if (mk[i] != mg[mh[i]]) { open = 1; break; }
  }
  if (__syncthreads_or(open)) {
    if (tid == 0) cnt[3] = 8;
    return;
  }

  // ---- orbits, the symmetrised coordinates, shift and residual
  const double dno = (double)nops;
  double shift = 0.0;
  if (have) {
    int mn = tid;
    for (int g = 0; g < nops; ++g) mn = min(mn, (int)mp[(size_t)g * n + tid]);
    orb[tid] = mn;
    const double ex = accx / dno, ey = accy / dno, ez = accz / dno;
    fh[0][tid] = ax + ex; fh[1][tid] = ay + ey; fh[2][tid] = az + ez;
    const double dx = fh[0][tid] - ax, dy = fh[1][tid] - ay, dz = fh[2][tid] - az;
    const double vx = dx * m[0] + dy * m[3] + dz * m[6], vy = dx * m[1] + dy * m[4] + dz * m[7],
                 vz = dx * m[2] + dy * m[5] + dz * m[8];
    shift = sqrt(vx * vx + vy * vy + vz * vz);
  }
  __syncthreads();
  double resid = 0.0;
  if (have) {
    int c = 0;
    for (int k = rlo; k < rhi; ++k) c += orb[k] == orb[tid];     // an orbit lies inside one species run
    const int a = oa + aperm[oa + tid];
    orbit[a] = aperm[oa + orb[tid]];
    mult[a] = c;
    sym_frac[3 * (size_t)a] = fh[0][tid]; sym_frac[3 * (size_t)a + 1] = fh[1][tid]; sym_frac[3 * (size_t)a + 2] = fh[2][tid];
    const double hx = fh[0][tid], hy = fh[1][tid], hz = fh[2][tid];
    for (int g = 0; g < nops; ++g) {
      const int* wi = wl[op_slot[ob + g] >> 16];
      const int br = mp[(size_t)g * n + tid];
      double dx = (wi[0] * hx + wi[1] * hy + wi[2] * hz + op_t[3 * (ob + g)]) - fh[0][br],
             dy = (wi[3] * hx + wi[4] * hy + wi[5] * hz + op_t[3 * (ob + g) + 1]) - fh[1][br],
             dz = (wi[6] * hx + wi[7] * hy + wi[8] * hz + op_t[3 * (ob + g) + 2]) - fh[2][br];
      dx -= rint(dx); dy -= rint(dy); dz -= rint(dz);
      const double vx = dx * m[0] + dy * m[3] + dz * m[6], vy = dx * m[1] + dy * m[4] + dz * m[7],
                   vz = dx * m[2] + dy * m[5] + dz * m[8];
      resid = fmax(resid, sqrt(vx * vx + vy * vy + vz * vz));
    }
  }
  shift = block_max(shift, red4, tid);
  resid = block_max(resid, red4, tid);
  double* o = sres + (size_t)11 * s;          // sym_G[9], sym_shift, sym_resid
  if (tid == 0) { o[9] = shift; o[10] = resid; }
  if (tid < 9) {
    // sym_G = mean over the distinct W (the operation list is sorted by code) of W^T G W
    const double* g6 = scell + (size_t)kCell * s + 18;
    const double gm[3][3] = {{g6[0], g6[1], g6[2]}, {g6[1], g6[3], g6[4]}, {g6[2], g6[4], g6[5]}};
    const int k = tid / 3, l = tid % 3;
    double acc = 0.0;
    int np = 0, last = -1;
    for (int g = 0; g < nops; ++g) {
      const int li = op_slot[ob + g] >> 16;
      if (li == last) continue;
      last = li; ++np;
      const int* wi = wl[li];
      double v = 0.0;
      for (int a = 0; a < 3; ++a) {
        const double gw = gm[a][0] * wi[l] + gm[a][1] * wi[3 + l] + gm[a][2] * wi[6 + l];
        v += wi[3 * a + k] * gw;
      }
      acc += v;
    }
    o[tid] = acc / (double)np;
  }
}

// The argument rules of ics_op_structure_symmetry for its inputs, every structure checked before anything is written: 0,
// or -1 with the error set naming the structure.
int structure_symmetry_check(const int32_t* offsets, const int32_t* species, const double* frac, const double* lattice,
                             const int32_t* eligible, int ns, double tol, double ltol, int max_ops) {
  const std::string op = "ics_op_structure_symmetry: ";
  ICS_CHECK(ns >= 1, op + "ns must be >= 1");
  ICS_CHECK(ns <= INT_MAX - 1, op + "too many structures");
  ICS_CHECK(offsets && lattice && eligible, op + "null argument");
  ICS_CHECK(std::isfinite(tol) && tol > 0.0, op + "tol must be finite and > 0");
  ICS_CHECK(std::isfinite(ltol) && ltol > 0.0, op + "ltol must be finite and > 0");
  ICS_CHECK(max_ops >= 1 && max_ops <= kSymMaxOpsLimit, op + "max_ops must be in 1..4096");
  return check_structures(op, offsets, species, frac, lattice, eligible, ns, tol);
}

}  // namespace
}  // namespace ics

using namespace ics;

// Eligible structures sorted by atom count on the host, one upload, lattice operations for all of them, then per chunk of
// structures (candidate table, nearest-atom maps and operation lists under kSymChunkBytes; ICSG3D_SYMMETRY_CHUNK_BYTES
// shrinks it) the operation, scan and group kernels; synchronous on the calling thread's stream.
extern "C" int ics_op_structure_symmetry(const int32_t* offsets, const int32_t* species, const double* frac,
                                         const double* lattice, const int32_t* eligible, int ns, double tol, double ltol,
                                         int max_ops, int32_t* n_lat, int32_t* n_ops, int32_t* n_point, int32_t* n_trans,
                                         int32_t* types, int32_t* reason, int32_t* op_code, int32_t* op_anchor, double* op_t,
                                         double* op_rms, int32_t* orbit, int32_t* mult, double* sym_frac, double* sym_G,
                                         double* sym_shift, double* sym_resid) {
  ICS_TRY(structure_symmetry_check(offsets, species, frac, lattice, eligible, ns, tol, ltol, max_ops));
  ICS_CHECK(n_lat && n_ops && n_point && n_trans && types && reason && op_code && op_anchor && op_t && op_rms && sym_G &&
                sym_shift && sym_resid,
            "ics_op_structure_symmetry: null output");
  ICS_CHECK((orbit && mult && sym_frac) || offsets[ns] == 0, "ics_op_structure_symmetry: null orbit, mult or sym_frac");
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  const double kNaN = std::numeric_limits<double>::quiet_NaN();
  // ---- the neutral result everywhere; eligible structures are overwritten below
  for (int s = 0; s < ns; ++s) {
    n_lat[s] = n_ops[s] = n_point[s] = n_trans[s] = 0;
    for (int k = 0; k < 10; ++k) types[10 * (size_t)s + k] = 0;
    reason[s] = eligible[s] ? 0 : 1;
    for (size_t k = (size_t)s * max_ops; k < (size_t)(s + 1) * max_ops; ++k) {
      op_code[k] = op_anchor[k] = -1;
      op_t[3 * k] = op_t[3 * k + 1] = op_t[3 * k + 2] = op_rms[k] = kNaN;
    }
    const int a0 = offsets[s], n = offsets[s + 1] - a0;
    for (int i = 0; i < n; ++i) {
      orbit[a0 + i] = i;
      mult[a0 + i] = 1;
      for (int c = 0; c < 3; ++c) {
        const double x = frac[3 * (size_t)(a0 + i) + c];
        sym_frac[3 * (size_t)(a0 + i) + c] = x - std::floor(x);
      }
    }
    double g6[6];
    double* G = sym_G + 9 * (size_t)s;
    cell_gram(lattice + 9 * (size_t)s, g6);
    G[0] = g6[0]; G[1] = G[3] = g6[1]; G[2] = G[6] = g6[2]; G[4] = g6[3]; G[5] = G[7] = g6[4]; G[8] = g6[5];
    sym_shift[s] = sym_resid[s] = 0.0;
  }
  std::vector<int> order;
  for (int s = 0; s < ns; ++s)
    if (eligible[s]) order.push_back(s);
  const int ne = (int)order.size();
  if (ne == 0) return 0;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    return offsets[a + 1] - offsets[a] < offsets[b + 1] - offsets[b];
  });
  size_t N = 0;
  for (int s : order) N += (size_t)(offsets[s + 1] - offsets[s]);

  // ---- the packed block: cells, sorted atoms, species runs, anchor runs, chunk prefixes
  Layout in(16);
  const auto i_cell = in.add<double>((size_t)ne * kCell), i_frac = in.add<double>(3 * N);
  const auto i_cand = in.add<long long>(ne + 1), i_map = in.add<long long>(ne + 1);
  const auto i_info = in.add<int4>(ne);
  const auto i_perm = in.add<int>(N), i_run = in.add<int>(N);
  if (in.bytes() > kSymTableBudget) {
    set_error("ics_op_structure_symmetry: the structure tables (" + std::to_string(in.bytes()) + " bytes) exceed the device budget");
    return -1;
  }
  std::vector<unsigned char> hin(in.bytes(), 0);
  double *hc, *hf;
  long long *hcand, *hmap;
  int4* hinfo;
  int *hperm, *hrun;
  ICS_TRY(in.bind(hin.data(), hin.size(), i_cell, &hc, i_frac, &hf, i_cand, &hcand, i_map, &hmap, i_info, &hinfo, i_perm,
                  &hperm, i_run, &hrun));
  std::vector<int> sz(kMapMaxAtoms);      // the sorted species of the structure at hand: not kept
  std::vector<size_t> cost(ne);
  size_t at = 0;
  hcand[0] = hmap[0] = 0;
  for (int k = 0; k < ne; ++k) {
    const int s = order[k], a0 = offsets[s], n = offsets[s + 1] - a0;
    const double* M = lattice + 9 * (size_t)s;
    double* c = hc + (size_t)kCell * k;
    double vol, g[3];
    int alo, ahi;
    std::memcpy(c, M, 72);
    cell_inverse(M, &vol, g, c + 9);
    cell_gram(M, c + 18);
    sort_atoms(species + a0, n, hperm + at, sz.data(), hrun + at, &alo, &ahi);
    for (int i = 0; i < n; ++i) std::memcpy(hf + 3 * (at + i), frac + 3 * (size_t)(a0 + hperm[at + i]), 24);
    hinfo[k] = make_int4((int)at, n, alo, ahi);
    const size_t ncand = (size_t)kSymLatCap * (ahi - alo), nmap = std::min((size_t)max_ops, ncand) * n;
    hcand[k + 1] = hcand[k] + (long long)ncand;
    hmap[k + 1] = hmap[k] + (long long)align_up(nmap, 16);
    cost[k] = ncand * sizeof(double4) + align_up(nmap, 16) + (size_t)max_ops * kOpBytes;
    at += n;
  }
  // ---- chunks: runs of sorted structures of one kernel kind under the byte cap (at least one structure each)
  std::vector<int> cuts(1, 0);
  size_t max_cand = 0, max_map = 0, max_ns = 0;
  for (int k = 0; k < ne;) {
    const bool small = hinfo[k].y <= kMapSmall;
    size_t bytes = 0;
    int e = k;
    while (e < ne && (hinfo[e].y <= kMapSmall) == small && (e == k || bytes + cost[e] <= chunk_bytes())) bytes += cost[e++];
    cuts.push_back(e);
    max_cand = std::max(max_cand, (size_t)(hcand[e] - hcand[k]));
    max_map = std::max(max_map, (size_t)(hmap[e] - hmap[k]));
    max_ns = std::max(max_ns, (size_t)(e - k));
    k = e;
  }

  Layout L;
  const auto s_in = L.add<unsigned char>(in.bytes());
  const auto s_nlat = L.add<int>(ne), s_lcode = L.add<int>((size_t)ne * kSymLatCap), s_cnt = L.add<int>((size_t)ne * kCounts);
  const auto s_orbit = L.add<int>(N), s_mult = L.add<int>(N);
  const auto s_sfrac = L.add<double>(3 * N), s_sres = L.add<double>((size_t)ne * 11);
  const auto s_cand = L.add<double4>(max_cand);
  const auto s_maps = L.add<unsigned char>(max_map);
  const auto s_ocode = L.add<int>(max_ns * max_ops), s_oanc = L.add<int>(max_ns * max_ops), s_oslot = L.add<int>(max_ns * max_ops);
  const auto s_ot = L.add<double>(3 * max_ns * max_ops), s_orms = L.add<double>(max_ns * max_ops);
  unsigned char *din, *dmaps;
  int *dnlat, *dlcode, *dcnt, *dorbit, *dmult, *docode, *doanc, *doslot, *dperm, *drun;
  double *dsfrac, *dsres, *dot, *dorms, *dcell, *dfrac;
  double4* dcand;
  long long *dcandoff, *dmapoff;
  int4* dinfo;
  ICS_TRY(L.reserve(s_in, &din, s_nlat, &dnlat, s_lcode, &dlcode, s_cnt, &dcnt, s_orbit, &dorbit, s_mult, &dmult, s_sfrac,
                    &dsfrac, s_sres, &dsres, s_cand, &dcand, s_maps, &dmaps, s_ocode, &docode, s_oanc, &doanc, s_oslot,
                    &doslot, s_ot, &dot, s_orms, &dorms));
  ICS_TRY(L.upload(s_in, hin.data(), in.bytes(), st));
  ICS_TRY(in.bind(din, s_in.count, i_cell, &dcell, i_frac, &dfrac, i_cand, &dcandoff, i_map, &dmapoff, i_info, &dinfo,
                  i_perm, &dperm, i_run, &drun));
  // outputs of structures the group kernel leaves alone are never read, but the blocks are downloaded whole
  ICS_TRY(L.fill(s_orbit, 0, N, st));
  ICS_TRY(L.fill(s_mult, 0, N, st));
  ICS_TRY(L.fill(s_sfrac, 0, 3 * N, st));
  ICS_TRY(L.fill(s_sres, 0, (size_t)ne * 11, st));
  ICS_TRY(L.fill(s_cnt, 0, (size_t)ne * kCounts, st));
  ICS_TRY(L.fill(s_nlat, 0, ne, st));

  ICS_LAUNCH(sym_lattice_kernel, dim3((unsigned)ne), dim3(256), 0, st, dcell, ltol, dnlat, dlcode);
  ICS_HIP(hipGetLastError());

  std::vector<int> hocode(max_ns * max_ops), hoanc(max_ns * max_ops), hnlat(ne), hcnt((size_t)ne * kCounts);
  std::vector<double> hot(3 * max_ns * max_ops), horms(max_ns * max_ops);
  for (size_t ci = 0; ci + 1 < cuts.size(); ++ci) {
    const int c0 = cuts[ci], c1 = cuts[ci + 1], nsc = c1 - c0;
    const unsigned units = (unsigned)nsc * kSymLatCap;
    if (hinfo[c0].y <= kMapSmall)
      ICS_LAUNCH(sym_ops_kernel<64>, dim3((units + 3) / 4), dim3(256), 0, st, c0, nsc, dinfo, dcell, dfrac, drun, dnlat,
                 dlcode, dcandoff, tol, dcand);
    else
      ICS_LAUNCH(sym_ops_kernel<256>, dim3(units), dim3(256), 0, st, c0, nsc, dinfo, dcell, dfrac, drun, dnlat, dlcode,
                 dcandoff, tol, dcand);
    ICS_HIP(hipGetLastError());
    ICS_LAUNCH(sym_scan_kernel, dim3((unsigned)nsc), dim3(256), 0, st, c0, dinfo, dperm, dnlat, dlcode, dcandoff, dcand,
               max_ops, dcnt, docode, doanc, doslot, dot, dorms);
    ICS_HIP(hipGetLastError());
    ICS_LAUNCH(sym_group_kernel, dim3((unsigned)nsc), dim3(256), 0, st, c0, dinfo, dcell, dfrac, dperm, drun, dnlat, dlcode,
               dmapoff, max_ops, dcnt, doslot, dot, dmaps, dorbit, dmult, dsfrac, dsres);
    ICS_HIP(hipGetLastError());
    const size_t no = (size_t)nsc * max_ops;
    ICS_TRY(L.download(hocode.data(), s_ocode, no, st));
    ICS_TRY(L.download(hoanc.data(), s_oanc, no, st));
    ICS_TRY(L.download(hot.data(), s_ot, 3 * no, st));
    ICS_TRY(L.download(horms.data(), s_orms, no, st));
    ICS_HIP(hipMemcpyAsync(hcnt.data() + (size_t)kCounts * c0, dcnt + (size_t)kCounts * c0, (size_t)nsc * kCounts * 4,
                           hipMemcpyDeviceToHost, st));
    ICS_HIP(hipStreamSynchronize(st));      // the chunk's buffers are reused by the next one
    for (int k = c0; k < c1; ++k) {
      const int s = order[k];
      const int* cnt = hcnt.data() + (size_t)kCounts * k;
      const size_t keep = (size_t)std::min(std::max(cnt[0], 0), max_ops), from = (size_t)(k - c0) * max_ops,
                   to = (size_t)s * max_ops;
      std::memcpy(op_code + to, hocode.data() + from, keep * 4);
      std::memcpy(op_anchor + to, hoanc.data() + from, keep * 4);
      std::memcpy(op_t + 3 * to, hot.data() + 3 * from, keep * 24);
      std::memcpy(op_rms + to, horms.data() + from, keep * 8);
    }
  }
  std::vector<int> horbit(N), hmult(N);
  std::vector<double> hsfrac(3 * N), hsres((size_t)ne * 11);
  ICS_TRY(L.download(hnlat.data(), s_nlat, ne, st));
  ICS_TRY(L.download(hcnt.data(), s_cnt, (size_t)ne * kCounts, st));      // the group kernel's reason bit
  ICS_TRY(L.download(horbit.data(), s_orbit, N, st));
  ICS_TRY(L.download(hmult.data(), s_mult, N, st));
  ICS_TRY(L.download(hsfrac.data(), s_sfrac, 3 * N, st));
  ICS_TRY(L.download(hsres.data(), s_sres, (size_t)ne * 11, st));
  ICS_HIP(hipStreamSynchronize(st));
  for (int k = 0; k < ne; ++k) {
    const int s = order[k], a0 = offsets[s], n = offsets[s + 1] - a0;
    const int* cnt = hcnt.data() + (size_t)kCounts * k;
    n_lat[s] = hnlat[k];
    n_ops[s] = cnt[0]; n_point[s] = cnt[1]; n_trans[s] = cnt[2]; reason[s] = cnt[3];
    for (int t = 0; t < 10; ++t) types[10 * (size_t)s + t] = cnt[4 + t];
    if (cnt[3] != 0) continue;
    const size_t b = (size_t)hinfo[k].x;
    std::memcpy(orbit + a0, horbit.data() + b, (size_t)n * 4);
    std::memcpy(mult + a0, hmult.data() + b, (size_t)n * 4);
    std::memcpy(sym_frac + 3 * (size_t)a0, hsfrac.data() + 3 * b, (size_t)n * 24);
    std::memcpy(sym_G + 9 * (size_t)s, hsres.data() + (size_t)11 * k, 72);
    sym_shift[s] = hsres[(size_t)11 * k + 9];
    sym_resid[s] = hsres[(size_t)11 * k + 10];
  }
  return 0;
}
