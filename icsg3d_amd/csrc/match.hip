// eval.py's emd() (reference eval.py:45-53) on the device: per sample, the minimum-cost one-to-one matching between two
// point sets under euclidean distance, solved exactly in fp64 by shortest augmenting paths with row and column
// potentials (Jonker-Volgenant in the form of Crouse 2016, the algorithm behind scipy's linear_sum_assignment).
//
// One workgroup per sample.  Rows are the smaller set; the columns are dealt round-robin to the threads (column j
// belongs to thread j % NT), and everything per column -- coordinates, path cost, potential, predecessor, owner,
// visited -- lives in LDS.  Each Dijkstra step is a reduced-cost update of the owned unvisited columns, distances
// computed on the fly (no n x m matrix), followed by a workgroup argmin: wave64 shuffles, then one LDS slot per wave
// combined in wave order.  Ties go to an unassigned column, then to the lowest column index, so results are the same
// run to run.  Only the augmentation walk along the predecessors is serial (thread 0).
#include "scratch.h"
#include "../../include/icsg3d.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace ics {
namespace {

constexpr int kMatchMaxPoints = 2048;              // points per set (MAX_SITES true sites, generate.py's max_atoms)
constexpr size_t kMatchBudget = (size_t)4 << 20;   // points (both sets) per chunk: 96 MB of coordinates
constexpr int kMatchMaxSamples = 1 << 20;          // samples per chunk
constexpr double kMatchMaxCoord = 1e150;           // |coordinate| bound: every distance stays finite
constexpr int kKeyAssigned = 4096;                 // argmin key = (assigned ? 4096 : 0) + column, column < 2048
constexpr int kKeyNone = 0x7fffffff;


__device__ __forceinline__ double dist3(double ax, double ay, double az, double bx, double by, double bz) {
  const double dx = ax - bx, dy = ay - by, dz = az - bz;
  return sqrt(dx * dx + dy * dy + dz * dz);
}

__device__ __forceinline__ bool better(double v1, int k1, double v2, int k2) {
  return v1 < v2 || (v1 == v2 && k1 < k2);
}

// dynamic LDS of one workgroup for `mc` columns and `mr` rows
__host__ __device__ inline size_t match_lds_bytes(int mc, int mr) {
  return (size_t)mc * (5 * sizeof(double) + 2 * sizeof(short) + 1) + (size_t)mr * (sizeof(double) + sizeof(short));
}

template <int NT>
__global__ __launch_bounds__(NT) void match_emd_kernel(const double* __restrict__ a, const int* __restrict__ a_off,
                                                       const double* __restrict__ b, const int* __restrict__ b_off,
                                                       int mc, int mr, double* __restrict__ emd,
                                                       int* __restrict__ match) {
  constexpr int NW = NT / 64;
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ double red_v[2][NW];
  __shared__ int red_k[2][NW];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a0 = a_off[s], na = a_off[s + 1] - a0;
  const int b0 = b_off[s], nb = b_off[s + 1] - b0;
  const bool tr = na > nb;                       // rows = the smaller set (A when the sizes are equal)
  const int nr = tr ? nb : na, nc = tr ? na : nb;
  const double* R = tr ? b + 3 * (size_t)b0 : a + 3 * (size_t)a0;
  const double* Cg = tr ? a + 3 * (size_t)a0 : b + 3 * (size_t)b0;
  if (nr == 0) {                                 // 0 / 0 as the reference
    if (tid == 0) emd[s] = __builtin_nan("");
    if (match)
      for (int i = tid; i < na; i += NT) match[a0 + i] = -1;
    return;
  }
  double* cx = reinterpret_cast<double*>(lds);
  double* cy = cx + mc;
  double* cz = cy + mc;
  double* sp = cz + mc;                          // shortest path cost to each column (this row's search)
  double* v = sp + mc;                           // column potentials
  double* u = v + mc;                            // row potentials [mr]
  short* path = reinterpret_cast<short*>(u + mr);   // predecessor row of each column
  short* r4c = path + mc;                        // owner row of each column, -1 = free
  short* c4r = r4c + mc;                         // column of each row [mr], -1 = unassigned
  unsigned char* sc = reinterpret_cast<unsigned char*>(c4r + mr);   // visited in this row's search

  for (int j = tid; j < nc; j += NT) {
    cx[j] = Cg[3 * j]; cy[j] = Cg[3 * j + 1]; cz[j] = Cg[3 * j + 2];
    v[j] = 0.0;
    r4c[j] = -1;
  }
  for (int i = tid; i < nr; i += NT) { u[i] = 0.0; c4r[i] = -1; }
  __syncthreads();

  bool failed = false;
  int par = 0;
  for (int cur = 0; cur < nr && !failed; ++cur) {
    for (int j = tid; j < nc; j += NT) { sp[j] = INFINITY; sc[j] = 0; }
    int i = cur, sink = -1;
    double minVal = 0.0;
    // every step visits a new column: at most nc steps
    for (int step = 0; step < nc && sink < 0; ++step) {
      const double xi = R[3 * i], yi = R[3 * i + 1], zi = R[3 * i + 2], ui = u[i];
      double bv = INFINITY;
      int bk = kKeyNone;
      for (int j = tid; j < nc; j += NT) {
        if (sc[j]) continue;
        const double r = minVal + dist3(xi, yi, zi, cx[j], cy[j], cz[j]) - ui - v[j];
        if (r < sp[j]) { sp[j] = r; path[j] = (short)i; }
        const int k = (r4c[j] >= 0 ? kKeyAssigned : 0) + j;
        if (better(sp[j], k, bv, bk)) { bv = sp[j]; bk = k; }
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const int ok = __shfl_xor(bk, o, 64);
        if (better(ov, ok, bv, bk)) { bv = ov; bk = ok; }
      }
      if (NW > 1) {
        if (lane == 0) { red_v[par][wave] = bv; red_k[par][wave] = bk; }
        __syncthreads();                         // red[par] is rewritten two steps later, past the next barrier
        bv = red_v[par][0]; bk = red_k[par][0];
#pragma unroll
        for (int w = 1; w < NW; ++w)
          if (better(red_v[par][w], red_k[par][w], bv, bk)) { bv = red_v[par][w]; bk = red_k[par][w]; }
        par ^= 1;
      }
      if (bk == kKeyNone || !(bv < INFINITY)) { failed = true; break; }   // uniform; unreachable for finite input
      const int j = bk & (kKeyAssigned - 1);
      minVal = bv;
      if ((j % NT) == tid) sc[j] = 1;            // the owner alone reads sc[j] inside the search
      const int owner = r4c[j];
      if (owner < 0) sink = j; else i = owner;
    }
    if (failed || sink < 0) { failed = true; break; }
    __syncthreads();
    // potentials: the rows visited are the owners of the visited columns other than the sink, plus cur
    if (tid == 0) u[cur] += minVal;
    for (int j = tid; j < nc; j += NT) {
      if (!sc[j]) continue;
      const double dlt = minVal - sp[j];
      if (j != sink) u[r4c[j]] += dlt;
      v[j] -= dlt;
    }
    __syncthreads();
    if (tid == 0) {                              // augment along the predecessors back to cur
      int j = sink;
      for (int n = 0; n <= nr; ++n) {
        const int pi = path[j];
        r4c[j] = (short)pi;
        const int t = c4r[pi];
        c4r[pi] = (short)j;
        j = t;
        if (pi == cur) break;
      }
    }
    __syncthreads();
  }

  // matched distance sum in a fixed order: per thread over its rows, then wave and workgroup in order
  double sum = 0.0;
  for (int i = tid; i < nr; i += NT) {
    const int j = c4r[i];
    if (j >= 0) sum += dist3(R[3 * i], R[3 * i + 1], R[3 * i + 2], cx[j], cy[j], cz[j]);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
  __syncthreads();
  if (lane == 0) red_v[0][wave] = sum;
  __syncthreads();
  if (tid == 0) {
    double t = red_v[0][0];
    for (int w = 1; w < NW; ++w) t += red_v[0][w];
    emd[s] = failed ? __builtin_nan("") : t / (double)nr;
  }
  if (match) {
    if (!tr) {
      for (int i = tid; i < na; i += NT) match[a0 + i] = failed ? -1 : c4r[i];
    } else {
      for (int j = tid; j < na; j += NT) match[a0 + j] = failed ? -1 : r4c[j];
    }
  }
}

int check_set(const double* p, const int32_t* off, int batch, char name) {
  ICS_CHECK(off[0] == 0, std::string("ics_op_match_emd: ") + name + "_off[0] must be 0");
  for (int s = 0; s < batch; ++s) {
    const long long n = (long long)off[s + 1] - off[s];
    ICS_CHECK(n >= 0, std::string("ics_op_match_emd: ") + name + "_off decreases at sample " + std::to_string(s));
    ICS_CHECK(n <= kMatchMaxPoints, std::string("ics_op_match_emd: sample ") + std::to_string(s) + " has " +
                                        std::to_string(n) + " points in " + name + ", above the limit of " +
                                        std::to_string(kMatchMaxPoints));
  }
  ICS_CHECK(p != nullptr || off[batch] == 0, std::string("ics_op_match_emd: null ") + name);
  for (int s = 0; s < batch; ++s)
    for (long long k = 3LL * off[s]; k < 3LL * off[s + 1]; ++k)
      ICS_CHECK(std::isfinite(p[k]) && std::fabs(p[k]) <= kMatchMaxCoord,
                std::string("ics_op_match_emd: sample ") + std::to_string(s) + " has a non-finite or out-of-range (> 1e150) coordinate in " + name);
  return 0;
}

template <int NT>
int launch_chunk(hipStream_t st, const double* da, const int* dao, const double* db, const int* dbo, int n, int mc,
                 int mr, double* demd, int* dmatch) {
  const size_t lds = match_lds_bytes(mc, mr);
  auto kern = match_emd_kernel<NT>;
  if (lds > 65536)
    ICS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
  ICS_LAUNCH(kern, dim3((unsigned)n), dim3(NT), lds, st, da, dao, db, dbo, mc, mr, demd, dmatch);
  ICS_HIP(hipGetLastError());
  return 0;
}

}  // namespace

}  // namespace ics

using namespace ics;

// The argument rules of include/icsg3d.h, every sample checked before anything is written; then the batch solved in chunks
// under a device-memory budget through the calling thread's scratch, synchronous on its stream.
extern "C" int ics_op_match_emd(const double* a, const int32_t* a_off, const double* b, const int32_t* b_off, int batch,
                                double* emd, int32_t* match) {
  ICS_CHECK(batch >= 1, "ics_op_match_emd: batch must be >= 1");
  ICS_CHECK(a_off && b_off && emd, "ics_op_match_emd: null argument");
  ICS_TRY(check_set(a, a_off, batch, 'a'));
  ICS_TRY(check_set(b, b_off, batch, 'b'));
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  std::vector<int> ao, bo;
  for (int s0 = 0; s0 < batch;) {
    // one chunk: samples [s0, s1) under the point budget (at least one sample)
    int s1 = s0, mc = 0, mr = 0;
    size_t pts = 0;
    while (s1 < batch && s1 - s0 < kMatchMaxSamples) {
      const int na = a_off[s1 + 1] - a_off[s1], nb = b_off[s1 + 1] - b_off[s1];
      if (s1 > s0 && pts + na + nb > kMatchBudget) break;
      pts += na + nb;
      mc = std::max(mc, std::max(na, nb));
      mr = std::max(mr, std::min(na, nb));
      ++s1;
    }
    const int n = s1 - s0;
    const int A0 = a_off[s0], NA = a_off[s1] - A0, B0 = b_off[s0], NB = b_off[s1] - B0;
    ao.resize(n + 1); bo.resize(n + 1);
    for (int k = 0; k <= n; ++k) { ao[k] = a_off[s0 + k] - A0; bo[k] = b_off[s0 + k] - B0; }
    Layout L;
    const auto s_a = L.add<double>(3 * (size_t)NA + 1), s_b = L.add<double>(3 * (size_t)NB + 1);   // one spare: never empty
    const auto s_ao = L.add<int>(n + 1), s_bo = L.add<int>(n + 1);
    const auto s_emd = L.add<double>(n);
    const auto s_match = L.add<int>(match ? (size_t)NA + 1 : 0);
    double *da, *db, *demd;
    int *dao, *dbo, *dmatch;
    ICS_TRY(L.reserve(s_a, &da, s_b, &db, s_ao, &dao, s_bo, &dbo, s_emd, &demd, s_match, &dmatch));
    ICS_TRY(L.upload(s_a, a + 3 * (size_t)A0, 3 * (size_t)NA, st));
    ICS_TRY(L.upload(s_b, b + 3 * (size_t)B0, 3 * (size_t)NB, st));
    ICS_TRY(L.upload(s_ao, ao.data(), n + 1, st));
    ICS_TRY(L.upload(s_bo, bo.data(), n + 1, st));
    // one wave per sample while every sample's columns fit in two passes of it; four waves above that
    if (mc <= 128) ICS_TRY(launch_chunk<64>(st, da, dao, db, dbo, n, mc, mr, demd, dmatch));
    else ICS_TRY(launch_chunk<256>(st, da, dao, db, dbo, n, mc, mr, demd, dmatch));
    ICS_TRY(L.download(emd + s0, s_emd, n, st));
    if (match) ICS_TRY(L.download(match + A0, s_match, NA, st));
    ICS_HIP(hipStreamSynchronize(st));
    s0 = s1;
  }
  return 0;
}
