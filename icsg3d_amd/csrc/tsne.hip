// The t-SNE map of the latent space (reference viz.py tsne_latent: sklearn.manifold.TSNE(n_components=2)) on the device,
// with the repulsion summed exactly over all pairs -- scikit-learn's objective at angle = 0.
//
// tsne_knn_kernel        exact k nearest neighbours.  One workgroup owns 64 rows and streams 64-column tiles: the tile's
//                        squared distances are a 4 x 4 register block per thread over fp64 operands staged in LDS, 16
//                        dimensions at a time, differences and squares summed in dimension order.  The tile then goes to LDS
//                        and one thread per row tests its 64 candidates against the row's current k-th distance; an
//                        insertion (rare after the first tiles) shifts the row's sorted list, which lives in LDS for
//                        k <= 128 and in the output arrays above that.  Columns arrive in index order, so ties keep the
//                        lower index first.  No n x n matrix anywhere.
// tsne_affinity_kernel   _binary_search_perplexity, one wave per row: sums by wave64 butterfly (the same bits in every lane).
// (host)                 P = (C + C^T) / sum as CSR with sorted columns, built once: a counting pass over the edges.
// tsne_repulsion_kernel  sum_j q^2 (y_i - y_j) and sum_j q over ALL j: grid = row blocks x column slabs, y tiles in LDS, pair
//                        arithmetic in float32, 16 pairs per float32 partial, fp64 above.  The pair j = i adds q = 1 and no
//                        force; Z subtracts n.
// tsne_combine_kernel    slab partials added in slab order per row; sum of q per block in a fixed tree.
// tsne_step_kernel       one wave per row: attraction over the row's CSR edges (scikit-learn's float32 pair arithmetic, fp64
//                        sums), the gradient, then _gradient_descent's gains / momentum update into the other y buffer.
// tsne_reduce2_kernel    KL divergence and squared gradient norm, one workgroup, fixed order (check iterations only).
// No floating-point atomics; every sum has a fixed order, so results are the same run to run.
#include "tsne.h"
#include "scratch.h"

#include <algorithm>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

struct ics_tsne {
  ics_tsne_config cfg{};
  int device = 0;
  hipStream_t st = nullptr;
  std::vector<void*> allocs;          // everything but the codes; released by drop_state
  float* codes = nullptr;             // [capacity][dim]
  int count = 0;                      // codes appended
  // graph + descent state of n points
  int n = 0;
  size_t nnz = 0;
  long long* indptr = nullptr;
  int* indices = nullptr;
  double* vals = nullptr;
  float* y[2] = {nullptr, nullptr};   // [n][2] each; y[cur] is the embedding
  int cur = 0;
  float *upd = nullptr, *gains = nullptr, *grad = nullptr;
  double *part = nullptr, *rep = nullptr, *zpart = nullptr, *klrow = nullptr, *gnrow = nullptr, *red = nullptr;
  int slabs = 1, slab_cols = 0, row_blocks = 0;
  // schedule
  int iter = 0;                       // next iteration index
  int last_iter = -1;
  bool phase2 = false, finished = false;
  double lr = 0.0, best_error = DBL_MAX, kl = NAN, grad_norm = NAN;
  int best_iter = 0;
};

namespace ics {
namespace {

constexpr int kKnnThreads = 256, kKnnTile = 64, kKnnDk = 16, kKnnLdsK = 128;
constexpr int kRepThreads = 256, kRepTile = 1024, kRepChunk = 16, kRepMaxSlabs = 64;
constexpr int kRowThreads = 256;      // 4 waves = 4 rows per workgroup in the wave-per-row kernels
constexpr float kFloatTiny = 1.17549435e-38f;   // np.finfo(np.float32).tiny


__host__ __device__ inline size_t knn_lds_bytes(int k, bool lists) {
  size_t b = (size_t)2 * kKnnDk * kKnnTile * 8 + (size_t)kKnnTile * (kKnnTile + 1) * 8;
  if (lists) b += (size_t)kKnnTile * k * 12;
  return b;
}

__global__ __launch_bounds__(kKnnThreads) void tsne_knn_kernel(const float* __restrict__ x, int n, int dim, int k,
                                                              int lists_in_lds, int* out_idx, double* out_d) {
  extern __shared__ __align__(16) unsigned char lds[];
  double* As = reinterpret_cast<double*>(lds);            // [16][64] this block's rows, dimension major
  double* Bs = As + kKnnDk * kKnnTile;                    // [16][64] the column tile
  double* Dt = Bs + kKnnDk * kKnnTile;                    // [64][65] the tile's squared distances
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int lr = tid >> 2, ld0 = (tid & 3) * 4;           // staging: row lr, dimensions ld0 .. ld0 + 3 of the chunk
  const int r0 = blockIdx.x * kKnnTile;
  double* Ld;                                             // this thread's row list (threads 0..63)
  int* Li;
  if (lists_in_lds) {
    double* base = Dt + kKnnTile * (kKnnTile + 1);
    Ld = base + (size_t)(tid & 63) * k;
    Li = reinterpret_cast<int*>(base + (size_t)kKnnTile * k) + (size_t)(tid & 63) * k;
  } else {
    const size_t row = (size_t)min(r0 + (tid & 63), n - 1);
    Ld = out_d + row * k;
    Li = out_idx + row * k;
  }
  const int my_row = r0 + tid;                            // meaningful for tid < 64
  const bool scans = tid < kKnnTile && my_row < n;
  int have = 0;
  double kth = INFINITY;

  for (int c0 = 0; c0 < n; c0 += kKnnTile) {
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int d0 = 0; d0 < dim; d0 += kKnnDk) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int d = d0 + ld0 + q;
        const int ra = r0 + lr, cb = c0 + lr;
        As[(ld0 + q) * kKnnTile + lr] = (ra < n && d < dim) ? (double)x[(size_t)ra * dim + d] : 0.0;
        Bs[(ld0 + q) * kKnnTile + lr] = (cb < n && d < dim) ? (double)x[(size_t)cb * dim + d] : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int dd = 0; dd < kKnnDk; ++dd) {
        double av[4], bv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) av[a] = As[dd * kKnnTile + ty * 4 + a];
#pragma unroll
        for (int b = 0; b < 4; ++b) bv[b] = Bs[dd * kKnnTile + tx * 4 + b];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const double t = av[a] - bv[b];
            acc[a][b] = acc[a][b] + t * t;
          }
      }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) Dt[(ty * 4 + a) * (kKnnTile + 1) + tx * 4 + b] = acc[a][b];
    __syncthreads();
    if (scans) {
      const int jn = min(kKnnTile, n - c0);
      for (int jj = 0; jj < jn; ++jj) {
        const int j = c0 + jj;
        if (j == my_row) continue;
        const double dv = Dt[tid * (kKnnTile + 1) + jj];
        if (have == k && !(dv < kth)) continue;
        int p = have < k ? have : k - 1;                  // a full list drops its last entry
        while (p > 0 && Ld[p - 1] > dv) { Ld[p] = Ld[p - 1]; Li[p] = Li[p - 1]; --p; }
        Ld[p] = dv; Li[p] = j;
        if (have < k) ++have;
        if (have == k) kth = Ld[k - 1];
      }
    }
    // Dt is rewritten after the next tile's staging barriers, which the scanning threads reach only when done
  }
  if (lists_in_lds) {
    __syncthreads();
    const double* base = Dt + kKnnTile * (kKnnTile + 1);
    const int* ibase = reinterpret_cast<const int*>(base + (size_t)kKnnTile * k);
    const int rows = min(kKnnTile, n - r0);
    for (int e = tid; e < rows * k; e += kKnnThreads) {
      out_d[(size_t)r0 * k + e] = base[e];
      out_idx[(size_t)r0 * k + e] = ibase[e];
    }
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(kRowThreads) void tsne_affinity_kernel(const double* __restrict__ d2, int n, int k,
                                                                  double perplexity, double* __restrict__ P) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (kRowThreads / 64) + (threadIdx.x >> 6);
  if (row >= n) return;                                   // wave-uniform
  const double* dr = d2 + (size_t)row * k;
  const double want = log((double)(float)perplexity);     // `float desired_perplexity`
  const double tol = (double)1e-5f, floor_sum = (double)1e-8f;   // both are C floats in _utils.pyx
  double beta = 1.0, lo = -INFINITY, hi = INFINITY, used = 1.0, sum = 1.0;
  for (int step = 0; step < 100; ++step) {
    double s = 0.0;
    for (int j = lane; j < k; j += 64) s += exp(-(double)(float)dr[j] * beta);
    s = wave_sum(s);
    if (s == 0.0) s = floor_sum;
    double sd = 0.0;
    for (int j = lane; j < k; j += 64) {
      const double d = (double)(float)dr[j];
      sd += d * (exp(-d * beta) / s);
    }
    sd = wave_sum(sd);
    used = beta; sum = s;
    const double diff = log(s) + beta * sd - want;
    if (fabs(diff) <= tol) break;
    if (diff > 0.0) {
      lo = beta;
      beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
    } else {
      hi = beta;
      beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
    }
  }
  for (int j = lane; j < k; j += 64) P[(size_t)row * k + j] = exp(-(double)(float)dr[j] * used) / sum;
}

__global__ void tsne_finite_kernel(const float* __restrict__ x, size_t count, int* __restrict__ flag) {
  bool bad = false;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
    bad |= !isfinite(x[i]);
  if (bad) *flag = 1;
}

__global__ void tsne_fill_kernel(float* __restrict__ p, size_t count, float v) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) p[i] = v;
}

// part [slabs][3][n] fp64: {sum q^2 dx, sum q^2 dy, sum q} of row i over the slab's columns
__global__ __launch_bounds__(kRepThreads) void tsne_repulsion_kernel(const float2* __restrict__ y, int n, int slab_cols,
                                                                    double* __restrict__ part) {
  __shared__ float2 tile[kRepTile];
  const int tid = threadIdx.x, i = blockIdx.x * kRepThreads + tid, slab = blockIdx.y;
  const int c_begin = slab * slab_cols, c_end = min(n, c_begin + slab_cols);
  const float2 yi = i < n ? y[i] : make_float2(0.f, 0.f);
  double fx = 0.0, fy = 0.0, sq = 0.0;
  for (int t0 = c_begin; t0 < c_end; t0 += kRepTile) {
    const int cnt = min(kRepTile, c_end - t0);
    __syncthreads();
    for (int e = tid; e < cnt; e += kRepThreads) tile[e] = y[t0 + e];
    __syncthreads();
    for (int c = 0; c < cnt; c += kRepChunk) {
      const int m = min(kRepChunk, cnt - c);
      float ax = 0.f, ay = 0.f, aq = 0.f;
      if (m == kRepChunk) {
#pragma unroll
        for (int u = 0; u < kRepChunk; ++u) {
          const float2 yj = tile[c + u];
          const float dx = yi.x - yj.x, dy = yi.y - yj.y;
          const float d = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, 1.0f));
          float q = __builtin_amdgcn_rcpf(d);
          q = __builtin_fmaf(q, __builtin_fmaf(-d, q, 1.0f), q);      // one Newton step on the hardware reciprocal
          const float q2 = q * q;
          aq += q;
          ax = __builtin_fmaf(q2, dx, ax);
          ay = __builtin_fmaf(q2, dy, ay);
        }
      } else {
        for (int u = 0; u < m; ++u) {
          const float2 yj = tile[c + u];
          const float dx = yi.x - yj.x, dy = yi.y - yj.y;
          const float d = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, 1.0f));
          float q = __builtin_amdgcn_rcpf(d);
          q = __builtin_fmaf(q, __builtin_fmaf(-d, q, 1.0f), q);
          const float q2 = q * q;
          aq += q;
          ax = __builtin_fmaf(q2, dx, ax);
          ay = __builtin_fmaf(q2, dy, ay);
        }
      }
      fx += (double)ax; fy += (double)ay; sq += (double)aq;
    }
  }
  if (i < n) {
    double* p = part + (size_t)slab * 3 * n;
    p[i] = fx; p[(size_t)n + i] = fy; p[2 * (size_t)n + i] = sq;
  }
}

// rep [2][n] = the slab partials in slab order; zpart[block] = this block's sum of q in a fixed tree
__global__ __launch_bounds__(kRepThreads) void tsne_combine_kernel(const double* __restrict__ part, int n, int slabs,
                                                                  double* __restrict__ rep, double* __restrict__ zpart) {
  __shared__ double red[kRepThreads / 64];
  const int tid = threadIdx.x, i = blockIdx.x * kRepThreads + tid;
  double fx = 0.0, fy = 0.0, sq = 0.0;
  if (i < n) {
    for (int s = 0; s < slabs; ++s) {
      const double* p = part + (size_t)s * 3 * n;
      fx += p[i]; fy += p[(size_t)n + i]; sq += p[2 * (size_t)n + i];
    }
    rep[i] = fx; rep[(size_t)n + i] = fy;
  }
  sq = wave_sum(sq);
  if ((tid & 63) == 0) red[tid >> 6] = sq;
  __syncthreads();
  if (tid == 0) {
    double t = red[0];
    for (int w = 1; w < kRepThreads / 64; ++w) t += red[w];
    zpart[blockIdx.x] = t;
  }
}

struct StepArgs {
  const float2* y_in;
  float2* y_out;      // nullptr: gradient only
  float2* upd;
  float2* gains;
  float2* grad_out;   // nullptr, or the gradient before the gains
  const long long* indptr;
  const int* indices;
  const double* vals;
  const double* rep;
  const double* zpart;
  double* klrow;
  double* gnrow;
  double exag;
  int nzpart, n, want_error;
  float momentum, lr;
};

__device__ __forceinline__ float gain_step(float& gain, float& upd, float g, float momentum, float lr) {
  gain = (upd * g < 0.0f) ? gain + 0.2f : gain * 0.8f;
  gain = fmaxf(gain, 0.01f);
  g = g * gain;
  const float a = momentum * upd, b = lr * g;
  upd = a - b;
  return g;
}

__global__ __launch_bounds__(kRowThreads) void tsne_step_kernel(StepArgs A) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (kRowThreads / 64) + (threadIdx.x >> 6);
  if (row >= A.n) return;                                 // wave-uniform
  double z = 0.0;
  for (int b = lane; b < A.nzpart; b += 64) z += A.zpart[b];
  z = wave_sum(z) - (double)A.n;                          // the n pairs j = i added 1 each
  z = fmax(z, DBL_EPSILON);
  const float2 yi = A.y_in[row];
  double ax = 0.0, ay = 0.0, kl = 0.0;
  const long long e1 = A.indptr[row + 1];
  for (long long e = A.indptr[row] + lane; e < e1; e += 64) {
    const float2 yj = A.y_in[A.indices[e]];
    const float pij = (float)(A.vals[e] * A.exag);
    const float bx = yi.x - yj.x, by = yi.y - yj.y;
    float dij = bx * bx;
    dij = dij + by * by;
    const float qij = 1.0f / (1.0f + dij);
    const float w = pij * qij;
    ax += (double)(w * bx); ay += (double)(w * by);
    if (A.want_error) {
      const float qn = (float)((double)qij / z);
      kl += (double)pij * log((double)(fmaxf(pij, kFloatTiny) / fmaxf(qn, kFloatTiny)));
    }
  }
  ax = wave_sum(ax); ay = wave_sum(ay);
  if (A.want_error) kl = wave_sum(kl);
  if (lane != 0) return;
  const float px = (float)ax, py = (float)ay;
  const float nx = (float)A.rep[row], ny = (float)A.rep[(size_t)A.n + row];
  float gx = (float)((double)px - (double)nx / z), gy = (float)((double)py - (double)ny / z);
  gx = gx * 4.0f; gy = gy * 4.0f;                          // c = 2 (dof + 1) / dof at dof = 1
  if (A.grad_out) A.grad_out[row] = make_float2(gx, gy);
  if (A.want_error) A.klrow[row] = kl;
  if (A.y_out) {
    float2 g = A.gains[row], u = A.upd[row];
    gx = gain_step(g.x, u.x, gx, A.momentum, A.lr);
    gy = gain_step(g.y, u.y, gy, A.momentum, A.lr);
    A.gains[row] = g; A.upd[row] = u;
    A.y_out[row] = make_float2(yi.x + u.x, yi.y + u.y);
    if (A.want_error) A.gnrow[row] = (double)gx * (double)gx + (double)gy * (double)gy;
  }
}

// out[0] = sum a, out[1] = sum b (b optional), one workgroup: strided partial sums, butterfly, waves in order
__global__ __launch_bounds__(1024) void tsne_reduce2_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                           int n, double* __restrict__ out) {
  __shared__ double red[2][16];
  const int tid = threadIdx.x;
  double sa = 0.0, sb = 0.0;
  for (int i = tid; i < n; i += 1024) { sa += a[i]; if (b) sb += b[i]; }
  sa = wave_sum(sa); sb = wave_sum(sb);
  if ((tid & 63) == 0) { red[0][tid >> 6] = sa; red[1][tid >> 6] = sb; }
  __syncthreads();
  if (tid == 0) {
    double ta = red[0][0], tb = red[1][0];
    for (int w = 1; w < 16; ++w) { ta += red[0][w]; tb += red[1][w]; }
    out[0] = ta; out[1] = tb;
  }
}

int launch_knn(hipStream_t st, const float* d_x, int n, int dim, int k, int* d_idx, double* d_dist) {
  const bool lists = k <= kKnnLdsK;
  const size_t lds = knn_lds_bytes(k, lists);
  auto kern = tsne_knn_kernel;
  if (lds > 65536)
    ICS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
  ICS_HIP(hipMemsetAsync(d_idx, 0, (size_t)n * k * 4, st));
  ICS_LAUNCH(kern, dim3((unsigned)((n + kKnnTile - 1) / kKnnTile)), dim3(kKnnThreads), lds, st, d_x, n, dim, k,
             lists ? 1 : 0, d_idx, d_dist);
  ICS_HIP(hipGetLastError());
  return 0;
}

int launch_affinities(hipStream_t st, const double* d_dist, int n, int k, double perplexity, double* d_p) {
  const int rows = kRowThreads / 64;
  ICS_LAUNCH(tsne_affinity_kernel, dim3((unsigned)((n + rows - 1) / rows)), dim3(kRowThreads), 0, st, d_dist, n, k,
             perplexity, d_p);
  ICS_HIP(hipGetLastError());
  return 0;
}

int check_init(const char* who, const float* init, int rows, int cols, int n) {
  const std::string p = std::string(who) + ": ";
  ICS_CHECK(init != nullptr, p + "null init");
  ICS_CHECK(rows == n && cols == 2, p + "init must be [" + std::to_string(n) + "][2], got [" + std::to_string(rows) +
                                        "][" + std::to_string(cols) + "]");
  for (size_t i = 0; i < (size_t)n * 2; ++i) ICS_CHECK(std::isfinite(init[i]), p + "init is not finite");
  return 0;
}

template <typename T>
int dev_alloc(ics_tsne* h, size_t count, T** out) {
  void* p = nullptr;
  ICS_HIP(hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)));
  h->allocs.push_back(p);
  *out = static_cast<T*>(p);
  return 0;
}

void drop_state(ics_tsne* h) {
  for (void* p : h->allocs) (void)hipFree(p);
  h->allocs.clear();
  h->n = 0; h->nnz = 0;
  h->indptr = nullptr; h->indices = nullptr; h->vals = nullptr;
}

// CSR on the host -> device, descent state for n points, embedding = init, iteration 0
int install(ics_tsne* h, int n, const long long* indptr, const int* indices, const double* vals, const float* init) {
  drop_state(h);
  const size_t nnz = (size_t)indptr[n];
  h->n = n; h->nnz = nnz;
  h->row_blocks = (n + kRepThreads - 1) / kRepThreads;
  // enough workgroups for every CU four times over, slabs a multiple of the chunk
  int slabs = std::min(kRepMaxSlabs, std::max(1, (1024 + h->row_blocks - 1) / h->row_blocks));
  int cols = ((n + slabs - 1) / slabs + kRepChunk - 1) / kRepChunk * kRepChunk;
  slabs = (n + cols - 1) / cols;
  h->slabs = slabs; h->slab_cols = cols;
  ICS_TRY(dev_alloc(h, (size_t)n + 1, &h->indptr));
  ICS_TRY(dev_alloc(h, nnz, &h->indices));
  ICS_TRY(dev_alloc(h, nnz, &h->vals));
  for (int b = 0; b < 2; ++b) ICS_TRY(dev_alloc(h, (size_t)n * 2, &h->y[b]));
  ICS_TRY(dev_alloc(h, (size_t)n * 2, &h->upd));
  ICS_TRY(dev_alloc(h, (size_t)n * 2, &h->gains));
  ICS_TRY(dev_alloc(h, (size_t)n * 2, &h->grad));
  ICS_TRY(dev_alloc(h, (size_t)slabs * 3 * n, &h->part));
  ICS_TRY(dev_alloc(h, (size_t)n * 2, &h->rep));
  ICS_TRY(dev_alloc(h, (size_t)h->row_blocks, &h->zpart));
  ICS_TRY(dev_alloc(h, (size_t)n, &h->klrow));
  ICS_TRY(dev_alloc(h, (size_t)n, &h->gnrow));
  ICS_TRY(dev_alloc(h, 2, &h->red));
  ICS_HIP(hipMemcpyAsync(h->indptr, indptr, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, h->st));
  if (nnz) {
    ICS_HIP(hipMemcpyAsync(h->indices, indices, nnz * 4, hipMemcpyHostToDevice, h->st));
    ICS_HIP(hipMemcpyAsync(h->vals, vals, nnz * 8, hipMemcpyHostToDevice, h->st));
  }
  h->cur = 0;
  ICS_HIP(hipMemcpyAsync(h->y[0], init, (size_t)n * 8, hipMemcpyHostToDevice, h->st));
  ICS_HIP(hipMemsetAsync(h->upd, 0, (size_t)n * 8, h->st));
  ICS_LAUNCH(tsne_fill_kernel, dim3((unsigned)((2 * (size_t)n + 255) / 256)), dim3(256), 0, h->st, h->gains,
             (size_t)n * 2, 1.0f);
  ICS_HIP(hipGetLastError());
  ICS_HIP(hipStreamSynchronize(h->st));
  h->iter = 0; h->last_iter = -1; h->phase2 = false; h->finished = false;
  h->best_error = DBL_MAX; h->best_iter = 0; h->kl = NAN; h->grad_norm = NAN;
  const double ee = h->cfg.early_exaggeration;
  h->lr = h->cfg.learning_rate > 0.0 ? h->cfg.learning_rate : std::max((double)n / ee / 4.0, 50.0);
  return 0;
}

// the three gradient launches on y_in; y_out == nullptr leaves the descent's state alone
int enqueue_gradient(ics_tsne* h, const float* y_in, float* y_out, float* grad_out, double exag, float momentum,
                     bool want_error) {
  const int n = h->n;
  ICS_LAUNCH(tsne_repulsion_kernel, dim3((unsigned)h->row_blocks, (unsigned)h->slabs), dim3(kRepThreads), 0, h->st,
             reinterpret_cast<const float2*>(y_in), n, h->slab_cols, h->part);
  ICS_LAUNCH(tsne_combine_kernel, dim3((unsigned)h->row_blocks), dim3(kRepThreads), 0, h->st, h->part, n, h->slabs,
             h->rep, h->zpart);
  StepArgs A;
  A.y_in = reinterpret_cast<const float2*>(y_in);
  A.y_out = reinterpret_cast<float2*>(y_out);
  A.upd = reinterpret_cast<float2*>(h->upd);
  A.gains = reinterpret_cast<float2*>(h->gains);
  A.grad_out = reinterpret_cast<float2*>(grad_out);
  A.indptr = h->indptr; A.indices = h->indices; A.vals = h->vals;
  A.rep = h->rep; A.zpart = h->zpart; A.klrow = h->klrow; A.gnrow = h->gnrow;
  A.exag = exag; A.nzpart = h->row_blocks; A.n = n; A.want_error = want_error ? 1 : 0;
  A.momentum = momentum; A.lr = (float)h->lr;
  const int rows = kRowThreads / 64;
  ICS_LAUNCH(tsne_step_kernel, dim3((unsigned)((n + rows - 1) / rows)), dim3(kRowThreads), 0, h->st, A);
  ICS_HIP(hipGetLastError());
  return 0;
}

int handle_enter(ics_tsne* h) {
  ICS_CHECK(h != nullptr, "null t-SNE handle");
  ICS_HIP(hipSetDevice(h->device));
  return 0;
}

double seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

// ---------------------------------------------------------------- what the engine's encode -> append path uses
int tsne_device(const ics_tsne* h) { return h->device; }
int tsne_dim(const ics_tsne* h) { return h->cfg.dim; }

int tsne_append_device(ics_tsne* h, const float* src, size_t stride_floats, int rows, hipStream_t src_stream) {
  ICS_TRY(handle_enter(h));
  ICS_CHECK(src != nullptr, "ics_op_tsne_append_vae: null source");
  ICS_CHECK(rows >= 1 && rows <= h->cfg.capacity - h->count, "ics_op_tsne_append_vae: rows exceed the handle's capacity");
  const size_t w = (size_t)h->cfg.dim * 4;
  ICS_HIP(hipMemcpy2DAsync(h->codes + (size_t)h->count * h->cfg.dim, w, src, stride_floats * 4, w, (size_t)rows,
                           hipMemcpyDeviceToDevice, src_stream));
  ICS_HIP(hipStreamSynchronize(src_stream));
  h->count += rows;
  return 0;
}

}  // namespace ics

using namespace ics;

extern "C" {

// ---------------------------------------------------------------- ops
int ics_op_tsne_knn(const float* x, int n, int dim, int k, int32_t* idx, double* dist2) {
  ICS_CHECK(x && idx && dist2, "ics_op_tsne_knn: null argument");
  ICS_CHECK(n >= 2 && n <= kTsneMaxPoints, "ics_op_tsne_knn: n must be 2.." + std::to_string(kTsneMaxPoints));
  ICS_CHECK(dim >= 1 && dim <= kTsneMaxDim, "ics_op_tsne_knn: dim must be 1..4096");
  ICS_CHECK(k >= 1 && k <= n - 1, "ics_op_tsne_knn: k must be 1..n-1");
  ICS_CHECK((long long)n * k <= kTsneMaxEdges, "ics_op_tsne_knn: n * k above the limit of 2^28");
  for (size_t i = 0; i < (size_t)n * dim; ++i) ICS_CHECK(std::isfinite(x[i]), "ics_op_tsne_knn: x is not finite");
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  Layout L;
  const auto s_x = L.add<float>((size_t)n * dim);
  const auto s_i = L.add<int>((size_t)n * k);
  const auto s_d = L.add<double>((size_t)n * k);
  float* dx;
  int* di;
  double* dd;
  ICS_TRY(L.reserve(s_x, &dx, s_i, &di, s_d, &dd));
  ICS_TRY(L.upload(s_x, x, s_x.count, st));
  ICS_TRY(launch_knn(st, dx, n, dim, k, di, dd));
  ICS_TRY(L.download(idx, s_i, s_i.count, st));
  ICS_TRY(L.download(dist2, s_d, s_d.count, st));
  ICS_HIP(hipStreamSynchronize(st));
  return 0;
}

int ics_op_tsne_affinities(const double* dist2, int n, int k, double perplexity, double* cond_p) {
  ICS_CHECK(dist2 && cond_p, "ics_op_tsne_affinities: null argument");
  ICS_CHECK(n >= 1 && n <= kTsneMaxPoints, "ics_op_tsne_affinities: n must be 1.." + std::to_string(kTsneMaxPoints));
  ICS_CHECK(k >= 1 && (long long)n * k <= kTsneMaxEdges, "ics_op_tsne_affinities: k must be >= 1 and n * k <= 2^28");
  ICS_CHECK(std::isfinite(perplexity) && perplexity > 0.0, "ics_op_tsne_affinities: perplexity must be positive");
  for (size_t i = 0; i < (size_t)n * k; ++i)
    ICS_CHECK(std::isfinite(dist2[i]) && dist2[i] >= 0.0, "ics_op_tsne_affinities: dist2 must be finite and >= 0");
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  Layout L;
  const auto s_d = L.add<double>((size_t)n * k), s_p = L.add<double>((size_t)n * k);
  double *dd, *dp;
  ICS_TRY(L.reserve(s_d, &dd, s_p, &dp));
  ICS_TRY(L.upload(s_d, dist2, s_d.count, st));
  ICS_TRY(launch_affinities(st, dd, n, k, perplexity, dp));
  ICS_TRY(L.download(cond_p, s_p, s_p.count, st));
  ICS_HIP(hipStreamSynchronize(st));
  return 0;
}

// ---------------------------------------------------------------- handle
int ics_op_tsne_create(const ics_tsne_config* cfg, ics_tsne** out) {
  ICS_CHECK(cfg && out, "ics_op_tsne_create: null argument");
  ICS_CHECK(cfg->n_components == 2, "ics_op_tsne_create: n_components must be 2");
  ICS_CHECK(cfg->dim >= 1 && cfg->dim <= kTsneMaxDim, "ics_op_tsne_create: dim must be 1..4096");
  ICS_CHECK(cfg->capacity >= 2 && cfg->capacity <= kTsneMaxPoints,
            "ics_op_tsne_create: capacity must be 2.." + std::to_string(kTsneMaxPoints));
  ICS_CHECK(std::isfinite(cfg->perplexity) && cfg->perplexity > 0.0, "ics_op_tsne_create: perplexity must be positive");
  ICS_CHECK(std::isfinite(cfg->early_exaggeration) && cfg->early_exaggeration >= 1.0,
            "ics_op_tsne_create: early_exaggeration must be >= 1");
  ICS_CHECK(cfg->max_iter >= 1 && cfg->exaggeration_iter >= 0 && cfg->exaggeration_iter <= cfg->max_iter,
            "ics_op_tsne_create: need 0 <= exaggeration_iter <= max_iter, max_iter >= 1");
  ICS_CHECK(cfg->n_iter_check >= 1 && cfg->n_iter_without_progress >= 0,
            "ics_op_tsne_create: n_iter_check must be >= 1, n_iter_without_progress >= 0");
  ICS_CHECK(std::isfinite(cfg->min_grad_norm) && std::isfinite(cfg->learning_rate),
            "ics_op_tsne_create: min_grad_norm / learning_rate must be finite");
  ics_tsne* h = new ics_tsne();
  h->cfg = *cfg;
  auto fail = [&]() { (void)ics_op_tsne_destroy(h); return -1; };
  if (hipGetDevice(&h->device) != hipSuccess) { set_error("ics_op_tsne_create: hipGetDevice failed"); return fail(); }
  if (hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) != hipSuccess) {
    h->st = nullptr;
    set_error("ics_op_tsne_create: hipStreamCreateWithFlags failed");
    return fail();
  }
  void* p = nullptr;
  if (hipMalloc(&p, (size_t)cfg->capacity * cfg->dim * 4) != hipSuccess) {
    set_error("ics_op_tsne_create: out of device memory for " + std::to_string(cfg->capacity) + " codes");
    return fail();
  }
  h->codes = static_cast<float*>(p);
  *out = h;
  return 0;
}

int ics_op_tsne_destroy(ics_tsne* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  if (h->st) (void)hipStreamSynchronize(h->st);
  drop_state(h);
  if (h->codes) (void)hipFree(h->codes);
  if (h->st) (void)hipStreamDestroy(h->st);
  delete h;
  return 0;
}

int ics_op_tsne_append(ics_tsne* h, const float* codes, int rows) {
  ICS_TRY(handle_enter(h));
  ICS_CHECK(codes != nullptr, "ics_op_tsne_append: null codes");
  ICS_CHECK(rows >= 1 && rows <= h->cfg.capacity - h->count, "ics_op_tsne_append: rows exceed the handle's capacity");
  const size_t cnt = (size_t)rows * h->cfg.dim;
  for (size_t i = 0; i < cnt; ++i) ICS_CHECK(std::isfinite(codes[i]), "ics_op_tsne_append: codes are not finite");
  ICS_HIP(hipMemcpyAsync(h->codes + (size_t)h->count * h->cfg.dim, codes, cnt * 4, hipMemcpyHostToDevice, h->st));
  ICS_HIP(hipStreamSynchronize(h->st));
  h->count += rows;
  return 0;
}

int ics_op_tsne_get_codes(ics_tsne* h, float* out, int rows) {
  ICS_TRY(handle_enter(h));
  ICS_CHECK(out != nullptr, "ics_op_tsne_get_codes: null out");
  ICS_CHECK(rows >= 1 && rows <= h->count, "ics_op_tsne_get_codes: rows exceed the codes appended");
  ICS_HIP(hipMemcpyAsync(out, h->codes, (size_t)rows * h->cfg.dim * 4, hipMemcpyDeviceToHost, h->st));
  ICS_HIP(hipStreamSynchronize(h->st));
  return 0;
}

int ics_op_tsne_prepare(ics_tsne* h, const float* init, int init_rows, int init_cols, double seconds[3]) {
  ICS_TRY(handle_enter(h));
  const int n = h->count, dim = h->cfg.dim;
  ICS_CHECK(n >= 2, "ics_op_tsne_prepare: at least 2 codes are needed, the handle has " + std::to_string(n));
  ICS_CHECK(h->cfg.perplexity < (double)n, "ics_op_tsne_prepare: perplexity must be less than n_samples (" +
                                               std::to_string(n) + ")");
  ICS_TRY(check_init("ics_op_tsne_prepare", init, init_rows, init_cols, n));
  const int k = std::min(n - 1, (int)(3.0 * h->cfg.perplexity + 1.0));
  ICS_CHECK(k >= 1 && (long long)n * k <= kTsneMaxEdges, "ics_op_tsne_prepare: n * k above the limit of 2^28");
  // non-finite codes (the device-resident path is not seen by the host)
  Layout L;
  const auto s_flag = L.add<int>(1);
  const auto s_idx = L.add<int>((size_t)n * k);
  const auto s_dist = L.add<double>((size_t)n * k), s_p = L.add<double>((size_t)n * k);
  int *d_flag, *d_idx;
  double *d_dist, *d_p;
  ICS_TRY(L.reserve(s_flag, &d_flag, s_idx, &d_idx, s_dist, &d_dist, s_p, &d_p));
  ICS_TRY(L.fill(s_flag, 0, 1, h->st));
  ICS_LAUNCH(tsne_finite_kernel, dim3(1024), dim3(256), 0, h->st, h->codes, (size_t)n * dim, d_flag);
  int flag = 0;
  ICS_TRY(L.download(&flag, s_flag, 1, h->st));
  ICS_HIP(hipStreamSynchronize(h->st));
  ICS_CHECK(flag == 0, "ics_op_tsne_prepare: codes are not finite");

  auto t0 = std::chrono::steady_clock::now();
  ICS_TRY(launch_knn(h->st, h->codes, n, dim, k, d_idx, d_dist));
  ICS_HIP(hipStreamSynchronize(h->st));
  const double t_knn = seconds_since(t0);
  t0 = std::chrono::steady_clock::now();
  ICS_TRY(launch_affinities(h->st, d_dist, n, k, h->cfg.perplexity, d_p));
  ICS_HIP(hipStreamSynchronize(h->st));
  const double t_aff = seconds_since(t0);

  // P = (C + C^T) / sum: rows with ascending columns.  Row i takes its own k edges and, by a counting pass over the
  // edges in (row, rank) order, every edge that points at it; an (i, j) held both ways is C_ij + C_ji in both rows.
  t0 = std::chrono::steady_clock::now();
  std::vector<int> idx((size_t)n * k);
  std::vector<double> cp((size_t)n * k);
  ICS_TRY(L.download(idx.data(), s_idx, idx.size(), h->st));
  ICS_TRY(L.download(cp.data(), s_p, cp.size(), h->st));
  ICS_HIP(hipStreamSynchronize(h->st));
  for (size_t e = 0; e < idx.size(); ++e)
    ICS_CHECK(idx[e] >= 0 && idx[e] < n, "ics_op_tsne_prepare: neighbour index out of range");
  std::vector<long long> start((size_t)n + 1, 0);
  for (size_t e = 0; e < idx.size(); ++e) ++start[(size_t)idx[e] + 1];
  for (int i = 0; i < n; ++i) start[i + 1] += start[i] + k;       // row i: k forward + its incoming edges
  struct Edge { int col; double v; };
  std::vector<Edge> raw((size_t)start[n]);
  std::vector<long long> fill(start.begin(), start.end() - 1);
  for (int i = 0; i < n; ++i)
    for (int r = 0; r < k; ++r) raw[(size_t)fill[i]++] = Edge{idx[(size_t)i * k + r], cp[(size_t)i * k + r]};
  for (int i = 0; i < n; ++i)
    for (int r = 0; r < k; ++r) raw[(size_t)fill[idx[(size_t)i * k + r]]++] = Edge{i, cp[(size_t)i * k + r]};
  std::vector<long long> indptr((size_t)n + 1, 0);
  std::vector<int> indices;
  std::vector<double> vals;
  indices.reserve(raw.size()); vals.reserve(raw.size());
  double total = 0.0;
  for (int i = 0; i < n; ++i) {
    Edge* b = raw.data() + start[i];
    Edge* e = raw.data() + start[i + 1];
    std::stable_sort(b, e, [](const Edge& l, const Edge& r) { return l.col < r.col; });
    for (Edge* p = b; p < e;) {
      double v = p->v;
      Edge* q = p + 1;
      for (; q < e && q->col == p->col; ++q) v += q->v;
      indices.push_back(p->col); vals.push_back(v);
      total += v;
      p = q;
    }
    indptr[(size_t)i + 1] = (long long)indices.size();
  }
  total = std::max(total, DBL_EPSILON);
  for (double& v : vals) v /= total;
  ICS_TRY(install(h, n, indptr.data(), indices.data(), vals.data(), init));
  if (seconds) { seconds[0] = t_knn; seconds[1] = t_aff; seconds[2] = seconds_since(t0); }
  return 0;
}

int ics_op_tsne_set_graph(ics_tsne* h, int n, const int64_t* indptr, const int32_t* indices, const double* vals,
                          const float* init, int init_rows, int init_cols) {
  ICS_TRY(handle_enter(h));
  ICS_CHECK(indptr != nullptr, "ics_op_tsne_set_graph: null indptr");
  ICS_CHECK(n >= 2 && n <= h->cfg.capacity, "ics_op_tsne_set_graph: n must be 2..capacity");
  ICS_CHECK(indptr[0] == 0, "ics_op_tsne_set_graph: indptr[0] must be 0");
  for (int i = 0; i < n; ++i) ICS_CHECK(indptr[i + 1] >= indptr[i], "ics_op_tsne_set_graph: indptr decreases");
  ICS_CHECK(indptr[n] <= 2 * kTsneMaxEdges, "ics_op_tsne_set_graph: too many edges");
  ICS_CHECK((indices && vals) || indptr[n] == 0, "ics_op_tsne_set_graph: null indices / vals");
  for (int64_t e = 0; e < indptr[n]; ++e) {
    ICS_CHECK(indices[e] >= 0 && indices[e] < n, "ics_op_tsne_set_graph: column index out of range");
    ICS_CHECK(std::isfinite(vals[e]) && vals[e] >= 0.0, "ics_op_tsne_set_graph: values must be finite and >= 0");
  }
  ICS_TRY(check_init("ics_op_tsne_set_graph", init, init_rows, init_cols, n));
  static_assert(sizeof(long long) == sizeof(int64_t), "int64 layout");
  return install(h, n, reinterpret_cast<const long long*>(indptr), indices, vals, init);
}

int ics_op_tsne_get_graph(ics_tsne* h, int64_t* indptr, int32_t* indices, double* vals, size_t capacity, size_t* nnz) {
  ICS_TRY(handle_enter(h));
  ICS_CHECK(h->n > 0, "ics_op_tsne_get_graph: no graph yet (ics_op_tsne_prepare / ics_op_tsne_set_graph)");
  ICS_CHECK(nnz != nullptr, "ics_op_tsne_get_graph: null nnz");
  ICS_CHECK((indices == nullptr && vals == nullptr && indptr == nullptr && capacity == 0) ||
                (indices && vals && indptr && capacity >= h->nnz),
            "ics_op_tsne_get_graph: capacity below the number of entries, or a null array");
  *nnz = h->nnz;
  if (indices) {
    ICS_HIP(hipMemcpyAsync(indptr, h->indptr, ((size_t)h->n + 1) * 8, hipMemcpyDeviceToHost, h->st));
    ICS_HIP(hipMemcpyAsync(indices, h->indices, h->nnz * 4, hipMemcpyDeviceToHost, h->st));
    ICS_HIP(hipMemcpyAsync(vals, h->vals, h->nnz * 8, hipMemcpyDeviceToHost, h->st));
    ICS_HIP(hipStreamSynchronize(h->st));
  }
  return 0;
}

int ics_op_tsne_gradient(ics_tsne* h, const float* y, double exaggeration, float* grad, double* kl) {
  ICS_TRY(handle_enter(h));
  ICS_CHECK(h->n > 0, "ics_op_tsne_gradient: no graph yet (ics_op_tsne_prepare / ics_op_tsne_set_graph)");
  ICS_CHECK(y && grad && kl, "ics_op_tsne_gradient: null argument");
  ICS_CHECK(std::isfinite(exaggeration) && exaggeration > 0.0, "ics_op_tsne_gradient: exaggeration must be positive");
  const int n = h->n;
  for (size_t i = 0; i < (size_t)n * 2; ++i) ICS_CHECK(std::isfinite(y[i]), "ics_op_tsne_gradient: y is not finite");
  float* ybuf = h->y[h->cur ^ 1];                          // the buffer the next iteration overwrites anyway
  ICS_HIP(hipMemcpyAsync(ybuf, y, (size_t)n * 8, hipMemcpyHostToDevice, h->st));
  ICS_TRY(enqueue_gradient(h, ybuf, nullptr, h->grad, exaggeration, 0.f, true));
  ICS_LAUNCH(tsne_reduce2_kernel, dim3(1), dim3(1024), 0, h->st, h->klrow, (const double*)nullptr, n, h->red);
  double red[2] = {0.0, 0.0};
  std::vector<float> g((size_t)n * 2);
  ICS_HIP(hipMemcpyAsync(g.data(), h->grad, (size_t)n * 8, hipMemcpyDeviceToHost, h->st));
  ICS_HIP(hipMemcpyAsync(red, h->red, 16, hipMemcpyDeviceToHost, h->st));
  ICS_HIP(hipStreamSynchronize(h->st));
  std::memcpy(grad, g.data(), (size_t)n * 8);
  *kl = red[0];
  return 0;
}

int ics_op_tsne_run(ics_tsne* h, int iters, int* done) {
  ICS_TRY(handle_enter(h));
  ICS_CHECK(h->n > 0, "ics_op_tsne_run: no graph yet (ics_op_tsne_prepare / ics_op_tsne_set_graph)");
  ICS_CHECK(iters >= 0, "ics_op_tsne_run: iters must be >= 0");
  const ics_tsne_config& c = h->cfg;
  const int n = h->n;
  for (int step = 0; step < iters && !h->finished; ++step) {
    if (!h->phase2 && h->iter >= c.exaggeration_iter) {
      // TSNE._tsne's second call of _gradient_descent: fresh update / gains / best error
      h->phase2 = true;
      ICS_HIP(hipMemsetAsync(h->upd, 0, (size_t)n * 8, h->st));
      ICS_LAUNCH(tsne_fill_kernel, dim3((unsigned)((2 * (size_t)n + 255) / 256)), dim3(256), 0, h->st, h->gains,
                 (size_t)n * 2, 1.0f);
      h->best_error = DBL_MAX; h->best_iter = h->iter;
      if (h->iter >= c.max_iter) { h->finished = true; break; }
    }
    const int i = h->iter;
    const int phase_end = h->phase2 ? c.max_iter : c.exaggeration_iter;
    const bool check = (i + 1) % c.n_iter_check == 0;
    const bool want_error = check || i == phase_end - 1;
    const int no_progress = h->phase2 ? c.n_iter_without_progress : c.exaggeration_iter;
    ICS_TRY(enqueue_gradient(h, h->y[h->cur], h->y[h->cur ^ 1], nullptr, h->phase2 ? 1.0 : c.early_exaggeration,
                             h->phase2 ? 0.8f : 0.5f, want_error));
    h->cur ^= 1;
    h->last_iter = i;
    h->iter = i + 1;
    bool stop = false;
    if (want_error) {
      ICS_LAUNCH(tsne_reduce2_kernel, dim3(1), dim3(1024), 0, h->st, h->klrow, (const double*)h->gnrow, n, h->red);
      double red[2] = {0.0, 0.0};
      ICS_HIP(hipMemcpyAsync(red, h->red, 16, hipMemcpyDeviceToHost, h->st));
      ICS_HIP(hipStreamSynchronize(h->st));
      h->kl = red[0];
      if (check) {
        h->grad_norm = std::sqrt(red[1]);
        if (h->kl < h->best_error) { h->best_error = h->kl; h->best_iter = i; }
        else if (i - h->best_iter > no_progress) stop = true;
        if (h->grad_norm <= c.min_grad_norm) stop = true;
      }
    }
    if (stop) {
      // a stop inside the exaggeration phase sends scikit-learn on to the second phase at i + 1
      if (!h->phase2) {
        h->phase2 = true;
        ICS_HIP(hipMemsetAsync(h->upd, 0, (size_t)n * 8, h->st));
        ICS_LAUNCH(tsne_fill_kernel, dim3((unsigned)((2 * (size_t)n + 255) / 256)), dim3(256), 0, h->st, h->gains,
                   (size_t)n * 2, 1.0f);
        h->best_error = DBL_MAX; h->best_iter = h->iter;
      } else {
        h->finished = true;
      }
    }
    if (h->iter >= c.max_iter) h->finished = true;
  }
  ICS_HIP(hipGetLastError());
  ICS_HIP(hipStreamSynchronize(h->st));
  if (done) *done = h->finished ? 1 : 0;
  return 0;
}

int ics_op_tsne_read(ics_tsne* h, float* embedding, double* kl, double* grad_norm, int* n_iter, int* count) {
  ICS_TRY(handle_enter(h));
  if (embedding) {
    ICS_CHECK(h->n > 0, "ics_op_tsne_read: no embedding yet (ics_op_tsne_prepare / ics_op_tsne_set_graph)");
    ICS_HIP(hipMemcpyAsync(embedding, h->y[h->cur], (size_t)h->n * 8, hipMemcpyDeviceToHost, h->st));
    ICS_HIP(hipStreamSynchronize(h->st));
  }
  if (kl) *kl = h->kl;
  if (grad_norm) *grad_norm = h->grad_norm;
  if (n_iter) *n_iter = h->last_iter;
  if (count) *count = h->n > 0 ? h->n : h->count;
  return 0;
}

}  // extern "C"
