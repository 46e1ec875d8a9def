// Connected-component post-processing of the U-Net's outputs on the device (gfx950 / MI355X only) -- the part of
// /root/reference/watershed.py that is integer work over a label volume:
//   * segment_nuclei step 1 (watershed.py:52-56): measure.label(binary, connectivity=1) = 6-connected components,
//     numbered in raster order of their first voxel, and the size filter  count > 3;
//   * the result matrix R when every kept component takes the `convexity >= min_convexity` branch
//     (watershed.py:85-92): kept components renumbered 1..n in ascending label order, everything else 0;
//   * centroids + majority_vote (watershed.py:153-187): per region the most frequent non-zero species (ties -> the
//     larger species id: a stable sort by count over ascending ids, last element) and the mean voxel index.
// NOT here: the convex-hull test (watershed.py:80) and the marker watershed that splits non-convex components
// (watershed.py:96-150) -- both are skimage routines that cannot be pinned in this image (skimage absent).
//
// Everything is integer: union-find with atomicMin on linear voxel indices (the root of a component is its smallest
// index, which is also what fixes the raster-order numbering), integer atomic sums, counts and histograms -- results
// are bit-exact and independent of scheduling.  Work is a few passes over 1 byte + 4 bytes per voxel (HBM/L2-bound,
// 1-2 M voxels per call).
#include "common.h"
#include "segment.h"
#include "scratch.h"
#include "../../include/icsg3d.h"
#include <algorithm>
#include <atomic>
#include <climits>
#include <condition_variable>
#include <functional>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <thread>
#include <tuple>
#include <utility>
#include <unistd.h>
#include <vector>

namespace ics {
namespace {

constexpr unsigned kNone = 0xffffffffu;

__device__ __forceinline__ unsigned seg_find(const unsigned* lab, unsigned i) {
  unsigned p;
  while ((p = __hip_atomic_load(lab + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != i) i = p;
  return i;
}

// attach the larger root under the smaller one (the root of a finished component is its minimum index)
__device__ __forceinline__ void seg_unite(unsigned* lab, unsigned a, unsigned b) {
  while (true) {
    a = seg_find(lab, a);
    b = seg_find(lab, b);
    if (a == b) return;
    if (a < b) { const unsigned t = a; a = b; b = t; }
    const unsigned old = atomicMin(lab + a, b);
    if (old == a) return;
    a = old;                              // somebody else re-parented a meanwhile: continue from there
  }
}

__global__ void seg_init_kernel(const unsigned char* __restrict__ mask, unsigned* __restrict__ lab, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) lab[i] = mask[i] ? (unsigned)i : kNone;
}

// one thread per voxel: unions with the -x, -y, -z neighbours inside the same sample (6-connectivity)
__global__ void seg_merge_kernel(const unsigned char* __restrict__ mask, unsigned* __restrict__ lab, int lgd, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !mask[i]) return;
  const unsigned d = 1u << lgd, m = d - 1;
  const unsigned x = (unsigned)i & m, y = ((unsigned)i >> lgd) & m, z = ((unsigned)i >> (2 * lgd)) & m;
  if (x > 0 && mask[i - 1]) seg_unite(lab, (unsigned)i, (unsigned)i - 1);
  if (y > 0 && mask[i - d]) seg_unite(lab, (unsigned)i, (unsigned)i - d);
  if (z > 0 && mask[i - d * d]) seg_unite(lab, (unsigned)i, (unsigned)(i - (size_t)d * d));
}

// path compression to the root + component sizes (stored at the root's slot)
__global__ void seg_flatten_kernel(unsigned* __restrict__ lab, unsigned* __restrict__ size, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || lab[i] == kNone) return;
  const unsigned r = seg_find(lab, (unsigned)i);
  lab[i] = r;                             // roots keep lab[r] == r, so concurrent finds stay correct
  atomicAdd(size + r, 1u);
}

// one workgroup per sample: raster-order ranks of the component roots.  rank[root] = 1-based number among the KEPT
// components (size > min_voxels), 0 for dropped ones; counts[b] = {all components, kept components}.
__global__ __launch_bounds__(1024) void seg_rank_kernel(const unsigned* __restrict__ lab, const unsigned* __restrict__ size,
                                                        unsigned* __restrict__ rank, int per, int min_voxels,
                                                        int* __restrict__ counts) {
  __shared__ unsigned s_all[1024], s_keep[1024];
  const int b = blockIdx.x, t = threadIdx.x;
  const int chunk = per / 1024;                         // per = d^3 >= 4096: a multiple of 1024
  const size_t base = (size_t)b * per + (size_t)t * chunk;
  unsigned na = 0, nk = 0;
  for (int j = 0; j < chunk; ++j) {
    const size_t i = base + j;
    if (lab[i] == (unsigned)i) { ++na; nk += size[i] > (unsigned)min_voxels; }
  }
  s_all[t] = na; s_keep[t] = nk;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {            // inclusive scan (Hillis-Steele)
    const unsigned a = t >= off ? s_all[t - off] : 0, k = t >= off ? s_keep[t - off] : 0;
    __syncthreads();
    s_all[t] += a; s_keep[t] += k;
    __syncthreads();
  }
  unsigned k0 = s_keep[t] - nk;
  for (int j = 0; j < chunk; ++j) {
    const size_t i = base + j;
    if (lab[i] == (unsigned)i) rank[i] = size[i] > (unsigned)min_voxels ? ++k0 : 0u;
  }
  if (t == 1023) { counts[2 * b] = (int)s_all[t]; counts[2 * b + 1] = (int)s_keep[t]; }
}

// R volume + per-region integer statistics: stats[b][a] = {species, voxels, sum z, sum y, sum x, z0, y0, x0, z1, y1, x1}
// (bounding box half-open like skimage's regionprops), hist[b][a][species]
// 13 of the 26 directions with components in {-1, 0, 1} (the others are their negatives): the ORDER is the one
// icsg3d_amd/watershed.py builds with itertools.product((-1, 0, 1), repeat=3) filtered by d > (0, 0, 0)
__constant__ int kDopDir[13][3] = {{0, 0, 1}, {0, 1, -1}, {0, 1, 0}, {0, 1, 1}, {1, -1, -1}, {1, -1, 0}, {1, -1, 1},
                                   {1, 0, -1}, {1, 0, 0}, {1, 0, 1}, {1, 1, -1}, {1, 1, 0}, {1, 1, 1}};
constexpr int kSupInts = 26;     // per region: max of d.p for the 13 directions, then min

__global__ void seg_stats_kernel(const unsigned* __restrict__ lab, const unsigned* __restrict__ rank,
                                 const unsigned char* __restrict__ species, int lgd, int per, size_t n, int max_atoms,
                                 int nbins, int* __restrict__ R, int* __restrict__ stats, unsigned* __restrict__ hist,
                                 int* __restrict__ sup, unsigned long long* __restrict__ mom) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned l = lab[i];
  const unsigned r = l == kNone ? 0u : rank[l];
  if (R) R[i] = (int)r;
  if (r == 0 || r > (unsigned)max_atoms) return;
  const unsigned d = 1u << lgd, m = d - 1;
  const int x = (int)((unsigned)i & m), y = (int)(((unsigned)i >> lgd) & m), z = (int)(((unsigned)i >> (2 * lgd)) & m);
  const size_t b = i / (size_t)per;
  int* s = stats + (b * max_atoms + (r - 1)) * kSegStatInts;
  atomicAdd(s + 1, 1);
  atomicAdd(s + 2, z); atomicAdd(s + 3, y); atomicAdd(s + 4, x);
  atomicMin(s + 5, z); atomicMin(s + 6, y); atomicMin(s + 7, x);
  atomicMax(s + 8, z + 1); atomicMax(s + 9, y + 1); atomicMax(s + 10, x + 1);
  const unsigned sp = species[i];
  if (sp != 0 && sp < (unsigned)nbins) atomicAdd(hist + (b * max_atoms + (r - 1)) * nbins + sp, 1u);
  if (sup != nullptr) {
    // what the convexity test of segment_nuclei (watershed.py:80-83) can be decided from without a convex hull: the
    // support values of the component along 26 directions (its discrete orientation polytope contains the hull) and the
    // second moments of its voxel coordinates (coplanar <=> the 3 x 3 scatter matrix is singular) -- integers, exact
    int* su = sup + (b * max_atoms + (r - 1)) * kSupInts;
#pragma unroll
    for (int k = 0; k < 13; ++k) {
      const int pr = kDopDir[k][0] * z + kDopDir[k][1] * y + kDopDir[k][2] * x;
      atomicMax(su + k, pr);
      atomicMin(su + 13 + k, pr);
    }
    unsigned long long* mo = mom + (b * max_atoms + (r - 1)) * 6;
    atomicAdd(mo + 0, (unsigned long long)(z * z)); atomicAdd(mo + 1, (unsigned long long)(y * y));
    atomicAdd(mo + 2, (unsigned long long)(x * x)); atomicAdd(mo + 3, (unsigned long long)(z * y));
    atomicAdd(mo + 4, (unsigned long long)(z * x)); atomicAdd(mo + 5, (unsigned long long)(y * x));
  }
}

__global__ void seg_sup_init_kernel(int* __restrict__ sup, unsigned long long* __restrict__ mom, size_t natoms) {
  const size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= natoms) return;
  for (int k = 0; k < 13; ++k) { sup[a * kSupInts + k] = -(1 << 30); sup[a * kSupInts + 13 + k] = 1 << 30; }
  for (int k = 0; k < 6; ++k) mom[a * 6 + k] = 0ull;
}

// One wave per region: the number of grid points of the region's bounding box inside its 26-direction polytope, on doubled
// coordinates (the reference's convex_hull_image offsets every voxel by +-0.5 along one axis at a time: a support value
// moves by max_k |d_k| / 2 = 1/2):  2 min_p(d.p) - 1 <= 2 d.g <= 2 max_p(d.p) + 1  for the 13 directions.  An UPPER bound
// of np.count_nonzero(convex_hull_image(component)).  bounds[a] = {count, sum zz, yy, xx, zy, zx, yx, 0}.
__global__ __launch_bounds__(64) void seg_dop_kernel(const int* __restrict__ stats, const int* __restrict__ sup,
                                                     const unsigned long long* __restrict__ mom,
                                                     long long* __restrict__ bounds) {
  const size_t a = blockIdx.x;
  const int* s = stats + a * kSegStatInts;
  long long* o = bounds + a * 8;
  const int nvox = s[1];
  if (nvox <= 0) {
    if (threadIdx.x < 8) o[threadIdx.x] = 0;
    return;
  }
  const int z0 = s[5], y0 = s[6], x0 = s[7], D = s[8] - z0, H = s[9] - y0, W = s[10] - x0;
  int hi[13], lo[13];
#pragma unroll
  for (int k = 0; k < 13; ++k) { hi[k] = 2 * sup[a * kSupInts + k] + 1; lo[k] = 2 * sup[a * kSupInts + 13 + k] - 1; }
  int cnt = 0;
  for (int i = threadIdx.x; i < D * H * W; i += 64) {
    const int x = x0 + i % W, y = y0 + (i / W) % H, z = z0 + i / (W * H);
    bool in = true;
#pragma unroll
    for (int k = 0; k < 13; ++k) {
      const int g = 2 * (kDopDir[k][0] * z + kDopDir[k][1] * y + kDopDir[k][2] * x);
      in = in && g <= hi[k] && g >= lo[k];
    }
    cnt += in ? 1 : 0;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d);
  if (threadIdx.x == 0) {
    o[0] = cnt;
    for (int k = 0; k < 6; ++k) o[1 + k] = (long long)mom[a * 6 + k];
    o[7] = 0;
  }
}

__global__ void seg_stats_init_kernel(int* __restrict__ stats, size_t natoms, int d) {
  const size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= natoms) return;
  int* s = stats + a * kSegStatInts;
  s[0] = s[1] = s[2] = s[3] = s[4] = 0;
  s[5] = s[6] = s[7] = d;
  s[8] = s[9] = s[10] = 0;
}

// the same statistics for an arbitrary label volume R [D][H][W] (labels 1..nlab; the result of segment_nuclei)
__global__ void region_stats_kernel(const int* __restrict__ R, const unsigned char* __restrict__ species, int D, int H,
                                    int W, int nlab, int nbins, int* __restrict__ stats, unsigned* __restrict__ hist) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D * H * W) return;
  const int r = R[i];
  if (r <= 0 || r > nlab) return;
  const int x = i % W, y = (i / W) % H, z = i / (W * H);
  int* s = stats + (size_t)(r - 1) * kSegStatInts;
  atomicAdd(s + 1, 1);
  atomicAdd(s + 2, z); atomicAdd(s + 3, y); atomicAdd(s + 4, x);
  atomicMin(s + 5, z); atomicMin(s + 6, y); atomicMin(s + 7, x);
  atomicMax(s + 8, z + 1); atomicMax(s + 9, y + 1); atomicMax(s + 10, x + 1);
  const unsigned sp = species[i];
  if (sp != 0 && sp < (unsigned)nbins) atomicAdd(hist + (size_t)(r - 1) * nbins + sp, 1u);
}

// majority_vote (watershed.py:153-163): most frequent non-zero species; equal counts -> the larger id
__global__ void seg_vote_kernel(const unsigned* __restrict__ hist, int nbins, size_t natoms, int* __restrict__ stats) {
  const size_t a = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= natoms) return;
  const unsigned* h = hist + a * nbins;
  unsigned best = 0, bestc = 0;
  for (int sp = 1; sp < nbins; ++sp) {
    const unsigned c = h[sp];
    if (c != 0 && c >= bestc) { best = (unsigned)sp; bestc = c; }
  }
  stats[a * kSegStatInts] = (int)best;
}


// ======================================================================================================================
// segment_nuclei's non-convex branch and its recursion (watershed.py:40-150), one workgroup per box
// ======================================================================================================================
// A "box" is a small dense int32 volume [D][H][W] (a component cropped to its bounding box, or a watershed result that is
// segmented again): D, H, W <= 64 for these kernels (larger boxes take the host forms below).  The scikit-image 0.17.2
// routines the reference calls on it are restated in oracle/watershed_ref.py (PARITY UNPINNED: skimage absent); these
// kernels are held to that file bit for bit.
struct BoxDesc {
  long long off;         // element offset of the box in the flat input / output arrays
  int D, H, W, cl;       // extents; cl: the component's label value (split kernel)
  long long heap_off;    // element offset of this box's heap scratch (split kernel)
};

__device__ __forceinline__ int ld_i(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_i(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Connected components of EQUAL non-zero value (measure.label on an integer image) by min-index propagation + pointer
// jumping inside one workgroup: lab[i] ends as the smallest linear index of i's component (0-based; -1 = background),
// which is also what orders the final numbering (raster order of the first voxel).  conn26: 26-neighbourhood.
// All label traffic bypasses the vector L1 (agent-scope relaxed atomics): the sweeps of different waves see each other.
__device__ void box_label_roots(const int* __restrict__ val, int* lab, int D, int H, int W, bool conn26, int* s_flag) {
  const int V = D * H * W, tid = threadIdx.x, nt = blockDim.x;
  for (int i = tid; i < V; i += nt) st_i(lab + i, val[i] != 0 ? i : -1);
  __syncthreads();
  while (true) {                                   // labels only ever decrease: terminates
    if (tid == 0) *s_flag = 0;
    __syncthreads();
    int changed = 0;
    for (int i = tid; i < V; i += nt) {
      const int v = val[i];
      if (v == 0) continue;
      const int x = i % W, y = (i / W) % H, z = i / (W * H);
      int best = ld_i(lab + i);
      const int cur = best;
      const int r = conn26 ? 1 : 0;
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            if (dz == 0 && dy == 0 && dx == 0) continue;
            if (!r && (dz != 0) + (dy != 0) + (dx != 0) != 1) continue;
            const int zz = z + dz, yy = y + dy, xx = x + dx;
            if (zz < 0 || zz >= D || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            const int j = (zz * H + yy) * W + xx;
            if (val[j] != v) continue;
            const int lj = ld_i(lab + j);
            best = lj < best ? lj : best;
          }
      const int lb = ld_i(lab + best);            // pointer jumping: the label of my label
      best = lb < best ? lb : best;
      if (best < cur) { st_i(lab + i, best); changed = 1; }
    }
    if (changed) *s_flag = 1;
    __syncthreads();
    const int any = *s_flag;
    __syncthreads();
    if (!any) break;
  }
}

// raster-order ranks of the roots (lab[i] == i) -> lab[i] = 1-based component number, 0 = background; returns the count
// (valid in every thread).  scratch: blockDim.x ints of LDS.
__device__ int box_rank_labels(int* lab, int V, int* s_scan) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int chunk = (V + nt - 1) / nt, lo = tid * chunk, hi = lo + chunk < V ? lo + chunk : V;
  int cnt = 0;
  for (int i = lo; i < hi; ++i) cnt += ld_i(lab + i) == i;
  s_scan[tid] = cnt;
  __syncthreads();
  for (int off = 1; off < nt; off <<= 1) {
    const int a = tid >= off ? s_scan[tid - off] : 0;
    __syncthreads();
    s_scan[tid] += a;
    __syncthreads();
  }
  const int total = s_scan[nt - 1];
  int k = s_scan[tid] - cnt;
  __syncthreads();
  // roots first get their NEGATIVE rank code (-(rank) - 1 <= -2) so that root slots stay recognisable while the other
  // voxels still look their root up
  for (int i = lo; i < hi; ++i)
    if (ld_i(lab + i) == i) st_i(lab + i, -(++k) - 1);
  __syncthreads();
  for (int i = tid; i < V; i += nt) {
    const int l = ld_i(lab + i);
    if (l >= 0) {                                  // non-root foreground voxel: l = root index (root != i)
      const int code = ld_i(lab + l);
      st_i(lab + i, code);                         // still negative: converted below
    }
  }
  __syncthreads();
  for (int i = tid; i < V; i += nt) {
    const int l = ld_i(lab + i);
    st_i(lab + i, l == -1 ? 0 : -(l + 1));
  }
  __syncthreads();
  return total;
}

// measure.label(vol, connectivity) per box + per-label {count, z0, y0, x0, z1, y1, x1} (half-open): stats[box][label-1][7]
__global__ __launch_bounds__(1024) void label_boxes_kernel(const int* __restrict__ vols, const BoxDesc* __restrict__ desc,
                                                            int conn26, int max_labels, int* __restrict__ labels,
                                                            int* __restrict__ nlabels, int* __restrict__ stats) {
  __shared__ int s_flag;
  __shared__ int s_scan[1024];
  const BoxDesc d = desc[blockIdx.x];
  const int V = d.D * d.H * d.W, tid = threadIdx.x, nt = blockDim.x;
  const int* val = vols + d.off;
  int* lab = labels + d.off;
  box_label_roots(val, lab, d.D, d.H, d.W, conn26 != 0, &s_flag);
  const int n = box_rank_labels(lab, V, s_scan);
  if (tid == 0) nlabels[blockIdx.x] = n;
  int* st = stats + (size_t)blockIdx.x * max_labels * 7;
  const int nst = n < max_labels ? n : max_labels;
  for (int a = tid; a < nst; a += nt) {
    int* s = st + a * 7;
    st_i(s, 0); st_i(s + 1, d.D); st_i(s + 2, d.H); st_i(s + 3, d.W); st_i(s + 4, 0); st_i(s + 5, 0); st_i(s + 6, 0);
  }
  __syncthreads();
  for (int i = tid; i < V; i += nt) {
    const int l = ld_i(lab + i);
    if (l <= 0 || l > max_labels) continue;
    const int x = i % d.W, y = (i / d.W) % d.H, z = i / (d.W * d.H);
    int* s = st + (l - 1) * 7;
    atomicAdd(s, 1);
    atomicMin(s + 1, z); atomicMin(s + 2, y); atomicMin(s + 3, x);
    atomicMax(s + 4, z + 1); atomicMax(s + 5, y + 1); atomicMax(s + 6, x + 1);
  }
}

// ---- skimage's watershed heap (oracle/watershed_ref.py::_Heap): an entry is {key = (image level << 31) | age, index},
// two 32-bit words; `smaller` compares the key only and is strict.
struct WsHeap {
  unsigned* key;   // [cap]
  unsigned* idx;   // [cap]
  int n;
  __device__ __forceinline__ void push(unsigned k, unsigned ix) {
    int child = n++;
    key[child] = k; idx[child] = ix;
    while (child > 0) {
      const int parent = (child + 1) / 2 - 1;
      const unsigned kc = key[child], kp = key[parent];
      if (kc < kp) {
        const unsigned ic = idx[child], ip = idx[parent];
        key[child] = kp; idx[child] = ip; key[parent] = kc; idx[parent] = ic;
        child = parent;
      } else break;
    }
  }
  __device__ __forceinline__ unsigned pop() {      // returns the index of the smallest entry
    const unsigned top = idx[0];
    --n;
    if (n == 0) return top;
    key[0] = key[n]; idx[0] = idx[n];
    int i = 0;
    while (true) {
      const int l = 2 * i + 1, r = 2 * i + 2;
      int smallest = i;
      if (l < n) {
        if (key[l] < key[i]) smallest = l;
        if (r < n && key[r] < key[smallest]) smallest = r;
      } else break;
      if (smallest == i) break;
      const unsigned ks = key[smallest], is = idx[smallest];
      key[smallest] = key[i]; idx[smallest] = idx[i]; key[i] = ks; idx[i] = is;
      i = smallest;
    }
    return top;
  }
};

// watershed.py:95-110 for one non-convex component in its bounding box (values {0, cl}); wss out = labels 2.. or 0
// (before the reference's max_class shift).  tie: 0 = skimage's heap order among equal (value, age) keys, 1 = FIFO.
// work: int scratch [4][V] per box (fg / markers, bg, root labels, unused); heap scratch 2 x V unsigned per box.
__global__ __launch_bounds__(1024) void ws_split_kernel(const int* __restrict__ boxes, const BoxDesc* __restrict__ desc,
                                                         int tie, int* __restrict__ work, unsigned* __restrict__ heap_mem,
                                                         int* __restrict__ wss_out) {
  __shared__ int s_flag;
  __shared__ int s_scan[1024];
  // The flood is sequential (one thread emulates skimage's heap operation by operation); with its heap and label array in
  // global memory every step was a chain of L2 round trips (38 ms for the slowest box of a level).  Boxes of up to
  // kWsLdsVox voxels -- every realistic atom pair; the whole-sample blobs of random-weight masks do not fit -- run it in LDS:
  // key [V] | index [V] | labels [V] = 12 bytes per voxel.
  constexpr int kWsLdsVox = 12288;
  __shared__ unsigned s_mem[3 * kWsLdsVox];
  const BoxDesc d = desc[blockIdx.x];
  const int D = d.D, H = d.H, W = d.W, V = D * H * W, tid = threadIdx.x, nt = blockDim.x, cl = d.cl;
  const int* val = boxes + d.off;
  int* fg = work + d.off * 4;                      // [V]   eroded image (4 ints of scratch per voxel, three used)
  int* bgm = fg + V;                               // [V]   dilated image
  int* lab = bgm + V;                              // [V]   labels of fg (26-connectivity)
  int* out = wss_out + d.off;
  // erosion / dilation with ball(1) = the 7-voxel cross; out-of-box neighbours are ignored (scipy 'reflect' at radius 1)
  for (int i = tid; i < V; i += nt) {
    const int x = i % W, y = (i / W) % H, z = i / (W * H);
    int mn = val[i], mx = val[i];
    if (z > 0) { const int v = val[i - H * W]; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
    if (z < D - 1) { const int v = val[i + H * W]; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
    if (y > 0) { const int v = val[i - W]; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
    if (y < H - 1) { const int v = val[i + W]; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
    if (x > 0) { const int v = val[i - 1]; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
    if (x < W - 1) { const int v = val[i + 1]; mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
    fg[i] = mn; bgm[i] = mx;
  }
  __threadfence_block();
  __syncthreads();
  box_label_roots(fg, lab, D, H, W, true, &s_flag);     // measure.label(fg): full connectivity
  box_rank_labels(lab, V, s_scan);
  // markers = label + 1; markers[unknown == 1] = 0 -- the reference compares (bg - fg) against 1, not against cl
  int zeros = 0;
  for (int i = tid; i < V; i += nt) {
    int m = ld_i(lab + i) + 1;
    if (bgm[i] - fg[i] == 1) { m = 0; zeros = 1; }
    st_i(out + i, m);
  }
  if (tid == 0) s_flag = 0;
  __syncthreads();
  if (zeros) s_flag = 1;
  __syncthreads();
  const bool flood = s_flag != 0;
  (void)cl;
  const bool in_lds = V <= kWsLdsVox;
  int* fl = in_lds ? reinterpret_cast<int*>(s_mem + 2 * V) : out;     // the label array the flood works on
  if (flood && in_lds) {
    for (int i = tid; i < V; i += nt) fl[i] = ld_i(out + i);
    __syncthreads();
  }
  if (flood && tid == 0) {
    // sequential priority flood (skimage _watershed_cy.pyx, restated in oracle/watershed_ref.py::watershed_flood)
    WsHeap hp{in_lds ? s_mem : heap_mem + d.heap_off * 2, in_lds ? s_mem + V : heap_mem + d.heap_off * 2 + V, 0};
    // key = (image level << 31) | age: two image values (0 < cl), every marker enters with age 0 in raster order.
    // FIFO tie rule (tie = 1): the markers carry their raster rank instead, and real ages start above every rank.
    // (only this thread touches fl from here to the barrier: plain accesses, in LDS or -- large boxes -- through L2)
    auto ldl = [&](int i) { return in_lds ? fl[i] : ld_i(fl + i); };
    auto stl = [&](int i, int v) { if (in_lds) fl[i] = v; else st_i(fl + i, v); };
    unsigned seq = 0;
    for (int i = 0; i < V; ++i)
      if (ldl(i) != 0) hp.push(((val[i] != 0 ? 1u : 0u) << 31) | (tie ? seq++ : 0u), (unsigned)i);
    unsigned age = tie ? (unsigned)V + 1u : 1u;
    const int nb[6] = {-H * W, -W, -1, 1, W, H * W};
    while (hp.n > 0) {
      const int i = (int)hp.pop();
      const int x = i % W, y = (i / W) % H, z = i / (W * H);
      const bool ok[6] = {z > 0, y > 0, x > 0, x < W - 1, y < H - 1, z < D - 1};
      const int li = ldl(i);
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        if (!ok[k]) continue;
        const int j = i + nb[k];
        if (ldl(j) != 0) continue;
        ++age;
        stl(j, li);
        hp.push(((val[j] != 0 ? 1u : 0u) << 31) | age, (unsigned)j);
      }
    }
  }
  __syncthreads();
  if (flood && in_lds) {
    for (int i = tid; i < V; i += nt) st_i(out + i, fl[i]);
    __syncthreads();
  }
  for (int i = tid; i < V; i += nt) {
    const int m = ld_i(out + i);
    st_i(out + i, m == 1 ? 0 : m);                 // wss[wss == 1] = 0
  }
}

}  // namespace

size_t segment_workspace_bytes(int B, int d, int max_atoms, int nbins) {
  const size_t n = (size_t)B * d * d * d;
  return n * 4 * 3 + (size_t)B * max_atoms * ((size_t)kSegStatInts * 4 + (size_t)nbins * 4) + (size_t)B * 8 + 256 +
         (size_t)B * max_atoms * ((size_t)kSupInts * 4 + 6 * 8 + 8 * 8) + 64;     // convexity bounds (optional)
}

int launch_segment_atoms(hipStream_t st, const unsigned char* mask, const unsigned char* species, int B, int d,
                         int min_voxels, int max_atoms, int nbins, void* workspace, size_t workspace_bytes, int* d_R,
                         int** d_counts, int** d_stats, long long** d_bounds) {
  int lgd = 0;
  while ((1 << lgd) < d) ++lgd;
  ICS_CHECK((1 << lgd) == d && d >= 16 && d <= 256, "grid must be a power of two in [16, 256]");
  ICS_CHECK(B >= 1 && max_atoms >= 1 && nbins >= 2 && nbins <= 256 && min_voxels >= 0, "bad segmentation arguments");
  ICS_CHECK(workspace_bytes >= segment_workspace_bytes(B, d, max_atoms, nbins), "segmentation workspace too small");
  const size_t n = (size_t)B * d * d * d;
  ICS_CHECK(n < (1ull << 31), "volume too large for 32-bit voxel indices");
  const int per = d * d * d;
  unsigned* lab = reinterpret_cast<unsigned*>(workspace);
  unsigned* size = lab + n;
  unsigned* rank = size + n;
  int* stats = reinterpret_cast<int*>(rank + n);
  unsigned* hist = reinterpret_cast<unsigned*>(stats + (size_t)B * max_atoms * kSegStatInts);
  int* counts = reinterpret_cast<int*>(hist + (size_t)B * max_atoms * nbins);
  const size_t natoms = (size_t)B * max_atoms;
  // optional convexity bounds: 8-byte aligned behind the counts
  uintptr_t bp = (reinterpret_cast<uintptr_t>(counts + (size_t)B * 2) + 63) & ~(uintptr_t)63;
  long long* bounds = reinterpret_cast<long long*>(bp);
  unsigned long long* mom = reinterpret_cast<unsigned long long*>(bounds + natoms * 8);
  int* sup = reinterpret_cast<int*>(mom + natoms * 6);
  const bool want_bounds = d_bounds != nullptr;
  const unsigned gv = (unsigned)((n + 255) / 256), ga = (unsigned)((natoms + 255) / 256);
  ICS_HIP(hipMemsetAsync(size, 0, n * 4, st));
  ICS_HIP(hipMemsetAsync(hist, 0, natoms * nbins * 4, st));
  ICS_HIP(hipMemsetAsync(counts, 0, (size_t)B * 2 * 4, st));
  ICS_LAUNCH(seg_init_kernel, dim3(gv), dim3(256), 0, st, mask, lab, n);
  ICS_LAUNCH(seg_stats_init_kernel, dim3(ga), dim3(256), 0, st, stats, natoms, d);
  ICS_LAUNCH(seg_merge_kernel, dim3(gv), dim3(256), 0, st, mask, lab, lgd, n);
  ICS_LAUNCH(seg_flatten_kernel, dim3(gv), dim3(256), 0, st, lab, size, n);
  ICS_LAUNCH(seg_rank_kernel, dim3(B), dim3(1024), 0, st, lab, size, rank, per, min_voxels, counts);
  if (want_bounds) ICS_LAUNCH(seg_sup_init_kernel, dim3(ga), dim3(256), 0, st, sup, mom, natoms);
  ICS_LAUNCH(seg_stats_kernel, dim3(gv), dim3(256), 0, st, lab, rank, species, lgd, per, n, max_atoms, nbins,
                     d_R, stats, hist, want_bounds ? sup : nullptr, want_bounds ? mom : nullptr);
  ICS_LAUNCH(seg_vote_kernel, dim3(ga), dim3(256), 0, st, hist, nbins, natoms, stats);
  if (want_bounds) {
    ICS_LAUNCH(seg_dop_kernel, dim3((unsigned)natoms), dim3(64), 0, st, stats, sup, mom, bounds);
    *d_bounds = bounds;
  }
  ICS_HIP(hipGetLastError());
  *d_counts = counts;
  *d_stats = stats;
  return 0;
}

}  // namespace ics

namespace ics {

// Box extents: the two box kernels run one workgroup per box and propagate labels by sweeps over the whole box, which is
// only sensible up to 64 per axis; the host forms (label, split, component bounds) take whole d^3 grids up to 256.
constexpr int kBoxDeviceMax = 64;
constexpr int kBoxHostMax = 256;

// Host-side batching: `dims` [nbox][3] (D, H, W), boxes laid out back to back in `vols`; every extent in [1, max_ext].
static int box_descs(const int* dims, const int* cls, int nbox, int max_ext, std::vector<BoxDesc>* out, size_t* total) {
  out->resize(nbox);
  size_t off = 0;
  for (int b = 0; b < nbox; ++b) {
    const int D = dims[3 * b], H = dims[3 * b + 1], W = dims[3 * b + 2];
    ICS_CHECK(D >= 1 && H >= 1 && W >= 1 && D <= max_ext && H <= max_ext && W <= max_ext,
              "box " + std::to_string(b) + ": extents must be in [1, " + std::to_string(max_ext) + "]");
    (*out)[b] = BoxDesc{(long long)off, D, H, W, cls ? cls[b] : 0, (long long)off};
    off += (size_t)D * H * W;
  }
  ICS_CHECK(off < (1ull << 31), "boxes too large for 32-bit voxel offsets");
  *total = off;
  return 0;
}
static bool box_fits_device(const BoxDesc& d) { return d.D <= kBoxDeviceMax && d.H <= kBoxDeviceMax && d.W <= kBoxDeviceMax; }
// ICSG3D_LABEL_HOST=1: every box of ics_op_label_boxes goes to the host labeller (read per call: tests flip it)
static bool label_host_forced() {
  const char* e = getenv("ICSG3D_LABEL_HOST");
  return e != nullptr && atoi(e) != 0;
}

// ---- a persistent pool of host threads for the box-level host operations below (round 6).  They are called several times per
// recursion level with a few milliseconds of work each; spawning up to 64 std::threads per call cost 1 - 2 ms of that.  The
// pool is created on first use, never destroyed (its threads are detached and die with the process: no static-destruction
// order to get wrong), re-created after a fork (the child has none of the parent's threads), and used by one call at a time.
namespace {
class HostPool {
 public:
  static HostPool& get() {
    static std::mutex mu;
    static HostPool* pool = nullptr;
    std::lock_guard<std::mutex> lk(mu);
    if (pool == nullptr || pool->pid_ != getpid()) pool = new HostPool();     // (a forked child leaks the parent's object)
    return *pool;
  }
  int max_threads() const { return nmax_; }
  // fn() on `n` threads (the caller is one of them); returns when all have finished.  fn pulls its work from an atomic counter.
  void run(int n, const std::function<void()>& fn) {
    n = std::max(1, std::min(n, nmax_));
    if (n == 1) { fn(); return; }
    std::lock_guard<std::mutex> one_call(run_mu_);
    {
      std::lock_guard<std::mutex> lk(mu_);
      job_ = &fn; want_ = n - 1; started_ = 0; finished_ = 0; ++gen_;
    }
    cv_work_.notify_all();
    fn();
    std::unique_lock<std::mutex> lk(mu_);
    cv_done_.wait(lk, [&] { return finished_ == want_; });
    job_ = nullptr;
  }

 private:
  HostPool() : pid_(getpid()) {
    unsigned hw = std::thread::hardware_concurrency();
    if (const char* e = getenv("ICSG3D_HOST_THREADS")) hw = 2u * (unsigned)std::max(1, atoi(e));
    nmax_ = (int)std::min<unsigned>(std::max(1u, hw / 2), 64u);
    for (int t = 1; t < nmax_; ++t) std::thread([this] { worker(); }).detach();
  }
  void worker() {
    unsigned long long seen = 0;
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      cv_work_.wait(lk, [&] { return gen_ != seen && job_ != nullptr && started_ < want_; });
      seen = gen_;
      ++started_;
      const std::function<void()>* job = job_;
      lk.unlock();
      (*job)();
      lk.lock();
      if (++finished_ == want_) cv_done_.notify_all();
    }
  }
  const pid_t pid_;
  int nmax_ = 1;
  std::mutex mu_, run_mu_;
  std::condition_variable cv_work_, cv_done_;
  const std::function<void()>* job_ = nullptr;
  int want_ = 0, started_ = 0, finished_ = 0;
  unsigned long long gen_ = 0;
};
}  // namespace

// ---- the same split on the HOST (round 6).  The priority flood is a chain of dependent heap operations: one GPU lane walks
// it at ~3 us per voxel (dependent LDS / L2 round trips at 2 GHz), a CPU core at ~0.1 us, and the pop order of equal keys is
// part of the result, so the flood cannot be spread over lanes without changing it (phases A / B of the
// flood are order-free, the competition for the pockets they leave is not).  The boxes of one recursion level are independent:
// they are dealt to host threads.  Same arithmetic as ws_split_kernel, statement by statement (tests hold both to
// oracle/watershed_ref.py bit for bit; ICSG3D_WS_DEVICE=1 keeps the kernel).
namespace {
struct HostHeap {                                    // oracle/watershed_ref.py::_Heap == WsHeap above
  std::vector<unsigned> key, idx;
  int n = 0;
  void push(unsigned k, unsigned ix) {
    int child = n++;
    key[child] = k; idx[child] = ix;
    while (child > 0) {
      const int parent = (child + 1) / 2 - 1;
      if (key[child] < key[parent]) { std::swap(key[child], key[parent]); std::swap(idx[child], idx[parent]); child = parent; }
      else break;
    }
  }
  unsigned pop() {
    const unsigned top = idx[0];
    --n;
    if (n == 0) return top;
    key[0] = key[n]; idx[0] = idx[n];
    int i = 0;
    while (true) {
      const int l = 2 * i + 1, r = 2 * i + 2;
      int smallest = i;
      if (l < n) {
        if (key[l] < key[i]) smallest = l;
        if (r < n && key[r] < key[smallest]) smallest = r;
      } else break;
      if (smallest == i) break;
      std::swap(key[i], key[smallest]); std::swap(idx[i], idx[smallest]);
      i = smallest;
    }
    return top;
  }
};

void host_split_box(const int* val, int D, int H, int W, int tie, int* out) {
  const int V = D * H * W, HW = H * W;
  std::vector<int> fg(V), bgm(V), lab(V, 0);
  for (int i = 0; i < V; ++i) {                      // ball(1) erosion / dilation, out-of-box neighbours ignored
    const int x = i % W, y = (i / W) % H, z = i / HW;
    int mn = val[i], mx = val[i];
    auto see = [&](int v) { mn = v < mn ? v : mn; mx = v > mx ? v : mx; };
    if (z > 0) see(val[i - HW]);
    if (z < D - 1) see(val[i + HW]);
    if (y > 0) see(val[i - W]);
    if (y < H - 1) see(val[i + W]);
    if (x > 0) see(val[i - 1]);
    if (x < W - 1) see(val[i + 1]);
    fg[i] = mn; bgm[i] = mx;
  }
  // measure.label(fg), full connectivity: components of equal non-zero value, numbered in raster order of their first voxel
  std::vector<int> stack;
  int next = 0;
  for (int s0 = 0; s0 < V; ++s0) {
    if (fg[s0] == 0 || lab[s0] != 0) continue;
    lab[s0] = ++next;
    stack.assign(1, s0);
    while (!stack.empty()) {
      const int i = stack.back(); stack.pop_back();
      const int x = i % W, y = (i / W) % H, z = i / HW;
      for (int dz = -1; dz <= 1; ++dz) {
        const int zz = z + dz; if (zz < 0 || zz >= D) continue;
        for (int dy = -1; dy <= 1; ++dy) {
          const int yy = y + dy; if (yy < 0 || yy >= H) continue;
          for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx; if (xx < 0 || xx >= W) continue;
            const int j = (zz * H + yy) * W + xx;
            if (lab[j] == 0 && fg[j] == fg[i]) { lab[j] = next; stack.push_back(j); }
          }
        }
      }
    }
  }
  bool zeros = false;                                // markers = label + 1; markers[(bg - fg) == 1] = 0 (the reference's quirk)
  for (int i = 0; i < V; ++i) {
    int m = lab[i] + 1;
    if (bgm[i] - fg[i] == 1) { m = 0; zeros = true; }
    out[i] = m;
  }
  if (zeros) {                                       // skimage _watershed_cy.pyx as restated in watershed_ref.watershed_flood
    HostHeap hp;
    hp.key.resize(V); hp.idx.resize(V);
    unsigned seq = 0;
    for (int i = 0; i < V; ++i)
      if (out[i] != 0) hp.push(((val[i] != 0 ? 1u : 0u) << 31) | (tie ? seq++ : 0u), (unsigned)i);
    unsigned age = tie ? (unsigned)V + 1u : 1u;
    const int nb[6] = {-HW, -W, -1, 1, W, HW};
    while (hp.n > 0) {
      const int i = (int)hp.pop();
      const int x = i % W, y = (i / W) % H, z = i / HW;
      const bool ok[6] = {z > 0, y > 0, x > 0, x < W - 1, y < H - 1, z < D - 1};
      const int li = out[i];
      for (int k = 0; k < 6; ++k) {
        if (!ok[k]) continue;
        const int j = i + nb[k];
        if (out[j] != 0) continue;
        ++age;
        out[j] = li;
        hp.push(((val[j] != 0 ? 1u : 0u) << 31) | age, (unsigned)j);
      }
    }
  }
  for (int i = 0; i < V; ++i) if (out[i] == 1) out[i] = 0;     // wss[wss == 1] = 0
}

// measure.label(box, connectivity) on the host, for boxes the label kernel does not take (an extent above 64: whole d^3
// grids of segment_nuclei's first level at d >= 128).  Union-find over the already-visited neighbours in raster order,
// always hanging the larger root under the smaller, so that a root is the smallest index of its set; numbering the roots
// in raster order is then label_boxes_kernel's numbering.  Same 7-int stats; rows past min(n, max_labels) stay as they are.
void host_label_box(const int* val, int D, int H, int W, bool conn26, int max_labels, int* lab, int* n_out, int* st) {
  const int V = D * H * W;
  std::vector<int> parent(V);
  auto find = [&](int i) {
    while (parent[i] != i) { parent[i] = parent[parent[i]]; i = parent[i]; }      // path halving
    return i;
  };
  auto unite = [&](int a, int b) {
    a = find(a); b = find(b);
    if (a == b) return;
    if (a < b) parent[b] = a; else parent[a] = b;
  };
  for (int z = 0, i = 0; z < D; ++z)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x, ++i) {
        const int v = val[i];
        if (v == 0) continue;
        parent[i] = i;
        // the neighbours that precede i in raster order: -x, -y, -z (6), or the 13 with (dz, dy, dx) < (0, 0, 0) (26)
        for (int dz = -1; dz <= 0; ++dz)
          for (int dy = -1; dy <= (dz < 0 ? 1 : 0); ++dy)
            for (int dx = -1; dx <= ((dz < 0 || dy < 0) ? 1 : -1); ++dx) {
              if (!conn26 && (dz != 0) + (dy != 0) + (dx != 0) != 1) continue;
              const int zz = z + dz, yy = y + dy, xx = x + dx;
              if (zz < 0 || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
              const int j = (zz * H + yy) * W + xx;
              if (val[j] == v) unite(i, j);
            }
      }
  int n = 0;
  for (int i = 0; i < V; ++i) {
    if (val[i] == 0) { lab[i] = 0; continue; }
    const int r = find(i);
    lab[i] = r == i ? ++n : lab[r];                    // r < i: already numbered
  }
  *n_out = n;
  if (st == nullptr) return;
  const int nst = n < max_labels ? n : max_labels;
  for (int a = 0; a < nst; ++a) {
    int* s = st + (size_t)a * 7;
    s[0] = 0; s[1] = D; s[2] = H; s[3] = W; s[4] = 0; s[5] = 0; s[6] = 0;
  }
  for (int z = 0, i = 0; z < D; ++z)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x, ++i) {
        const int l = lab[i];
        if (l <= 0 || l > nst) continue;
        int* s = st + (size_t)(l - 1) * 7;
        ++s[0];
        s[1] = std::min(s[1], z); s[2] = std::min(s[2], y); s[3] = std::min(s[3], x);
        s[4] = std::max(s[4], z + 1); s[5] = std::max(s[5], y + 1); s[6] = std::max(s[6], x + 1);
      }
}

// fn(b) for the boxes `which` on host threads: largest boxes first (a level lasts as long as its slowest box), one box at a
// time per thread, one thread per ~16 k voxels of boxes, at most one per box
void host_boxes_run(const std::vector<BoxDesc>& desc, std::vector<int> which, const std::function<void(int)>& fn) {
  if (which.empty()) return;
  std::sort(which.begin(), which.end(), [&](int a, int b) {
    return (long long)desc[a].D * desc[a].H * desc[a].W > (long long)desc[b].D * desc[b].H * desc[b].W;
  });
  size_t vox = 0;
  for (int b : which) vox += (size_t)desc[b].D * desc[b].H * desc[b].W;
  std::atomic<size_t> next{0};
  auto work = [&]() {
    for (size_t k = next.fetch_add(1); k < which.size(); k = next.fetch_add(1)) fn(which[k]);
  };
  HostPool::get().run((int)std::min<size_t>(which.size(), vox / 16384 + 1), work);
}

// the boxes the kernels take (box_fits_device) packed back to back, and their descriptors re-based onto the packing;
// `pos` = their indices in the caller's list.  Used when a call mixes them with boxes that go to the host.
size_t pack_device_boxes(const int* h_vols, const std::vector<BoxDesc>& desc, const std::vector<int>& pos,
                         std::vector<int>* vols, std::vector<BoxDesc>* ddesc) {
  size_t off = 0;
  ddesc->clear();
  for (int b : pos) {
    BoxDesc d = desc[b];
    d.off = d.heap_off = (long long)off;
    ddesc->push_back(d);
    off += (size_t)d.D * d.H * d.W;
  }
  vols->resize(off);
  for (size_t k = 0; k < pos.size(); ++k)
    std::memcpy(vols->data() + (*ddesc)[k].off, h_vols + desc[pos[k]].off,
                (size_t)desc[pos[k]].D * desc[pos[k]].H * desc[pos[k]].W * sizeof(int));
  return off;
}
// The split on host threads (no device work: the flood is a chain of dependent heap operations);
// bit-identical to the kernel.
int watershed_split_host(const int* h_boxes, const int* h_dims, const int* h_cls, int nbox, int tie, int* h_wss) {
  ICS_CHECK(h_boxes && h_dims && h_cls && h_wss && nbox >= 1 && (tie == 0 || tie == 1), "bad watershed_split arguments");
  std::vector<BoxDesc> desc;
  size_t total = 0;
  ICS_TRY(box_descs(h_dims, h_cls, nbox, kBoxHostMax, &desc, &total));
  std::vector<int> all(nbox);
  for (int b = 0; b < nbox; ++b) all[b] = b;
  host_boxes_run(desc, all, [&](int b) {
    const BoxDesc& d = desc[b];
    host_split_box(h_boxes + d.off, d.D, d.H, d.W, tie, h_wss + d.off);
  });
  return 0;
}
}  // namespace

// ---- exact-integer convexity bounds of the components of labelled boxes, on host threads (round 6).
// icsg3d_amd/watershed.py decides `voxels / count_nonzero(convex_hull_image(component)) >= min_convexity`
// (/root/reference/watershed.py:80-83) from two bounds of the hull's grid-point count wherever they are conclusive, and
// calls Qhull only in between: P >= hull >= F with P = grid points of the bounding box inside the component's 26-direction
// polytope (the voxel set offset by +-0.5 along one axis at a time, as convex_hull_image builds it) and F = the component
// closed under "every grid point between two voxels of an axis-parallel line".  Also the flatness test (coplanar /
// collinear sets make the reference stack's Qhull call fail).  In numpy these cost 0.17 ms per component -- more than
// everything else of a recursion level once the flood left the GPU; here ~10 us, all components of a level in parallel.
// bounds [nbox][max_labels][5] = {voxels, P, F, flat, H}; rows of labels with <= min_voxels voxels stay zero; H = the exact
// hull count, computed only where hull_threshold > 0 and voxels / P < hull_threshold <= voxels / F (else 0).
namespace {
// ---- exact grid-point count of convex_hull_image(component) (round 6).  skimage offsets every voxel centre by +-0.5 along one
// axis at a time and counts the grid points inside the hull of those points; on doubled coordinates everything is an integer:
// S' = {2p +- e_k}.  The facet planes of conv(S') are found by gift wrapping with exact predicates and -- lattice sets being
// as degenerate as point sets get -- with whole coplanar groups per facet: a
// supporting plane's points are hulled in 2-D, its polygon's edges are pivoted across to the neighbouring planes.  A grid point
// is inside iff no plane excludes it; a point ON a plane is inside (Qhull evaluates those to ~1e-16 < the reference's 1e-10
// tolerance, watershed.py:80-81 / convex_hull_image).  Only the points between the two integer bounds need the test.
// Magnitudes, for box extents up to kBoxHostMax = 256: doubled coordinates lie in [-1, 511], so a coordinate difference is
// at most 512 = 2^9; a 2 x 2 minor (h_collinear, h_face_edges' cross, a plane normal in h_plane / h_planes) is at most 2^19;
// a triple product (h_triple) and a plane offset or evaluation n . p (h_plane, h_face_edges, the count below) are at most
// 3 * 2^9 * 2^19 < 2^31.  Every product is taken in long long: exact with 2^32 to spare.
struct HP { int x, y, z; };
inline long long h_triple(const HP& a, const HP& b, const HP& c, const HP& d) {
  const long long ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z, vx = c.x - a.x, vy = c.y - a.y, vz = c.z - a.z,
                  wx = d.x - a.x, wy = d.y - a.y, wz = d.z - a.z;
  return ux * (vy * wz - vz * wy) - uy * (vx * wz - vz * wx) + uz * (vx * wy - vy * wx);
}
inline bool h_collinear(const HP& a, const HP& b, const HP& p) {
  const long long ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z, vx = p.x - a.x, vy = p.y - a.y, vz = p.z - a.z;
  return uy * vz - uz * vy == 0 && uz * vx - ux * vz == 0 && ux * vy - uy * vx == 0;
}
struct HPlane {
  long long nx, ny, nz, d;      // n . p <= d for every point of the set; (n, d) reduced by their gcd
  bool operator<(const HPlane& o) const { return std::tie(nx, ny, nz, d) < std::tie(o.nx, o.ny, o.nz, o.d); }
};
long long h_gcd(long long a, long long b) { a = a < 0 ? -a : a; b = b < 0 ? -b : b; while (b) { const long long t = a % b; a = b; b = t; } return a; }
// the supporting plane through a, b, c (not collinear), oriented away from the set; false if points lie on both sides
bool h_plane(const std::vector<HP>& pts, const HP& a, const HP& b, const HP& c, HPlane* out) {
  long long nx = (long long)(b.y - a.y) * (c.z - a.z) - (long long)(b.z - a.z) * (c.y - a.y);
  long long ny = (long long)(b.z - a.z) * (c.x - a.x) - (long long)(b.x - a.x) * (c.z - a.z);
  long long nz = (long long)(b.x - a.x) * (c.y - a.y) - (long long)(b.y - a.y) * (c.x - a.x);
  const long long g = h_gcd(h_gcd(nx, ny), nz);
  if (g == 0) return false;
  nx /= g; ny /= g; nz /= g;
  const long long d = nx * a.x + ny * a.y + nz * a.z;
  int side = 0;
  for (const HP& p : pts) {
    const long long v = nx * p.x + ny * p.y + nz * p.z - d;
    if (v == 0) continue;
    const int s = v > 0 ? 1 : -1;
    if (side == 0) side = s;
    else if (side != s) return false;
  }
  if (side > 0) { nx = -nx; ny = -ny; nz = -nz; *out = HPlane{nx, ny, nz, -d}; }
  else *out = HPlane{nx, ny, nz, d};
  return true;
}
// boundary edges (index pairs into pts) of the convex polygon formed by the points on `pl`
void h_face_edges(const std::vector<HP>& pts, const HPlane& pl, std::vector<std::pair<int, int>>* edges) {
  std::vector<int> on;
  for (int i = 0; i < (int)pts.size(); ++i)
    if (pl.nx * pts[i].x + pl.ny * pts[i].y + pl.nz * pts[i].z == pl.d) on.push_back(i);
  const long long ax = pl.nx < 0 ? -pl.nx : pl.nx, ay = pl.ny < 0 ? -pl.ny : pl.ny, az = pl.nz < 0 ? -pl.nz : pl.nz;
  const int drop = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
  auto U = [&](int i) { return drop == 0 ? pts[i].y : pts[i].x; };
  auto V = [&](int i) { return drop == 2 ? pts[i].y : pts[i].z; };
  std::sort(on.begin(), on.end(), [&](int i, int j) { return U(i) != U(j) ? U(i) < U(j) : V(i) < V(j); });
  auto cross = [&](int o, int a, int b) {
    return (long long)(U(a) - U(o)) * (V(b) - V(o)) - (long long)(V(a) - V(o)) * (U(b) - U(o));
  };
  std::vector<int> h(2 * on.size());
  int k = 0;
  for (int i = 0; i < (int)on.size(); ++i) {                      // monotone chain, collinear points dropped
    while (k >= 2 && cross(h[k - 2], h[k - 1], on[i]) <= 0) --k;
    h[k++] = on[i];
  }
  for (int i = (int)on.size() - 2, t = k + 1; i >= 0; --i) {
    while (k >= t && cross(h[k - 2], h[k - 1], on[i]) <= 0) --k;
    h[k++] = on[i];
  }
  --k;
  for (int i = 0; i < k; ++i) edges->push_back({h[i], h[(i + 1) % k]});
}
// both supporting planes through the hull edge (a, b): the extreme directions of the set seen along the edge.  false if
// every point is collinear with the edge or a candidate's plane does not support the set (then the search cannot be trusted)
bool h_pivot(const std::vector<HP>& pts, int ia, int ib, HPlane out[2]) {
  const HP &a = pts[ia], &b = pts[ib];
  int c1 = -1, c2 = -1;
  for (int i = 0; i < (int)pts.size(); ++i) {
    if (i == ia || i == ib || h_collinear(a, b, pts[i])) continue;
    if (c1 < 0) { c1 = c2 = i; continue; }
    if (h_triple(a, b, pts[c1], pts[i]) < 0) c1 = i;
    if (h_triple(a, b, pts[c2], pts[i]) > 0) c2 = i;
  }
  return c1 >= 0 && h_plane(pts, a, b, pts[c1], &out[0]) && h_plane(pts, a, b, pts[c2], &out[1]);
}
// all facet planes of conv(pts); false if the search did not close -- a hull edge without two distinct supporting planes,
// a pivot candidate without a supporting plane, or the step guard (never observed; the caller then leaves the component to
// Qhull)
bool h_planes(const std::vector<HP>& pts, std::set<HPlane>* planes) {
  if (pts.size() < 4) return false;
  // a first supporting plane: the points of minimal x lie on x = xmin; tilt it around its extreme points until it is a facet
  int v0 = 0;
  for (int i = 1; i < (int)pts.size(); ++i)
    if (std::tie(pts[i].x, pts[i].y, pts[i].z) < std::tie(pts[v0].x, pts[v0].y, pts[v0].z)) v0 = i;
  // an edge from the vertex v0: gift wrapping in the projection along z gives a vertical supporting plane through v0; the
  // points on it are hulled in that plane; any boundary edge of that (possibly degenerate) polygon is a hull edge
  int v1 = -1;
  for (int i = 0; i < (int)pts.size(); ++i) {
    if (pts[i].x == pts[v0].x && pts[i].y == pts[v0].y) continue;            // same projection
    if (v1 < 0) { v1 = i; continue; }
    const long long cr = (long long)(pts[v1].x - pts[v0].x) * (pts[i].y - pts[v0].y) -
                         (long long)(pts[v1].y - pts[v0].y) * (pts[i].x - pts[v0].x);
    if (cr < 0) v1 = i;
  }
  std::vector<std::pair<int, int>> todo;
  if (v1 < 0) return false;                                                   // every point projects onto v0: a z line
  {
    // vertical plane through v0, v1: normal (dy, -dx, 0)
    long long nx = pts[v1].y - pts[v0].y, ny = -(long long)(pts[v1].x - pts[v0].x);
    const long long g = h_gcd(nx, ny);
    nx /= g; ny /= g;
    long long d = nx * pts[v0].x + ny * pts[v0].y;
    int side = 0;
    for (const HP& p : pts) { const long long v = nx * p.x + ny * p.y - d; if (v != 0) { side = v > 0 ? 1 : -1; break; } }
    if (side > 0) { nx = -nx; ny = -ny; d = -d; }
    const HPlane vp{nx, ny, 0, d};
    // is it a facet (three non-collinear points on it)?  then start from its polygon; else from the edge it holds
    std::vector<int> on;
    for (int i = 0; i < (int)pts.size(); ++i)
      if (nx * pts[i].x + ny * pts[i].y == d) on.push_back(i);
    bool facet = false;
    for (size_t i = 2; i < on.size() && !facet; ++i) facet = !h_collinear(pts[on[0]], pts[on[1]], pts[on[i]]);
    if (facet) {
      planes->insert(vp);
      h_face_edges(pts, vp, &todo);
    } else {
      int lo = on[0], hi = on[0];                                              // the segment's end points
      for (int i : on) {
        if (std::tie(pts[i].x, pts[i].y, pts[i].z) < std::tie(pts[lo].x, pts[lo].y, pts[lo].z)) lo = i;
        if (std::tie(pts[hi].x, pts[hi].y, pts[hi].z) < std::tie(pts[i].x, pts[i].y, pts[i].z)) hi = i;
      }
      if (lo == hi) return false;
      todo.push_back({lo, hi});
    }
  }
  std::set<std::pair<int, int>> seen;
  size_t guard = 0;
  while (!todo.empty()) {
    const std::pair<int, int> e = todo.back();
    todo.pop_back();
    const std::pair<int, int> key = e.first < e.second ? e : std::make_pair(e.second, e.first);
    if (!seen.insert(key).second) continue;
    if (++guard > 200000) return false;
    HPlane two[2];
    if (!h_pivot(pts, e.first, e.second, two)) return false;
    if (!(two[0] < two[1]) && !(two[1] < two[0])) return false;            // one plane where a hull edge has two
    for (const HPlane& pl : two)
      if (planes->insert(pl).second) h_face_edges(pts, pl, &todo);
  }
  return planes->size() >= 4;
}

// bounds of one component; hull_thr > 0: where voxels / P < hull_thr <= voxels / F the exact hull count goes to out[4]
void component_bounds_one(const int* lab, int H, int W, int cl, const int* st, double hull_thr, long long* out) {
  const int z0 = st[1], y0 = st[2], x0 = st[3], bd = st[4] - st[1], bh = st[5] - st[2], bw = st[6] - st[3];
  const int V = bd * bh * bw;
  std::vector<unsigned char> a(V), f, inP(V);
  std::vector<int> px, py, pz;
  for (int z = 0; z < bd; ++z)
    for (int y = 0; y < bh; ++y)
      for (int x = 0; x < bw; ++x) {
        const bool in = lab[((size_t)(z0 + z) * H + (y0 + y)) * W + (x0 + x)] == cl;
        a[(z * bh + y) * bw + x] = in;
        if (in) { pz.push_back(z); py.push_back(y); px.push_back(x); }
      }
  const int n = (int)px.size();
  out[0] = n;
  out[4] = 0;
  if (n == 0) { out[1] = out[2] = 0; out[3] = 1; return; }
  // flat: all points collinear or coplanar (icsg3d_amd/watershed.py::is_flat, exact integers)
  bool flat = true;
  {
    int i1 = -1;
    for (int i = 1; i < n && i1 < 0; ++i)
      if (pz[i] != pz[0] || py[i] != py[0] || px[i] != px[0]) i1 = i;
    if (i1 >= 0) {
      const int az = pz[i1] - pz[0], ay = py[i1] - py[0], ax = px[i1] - px[0];
      int cz = 0, cy = 0, cx = 0;
      bool have = false;
      for (int i = 1; i < n && !have; ++i) {
        const int vz = pz[i] - pz[0], vy = py[i] - py[0], vx = px[i] - px[0];
        cz = vy * ax - vx * ay; cy = vx * az - vz * ax; cx = vz * ay - vy * az;      // cross(v, a)
        have = cz != 0 || cy != 0 || cx != 0;
      }
      if (have)
        for (int i = 1; i < n && flat; ++i)
          if ((pz[i] - pz[0]) * cz + (py[i] - py[0]) * cy + (px[i] - px[0]) * cx != 0) flat = false;
    }
  }
  out[3] = flat ? 1 : 0;
  // P: the 13 direction classes with components in {-1, 0, 1}; doubled coordinates, the +-0.5 offsets move a support value by
  // max_k |d_k| / 2 = 1/2 -> pad 1 on the doubled scale
  int dirs[13][3], nd = 0;
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx)
        if (dz > 0 || (dz == 0 && (dy > 0 || (dy == 0 && dx > 0)))) { dirs[nd][0] = dz; dirs[nd][1] = dy; dirs[nd][2] = dx; ++nd; }
  int lo[13], hi[13];
  for (int k = 0; k < 13; ++k) { lo[k] = INT_MAX; hi[k] = INT_MIN; }
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 13; ++k) {
      const int pr = dirs[k][0] * pz[i] + dirs[k][1] * py[i] + dirs[k][2] * px[i];
      lo[k] = pr < lo[k] ? pr : lo[k]; hi[k] = pr > hi[k] ? pr : hi[k];
    }
  long long P = 0;
  for (int z = 0; z < bd; ++z)
    for (int y = 0; y < bh; ++y)
      for (int x = 0; x < bw; ++x) {
        bool in = true;
        for (int k = 0; k < 13 && in; ++k) {
          const int g = 2 * (dirs[k][0] * z + dirs[k][1] * y + dirs[k][2] * x);
          in = g <= 2 * hi[k] + 1 && g >= 2 * lo[k] - 1;
        }
        inP[(z * bh + y) * bw + x] = in;
        P += in;
      }
  out[1] = P;
  // F: closure under axis-line fills (icsg3d_amd/watershed.py::_fill_mask: at most 4 rounds, which the tests hold equal)
  f = a;
  long long cnt = n;
  const int stride[3] = {bh * bw, bw, 1}, ext[3] = {bd, bh, bw};
  for (int round = 0; round < 4; ++round) {
    for (int ax = 0; ax < 3; ++ax) {
      const int o1 = (ax + 1) % 3, o2 = (ax + 2) % 3;
      for (int u = 0; u < ext[o1]; ++u)
        for (int v = 0; v < ext[o2]; ++v) {
          const int base = u * stride[o1] + v * stride[o2];
          int first = -1, last = -1;
          for (int t = 0; t < ext[ax]; ++t)
            if (f[base + t * stride[ax]]) { if (first < 0) first = t; last = t; }
          for (int t = first; t >= 0 && t <= last; ++t) f[base + t * stride[ax]] = 1;
        }
    }
    long long m = 0;
    for (int i = 0; i < V; ++i) m += f[i];
    if (m == cnt) break;
    cnt = m;
  }
  out[2] = cnt;
  if (!(hull_thr > 0) || (double)n / (double)P >= hull_thr || (double)n / (double)cnt < hull_thr) return;
  // undecided by the bounds: the exact count.  Vertex candidates: voxels that end all three of their axis lines.
  std::vector<HP> pts;
  for (int i = 0; i < n; ++i) {
    const int z = pz[i], y = py[i], x = px[i];
    auto inner = [&](int dz, int dy, int dx) {      // a voxel of the set on BOTH sides along this axis line
      bool before = false, after = false;
      for (int t = 1; !before; ++t) {
        const int zz = z - t * dz, yy = y - t * dy, xx = x - t * dx;
        if (zz < 0 || yy < 0 || xx < 0) break;
        before = a[(zz * bh + yy) * bw + xx] != 0;
      }
      for (int t = 1; !after; ++t) {
        const int zz = z + t * dz, yy = y + t * dy, xx = x + t * dx;
        if (zz >= bd || yy >= bh || xx >= bw) break;
        after = a[(zz * bh + yy) * bw + xx] != 0;
      }
      return before && after;
    };
    if (inner(1, 0, 0) || inner(0, 1, 0) || inner(0, 0, 1)) continue;
    const int X = 2 * x, Y = 2 * y, Z = 2 * z;
    pts.push_back({X - 1, Y, Z}); pts.push_back({X + 1, Y, Z}); pts.push_back({X, Y - 1, Z});
    pts.push_back({X, Y + 1, Z}); pts.push_back({X, Y, Z - 1}); pts.push_back({X, Y, Z + 1});
  }
  std::sort(pts.begin(), pts.end(), [](const HP& p, const HP& q) { return std::tie(p.x, p.y, p.z) < std::tie(q.x, q.y, q.z); });
  pts.erase(std::unique(pts.begin(), pts.end(), [](const HP& p, const HP& q) { return p.x == q.x && p.y == q.y && p.z == q.z; }), pts.end());
  std::set<HPlane> planes;
  if (!h_planes(pts, &planes)) return;             // out[4] stays 0: the caller decides this one with Qhull
  long long Hc = cnt;
  for (int z = 0; z < bd; ++z)
    for (int y = 0; y < bh; ++y)
      for (int x = 0; x < bw; ++x) {
        const int i = (z * bh + y) * bw + x;
        if (!inP[i] || f[i]) continue;
        bool in = true;
        for (const HPlane& pl : planes)
          if (pl.nx * (2 * x) + pl.ny * (2 * y) + pl.nz * (2 * z) > pl.d) { in = false; break; }
        Hc += in;
      }
  if (Hc < cnt || Hc > P) return;                  // outside F <= H <= P: a plane is missing; out[4] stays 0 (Qhull)
  out[4] = Hc;
}
}  // namespace

}  // namespace ics

// ==========================================================================================
// C ABI: the box-level ops, HOST pointers in and out (include/icsg3d.h)
// ==========================================================================================
using namespace ics;

extern "C" {

// Boxes with an extent above 64 (or every box, ICSG3D_LABEL_HOST=1) go to host_label_box on host threads, the others to
// label_boxes_kernel; the stream is only asked for when a box goes to the device.
int ics_op_label_boxes(const int32_t* h_vols, const int32_t* h_dims, int nbox, int connectivity, int max_labels,
                       int32_t* h_labels, int32_t* h_nlabels, int32_t* h_stats) {
  ICS_CHECK(h_vols && h_dims && h_labels && h_nlabels && nbox >= 1 && max_labels >= 1, "bad label_boxes arguments");
  ICS_CHECK(connectivity == 1 || connectivity == 3, "connectivity must be 1 (6 neighbours) or 3 (26)");
  std::vector<BoxDesc> desc;
  size_t total = 0;
  ICS_TRY(box_descs(h_dims, nullptr, nbox, kBoxHostMax, &desc, &total));
  const bool host_all = label_host_forced();
  std::vector<int> on_host, on_dev;
  for (int b = 0; b < nbox; ++b) (host_all || !box_fits_device(desc[b]) ? on_host : on_dev).push_back(b);
  const size_t row = (size_t)max_labels * 7;
  host_boxes_run(desc, on_host, [&](int b) {
    const BoxDesc& d = desc[b];
    host_label_box(h_vols + d.off, d.D, d.H, d.W, connectivity == 3, max_labels, h_labels + d.off, h_nlabels + b,
                   h_stats ? h_stats + b * row : nullptr);
  });
  if (on_dev.empty()) return 0;
  // a mixed call: the device boxes are packed, and their results dealt back afterwards
  const bool mixed = (int)on_dev.size() != nbox;
  std::vector<int> pvol, plab, pn, pst;
  std::vector<BoxDesc> pdesc;
  const int* vols = h_vols;
  int *labels = h_labels, *nlabels = h_nlabels, *stats = h_stats;
  const std::vector<BoxDesc>* dd = &desc;
  size_t dtotal = total;
  if (mixed) {
    dtotal = pack_device_boxes(h_vols, desc, on_dev, &pvol, &pdesc);
    plab.resize(dtotal); pn.resize(on_dev.size());
    if (h_stats) pst.resize(on_dev.size() * row);
    vols = pvol.data(); labels = plab.data(); nlabels = pn.data(); stats = h_stats ? pst.data() : nullptr; dd = &pdesc;
  }
  const int ndev = (int)on_dev.size();
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  Layout L;
  const auto s_vol = L.add<int>(dtotal), s_lab = L.add<int>(dtotal);
  const auto s_desc = L.add<BoxDesc>(ndev);
  const auto s_n = L.add<int>(ndev);
  const auto s_st = L.add<int>((size_t)ndev * row);
  int *d_vol, *d_lab, *d_n, *d_st;
  BoxDesc* d_desc;
  ICS_TRY(L.reserve(s_vol, &d_vol, s_lab, &d_lab, s_desc, &d_desc, s_n, &d_n, s_st, &d_st));
  ICS_TRY(L.upload(s_vol, vols, dtotal, st));
  ICS_TRY(L.upload(s_desc, dd->data(), ndev, st));
  ICS_LAUNCH(label_boxes_kernel, dim3(ndev), dim3(1024), 0, st, d_vol, d_desc, connectivity == 3 ? 1 : 0, max_labels,
             d_lab, d_n, d_st);
  ICS_HIP(hipGetLastError());
  ICS_TRY(L.download(labels, s_lab, dtotal, st));
  ICS_TRY(L.download(nlabels, s_n, ndev, st));
  if (stats) ICS_TRY(L.download(stats, s_st, s_st.count, st));
  ICS_HIP(hipStreamSynchronize(st));
  if (mixed)
    for (int k = 0; k < ndev; ++k) {
      const int b = on_dev[k];
      const BoxDesc &d = desc[b], &p = pdesc[k];
      std::memcpy(h_labels + d.off, plab.data() + p.off, (size_t)d.D * d.H * d.W * sizeof(int));
      h_nlabels[b] = pn[k];
      if (h_stats) std::memcpy(h_stats + b * row, pst.data() + k * row, row * sizeof(int));
    }
  return 0;
}

int ics_op_region_stats(const int32_t* h_R, const uint8_t* h_species, int D, int H, int W, int nlab, int nbins,
                        int32_t* h_stats) {
  ICS_CHECK(h_R && h_species && h_stats && D >= 1 && H >= 1 && W >= 1 && nlab >= 1 && nbins >= 2 && nbins <= 256,
            "bad region_stats arguments");
  const size_t V = (size_t)D * H * W;
  ICS_CHECK(V < (1u << 30), "volume too large");
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  Layout L;
  const auto s_R = L.add<int>(V);
  const auto s_sp = L.add<unsigned char>(V);
  const auto s_st = L.add<int>((size_t)nlab * kSegStatInts);
  const auto s_h = L.add<unsigned>((size_t)nlab * nbins);
  int *d_R, *d_st;
  unsigned char* d_sp;
  unsigned* d_h;
  ICS_TRY(L.reserve(s_R, &d_R, s_sp, &d_sp, s_st, &d_st, s_h, &d_h));
  ICS_TRY(L.upload(s_R, h_R, V, st));
  ICS_TRY(L.upload(s_sp, h_species, V, st));
  ICS_TRY(L.fill(s_h, 0, s_h.count, st));
  const int dmax = D > H ? (D > W ? D : W) : (H > W ? H : W);
  ICS_LAUNCH(seg_stats_init_kernel, dim3((unsigned)((nlab + 255) / 256)), dim3(256), 0, st, d_st, (size_t)nlab, dmax);
  ICS_LAUNCH(region_stats_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, st, d_R, d_sp, D, H, W, nlab, nbins,
             d_st, d_h);
  ICS_LAUNCH(seg_vote_kernel, dim3((unsigned)((nlab + 255) / 256)), dim3(256), 0, st, d_h, nbins, (size_t)nlab, d_st);
  ICS_HIP(hipGetLastError());
  ICS_TRY(L.download(h_stats, s_st, s_st.count, st));
  ICS_HIP(hipStreamSynchronize(st));
  return 0;
}

int ics_op_component_bounds(const int32_t* h_labels, const int32_t* h_dims, int nbox, const int32_t* h_nlabels,
                            const int32_t* h_stats, int max_labels, int min_voxels, double hull_threshold, int64_t* bounds) {
  static_assert(sizeof(long long) == sizeof(int64_t), "int64 layout");
  long long* h_bounds = reinterpret_cast<long long*>(bounds);
  ICS_CHECK(h_labels && h_dims && h_nlabels && h_stats && h_bounds && nbox >= 1 && max_labels >= 1, "bad component_bounds arguments");
  std::vector<BoxDesc> desc;
  size_t total = 0;
  ICS_TRY(box_descs(h_dims, nullptr, nbox, kBoxHostMax, &desc, &total));
  struct Job { int box, cl; };
  std::vector<Job> jobs;
  for (int b = 0; b < nbox; ++b) {
    ICS_CHECK(h_nlabels[b] >= 0 && h_nlabels[b] <= max_labels, "component_bounds: nlabels exceeds max_labels");
    const BoxDesc& d = desc[b];
    for (int c = 0; c < h_nlabels[b]; ++c) {
      const int* s = h_stats + ((size_t)b * max_labels + c) * 7;
      if (s[0] <= min_voxels) continue;
      // component_bounds_one reads the label volume inside this box: a stale or inverted row must not reach it
      ICS_CHECK(0 <= s[1] && s[1] < s[4] && s[4] <= d.D && 0 <= s[2] && s[2] < s[5] && s[5] <= d.H && 0 <= s[3] &&
                    s[3] < s[6] && s[6] <= d.W,
                "component_bounds: box " + std::to_string(b) + " label " + std::to_string(c + 1) + ": stats box [" +
                    std::to_string(s[1]) + "," + std::to_string(s[4]) + ")x[" + std::to_string(s[2]) + "," +
                    std::to_string(s[5]) + ")x[" + std::to_string(s[3]) + "," + std::to_string(s[6]) + ") must be non-empty and inside " +
                    std::to_string(d.D) + "x" + std::to_string(d.H) + "x" + std::to_string(d.W));
      jobs.push_back(Job{b, c + 1});
    }
  }
  std::memset(h_bounds, 0, (size_t)nbox * max_labels * 5 * sizeof(long long));
  std::atomic<size_t> next{0};
  auto work = [&]() {
    for (size_t k = next.fetch_add(1); k < jobs.size(); k = next.fetch_add(1)) {
      const Job j = jobs[k];
      const BoxDesc& d = desc[j.box];
      component_bounds_one(h_labels + d.off, d.H, d.W, j.cl, h_stats + ((size_t)j.box * max_labels + j.cl - 1) * 7,
                           hull_threshold, h_bounds + ((size_t)j.box * max_labels + j.cl - 1) * 5);
    }
  };
  HostPool::get().run((int)(jobs.size() / 8 + 1), work);
  return 0;
}

int ics_op_watershed_split(const int32_t* h_boxes, const int32_t* h_dims, const int32_t* h_cls, int nbox, int tie,
                           int32_t* h_wss) {
  // Round 6: the boxes of a level go to host threads (watershed_split_host: the flood is sequential per box and a CPU core
  // walks it ~30x faster than one GPU lane); ICSG3D_WS_DEVICE=1 keeps the kernel (A/B, tests run both) for the boxes it
  // takes (extents <= 64), the others still go to the host flood (host_split_box, the same arithmetic).
  const char* env = getenv("ICSG3D_WS_DEVICE");       // read per call: tests flip it inside one process
  const bool on_device = env != nullptr && atoi(env) != 0;
  if (!on_device) return watershed_split_host(h_boxes, h_dims, h_cls, nbox, tie, h_wss);
  ICS_CHECK(h_boxes && h_dims && h_cls && h_wss && nbox >= 1 && (tie == 0 || tie == 1), "bad watershed_split arguments");
  std::vector<BoxDesc> desc;
  size_t total = 0;
  ICS_TRY(box_descs(h_dims, h_cls, nbox, kBoxHostMax, &desc, &total));
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  std::vector<int> on_host, on_dev;
  for (int b = 0; b < nbox; ++b) (box_fits_device(desc[b]) ? on_dev : on_host).push_back(b);
  host_boxes_run(desc, on_host, [&](int b) {
    const BoxDesc& d = desc[b];
    host_split_box(h_boxes + d.off, d.D, d.H, d.W, tie, h_wss + d.off);
  });
  if (on_dev.empty()) return 0;
  const bool mixed = (int)on_dev.size() != nbox;
  std::vector<int> pvol, pout;
  std::vector<BoxDesc> pdesc;
  const int* boxes = h_boxes;
  int* wss = h_wss;
  const std::vector<BoxDesc>* dd = &desc;
  size_t dtotal = total;
  if (mixed) {
    dtotal = pack_device_boxes(h_boxes, desc, on_dev, &pvol, &pdesc);
    pout.resize(dtotal);
    boxes = pvol.data(); wss = pout.data(); dd = &pdesc;
  }
  const int ndev = (int)on_dev.size();
  Layout L;
  const auto s_box = L.add<int>(dtotal), s_out = L.add<int>(dtotal);
  const auto s_desc = L.add<BoxDesc>(ndev);
  // work: 4 ints per voxel (BoxDesc::heap_off * 2 with room to spare), heap: 2 unsigned per voxel
  const auto s_work = L.add<int>(dtotal * 4);
  const auto s_heap = L.add<unsigned>(dtotal * 2);
  int *d_box, *d_out, *d_work;
  BoxDesc* d_desc;
  unsigned* d_heap;
  ICS_TRY(L.reserve(s_box, &d_box, s_out, &d_out, s_desc, &d_desc, s_work, &d_work, s_heap, &d_heap));
  ICS_TRY(L.upload(s_box, boxes, dtotal, st));
  ICS_TRY(L.upload(s_desc, dd->data(), ndev, st));
  ICS_LAUNCH(ws_split_kernel, dim3(ndev), dim3(1024), 0, st, d_box, d_desc, tie, d_work, d_heap, d_out);
  ICS_HIP(hipGetLastError());
  ICS_TRY(L.download(wss, s_out, dtotal, st));
  ICS_HIP(hipStreamSynchronize(st));
  if (mixed)
    for (int k = 0; k < ndev; ++k) {
      const BoxDesc &d = desc[on_dev[k]], &p = pdesc[k];
      std::memcpy(h_wss + d.off, pout.data() + p.off, (size_t)d.D * d.H * d.W * sizeof(int));
    }
  return 0;
}

}  // extern "C"
