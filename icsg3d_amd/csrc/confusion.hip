// The confusion matrix of a segmentation (gfx950 / MI355X only): (true label, predicted species) pairs counted per class
// pair on the device, with the 2 x 2 occupancy table of the sigmoid head next to it.  confusion.h has the contract.
//
// The kernel follows label_counts_kernel (feed.hip) -- the same label kinds, the same validity rule, the same way of
// defusing the hot bin -- with two differences that the size of the table forces:
//   * ONE table per workgroup, not one per wave.  The bins are 32-bit in LDS; at 127 classes the table is 64 536 bytes, so
//     four per-wave copies would not fit a CU's 160 KiB even once, and a table per workgroup still leaves two workgroups
//     resident.  Smaller class counts use the same layout (95 classes: 36 120 bytes, four workgroups a CU): one code
//     path, and nothing in the result can depend on the choice.  The contention a shared table could bring is the hot
//     bin's, and that one is removed at the source:
//   * about 98 % of the pairs are (background, background).  The lanes of a wave that agree with its first active lane
//     are counted by ONE LDS add of their number (readfirstlane + ballot); the others add their own 1.  A wave of
//     background voxels costs one atomic per pair position instead of 64 queued on one address.
// Loads: one lane takes 16 consecutive pairs per pass -- one 16-byte load of the predictions, one of the mask, and 1 / 4 / 8
// 16-byte loads of the uint8 / float32 / float64 labels; the n % 16 last pairs are taken one per lane by block 0.
// Flush: one 64-bit atomicAdd per non-empty bin and block.  Integer sums: any order gives the same counts.
#include "confusion.h"
#include "scratch.h"

namespace ics {

typedef unsigned conf_v4 __attribute__((ext_vector_type(4)));

// the class id of a true label, or -1: 0 <= v < ncls and v integral, compared in v's own type; a NaN fails the first test
__device__ __forceinline__ int conf_true_id(unsigned char v, int ncls) { return (int)v < ncls ? (int)v : -1; }
__device__ __forceinline__ int conf_true_id(float v, int ncls) {
  return (v >= 0.f && v < (float)ncls && v == truncf(v)) ? (int)v : -1;
}
__device__ __forceinline__ int conf_true_id(double v, int ncls) {
  return (v >= 0.0 && v < (double)ncls && v == trunc(v)) ? (int)v : -1;
}

template <typename T, bool MASK>
__global__ __launch_bounds__(kConfThreads) void confusion_kernel(const T* __restrict__ tru, const unsigned char* __restrict__ pred,
                                                                 const unsigned char* __restrict__ mask, size_t n, int ncls,
                                                                 unsigned long long* __restrict__ acc) {
  constexpr int V = 16 / (int)sizeof(T);          // labels per 16-byte load
  constexpr int P = kConfLanePairs;
  extern __shared__ __attribute__((aligned(16))) unsigned conf_bins[];   // the accumulator's layout, 32-bit
  const int tid = threadIdx.x, lane = tid & 63;
  const int nn = ncls * ncls, nbins = nn + 5;
  for (int i = tid; i < nbins; i += kConfThreads) conf_bins[i] = 0u;
  __syncthreads();
  auto add = [&](int bin) {                                    // called by any subset of a wave's lanes
    const unsigned long long active = __ballot(1);
    const int first = __builtin_amdgcn_readfirstlane(bin);    // the first active lane's bin
    const unsigned long long same = __ballot(bin == first);
    if (lane == __ffsll((long long)active) - 1) atomicAdd(&conf_bins[first], (unsigned)__popcll(same));
    else if (bin != first) atomicAdd(&conf_bins[bin], 1u);
  };
  auto count = [&](T t, unsigned p, unsigned m) {
    const int ti = conf_true_id(t, ncls);
    add((ti >= 0 && (int)p < ncls) ? ti * ncls + (int)p : nn);
    if (MASK) {
      if (ti >= 0) add(nn + 1 + (ti != 0) * 2 + (m != 0));
    }
  };
  const size_t nvec = n / P;
  for (size_t q = (size_t)blockIdx.x * kConfThreads + tid; q < nvec; q += (size_t)gridDim.x * kConfThreads) {
    union { conf_v4 u; unsigned char b[P]; } pv, mv;
    union { conf_v4 u[P / V]; T v[P]; } tv;
    pv.u = reinterpret_cast<const conf_v4*>(pred)[q];
    if (MASK) mv.u = reinterpret_cast<const conf_v4*>(mask)[q];
#pragma unroll
    for (int j = 0; j < P / V; ++j) tv.u[j] = reinterpret_cast<const conf_v4*>(tru)[q * (P / V) + j];
#pragma unroll
    for (int k = 0; k < P; ++k) count(tv.v[k], pv.b[k], MASK ? mv.b[k] : 0u);
  }
  if (blockIdx.x == 0 && (size_t)tid < n - nvec * P) {
    const size_t i = nvec * P + tid;
    count(tru[i], pred[i], MASK ? mask[i] : 0u);
  }
  __syncthreads();
  for (int i = tid; i < nbins; i += kConfThreads) {
    const unsigned v = conf_bins[i];
    if (v) atomicAdd(&acc[i], (unsigned long long)v);
  }
}

template <typename T>
static void confusion_launch(hipStream_t st, unsigned nblk, size_t lds, const void* t, const unsigned char* pred,
                             const unsigned char* mask, size_t n, int ncls, unsigned long long* acc) {
  const dim3 grid(nblk), block(kConfThreads);
  if (mask) ICS_LAUNCH(confusion_kernel<T, true>, grid, block, lds, st, static_cast<const T*>(t), pred, mask, n, ncls, acc);
  else ICS_LAUNCH(confusion_kernel<T, false>, grid, block, lds, st, static_cast<const T*>(t), pred, mask, n, ncls, acc);
}

int launch_confusion(hipStream_t st, const void* true_labels, int label_kind, const unsigned char* pred,
                     const unsigned char* mask_or_null, size_t n, int ncls, unsigned long long* acc) {
  ICS_CHECK(label_kind == FEED_LABELS_U8 || label_kind == FEED_LABELS_F64 || label_kind == FEED_LABELS_F32,
            "confusion: label_kind must be 1 (uint8), 2 (float64) or 3 (float32)");
  ICS_CHECK(ncls >= kConfMinCls && ncls <= kConfMaxCls, "confusion: num_classes must be in [2, 127]");
  ICS_CHECK(n <= kConfMaxPairs, "confusion: at most 2^40 pairs per call");
  ICS_CHECK(acc != nullptr, "confusion: null accumulator");
  if (n == 0) return 0;
  ICS_CHECK(true_labels && pred, "confusion: null label pointer");
  ICS_CHECK(((reinterpret_cast<uintptr_t>(true_labels) | reinterpret_cast<uintptr_t>(pred) |
              reinterpret_cast<uintptr_t>(mask_or_null)) & 15) == 0,
            "confusion: the label, prediction and mask volumes must be 16-byte aligned");
  const size_t nvec = n / kConfLanePairs;
  size_t nblk = (nvec + kConfThreads - 1) / kConfThreads;
  nblk = nblk < 1 ? 1 : (nblk > (size_t)kConfMaxBlocks ? (size_t)kConfMaxBlocks : nblk);
  const size_t lds = align_up(conf_acc_len(ncls) * sizeof(unsigned), 16);      // <= 64 544 bytes
  if (label_kind == FEED_LABELS_U8) confusion_launch<unsigned char>(st, (unsigned)nblk, lds, true_labels, pred, mask_or_null, n, ncls, acc);
  else if (label_kind == FEED_LABELS_F32) confusion_launch<float>(st, (unsigned)nblk, lds, true_labels, pred, mask_or_null, n, ncls, acc);
  else confusion_launch<double>(st, (unsigned)nblk, lds, true_labels, pred, mask_or_null, n, ncls, acc);
  ICS_HIP(hipGetLastError());
  return 0;
}

}  // namespace ics

// ==========================================================================================
// C ABI
// ==========================================================================================
using namespace ics;

extern "C" {

int ics_op_confusion(const void* true_labels, int label_kind, const uint8_t* pred, const uint8_t* mask_or_null, size_t n,
                     int ncls, int64_t* matrix, int64_t* occupancy_or_null, int64_t* out_of_range) {
  ICS_CHECK(label_kind != FEED_LABELS_ONEHOT, "ics_op_confusion: one-hot labels are not class ids: pass their argmax instead");
  ICS_CHECK(label_kind == FEED_LABELS_U8 || label_kind == FEED_LABELS_F64 || label_kind == FEED_LABELS_F32,
            "ics_op_confusion: label_kind must be 1 (uint8), 2 (float64) or 3 (float32)");
  ICS_CHECK(ncls >= kConfMinCls && ncls <= kConfMaxCls, "ics_op_confusion: num_classes must be in [2, 127]");
  ICS_CHECK(matrix && out_of_range && ((true_labels && pred) || n == 0), "ics_op_confusion: null argument");
  ICS_CHECK((mask_or_null != nullptr) == (occupancy_or_null != nullptr),
            "ics_op_confusion: the mask and the occupancy table come together (both or neither)");
  ICS_CHECK(n <= kConfMaxPairs, "ics_op_confusion: at most 2^40 pairs per call");
  const size_t lab_bytes = feed_label_bytes(label_kind, ncls);
  ICS_CHECK((reinterpret_cast<uintptr_t>(true_labels) & (lab_bytes - 1)) == 0,
            "ics_op_confusion: unaligned label pointer: the true labels must be aligned to their element size (1, 4 or 8 bytes)");
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  const size_t len = conf_acc_len(ncls);
  Layout L;                       // every segment at a 256-byte aligned offset: the kernel's 16-byte rule holds
  const auto s_lab = L.add<unsigned char>(n * lab_bytes);
  const auto s_pred = L.add<unsigned char>(n);
  const auto s_mask = L.add<unsigned char>(mask_or_null ? n : 0);
  const auto s_acc = L.add<unsigned long long>(len);
  unsigned char *d_lab, *d_pred, *d_mask;
  unsigned long long* d_acc;
  ICS_TRY(L.reserve(s_lab, &d_lab, s_pred, &d_pred, s_mask, &d_mask, s_acc, &d_acc));
  ICS_TRY(L.upload(s_lab, true_labels, s_lab.count, st));
  ICS_TRY(L.upload(s_pred, pred, s_pred.count, st));
  ICS_TRY(L.upload(s_mask, mask_or_null, s_mask.count, st));
  ICS_TRY(L.fill(s_acc, 0, len, st));
  ICS_TRY(launch_confusion(st, d_lab, label_kind, d_pred, d_mask, n, ncls, d_acc));
  std::vector<unsigned long long> host(len);
  ICS_TRY(L.download(host.data(), s_acc, len, st));
  ICS_HIP(hipStreamSynchronize(st));
  const size_t nn = (size_t)ncls * ncls;
  for (size_t i = 0; i < nn; ++i) matrix[i] = (int64_t)host[i];
  *out_of_range = (int64_t)host[nn];
  if (occupancy_or_null)
    for (int k = 0; k < 4; ++k) occupancy_or_null[k] = (int64_t)host[nn + 1 + k];
  return 0;
}

int ics_op_confusion_grid(int* threads, int* lane_pairs, int* max_blocks) {
  ICS_CHECK(threads && lane_pairs && max_blocks, "ics_op_confusion_grid: null argument");
  *threads = kConfThreads; *lane_pairs = kConfLanePairs; *max_blocks = kConfMaxBlocks;
  return 0;
}

}  // extern "C"
