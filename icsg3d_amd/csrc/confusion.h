// Declarations for confusion.hip: the per-class confusion matrix of (true label, predicted species) pairs and the 2 x 2
// occupancy table of (true label != 0, mask != 0), counted on the device (include/icsg3d.h, "confusion matrix").
//
// THE CONTRACT of launch_confusion:
//   true labels   n class ids of kind FEED_LABELS_U8 / _F32 / _F64 (feed.h; one-hot is refused), 16-byte aligned;
//   pred          n uint8, 16-byte aligned;  mask: n uint8, 16-byte aligned, or nullptr (no occupancy table);
//   n             any count from 0 to 2^40;  ncls in [2, 127];
//   acc           [conf_acc_len(ncls)] uint64 on the device, ADDED to (zero it first for the counts of one call):
//                   [t * ncls + p]            pairs whose t and p are both class ids
//                   [ncls * ncls]             every other pair ("out of range"): it indexes nothing
//                   [ncls * ncls + 1 + k]     k = (t != 0) * 2 + (mask != 0), over the pairs whose t is a class id (whatever
//                                             p is); pairs with an invalid t are in none of the four
//   validity      t is a class id when 0 <= t < ncls and t == trunc(t), compared in t's own type (a NaN fails): count_bin's
//                 rule in feed.hip.  p is one when p < ncls.
// Integer sums in 64 bits: the counts do not depend on the grid, on the order of the atomics or on the run.
//
// THE GRID: kConfThreads lanes a block, one lane = kConfLanePairs pairs per grid-stride pass, at most kConfMaxBlocks
// blocks.  512 blocks are two per CU on 256 CUs, what the largest table (127 * 127 + 5 bins of 4 bytes = 64 536 bytes of
// the CU's 160 KiB) lets be resident at once.  With n <= 2^40 a block sees at most 2^40 / 512 = 2^31 pairs (+ 15 of
// the ragged tail in block 0), so its 32-bit LDS bins cannot wrap.
#pragma once
#include "common.h"
#include "feed.h"

namespace ics {

constexpr int kConfThreads = 256, kConfLanePairs = 16, kConfMaxBlocks = 512;
constexpr size_t kConfMaxPairs = (size_t)1 << 40;
constexpr int kConfMinCls = 2, kConfMaxCls = 127;

// elements of an accumulator: the matrix, the out-of-range counter, the four occupancy bins
constexpr size_t conf_acc_len(int ncls) { return (size_t)ncls * ncls + 1 + 4; }

// Enqueues the count of n pairs into acc on st (see the contract above); n = 0 launches nothing.
int launch_confusion(hipStream_t st, const void* true_labels, int label_kind, const unsigned char* pred,
                     const unsigned char* mask_or_null, size_t n, int ncls, unsigned long long* acc);

}  // namespace ics
