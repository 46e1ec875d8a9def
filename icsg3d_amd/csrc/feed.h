// Declarations for feed.hip: staging slots, a copy stream and the pack kernel that take the batch upload and the host-side
// cast / concatenate / label work off the train step (include/icsg3d.h, "fed steps").
//
// A feed is attached to one engine.  It owns `slots` staging slots -- a pinned host buffer and a device staging buffer of
// the same layout (up to two x parts, a label source, cond, eps; each part at a 256-byte aligned offset, sized for
// max_batch) -- one non-blocking stream feed_st, two events per slot (uploaded, consumed) and a pinned ring of 64 metric
// entries with an event each.  The device staging comes from the engine's allocator (guard bytes under
// ICSG3D_DEBUG_CANARY), as one allocation per slot that stays with the engine when the feed closes: re-opening
// allocates nothing, and a later feed with a larger layout gives the smaller buffer back before it takes its own.
//
// ORDERING RULES -- the whole correctness argument:
//  1. submit(slot, batch):   feed_st waits on consumed[slot];
//                            one hipMemcpyAsync per part, pinned -> device staging, of the bytes `batch` samples use
//                            (a rotation table's orientation bytes are one more part, the slot's last);
//                            uploaded[slot] is recorded on feed_st.
//  2. step_fed(slot):        the compute stream n.st waits on uploaded[slot];
//                            the pack kernel runs ON n.st, reads staging, writes n.x_in, n.labels, n.cond_in, n.eps_in;
//                            consumed[slot] is recorded on n.st;
//                            the bookkeeping of unet_upload / vae_upload is set (resident_batch, labels_batch, pred_kind,
//                            enc_batch, recon_fresh);
//                            the existing resident step runs, without its final stream synchronisation.
//     The engine's input buffers stay single: a whole step reads x_in (c1's weight gradient does), and the pack kernel
//     of step k+1 is ordered behind step k because both are on n.st.  So the upload of batch k+1 overlaps step k, its
//     pack does not, and no pointer is swapped.
//  3. The host may rewrite a slot's pinned buffer once uploaded[slot] has completed: ics_net_feed_slot blocks on exactly
//     that event.  The staging copy is protected by rule 1 (the next upload waits for the pack that read it).
//  4. Metrics: the fed step copies d_metrics into the next ring entry on n.st, records that entry's event and returns
//     the entry's ticket; ics_net_feed_metrics waits on that one event.  A fed step always takes the "metrics wanted"
//     path of the step, so the rank reduction under data parallelism behaves as in the synchronous step.
//
// Label ids outside 0..255 and non-integer ids are the caller's error, as in the host path the kernel replaces
// (ndarray.astype(np.uint8)): they are converted as (uint8)(int)v and nothing checks them.
#pragma once
#include "common.h"
#include "../../include/icsg3d.h"

namespace ics {

constexpr int kFeedMaxSlots = 4;
constexpr int kFeedRing = 64;        // metric entries kept
constexpr int kFeedMetricFloats = 8; // floats per ring entry (5 U-Net, 4 VAE)
constexpr int kDtypeF32 = 0, kDtypeF64 = 3;   // ics_op_render_slice's codes, plus float64
enum FeedLabels : int { FEED_LABELS_NONE = 0, FEED_LABELS_U8 = 1, FEED_LABELS_F64 = 2, FEED_LABELS_F32 = 3, FEED_LABELS_ONEHOT = 4 };

// One launch of the pack kernel.  nvox = batch * d^3 (a multiple of 512).  Every source pointer is 16-byte aligned.
struct FeedPack {
  const void* x[2] = {nullptr, nullptr};
  int xc[2] = {0, 0};
  int xdt[2] = {0, 0};
  int nparts = 0;
  const void* lab = nullptr;
  int label_kind = FEED_LABELS_NONE;
  int ncls = 0;
  size_t nvox = 0;
  float* x_out = nullptr;            // [nvox][xc[0] + xc[1]]
  unsigned char* lab_out = nullptr;  // [nvox]
  const float* tail_src[2] = {nullptr, nullptr};   // cond, eps: float32 passthrough
  float* tail_dst[2] = {nullptr, nullptr};
  size_t tail_n[2] = {0, 0};
  const unsigned char* orient = nullptr;   // [nvox / d^3] orientation bytes (orient.h); null: no sample is rotated
  int d = 0;                               // grid edge (read with orient only)
};
// bytes per voxel of a label source (0: none)
size_t feed_label_bytes(int label_kind, int ncls);
// the x parts and the label kind of a config (not its slot count); `who` prefixes the message
int feed_config_check(const char* who, const ics_feed_config* cfg, int in_channels, int ncls, bool want_labels);
// p.orient set: the rotating pack (feed_pack_rot_kernel); null: feed_pack_kernel
int launch_feed_pack(hipStream_t st, const FeedPack& p);
// a rotation table [batch][3] (entries -1..2) as one orientation byte a sample; *any: some sample is rotated.  An entry
// outside -1..2 is refused, naming the sample and the value.
int feed_orientations(const char* who, const int32_t* rot, int batch, unsigned char* out, bool* any);

// ---- what feed.hip needs of the engine behind an ics_net; defined in engine.hip, where Net lives
struct Feed;
struct FeedPort {
  int kind = 0;          // 0 U-Net, 1 VAE
  int max_batch = 0, d = 0, C = 0, ncls = 0, ncond = 0, latent = 0;
  hipStream_t st = nullptr;
  float* x_in = nullptr;
  unsigned char* labels = nullptr;
  float *cond_in = nullptr, *eps_in = nullptr;
  const float* d_metrics = nullptr;
  Feed** feed = nullptr; // the engine's open feed (owned by feed.hip; nullptr: none)
};
int feed_port(ics_net* net, FeedPort* out);
// device staging of slot `slot`: at least `bytes`, kept by the engine across feeds
int feed_port_stage(ics_net* net, int slot, size_t bytes, unsigned char** out);
// the bookkeeping of unet_upload / vae_upload for `batch` samples, then the resident train / test step, enqueued only
int feed_port_step(ics_net* net, int batch, int training);
// after a ticket's event: the profiler's pending rows (waits for the stream first while profiling is on)
int feed_port_resolve(ics_net* net);
// ics_net_destroy: closes the engine's feed if one is open
void feed_release(ics_net* net);

}  // namespace ics
