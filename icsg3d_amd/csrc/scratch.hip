// The per-thread caches of the host-pointer ops (scratch.h): the op stream and the grow-only device scratch.
#include "scratch.h"
#include "../../include/icsg3d.h"

#include <algorithm>
#include <mutex>

namespace ics {
namespace {

// One resource of type R per host thread, bound to the device it was made on.  A host thread that used the ops and then
// exits (a pool worker, a loader thread) must not leak its resource until the process ends -- and a thread_local
// destructor must not call into a HIP runtime that may already be shutting down.  So the destructor only hands the
// resource to a process-wide list of orphans; the next creation on any thread, and release(), destroy them.
template <typename R, void (*Destroy)(R&)>
class ThreadCache {
 public:
  // *out = the calling thread's resource, or nullptr if it has none on the current device
  static int current(R** out) {
    int dev = 0;
    ICS_HIP(hipGetDevice(&dev));
    *out = tl_.device == dev ? &tl_.r : nullptr;
    return 0;
  }
  // replaces the calling thread's resource by what make(&r) builds on the current device
  template <typename Make> static int renew(Make make, R** out) {
    int dev = 0;
    ICS_HIP(hipGetDevice(&dev));
    release();
    ICS_TRY(make(&tl_.r));
    tl_.device = dev;
    *out = &tl_.r;
    return 0;
  }
  static void release() {
    if (tl_.device >= 0) Destroy(tl_.r);
    tl_.r = R{}; tl_.device = -1;
    std::vector<R> take;
    { std::lock_guard<std::mutex> lk(mu_); take.swap(orphans_); }
    for (R& r : take) Destroy(r);
  }

 private:
  struct Holder {
    R r{};
    int device = -1;      // -1: no resource
    ~Holder() {
      if (device >= 0) { std::lock_guard<std::mutex> lk(mu_); orphans_.push_back(r); }
    }
  };
  static inline std::mutex mu_;
  static inline std::vector<R> orphans_;
  static inline thread_local Holder tl_;
};

struct Buf { unsigned char* p = nullptr; size_t cap = 0; };
void free_buf(Buf& b) { (void)hipFree(b.p); }
void destroy_stream(hipStream_t& s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
using ScratchCache = ThreadCache<Buf, free_buf>;
using StreamCache = ThreadCache<hipStream_t, destroy_stream>;

}  // namespace

int op_stream(hipStream_t* out) {
  hipStream_t* s = nullptr;
  ICS_TRY(StreamCache::current(&s));
  if (s == nullptr)
    ICS_TRY(StreamCache::renew([](hipStream_t* n) { ICS_HIP(hipStreamCreateWithFlags(n, hipStreamNonBlocking)); return 0; }, &s));
  *out = *s;
  return 0;
}

// A hipMalloc / hipFree pair per call (the free synchronises the device) cost more than the kernels of the box-level ops,
// which run tens of times per sample with a few tens of KB each: the buffer only grows, by half as much again.
int scratch_get(size_t bytes, unsigned char** out) {
  Buf* b = nullptr;
  ICS_TRY(ScratchCache::current(&b));
  if (b == nullptr || b->cap < bytes)
    ICS_TRY(ScratchCache::renew([bytes](Buf* n) {
      const size_t want = std::max(bytes + bytes / 2, (size_t)1 << 20);
      ICS_HIP(hipMalloc(reinterpret_cast<void**>(&n->p), want));
      n->cap = want;
      return 0;
    }, &b));
  *out = b->p;
  return 0;
}

}  // namespace ics

// frees the calling thread's stream and scratch, and those that exited threads left behind
extern "C" int ics_release_caches() {
  ics::StreamCache::release();
  ics::ScratchCache::release();
  return 0;
}
