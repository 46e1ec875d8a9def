// What a host-pointer op (ics_op_*, the resident render entry points) needs from its calling thread: a stream, a grow-only
// device scratch, and a typed layout that carves the scratch into segments.  One per-thread cache mechanism (scratch.hip)
// holds both the stream and the scratch.
#pragma once
#include "common.h"

namespace ics {

// v rounded up to a multiple of a (a power of two)
constexpr size_t align_up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }

// The calling thread's stream for the host-pointer ops (non-blocking, created on first use and kept: a handle with two
// streams, two events and its own allocations per call cost 10 - 16 ms against kernels of tens of microseconds).
int op_stream(hipStream_t* out);
// The calling thread's grow-only device scratch (>= bytes; contents not kept across calls that grow it).  Layout::reserve
// is its only caller.
int scratch_get(size_t bytes, unsigned char** out);

// One segment of a Layout: `count` elements of T at byte offset `off`.  count = 0: no space, a null pointer.
template <typename T> struct Seg { size_t off = 0, count = 0; };

// Segments declared in order; the only source of the total size and of every offset.  Every segment starts at a multiple
// of `align` (256 for device scratch; 16 for the packed single-copy blocks of structure.hip / structure_match.hip, which
// apply one layout to a host vector and to the device block).  Lives on the stack: no allocation.
class Layout {
 public:
  explicit Layout(size_t align = 256) : align_(align) {}
  template <typename T> Seg<T> add(size_t count) {
    const Seg<T> s{end_, count};
    end_ = align_up(end_ + count * sizeof(T), align_);
    return s;
  }
  size_t bytes() const { return end_; }
  // binds the layout to the calling thread's scratch, grown to bytes(), or to `cap` bytes at `base` (a host vector, a
  // segment of another layout); then *out = each segment's address, as ptr() gives it
  template <typename... SegOut> int reserve(SegOut... seg_out) {
    ICS_TRY(scratch_get(end_, &base_));
    cap_ = end_;
    return ptrs(seg_out...);
  }
  template <typename... SegOut> int bind(void* base, size_t cap, SegOut... seg_out) {
    ICS_CHECK(base != nullptr && cap >= end_, "scratch layout: bound to a block smaller than its segments");
    base_ = static_cast<unsigned char*>(base); cap_ = cap;
    return ptrs(seg_out...);
  }
  // refused unless the layout is bound and the segment (count elements of it) lies inside the block
  template <typename T> int ptr(Seg<T> s, T** out, size_t count = 0) const {
    ICS_CHECK(base_ != nullptr, "scratch layout: segment taken before reserve / bind");
    ICS_CHECK(s.off + s.count * sizeof(T) <= cap_, "scratch layout: segment lies outside the reserved block");
    ICS_CHECK(count <= s.count, "scratch layout: copy or fill longer than its segment");
    *out = s.count ? reinterpret_cast<T*>(base_ + s.off) : nullptr;
    return 0;
  }
  int ptrs() const { return 0; }
  template <typename T, typename... Rest> int ptrs(Seg<T> s, T** out, Rest... rest) const {
    ICS_TRY(ptr(s, out));
    return ptrs(rest...);
  }
  // copies and fills of the first `count` elements of a segment, on st; a count above the segment's is refused
  template <typename T> int upload(Seg<T> s, const void* host, size_t count, hipStream_t st) const {
    T* d = nullptr;
    ICS_TRY(ptr(s, &d, count));
    if (count) ICS_HIP(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, st));
    return 0;
  }
  template <typename T> int download(void* host, Seg<T> s, size_t count, hipStream_t st) const {
    T* d = nullptr;
    ICS_TRY(ptr(s, &d, count));
    if (count) ICS_HIP(hipMemcpyAsync(host, d, count * sizeof(T), hipMemcpyDeviceToHost, st));
    return 0;
  }
  template <typename T> int fill(Seg<T> s, int byte, size_t count, hipStream_t st) const {
    T* d = nullptr;
    ICS_TRY(ptr(s, &d, count));
    if (count) ICS_HIP(hipMemsetAsync(d, byte, count * sizeof(T), st));
    return 0;
  }

 private:
  size_t align_, end_ = 0, cap_ = 0;
  unsigned char* base_ = nullptr;
};

}  // namespace ics
