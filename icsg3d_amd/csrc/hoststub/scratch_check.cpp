// Stand-alone check of scratch.h / scratch.hip under AddressSanitizer and LeakSanitizer (`make asan`): linked against
// hip_host_stub.cpp only, so "device" memory is malloc memory and a leaked scratch or stream is a reported leak.
#include "scratch.h"
#include "icsg3d.h"

#include <sanitizer/asan_interface.h>

#include <cstdlib>
#include <thread>

namespace ics {
static std::string g_msg;
void set_error(const std::string& msg) { g_msg = msg; }
}  // namespace ics
using namespace ics;

#define REQUIRE(cond)                                                       \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "scratch_check: %s failed @%d (last error: %s)\n", #cond, __LINE__, g_msg.c_str()); \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)
// the call is refused: -1 and a message
#define REFUSED(expr)                      \
  do {                                     \
    g_msg.clear();                         \
    REQUIRE((expr) == -1 && !g_msg.empty()); \
  } while (0)

template <typename T> static unsigned char* bytes_of(T* p) { return reinterpret_cast<unsigned char*>(p); }

static void check_layout(size_t align) {
  Layout L(align);
  const auto a = L.add<float>(3);
  const auto z = L.add<double>(0);
  const auto b = L.add<unsigned char>(align + 1);
  const auto c = L.add<double>(5);
  // in order, each at a multiple of the alignment, the total the rounded end of the last
  REQUIRE(a.off == 0 && b.off == align_up(3 * sizeof(float), align) && c.off == b.off + 2 * align);
  REQUIRE(a.off % align == 0 && b.off % align == 0 && c.off % align == 0);
  REQUIRE(L.bytes() == align_up(c.off + 5 * sizeof(double), align));
  REQUIRE(z.off == b.off);                                  // the empty segment took no space
  float* pa = nullptr;
  REFUSED(L.ptr(a, &pa));                                   // not reserved yet
  REQUIRE(pa == nullptr);
  REQUIRE(L.reserve() == 0);
  double *pz = reinterpret_cast<double*>(&pa), *pc = nullptr;
  unsigned char* pb = nullptr;
  REQUIRE(L.ptrs(a, &pa, z, &pz, b, &pb, c, &pc) == 0);
  REQUIRE(pz == nullptr);
  REQUIRE(bytes_of(pa) + 3 * sizeof(float) <= pb && pb + align + 1 <= bytes_of(pc));   // disjoint
  REQUIRE(bytes_of(pc) + 5 * sizeof(double) <= bytes_of(pa) + L.bytes());
  // a segment declared after the reservation lies outside it
  const auto late = L.add<int>(1);
  int* pl = nullptr;
  REFUSED(L.ptr(late, &pl));
  REQUIRE(pl == nullptr);
}

static void check_copies() {
  Layout L;
  const auto a = L.add<int>(4);
  const auto b = L.add<int>(4);
  const int src[5] = {1, 2, 3, 4, 5};
  int back[5] = {0, 0, 0, 0, 0};
  REFUSED(L.upload(a, src, 4, nullptr));                    // not reserved
  REQUIRE(L.reserve() == 0);
  int *pa, *pb;
  REQUIRE(L.ptrs(a, &pa, b, &pb) == 0);
  REQUIRE(L.fill(a, 0, 4, nullptr) == 0 && L.fill(b, 0, 4, nullptr) == 0);
  REFUSED(L.upload(a, src, 5, nullptr));                    // one element too many: refused, nothing copied
  REQUIRE(pa[0] == 0 && pa[3] == 0 && pb[0] == 0);
  REFUSED(L.fill(a, 0xff, 5, nullptr));
  REQUIRE(pa[0] == 0 && pa[3] == 0);
  REQUIRE(L.upload(a, src, 4, nullptr) == 0);
  REFUSED(L.download(back, a, 5, nullptr));
  REQUIRE(back[0] == 0 && back[4] == 0);
  REQUIRE(L.download(back, a, 4, nullptr) == 0);
  REQUIRE(back[0] == 1 && back[3] == 4 && back[4] == 0);
  // a packed layout over a host block, and over a block too small for it
  Layout P(16);
  const auto x = P.add<double>(3);
  const auto y = P.add<int>(1);
  unsigned char block[48];
  REQUIRE(P.bytes() == 48);
  REFUSED(P.bind(block, 47));
  REQUIRE(P.bind(block, sizeof(block)) == 0);
  double* px;
  int* py;
  REQUIRE(P.ptrs(x, &px, y, &py) == 0);
  REQUIRE(bytes_of(px) == block && bytes_of(py) == block + 32);
}

static void check_growth() {
  unsigned char *p0, *p1, *p2, *p3;
  REQUIRE(scratch_get(1000, &p0) == 0);
  p0[((size_t)1 << 20) - 1] = 1;                            // the 1 MB floor
  REQUIRE(scratch_get((size_t)4 << 20, &p1) == 0);          // grows: by half as much again
  p1[((size_t)6 << 20) - 1] = 1;
  REQUIRE(scratch_get(1000, &p2) == 0 && p2 == p1);         // smaller again: the same buffer
  REQUIRE(scratch_get((size_t)6 << 20, &p3) == 0 && p3 == p1);
}

int main() {
  check_layout(256);
  check_layout(16);
  check_copies();
  check_growth();
  // a thread that used both caches and exits leaves them to the orphan lists; release frees them (LeakSanitizer at exit)
  hipStream_t main_st = nullptr, thread_st = nullptr;
  unsigned char* thread_buf = nullptr;
  REQUIRE(op_stream(&main_st) == 0 && main_st != nullptr);
  std::thread([&] {
    REQUIRE(scratch_get(100, &thread_buf) == 0 && thread_buf != nullptr);
    REQUIRE(op_stream(&thread_st) == 0 && thread_st != nullptr);
  }).join();
  REQUIRE(thread_st != main_st);
  REQUIRE(!__asan_address_is_poisoned(thread_st) && !__asan_address_is_poisoned(thread_buf));   // orphaned, not destroyed
  hipStream_t again = nullptr;
  REQUIRE(op_stream(&again) == 0 && again == main_st);
  (void)ics_release_caches();
  REQUIRE(__asan_address_is_poisoned(thread_st) && __asan_address_is_poisoned(thread_buf) && __asan_address_is_poisoned(main_st));
  (void)ics_release_caches();                               // nothing left: a no-op
  std::puts("scratch_check: ok");
  return 0;
}
