// orient.h on the CPU: the composed orientation of every rotation table against the chain of rot_source calls it stands
// for, and the unit / tile arithmetic of the rotating pack kernel (feed.hip) walked exactly as the kernel walks it -- every
// global and LDS index in bounds, every quad aligned, every output voxel written once from the voxel the chain names.
#include "../orient.h"

#include <cstdio>
#include <set>
#include <vector>

using namespace ics;

static int fail(const char* what, int d, const int* rot) {
  std::fprintf(stderr, "orient_check: %s (d %d, table %d %d %d)\n", what, d, rot[0], rot[1], rot[2]);
  return 1;
}

int main() {
  std::set<int> orients, classes, plain;
  for (int d : {8, 16, 32, 64}) {
    const int T = orient_tile(d), TT = T * T, qrow = T / 4;
    const long long V = (long long)d * d * d;
    std::vector<long long> want((size_t)V), got((size_t)V);
    for (int code = 0; code < 64; ++code) {
      const int rot[3] = {code / 16 - 1, code / 4 % 4 - 1, code % 4 - 1};
      const unsigned char ob = orient_compose(rot);
      const Orient o = orient_decode(ob);
      if (d == 8) {
        orients.insert(ob);
        classes.insert(o.p2 * 2 + o.f2);
        if (rot[0] >= 0 && rot[1] >= 0 && rot[2] >= 0) plain.insert(ob);
      }
      if ((ob == kOrientIdentity) != (o.p0 == 0 && o.p1 == 1 && !o.f0 && !o.f1 && !o.f2)) return fail("identity byte", d, rot);
      for (long long v = 0; v < V; ++v) {
        int i = (int)(v / (d * d)), j = (int)(v / d % d), k = (int)(v % d);
        rot_source(rot[2], d, i, j, k);
        rot_source(rot[1], d, i, j, k);
        rot_source(rot[0], d, i, j, k);
        want[(size_t)v] = ((long long)i * d + j) * d + k;
        if (orient_source_voxel(o, d, v) != want[(size_t)v]) return fail("composed orientation differs from the chain", d, rot);
        got[(size_t)v] = -1;
      }
      auto put = [&](long long out, long long src) {
        if (out < 0 || out >= V || src < 0 || src >= V || got[(size_t)out] != -1) return false;
        got[(size_t)out] = src;
        return true;
      };
      for (int t = 0; t < (int)(V / TT); ++t) {
        if (o.p2 == 2) {                                   // class A, as the kernel
          for (int q = 0; q < TT / 4; ++q) {
            const long long vo = (long long)t * TT + 4 * q;
            int i = (int)(vo / (d * d)), j = (int)(vo / d % d), k = (int)(vo % d);
            if (o.f2) k += 3;
            orient_source(o, d, i, j, k);
            const long long vs = ((long long)i * d + j) * d + k;
            if (vs % 4 || vo % 4 || vs + 3 >= V) return fail("class A quad", d, rot);
            for (int e = 0; e < 4; ++e)
              if (!put(vo + e, o.f2 ? vs + 3 - e : vs + e)) return fail("class A store", d, rot);
          }
          continue;
        }
        const OrientTile tl = orient_tile_of(o, d, t);     // class B
        std::vector<long long> lds((size_t)T * (T + 1), -1);
        for (int q = 0; q < T * qrow; ++q) {
          const int r = q / qrow, c = q % qrow * 4;
          const long long vs = orient_tile_source(tl, d, r, c);
          if (vs % 4 || vs < 0 || vs + 3 >= V) return fail("class B load", d, rot);
          for (int e = 0; e < 4; ++e) lds[(size_t)r * (T + 1) + c + e] = vs + e;
        }
        for (int u = 0; u < T; ++u)
          for (int k = 0; k < T; ++k) {
            const int row = orient_tile_row(tl, T, k), col = orient_tile_col(tl, T, u);
            if (row < 0 || row >= T || col < 0 || col >= T) return fail("class B LDS index", d, rot);
            const long long out = orient_tile_output(tl, d, u, k);
            if (k % 4 == 0 && out % 4) return fail("class B store quad", d, rot);
            if (!put(out, lds[(size_t)row * (T + 1) + col])) return fail("class B store", d, rot);
          }
      }
      for (long long v = 0; v < V; ++v)
        if (got[(size_t)v] != want[(size_t)v]) return fail("a unit wrote another voxel than the chain names", d, rot);
    }
  }
  // 64 tables are 20 orientations in all six access classes; three positive turns reach 12, never the identity
  if (orients.size() != 20 || classes.size() != 6 || plain.size() != 12 || plain.count(kOrientIdentity)) {
    std::fprintf(stderr, "orient_check: %zu orientations, %zu classes, %zu from positive tables\n", orients.size(),
                 classes.size(), plain.size());
    return 1;
  }
  std::puts("orient_check: ok");
  return 0;
}
