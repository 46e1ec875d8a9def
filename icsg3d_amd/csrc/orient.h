// Quarter-turn rotations of a d^3 grid as index arithmetic, shared by the voxeliser (voxelise.hip) and the rotating pack
// of the feed (feed.hip).  Plain C++ that compiles for host and device; hoststub/orient_check.cpp walks it on the CPU.
//
// A rotation table is {r0, r1, r2}, each in {-1, 0, 1, 2}: r >= 0 is np.rot90(X, 1, axes=[(0,1), (0,2), (1,2)][r]), applied
// in the order r0, r1, r2; -1 is nothing.  rot_source is one such turn read backwards (where an output voxel comes from),
// so a table is undone last-first: rot_source(r2), rot_source(r1), rot_source(r0).
//
// Any table composes to ONE orientation, a signed axis permutation:
//     src[a] = flip[a] ? d - 1 - out[perm[a]] : out[perm[a]],   a = 0, 1, 2,
// held in a byte: bits 0-1 perm[0], bits 2-3 perm[1] (perm[2] is what is left), bits 4-6 flip[0..2].
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ICS_HD __host__ __device__ __forceinline__
#else
#define ICS_HD inline
#endif

namespace ics {

// np.rot90(X, 1, axes=(a0, a1)) reads out[idx] = X[src] with src[a0] = idx[a1], src[a1] = d-1-idx[a0]
ICS_HD void rot_source(int code, int d, int& i, int& j, int& k) {
  int t;
  switch (code) {
    case 0: t = i; i = j; j = d - 1 - t; break;   // axes (0,1)
    case 1: t = i; i = k; k = d - 1 - t; break;   // axes (0,2)
    case 2: t = j; j = k; k = d - 1 - t; break;   // axes (1,2)
    default: break;
  }
}

constexpr unsigned char kOrientIdentity = 0x04;   // perm (0, 1, 2), no flips

struct Orient {
  int p0, p1, p2;   // perm
  int f0, f1, f2;   // flip (0 / 1)
};
ICS_HD Orient orient_decode(unsigned char o) {
  Orient r;
  r.p0 = o & 3; r.p1 = (o >> 2) & 3; r.p2 = 3 - r.p0 - r.p1;
  r.f0 = (o >> 4) & 1; r.f1 = (o >> 5) & 1; r.f2 = (o >> 6) & 1;
  return r;
}
ICS_HD int orient_pick(int p, int i, int j, int k) { return p == 0 ? i : (p == 1 ? j : k); }
// the source voxel of output voxel (i, j, k)
ICS_HD void orient_source(const Orient& o, int d, int& i, int& j, int& k) {
  const int a = orient_pick(o.p0, i, j, k), b = orient_pick(o.p1, i, j, k), c = orient_pick(o.p2, i, j, k);
  i = o.f0 ? d - 1 - a : a;
  j = o.f1 ? d - 1 - b : b;
  k = o.f2 ? d - 1 - c : c;
}
ICS_HD long long orient_source_voxel(const Orient& o, int d, long long v) {   // both linear, inside one sample
  int i = (int)(v / ((long long)d * d)), j = (int)((v / d) % d), k = (int)(v % d);
  orient_source(o, d, i, j, k);
  return ((long long)i * d + j) * d + k;
}

// The orientation of a table, by probing rot_source itself: where the origin and the three unit steps come from.
inline unsigned char orient_compose(const int rot[3]) {
  const int d = 4;
  int s[4][3];
  for (int e = 0; e < 4; ++e) {
    int i = e == 1, j = e == 2, k = e == 3;
    rot_source(rot[2], d, i, j, k);
    rot_source(rot[1], d, i, j, k);
    rot_source(rot[0], d, i, j, k);
    s[e][0] = i; s[e][1] = j; s[e][2] = k;
  }
  int perm[3] = {0, 0, 0}, flip[3] = {0, 0, 0};
  for (int b = 0; b < 3; ++b)          // a unit step along output axis b moves exactly one source axis, by +1 or -1
    for (int a = 0; a < 3; ++a) {
      const int delta = s[b + 1][a] - s[0][a];
      if (delta != 0) { perm[a] = b; flip[a] = delta < 0; }
    }
  return (unsigned char)(perm[0] | (perm[1] << 2) | (flip[0] << 4) | (flip[1] << 5) | (flip[2] << 6));
}

// ---- the tiles of the rotating pack.  A sample is cut into d^3 / T^2 units of T x T voxels, T = min(d, 32).
//  class A (perm[2] == 2: the source's fastest axis is the output's): unit t is the output voxels [t T^2, (t + 1) T^2); a
//          quad of four output voxels along k comes from one aligned source quad, reversed when flip[2].
//  class B (perm[2] = b in {0, 1}): unit t = (w, tu, tk) is the T x T tile k0 <= k < k0 + T, u0 <= u < u0 + T of the plane
//          (output axis 2, output axis b) at index w of the third output axis c = 1 - b.  Source axis 2 runs along u, the
//          source axis a with perm[a] == 2 along k, the third source axis e = 1 - a is fixed by w.  Row r of the tile in
//          LDS is source index sa0 + r along a, a run of T voxels from s20 along source axis 2.
ICS_HD int orient_tile(int d) { return d < 32 ? d : 32; }
struct OrientTile {
  int a, b;            // source axis that feeds output axis 2; output axis that source axis 2 feeds
  int w, u0, k0;       // the unit's place in the output
  int se, sa0, s20;    // the unit's place in the source
  int fa, f2;          // flips of source axis a and of source axis 2
};
ICS_HD OrientTile orient_tile_of(const Orient& o, int d, int t) {
  const int T = orient_tile(d), n = d / T;
  OrientTile r;
  r.b = o.p2;
  r.a = o.p0 == 2 ? 0 : 1;
  r.w = t / (n * n); r.u0 = (t / n) % n * T; r.k0 = t % n * T;
  const int fe = r.a == 0 ? o.f1 : o.f0;
  r.fa = r.a == 0 ? o.f0 : o.f1;
  r.f2 = o.f2;
  r.se = fe ? d - 1 - r.w : r.w;
  r.sa0 = r.fa ? d - T - r.k0 : r.k0;
  r.s20 = r.f2 ? d - T - r.u0 : r.u0;
  return r;
}
// source voxel (linear, inside the sample) of tile row r, column c: c runs along source axis 2
ICS_HD long long orient_tile_source(const OrientTile& t, int d, int r, int c) {
  const int sa = t.sa0 + r;
  return ((long long)(t.a == 0 ? sa : t.se) * d + (t.a == 0 ? t.se : sa)) * d + t.s20 + c;
}
// output voxel of (u, k), both relative to the tile
ICS_HD long long orient_tile_output(const OrientTile& t, int d, int u, int k) {
  const int U = t.u0 + u;
  return ((long long)(t.b == 0 ? U : t.w) * d + (t.b == 0 ? t.w : U)) * d + t.k0 + k;
}
// where output (u, k) of the tile lies in LDS: (row, column)
ICS_HD int orient_tile_row(const OrientTile& t, int T, int k) { return t.fa ? T - 1 - k : k; }
ICS_HD int orient_tile_col(const OrientTile& t, int T, int u) { return t.f2 ? T - 1 - u : u; }

}  // namespace ics
