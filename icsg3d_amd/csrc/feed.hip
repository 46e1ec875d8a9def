// Fed steps (gfx950 / MI355X only): pinned staging slots uploaded on a copy stream while the previous step runs, and the
// pack kernel that does on the device what the synchronous path does on host threads -- float64 -> float32, the (M | p)
// channel concatenate, labels to uint8 class ids (argmax of a one-hot included).  feed.h has the ordering rules.
#include "feed.h"
#include "orient.h"
#include "scratch.h"

#include <climits>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace ics {

// ------------------------------------------------------------------------------------------ the pack kernel
// Purely memory-bound: every byte is read once and written once, so the only rules are wide, contiguous accesses.
//   quad blocks    one lane = 4 consecutive voxels.  Each x part is read with 16-byte loads (a float32 quad is one load, a
//                  float64 quad two; a lane's loads are adjacent, a wave covers one contiguous range) and written as
//                  float4: C = 1 one store per four voxels, C = 4 (1 + 3 channels) one store per voxel.  Id labels ride
//                  along: four ids in, one 32-bit store of four bytes out.
//   one-hot blocks 16 lanes per voxel stride the columns (any count from 2 to 127), then four xor-shuffle steps reduce
//                  (value, index) under np.argmax's rule: the larger value (a NaN above every number), the lower index
//                  among equals.  Four voxels per wave and pass; lane 0 stores their four bytes at once.
//   tail blocks    cond and eps, float32 passthrough.
// nvox is a multiple of 512 (d is a power of two >= 8), so quads and 64-voxel one-hot blocks always divide.
constexpr int kPackThreads = 256;
constexpr int kPackOneHotVox = 64;    // voxels per one-hot block: 4 waves x 4 voxels x 4 passes
constexpr int kPackTailBlocks = 8;

template <typename T> __device__ __forceinline__ float4 load4(const T* p);
template <> __device__ __forceinline__ float4 load4<float>(const float* p) { return *reinterpret_cast<const float4*>(p); }
template <> __device__ __forceinline__ float4 load4<double>(const double* p) {
  const double2 a = reinterpret_cast<const double2*>(p)[0];
  const double2 b = reinterpret_cast<const double2*>(p)[1];
  return make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);   // v_cvt_f32_f64: round to nearest even
}
__device__ __forceinline__ unsigned id_byte(float v) { return (unsigned)(unsigned char)(int)v; }
__device__ __forceinline__ unsigned pack_ids(float4 v) {
  return id_byte(v.x) | (id_byte(v.y) << 8) | (id_byte(v.z) << 16) | (id_byte(v.w) << 24);
}
// np.argmax's order: a NaN is above every number (the first NaN wins), two NaNs are equal
__device__ __forceinline__ bool arg_above(float a, float b) { return a > b || (a != a && b == b); }
__device__ __forceinline__ float load_as_float(const void* p, int dt, size_t i) {
  return dt == kDtypeF64 ? (float)static_cast<const double*>(p)[i] : static_cast<const float*>(p)[i];
}

// One one-hot block: 64 voxels.  ROT: voxel v of the output reads the row of its source voxel (a row is contiguous).
template <bool ROT>
__device__ __forceinline__ void pack_onehot_block(const FeedPack& p, unsigned rel) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = lane >> 4, gl = lane & 15;
  const float* lab = static_cast<const float*>(p.lab);
  for (int pass = 0; pass < 4; ++pass) {
    const size_t base = (size_t)rel * kPackOneHotVox + pass * 16 + wave * 4;   // wave-uniform
    if (base + 4 > p.nvox) break;
    size_t src = base + grp;
    if (ROT) {
      const size_t V = (size_t)p.d * p.d * p.d, b = base / V;                  // four voxels never straddle two samples
      const Orient o = orient_decode((unsigned char)__builtin_amdgcn_readfirstlane((int)p.orient[b]));
      src = b * V + (size_t)orient_source_voxel(o, p.d, (long long)(src - b * V));
    }
    const float* row = lab + src * (size_t)p.ncls;
    float best = -INFINITY;
    int bidx = INT_MAX;                        // no column taken yet: loses every tie
    for (int c = gl; c < p.ncls; c += 16) {
      const float v = row[c];
      if (arg_above(v, best)) { best = v; bidx = c; }   // ascending columns, strictly above: the lowest index of this lane's maxima
    }
    for (int off = 8; off >= 1; off >>= 1) {
      const float ov = __shfl_xor(best, off);
      const int oi = __shfl_xor(bidx, off);
      if (arg_above(ov, best) || (!arg_above(best, ov) && oi < bidx)) { best = ov; bidx = oi; }
    }
    if (bidx == INT_MAX) bidx = 0;             // a row without a value above -inf: argmax's first column
    const unsigned r0 = (unsigned)__shfl(bidx, 0), r1 = (unsigned)__shfl(bidx, 16), r2 = (unsigned)__shfl(bidx, 32),
                   r3 = (unsigned)__shfl(bidx, 48);
    if (lane == 0) reinterpret_cast<unsigned*>(p.lab_out)[base / 4] = r0 | (r1 << 8) | (r2 << 16) | (r3 << 24);
  }
}
__device__ __forceinline__ void pack_tail_block(const FeedPack& p, unsigned rel) {
  const size_t t0 = (size_t)rel * kPackThreads + threadIdx.x;
  const size_t stride = (size_t)kPackTailBlocks * kPackThreads;
  for (int k = 0; k < 2; ++k)
    for (size_t i = t0; i < p.tail_n[k]; i += stride) p.tail_dst[k][i] = p.tail_src[k][i];
}

// MODE 1: one part (any channel count: its layout is the output's).  MODE 4: parts of 1 + 3 channels.  MODE 0: any other
// split, element by element.
template <typename T0, typename T1, int MODE>
__global__ __launch_bounds__(kPackThreads) void feed_pack_kernel(FeedPack p, unsigned quad_blocks, unsigned onehot_blocks) {
  const unsigned blk = blockIdx.x;
  if (blk < quad_blocks) {
    const size_t q = (size_t)blk * kPackThreads + threadIdx.x;
    if (MODE == 1) {             // a cast copy of nvox * C elements: the quads run over elements, beyond the voxel quads
      if (q < p.nvox / 4 * p.xc[0]) reinterpret_cast<float4*>(p.x_out)[q] = load4(static_cast<const T0*>(p.x[0]) + 4 * q);
    }
    if (q >= p.nvox / 4) return;
    if (MODE == 4) {
      const float4 m = load4(static_cast<const T0*>(p.x[0]) + 4 * q);
      const T1* s = static_cast<const T1*>(p.x[1]) + 12 * q;
      const float4 a = load4(s), b = load4(s + 4), c = load4(s + 8);
      float4* o = reinterpret_cast<float4*>(p.x_out) + 4 * q;
      o[0] = make_float4(m.x, a.x, a.y, a.z);
      o[1] = make_float4(m.y, a.w, b.x, b.y);
      o[2] = make_float4(m.z, b.z, b.w, c.x);
      o[3] = make_float4(m.w, c.y, c.z, c.w);
    } else if (MODE == 0) {
      const int C = p.xc[0] + p.xc[1];
      for (int k = 0; k < 4; ++k) {
        const size_t v = 4 * q + k;
        float* o = p.x_out + v * C;
        for (int c = 0; c < p.xc[0]; ++c) o[c] = load_as_float(p.x[0], p.xdt[0], v * p.xc[0] + c);
        for (int c = 0; c < p.xc[1]; ++c) o[p.xc[0] + c] = load_as_float(p.x[1], p.xdt[1], v * p.xc[1] + c);
      }
    }
    if (p.label_kind == FEED_LABELS_U8)
      reinterpret_cast<unsigned*>(p.lab_out)[q] = static_cast<const unsigned*>(p.lab)[q];
    else if (p.label_kind == FEED_LABELS_F32)
      reinterpret_cast<unsigned*>(p.lab_out)[q] = pack_ids(load4(static_cast<const float*>(p.lab) + 4 * q));
    else if (p.label_kind == FEED_LABELS_F64)
      reinterpret_cast<unsigned*>(p.lab_out)[q] = pack_ids(load4(static_cast<const double*>(p.lab) + 4 * q));
    return;
  }
  if (blk < quad_blocks + onehot_blocks) { pack_onehot_block<false>(p, blk - quad_blocks); return; }
  pack_tail_block(p, blk - quad_blocks - onehot_blocks);
}

// ------------------------------------------------------------------------------------------ the rotating pack kernel
// out[b, i, j, k, :] = cast(src[b, s_b(i, j, k), :]) with s_b the sample's orientation (orient.h): a quarter-turn rotation
// is an index permutation of exactly the arrays the pack kernel reads, so it costs no pass of its own.  Launched only for
// a batch that has a rotated sample; everything else takes feed_pack_kernel above.
//   unit blocks    one block = one unit of T x T voxels of ONE sample (T = min(d, 32); d^3 / T^2 units per sample), so the
//                  orientation is block-uniform (read once, made scalar).
//       class A    the source's fastest axis is the output's (forward or reversed): no LDS.  A quad of four output voxels
//                  is one aligned source quad -- the 16-byte loads of feed_pack_kernel -- reversed in registers when the
//                  axis is flipped; float4 stores and 4-byte id stores as there.
//       class B    the source's fastest axis lands on output axis 0 or 1: the unit is a T x T tile in the plane of output
//                  axis 2 and that axis.  Quad loads run along source axis 2 into LDS rows (cast first, so a tile holds
//                  float32 whatever the files hold); the stores read the tile transposed and run along output axis 2.
//                  A row is padded by one voxel: 4 T + 4 floats at 1 + 3 channels, where the 16 lanes that one 16-byte
//                  LDS read serves together step by 4 banks and cover all 64 once; T + 1 floats at one channel and for
//                  the ids (kept as 32-bit words), an odd stride, so a column walks through all banks.  32 x 132 x 4 B +
//                  32 x 33 x 4 B = 21 KB a block: seven blocks fit a CU's 160 KB.
//       gather     MODE 0 (any other split, a single part of several channels): voxel by voxel through the same map.
//   one-hot, tail  the blocks of feed_pack_kernel; a one-hot voxel reads the row of its source voxel.
constexpr int kRotTile = 32;

__device__ __forceinline__ unsigned src_ids4(const FeedPack& p, size_t v) {   // ids of source voxels v .. v + 3 (v % 4 == 0), as four bytes
  if (p.label_kind == FEED_LABELS_U8) return static_cast<const unsigned*>(p.lab)[v / 4];
  if (p.label_kind == FEED_LABELS_F32) return pack_ids(load4(static_cast<const float*>(p.lab) + v));
  return pack_ids(load4(static_cast<const double*>(p.lab) + v));
}
__device__ __forceinline__ unsigned src_id(const FeedPack& p, size_t v) {
  if (p.label_kind == FEED_LABELS_U8) return static_cast<const unsigned char*>(p.lab)[v];
  return id_byte(load_as_float(p.lab, p.label_kind == FEED_LABELS_F64 ? kDtypeF64 : kDtypeF32, v));
}

// MODE 1: one part of ONE channel.  MODE 4: parts of 1 + 3 channels.  MODE 0: the gather.
template <typename T0, typename T1, int MODE>
__global__ __launch_bounds__(kPackThreads) void feed_pack_rot_kernel(FeedPack p, unsigned unit_blocks, unsigned onehot_blocks) {
  constexpr int XC = MODE == 4 ? 4 : 1;
  __shared__ __attribute__((aligned(16))) float xt[MODE == 0 ? 4 : kRotTile * (kRotTile * XC + XC)];
  __shared__ unsigned idt[MODE == 0 ? 4 : kRotTile * (kRotTile + 1)];
  const unsigned blk = blockIdx.x;
  if (blk >= unit_blocks) {
    if (blk < unit_blocks + onehot_blocks) pack_onehot_block<true>(p, blk - unit_blocks);
    else pack_tail_block(p, blk - unit_blocks - onehot_blocks);
    return;
  }
  const int d = p.d, T = orient_tile(d), TT = T * T, tid = threadIdx.x;
  const size_t V = (size_t)d * d * d;
  const unsigned per = (unsigned)(V / TT);                 // units per sample
  const unsigned b = blk / per;
  const int t = (int)(blk % per);
  const Orient o = orient_decode((unsigned char)__builtin_amdgcn_readfirstlane((int)p.orient[b]));
  const size_t s0 = (size_t)b * V;                         // the sample's first voxel
  const bool ids = p.label_kind == FEED_LABELS_U8 || p.label_kind == FEED_LABELS_F32 || p.label_kind == FEED_LABELS_F64;
  unsigned* lab_out = reinterpret_cast<unsigned*>(p.lab_out);

  if (MODE == 0) {
    const int C = p.xc[0] + p.xc[1];
    for (int q = tid; q < TT / 4; q += kPackThreads) {
      const size_t vo = (size_t)t * TT + 4 * q;
      unsigned w = 0;
      for (int k = 0; k < 4; ++k) {
        const size_t vs = s0 + (size_t)orient_source_voxel(o, d, (long long)(vo + k));
        float* out = p.x_out + (s0 + vo + k) * C;
        for (int c = 0; c < p.xc[0]; ++c) out[c] = load_as_float(p.x[0], p.xdt[0], vs * p.xc[0] + c);
        for (int c = 0; c < p.xc[1]; ++c) out[p.xc[0] + c] = load_as_float(p.x[1], p.xdt[1], vs * p.xc[1] + c);
        if (ids) w |= src_id(p, vs) << (8 * k);
      }
      if (ids) lab_out[(s0 + vo) / 4] = w;
    }
    return;
  }

  const T0* x0 = static_cast<const T0*>(p.x[0]);
  const T1* x1 = static_cast<const T1*>(p.x[1]);
  float4* out4 = reinterpret_cast<float4*>(p.x_out);
  if (o.p2 == 2) {                                         // class A
    for (int q = tid; q < TT / 4; q += kPackThreads) {
      const size_t vo = (size_t)t * TT + 4 * q;
      int i = (int)(vo / ((size_t)d * d)), j = (int)((vo / d) % d), k = (int)(vo % d);
      if (o.f2) k += 3;                                    // the quad's last voxel is the source quad's first
      orient_source(o, d, i, j, k);
      const size_t vs = s0 + ((size_t)i * d + j) * d + k, go = s0 + vo;
      const float4 m = load4(x0 + vs);
      if (MODE == 1) {
        out4[go / 4] = o.f2 ? make_float4(m.w, m.z, m.y, m.x) : m;
      } else {
        const T1* s = x1 + 3 * vs;
        const float4 a = load4(s), bb = load4(s + 4), c = load4(s + 8);
        const float4 v0 = make_float4(m.x, a.x, a.y, a.z), v1 = make_float4(m.y, a.w, bb.x, bb.y),
                     v2 = make_float4(m.z, bb.z, bb.w, c.x), v3 = make_float4(m.w, c.y, c.z, c.w);
        out4[go + 0] = o.f2 ? v3 : v0;
        out4[go + 1] = o.f2 ? v2 : v1;
        out4[go + 2] = o.f2 ? v1 : v2;
        out4[go + 3] = o.f2 ? v0 : v3;
      }
      if (ids) {
        const unsigned w = src_ids4(p, vs);
        lab_out[go / 4] = o.f2 ? __builtin_bswap32(w) : w;
      }
    }
    return;
  }

  // class B
  const OrientTile tl = orient_tile_of(o, d, t);
  const int qrow = T / 4, S = T * XC + XC, SI = T + 1;
  for (int q = tid; q < T * qrow; q += kPackThreads) {     // loads: contiguous along source axis 2
    const int r = q / qrow, c = (q % qrow) * 4;
    const size_t vs = s0 + (size_t)orient_tile_source(tl, d, r, c);
    const float4 m = load4(x0 + vs);
    float* row = xt + r * S;
    if (MODE == 1) {
      row[c] = m.x; row[c + 1] = m.y; row[c + 2] = m.z; row[c + 3] = m.w;
    } else {
      const T1* s = x1 + 3 * vs;
      const float4 a = load4(s), bb = load4(s + 4), cc = load4(s + 8);
      float4* r4 = reinterpret_cast<float4*>(row) + c;
      r4[0] = make_float4(m.x, a.x, a.y, a.z);
      r4[1] = make_float4(m.y, a.w, bb.x, bb.y);
      r4[2] = make_float4(m.z, bb.z, bb.w, cc.x);
      r4[3] = make_float4(m.w, cc.y, cc.z, cc.w);
    }
    if (ids) {
      const unsigned w = src_ids4(p, vs);
      unsigned* ir = idt + r * SI + c;
      ir[0] = w & 255u; ir[1] = (w >> 8) & 255u; ir[2] = (w >> 16) & 255u; ir[3] = w >> 24;
    }
  }
  __syncthreads();
  if (MODE == 4) {                                         // stores: one voxel a lane, contiguous along output axis 2
    for (int e = tid; e < TT; e += kPackThreads) {
      const int u = e / T, k = e % T;
      out4[s0 + (size_t)orient_tile_output(tl, d, u, k)] =
          reinterpret_cast<const float4*>(xt + orient_tile_row(tl, T, k) * S)[orient_tile_col(tl, T, u)];
    }
  }
  for (int q = tid; q < T * qrow; q += kPackThreads) {     // four voxels along output axis 2 a lane
    const int u = q / qrow, k = (q % qrow) * 4, col = orient_tile_col(tl, T, u);
    const size_t go = s0 + (size_t)orient_tile_output(tl, d, u, k);
    const int r0 = orient_tile_row(tl, T, k), r1 = orient_tile_row(tl, T, k + 1), r2 = orient_tile_row(tl, T, k + 2),
              r3 = orient_tile_row(tl, T, k + 3);
    if (MODE == 1) out4[go / 4] = make_float4(xt[r0 * S + col], xt[r1 * S + col], xt[r2 * S + col], xt[r3 * S + col]);
    if (ids) lab_out[go / 4] = idt[r0 * SI + col] | (idt[r1 * SI + col] << 8) | (idt[r2 * SI + col] << 16) | (idt[r3 * SI + col] << 24);
  }
}

// rot [batch][3] -> one orientation byte a sample; *any: some sample is rotated
int feed_orientations(const char* who, const int32_t* rot, int batch, unsigned char* out, bool* any) {
  *any = false;
  for (int b = 0; b < batch; ++b) {
    int r[3];
    for (int a = 0; a < 3; ++a) {
      r[a] = rot[b * 3 + a];
      ICS_CHECK(r[a] >= -1 && r[a] <= 2, std::string(who) + ": sample " + std::to_string(b) + ": rotation index " +
                                             std::to_string(r[a]) + " not in {-1,0,1,2}");
    }
    out[b] = orient_compose(r);
    *any = *any || out[b] != kOrientIdentity;
  }
  return 0;
}

static int launch_feed_pack_rot(hipStream_t st, const FeedPack& p) {
  const int d = p.d;
  ICS_CHECK(d >= 8 && d <= 256 && (d & (d - 1)) == 0, "feed pack: a rotated batch needs a grid edge that is a power of two in 8..256");
  const size_t V = (size_t)d * d * d;
  ICS_CHECK(p.nvox % V == 0, "feed pack: the voxel count is no whole number of samples");
  const int T = d < kRotTile ? d : kRotTile;
  const size_t ub = p.nvox / ((size_t)T * T);
  const size_t ob = p.label_kind == FEED_LABELS_ONEHOT ? p.nvox / kPackOneHotVox : 0;
  const size_t tb = (p.tail_n[0] + p.tail_n[1]) ? kPackTailBlocks : 0;
  ICS_CHECK(ub + ob + tb < ((size_t)1 << 31), "feed pack: batch too large for one launch");
  const dim3 grid((unsigned)(ub + ob + tb)), block(kPackThreads);
  const bool d0 = p.xdt[0] == kDtypeF64, d1 = p.xdt[1] == kDtypeF64;
  const unsigned uu = (unsigned)ub, uo = (unsigned)ob;
  if (p.nparts == 1 && p.xc[0] == 1) {
    if (d0) ICS_LAUNCH(feed_pack_rot_kernel<double, float, 1>, grid, block, 0, st, p, uu, uo);
    else ICS_LAUNCH(feed_pack_rot_kernel<float, float, 1>, grid, block, 0, st, p, uu, uo);
  } else if (p.nparts == 2 && p.xc[0] == 1 && p.xc[1] == 3) {
    if (d0 && d1) ICS_LAUNCH(feed_pack_rot_kernel<double, double, 4>, grid, block, 0, st, p, uu, uo);
    else if (d0) ICS_LAUNCH(feed_pack_rot_kernel<double, float, 4>, grid, block, 0, st, p, uu, uo);
    else if (d1) ICS_LAUNCH(feed_pack_rot_kernel<float, double, 4>, grid, block, 0, st, p, uu, uo);
    else ICS_LAUNCH(feed_pack_rot_kernel<float, float, 4>, grid, block, 0, st, p, uu, uo);
  } else {
    ICS_LAUNCH(feed_pack_rot_kernel<float, float, 0>, grid, block, 0, st, p, uu, uo);
  }
  ICS_HIP(hipGetLastError());
  return 0;
}

size_t feed_label_bytes(int label_kind, int ncls) {
  switch (label_kind) {
    case FEED_LABELS_U8: return 1;
    case FEED_LABELS_F64: return 8;
    case FEED_LABELS_F32: return 4;
    case FEED_LABELS_ONEHOT: return (size_t)ncls * 4;
    default: return 0;
  }
}
static size_t dtype_bytes(int dt) { return dt == kDtypeF64 ? 8 : 4; }

int feed_config_check(const char* who, const ics_feed_config* cfg, int in_channels, int ncls, bool want_labels) {
  const std::string w = std::string(who) + ": ";
  ICS_CHECK(cfg != nullptr, w + "null feed config");
  ICS_CHECK(cfg->x_parts == 1 || cfg->x_parts == 2, w + "x_parts must be 1 or 2");
  int sum = 0;
  for (int i = 0; i < cfg->x_parts; ++i) {
    ICS_CHECK(cfg->x_channels[i] >= 1 && cfg->x_channels[i] <= 16384, w + "every x part needs 1..16384 channels");
    ICS_CHECK(cfg->x_dtype[i] == kDtypeF32 || cfg->x_dtype[i] == kDtypeF64, w + "x_dtype must be 0 (float32) or 3 (float64)");
    sum += cfg->x_channels[i];
  }
  ICS_CHECK(sum == in_channels, w + "the x parts' channels do not add up to in_channels");
  ICS_CHECK(cfg->label_kind >= FEED_LABELS_NONE && cfg->label_kind <= FEED_LABELS_ONEHOT, w + "label_kind must be in 0..4");
  ICS_CHECK(want_labels || cfg->label_kind == FEED_LABELS_NONE, w + "a VAE engine takes no labels: label_kind must be 0");
  ICS_CHECK(!want_labels || cfg->label_kind != FEED_LABELS_NONE, w + "a U-Net engine needs labels: label_kind must be 1..4");
  ICS_CHECK(cfg->label_kind != FEED_LABELS_ONEHOT || (ncls >= 2 && ncls <= 127), w + "one-hot labels need 2..127 columns");
  return 0;
}

int launch_feed_pack(hipStream_t st, const FeedPack& p) {
  ICS_CHECK(p.nvox > 0 && p.nvox % 512 == 0, "feed pack: the voxel count must be a positive multiple of 512");
  ICS_CHECK(p.x_out && p.x[0] && (p.nparts == 1 || (p.nparts == 2 && p.x[1])), "feed pack: null x pointer");
  ICS_CHECK(p.label_kind == FEED_LABELS_NONE || (p.lab && p.lab_out), "feed pack: null label pointer");
  if (p.orient) return launch_feed_pack_rot(st, p);
  const size_t quads = p.nvox / 4 * (p.nparts == 1 ? (size_t)p.xc[0] : 1);
  const size_t qb = (quads + kPackThreads - 1) / kPackThreads;
  const size_t ob = p.label_kind == FEED_LABELS_ONEHOT ? p.nvox / kPackOneHotVox : 0;
  const size_t tb = (p.tail_n[0] + p.tail_n[1]) ? kPackTailBlocks : 0;
  ICS_CHECK(qb + ob + tb < ((size_t)1 << 31), "feed pack: batch too large for one launch");
  const dim3 grid((unsigned)(qb + ob + tb)), block(kPackThreads);
  const bool d0 = p.xdt[0] == kDtypeF64, d1 = p.xdt[1] == kDtypeF64;
  const unsigned uq = (unsigned)qb, uo = (unsigned)ob;
  if (p.nparts == 1) {
    if (d0) ICS_LAUNCH(feed_pack_kernel<double, float, 1>, grid, block, 0, st, p, uq, uo);
    else ICS_LAUNCH(feed_pack_kernel<float, float, 1>, grid, block, 0, st, p, uq, uo);
  } else if (p.nparts == 2 && p.xc[0] == 1 && p.xc[1] == 3) {
    if (d0 && d1) ICS_LAUNCH(feed_pack_kernel<double, double, 4>, grid, block, 0, st, p, uq, uo);
    else if (d0) ICS_LAUNCH(feed_pack_kernel<double, float, 4>, grid, block, 0, st, p, uq, uo);
    else if (d1) ICS_LAUNCH(feed_pack_kernel<float, double, 4>, grid, block, 0, st, p, uq, uo);
    else ICS_LAUNCH(feed_pack_kernel<float, float, 4>, grid, block, 0, st, p, uq, uo);
  } else {
    ICS_LAUNCH(feed_pack_kernel<float, float, 0>, grid, block, 0, st, p, uq, uo);
  }
  ICS_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------ class counts of labels
// Exact counts per class id over n labels (the inverse-frequency class weights of train_unet.py: DESIGN.md section 25).
// The labels are what the pack kernel converts -- uint8, float32 or float64 ids -- but nothing is converted blindly here:
// a value outside 0..ncls-1 or a non-integral one (compared in its own type) goes to bin kCountOor and indexes nothing.
//   * one lane = 16 bytes per pass (16 / 4 / 2 labels), grid-stride; the n % (labels per 16 bytes) last labels are
//     taken one per lane by block 0;
//   * every wave owns a row of LDS bins.  About 98 % of the voxels are background, so 64 atomics of a wave would queue
//     on one address: the lanes that agree with the wave's first active lane are counted by ONE add of their number
//     (a ballot), the others add their own 1;
//   * the four rows merge once per block, then one 64-bit atomic add per non-empty bin and block.  Integer sums: the
//     order does not matter.  A block sees at most 2^31 labels (launch_label_counts), so the 32-bit bins cannot wrap.
constexpr int kCountThreads = 256, kCountMaxBlocks = 2048;
typedef unsigned cv4 __attribute__((ext_vector_type(4)));
constexpr int kCountOor = 128, kCountBins = kCountOor + 1;     // ncls <= 127

__device__ __forceinline__ int count_bin(unsigned char v, int ncls) { return (int)v < ncls ? (int)v : kCountOor; }
__device__ __forceinline__ int count_bin(float v, int ncls) {
  return (v >= 0.f && v < (float)ncls && v == truncf(v)) ? (int)v : kCountOor;       // a NaN fails the first comparison
}
__device__ __forceinline__ int count_bin(double v, int ncls) {
  return (v >= 0.0 && v < (double)ncls && v == trunc(v)) ? (int)v : kCountOor;
}

template <typename T>
__global__ __launch_bounds__(kCountThreads) void label_counts_kernel(const T* __restrict__ lab, size_t n, int ncls,
                                                                     unsigned long long* __restrict__ counts) {
  constexpr int V = 16 / (int)sizeof(T);
  __shared__ unsigned bins[kCountThreads / 64][kCountBins];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < (kCountThreads / 64) * kCountBins; i += kCountThreads) (&bins[0][0])[i] = 0u;
  __syncthreads();
  unsigned* mine = bins[wave];
  auto add = [&](int bin) {                                    // called by any subset of a wave's lanes
    const unsigned long long active = __ballot(1);
    const int first = __builtin_amdgcn_readfirstlane(bin);    // the first active lane's bin
    const unsigned long long same = __ballot(bin == first);
    if (lane == __ffsll((long long)active) - 1) atomicAdd(&mine[first], (unsigned)__popcll(same));
    else if (bin != first) atomicAdd(&mine[bin], 1u);
  };
  const size_t nvec = n / V;
  for (size_t q = (size_t)blockIdx.x * kCountThreads + tid; q < nvec; q += (size_t)gridDim.x * kCountThreads) {
    union { cv4 u; T v[V]; } w;
    w.u = reinterpret_cast<const cv4*>(lab)[q];                // one 16-byte load
#pragma unroll
    for (int k = 0; k < V; ++k) add(count_bin(w.v[k], ncls));
  }
  if (blockIdx.x == 0 && (size_t)tid < n - nvec * V) add(count_bin(lab[nvec * V + tid], ncls));
  __syncthreads();
  if (tid < kCountBins) {
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < kCountThreads / 64; ++w) s += bins[w][tid];
    if (s) atomicAdd(&counts[tid], s);
  }
}

// counts: [kCountBins] device, zeroed here; [0..ncls-1] the classes, [kCountOor] everything that is no class id
static int launch_label_counts(hipStream_t st, const void* lab, int label_kind, size_t n, int ncls, unsigned long long* counts) {
  ICS_CHECK(ncls >= 2 && ncls <= 127, "label counts: num_classes must be in [2, 127]");
  ICS_CHECK(n <= ((size_t)1 << 40), "label counts: at most 2^40 labels per call");
  ICS_CHECK((reinterpret_cast<uintptr_t>(lab) & 15) == 0, "label counts: the labels must be 16-byte aligned");
  ICS_HIP(hipMemsetAsync(counts, 0, kCountBins * sizeof(unsigned long long), st));
  if (n == 0) return 0;
  const size_t per = label_kind == FEED_LABELS_U8 ? 16 : (label_kind == FEED_LABELS_F32 ? 4 : 2);
  const size_t nvec = n / per;
  size_t nblk = (nvec + kCountThreads - 1) / kCountThreads;
  nblk = nblk < 1 ? 1 : (nblk > (size_t)kCountMaxBlocks ? (size_t)kCountMaxBlocks : nblk);      // 2^40 / 2048 = 2^29 labels a block
  const dim3 grid((unsigned)nblk), block(kCountThreads);
  if (label_kind == FEED_LABELS_U8)
    ICS_LAUNCH(label_counts_kernel<unsigned char>, grid, block, 0, st, static_cast<const unsigned char*>(lab), n, ncls, counts);
  else if (label_kind == FEED_LABELS_F32)
    ICS_LAUNCH(label_counts_kernel<float>, grid, block, 0, st, static_cast<const float*>(lab), n, ncls, counts);
  else
    ICS_LAUNCH(label_counts_kernel<double>, grid, block, 0, st, static_cast<const double*>(lab), n, ncls, counts);
  ICS_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------ the feed of an engine
struct FeedSlot {
  unsigned char* host = nullptr;   // pinned
  unsigned char* dev = nullptr;    // the engine's
  hipEvent_t uploaded = nullptr, consumed = nullptr;
  bool obtained = false;           // the host holds the views (ics_net_feed_slot since the last submit)
  bool pending = false;            // submitted and not consumed by a step yet
  bool ever = false;               // submitted at least once
  bool rotated = false;            // the last submit carried a table with a rotated sample: the step packs through it
  int batch = 0;
};
struct Feed {
  ics_feed_config cfg{};
  int max_batch = 0, d = 0, C = 0, ncls = 0, ncond = 0, latent = 0, kind = 0;
  size_t off_x[2] = {0, 0}, off_lab = 0, off_cond = 0, off_eps = 0, off_orient = 0, slot_bytes = 0;   // the layout of every slot
  size_t vox_x[2] = {0, 0}, vox_lab = 0;                                                // bytes per voxel
  hipStream_t feed_st = nullptr;
  FeedSlot slot[kFeedMaxSlots];
  float* ring = nullptr;           // pinned [kFeedRing][kFeedMetricFloats]
  hipEvent_t ring_ev[kFeedRing] = {};
  long long next_ticket = 0;
  ~Feed() {
    if (feed_st) { (void)hipStreamSynchronize(feed_st); (void)hipStreamDestroy(feed_st); }
    for (FeedSlot& s : slot) {
      if (s.uploaded) (void)hipEventDestroy(s.uploaded);
      if (s.consumed) (void)hipEventDestroy(s.consumed);
      if (s.host) (void)hipHostFree(s.host);
    }
    for (hipEvent_t e : ring_ev) if (e) (void)hipEventDestroy(e);
    if (ring) (void)hipHostFree(ring);
  }
};

static int feed_get(ics_net* net, const char* who, FeedPort* port, Feed** f) {
  ICS_CHECK(net != nullptr, std::string(who) + ": null handle");
  ICS_TRY(feed_port(net, port));
  ICS_CHECK(*port->feed != nullptr, std::string(who) + ": the engine has no open feed (ics_net_feed_open)");
  *f = *port->feed;
  return 0;
}
static int slot_check(const char* who, const Feed& f, int slot) {
  ICS_CHECK(slot >= 0 && slot < f.cfg.slots,
            std::string(who) + ": bad slot index " + std::to_string(slot) + " (the feed has " + std::to_string(f.cfg.slots) + " slots)");
  return 0;
}

static int feed_open(ics_net* net, const ics_feed_config* cfg) {
  ICS_CHECK(net != nullptr, "ics_net_feed_open: null handle");
  FeedPort P;
  ICS_TRY(feed_port(net, &P));
  ICS_CHECK(*P.feed == nullptr, "ics_net_feed_open: a feed is already open on this engine (ics_net_feed_close first)");
  ICS_TRY(feed_config_check("ics_net_feed_open", cfg, P.C, P.ncls, P.kind == 0));
  ICS_CHECK(cfg->slots >= 2 && cfg->slots <= kFeedMaxSlots, "ics_net_feed_open: slots must be in 2..4");
  auto f = std::make_unique<Feed>();
  f->cfg = *cfg;
  f->max_batch = P.max_batch; f->d = P.d; f->C = P.C; f->ncls = P.ncls; f->kind = P.kind;
  f->ncond = P.kind == 1 ? P.ncond : 0;
  f->latent = P.kind == 1 ? P.latent : 0;
  const size_t vox = (size_t)P.max_batch * P.d * P.d * P.d;
  Layout L;                       // every part at a 256-byte aligned offset
  for (int i = 0; i < cfg->x_parts; ++i) {
    f->vox_x[i] = (size_t)cfg->x_channels[i] * dtype_bytes(cfg->x_dtype[i]);
    f->off_x[i] = L.add<unsigned char>(vox * f->vox_x[i]).off;
  }
  f->vox_lab = feed_label_bytes(cfg->label_kind, P.ncls);
  f->off_lab = L.add<unsigned char>(vox * f->vox_lab).off;
  f->off_cond = L.add<float>((size_t)P.max_batch * f->ncond).off;
  f->off_eps = L.add<float>((size_t)P.max_batch * f->latent).off;
  f->off_orient = L.add<unsigned char>((size_t)P.max_batch).off;     // one orientation byte a sample (orient.h), last
  f->slot_bytes = L.bytes();
  ICS_HIP(hipStreamCreateWithFlags(&f->feed_st, hipStreamNonBlocking));
  for (int s = 0; s < cfg->slots; ++s) {
    FeedSlot& S = f->slot[s];
    ICS_HIP(hipHostMalloc(reinterpret_cast<void**>(&S.host), f->slot_bytes, hipHostMallocDefault));
    ICS_TRY(feed_port_stage(net, s, f->slot_bytes, &S.dev));
    ICS_HIP(hipEventCreateWithFlags(&S.uploaded, hipEventDisableTiming));
    ICS_HIP(hipEventCreateWithFlags(&S.consumed, hipEventDisableTiming));
  }
  ICS_HIP(hipHostMalloc(reinterpret_cast<void**>(&f->ring), sizeof(float) * kFeedRing * kFeedMetricFloats, hipHostMallocDefault));
  std::memset(f->ring, 0, sizeof(float) * kFeedRing * kFeedMetricFloats);
  for (hipEvent_t& e : f->ring_ev) ICS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  ICS_HIP(hipStreamSynchronize(P.st));     // the staging buffers' zero fill (the engine's allocator enqueues it)
  *P.feed = f.release();
  return 0;
}

static int feed_close(ics_net* net) {
  FeedPort P;
  Feed* f;
  ICS_TRY(feed_get(net, "ics_net_feed_close", &P, &f));
  const hipError_t e0 = hipStreamSynchronize(f->feed_st), e1 = hipStreamSynchronize(P.st);
  *P.feed = nullptr;
  delete f;
  ICS_HIP(e0);
  ICS_HIP(e1);
  return feed_port_resolve(net);
}

void feed_release(ics_net* net) {
  FeedPort P;
  if (net == nullptr || feed_port(net, &P) != 0 || *P.feed == nullptr) return;
  (void)feed_close(net);
}

static int feed_step(ics_net* net, const char* who, int kind, int training, int slot, int* ticket) {
  FeedPort P;
  Feed* f;
  ICS_TRY(feed_get(net, who, &P, &f));
  ICS_CHECK(P.kind == kind, std::string(who) + (kind == 0 ? ": wrong engine kind: a U-Net engine is required"
                                                          : ": wrong engine kind: a VAE engine is required"));
  ICS_CHECK(ticket != nullptr, std::string(who) + ": null ticket");
  ICS_TRY(slot_check(who, *f, slot));
  FeedSlot& S = f->slot[slot];
  ICS_CHECK(S.ever, std::string(who) + ": slot " + std::to_string(slot) + " was never submitted");
  ICS_CHECK(S.pending, std::string(who) + ": slot " + std::to_string(slot) + " was already consumed by a step: submit it again first");
  const int B = S.batch;
  ICS_HIP(hipStreamWaitEvent(P.st, S.uploaded, 0));
  FeedPack k;
  k.nparts = f->cfg.x_parts;
  for (int i = 0; i < k.nparts; ++i) {
    k.x[i] = S.dev + f->off_x[i];
    k.xc[i] = f->cfg.x_channels[i];
    k.xdt[i] = f->cfg.x_dtype[i];
  }
  k.label_kind = f->cfg.label_kind;
  k.ncls = f->ncls;
  if (k.label_kind != FEED_LABELS_NONE) { k.lab = S.dev + f->off_lab; k.lab_out = P.labels; }
  k.nvox = (size_t)B * f->d * f->d * f->d;
  k.d = f->d;
  if (S.rotated) k.orient = S.dev + f->off_orient;
  k.x_out = P.x_in;
  if (kind == 1) {
    k.tail_src[0] = reinterpret_cast<const float*>(S.dev + f->off_cond); k.tail_dst[0] = P.cond_in; k.tail_n[0] = (size_t)B * f->ncond;
    k.tail_src[1] = reinterpret_cast<const float*>(S.dev + f->off_eps);  k.tail_dst[1] = P.eps_in;  k.tail_n[1] = (size_t)B * f->latent;
  }
  ICS_TRY(launch_feed_pack(P.st, k));
  ICS_HIP(hipEventRecord(S.consumed, P.st));
  S.pending = false;
  ICS_TRY(feed_port_step(net, B, training));
  ICS_CHECK(f->next_ticket < INT_MAX, std::string(who) + ": out of tickets: close the feed and open it again");
  const int entry = (int)(f->next_ticket % kFeedRing);
  ICS_HIP(hipMemcpyAsync(f->ring + (size_t)entry * kFeedMetricFloats, P.d_metrics, (kind == 0 ? 5 : 4) * sizeof(float),
                         hipMemcpyDeviceToHost, P.st));
  ICS_HIP(hipEventRecord(f->ring_ev[entry], P.st));
  *ticket = (int)f->next_ticket;
  f->next_ticket += 1;
  return 0;
}

}  // namespace ics

// ==========================================================================================
// C ABI
// ==========================================================================================
using namespace ics;

extern "C" {

int ics_net_feed_open(ics_net* net, const ics_feed_config* cfg) { return feed_open(net, cfg); }
int ics_net_feed_close(ics_net* net) { return feed_close(net); }

int ics_net_feed_slot(ics_net* net, int slot, void** x0, void** x1, void** labels, float** cond, float** eps) {
  FeedPort P;
  Feed* f;
  ICS_TRY(feed_get(net, "ics_net_feed_slot", &P, &f));
  ICS_TRY(slot_check("ics_net_feed_slot", *f, slot));
  FeedSlot& S = f->slot[slot];
  if (S.ever) ICS_HIP(hipEventSynchronize(S.uploaded));     // the one wait: the slot's last upload has left the pinned buffer
  S.obtained = true;
  if (x0) *x0 = S.host + f->off_x[0];
  if (x1) *x1 = f->cfg.x_parts == 2 ? S.host + f->off_x[1] : nullptr;
  if (labels) *labels = f->vox_lab ? S.host + f->off_lab : nullptr;
  if (cond) *cond = f->ncond ? reinterpret_cast<float*>(S.host + f->off_cond) : nullptr;
  if (eps) *eps = f->latent ? reinterpret_cast<float*>(S.host + f->off_eps) : nullptr;
  return 0;
}

static int feed_submit(const char* who_, ics_net* net, int slot, int batch, const int32_t* rot) {
  const std::string who = who_;
  FeedPort P;
  Feed* f;
  ICS_TRY(feed_get(net, who_, &P, &f));
  ICS_TRY(slot_check(who_, *f, slot));
  FeedSlot& S = f->slot[slot];
  ICS_CHECK(batch >= 1 && batch <= f->max_batch, who + ": batch exceeds max_batch (or is below 1)");
  ICS_CHECK(!S.pending, who + ": slot " + std::to_string(slot) + " holds a submitted batch that no step has consumed");
  ICS_CHECK(S.obtained, who + ": slot " + std::to_string(slot) + " was never obtained: call ics_net_feed_slot and fill it first");
  bool rotated = false;            // the table is composed into the slot's pinned memory, which the host holds (obtained)
  if (rot) ICS_TRY(feed_orientations(who_, rot, batch, S.host + f->off_orient, &rotated));
  const size_t vox = (size_t)batch * f->d * f->d * f->d;
  ICS_HIP(hipStreamWaitEvent(f->feed_st, S.consumed, 0));   // (never recorded yet: no wait)
  auto up = [&](size_t off, size_t bytes) -> hipError_t {
    return bytes ? hipMemcpyAsync(S.dev + off, S.host + off, bytes, hipMemcpyHostToDevice, f->feed_st) : hipSuccess;
  };
  for (int i = 0; i < f->cfg.x_parts; ++i) ICS_HIP(up(f->off_x[i], vox * f->vox_x[i]));
  ICS_HIP(up(f->off_lab, vox * f->vox_lab));
  ICS_HIP(up(f->off_cond, (size_t)batch * f->ncond * sizeof(float)));
  ICS_HIP(up(f->off_eps, (size_t)batch * f->latent * sizeof(float)));
  if (rotated) ICS_HIP(up(f->off_orient, (size_t)batch));
  ICS_HIP(hipEventRecord(S.uploaded, f->feed_st));
  S.obtained = false; S.pending = true; S.ever = true; S.batch = batch; S.rotated = rotated;
  return 0;
}

int ics_net_feed_submit(ics_net* net, int slot, int batch) { return feed_submit("ics_net_feed_submit", net, slot, batch, nullptr); }
int ics_net_feed_submit_rot(ics_net* net, int slot, int batch, const int32_t* rot) {
  return feed_submit("ics_net_feed_submit_rot", net, slot, batch, rot);
}

int ics_unet_train_step_fed(ics_net* net, int slot, int* ticket) { return feed_step(net, "ics_unet_train_step_fed", 0, 1, slot, ticket); }
int ics_unet_test_step_fed(ics_net* net, int slot, int* ticket) { return feed_step(net, "ics_unet_test_step_fed", 0, 0, slot, ticket); }
int ics_vae_train_step_fed(ics_net* net, int slot, int* ticket) { return feed_step(net, "ics_vae_train_step_fed", 1, 1, slot, ticket); }
int ics_vae_test_step_fed(ics_net* net, int slot, int* ticket) { return feed_step(net, "ics_vae_test_step_fed", 1, 0, slot, ticket); }

int ics_net_feed_metrics(ics_net* net, int ticket, float* metrics) {
  FeedPort P;
  Feed* f;
  ICS_TRY(feed_get(net, "ics_net_feed_metrics", &P, &f));
  ICS_CHECK(metrics != nullptr, "ics_net_feed_metrics: null argument");
  ICS_CHECK(ticket >= 0 && ticket < f->next_ticket, "ics_net_feed_metrics: no step has returned ticket " + std::to_string(ticket));
  ICS_CHECK(f->next_ticket - ticket <= kFeedRing,
            "ics_net_feed_metrics: ticket " + std::to_string(ticket) + " is older than the ring of " + std::to_string(kFeedRing) + " entries");
  const int entry = ticket % kFeedRing;
  ICS_HIP(hipEventSynchronize(f->ring_ev[entry]));
  std::memcpy(metrics, f->ring + (size_t)entry * kFeedMetricFloats, (f->kind == 0 ? 5 : 4) * sizeof(float));
  return feed_port_resolve(net);
}

static int op_feed_pack(const char* who_, const ics_feed_config* cfg, const void* x0, const void* x1, const void* labels,
                        const int32_t* rot, int batch, int d, int num_classes, float* x, uint8_t* out_labels) {
  const std::string who = who_;
  ICS_CHECK(cfg != nullptr, who + ": null feed config");
  ICS_CHECK(batch >= 1 && batch <= 65535, who + ": batch must be in 1..65535");
  ICS_CHECK(d >= 8 && d <= 256 && (d & (d - 1)) == 0, who + ": d must be a power of two in 8..256");
  const int C = cfg->x_parts >= 1 && cfg->x_parts <= 2 ? cfg->x_channels[0] + (cfg->x_parts == 2 ? cfg->x_channels[1] : 0) : 0;
  ICS_TRY(feed_config_check(who_, cfg, C, num_classes, cfg->label_kind != FEED_LABELS_NONE));
  ICS_CHECK(x0 && x && (cfg->x_parts == 1 || x1), who + ": null x pointer");
  ICS_CHECK(cfg->label_kind == FEED_LABELS_NONE || (labels && out_labels), who + ": null label pointer");
  std::vector<unsigned char> orient;
  bool rotated = false;
  if (rot) {
    orient.resize((size_t)batch);
    ICS_TRY(feed_orientations(who_, rot, batch, orient.data(), &rotated));
  }
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  const size_t vox = (size_t)batch * d * d * d;
  const size_t lab_bytes = vox * feed_label_bytes(cfg->label_kind, num_classes);
  Layout L;
  const auto s_x0 = L.add<unsigned char>(vox * cfg->x_channels[0] * dtype_bytes(cfg->x_dtype[0]));
  const auto s_x1 = L.add<unsigned char>(cfg->x_parts == 2 ? vox * cfg->x_channels[1] * dtype_bytes(cfg->x_dtype[1]) : 0);
  const auto s_lab = L.add<unsigned char>(lab_bytes);
  const auto s_out = L.add<float>(vox * C);
  const auto s_lout = L.add<unsigned char>(lab_bytes ? vox : 0);
  const auto s_or = L.add<unsigned char>(rotated ? (size_t)batch : 0);
  unsigned char *d_x0, *d_x1, *d_lab, *d_lout, *d_or;
  float* d_out;
  ICS_TRY(L.reserve(s_x0, &d_x0, s_x1, &d_x1, s_lab, &d_lab, s_out, &d_out, s_lout, &d_lout, s_or, &d_or));
  ICS_TRY(L.upload(s_or, orient.data(), s_or.count, st));
  ICS_TRY(L.upload(s_x0, x0, s_x0.count, st));
  ICS_TRY(L.upload(s_x1, x1, s_x1.count, st));
  ICS_TRY(L.upload(s_lab, labels, s_lab.count, st));
  FeedPack k;
  k.nparts = cfg->x_parts;
  k.x[0] = d_x0; k.x[1] = d_x1;
  for (int i = 0; i < k.nparts; ++i) { k.xc[i] = cfg->x_channels[i]; k.xdt[i] = cfg->x_dtype[i]; }
  k.lab = d_lab; k.label_kind = cfg->label_kind; k.ncls = num_classes;
  k.nvox = vox; k.x_out = d_out; k.lab_out = d_lout;
  k.d = d; k.orient = d_or;         // null unless a sample is rotated: feed_pack_kernel then
  ICS_TRY(launch_feed_pack(st, k));
  ICS_TRY(L.download(x, s_out, s_out.count, st));
  ICS_TRY(L.download(out_labels, s_lout, s_lout.count, st));
  ICS_HIP(hipStreamSynchronize(st));
  return 0;
}

int ics_op_feed_pack(const ics_feed_config* cfg, const void* x0, const void* x1, const void* labels, int batch, int d,
                     int num_classes, float* x, uint8_t* out_labels) {
  return op_feed_pack("ics_op_feed_pack", cfg, x0, x1, labels, nullptr, batch, d, num_classes, x, out_labels);
}
int ics_op_feed_pack_rot(const ics_feed_config* cfg, const void* x0, const void* x1, const void* labels, const int32_t* rot,
                         int batch, int d, int num_classes, float* x, uint8_t* out_labels) {
  return op_feed_pack("ics_op_feed_pack_rot", cfg, x0, x1, labels, rot, batch, d, num_classes, x, out_labels);
}

int ics_op_label_counts(const void* labels, int label_kind, size_t n, int ncls, int64_t* counts, int64_t* out_of_range) {
  ICS_CHECK(label_kind != FEED_LABELS_ONEHOT, "ics_op_label_counts: one-hot labels are not class ids: count their argmax instead");
  ICS_CHECK(label_kind == FEED_LABELS_U8 || label_kind == FEED_LABELS_F64 || label_kind == FEED_LABELS_F32,
            "ics_op_label_counts: label_kind must be 1 (uint8), 2 (float64) or 3 (float32)");
  ICS_CHECK(ncls >= 2 && ncls <= 127, "ics_op_label_counts: num_classes must be in [2, 127]");
  ICS_CHECK(counts && out_of_range && (labels || n == 0), "ics_op_label_counts: null argument");
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  Layout L;
  const auto s_lab = L.add<unsigned char>(n * feed_label_bytes(label_kind, ncls));
  const auto s_cnt = L.add<unsigned long long>(kCountBins);
  unsigned char* d_lab;
  unsigned long long* d_cnt;
  ICS_TRY(L.reserve(s_lab, &d_lab, s_cnt, &d_cnt));
  ICS_TRY(L.upload(s_lab, labels, s_lab.count, st));
  ICS_TRY(launch_label_counts(st, d_lab, label_kind, n, ncls, d_cnt));
  unsigned long long host[kCountBins];
  ICS_TRY(L.download(host, s_cnt, s_cnt.count, st));
  ICS_HIP(hipStreamSynchronize(st));
  for (int c = 0; c < ncls; ++c) counts[c] = (int64_t)host[c];
  *out_of_range = (int64_t)host[kCountOor];
  return 0;
}

}  // extern "C"
