/* Host driver of the `make asan` build: walks the C ABI of include/icsg3d.h end to end on the stubbed runtime
 * (hoststub/hip_host_stub.cpp) so that AddressSanitizer / UBSan / LeakSanitizer see every host-side code path:
 * engine construction (tensor tables, BN slab, workspace planners), named tensor I/O, train / test / predict
 * call chains (launch planning, split-K and bucket bookkeeping, profiler rows), the data-parallel entry points,
 * the fused inference tail, optimizer-state export and destruction.  Kernels do not run; results are not checked. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "icsg3d.h"

#define OK(x)                                                              \
  do {                                                                     \
    if ((x) != 0) {                                                        \
      fprintf(stderr, "FAILED %s: %s\n", #x, ics_last_error());            \
      return 1;                                                            \
    }                                                                      \
  } while (0)

static int tensor_io(ics_net* net) {
  int n = 0;
  OK(ics_net_num_tensors(net, &n));
  for (int i = 0; i < n; ++i) {
    const char* name; int nd, tr; int64_t dims[5];
    OK(ics_net_tensor_info(net, i, &name, &nd, dims, &tr));
    size_t cnt = 1;
    for (int k = 0; k < nd; ++k) cnt *= (size_t)dims[k];
    float* buf = (float*)malloc(cnt * sizeof(float));      /* exact size: an over-read/-write is an ASan report */
    for (size_t k = 0; k < cnt; ++k) buf[k] = 0.01f * (float)(k % 7);
    OK(ics_net_set_tensor(net, name, buf, cnt));
    OK(ics_net_get_tensor(net, name, buf, cnt));
    if (tr) OK(ics_net_get_grad(net, name, buf, cnt));
    if (ics_net_set_tensor(net, name, buf, cnt + 1) == 0) { fprintf(stderr, "size check missing for %s\n", name); return 1; }
    free(buf);
  }
  return 0;
}

/* Voxelisation: the host-pointer op (valid and invalid arguments, internal chunking) and both engine feeds; padding rows
 * beyond nsites are left out of the allocation's reach by a max_sites stride that is larger than any nsites. */
static int voxelise_walk(ics_net* unet, ics_net* vae, int d, int B, const float* cond, const float* eps) {
  enum { NS = 3, MS = 5 };
  int32_t nsites[NS] = {1, 5, 3};
  double xyz[NS * MS * 3], z[NS * MS], sigma[NS * MS], abc[NS * 3];
  for (int i = 0; i < NS * MS; ++i) {
    xyz[3 * i] = 0.1 * i; xyz[3 * i + 1] = 0.2 * (i % 4); xyz[3 * i + 2] = 0.05 * i;
    z[i] = 1 + i % 90; sigma[i] = 0.5 + 0.1 * (i % 3);
  }
  for (int i = 0; i < NS * 3; ++i) abc[i] = 3.0 + i;
  ics_structures s = {NS, MS, nsites, xyz, z, sigma, abc};
  const int nj = 7;
  int32_t jobs[7 * 4] = {0, -1, -1, -1, 1, 0, 1, 2, 2, 2, 2, 2, 1, 1, -1, 0, 0, -1, -1, -1, 2, 0, 0, 0, 1, 2, 1, 0};
  const int dv = 6;
  const size_t V = (size_t)dv * dv * dv;
  double* M = (double*)malloc(nj * V * 8);
  double* S = (double*)malloc(nj * V * 8);
  double* p = (double*)malloc(nj * V * 24);
  OK(ics_op_voxelise(&s, jobs, nj, dv, 0.25, 1.0, M, S, p));
  OK(ics_op_voxelise(&s, jobs, nj, dv, 0.1, 0.6, NULL, S, NULL));
  OK(ics_op_voxelise(&s, jobs, nj, dv, 0.1, 0.6, NULL, NULL, NULL));
  {   /* more jobs than one chunk holds */
    const int big = 2100;
    int32_t* bj = (int32_t*)malloc((size_t)big * 16);
    for (int j = 0; j < big; ++j) { bj[4 * j] = j % NS; bj[4 * j + 1] = j % 4 - 1; bj[4 * j + 2] = -1; bj[4 * j + 3] = (j / 4) % 3; }
    double* bM = (double*)malloc((size_t)big * 8 * 8 * 8 * 8);
    OK(ics_op_voxelise(&s, bj, big, 8, 0.25, 1.0, bM, NULL, NULL));
    free(bj); free(bM);
  }
  /* every invalid argument is refused with a message, and nothing is written */
  int bad = 0;
  ics_structures t = s;
  bad += ics_op_voxelise(NULL, jobs, nj, dv, 0.25, 1.0, M, S, p) == 0;
  bad += ics_op_voxelise(&s, NULL, nj, dv, 0.25, 1.0, M, S, p) == 0;
  bad += ics_op_voxelise(&s, jobs, 0, dv, 0.25, 1.0, M, S, p) == 0;
  bad += ics_op_voxelise(&s, jobs, nj, 1, 0.25, 1.0, M, S, p) == 0;
  bad += ics_op_voxelise(&s, jobs, nj, 300, 0.25, 1.0, M, S, p) == 0;
  bad += ics_op_voxelise(&s, jobs, nj, dv, -0.1, 1.0, M, S, p) == 0;
  bad += ics_op_voxelise(&s, jobs, nj, dv, 0.25, NAN, M, S, p) == 0;
  t.xyz = NULL; bad += ics_op_voxelise(&t, jobs, nj, dv, 0.25, 1.0, M, S, p) == 0; t = s;
  t.count = 0; bad += ics_op_voxelise(&t, jobs, nj, dv, 0.25, 1.0, M, S, p) == 0; t = s;
  t.max_sites = 4; bad += ics_op_voxelise(&t, jobs, nj, dv, 0.25, 1.0, M, S, p) == 0; t = s;   /* nsites 5 > stride */
  jobs[4] = 3; bad += ics_op_voxelise(&s, jobs, nj, dv, 0.25, 1.0, M, S, p) == 0; jobs[4] = 1;
  jobs[5] = 3; bad += ics_op_voxelise(&s, jobs, nj, dv, 0.25, 1.0, M, S, p) == 0; jobs[5] = 0;
  jobs[6] = -2; bad += ics_op_voxelise(&s, jobs, nj, dv, 0.25, 1.0, M, S, p) == 0; jobs[6] = 1;
  nsites[1] = 0; bad += ics_op_voxelise(&s, jobs, nj, dv, 0.25, 1.0, M, S, p) == 0; nsites[1] = 5;
  nsites[1] = 300; bad += ics_op_voxelise(&s, jobs, nj, dv, 0.25, 1.0, M, S, p) == 0; nsites[1] = 5;
  sigma[MS + 2] = 0.0; bad += ics_op_voxelise(&s, jobs, nj, dv, 0.25, 1.0, M, S, p) == 0; sigma[MS + 2] = 0.5;
  sigma[MS + 2] = INFINITY; bad += ics_op_voxelise(&s, jobs, nj, dv, 0.25, 1.0, M, S, p) == 0; sigma[MS + 2] = 0.5;
  abc[4] = -1.0; bad += ics_op_voxelise(&s, jobs, nj, dv, 0.25, 1.0, M, S, p) == 0; abc[4] = 4.0;
  xyz[3 * MS + 1] = NAN; bad += ics_op_voxelise(&s, jobs, nj, dv, 0.25, 1.0, M, S, p) == 0; xyz[3 * MS + 1] = 0.2;
  z[MS] = -1.0; bad += ics_op_voxelise(&s, jobs, nj, dv, 0.25, 1.0, M, S, p) == 0; z[MS] = 1.0;
  if (bad) { fprintf(stderr, "voxelise: %d invalid argument sets accepted\n", bad); return 1; }
  if (!ics_last_error()[0]) { fprintf(stderr, "voxelise: no error message\n"); return 1; }
  OK(ics_op_voxelise(&s, jobs, nj, dv, 0.25, 1.0, M, S, p));     /* still usable */
  free(M); free(S); free(p);
  /* engine feeds: a batch of B jobs at the engines' grid */
  int32_t* ej = (int32_t*)malloc((size_t)B * 16);
  for (int b = 0; b < B; ++b) { ej[4 * b] = b % NS; ej[4 * b + 1] = b % 3; ej[4 * b + 2] = -1; ej[4 * b + 3] = 1; }
  OK(ics_unet_voxelise_batch(unet, &s, ej, B, 0.25, 1.0));
  OK(ics_unet_train_step_resident(unet, NULL));
  OK(ics_unet_predict_resident(unet, 1, 0.8f));
  OK(ics_vae_voxelise_batch(vae, &s, ej, B, 0.25, 1.0, cond, eps));
  OK(ics_vae_train_step_resident(vae, NULL));
  OK(ics_unet_voxelise_batch(unet, &s, ej, 1, 0.1, 0.6));
  bad = 0;
  bad += ics_unet_voxelise_batch(unet, &s, ej, B + 1, 0.25, 1.0) == 0;
  bad += ics_unet_voxelise_batch(vae, &s, ej, B, 0.25, 1.0) == 0;
  bad += ics_vae_voxelise_batch(unet, &s, ej, B, 0.25, 1.0, cond, eps) == 0;
  bad += ics_vae_voxelise_batch(vae, &s, ej, B, 0.25, 1.0, NULL, eps) == 0;
  bad += ics_unet_voxelise_batch(NULL, &s, ej, B, 0.25, 1.0) == 0;
  z[MS] = 95.0; bad += ics_unet_voxelise_batch(unet, &s, ej, B, 0.25, 1.0) == 0; z[MS] = 1.0;
  z[MS] = 2.5; bad += ics_unet_voxelise_batch(unet, &s, ej, B, 0.25, 1.0) == 0; z[MS] = 1.0;
  z[MS] = 95.0; OK(ics_vae_voxelise_batch(vae, &s, ej, B, 0.25, 1.0, cond, eps)); z[MS] = 1.0;   /* no class-id rule */
  if (bad) { fprintf(stderr, "voxelise feed: %d invalid argument sets accepted\n", bad); return 1; }
  free(ej);
  (void)d;
  return 0;
}

/* Batched matching: valid batches (both orientations, empty sets, the 2048-point limit, more points than one chunk
 * holds) and every refused argument, after which the op still works. */
static int match_walk(void) {
  enum { NB = 4 };
  int32_t ao[NB + 1] = {0, 3, 3, 10, 12}, bo[NB + 1] = {0, 5, 7, 9, 9};
  double a[12 * 3], b[9 * 3], emd[NB];
  int32_t match[12];
  for (int i = 0; i < 36; ++i) a[i] = 0.37 * i - 2.0;
  for (int i = 0; i < 27; ++i) b[i] = 1.0 - 0.21 * i;
  OK(ics_op_match_emd(a, ao, b, bo, NB, emd, match));
  OK(ics_op_match_emd(a, ao, b, bo, NB, emd, NULL));
  OK(ics_op_match_emd(b, bo, a, ao, NB, emd, match));
  {   /* 1030 samples of 2048 x 2048 points: more than one chunk's point budget */
    const int ns = 1030, np = 2048;
    double* big = (double*)calloc((size_t)ns * np * 3, sizeof(double));
    int32_t* off = (int32_t*)malloc((ns + 1) * sizeof(int32_t));
    double* e = (double*)malloc(ns * sizeof(double));
    int32_t* m = (int32_t*)malloc((size_t)ns * np * sizeof(int32_t));
    for (int k = 0; k <= ns; ++k) off[k] = k * np;
    OK(ics_op_match_emd(big, off, big, off, ns, e, m));
    off[1] = np + 1;   /* a set above the limit */
    if (ics_op_match_emd(big, off, big, off, 1, e, m) == 0) { fprintf(stderr, "match: 2049 points accepted\n"); return 1; }
    free(big); free(off); free(e); free(m);
  }
  int bad = 0;
  bad += ics_op_match_emd(a, ao, b, bo, 0, emd, match) == 0;
  bad += ics_op_match_emd(a, NULL, b, bo, NB, emd, match) == 0;
  bad += ics_op_match_emd(a, ao, b, bo, NB, NULL, match) == 0;
  bad += ics_op_match_emd(NULL, ao, b, bo, NB, emd, match) == 0;
  ao[0] = 1; bad += ics_op_match_emd(a, ao, b, bo, NB, emd, match) == 0; ao[0] = 0;
  ao[2] = 2; bad += ics_op_match_emd(a, ao, b, bo, NB, emd, match) == 0; ao[2] = 3;
  a[7] = NAN; bad += ics_op_match_emd(a, ao, b, bo, NB, emd, match) == 0; a[7] = 0.5;
  b[20] = INFINITY; bad += ics_op_match_emd(a, ao, b, bo, NB, emd, match) == 0; b[20] = 0.5;
  b[20] = 1e200; bad += ics_op_match_emd(a, ao, b, bo, NB, emd, match) == 0; b[20] = 0.5;
  if (bad) { fprintf(stderr, "match: %d invalid argument sets accepted\n", bad); return 1; }
  if (!ics_last_error()[0]) { fprintf(stderr, "match: no error message\n"); return 1; }
  OK(ics_op_match_emd(a, ao, b, bo, NB, emd, match));     /* still usable */
  return 0;
}

/* Batched structure screening: a ragged batch with empty, one-wave and whole-workgroup structures, more atoms than one
 * chunk holds, and every refused argument, after which the op still works. */
static int structure_walk(void) {
  enum { NB = 5, NA = 2 + 0 + 1 + 70 + 40 };
  int32_t off[NB + 1] = {0, 2, 2, 3, 73, 113}, sp[NA];
  double xyz[NA * 3], abc[NB * 3], ang[NB * 3];
  for (int i = 0; i < NA; ++i) { sp[i] = i % 97; xyz[3 * i] = 0.31 * i; xyz[3 * i + 1] = 7.0 - 0.17 * i; xyz[3 * i + 2] = 0.05 * i; }
  for (int i = 0; i < NB; ++i) {
    abc[3 * i] = 4.0 + i; abc[3 * i + 1] = 5.0; abc[3 * i + 2] = 6.5;
    ang[3 * i] = 90.0; ang[3 * i + 1] = i % 2 ? 100.0 : 90.0; ang[3 * i + 2] = i % 2 ? 120.0 : 90.0;
  }
  double lat[NB * 9], vol[NB], frac[NA * 3], dmin[NB], nearest[NA];
  int32_t pair[NB * 2], nclose[NB], valid[NB], reason[NB], hist[NB * 95];
#define SCREEN(o, s, x, l, g, n, t) ics_op_structure_screen(o, s, x, l, g, n, t, lat, vol, frac, dmin, pair, nclose, valid, reason, nearest, hist)
  OK(SCREEN(off, sp, xyz, abc, ang, NB, 0.5));
  OK(SCREEN(off, sp, xyz, abc, ang, 2, 0.0));
  {   /* 600 structures of 2048 atoms: more than one chunk's atom budget */
    const int ns = 600, np = 2048;
    double* bx = (double*)calloc((size_t)ns * np * 3, sizeof(double));
    int32_t* bs = (int32_t*)calloc((size_t)ns * np, sizeof(int32_t));
    int32_t* bo = (int32_t*)malloc((ns + 1) * sizeof(int32_t));
    double* bl = (double*)malloc((size_t)ns * 3 * sizeof(double));
    double* bg = (double*)malloc((size_t)ns * 3 * sizeof(double));
    double* o_lat = (double*)malloc((size_t)ns * 9 * 8);
    double* o_vol = (double*)malloc((size_t)ns * 8);
    double* o_frac = (double*)malloc((size_t)ns * np * 24);
    double* o_dmin = (double*)malloc((size_t)ns * 8);
    double* o_near = (double*)malloc((size_t)ns * np * 8);
    int32_t* o_int = (int32_t*)malloc((size_t)ns * (2 + 1 + 1 + 1 + 95) * 4);
    for (int k = 0; k <= ns; ++k) bo[k] = k * np;
    for (int k = 0; k < 3 * ns; ++k) { bl[k] = 9.0; bg[k] = 90.0; }
    OK(ics_op_structure_screen(bo, bs, bx, bl, bg, ns, 0.5, o_lat, o_vol, o_frac, o_dmin, o_int, o_int + 2 * ns, o_int + 3 * ns,
                               o_int + 4 * ns, o_near, o_int + 5 * ns));
    bo[1] = np + 1;   /* a structure above the limit */
    if (ics_op_structure_screen(bo, bs, bx, bl, bg, 1, 0.5, o_lat, o_vol, o_frac, o_dmin, o_int, o_int + 2 * ns, o_int + 3 * ns,
                                o_int + 4 * ns, o_near, o_int + 5 * ns) == 0) {
      fprintf(stderr, "structure: 2049 atoms accepted\n"); return 1;
    }
    free(bx); free(bs); free(bo); free(bl); free(bg); free(o_lat); free(o_vol); free(o_frac); free(o_dmin); free(o_near); free(o_int);
  }
  int bad = 0;
  bad += SCREEN(off, sp, xyz, abc, ang, 0, 0.5) == 0;
  bad += SCREEN(NULL, sp, xyz, abc, ang, NB, 0.5) == 0;
  bad += SCREEN(off, NULL, xyz, abc, ang, NB, 0.5) == 0;
  bad += SCREEN(off, sp, NULL, abc, ang, NB, 0.5) == 0;
  bad += SCREEN(off, sp, xyz, NULL, ang, NB, 0.5) == 0;
  bad += SCREEN(off, sp, xyz, abc, NULL, NB, 0.5) == 0;
  bad += SCREEN(off, sp, xyz, abc, ang, NB, NAN) == 0;
  bad += SCREEN(off, sp, xyz, abc, ang, NB, -0.5) == 0;
  bad += ics_op_structure_screen(off, sp, xyz, abc, ang, NB, 0.5, lat, vol, frac, NULL, pair, nclose, valid, reason, nearest, hist) == 0;
  off[0] = 1; bad += SCREEN(off, sp, xyz, abc, ang, NB, 0.5) == 0; off[0] = 0;
  off[2] = 1; bad += SCREEN(off, sp, xyz, abc, ang, NB, 0.5) == 0; off[2] = 2;
  xyz[7] = NAN; bad += SCREEN(off, sp, xyz, abc, ang, NB, 0.5) == 0; xyz[7] = 0.5;
  xyz[7] = 1e200; bad += SCREEN(off, sp, xyz, abc, ang, NB, 0.5) == 0; xyz[7] = 0.5;
  abc[4] = 0.0; bad += SCREEN(off, sp, xyz, abc, ang, NB, 0.5) == 0; abc[4] = 5.0;
  abc[4] = INFINITY; bad += SCREEN(off, sp, xyz, abc, ang, NB, 0.5) == 0; abc[4] = 5.0;
  abc[3] = 0.01; bad += SCREEN(off, sp, xyz, abc, ang, NB, 0.5) == 0; abc[3] = 5.0;                 /* image range */
  ang[5] = 180.0; bad += SCREEN(off, sp, xyz, abc, ang, NB, 0.5) == 0; ang[5] = 120.0;
  ang[3] = 60.0; ang[4] = 60.0; bad += SCREEN(off, sp, xyz, abc, ang, NB, 0.5) == 0; ang[3] = 90.0; ang[4] = 100.0;   /* no cell */
  ang[5] = NAN; bad += SCREEN(off, sp, xyz, abc, ang, NB, 0.5) == 0; ang[5] = 120.0;
  if (bad) { fprintf(stderr, "structure: %d invalid argument sets accepted\n", bad); return 1; }
  if (!ics_last_error()[0]) { fprintf(stderr, "structure: no error message\n"); return 1; }
  OK(SCREEN(off, sp, xyz, abc, ang, NB, 0.5));     /* still usable */
#undef SCREEN
  return 0;
}

/* Structure matching: the argument checks, the bucket planner (several compositions, one-wave and whole-workgroup
 * structures, ineligible entries, queries without partner, no references) and a pair count far above the chunk that
 * ICSG3D_MATCH_CHUNK_PAIRS (set by main before the first call) leaves. */
static int structure_match_walk(void) {
  enum { NQ = 40, NR = 30, NS = NQ + NR };
  static int32_t off[NS + 1], sp[NS * 70], el[NS];
  static double fr[NS * 70 * 3], lat[NS * 9];
  int32_t dup[NQ], ref[NQ], dop[NQ * 2], rop[NQ * 2], ncmp[NQ * 2];
  double drms[NQ], rrms[NQ];
  int at = 0;
  for (int s = 0; s < NS; ++s) {
    const int n = s % 7 == 0 ? 70 : (s % 3 == 0 ? 5 : 3);       /* three atom counts, two compositions of 3 */
    off[s] = at;
    for (int i = 0; i < n; ++i, ++at) {
      sp[at] = n == 3 && s % 2 ? 8 + i : 1 + (i * 5) % 11;
      fr[3 * at] = 0.013 * at - 3.0; fr[3 * at + 1] = 0.37 * i; fr[3 * at + 2] = 1.0 - 0.11 * i;
    }
    for (int k = 0; k < 9; ++k) lat[9 * s + k] = k % 4 == 0 ? 5.0 + k : (k == 3 ? -1.5 : 0.0);
    el[s] = s % 11 != 10;
  }
  off[NS] = at;
#define MATCH(o, z, f, l, e, nq, nr, t, lt, m) ics_op_structure_match(o, z, f, l, e, nq, nr, t, lt, m, dup, drms, dop, ref, rrms, rop, ncmp)
  OK(MATCH(off, sp, fr, lat, el, NQ, NR, 0.1, 0.05, 1));
  OK(MATCH(off, sp, fr, lat, el, NQ, NR, 0.1, 0.05, 0));
  OK(MATCH(off, sp, fr, lat, el, NQ, NR, 0.1, 0.05, 2));
  OK(MATCH(off, sp, fr, lat, el, NQ, 0, 0.1, 0.05, 1));            /* no references */
  OK(MATCH(off, sp, fr, lat, el, 1, 0, 0.1, 0.05, 1));             /* no pair at all */
  for (int q = 0; q < NQ; ++q)
    if (dup[q] != -1 || ref[q] != -1) { fprintf(stderr, "structure match: a match without a kernel\n"); return 1; }
  { int32_t none[NS]; memset(none, 0, sizeof none); OK(MATCH(off, sp, fr, lat, none, NQ, NR, 0.1, 0.05, 1)); }
  int bad = 0;
  bad += MATCH(off, sp, fr, lat, el, 0, NR, 0.1, 0.05, 1) == 0;
  bad += MATCH(off, sp, fr, lat, el, NQ, -1, 0.1, 0.05, 1) == 0;
  bad += MATCH(NULL, sp, fr, lat, el, NQ, NR, 0.1, 0.05, 1) == 0;
  bad += MATCH(off, NULL, fr, lat, el, NQ, NR, 0.1, 0.05, 1) == 0;
  bad += MATCH(off, sp, NULL, lat, el, NQ, NR, 0.1, 0.05, 1) == 0;
  bad += MATCH(off, sp, fr, NULL, el, NQ, NR, 0.1, 0.05, 1) == 0;
  bad += MATCH(off, sp, fr, lat, NULL, NQ, NR, 0.1, 0.05, 1) == 0;
  bad += ics_op_structure_match(off, sp, fr, lat, el, NQ, NR, 0.1, 0.05, 1, dup, NULL, dop, ref, rrms, rop, ncmp) == 0;
  bad += MATCH(off, sp, fr, lat, el, NQ, NR, 0.0, 0.05, 1) == 0;
  bad += MATCH(off, sp, fr, lat, el, NQ, NR, NAN, 0.05, 1) == 0;
  bad += MATCH(off, sp, fr, lat, el, NQ, NR, 0.1, -0.05, 1) == 0;
  bad += MATCH(off, sp, fr, lat, el, NQ, NR, 0.1, INFINITY, 1) == 0;
  bad += MATCH(off, sp, fr, lat, el, NQ, NR, 0.1, 0.05, 3) == 0;
  bad += MATCH(off, sp, fr, lat, el, NQ, NR, 0.1, 0.05, -1) == 0;
  bad += MATCH(off, sp, fr, lat, el, NQ, NR, 3.0, 0.05, 1) == 0;                                   /* too thin for tol */
  off[0] = 1; bad += MATCH(off, sp, fr, lat, el, NQ, NR, 0.1, 0.05, 1) == 0; off[0] = 0;
  { const int32_t keep = off[2]; off[2] = off[1] - 1; bad += MATCH(off, sp, fr, lat, el, NQ, NR, 0.1, 0.05, 1) == 0; off[2] = keep; }
  fr[7] = NAN; bad += MATCH(off, sp, fr, lat, el, NQ, NR, 0.1, 0.05, 1) == 0; fr[7] = 0.5;
  lat[9 + 4] = INFINITY; bad += MATCH(off, sp, fr, lat, el, NQ, NR, 0.1, 0.05, 1) == 0; lat[9 + 4] = 9.0;
  lat[9 + 4] = -9.0; bad += MATCH(off, sp, fr, lat, el, NQ, NR, 0.1, 0.05, 1) == 0; lat[9 + 4] = 9.0;  /* volume < 0 */
  sp[1] = 95; bad += MATCH(off, sp, fr, lat, el, NQ, NR, 0.1, 0.05, 1) == 0;
  sp[1] = 0; bad += MATCH(off, sp, fr, lat, el, NQ, NR, 0.1, 0.05, 1) == 0; sp[1] = 6;
  {   /* 257 atoms, and an empty eligible structure */
    static int32_t bo[3] = {0, 257, 257}, bs[257], be[2] = {1, 0};
    static double bf[257 * 3], bl[18] = {20, 0, 0, 0, 20, 0, 0, 0, 20, 20, 0, 0, 0, 20, 0, 0, 0, 20};
    for (int i = 0; i < 257; ++i) bs[i] = 8;
    bad += MATCH(bo, bs, bf, bl, be, 2, 0, 0.1, 0.05, 1) == 0;
    be[0] = 0; be[1] = 1; bad += MATCH(bo, bs, bf, bl, be, 2, 0, 0.1, 0.05, 1) == 0;
    be[1] = 0; OK(MATCH(bo, bs, bf, bl, be, 2, 0, 0.1, 0.05, 1));                      /* ineligible: not looked at */
  }
  if (bad) { fprintf(stderr, "structure match: %d invalid argument sets accepted\n", bad); return 1; }
  if (!ics_last_error()[0]) { fprintf(stderr, "structure match: no error message\n"); return 1; }
  OK(MATCH(off, sp, fr, lat, el, NQ, NR, 0.1, 0.05, 1));     /* still usable */
#undef MATCH
  return 0;
}

/* Structure symmetry: the argument checks, the packing (two kernel kinds, an ineligible entry, several chunks under the
 * ICSG3D_SYMMETRY_CHUNK_BYTES main sets) and one refusal of each kind; the kernels are no-ops here, so the counts the
 * host reads back are whatever the stand-in memory holds and must be clamped before they index anything. */
static int structure_symmetry_walk(void) {
  enum { NS = 9, MO = 6, NA = NS * 70 };
  static int32_t off[NS + 1], sp[NA], el[NS], orbit[NA], mult[NA];
  static double fr[NA * 3], lat[NS * 9], sfrac[NA * 3];
  int32_t nlat[NS], nops[NS], npoint[NS], ntrans[NS], types[NS * 10], reason[NS], ocode[NS * MO], oanc[NS * MO];
  double ot[NS * MO * 3], orms[NS * MO], sg[NS * 9], sshift[NS], sresid[NS];
  int at = 0;
  for (int s = 0; s < NS; ++s) {
    const int n = s % 4 == 0 ? 70 : (s % 3 == 0 ? 5 : 3);
    off[s] = at;
    for (int i = 0; i < n; ++i, ++at) {
      sp[at] = 1 + (i * 5) % 11;
      fr[3 * at] = 0.013 * at - 3.0; fr[3 * at + 1] = 0.37 * i; fr[3 * at + 2] = 1.0 - 0.11 * i;
    }
    for (int k = 0; k < 9; ++k) lat[9 * s + k] = k % 4 == 0 ? 5.0 + k : (k == 3 ? -1.5 : 0.0);
    el[s] = s != 5;
  }
  off[NS] = at;
#define SYMM(o, z, f, l, e, ns, t, lt, mo) ics_op_structure_symmetry(o, z, f, l, e, ns, t, lt, mo, nlat, nops, npoint, ntrans, types, reason, ocode, oanc, ot, orms, orbit, mult, sfrac, sg, sshift, sresid)
  OK(SYMM(off, sp, fr, lat, el, NS, 0.1, 0.05, MO));
  if (reason[5] != 1 || orbit[off[5] + 2] != 2 || mult[off[5]] != 1 || sg[9 * 5] != 25.0) {
    fprintf(stderr, "structure symmetry: the ineligible entry is not neutral\n");
    return 1;
  }
  OK(SYMM(off, sp, fr, lat, el, 1, 0.1, 0.05, 1));
  { int32_t none[NS]; memset(none, 0, sizeof none); OK(SYMM(off, sp, fr, lat, none, NS, 0.1, 0.05, MO)); }
  int bad = 0;
  bad += SYMM(off, sp, fr, lat, el, 0, 0.1, 0.05, MO) == 0;
  bad += SYMM(NULL, sp, fr, lat, el, NS, 0.1, 0.05, MO) == 0;
  bad += SYMM(off, NULL, fr, lat, el, NS, 0.1, 0.05, MO) == 0;
  bad += SYMM(off, sp, NULL, lat, el, NS, 0.1, 0.05, MO) == 0;
  bad += SYMM(off, sp, fr, NULL, el, NS, 0.1, 0.05, MO) == 0;
  bad += SYMM(off, sp, fr, lat, NULL, NS, 0.1, 0.05, MO) == 0;
  bad += ics_op_structure_symmetry(off, sp, fr, lat, el, NS, 0.1, 0.05, MO, nlat, nops, npoint, ntrans, types, reason, ocode,
                                   oanc, ot, NULL, orbit, mult, sfrac, sg, sshift, sresid) == 0;
  bad += ics_op_structure_symmetry(off, sp, fr, lat, el, NS, 0.1, 0.05, MO, nlat, nops, npoint, ntrans, types, reason, ocode,
                                   oanc, ot, orms, NULL, mult, sfrac, sg, sshift, sresid) == 0;
  bad += SYMM(off, sp, fr, lat, el, NS, 0.0, 0.05, MO) == 0;
  bad += SYMM(off, sp, fr, lat, el, NS, 0.1, NAN, MO) == 0;
  bad += SYMM(off, sp, fr, lat, el, NS, 0.1, 0.05, 0) == 0;
  bad += SYMM(off, sp, fr, lat, el, NS, 0.1, 0.05, 4097) == 0;
  bad += SYMM(off, sp, fr, lat, el, NS, 3.0, 0.05, MO) == 0;                                       /* too thin for tol */
  off[0] = 1; bad += SYMM(off, sp, fr, lat, el, NS, 0.1, 0.05, MO) == 0; off[0] = 0;
  fr[7] = NAN; bad += SYMM(off, sp, fr, lat, el, NS, 0.1, 0.05, MO) == 0; fr[7] = 0.5;
  lat[9 + 4] = -9.0; bad += SYMM(off, sp, fr, lat, el, NS, 0.1, 0.05, MO) == 0; lat[9 + 4] = 9.0;   /* volume < 0 */
  sp[1] = 95; bad += SYMM(off, sp, fr, lat, el, NS, 0.1, 0.05, MO) == 0; sp[1] = 6;
  {   /* 257 atoms eligible: refused; ineligible: not looked at */
    static int32_t bo[2] = {0, 257}, bs[257], be[1] = {1}, borb[257], bmul[257];
    static double bf[257 * 3], bsf[257 * 3], bl[9] = {20, 0, 0, 0, 20, 0, 0, 0, 20};
    for (int i = 0; i < 257; ++i) bs[i] = 8;
    bad += ics_op_structure_symmetry(bo, bs, bf, bl, be, 1, 0.1, 0.05, MO, nlat, nops, npoint, ntrans, types, reason, ocode,
                                     oanc, ot, orms, borb, bmul, bsf, sg, sshift, sresid) == 0;
    be[0] = 0;
    OK(ics_op_structure_symmetry(bo, bs, bf, bl, be, 1, 0.1, 0.05, MO, nlat, nops, npoint, ntrans, types, reason, ocode,
                                 oanc, ot, orms, borb, bmul, bsf, sg, sshift, sresid));
    if (reason[0] != 1 || borb[256] != 256) { fprintf(stderr, "structure symmetry: 257 ineligible atoms not neutral\n"); return 1; }
  }
  if (bad) { fprintf(stderr, "structure symmetry: %d invalid argument sets accepted\n", bad); return 1; }
  if (!ics_last_error()[0]) { fprintf(stderr, "structure symmetry: no error message\n"); return 1; }
  OK(SYMM(off, sp, fr, lat, el, NS, 0.1, 0.05, MO));     /* still usable */
#undef SYMM
  return 0;
}

/* Structure fingerprints: the argument checks, the packing (two kernel kinds, an ineligible entry, a cell whose image
 * range is above 32, several chunks under the ICSG3D_FINGERPRINT_CHUNK_BYTES main sets) and one refusal of each kind.
 * The nearest op folds its partners on the device; the kernels are no-ops here, so the partners read back are whatever the
 * stand-in memory holds: the call may refuse them, it must not index with them. */
static int structure_fingerprint_walk(void) {
  enum { NS = 9, NB = 7, NA = NS * 70 };
  static int32_t off[NS + 1], sp[NA], el[NS], cn[NA], reason[NS];
  static double fr[NA * 3], lat[NS * 9], nn[NA], rdf[NS * 2 * NB], cnt[NS * NB];
  static int64_t np_[NS];
  int at = 0;
  for (int s = 0; s < NS; ++s) {
    const int n = s % 4 == 0 ? 70 : (s % 3 == 0 ? 5 : 3);
    off[s] = at;
    for (int i = 0; i < n; ++i, ++at) {
      sp[at] = 1 + (i * 5) % 11;
      fr[3 * at] = 0.013 * at - 3.0; fr[3 * at + 1] = 0.37 * i; fr[3 * at + 2] = 1.0 - 0.11 * i;
    }
    for (int k = 0; k < 9; ++k) lat[9 * s + k] = k % 4 == 0 ? (s == 7 ? 0.15 : 5.0 + k) : (k == 3 && s != 7 ? -1.5 : 0.0);
    el[s] = s != 5;
  }
  off[NS] = at;
#define FPR(o, z, f, l, e, ns, rm, nb, w, ct) ics_op_structure_fingerprint(o, z, f, l, e, ns, rm, nb, w, ct, rdf, cnt, np_, nn, cn, reason)
  OK(FPR(off, sp, fr, lat, el, NS, 6.0, NB, 0.1, 0.1));
  if (reason[5] != 1 || reason[7] != 2 || reason[0] != 0 || np_[5] != -1 || cn[off[7]] != -1 || nn[off[5]] == nn[off[5]] ||
      rdf[7 * 2 * NB] == rdf[7 * 2 * NB]) {
    fprintf(stderr, "structure fingerprint: the reason bits or the neutral outputs are wrong\n");
    return 1;
  }
  OK(FPR(off, sp, fr, lat, el, 1, 3.0, 1, 2.0, 0.0));
  { int32_t none[NS]; memset(none, 0, sizeof none); OK(FPR(off, sp, fr, lat, none, NS, 6.0, NB, 0.1, 0.1)); }
  int bad = 0;
  bad += FPR(off, sp, fr, lat, el, 0, 6.0, NB, 0.1, 0.1) == 0;
  bad += FPR(NULL, sp, fr, lat, el, NS, 6.0, NB, 0.1, 0.1) == 0;
  bad += FPR(off, NULL, fr, lat, el, NS, 6.0, NB, 0.1, 0.1) == 0;
  bad += FPR(off, sp, NULL, lat, el, NS, 6.0, NB, 0.1, 0.1) == 0;
  bad += FPR(off, sp, fr, NULL, el, NS, 6.0, NB, 0.1, 0.1) == 0;
  bad += FPR(off, sp, fr, lat, NULL, NS, 6.0, NB, 0.1, 0.1) == 0;
  bad += ics_op_structure_fingerprint(off, sp, fr, lat, el, NS, 6.0, NB, 0.1, 0.1, rdf, cnt, np_, NULL, cn, reason) == 0;
  bad += ics_op_structure_fingerprint(off, sp, fr, lat, el, NS, 6.0, NB, 0.1, 0.1, NULL, cnt, np_, nn, cn, reason) == 0;
  bad += FPR(off, sp, fr, lat, el, NS, 0.0, NB, 0.1, 0.1) == 0;
  bad += FPR(off, sp, fr, lat, el, NS, NAN, NB, 0.1, 0.1) == 0;
  bad += FPR(off, sp, fr, lat, el, NS, 6.0, 0, 0.1, 0.1) == 0;
  bad += FPR(off, sp, fr, lat, el, NS, 6.0, 257, 0.1, 0.1) == 0;
  bad += FPR(off, sp, fr, lat, el, NS, 6.0, NB, 0.0, 0.1) == 0;
  bad += FPR(off, sp, fr, lat, el, NS, 6.0, NB, 0.1, -0.1) == 0;
  off[0] = 1; bad += FPR(off, sp, fr, lat, el, NS, 6.0, NB, 0.1, 0.1) == 0; off[0] = 0;
  fr[7] = NAN; bad += FPR(off, sp, fr, lat, el, NS, 6.0, NB, 0.1, 0.1) == 0; fr[7] = 0.5;
  lat[9 + 4] = -9.0; bad += FPR(off, sp, fr, lat, el, NS, 6.0, NB, 0.1, 0.1) == 0; lat[9 + 4] = 9.0;   /* volume < 0 */
  sp[1] = 95; bad += FPR(off, sp, fr, lat, el, NS, 6.0, NB, 0.1, 0.1) == 0; sp[1] = 6;
  {   /* 257 atoms eligible: refused; ineligible: not looked at */
    static int32_t bo[2] = {0, 257}, bs[257], be[1] = {1}, bcn[257];
    static double bf[257 * 3], bnn[257], bl[9] = {20, 0, 0, 0, 20, 0, 0, 0, 20};
    for (int i = 0; i < 257; ++i) bs[i] = 8;
    bad += ics_op_structure_fingerprint(bo, bs, bf, bl, be, 1, 6.0, NB, 0.1, 0.1, rdf, cnt, np_, bnn, bcn, reason) == 0;
    be[0] = 0;
    OK(ics_op_structure_fingerprint(bo, bs, bf, bl, be, 1, 6.0, NB, 0.1, 0.1, rdf, cnt, np_, bnn, bcn, reason));
    if (reason[0] != 1 || bcn[256] != -1) { fprintf(stderr, "structure fingerprint: 257 ineligible atoms not neutral\n"); return 1; }
  }
  if (bad) { fprintf(stderr, "structure fingerprint: %d invalid argument sets accepted\n", bad); return 1; }
  OK(FPR(off, sp, fr, lat, el, NS, 6.0, NB, 0.1, 0.1));     /* still usable */
#undef FPR
  {
    enum { NQ = 600, NR = 700, LEN = 9 };
    static double fp[(NQ + NR) * LEN], qd[NQ], rd[NR], gd[NQ], dsum;
    static int32_t valid[NQ + NR], qr[NQ], rq[NR], qq[NQ];
    int64_t dpairs = 0;
    for (int k = 0; k < (NQ + NR) * LEN; ++k) fp[k] = 0.001 * (k % 977);
    for (int k = 0; k < NQ + NR; ++k) valid[k] = k % 11 != 3;
#define NEAR(f, v, len, nq, nr) ics_op_fingerprint_nearest(f, v, len, nq, nr, qr, qd, rq, rd, qq, gd, &dsum, &dpairs)
    (void)NEAR(fp, valid, LEN, NQ, NR);
    (void)NEAR(fp, valid, LEN, NQ, 0);
    (void)NEAR(fp, valid, 1, 1, 0);
    { static int32_t none[NQ + NR]; OK(NEAR(fp, none, LEN, NQ, NR)); if (qr[0] != -1 || rq[NR - 1] != -1 || dpairs != 0) return 1; }
    bad += NEAR(NULL, valid, LEN, NQ, NR) == 0;
    bad += NEAR(fp, NULL, LEN, NQ, NR) == 0;
    bad += NEAR(fp, valid, 0, NQ, NR) == 0;
    bad += NEAR(fp, valid, LEN, 0, NR) == 0;
    bad += NEAR(fp, valid, LEN, NQ, -1) == 0;
    bad += ics_op_fingerprint_nearest(fp, valid, LEN, NQ, NR, qr, qd, NULL, rd, qq, gd, &dsum, &dpairs) == 0;
    bad += ics_op_fingerprint_nearest(fp, valid, LEN, NQ, NR, qr, qd, rq, rd, qq, gd, NULL, &dpairs) == 0;
    fp[5 * LEN + 2] = INFINITY; bad += NEAR(fp, valid, LEN, NQ, NR) == 0; fp[5 * LEN + 2] = 0.25;
#undef NEAR
    if (bad) { fprintf(stderr, "fingerprint nearest: %d invalid argument sets accepted\n", bad); return 1; }
    if (!ics_last_error()[0]) { fprintf(stderr, "fingerprint nearest: no error message\n"); return 1; }
  }
  return 0;
}

/* view_results.py's pictures: the three ops over more than one picture and an image that is no multiple of the tile, an
 * empty atom set, every refusal, and the ops still usable afterwards. */
static int render_walk(void) {
  enum { B = 3, D = 8, C = 4, W = 50, H = 37, NA = 4 };
  static float vol[B * D * D * D * C], lut[256 * 3], out[B * W * H * 4];
  static int32_t lab[B * D * D * D];
  float pal[2 * 3] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
  int32_t off[B + 1] = {0, 3, 3, 4}, sp[NA] = {1, 12, -5, 7};
  double xyz[NA * 3] = {4, 4, 4, 5, 4.5, 3, 2, 3, 6, 1, 1, 1}, cam[2] = {30.0, -60.0}, top[2] = {90.0, 0.0};
  int bad = 0;
  for (int i = 0; i < B * D * D * D * C; ++i) vol[i] = (float)((i * 37) % 101) * 0.012f - 0.1f;
  for (int i = 0; i < B * D * D * D; ++i) lab[i] = (i * 13) % 7 == 0 ? i % 40 : 0;
  for (int i = 0; i < 256 * 3; ++i) lut[i] = (float)i / 768.f;
#define DENS(v, b, d, sc, ch, l, m, a, c, w, h, o) ics_op_render_density(v, b, d, sc, ch, l, m, a, -1.f, c, w, h, o)
  OK(DENS(vol, B, D, C, 0, lut, 0, 0.2f, cam, W, H, out));
  OK(DENS(vol, B, D, C, 3, lut, 1, 1.f, top, W, H, out));
  OK(DENS(vol, 1, 1, 1, 0, lut, 1, 0.5f, cam, 1, 1, out));
  OK(ics_op_render_labels(lab, B, D, pal, 2, 0.5f, cam, W, H, out));
  OK(ics_op_render_atoms(off, sp, xyz, B, D, 1.5, pal, 2, top, W, H, out));
  bad += ics_op_render_atoms(off, NULL, NULL, 1, D, 1.5, pal, 2, cam, W, H, out) == 0;   /* atoms without arrays */
  { int32_t none[2] = {0, 0}; OK(ics_op_render_atoms(none, NULL, NULL, 1, D, 1.5, pal, 2, cam, W, H, out)); }
  bad += DENS(NULL, B, D, C, 0, lut, 0, 0.2f, cam, W, H, out) == 0;
  bad += DENS(vol, 0, D, C, 0, lut, 0, 0.2f, cam, W, H, out) == 0;
  bad += DENS(vol, B, 0, C, 0, lut, 0, 0.2f, cam, W, H, out) == 0;
  bad += DENS(vol, B, 257, C, 0, lut, 0, 0.2f, cam, W, H, out) == 0;
  bad += DENS(vol, B, D, C, C, lut, 0, 0.2f, cam, W, H, out) == 0;
  bad += DENS(vol, B, D, 0, 0, lut, 0, 0.2f, cam, W, H, out) == 0;
  bad += DENS(vol, B, D, C, 0, NULL, 0, 0.2f, cam, W, H, out) == 0;
  bad += DENS(vol, B, D, C, 0, lut, 2, 0.2f, cam, W, H, out) == 0;
  bad += DENS(vol, B, D, C, 0, lut, 0, 1.5f, cam, W, H, out) == 0;
  bad += DENS(vol, B, D, C, 0, lut, 0, NAN, cam, W, H, out) == 0;
  bad += DENS(vol, B, D, C, 0, lut, 0, 0.2f, NULL, W, H, out) == 0;
  bad += DENS(vol, B, D, C, 0, lut, 0, 0.2f, cam, 0, H, out) == 0;
  bad += DENS(vol, B, D, C, 0, lut, 0, 0.2f, cam, W, 4097, out) == 0;
  bad += DENS(vol, B, D, C, 0, lut, 0, 0.2f, cam, W, H, NULL) == 0;
  bad += ics_op_render_density(vol, B, D, C, 0, lut, 0, 0.2f, NAN, cam, W, H, out) == 0;
  cam[1] = INFINITY; bad += DENS(vol, B, D, C, 0, lut, 0, 0.2f, cam, W, H, out) == 0; cam[1] = -60.0;
#undef DENS
  bad += ics_op_render_labels(NULL, B, D, pal, 2, 0.5f, cam, W, H, out) == 0;
  bad += ics_op_render_labels(lab, B, D, NULL, 2, 0.5f, cam, W, H, out) == 0;
  bad += ics_op_render_labels(lab, B, D, pal, 0, 0.5f, cam, W, H, out) == 0;
  bad += ics_op_render_labels(lab, B, D, pal, 2, -0.5f, cam, W, H, out) == 0;
  bad += ics_op_render_atoms(NULL, sp, xyz, B, D, 1.5, pal, 2, cam, W, H, out) == 0;
  bad += ics_op_render_atoms(off, sp, xyz, B, D, 0.0, pal, 2, cam, W, H, out) == 0;
  bad += ics_op_render_atoms(off, sp, xyz, B, D, 1.5, pal, 0, cam, W, H, out) == 0;
  off[0] = 1; bad += ics_op_render_atoms(off, sp, xyz, B, D, 1.5, pal, 2, cam, W, H, out) == 0; off[0] = 0;
  off[2] = 2; bad += ics_op_render_atoms(off, sp, xyz, B, D, 1.5, pal, 2, cam, W, H, out) == 0; off[2] = 3;
  xyz[4] = NAN; bad += ics_op_render_atoms(off, sp, xyz, B, D, 1.5, pal, 2, cam, W, H, out) == 0; xyz[4] = 4.5;
  if (bad) { fprintf(stderr, "render: %d invalid calls accepted\n", bad); return 1; }
  OK(ics_op_render_labels(lab, B, D, pal, 2, 0.5f, cam, W, H, out));
  return 0;
}

/* The training monitors: the three ops at sizes that are no multiple of a tile or a chunk, every refusal, the resident
 * slices of both engines with each `which` refused until the pass that fills it has run, and the KDE handle fed from the
 * host and from the VAE engine. */
static int monitor_walk(ics_net* unet, ics_net* vae, const float* x, const uint8_t* lab, const float* cond, const float* eps,
                        int B, int d) {
  enum { NB = 3, D = 5, SC = 4, Z = 3, NC = 3, NP = 5, W = 37, H = 21, KD = 3, KN = 7, KP = 6 };
  static float vol[NB * D * D * D * SC], lut[256 * 3], out[NB * D * Z * D * Z * 4], img[W * H * 4];
  static uint8_t vol8[NB * D * D * D * SC];
  static int32_t vol32[NB * D * D * D * SC];
  float range[2] = {0.25f, 0.75f}, pal[2 * 3] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f}, codes[KN * KD];
  double xy[NC * NP * 2], win[4] = {0.0, 4.0, -1.0, 1.0}, grid[KP], dens[KD * KP], bw[KD];
  int32_t status[KD];
  int bad = 0, cnt = 0;
#define REFUSED(x) do { if ((x) == 0) { ++bad; fprintf(stderr, "monitor: accepted at line %d: %s\n", __LINE__, #x); } } while (0)
  for (int i = 0; i < NB * D * D * D * SC; ++i) { vol[i] = (float)((i * 37) % 101) / 64.f; vol8[i] = (uint8_t)(i * 7); vol32[i] = i * 13 - 900; }
  vol[11] = NAN;
  for (int i = 0; i < 256 * 3; ++i) lut[i] = (float)i / 768.f;
  for (int c = 0; c < NC; ++c)
    for (int k = 0; k < NP; ++k) { xy[(c * NP + k) * 2] = (double)k; xy[(c * NP + k) * 2 + 1] = 0.3 * c - 0.1 * k; }
  xy[(1 * NP + 2) * 2] = NAN;
  for (int i = 0; i < KN * KD; ++i) codes[i] = i % KD == 2 ? 0.5f : 0.01f * (float)((i * 29) % 53) - 0.2f;
  for (int k = 0; k < KP; ++k) grid[k] = -3.0 + 1.2 * k;
#define SLICE(v, t, b, dd, sc, ch, ax, ix, l, r, z, o) ics_op_render_slice(v, t, b, dd, sc, ch, ax, ix, l, r, z, o)
  for (int ax = 0; ax < 3; ++ax) {
    OK(SLICE(vol, 0, NB, D, SC, 2, ax, ax + 1, lut, NULL, Z, out));
    OK(SLICE(vol8, 1, NB, D, SC, 0, ax, 0, lut, range, 1, out));
    OK(SLICE(vol32, 2, NB, D, SC, 3, ax, D - 1, lut, NULL, 2, out));
  }
  OK(SLICE(vol, 0, 1, 1, 1, 0, 0, 0, lut, NULL, 1, out));
  REFUSED(SLICE(NULL, 0, NB, D, SC, 2, 2, 2, lut, NULL, Z, out));
  REFUSED(SLICE(vol, 0, NB, D, SC, 2, 2, 2, NULL, NULL, Z, out));
  REFUSED(SLICE(vol, 0, NB, D, SC, 2, 2, 2, lut, NULL, Z, NULL));
  REFUSED(SLICE(vol, 3, NB, D, SC, 2, 2, 2, lut, NULL, Z, out));
  REFUSED(SLICE(vol, -1, NB, D, SC, 2, 2, 2, lut, NULL, Z, out));
  REFUSED(SLICE(vol, 0, 0, D, SC, 2, 2, 2, lut, NULL, Z, out));
  REFUSED(SLICE(vol, 0, NB, 0, SC, 2, 2, 0, lut, NULL, Z, out));
  REFUSED(SLICE(vol, 0, NB, 257, SC, 2, 2, 2, lut, NULL, Z, out));
  REFUSED(SLICE(vol, 0, NB, D, SC, SC, 2, 2, lut, NULL, Z, out));
  REFUSED(SLICE(vol, 0, NB, D, SC, -1, 2, 2, lut, NULL, Z, out));
  REFUSED(SLICE(vol, 0, NB, D, 0, 0, 2, 2, lut, NULL, Z, out));
  REFUSED(SLICE(vol, 0, NB, D, SC, 2, 3, 2, lut, NULL, Z, out));
  REFUSED(SLICE(vol, 0, NB, D, SC, 2, -1, 2, lut, NULL, Z, out));
  REFUSED(SLICE(vol, 0, NB, D, SC, 2, 2, D, lut, NULL, Z, out));
  REFUSED(SLICE(vol, 0, NB, D, SC, 2, 2, -1, lut, NULL, Z, out));
  REFUSED(SLICE(vol, 0, NB, D, SC, 2, 2, 2, lut, NULL, 0, out));
  REFUSED(SLICE(vol, 0, NB, D, SC, 2, 2, 2, lut, NULL, 65, out));
  REFUSED(SLICE(vol, 0, NB, 256, SC, 2, 2, 2, lut, NULL, 17, out));          /* side 4352 */
  range[0] = NAN; REFUSED(SLICE(vol, 0, NB, D, SC, 2, 2, 2, lut, range, Z, out)); range[0] = 0.25f;
  range[1] = INFINITY; REFUSED(SLICE(vol, 0, NB, D, SC, 2, 2, 2, lut, range, Z, out)); range[1] = 0.75f;
  range[1] = 0.f; REFUSED(SLICE(vol, 0, NB, D, SC, 2, 2, 2, lut, range, Z, out)); range[1] = 0.75f;
#undef SLICE
#define LINES(p, nc, np, w, pl, npl, wp, a, ww, hh, o) ics_op_render_lines(p, nc, np, w, pl, npl, wp, a, ww, hh, o)
  OK(LINES(xy, NC, NP, win, pal, 2, 1.5, 0.5f, W, H, img));
  OK(LINES(xy, 1, 2, win, pal, 1, 0.25, 1.f, 1, 1, img));
  REFUSED(LINES(NULL, NC, NP, win, pal, 2, 1.5, 0.5f, W, H, img));
  REFUSED(LINES(xy, NC, NP, NULL, pal, 2, 1.5, 0.5f, W, H, img));
  REFUSED(LINES(xy, NC, NP, win, NULL, 2, 1.5, 0.5f, W, H, img));
  REFUSED(LINES(xy, NC, NP, win, pal, 2, 1.5, 0.5f, W, H, NULL));
  REFUSED(LINES(xy, NC, 1, win, pal, 2, 1.5, 0.5f, W, H, img));
  REFUSED(LINES(xy, NC, 4097, win, pal, 2, 1.5, 0.5f, W, H, img));
  REFUSED(LINES(xy, 0, NP, win, pal, 2, 1.5, 0.5f, W, H, img));
  REFUSED(LINES(xy, 65536, NP, win, pal, 2, 1.5, 0.5f, W, H, img));
  REFUSED(LINES(xy, NC, NP, win, pal, 0, 1.5, 0.5f, W, H, img));
  REFUSED(LINES(xy, NC, NP, win, pal, 2, 0.0, 0.5f, W, H, img));
  REFUSED(LINES(xy, NC, NP, win, pal, 2, NAN, 0.5f, W, H, img));
  REFUSED(LINES(xy, NC, NP, win, pal, 2, 1.5, 1.5f, W, H, img));
  REFUSED(LINES(xy, NC, NP, win, pal, 2, 1.5, -0.5f, W, H, img));
  REFUSED(LINES(xy, NC, NP, win, pal, 2, 1.5, 0.5f, 0, H, img));
  REFUSED(LINES(xy, NC, NP, win, pal, 2, 1.5, 0.5f, W, 4097, img));
  win[1] = 0.0; REFUSED(LINES(xy, NC, NP, win, pal, 2, 1.5, 0.5f, W, H, img)); win[1] = 4.0;
  win[3] = -1.0; REFUSED(LINES(xy, NC, NP, win, pal, 2, 1.5, 0.5f, W, H, img)); win[3] = 1.0;
  win[2] = NAN; REFUSED(LINES(xy, NC, NP, win, pal, 2, 1.5, 0.5f, W, H, img)); win[2] = -1.0;
#undef LINES
  {
    ics_kde* h = NULL;
    REFUSED(ics_op_kde_create(0, 8, &h));
    REFUSED(ics_op_kde_create(4097, 8, &h));
    REFUSED(ics_op_kde_create(KD, 1, &h));
    REFUSED(ics_op_kde_create(KD, (1 << 20) + 1, &h));
    REFUSED(ics_op_kde_create(KD, 8, NULL));
    OK(ics_op_kde_create(KD, KN, &h));
    OK(ics_op_kde_append(h, codes, 1));
    REFUSED(ics_op_kde_evaluate(h, grid, KP, dens, bw, status, &cnt));        /* one code */
    OK(ics_op_kde_append(h, codes + KD, KN - 1));
    REFUSED(ics_op_kde_append(h, codes, 1));                                  /* over capacity */
    REFUSED(ics_op_kde_append(NULL, codes, 1));
    OK(ics_op_kde_evaluate(h, grid, KP, dens, bw, status, &cnt));
    OK(ics_op_kde_evaluate(h, grid, 1, dens, NULL, NULL, NULL));
    if (cnt != KN) { fprintf(stderr, "kde: count %d\n", cnt); return 1; }
    REFUSED(ics_op_kde_evaluate(h, NULL, KP, dens, bw, status, &cnt));
    REFUSED(ics_op_kde_evaluate(h, grid, KP, NULL, bw, status, &cnt));
    REFUSED(ics_op_kde_evaluate(h, grid, 0, dens, bw, status, &cnt));
    REFUSED(ics_op_kde_evaluate(h, grid, 4097, dens, bw, status, &cnt));
    REFUSED(ics_op_kde_evaluate(NULL, grid, KP, dens, bw, status, &cnt));
    OK(ics_op_kde_destroy(h));
    OK(ics_op_kde_destroy(NULL));
    OK(ics_op_kde_create(KD, KN, &h));
    codes[4] = INFINITY; REFUSED(ics_op_kde_append(h, codes, 2)); codes[4] = 0.f;
    REFUSED(ics_op_kde_append(h, NULL, 2));
    REFUSED(ics_op_kde_append(h, codes, 0));
    OK(ics_op_kde_destroy(h));
  }
  if (vae) {
    const size_t side = (size_t)d * 2;
    float* pic = (float*)malloc((size_t)B * side * side * 4 * sizeof(float));
    static float z[3 * 8 * 256];
    static double vd[256 * KP];
    ics_net* v2 = NULL;
    ics_vae_config vc = {1, 10, 256, {16, 32, 64, 128}, d, B, 5e-4f, 0.5f, 3e-4f, {1.f, 1.f, 1.f, 1.f}, 1};
    ics_unet_config uc = {1, 95, d, B, 1e-3f, 0.f, 1, 1, 0};
    ics_net* u2 = NULL;
    ics_kde* hv = NULL;
#define VS(n, wh, ch, c, ax, ix, l, r, zz, o) ics_vae_render_slice_resident(n, wh, ch, c, ax, ix, l, r, zz, o)
#define US(n, wh, ch, c, ax, ix, l, r, zz, o) ics_unet_render_slice_resident(n, wh, ch, c, ax, ix, l, r, zz, o)
    OK(ics_vae_create(&vc, unet, &v2));
    REFUSED(VS(v2, 0, 0, 1, 2, d / 2, lut, NULL, 2, pic));                  /* no resident batch */
    OK(ics_vae_upload_batch(v2, x, cond, eps, B));
    OK(VS(v2, 0, 0, B, 2, d / 2, lut, NULL, 2, pic));
    OK(VS(v2, 0, 0, 1, 0, 0, lut, range, 1, pic));
    REFUSED(VS(v2, 1, 0, 1, 2, d / 2, lut, NULL, 2, pic));                  /* no decoder pass */
    REFUSED(VS(v2, 2, 0, 1, 2, d / 2, lut, NULL, 2, pic));
    REFUSED(VS(v2, 0, 1, 1, 2, d / 2, lut, NULL, 2, pic));                  /* channel */
    REFUSED(VS(v2, 0, 0, B + 1, 2, d / 2, lut, NULL, 2, pic));
    REFUSED(VS(v2, 0, 0, 0, 2, d / 2, lut, NULL, 2, pic));
    REFUSED(VS(v2, 0, 0, 1, 3, d / 2, lut, NULL, 2, pic));
    REFUSED(VS(v2, 0, 0, 1, 2, d, lut, NULL, 2, pic));
    REFUSED(VS(v2, 0, 0, 1, 2, d / 2, NULL, NULL, 2, pic));
    REFUSED(VS(v2, 0, 0, 1, 2, d / 2, lut, NULL, 2, NULL));
    REFUSED(VS(v2, 0, 0, 1, 2, d / 2, lut, NULL, 65, pic));
    REFUSED(VS(unet, 0, 0, 1, 2, d / 2, lut, NULL, 2, pic));
    REFUSED(VS(NULL, 0, 0, 1, 2, d / 2, lut, NULL, 2, pic));
    OK(ics_vae_encode(v2, x, cond, eps, B, z, z + 8 * 256, z + 16 * 256));
    {
      float* rec = (float*)malloc((size_t)B * d * d * d * sizeof(float));
      OK(ics_vae_decode(v2, z + 16 * 256, cond, B, rec));
      free(rec);
    }
    OK(VS(v2, 1, 0, B, 1, d - 1, lut, NULL, 2, pic));
    OK(ics_op_kde_create(256, 2 * B + 1, &hv));
    OK(ics_op_kde_append_vae(hv, v2, B, 1));
    OK(ics_op_kde_append_vae(hv, v2, B, 0));
    OK(ics_op_kde_append_vae(hv, v2, 1, 1));
    REFUSED(ics_op_kde_append_vae(hv, v2, 1, 1));                           /* over capacity */
    OK(ics_op_kde_evaluate(hv, grid, KP, vd, NULL, NULL, &cnt));
    OK(ics_op_kde_destroy(hv));
    OK(ics_op_kde_create(256, 4 * B, &hv));
    REFUSED(ics_op_kde_append_vae(hv, v2, B + 1, 1));
    REFUSED(ics_op_kde_append_vae(hv, v2, 0, 1));
    REFUSED(ics_op_kde_append_vae(hv, v2, 1, 2));
    REFUSED(ics_op_kde_append_vae(hv, unet, 1, 1));
    REFUSED(ics_op_kde_append_vae(hv, NULL, 1, 1));
    REFUSED(ics_op_kde_append_vae(NULL, v2, 1, 1));
    OK(ics_op_kde_destroy(hv));
    OK(ics_op_kde_create(7, 4, &hv)); REFUSED(ics_op_kde_append_vae(hv, v2, 1, 1)); OK(ics_op_kde_destroy(hv));
    OK(ics_net_destroy(v2));
    OK(ics_unet_create(&uc, &u2));
    REFUSED(US(u2, 0, 0, 1, 2, d / 2, lut, NULL, 2, pic));                  /* no resident batch */
    {
      float* soft = (float*)malloc((size_t)B * d * d * d * 95 * sizeof(float));
      OK(ics_unet_predict(u2, x, B, soft, NULL));                              /* uploads without labels */
      free(soft);
    }
    OK(US(u2, 0, 0, B, 2, d / 2, lut, NULL, 2, pic));
    OK(US(u2, 2, 0, B, 2, d / 2, lut, NULL, 2, pic));
    REFUSED(US(u2, 1, 0, 1, 2, d / 2, lut, NULL, 2, pic));                  /* probabilities only */
    REFUSED(US(u2, 3, 0, 1, 2, d / 2, lut, NULL, 2, pic));                  /* no labels uploaded */
    OK(ics_unet_upload_batch(u2, x, lab, B));
    OK(US(u2, 3, 0, B, 2, d / 2, lut, NULL, 2, pic));
    REFUSED(US(u2, 2, 0, B, 2, d / 2, lut, NULL, 2, pic));                  /* the predict was of the batch before */
    OK(ics_unet_predict_resident(u2, 1, 0.8f));
    OK(US(u2, 1, 0, B, 0, 1, lut, range, 1, pic));
    REFUSED(US(u2, 2, 0, 1, 2, d / 2, lut, NULL, 2, pic));                  /* labels only */
    OK(ics_unet_predict_resident(u2, 0, 0.8f));
    OK(US(u2, 2, 0, 1, 1, 0, lut, NULL, 2, pic));
    REFUSED(US(u2, 1, 0, 1, 2, d / 2, lut, NULL, 2, pic));
    REFUSED(US(u2, 4, 0, 1, 2, d / 2, lut, NULL, 2, pic));
    REFUSED(US(u2, -1, 0, 1, 2, d / 2, lut, NULL, 2, pic));
    REFUSED(US(u2, 2, 1, 1, 2, d / 2, lut, NULL, 2, pic));                  /* channel of a one-channel volume */
    REFUSED(US(u2, 0, 1, 1, 2, d / 2, lut, NULL, 2, pic));
    REFUSED(US(u2, 0, 0, B + 1, 2, d / 2, lut, NULL, 2, pic));
    REFUSED(US(vae, 0, 0, 1, 2, d / 2, lut, NULL, 2, pic));
    {
      float mm[5];
      OK(ics_unet_test_step(u2, x, lab, B, mm));                               /* another forward pass discards the predict */
      REFUSED(US(u2, 2, 0, 1, 2, d / 2, lut, NULL, 2, pic));
      OK(US(u2, 3, 0, B, 2, d / 2, lut, NULL, 2, pic));
    }
    OK(ics_net_destroy(u2));
#undef VS
#undef US
    free(pic);
  }
#undef REFUSED
  if (bad) { fprintf(stderr, "monitor: %d invalid calls accepted\n", bad); return 1; }
  if (!ics_last_error()[0]) { fprintf(stderr, "monitor: no error message\n"); return 1; }
  return 0;
}

/* The reconstruction chain's refusals: no resident batch, a U-Net of other channels, a resident batch above the U-Net's
 * max_batch. */
static int reconstruct_refusals(ics_net* unet, const ics_vae_config* vc, const ics_unet_config* uc, const float* x,
                                const float* cond, const float* eps, int B) {
  int32_t counts[2 * 8];
  int32_t* stats = (int32_t*)malloc((size_t)B * 16 * 11 * sizeof(int32_t));
  ics_net* v2 = NULL;
  int bad = 0;
  OK(ics_vae_create(vc, unet, &v2));
  bad += ics_vae_reconstruct_resident_to_unet_atoms(v2, unet, 0.8f, 3, 16, NULL, NULL, NULL, NULL, NULL, counts, stats,
                                                    NULL) == 0;
  /* ics_vae_render_resident: refused without a resident batch, the reconstruction refused before a decoder pass */
  static float lut[256 * 3];
  const double cam[2] = {30.0, -60.0};
  float* img = (float*)malloc((size_t)B * 20 * 13 * 4 * sizeof(float));
  bad += ics_vae_render_resident(v2, 0, 1, 0.5f, -1.f, lut, cam, 20, 13, img) == 0;
  OK(ics_vae_upload_batch(v2, x, cond, eps, B));
  OK(ics_vae_render_resident(v2, 0, 1, 0.5f, -1.f, lut, cam, 20, 13, img));
  bad += ics_vae_render_resident(v2, 1, 1, 0.5f, -1.f, lut, cam, 20, 13, img) == 0;
  bad += ics_vae_render_resident(v2, 2, 1, 0.5f, -1.f, lut, cam, 20, 13, img) == 0;
  bad += ics_vae_render_resident(unet, 0, 1, 0.5f, -1.f, lut, cam, 20, 13, img) == 0;
  bad += ics_vae_render_resident(v2, 0, 1, 0.5f, -1.f, NULL, cam, 20, 13, img) == 0;
  bad += ics_vae_render_resident(v2, 0, 1, 0.5f, -1.f, lut, cam, 20, 13, NULL) == 0;
  OK(ics_vae_reconstruct_resident_to_unet_atoms(v2, unet, 0.8f, 3, 16, NULL, NULL, NULL, NULL, NULL, counts, stats, NULL));
  OK(ics_vae_render_resident(v2, 1, 0, 0.2f, 0.1f, lut, cam, 20, 13, img));
  free(img);
  bad += ics_vae_reconstruct_resident_to_unet_atoms(v2, unet, 0.8f, 3, 16, NULL, NULL, NULL, NULL, NULL, NULL, stats,
                                                    NULL) == 0;
  bad += ics_vae_reconstruct_resident_to_unet_atoms(unet, v2, 0.8f, 3, 16, NULL, NULL, NULL, NULL, NULL, counts, stats,
                                                    NULL) == 0;
  {
    ics_unet_config u2 = *uc;
    u2.in_channels = uc->in_channels == 1 ? 4 : 1;
    ics_net* un2 = NULL;
    OK(ics_unet_create(&u2, &un2));
    bad += ics_vae_reconstruct_resident_to_unet_atoms(v2, un2, 0.8f, 3, 16, NULL, NULL, NULL, NULL, NULL, counts, stats,
                                                      NULL) == 0;
    OK(ics_net_destroy(un2));
  }
  if (B > 1) {
    ics_unet_config u3 = *uc;
    u3.max_batch = B - 1;
    ics_net* un3 = NULL;
    OK(ics_unet_create(&u3, &un3));
    bad += ics_vae_reconstruct_resident_to_unet_atoms(v2, un3, 0.8f, 3, 16, NULL, NULL, NULL, NULL, NULL, counts,
                                                      stats, NULL) == 0;
    OK(ics_vae_upload_batch(v2, x, cond, eps, B - 1));
    OK(ics_vae_reconstruct_resident_to_unet_atoms(v2, un3, 0.8f, 3, 16, NULL, NULL, NULL, NULL, NULL, counts, stats,
                                                  NULL));
    OK(ics_net_destroy(un3));
  }
  OK(ics_net_destroy(v2));
  free(stats);
  if (bad) { fprintf(stderr, "reconstruct: %d invalid calls accepted\n", bad); return 1; }
  return 0;
}

/* interpolate.py's walk: the kernel's op and the two chains (valid calls over several groups, then every refusal; the
 * handle stays usable and a resident step is refused afterwards). */
static int latent_walk(void) {
  enum { P = 3, LAT = 70, S = 4 };
  float za[P * LAT], zb[P * LAT];
  static float path[P * S * LAT];
  double alpha[S] = {0.0, 0.5, 1.0, 1.5};
  int bad = 0;
  for (int i = 0; i < P * LAT; ++i) { za[i] = 0.01f * i; zb[i] = 1.f - 0.02f * i; }
  OK(ics_op_latent_path(za, zb, P, LAT, alpha, S, 0, path));
  OK(ics_op_latent_path(za, zb, P, LAT, alpha, S, 1, path));
  OK(ics_op_latent_path(za, zb, 1, 1, alpha, 1, 0, path));
  bad += ics_op_latent_path(za, zb, 0, LAT, alpha, S, 0, path) == 0;
  bad += ics_op_latent_path(za, zb, P, 0, alpha, S, 0, path) == 0;
  bad += ics_op_latent_path(za, zb, P, LAT, alpha, 0, 0, path) == 0;
  bad += ics_op_latent_path(za, zb, P, LAT, alpha, S, 2, path) == 0;
  bad += ics_op_latent_path(NULL, zb, P, LAT, alpha, S, 0, path) == 0;
  bad += ics_op_latent_path(za, NULL, P, LAT, alpha, S, 0, path) == 0;
  bad += ics_op_latent_path(za, zb, P, LAT, NULL, S, 0, path) == 0;
  bad += ics_op_latent_path(za, zb, P, LAT, alpha, S, 0, NULL) == 0;
  alpha[2] = NAN; bad += ics_op_latent_path(za, zb, P, LAT, alpha, S, 0, path) == 0;
  alpha[2] = INFINITY; bad += ics_op_latent_path(za, zb, P, LAT, alpha, S, 1, path) == 0; alpha[2] = 1.0;
  if (bad) { fprintf(stderr, "latent path: %d invalid calls accepted\n", bad); return 1; }
  OK(ics_op_latent_path(za, zb, P, LAT, alpha, S, 0, path));
  return 0;
}

/* The t-SNE map: the two ops, the handle from host codes and from a VAE engine's encoder output, every refusal (outputs
 * untouched), and the handle still usable afterwards. */
static int tsne_walk(ics_net* vae, ics_net* unet, const float* x, const float* cond, const float* eps, int B) {
  enum { N = 70, D = 5, K = 16 };
  static float codes[N * D];
  static int32_t idx[N * K];
  static double d2[N * K], cp[N * K], sec[3];
  static float init[N * 2], emb[N * 2], grad[N * 2];
  int bad = 0, done = 0, n_iter = 0, count = 0;
  double kl = 0, gn = 0;
  for (int i = 0; i < N * D; ++i) codes[i] = (float)((i * 37) % 101) * 0.01f;
  for (int i = 0; i < N * 2; ++i) init[i] = 1e-4f * (float)(i % 13);
  OK(ics_op_tsne_knn(codes, N, D, K, idx, d2));
  OK(ics_op_tsne_knn(codes, 2, 1, 1, idx, d2));
  for (int i = 0; i < N * K; ++i) d2[i] = 0.5 + 0.01 * i;
  OK(ics_op_tsne_affinities(d2, N, K, 5.0, cp));
  bad += ics_op_tsne_knn(NULL, N, D, K, idx, d2) == 0;
  bad += ics_op_tsne_knn(codes, 1, D, 1, idx, d2) == 0;
  bad += ics_op_tsne_knn(codes, N, 0, K, idx, d2) == 0;
  bad += ics_op_tsne_knn(codes, N, 4097, K, idx, d2) == 0;
  bad += ics_op_tsne_knn(codes, N, D, N, idx, d2) == 0;
  bad += ics_op_tsne_knn(codes, N, D, 0, idx, d2) == 0;
  codes[3] = NAN; bad += ics_op_tsne_knn(codes, N, D, K, idx, d2) == 0; codes[3] = 0.5f;
  bad += ics_op_tsne_affinities(d2, N, K, 0.0, cp) == 0;
  bad += ics_op_tsne_affinities(NULL, N, K, 5.0, cp) == 0;
  bad += ics_op_tsne_affinities(d2, N, 0, 5.0, cp) == 0;
  d2[5] = -1.0; bad += ics_op_tsne_affinities(d2, N, K, 5.0, cp) == 0; d2[5] = 1.0;

  ics_tsne_config c = {D, N, 2, 5.0, 12.0, 4, 12, 2, 300, 1e-7, -1.0};
  ics_tsne* h = NULL;
  { ics_tsne_config b2 = c; b2.n_components = 3; bad += ics_op_tsne_create(&b2, &h) == 0; }
  { ics_tsne_config b2 = c; b2.capacity = 1; bad += ics_op_tsne_create(&b2, &h) == 0; }
  { ics_tsne_config b2 = c; b2.dim = 0; bad += ics_op_tsne_create(&b2, &h) == 0; }
  { ics_tsne_config b2 = c; b2.exaggeration_iter = 13; bad += ics_op_tsne_create(&b2, &h) == 0; }
  bad += ics_op_tsne_create(NULL, &h) == 0;
  OK(ics_op_tsne_create(&c, &h));
  bad += ics_op_tsne_prepare(h, init, 0, 2, sec) == 0;                 /* no codes */
  bad += ics_op_tsne_run(h, 1, &done) == 0;                           /* no graph */
  OK(ics_op_tsne_append(h, codes, 1));
  bad += ics_op_tsne_prepare(h, init, 1, 2, sec) == 0;                 /* N < 2 */
  OK(ics_op_tsne_append(h, codes + D, 3));
  bad += ics_op_tsne_prepare(h, init, 4, 2, sec) == 0;                 /* perplexity 5 >= N = 4 */
  OK(ics_op_tsne_append(h, codes + 4 * D, N - 4));
  bad += ics_op_tsne_append(h, codes, 1) == 0;                        /* over capacity */
  codes[7] = INFINITY; bad += ics_op_tsne_append(h, codes, 1) == 0; codes[7] = 0.5f;
  bad += ics_op_tsne_prepare(h, init, N - 1, 2, sec) == 0;             /* init of the wrong shape */
  bad += ics_op_tsne_prepare(h, init, N, 3, sec) == 0;
  bad += ics_op_tsne_prepare(h, NULL, N, 2, sec) == 0;
  OK(ics_op_tsne_get_codes(h, codes, N));
  OK(ics_op_tsne_prepare(h, init, N, 2, sec));
  OK(ics_op_tsne_prepare(h, init, N, 2, NULL));                        /* again: the state is rebuilt */
  for (int r = 0; r < 8 && !done; ++r) OK(ics_op_tsne_run(h, 3, &done));
  OK(ics_op_tsne_read(h, emb, &kl, &gn, &n_iter, &count));
  OK(ics_op_tsne_read(h, NULL, NULL, NULL, NULL, NULL));
  OK(ics_op_tsne_gradient(h, init, 12.0, grad, &kl));
  bad += ics_op_tsne_gradient(h, init, 0.0, grad, &kl) == 0;
  {
    size_t nnz = 0;
    OK(ics_op_tsne_get_graph(h, NULL, NULL, NULL, 0, &nnz));
    int64_t* ip = (int64_t*)malloc((N + 1) * sizeof(int64_t));
    int32_t* ix = (int32_t*)malloc((nnz + 1) * sizeof(int32_t));
    double* vv = (double*)malloc((nnz + 1) * sizeof(double));
    OK(ics_op_tsne_get_graph(h, ip, ix, vv, nnz, &nnz));
    if (nnz > 0) bad += ics_op_tsne_get_graph(h, ip, ix, vv, nnz - 1, &nnz) == 0;
    for (size_t e = 0; e < nnz; ++e) vv[e] = 1.0 / (double)(nnz ? nnz : 1);
    OK(ics_op_tsne_set_graph(h, N, ip, ix, vv, init, N, 2));
    OK(ics_op_tsne_run(h, 5, &done));
    ip[0] = 1; bad += ics_op_tsne_set_graph(h, N, ip, ix, vv, init, N, 2) == 0; ip[0] = 0;
    if (nnz > 0) { ix[0] = N; bad += ics_op_tsne_set_graph(h, N, ip, ix, vv, init, N, 2) == 0; ix[0] = 0; }
    bad += ics_op_tsne_set_graph(h, N + 1, ip, ix, vv, init, N + 1, 2) == 0;
    bad += ics_op_tsne_set_graph(h, N, ip, ix, vv, init, N, 1) == 0;
    free(ip); free(ix); free(vv);
  }
  OK(ics_op_tsne_destroy(h));
  OK(ics_op_tsne_destroy(NULL));
  if (vae) {   /* encode -> append, device to device */
    static float z[3 * 8 * 256];
    ics_tsne_config cv = {256, 2 * 8, 2, 1.5, 12.0, 2, 4, 2, 300, 1e-7, 50.0};
    ics_tsne* hv = NULL;
    OK(ics_op_tsne_create(&cv, &hv));
    OK(ics_vae_encode(vae, x, cond, eps, B, z, z + 8 * 256, z + 16 * 256));
    OK(ics_op_tsne_append_vae(hv, vae, B));
    OK(ics_op_tsne_append_vae(hv, vae, 1));
    bad += ics_op_tsne_append_vae(hv, vae, B + 1) == 0;
    bad += ics_op_tsne_append_vae(hv, unet, 1) == 0;
    bad += ics_op_tsne_append_vae(NULL, vae, 1) == 0;
    bad += ics_op_tsne_append_vae(hv, NULL, 1) == 0;
    OK(ics_op_tsne_prepare(hv, init, B + 1, 2, sec));
    OK(ics_op_tsne_run(hv, 4, &done));
    OK(ics_op_tsne_destroy(hv));
    { ics_tsne_config c7 = cv; c7.dim = 7; OK(ics_op_tsne_create(&c7, &hv)); bad += ics_op_tsne_append_vae(hv, vae, 1) == 0; OK(ics_op_tsne_destroy(hv)); }
  }
  if (bad) { fprintf(stderr, "tsne: %d invalid calls accepted\n", bad); return 1; }
  return 0;
}

static int interp_walk(ics_net* unet, ics_net* vae, const ics_unet_config* uc, const float* x, const float* cond,
                       const float* eps, int B, int d, int C) {
  const int pairs = B, steps = 2, frames = pairs * steps;      /* max_batch B: groups of B / 2 pairs */
  const size_t vox = (size_t)d * d * d;
  double alpha[2] = {0.0, 1.25};
  float* z_ends = (float*)malloc((size_t)pairs * 2 * 256 * sizeof(float));
  float* z_path = (float*)malloc((size_t)frames * 256 * sizeof(float));
  float* rec = (float*)malloc(frames * vox * C * sizeof(float));
  uint8_t* sp = (uint8_t*)malloc(frames * vox);
  uint8_t* mk = (uint8_t*)malloc(frames * vox);
  float* dens = (float*)malloc(frames * vox * sizeof(float));
  float* minmax = (float*)malloc((size_t)frames * 6 * sizeof(float));
  int32_t* regions = (int32_t*)malloc(frames * vox * sizeof(int32_t));
  int32_t* counts = (int32_t*)malloc((size_t)frames * 2 * sizeof(int32_t));
  int32_t* stats = (int32_t*)malloc((size_t)frames * 16 * 11 * sizeof(int32_t));
  int64_t* bnd = (int64_t*)calloc((size_t)frames * 16 * 8, 8);
  float mv[4];
  int bad = 0;
  for (int mode = 0; mode < 2; ++mode) {
    OK(ics_vae_interpolate(vae, x, x, cond, eps, eps, pairs, alpha, steps, mode, z_ends, z_path, rec));
    OK(ics_vae_interpolate(vae, x, x, cond, eps, eps, 1, alpha, 1, mode, NULL, NULL, NULL));
    OK(ics_vae_interpolate_to_unet_atoms(vae, unet, x, x, cond, eps, eps, pairs, alpha, steps, mode, 0.8f, 3, 16, z_ends,
                                         z_path, sp, mk, dens, minmax, regions, counts, stats, bnd));
    OK(ics_vae_interpolate_to_unet_atoms(vae, unet, x, x, cond, eps, eps, pairs, alpha, steps, mode, 0.8f, 3, 16, NULL,
                                         NULL, NULL, NULL, NULL, NULL, NULL, counts, stats, NULL));
  }
  /* the chain cleared the resident batch */
  bad += ics_vae_train_step_resident(vae, mv) == 0;
  bad += ics_vae_interpolate(vae, x, x, cond, eps, eps, 0, alpha, steps, 0, z_ends, z_path, rec) == 0;
  bad += ics_vae_interpolate(vae, x, x, cond, eps, eps, pairs, alpha, 0, 0, z_ends, z_path, rec) == 0;
  bad += ics_vae_interpolate(vae, x, x, cond, eps, eps, pairs, alpha, steps, 7, z_ends, z_path, rec) == 0;
  bad += ics_vae_interpolate(vae, NULL, x, cond, eps, eps, pairs, alpha, steps, 0, z_ends, z_path, rec) == 0;
  bad += ics_vae_interpolate(vae, x, NULL, cond, eps, eps, pairs, alpha, steps, 0, z_ends, z_path, rec) == 0;
  bad += ics_vae_interpolate(vae, x, x, NULL, eps, eps, pairs, alpha, steps, 0, z_ends, z_path, rec) == 0;
  bad += ics_vae_interpolate(vae, x, x, cond, NULL, eps, pairs, alpha, steps, 0, z_ends, z_path, rec) == 0;
  bad += ics_vae_interpolate(vae, x, x, cond, eps, NULL, pairs, alpha, steps, 0, z_ends, z_path, rec) == 0;
  bad += ics_vae_interpolate(vae, x, x, cond, eps, eps, pairs, NULL, steps, 0, z_ends, z_path, rec) == 0;
  bad += ics_vae_interpolate(unet, x, x, cond, eps, eps, pairs, alpha, steps, 0, z_ends, z_path, rec) == 0;
  alpha[1] = NAN;
  bad += ics_vae_interpolate(vae, x, x, cond, eps, eps, pairs, alpha, steps, 0, z_ends, z_path, rec) == 0;
  alpha[1] = 1.25;
  {   /* steps above max_batch */
    double* many = (double*)calloc((size_t)B + 1, sizeof(double));
    bad += ics_vae_interpolate(vae, x, x, cond, eps, eps, 1, many, B + 1, 0, NULL, NULL, NULL) == 0;
    free(many);
  }
  bad += ics_vae_interpolate_to_unet_atoms(vae, unet, x, x, cond, eps, eps, pairs, alpha, steps, 0, 0.8f, 3, 16, NULL, NULL,
                                           NULL, NULL, NULL, NULL, NULL, NULL, stats, NULL) == 0;
  bad += ics_vae_interpolate_to_unet_atoms(vae, unet, x, x, cond, eps, eps, pairs, alpha, steps, 0, 0.8f, 3, 16, NULL, NULL,
                                           NULL, NULL, NULL, NULL, NULL, counts, NULL, NULL) == 0;
  bad += ics_vae_interpolate_to_unet_atoms(vae, unet, x, x, cond, eps, eps, pairs, alpha, steps, 0, 0.8f, 3, 0, NULL, NULL,
                                           NULL, NULL, NULL, NULL, NULL, counts, stats, NULL) == 0;
  bad += ics_vae_interpolate_to_unet_atoms(vae, vae, x, x, cond, eps, eps, pairs, alpha, steps, 0, 0.8f, 3, 16, NULL, NULL,
                                           NULL, NULL, NULL, NULL, NULL, counts, stats, NULL) == 0;
  {   /* a U-Net of other channels is refused; a smaller one only shortens the groups (steps above ITS max_batch: refused) */
    ics_unet_config u2 = *uc;
    ics_net* un2 = NULL;
    u2.in_channels = uc->in_channels == 1 ? 4 : 1;
    OK(ics_unet_create(&u2, &un2));
    bad += ics_vae_interpolate_to_unet_atoms(vae, un2, x, x, cond, eps, eps, pairs, alpha, steps, 0, 0.8f, 3, 16, NULL, NULL,
                                             NULL, NULL, NULL, NULL, NULL, counts, stats, NULL) == 0;
    OK(ics_net_destroy(un2));
    u2 = *uc; u2.max_batch = 1;
    OK(ics_unet_create(&u2, &un2));
    bad += ics_vae_interpolate_to_unet_atoms(vae, un2, x, x, cond, eps, eps, pairs, alpha, steps, 0, 0.8f, 3, 16, NULL, NULL,
                                             NULL, NULL, NULL, NULL, NULL, counts, stats, NULL) == 0;
    OK(ics_vae_interpolate_to_unet_atoms(vae, un2, x, x, cond, eps, eps, pairs, alpha, 1, 0, 0.8f, 3, 16, NULL, NULL, NULL,
                                         NULL, NULL, NULL, NULL, counts, stats, NULL));
    OK(ics_net_destroy(un2));
  }
  if (bad) { fprintf(stderr, "interpolate: %d invalid calls accepted\n", bad); return 1; }
  OK(ics_vae_interpolate(vae, x, x, cond, eps, eps, pairs, alpha, steps, 0, z_ends, z_path, rec));   /* still usable */
  OK(ics_vae_upload_batch(vae, x, cond, eps, B));          /* a resident batch again for what follows */
  OK(ics_vae_train_step_resident(vae, mv));
  free(z_ends); free(z_path); free(rec); free(sp); free(mk); free(dens); free(minmax); free(regions); free(counts);
  free(stats); free(bnd);
  return 0;
}

/* Per-class loss weights: set / get / unset around every kind of step, the refusals, and the table through a state
 * broadcast; the label histogram on buffers of the exact size (every id kind, lengths that are no multiple of a
 * 16-byte load, the empty array) and its refusals. */
static int class_weight_walk(ics_net* unet, ics_net* vae, int ncls, const float* x, const uint8_t* lab, int B, int with_comm) {
  float* w = (float*)malloc((size_t)ncls * sizeof(float));
  float* back = (float*)malloc((size_t)ncls * sizeof(float));
  float mm[5];
  int active = -1, bad = 0;
  for (int c = 0; c < ncls; ++c) w[c] = c == 0 ? 0.f : 0.25f + (float)(c % 7);
  OK(ics_unet_get_class_weights(unet, back, ncls, &active));
  if (active != 0) { fprintf(stderr, "class weights: active before any set\n"); return 1; }
  OK(ics_unet_set_class_weights(unet, w, ncls));
  OK(ics_unet_get_class_weights(unet, back, ncls, &active));
  OK(ics_unet_get_class_weights(unet, NULL, 0, NULL));
  if (active != 1 || memcmp(w, back, (size_t)ncls * sizeof(float)) != 0) { fprintf(stderr, "class weights: table not returned\n"); return 1; }
  OK(ics_unet_train_step(unet, x, lab, B, mm));
  OK(ics_unet_test_step(unet, x, lab, B, mm));
  OK(ics_unet_upload_batch(unet, x, lab, B));
  OK(ics_unet_train_step_resident(unet, mm));
  if (with_comm) {
    OK(ics_net_comm_broadcast_state(unet, 0));
    OK(ics_unet_get_class_weights(unet, back, ncls, &active));
    if (active != 1 || memcmp(w, back, (size_t)ncls * sizeof(float)) != 0) { fprintf(stderr, "class weights: lost in the broadcast\n"); return 1; }
  }
  bad += ics_unet_set_class_weights(NULL, w, ncls) == 0;
  bad += ics_unet_set_class_weights(vae, w, ncls) == 0;
  bad += ics_unet_set_class_weights(unet, w, ncls - 1) == 0;
  bad += ics_unet_set_class_weights(unet, w, ncls + 1) == 0;
  w[1] = -1.f; bad += ics_unet_set_class_weights(unet, w, ncls) == 0;
  w[1] = NAN; bad += ics_unet_set_class_weights(unet, w, ncls) == 0;
  w[1] = INFINITY; bad += ics_unet_set_class_weights(unet, w, ncls) == 0;
  w[1] = 1.f;
  bad += ics_unet_get_class_weights(NULL, back, ncls, &active) == 0;
  bad += ics_unet_get_class_weights(vae, back, ncls, &active) == 0;
  bad += ics_unet_get_class_weights(unet, back, ncls - 1, &active) == 0;
  if (bad) { fprintf(stderr, "class weights: %d invalid argument sets accepted\n", bad); return 1; }
  OK(ics_unet_get_class_weights(unet, back, ncls, &active));      /* a refused set leaves the table in force */
  if (active != 1) { fprintf(stderr, "class weights: a refused set cleared the table\n"); return 1; }
  OK(ics_unet_set_class_weights(unet, NULL, 0));
  OK(ics_unet_get_class_weights(unet, back, ncls, &active));
  if (active != 0) { fprintf(stderr, "class weights: still active after NULL\n"); return 1; }
  OK(ics_unet_train_step(unet, x, lab, B, mm));
  free(w); free(back);
  return 0;
}
static int label_counts_walk(void) {
  const size_t ns[6] = {0, 1, 15, 16, 1037, 4099};
  const int cols[3] = {2, 95, 127};
  int bad = 0;
  for (int kind = 1; kind <= 3; ++kind)
    for (int i = 0; i < 6; ++i) {
      const size_t n = ns[i], lb = kind == 1 ? 1 : kind == 2 ? 8 : 4;
      const int ncls = cols[(kind + i) % 3];
      void* lab = n ? calloc(n, lb) : NULL;
      int64_t* counts = (int64_t*)malloc((size_t)ncls * sizeof(int64_t));
      int64_t oor = -1;
      OK(ics_op_label_counts(lab, kind, n, ncls, counts, &oor));
      free(lab); free(counts);
    }
  float lab[16] = {0};
  int64_t counts[127], oor;
  bad += ics_op_label_counts(lab, 4, 16, 95, counts, &oor) == 0;      /* one-hot: no class ids */
  bad += ics_op_label_counts(lab, 0, 16, 95, counts, &oor) == 0;
  bad += ics_op_label_counts(lab, 5, 16, 95, counts, &oor) == 0;
  bad += ics_op_label_counts(NULL, 3, 16, 95, counts, &oor) == 0;
  bad += ics_op_label_counts(lab, 3, 16, 95, NULL, &oor) == 0;
  bad += ics_op_label_counts(lab, 3, 16, 95, counts, NULL) == 0;
  bad += ics_op_label_counts(lab, 3, 16, 1, counts, &oor) == 0;
  bad += ics_op_label_counts(lab, 3, 16, 128, counts, &oor) == 0;
  if (bad) { fprintf(stderr, "label counts: %d invalid argument sets accepted\n", bad); return 1; }
  OK(ics_op_label_counts(lab, 3, 16, 95, counts, &oor));
  return 0;
}

/* The confusion matrix: the op on buffers of the exact size (every id kind, lengths that are no multiple of a 16-byte
 * load, the empty array, with and without a mask) and its refusals with guarded outputs; then the engine's accumulator --
 * every entry point before open, open / batch / step / read twice / reset / re-open, a resident batch without labels, a
 * VAE handle, null arguments -- after which the engine still trains. */
static int confusion_walk(ics_net* unet, ics_net* vae, int ncls, int d, const float* x, const uint8_t* lab, int B) {
  const size_t ns[6] = {0, 1, 15, 16, 1037, 4099};
  const int cols[3] = {2, 95, 127};
  int bad = 0, a = 0, b = 0, c = 0;
  OK(ics_op_confusion_grid(&a, &b, &c));
  bad += ics_op_confusion_grid(NULL, &b, &c) == 0;
  for (int kind = 1; kind <= 3; ++kind)
    for (int i = 0; i < 6; ++i) {
      const size_t n = ns[i], lb = kind == 1 ? 1 : kind == 2 ? 8 : 4;
      const int k = cols[(kind + i) % 3];
      void* t = n ? calloc(n, lb) : NULL;
      uint8_t *p = n ? calloc(n, 1) : NULL, *m = n ? calloc(n, 1) : NULL;
      int64_t* mat = (int64_t*)malloc((size_t)k * k * sizeof(int64_t));
      int64_t occ[4], oor = -1;
      OK(ics_op_confusion(t, kind, p, n ? m : (const uint8_t*)"", n, k, mat, occ, &oor));
      OK(ics_op_confusion(t, kind, p, NULL, n, k, mat, NULL, &oor));
      free(t); free(p); free(m); free(mat);
    }
  {
    float t[16] = {0};
    uint8_t p[16] = {0}, m[16] = {0};
    int64_t mat[95 * 95], occ[4], oor;
    bad += ics_op_confusion(t, 4, p, m, 16, 95, mat, occ, &oor) == 0;      /* one-hot: no class ids */
    bad += ics_op_confusion(t, 0, p, m, 16, 95, mat, occ, &oor) == 0;
    bad += ics_op_confusion(t, 5, p, m, 16, 95, mat, occ, &oor) == 0;
    bad += ics_op_confusion(NULL, 3, p, m, 16, 95, mat, occ, &oor) == 0;
    bad += ics_op_confusion(t, 3, NULL, m, 16, 95, mat, occ, &oor) == 0;
    bad += ics_op_confusion(t, 3, p, m, 16, 95, NULL, occ, &oor) == 0;
    bad += ics_op_confusion(t, 3, p, m, 16, 95, mat, occ, NULL) == 0;
    bad += ics_op_confusion(t, 3, p, m, 16, 95, mat, NULL, &oor) == 0;     /* a mask without a table, a table without a mask */
    bad += ics_op_confusion(t, 3, p, NULL, 16, 95, mat, occ, &oor) == 0;
    bad += ics_op_confusion(t, 3, p, m, 16, 1, mat, occ, &oor) == 0;
    bad += ics_op_confusion(t, 3, p, m, 16, 128, mat, occ, &oor) == 0;
    bad += ics_op_confusion((const char*)t + 2, 3, p, m, 15, 95, mat, occ, &oor) == 0;   /* unaligned float labels */
    OK(ics_op_confusion(t, 3, p, m, 16, 95, mat, occ, &oor));
  }
  const size_t kk = (size_t)ncls * ncls;
  int64_t* mat = (int64_t*)malloc(kk * sizeof(int64_t));
  int64_t occ[4], oor = 0, vox = 0;
  float mm[5];
  bad += ics_unet_confusion_step(unet, 0.8f) == 0;                        /* before open */
  bad += ics_unet_confusion_batch(unet, x, lab, B, 0.8f) == 0;
  bad += ics_unet_confusion_read(unet, mat, occ, &oor, &vox) == 0;
  bad += ics_unet_confusion_reset(unet) == 0;
  OK(ics_unet_confusion_open(unet));
  OK(ics_unet_confusion_batch(unet, x, lab, B, 0.8f));
  OK(ics_unet_confusion_batch(unet, x, lab, 1, 0.8f));
  OK(ics_unet_upload_batch(unet, x, lab, B));
  OK(ics_unet_confusion_step(unet, 0.8f));
  {
    float* img = calloc((size_t)B * d * d * 4, 4);
    float lut[256 * 3] = {0};
    OK(ics_unet_render_slice_resident(unet, 1, 0, B, 2, d / 2, lut, NULL, 1, img));   /* the species are where a labels predict leaves them */
    free(img);
  }
  OK(ics_unet_confusion_read(unet, mat, occ, &oor, &vox));
  OK(ics_unet_confusion_read(unet, mat, occ, &oor, &vox));
  if (vox != (int64_t)(2 * B + 1) * d * d * d) { fprintf(stderr, "confusion: %lld voxels counted\n", (long long)vox); return 1; }
  OK(ics_unet_confusion_reset(unet));
  OK(ics_unet_confusion_read(unet, mat, occ, &oor, &vox));
  if (vox != 0) { fprintf(stderr, "confusion: voxels left after a reset\n"); return 1; }
  OK(ics_unet_confusion_open(unet));                                        /* a second open: the same buffer, zeroed */
  OK(ics_unet_upload_batch(unet, x, NULL, B));                              /* a resident batch without labels */
  bad += ics_unet_confusion_step(unet, 0.8f) == 0;
  bad += ics_unet_confusion_batch(unet, NULL, lab, B, 0.8f) == 0;
  bad += ics_unet_confusion_batch(unet, x, NULL, B, 0.8f) == 0;
  bad += ics_unet_confusion_batch(unet, x, lab, 0, 0.8f) == 0;
  bad += ics_unet_confusion_batch(unet, x, lab, B + 100, 0.8f) == 0;
  bad += ics_unet_confusion_read(unet, NULL, occ, &oor, &vox) == 0;
  bad += ics_unet_confusion_read(unet, mat, NULL, &oor, &vox) == 0;
  bad += ics_unet_confusion_read(unet, mat, occ, NULL, &vox) == 0;
  bad += ics_unet_confusion_read(unet, mat, occ, &oor, NULL) == 0;
  bad += ics_unet_confusion_open(NULL) == 0;
  bad += ics_unet_confusion_open(vae) == 0;
  bad += ics_unet_confusion_reset(vae) == 0;
  bad += ics_unet_confusion_step(vae, 0.8f) == 0;
  bad += ics_unet_confusion_batch(vae, x, lab, B, 0.8f) == 0;
  bad += ics_unet_confusion_read(vae, mat, occ, &oor, &vox) == 0;
  if (bad) { fprintf(stderr, "confusion: %d invalid calls accepted\n", bad); return 1; }
  OK(ics_unet_confusion_batch(unet, x, lab, B, 0.8f));                      /* still usable */
  OK(ics_unet_confusion_read(unet, mat, occ, &oor, &vox));
  OK(ics_unet_train_step(unet, x, lab, B, mm));
  free(mat);
  return 0;
}

/* The atom score: the ragged op on buffers of the exact size (empty sets, the largest set, a batch that takes several
 * launches, with and without the per-sample outputs) and each of its refusals with guarded outputs; the volumes op on a
 * small and a regular grid; then the engine's accumulator -- every entry point before open, open / batch / step / read
 * twice / reset / re-open, with and without the confusion accumulator, null arguments, a VAE handle -- after which the
 * engine still trains.  Runs after confusion_walk, which leaves a confusion accumulator open. */
static int atom_score_walk(ics_net* unet, ics_net* vae, int ncls, int d, const float* x, const uint8_t* lab, int B) {
  int bad = 0, a = 0, b = 0, c = 0, e = 0;
  OK(ics_op_atom_score_limits(&a, &b, &c, &e));
  bad += ics_op_atom_score_limits(&a, NULL, &c, &e) == 0;
  const size_t KK = 128 * 128;
  int64_t* mat = (int64_t*)malloc(KK * sizeof(int64_t));
  int64_t dq[127], d2q[127], dup[127], sh[127], hist[16], tot[8];
  {
    /* 40 samples: sample 0 empty on both sides, sample 1 of 1024 x 1024 atoms, the rest 900 x 800: several launches */
    const int nb = 40;
    int32_t *to = (int32_t*)malloc((nb + 1) * sizeof(int32_t)), *po = (int32_t*)malloc((nb + 1) * sizeof(int32_t));
    to[0] = po[0] = 0;
    for (int s = 0; s < nb; ++s) {
      to[s + 1] = to[s] + (s == 0 ? 0 : s == 1 ? 1024 : 900);
      po[s + 1] = po[s] + (s == 0 ? 0 : s == 1 ? 1024 : 800);
    }
    const size_t nt = (size_t)to[nb], np = (size_t)po[nb];
    double *tx = (double*)calloc(3 * nt, sizeof(double)), *px = (double*)calloc(3 * np, sizeof(double));
    int32_t *ts = (int32_t*)calloc(nt, sizeof(int32_t)), *ps = (int32_t*)calloc(np, sizeof(int32_t));
    int32_t *match = (int32_t*)malloc(nt * sizeof(int32_t)), *st = (int32_t*)malloc((size_t)nb * 6 * sizeof(int32_t));
    double* ds = (double*)malloc(nb * sizeof(double));
    OK(ics_op_atom_score(tx, ts, to, px, ps, po, nb, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds));
    OK(ics_op_atom_score(tx, ts, to, px, ps, po, nb, 127, 2.0, mat, dq, d2q, dup, sh, hist, tot, NULL, NULL, NULL));
    OK(ics_op_atom_score(tx, ts, to, px, ps, po, 1, 2, 0.5, mat, dq, d2q, dup, sh, hist, tot, match, NULL, ds));   /* one empty sample */
    OK(ics_op_atom_score(NULL, NULL, to, NULL, NULL, po, 1, 2, 0.5, mat, dq, d2q, dup, sh, hist, tot, NULL, NULL, NULL));
    bad += ics_op_atom_score(tx, ts, NULL, px, ps, po, nb, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    bad += ics_op_atom_score(tx, ts, to, px, ps, NULL, nb, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    bad += ics_op_atom_score(NULL, ts, to, px, ps, po, nb, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    bad += ics_op_atom_score(tx, ts, to, px, NULL, po, nb, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    bad += ics_op_atom_score(tx, ts, to, px, ps, po, nb, 17, 2.0, NULL, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    bad += ics_op_atom_score(tx, ts, to, px, ps, po, nb, 17, 2.0, mat, dq, d2q, dup, sh, hist, NULL, match, st, ds) == 0;
    bad += ics_op_atom_score(tx, ts, to, px, ps, po, 0, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    bad += ics_op_atom_score(tx, ts, to, px, ps, po, nb, 1, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    bad += ics_op_atom_score(tx, ts, to, px, ps, po, nb, 128, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    bad += ics_op_atom_score(tx, ts, to, px, ps, po, nb, 17, 0.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    bad += ics_op_atom_score(tx, ts, to, px, ps, po, nb, 17, __builtin_inf(), mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    to[0] = 1;
    bad += ics_op_atom_score(tx, ts, to, px, ps, po, nb, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    to[0] = 0; po[3] = po[2] - 1;
    bad += ics_op_atom_score(tx, ts, to, px, ps, po, nb, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    po[3] = po[2] + 800; po[2] += 1;                              /* sample 1 of 1025 predicted atoms */
    bad += ics_op_atom_score(tx, ts, to, px, ps, po, nb, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    po[2] -= 1; ts[nt - 1] = 17;
    bad += ics_op_atom_score(tx, ts, to, px, ps, po, nb, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    ts[nt - 1] = 0; ps[0] = -1;
    bad += ics_op_atom_score(tx, ts, to, px, ps, po, nb, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    ps[0] = 0; px[3 * np - 1] = __builtin_nan("");
    bad += ics_op_atom_score(tx, ts, to, px, ps, po, nb, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    px[3 * np - 1] = 0; tx[0] = 2e150;
    bad += ics_op_atom_score(tx, ts, to, px, ps, po, nb, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    tx[0] = 0;
    OK(ics_op_atom_score(tx, ts, to, px, ps, po, nb, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds));
    free(to); free(po); free(tx); free(px); free(ts); free(ps); free(match); free(st); free(ds);
  }
  for (int dv = 8; dv <= 16; dv += 8) {      /* a grid below the segmentation's 16 is padded on the host */
    const size_t vox = (size_t)3 * dv * dv * dv;
    uint8_t *l = (uint8_t*)calloc(vox, 1), *s = (uint8_t*)calloc(vox, 1), *m = (uint8_t*)calloc(vox, 1);
    int32_t *match = (int32_t*)malloc(3 * 5 * sizeof(int32_t)), st[3 * 6];
    double ds[3];
    OK(ics_op_atom_score_volumes(l, s, m, 3, dv, 3, 5, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds));
    OK(ics_op_atom_score_volumes(l, s, m, 3, dv, 0, 1024, 127, 2.0, mat, dq, d2q, dup, sh, hist, tot, NULL, NULL, NULL));
    bad += ics_op_atom_score_volumes(NULL, s, m, 3, dv, 3, 5, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    bad += ics_op_atom_score_volumes(l, s, NULL, 3, dv, 3, 5, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    bad += ics_op_atom_score_volumes(l, s, m, 3, dv, 3, 5, 17, 2.0, mat, dq, NULL, dup, sh, hist, tot, match, st, ds) == 0;
    bad += ics_op_atom_score_volumes(l, s, m, 0, dv, 3, 5, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    bad += ics_op_atom_score_volumes(l, s, m, 3, dv + 4, 3, 5, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    bad += ics_op_atom_score_volumes(l, s, m, 3, dv, -1, 5, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    bad += ics_op_atom_score_volumes(l, s, m, 3, dv, 3, 0, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    bad += ics_op_atom_score_volumes(l, s, m, 3, dv, 3, 1025, 17, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    bad += ics_op_atom_score_volumes(l, s, m, 3, dv, 3, 5, 128, 2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    bad += ics_op_atom_score_volumes(l, s, m, 3, dv, 3, 5, 17, -2.0, mat, dq, d2q, dup, sh, hist, tot, match, st, ds) == 0;
    free(l); free(s); free(m); free(match);
  }
  if (bad) { fprintf(stderr, "atom score ops: %d invalid calls accepted\n", bad); return 1; }
  (void)ncls;
  float mm[5];
  bad += ics_unet_atom_score_step(unet, 0.8f, 0) == 0;                       /* before open */
  bad += ics_unet_atom_score_batch(unet, x, lab, B, 0.8f, 0) == 0;
  bad += ics_unet_atom_score_read(unet, mat, dq, d2q, dup, sh, hist, tot) == 0;
  bad += ics_unet_atom_score_reset(unet) == 0;
  bad += ics_unet_atom_score_open(unet, 0.0, 3, 64) == 0;
  bad += ics_unet_atom_score_open(unet, 2.0, -1, 64) == 0;
  bad += ics_unet_atom_score_open(unet, 2.0, 3, 0) == 0;
  bad += ics_unet_atom_score_open(unet, 2.0, 3, 1025) == 0;
  bad += ics_unet_atom_score_read(unet, mat, dq, d2q, dup, sh, hist, tot) == 0;   /* a refused open opened nothing */
  OK(ics_unet_atom_score_open(unet, 2.0, 3, 64));
  OK(ics_unet_atom_score_batch(unet, x, lab, B, 0.8f, 0));
  OK(ics_unet_atom_score_batch(unet, x, lab, 1, 0.8f, 1));                   /* confusion_walk left its accumulator open */
  OK(ics_unet_upload_batch(unet, x, lab, B));
  OK(ics_unet_atom_score_step(unet, 0.8f, 1));
  {
    float* img = calloc((size_t)B * d * d * 4, 4);
    float lut[256 * 3] = {0};
    OK(ics_unet_render_slice_resident(unet, 1, 0, B, 2, d / 2, lut, NULL, 1, img));   /* the species are where a labels predict leaves them */
    free(img);
  }
  OK(ics_unet_atom_score_read(unet, mat, dq, d2q, dup, sh, hist, tot));
  OK(ics_unet_atom_score_read(unet, mat, dq, d2q, dup, sh, hist, tot));
  OK(ics_unet_atom_score_reset(unet));
  OK(ics_unet_atom_score_open(unet, 1.5, 0, 64));                            /* a second open: new tol and min_voxels */
  bad += ics_unet_atom_score_open(unet, 1.5, 0, 65) == 0;                    /* ... but not another max_atoms */
  bad += ics_unet_atom_score_step(unet, 0.8f, 2) == 0;
  OK(ics_unet_upload_batch(unet, x, NULL, B));                               /* a resident batch without labels */
  bad += ics_unet_atom_score_step(unet, 0.8f, 0) == 0;
  bad += ics_unet_atom_score_batch(unet, NULL, lab, B, 0.8f, 0) == 0;
  bad += ics_unet_atom_score_batch(unet, x, NULL, B, 0.8f, 0) == 0;
  bad += ics_unet_atom_score_batch(unet, x, lab, 0, 0.8f, 0) == 0;
  bad += ics_unet_atom_score_batch(unet, x, lab, B + 100, 0.8f, 0) == 0;
  bad += ics_unet_atom_score_read(unet, NULL, dq, d2q, dup, sh, hist, tot) == 0;
  bad += ics_unet_atom_score_read(unet, mat, dq, d2q, dup, sh, NULL, tot) == 0;
  bad += ics_unet_atom_score_read(unet, mat, dq, d2q, dup, sh, hist, NULL) == 0;
  bad += ics_unet_atom_score_open(NULL, 2.0, 3, 64) == 0;
  bad += ics_unet_atom_score_open(vae, 2.0, 3, 64) == 0;
  bad += ics_unet_atom_score_reset(vae) == 0;
  bad += ics_unet_atom_score_step(vae, 0.8f, 0) == 0;
  bad += ics_unet_atom_score_batch(vae, x, lab, B, 0.8f, 0) == 0;
  bad += ics_unet_atom_score_read(vae, mat, dq, d2q, dup, sh, hist, tot) == 0;
  if (bad) { fprintf(stderr, "atom score accumulator: %d invalid calls accepted\n", bad); return 1; }
  OK(ics_unet_atom_score_batch(unet, x, lab, B, 0.8f, 1));                   /* still usable */
  OK(ics_unet_atom_score_read(unet, mat, dq, d2q, dup, sh, hist, tot));
  OK(ics_unet_train_step(unet, x, lab, B, mm));
  free(mat);
  return 0;
}

/* Fed steps: the pack op alone on buffers of the exact size (every dtype mix, every label kind, odd column counts), then the
 * whole feed on both engines -- open, slot, submit, fed train / test step, metrics (late and twice), close, re-open with
 * another layout -- and every refusal, after which the feed and the engine still work. */
static int feed_walk(ics_net* unet, ics_net* vae, int d, int C, int B, int ncond, int latent) {
  const size_t V = (size_t)d * d * d;
  int bad = 0;
  if (d >= 8) {   /* ics_op_feed_pack */
    const int dts[2] = {0, 3}, cols[3] = {2, 95, 127};
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b)
        for (int kind = 0; kind <= 4; ++kind)
          for (int parts = 1; parts <= 2; ++parts) {
            const int ncls = cols[(a + b + kind) % 3], nb = 1 + (a + kind) % 2;
            ics_feed_config fc = {2, parts, {parts == 1 ? 4 : 1, 3}, {dts[a], dts[b]}, kind};
            const size_t vox = (size_t)nb * V, lb = kind == 1 ? 1 : kind == 2 ? 8 : kind == 3 ? 4 : kind == 4 ? (size_t)ncls * 4 : 0;
            void* x0 = calloc(vox * fc.x_channels[0], a ? 8 : 4);
            void* x1 = parts == 2 ? calloc(vox * 3, b ? 8 : 4) : NULL;
            void* lab = lb ? calloc(vox, lb) : NULL;
            float* out = (float*)malloc(vox * 4 * sizeof(float));
            uint8_t* lo = lb ? (uint8_t*)malloc(vox) : NULL;
            OK(ics_op_feed_pack(&fc, x0, x1, lab, nb, d, ncls, out, lo));
            free(x0); free(x1); free(lab); free(out); free(lo);
          }
    ics_feed_config fc = {2, 2, {1, 3}, {3, 3}, 4};
    double* x0 = (double*)calloc(V, 8); double* x1 = (double*)calloc(V * 3, 8);
    float* lab = (float*)calloc(V * 95, 4); float* out = (float*)malloc(V * 16); uint8_t* lo = (uint8_t*)malloc(V);
    ics_feed_config t = fc;
    bad += ics_op_feed_pack(NULL, x0, x1, lab, 1, d, 95, out, lo) == 0;
    bad += ics_op_feed_pack(&fc, NULL, x1, lab, 1, d, 95, out, lo) == 0;
    bad += ics_op_feed_pack(&fc, x0, NULL, lab, 1, d, 95, out, lo) == 0;
    bad += ics_op_feed_pack(&fc, x0, x1, NULL, 1, d, 95, out, lo) == 0;
    bad += ics_op_feed_pack(&fc, x0, x1, lab, 1, d, 95, NULL, lo) == 0;
    bad += ics_op_feed_pack(&fc, x0, x1, lab, 1, d, 95, out, NULL) == 0;
    bad += ics_op_feed_pack(&fc, x0, x1, lab, 0, d, 95, out, lo) == 0;
    bad += ics_op_feed_pack(&fc, x0, x1, lab, 1, 12, 95, out, lo) == 0;
    bad += ics_op_feed_pack(&fc, x0, x1, lab, 1, 4, 95, out, lo) == 0;
    bad += ics_op_feed_pack(&fc, x0, x1, lab, 1, d, 1, out, lo) == 0;
    bad += ics_op_feed_pack(&fc, x0, x1, lab, 1, d, 128, out, lo) == 0;
    t.x_parts = 3; bad += ics_op_feed_pack(&t, x0, x1, lab, 1, d, 95, out, lo) == 0; t = fc;
    t.x_channels[1] = 0; bad += ics_op_feed_pack(&t, x0, x1, lab, 1, d, 95, out, lo) == 0; t = fc;
    t.x_dtype[0] = 1; bad += ics_op_feed_pack(&t, x0, x1, lab, 1, d, 95, out, lo) == 0; t = fc;
    t.label_kind = 5; bad += ics_op_feed_pack(&t, x0, x1, lab, 1, d, 95, out, lo) == 0; t = fc;
    if (bad) { fprintf(stderr, "feed pack: %d invalid argument sets accepted\n", bad); return 1; }
    OK(ics_op_feed_pack(&fc, x0, x1, lab, 1, d, 95, out, lo));
    /* ics_op_feed_pack_rot: all 64 tables, no table, an entry on either side of -1..2 */
    int32_t rt[3];
    for (int c = 0; c < 64; ++c) {
      rt[0] = c / 16 - 1; rt[1] = c / 4 % 4 - 1; rt[2] = c % 4 - 1;
      OK(ics_op_feed_pack_rot(&fc, x0, x1, lab, rt, 1, d, 95, out, lo));
    }
    OK(ics_op_feed_pack_rot(&fc, x0, x1, lab, NULL, 1, d, 95, out, lo));
    rt[1] = 3; bad += ics_op_feed_pack_rot(&fc, x0, x1, lab, rt, 1, d, 95, out, lo) == 0;
    rt[1] = -2; bad += ics_op_feed_pack_rot(&fc, x0, x1, lab, rt, 1, d, 95, out, lo) == 0;
    rt[1] = 0; bad += ics_op_feed_pack_rot(NULL, x0, x1, lab, rt, 1, d, 95, out, lo) == 0;
    bad += ics_op_feed_pack_rot(&fc, x0, x1, lab, rt, 1, 12, 95, out, lo) == 0;
    if (bad || !strstr(ics_last_error(), "ics_op_feed_pack_rot")) { fprintf(stderr, "feed pack rot: %d invalid argument sets accepted\n", bad); return 1; }
    rt[1] = 3;
    if (ics_op_feed_pack_rot(&fc, x0, x1, lab, rt, 1, d, 95, out, lo) == 0 || !strstr(ics_last_error(), "rotation index 3")) {
      fprintf(stderr, "feed pack rot: the refusal does not name the rotation index\n"); return 1;
    }
    free(x0); free(x1); free(lab); free(out); free(lo);
  }
  int32_t* rot = (int32_t*)malloc((size_t)B * 3 * sizeof(int32_t));   /* exactly max_batch rows */
  for (int kind = 0; kind < 2; ++kind) {
    ics_net* net = kind ? vae : unet;
    for (int lay = 0; lay < 3; ++lay) {   /* raw files (float64 parts, float64 ids); one float32 part; one-hot labels */
      ics_feed_config fc = {2 + lay, 1, {C, 0}, {lay == 1 ? 0 : 3, 0}, kind ? 0 : (lay == 0 ? 2 : lay == 1 ? 1 : 4)};
      if (lay == 0 && C == 4) { fc.x_parts = 2; fc.x_channels[0] = 1; fc.x_channels[1] = 3; fc.x_dtype[1] = 3; }
      OK(ics_net_feed_open(net, &fc));
      void *x0, *x1, *lab; float *cond, *eps, m[5];
      int ticket[8], nt = 0;
      for (int step = 0; step < 6; ++step) {
        const int slot = step % fc.slots, b = 1 + step % B;
        OK(ics_net_feed_slot(net, slot, &x0, &x1, &lab, &cond, &eps));
        /* the last byte of every part a batch of max_batch samples uses: the slot's layout must hold them */
        const size_t e0 = fc.x_dtype[0] ? 8 : 4;
        memset(x0, 0, (size_t)B * V * fc.x_channels[0] * e0);
        if (fc.x_parts == 2) memset(x1, 0, (size_t)B * V * 3 * 8); else if (x1) { fprintf(stderr, "feed: x1 of a one-part feed\n"); return 1; }
        if (kind == 0) memset(lab, 0, (size_t)B * V * (fc.label_kind == 2 ? 8 : fc.label_kind == 1 ? 1 : 95 * 4));
        else { if (lab) { fprintf(stderr, "feed: labels of a VAE feed\n"); return 1; } memset(cond, 0, (size_t)B * ncond * sizeof(float)); memset(eps, 0, (size_t)B * latent * sizeof(float)); }
        for (int i = 0; i < b * 3; ++i) rot[i] = step == 4 ? -1 : (i + step + lay) % 4 - 1;
        if (step % 2 == 0) OK(ics_net_feed_submit_rot(net, slot, b, step == 2 ? NULL : rot));   /* a table, none, all -1 */
        else OK(ics_net_feed_submit(net, slot, b));                                              /* plain, after a table */
        if (kind == 0) OK(step == 3 ? ics_unet_test_step_fed(net, slot, &ticket[nt]) : ics_unet_train_step_fed(net, slot, &ticket[nt]));
        else OK(step == 3 ? ics_vae_test_step_fed(net, slot, &ticket[nt]) : ics_vae_train_step_fed(net, slot, &ticket[nt]));
        ++nt;
        if (step >= 2) OK(ics_net_feed_metrics(net, ticket[step - 2], m));     /* two steps late */
      }
      OK(ics_net_feed_metrics(net, ticket[nt - 1], m));
      OK(ics_net_feed_metrics(net, ticket[0], m));                             /* again */
      /* refusals */
      bad = 0;
      int tk = -1;
      bad += ics_net_feed_open(net, &fc) == 0;                                 /* already open */
      bad += ics_net_feed_slot(net, -1, &x0, &x1, &lab, &cond, &eps) == 0;
      bad += ics_net_feed_slot(net, fc.slots, &x0, &x1, &lab, &cond, &eps) == 0;
      bad += ics_net_feed_submit(net, fc.slots, 1) == 0;
      bad += ics_net_feed_submit(net, 1, 1) == 0;                              /* not obtained since its last submit */
      OK(ics_net_feed_slot(net, 1, NULL, NULL, NULL, NULL, NULL));
      bad += ics_net_feed_submit(net, 1, B + 1) == 0;
      bad += ics_net_feed_submit(net, 1, 0) == 0;
      bad += (kind ? ics_vae_train_step_fed(net, 1, &tk) : ics_unet_train_step_fed(net, 1, &tk)) == 0;   /* consumed */
      bad += (kind ? ics_vae_train_step_fed(net, 9, &tk) : ics_unet_train_step_fed(net, 9, &tk)) == 0;
      bad += (kind ? ics_unet_train_step_fed(net, 1, &tk) : ics_vae_train_step_fed(net, 1, &tk)) == 0;   /* wrong kind */
      bad += (kind ? ics_unet_test_step_fed(net, 1, &tk) : ics_vae_test_step_fed(net, 1, &tk)) == 0;
      bad += (kind ? ics_vae_test_step_fed(net, 1, NULL) : ics_unet_test_step_fed(net, 1, NULL)) == 0;
      for (int i = 0; i < B * 3; ++i) rot[i] = i % 4 - 1;
      bad += ics_net_feed_submit_rot(net, 1, B + 1, rot) == 0;
      rot[B * 3 - 1] = 3; bad += ics_net_feed_submit_rot(net, 1, B, rot) == 0;
      if (!strstr(ics_last_error(), "rotation index 3")) { fprintf(stderr, "feed: the refusal does not name the rotation index\n"); return 1; }
      rot[B * 3 - 1] = -2; bad += ics_net_feed_submit_rot(net, 1, B, rot) == 0;
      rot[B * 3 - 1] = 2;
      bad += ics_net_feed_submit_rot(net, fc.slots, B, rot) == 0;
      OK(ics_net_feed_submit_rot(net, 1, B, rot));                             /* the refused tables left the slot obtained */
      bad += ics_net_feed_submit_rot(net, 1, B, rot) == 0;                     /* pending */
      bad += ics_net_feed_submit(net, 1, B) == 0;
      bad += ics_net_feed_metrics(net, nt, m) == 0;
      bad += ics_net_feed_metrics(net, -1, m) == 0;
      bad += ics_net_feed_metrics(net, 0, NULL) == 0;
      if (bad) { fprintf(stderr, "feed (kind %d, layout %d): %d invalid calls accepted\n", kind, lay, bad); return 1; }
      if (!ics_last_error()[0]) { fprintf(stderr, "feed: no error message\n"); return 1; }
      OK(kind ? ics_vae_train_step_fed(net, 1, &tk) : ics_unet_train_step_fed(net, 1, &tk));   /* still usable */
      OK(ics_net_feed_metrics(net, tk, m));
      if (lay == 2) {   /* a ticket older than the ring */
        for (int step = 0; step < 70; ++step) {
          OK(ics_net_feed_slot(net, 0, NULL, NULL, NULL, NULL, NULL));
          OK(ics_net_feed_submit(net, 0, 1));
          OK(kind ? ics_vae_test_step_fed(net, 0, &tk) : ics_unet_test_step_fed(net, 0, &tk));
        }
        if (ics_net_feed_metrics(net, ticket[0], m) == 0) { fprintf(stderr, "feed: a ticket older than the ring was read\n"); return 1; }
        OK(ics_net_feed_metrics(net, tk, m));
        /* left open: ics_net_destroy closes it */
      } else {
        OK(ics_net_feed_close(net));
      }
    }
  }
  {   /* engines without a feed, and configs that do not match the engine */
    ics_net* u2 = NULL;
    ics_unet_config uc = {C, 95, d, B, 1e-3f, 0.f, 1, 1, 0};
    OK(ics_unet_create(&uc, &u2));
    ics_feed_config fc = {2, 1, {C, 0}, {0, 0}, 1}, t = fc;
    float m[5]; int tk;
    bad = 0;
    bad += ics_net_feed_close(u2) == 0;
    bad += ics_net_feed_slot(u2, 0, NULL, NULL, NULL, NULL, NULL) == 0;
    bad += ics_net_feed_submit(u2, 0, 1) == 0;
    rot[0] = rot[1] = rot[2] = 0;
    bad += ics_net_feed_submit_rot(u2, 0, 1, rot) == 0;
    bad += ics_net_feed_submit_rot(NULL, 0, 1, rot) == 0;
    bad += ics_unet_train_step_fed(u2, 0, &tk) == 0;
    bad += ics_net_feed_metrics(u2, 0, m) == 0;
    bad += ics_net_feed_open(NULL, &fc) == 0;
    bad += ics_net_feed_open(u2, NULL) == 0;
    t.slots = 1; bad += ics_net_feed_open(u2, &t) == 0; t = fc;
    t.slots = 5; bad += ics_net_feed_open(u2, &t) == 0; t = fc;
    t.x_channels[0] = C + 1; bad += ics_net_feed_open(u2, &t) == 0; t = fc;
    t.label_kind = 0; bad += ics_net_feed_open(u2, &t) == 0; t = fc;
    t.x_dtype[0] = 2; bad += ics_net_feed_open(u2, &t) == 0; t = fc;
    if (bad) { fprintf(stderr, "feed: %d invalid open / no-feed calls accepted\n", bad); return 1; }
    OK(ics_net_feed_open(u2, &fc));
    OK(ics_net_feed_slot(u2, 0, NULL, NULL, NULL, NULL, NULL));
    OK(ics_net_feed_submit(u2, 0, B));
    OK(ics_net_destroy(u2));               /* with an open feed and an upload that no step consumed */
  }
  free(rot);
  return 0;
}

static int run(int d, int C, int B, int with_comm) {
  const size_t M = (size_t)B * d * d * d;
  ics_unet_config uc = {C, 95, d, B, 1e-3f, 0.f, 1, 1, with_comm == 2};
  ics_vae_config vc = {C, 10, 256, {16, 32, 64, 128}, d, B, 5e-4f, 0.5f, 3e-4f, {1.f, 1.f, 1.f, 1.f}, 1};
  ics_net *unet = NULL, *vae = NULL;
  OK(ics_unet_create(&uc, &unet));
  OK(ics_vae_create(&vc, unet, &vae));
  if (tensor_io(unet) || tensor_io(vae)) return 1;
  if (with_comm) {
    char uid[128];
    OK(ics_comm_unique_id(uid));
    OK(ics_net_comm_init(unet, 0, 1, uid));
    OK(ics_net_comm_init(vae, 0, 1, uid));
    OK(ics_net_comm_broadcast_state(unet, 0));
    OK(ics_net_comm_broadcast_state(vae, 0));
    OK(ics_net_set_sync_bn(unet, with_comm > 1));
    OK(ics_net_set_sync_bn(vae, with_comm > 1));
    double v = 1.0;
    OK(ics_net_comm_allreduce_max(unet, &v));
  }
  float* x = (float*)calloc(M * C, sizeof(float));
  uint8_t* lab = (uint8_t*)calloc(M, 1);
  float* soft = (float*)malloc(M * 95 * sizeof(float));
  float* sig = (float*)malloc(M * sizeof(float));
  uint8_t* sp = (uint8_t*)malloc(M);
  uint8_t* mk = (uint8_t*)malloc(M);
  float* cond = (float*)calloc((size_t)B * 10, sizeof(float));
  float* eps = (float*)calloc((size_t)B * 256, sizeof(float));
  float* z = (float*)calloc((size_t)B * 256 * 3, sizeof(float));
  float* rec = (float*)malloc(M * C * sizeof(float));
  float mm[5], mv[4], minmax[6 * 8];
  { ics_net* v2 = NULL; OK(ics_vae_create(&vc, unet, &v2)); OK(ics_net_share_stream(v2, unet)); OK(ics_net_destroy(v2)); }
  OK(ics_net_profile_enable(unet, 1));
  OK(ics_net_profile_enable(vae, 1));
  for (int b = 1; b <= B; ++b) {   /* every batch size up to max_batch: the split plans depend on it */
    OK(ics_unet_train_step(unet, x, lab, b, mm));
    OK(ics_unet_test_step(unet, x, lab, b, mm));
    { double ms[7]; OK(ics_unet_metric_sums(unet, ms)); }
    OK(ics_unet_upload_batch(unet, x, lab, b));
    OK(ics_net_timer_start(unet));
    OK(ics_unet_predict_resident(unet, 0, 0.8f));
    OK(ics_unet_predict_resident(unet, 1, 0.8f));
    { double tms; OK(ics_net_timer_stop(unet, &tms)); }
    OK(ics_unet_predict(unet, x, b, soft, sig));
    OK(ics_unet_predict_labels(unet, x, b, 0.8f, sp, mk));
    OK(ics_vae_train_step(vae, x, cond, eps, b, mv));
    OK(ics_vae_test_step(vae, x, cond, eps, b, mv));
    OK(ics_vae_encode(vae, x, cond, eps, b, z, z + (size_t)B * 256, z + (size_t)B * 512));
    OK(ics_vae_decode(vae, z, cond, b, rec));
    OK(ics_vae_decode_to_unet_labels(vae, unet, z, cond, b, 0.8f, sp, mk, rec, minmax));
    {   /* ... continued through connected components / region statistics */
      int32_t* regions = (int32_t*)malloc(M * sizeof(int32_t));
      int32_t counts[2 * 8];
      int32_t* stats = (int32_t*)malloc((size_t)b * 64 * 11 * sizeof(int32_t));
      { int64_t* bnd = calloc((size_t)b * 64 * 8, 8); OK(ics_vae_decode_to_unet_atoms(vae, unet, z, cond, b, 0.8f, 3, 64, sp, mk, rec, minmax, regions, counts, stats, bnd)); free(bnd); }
      OK(ics_vae_decode_to_unet_atoms(vae, unet, z, cond, b, 0.8f, 3, 64, NULL, NULL, NULL, NULL, NULL, counts, stats, NULL));
      OK(ics_vae_upload_batch(vae, x, cond, eps, b));     /* the same chain from the resident batch */
      { int64_t* bnd = calloc((size_t)b * 64 * 8, 8); OK(ics_vae_reconstruct_resident_to_unet_atoms(vae, unet, 0.8f, 3, 64, sp, mk, rec, minmax, regions, counts, stats, bnd)); free(bnd); }
      OK(ics_vae_reconstruct_resident_to_unet_atoms(vae, unet, 0.8f, 3, 64, NULL, NULL, NULL, NULL, NULL, counts, stats, NULL));
      free(regions); free(stats);
    }
  }
  OK(ics_unet_upload_batch(unet, x, lab, B));
  OK(ics_unet_train_step_resident(unet, NULL));
  OK(ics_vae_upload_batch(vae, x, cond, eps, B));
  OK(ics_vae_train_step_resident(vae, mv));
  if (class_weight_walk(unet, vae, uc.num_classes, x, lab, B, with_comm)) return 1;
  if (confusion_walk(unet, vae, uc.num_classes, d, x, lab, B)) return 1;
  if (atom_score_walk(unet, vae, uc.num_classes, d, x, lab, B)) return 1;
  if ((C == 1 || C == 4) && voxelise_walk(unet, vae, d, B, cond, eps)) return 1;
  if (interp_walk(unet, vae, &uc, x, cond, eps, B, d, C)) return 1;
  if (feed_walk(unet, vae, d, C, B, vc.cond_shape, vc.latent_dim)) return 1;
  if (B >= 2 && B <= 8 && tsne_walk(vae, unet, x, cond, eps, B)) return 1;
  if (reconstruct_refusals(unet, &vc, &uc, x, cond, eps, B)) return 1;
  if (C == 1 && B >= 2 && B <= 8 && monitor_walk(unet, vae, x, lab, cond, eps, B, d)) return 1;
  if (ics_unet_train_step(unet, x, lab, B + 1, mm) == 0) { fprintf(stderr, "max_batch check missing\n"); return 1; }
  int rows = 0;
  OK(ics_net_profile_count(unet, &rows));
  for (int r = 0; r < rows; ++r) {
    const char* label; int64_t launches; double ms, fl, by;
    OK(ics_net_profile_row(unet, r, &label, &launches, &ms, &fl, &by));
  }
  size_t np = 0;
  OK(ics_net_num_params(unet, &np));
  float* m1 = (float*)malloc(np * sizeof(float));
  float* v1 = (float*)malloc(np * sizeof(float));
  int step = 0;
  OK(ics_net_get_optimizer_state(unet, m1, v1, np, &step));
  OK(ics_net_set_optimizer_state(unet, m1, v1, np, step));
  OK(ics_net_reset_optimizer(unet));
  { int dirty = -1; OK(ics_net_check_canaries(unet, &dirty)); OK(ics_net_check_canaries(vae, &dirty)); }
  {   /* the graph probe needs the profiler off and a resident batch */
    double em, gm; int nodes, rk, nr, nb;
    OK(ics_net_profile_enable(unet, 0)); OK(ics_net_profile_enable(vae, 0));
    OK(ics_net_comm_info(unet, &rk, &nr, &nb));
    if (nr == 0) {
      OK(ics_net_graph_probe(unet, 2, &em, &gm, &nodes));
      OK(ics_net_graph_probe(vae, 2, &em, &gm, &nodes));
    } else if (ics_net_graph_probe(unet, 2, &em, &gm, &nodes) == 0) {
      fprintf(stderr, "graph probe must refuse an engine with a communicator\n"); return 1;
    }
    OK(ics_net_profile_enable(unet, 1)); OK(ics_net_profile_enable(vae, 1));
  }
  {
    size_t cnt = (size_t)B * (d / 8) * (d / 8) * (d / 8) * 512;      /* c10 activation */
    float* act = (float*)malloc(cnt * sizeof(float));
    float sc[512], sh[512];
    OK(ics_net_get_activation(unet, "c10", act, cnt));
    OK(ics_net_get_bn_affine(unet, "c10", sc, sh, 512));
    free(act);
  }
  int rk, nr, nb;
  OK(ics_net_comm_info(unet, &rk, &nr, &nb));
  free(m1); free(v1); free(x); free(lab); free(soft); free(sig); free(sp); free(mk); free(cond); free(eps); free(z); free(rec);
  OK(ics_net_destroy(vae));
  OK(ics_net_destroy(unet));
  return 0;
}

/* ics_op_conv_layer: one layer through the engines' construction and dispatch at every geometry class its planners
 * distinguish (Winograd 64 / 32 / S = 4, implicit GEMM, 1x1x1, thin-N, padded thin input, [skip | up], up only), forward
 * only and with the backward pass, on a handle larger than the batch, with buffers of the exact size; then the same
 * upsampled layers with the up-split switched off (the host-side 8-children sum) and every refusal. */
static int g_ranks = 0;   /* ics_conv_layer.ranks / ics_conv_link.ranks of the *_one walkers: every buffer is sized for exactly
                             that many ranks (batch tensors R * B samples, per-rank outputs [R], R site texts) */
static int g_bcast = 0;   /* > 0: the second source of conv_layer_one is a condition, x [R * B][g_bcast] of the exact size */
static int conv_layer_one(int B, int maxB, int S, int taps, int Cout, int form, int pad, int nsrc, const int* sc, const int* sup,
                          int aff, int bwd) {
  ics_conv_layer a;
  const int R = g_ranks > 0 ? g_ranks : 1;
  const int cap = 4096;
  char* text = malloc((size_t)cap * R);
  size_t M = (size_t)R * B * S * S * S;
  int Cin = 0;
  memset(&a, 0, sizeof a);
  a.ranks = g_ranks;
  a.B = B; a.max_batch = maxB; a.S = S; a.taps = taps; a.Cout = Cout; a.pad_input = pad; a.nsrc = nsrc;
  a.has_bn = form != 2; a.pre_act = form == 0 ? 1 : 0; a.post_act = form == 1 ? 2 : 0;
  for (int i = 0; i < nsrc; ++i) {
    size_t rows = sup[i] ? M / 8 : M;
    if (i == 1 && g_bcast > 0) {                       /* no affine, no activation, no dx */
      a.src[i].C = sc[i]; a.src[i].bcast = g_bcast;
      a.src[i].x = calloc((size_t)R * B * g_bcast, 4);
      Cin += sc[i];
      continue;
    }
    a.src[i].C = sc[i]; a.src[i].up = sup[i]; a.src[i].act = (aff && form == 1) ? 2 : 0;
    a.src[i].x = calloc(rows * sc[i], 4);
    if (aff) { a.src[i].scale = calloc(sc[i], 4); a.src[i].shift = calloc(sc[i], 4); }
    if (bwd) a.src[i].dx = malloc(rows * sc[i] * 4);
    Cin += sc[i];
  }
  a.w = calloc((size_t)taps * Cin * Cout, 4); a.bias = calloc(Cout, 4); a.gamma = calloc(Cout, 4); a.beta = calloc(Cout, 4);
  a.y = malloc(M * Cout * 4);
  {
    const size_t pc = (size_t)R * Cout * 4;            /* per-rank outputs: [R][Cout] */
    a.mean = malloc(pc); a.rstd = malloc(pc); a.scale = malloc(pc); a.shift = malloc(pc);
    a.moving_mean = malloc(pc); a.moving_var = malloc(pc);
    if (bwd) {
      a.dout = calloc(M * Cout, 4);
      a.dw = malloc((size_t)R * taps * Cin * Cout * 4); a.dbias = malloc(pc); a.dgamma = malloc(pc); a.dbeta = malloc(pc);
    }
  }
  a.kernels = text; a.kernels_cap = cap;
  OK(ics_op_conv_layer(&a));
  for (int r = 0; r < R; ++r)
    if (!strstr(text + (size_t)r * cap, "conv_fwd:L")) { fprintf(stderr, "conv layer: no forward launch site reported\n"); return 1; }
  a.kernels_cap = 9;                                   /* truncated, still terminated */
  OK(ics_op_conv_layer(&a));
  for (int r = 0; r < R; ++r)
    if (strlen(text + 9 * r) > 8) { fprintf(stderr, "conv layer: kernel text not truncated\n"); return 1; }
  free(text);
  for (int i = 0; i < nsrc; ++i) { free((void*)a.src[i].x); free((void*)a.src[i].scale); free((void*)a.src[i].shift); free(a.src[i].dx); }
  free((void*)a.w); free((void*)a.bias); free((void*)a.gamma); free((void*)a.beta); free((void*)a.dout); free(a.y);
  free(a.mean); free(a.rstd); free(a.scale); free(a.shift); free(a.moving_mean); free(a.moving_var);
  free(a.dw); free(a.dbias); free(a.dgamma); free(a.dbeta);
  return 0;
}
static int conv_layer_walk(void) {
  const int one[2] = {0, 0}, up1[2] = {1, 0}, su[2] = {0, 1};
  int c[2];
  for (int form = 0; form < 3; ++form)
    for (int bwd = 0; bwd < 2; ++bwd) {
      const int aff = form != 2;
      c[0] = 64; if (conv_layer_one(3, 5, 8, 27, 64, form, 0, 1, c, one, aff, bwd)) return 1;
      c[0] = 32; if (conv_layer_one(2, 2, 8, 27, 96, form, 0, 1, c, one, aff, bwd)) return 1;
      c[0] = 64; if (conv_layer_one(4, 4, 4, 27, 64, form, 0, 1, c, one, aff, bwd)) return 1;
      c[0] = 128; if (conv_layer_one(3, 5, 4, 27, 64, form, 0, 1, c, one, aff, bwd)) return 1;
      c[0] = 40; if (conv_layer_one(2, 3, 8, 27, 24, form, 0, 1, c, one, aff, bwd)) return 1;
      c[0] = 96; if (conv_layer_one(3, 5, 4, 1, 48, form, 0, 1, c, one, aff, bwd)) return 1;
      c[0] = 512; if (conv_layer_one(1, 2, 2, 27, 64, form, 0, 1, c, one, aff, bwd)) return 1;
      c[0] = 16; if (conv_layer_one(2, 7, 8, 27, 1, form, 0, 1, c, one, aff, bwd)) return 1;
      c[0] = 1; if (conv_layer_one(2, 3, 8, 27, 16, form, 1, 1, c, one, 0, bwd)) return 1;
      c[0] = 4; if (conv_layer_one(2, 2, 8, 27, 32, form, 1, 1, c, one, 0, bwd)) return 1;
      c[0] = 11; if (conv_layer_one(2, 2, 8, 27, 16, form, 1, 1, c, one, aff, bwd)) return 1;
      c[0] = 32; c[1] = 64; if (conv_layer_one(2, 5, 8, 27, 64, form, 0, 2, c, su, aff, bwd)) return 1;
      c[0] = 32; if (conv_layer_one(3, 7, 8, 27, 16, form, 0, 1, c, up1, aff, bwd)) return 1;
    }
  setenv("ICSG3D_NO_UPSPLIT", "1", 1);
  c[0] = 32; c[1] = 64; if (conv_layer_one(2, 3, 4, 27, 64, 0, 0, 2, c, su, 1, 1)) return 1;
  c[0] = 32; if (conv_layer_one(3, 3, 4, 27, 16, 1, 0, 1, c, up1, 1, 1)) return 1;
  unsetenv("ICSG3D_NO_UPSPLIT");
  /* emulated ranks (SyncBN through the rank tables): the geometry classes of tests/syncbn_cases.py, handle = and > batch */
  for (g_ranks = 1; g_ranks <= 3; ++g_ranks)
    for (int form = 0; form < 2; ++form)
      for (int bwd = 0; bwd < 2; ++bwd) {
        c[0] = 16; if (conv_layer_one(2, 2, 8, 27, 64, form, 0, 1, c, one, 1, bwd)) return 1;
        c[0] = 16; if (conv_layer_one(2, 4, 4, 27, 6, form, 0, 1, c, one, 1, bwd)) return 1;
        c[0] = 1; if (conv_layer_one(2, 3, 8, 27, 16, form, 1, 1, c, one, 0, bwd)) return 1;
        c[0] = 16; c[1] = 32; if (conv_layer_one(2, 3, 8, 27, 16, form, 0, 2, c, su, 1, bwd)) return 1;
        c[0] = 64; if (conv_layer_one(4, 4, 4, 27, 64, form, 0, 1, c, one, 1, bwd)) return 1;
      }
  g_ranks = 0;
  /* condition sources: folded (one x channel, 16 / 32 filters; 1 + 3 needs no padding), not folded under either switch,
   * four x channels through the materialised input (4 + 40 -> 64) and the broadcast loader (4 + 12 = 16), without padding,
   * and two emulated ranks (the condition is offset per rank by B * bcast) */
  {
    const int two[2] = {0, 0};
    for (int form = 0; form < 3; ++form)
      for (int bwd = 0; bwd < 2; ++bwd) {
        g_bcast = 10; c[0] = 1; c[1] = 10; if (conv_layer_one(2, 3, 4, 27, 16, form, 1, 2, c, two, 0, bwd)) return 1;
        g_bcast = 3; c[0] = 1; c[1] = 3; if (conv_layer_one(3, 3, 8, 27, 32, form, 1, 2, c, two, 0, bwd)) return 1;
        g_bcast = 10; c[0] = 1; c[1] = 10; if (conv_layer_one(2, 2, 8, 27, 16, form, 0, 2, c, two, 0, bwd)) return 1;
        g_bcast = 10; c[0] = 4; c[1] = 40; if (conv_layer_one(2, 3, 8, 27, 16, form, 1, 2, c, two, 0, bwd)) return 1;
        g_bcast = 3; c[0] = 4; c[1] = 12; if (conv_layer_one(3, 5, 4, 27, 16, form, 1, 2, c, two, 0, bwd)) return 1;
        setenv("ICSG3D_NO_COND_FOLD", "1", 1);
        g_bcast = 7; c[0] = 1; c[1] = 7; if (conv_layer_one(2, 3, 8, 27, 32, form, 1, 2, c, two, 0, bwd)) return 1;
        unsetenv("ICSG3D_NO_COND_FOLD");
        setenv("ICSG3D_NO_THIN_C", "1", 1);
        g_bcast = 1; c[0] = 1; c[1] = 1; if (conv_layer_one(2, 2, 8, 27, 16, form, 1, 2, c, two, 0, bwd)) return 1;
        unsetenv("ICSG3D_NO_THIN_C");
      }
    g_ranks = 2; g_bcast = 10; c[0] = 1; c[1] = 10;
    if (conv_layer_one(2, 3, 8, 27, 16, 1, 1, 2, c, two, 0, 1)) return 1;
    g_ranks = 0; g_bcast = 0;
  }
  {
    ics_conv_layer a;
    float buf[8 * 4] = {0};
    int bad = 0;
    memset(&a, 0, sizeof a);
    a.B = 1; a.max_batch = 1; a.S = 2; a.taps = 1; a.Cout = 4; a.nsrc = 1;
    a.src[0].x = buf; a.src[0].C = 4; a.w = buf; a.y = buf;
    OK(ics_op_conv_layer(&a));
    bad += ics_op_conv_layer(NULL) == 0;
    a.max_batch = 0; bad += ics_op_conv_layer(&a) == 0; a.max_batch = 1;
    a.S = 3; bad += ics_op_conv_layer(&a) == 0; a.S = 2;
    a.taps = 9; bad += ics_op_conv_layer(&a) == 0; a.taps = 1;
    a.nsrc = 3; bad += ics_op_conv_layer(&a) == 0; a.nsrc = 1;
    a.pre_act = 3; bad += ics_op_conv_layer(&a) == 0; a.pre_act = 0;
    a.has_bn = 1; bad += ics_op_conv_layer(&a) == 0; a.has_bn = 0;          /* no gamma / beta */
    a.post_act = 1; bad += ics_op_conv_layer(&a) == 0; a.post_act = 0;      /* post_act without BatchNorm */
    a.src[0].scale = buf; bad += ics_op_conv_layer(&a) == 0; a.src[0].scale = NULL;
    a.src[0].dx = buf; bad += ics_op_conv_layer(&a) == 0; a.src[0].dx = NULL;   /* gradients without dout */
    a.dw = buf; bad += ics_op_conv_layer(&a) == 0; a.dw = NULL;
    a.S = 1; a.src[0].up = 1; bad += ics_op_conv_layer(&a) == 0; a.S = 2; a.src[0].up = 0;
    a.w = NULL; bad += ics_op_conv_layer(&a) == 0; a.w = buf;
    a.src[0].bcast = 4; bad += ics_op_conv_layer(&a) == 0; a.src[0].bcast = 0;      /* a condition is the last of TWO sources */
    a.src[0].bcast = -1; bad += ics_op_conv_layer(&a) == 0; a.src[0].bcast = 0;
    {   /* a well-formed condition layer (1 + 2 channels, S = 4, 3x3x3), then each thing a condition source may not have */
      ics_conv_layer b = a;
      float big[2 * 64 * 3 * 27] = {0}, ybuf[2 * 64 * 4], gbuf[2 * 64 * 4] = {0};
      b.B = 2; b.max_batch = 2; b.S = 4; b.taps = 27; b.nsrc = 2; b.w = big; b.y = ybuf;
      b.src[0].x = big; b.src[0].C = 1; b.src[1].x = big; b.src[1].C = 2; b.src[1].bcast = 2;
      OK(ics_op_conv_layer(&b));
      b.src[1].scale = big; b.src[1].shift = big; bad += ics_op_conv_layer(&b) == 0; b.src[1].scale = NULL; b.src[1].shift = NULL;
      b.src[1].act = 1; bad += ics_op_conv_layer(&b) == 0; b.src[1].act = 0;
      b.src[1].up = 1; bad += ics_op_conv_layer(&b) == 0; b.src[1].up = 0;
      b.src[1].C = 3; bad += ics_op_conv_layer(&b) == 0; b.src[1].C = 2;           /* C = bcast * channels of the first */
      b.src[0].bcast = 1; bad += ics_op_conv_layer(&b) == 0; b.src[0].bcast = 0;
      b.dout = gbuf; b.src[1].dx = gbuf; bad += ics_op_conv_layer(&b) == 0;        /* no gradient w.r.t. the condition */
      if (!strstr(ics_last_error(), "never differentiate")) { fprintf(stderr, "conv layer: dx of a condition refused without its reason\n"); return 1; }
      b.src[1].dx = NULL;
      OK(ics_op_conv_layer(&b));
    }
    a.ranks = 5; bad += ics_op_conv_layer(&a) == 0;
    a.ranks = -1; bad += ics_op_conv_layer(&a) == 0;
    a.ranks = 2; a.max_batch = 0; bad += ics_op_conv_layer(&a) == 0; a.max_batch = 1; a.ranks = 0;   /* max_batch < B */
    if (bad) { fprintf(stderr, "conv layer: %d invalid argument sets accepted\n", bad); return 1; }
    OK(ics_op_conv_layer(&a));                                              /* still usable */
  }
  return 0;
}

/* ics_op_conv_link: every link in both forms, on a handle larger than the batch, with the linear folds at their default
 * threshold and forced on (ICSG3D_DGRAD_BNFUSE_MIN=0), without the up-split, under both tie rules; then every refusal. */
static void link_layer(ics_conv_link_layer* l, int Cin, int Cout, size_t rows) {
  const size_t pc = (size_t)(g_ranks > 0 ? g_ranks : 1) * Cout * 4;     /* per-rank outputs: [R][Cout] */
  l->Cout = Cout;
  l->w = calloc((size_t)27 * Cin * Cout, 4); l->bias = calloc(Cout, 4); l->gamma = calloc(Cout, 4); l->beta = calloc(Cout, 4);
  l->y = malloc(rows * Cout * 4);
  l->mean = malloc(pc); l->rstd = malloc(pc); l->scale = malloc(pc); l->shift = malloc(pc);
  l->dw = malloc(pc * 27 * Cin); l->dbias = malloc(pc); l->dgamma = malloc(pc); l->dbeta = malloc(pc);
}
static void link_layer_free(ics_conv_link_layer* l) {
  free((void*)l->w); free((void*)l->bias); free((void*)l->gamma); free((void*)l->beta); free(l->y);
  free(l->mean); free(l->rstd); free(l->scale); free(l->shift); free(l->dw); free(l->dbias); free(l->dgamma); free(l->dbeta);
}
static int conv_link_one(int link, int form, int B, int maxB, int S, int C0, int Cp, int Ck, int Cl, int Cq, int ties,
                         const char* site) {
  ics_conv_link a;
  const int R = g_ranks > 0 ? g_ranks : 1;
  const int cap = 8192;
  char* text = malloc((size_t)cap * R);
  const size_t M = (size_t)R * B * S * S * S;            /* rows of every batch tensor: R * B samples */
  const int has_k = link >= ICS_LINK_POOL, has_l = link != ICS_LINK_POOL;
  const size_t ML = link == ICS_LINK_UP ? 8 * M : M;
  memset(&a, 0, sizeof a);
  a.ranks = g_ranks;
  a.link = link; a.form = form; a.B = B; a.max_batch = maxB; a.S = S; a.C0 = C0; a.pool_ties_all = ties;
  a.x0 = calloc(M * C0, 4);
  link_layer(&a.P, C0, Cp, M);
  if (has_k) link_layer(&a.K, Cp, Ck, M / 8);
  if (has_l) link_layer(&a.L, Cp + (link == ICS_LINK_POOL_SKIP ? Cq : 0), Cl, ML);
  a.dout = has_k ? calloc(M / 8 * Ck, 4) : calloc(ML * Cl, 4);
  if (link == ICS_LINK_POOL_SKIP) { a.Cq = Cq; a.q = calloc(M / 8 * Cq, 4); a.dout_l = calloc(M * Cl, 4); }
  if (has_k) a.pooled = malloc(M / 8 * Cp * 4);
  a.dy_p = malloc(M * Cp * 4); a.dx0 = malloc(M * C0 * 4);
  a.sites = text; a.sites_cap = cap;
  OK(ics_op_conv_link(&a));
  for (int r = 0; r < R; ++r) {
    const char* t = text + (size_t)r * cap;
    if (!strstr(t, "conv_fwd:P|") || !strstr(t, "bn_act_bwd:") || (site && !strstr(t, site)) || (g_ranks && strstr(t, "bnfuse:"))) {
      fprintf(stderr, "conv link %d form %d ranks %d: launch sites missing (%s), or a fold under SyncBN, in\n%s", link, form,
              g_ranks, site ? site : "-", t);
      return 1;
    }
  }
  a.sites_cap = 9;                                     /* truncated, still terminated */
  OK(ics_op_conv_link(&a));
  for (int r = 0; r < R; ++r)
    if (strlen(text + 9 * r) > 8) { fprintf(stderr, "conv link: site text not truncated\n"); return 1; }
  free(text);
  free((void*)a.x0); free((void*)a.q); free((void*)a.dout); free((void*)a.dout_l); free(a.pooled); free(a.dy_p); free(a.dx0);
  link_layer_free(&a.P);
  if (has_k) link_layer_free(&a.K);
  if (has_l) link_layer_free(&a.L);
  return 0;
}
static int conv_link_walk(void) {
  for (int fused = 0; fused < 2; ++fused) {
    if (fused) setenv("ICSG3D_DGRAD_BNFUSE_MIN", "0", 1);
    for (int form = 0; form < 2; ++form)
      for (int big = 0; big < 2; ++big) {
        const int mb = big ? 5 : 3, u = fused && form == 0;
        if (conv_link_one(ICS_LINK_SAME, form, 3, mb, 8, 16, 64, 0, 128, 0, 1, u ? "bnfuse:L" : NULL)) return 1;
        if (conv_link_one(ICS_LINK_SAME, form, 2, mb, 8, 16, 96, 0, 32, 0, 1, NULL)) return 1;
        if (conv_link_one(ICS_LINK_SAME, form, 4, mb + 1, 4, 16, 64, 0, 64, 0, 1, NULL)) return 1;
        if (conv_link_one(ICS_LINK_SAME, form, 2, mb, 8, 16, 40, 0, 24, 0, 1, NULL)) return 1;
        if (conv_link_one(ICS_LINK_SAME, form, 3, mb, 4, 16, 128, 0, 40, 0, 1, NULL)) return 1;
        if (conv_link_one(ICS_LINK_UP, form, 2, mb, 4, 16, 64, 0, 64, 0, 1, "conv_dgrad:L.up|")) return 1;
        if (conv_link_one(ICS_LINK_UP, form, 2, mb, 4, 16, 32, 0, 16, 0, 1, "conv_dgrad:L.up|")) return 1;
        for (int ties = 0; ties < 2; ++ties) {
          if (conv_link_one(ICS_LINK_POOL, form, 3, mb, 8, 16, 64, 64, 0, 0, ties, form == 0 ? "pool_presum:P" : "pool_fwd")) return 1;
          if (conv_link_one(ICS_LINK_POOL, form, 2, mb, 8, 16, 16, 32, 0, 0, ties, "pool_fwd")) return 1;
          if (conv_link_one(ICS_LINK_POOL_SKIP, form, 2, mb, 8, 16, 64, 64, 128, 128, ties, u ? "bnfuse:P.pool" : "conv_dgrad:L.skip|"))
            return 1;
        }
      }
  }
  unsetenv("ICSG3D_DGRAD_BNFUSE_MIN");
  setenv("ICSG3D_NO_UPSPLIT", "1", 1);
  if (conv_link_one(ICS_LINK_UP, 0, 2, 3, 4, 16, 64, 0, 64, 0, 1, "conv_dgrad:L|")) return 1;
  if (conv_link_one(ICS_LINK_POOL_SKIP, 1, 2, 3, 4, 16, 32, 32, 32, 64, 0, "conv_dgrad:L|")) return 1;
  unsetenv("ICSG3D_NO_UPSPLIT");
  setenv("ICSG3D_NO_POOL_PRESUM", "1", 1);
  if (conv_link_one(ICS_LINK_POOL, 0, 3, 5, 8, 16, 64, 64, 0, 0, 1, "pool_fwd")) return 1;
  unsetenv("ICSG3D_NO_POOL_PRESUM");
  /* emulated ranks: every link, both forms, the folds forced on (they must be refused: no "bnfuse:" row), handle > batch */
  setenv("ICSG3D_DGRAD_BNFUSE_MIN", "0", 1);
  for (g_ranks = 1; g_ranks <= 3; ++g_ranks)
    for (int form = 0; form < 2; ++form) {
      if (conv_link_one(ICS_LINK_SAME, form, 2, 2, 8, 16, 64, 0, 128, 0, 1, "bn_act_bwd:P")) return 1;
      if (conv_link_one(ICS_LINK_SAME, form, 2, 3, 8, 16, 72, 0, 32, 0, 1, "bn_act_bwd:P")) return 1;
      if (conv_link_one(ICS_LINK_UP, form, 2, 4, 4, 16, 32, 0, 16, 0, 1, "conv_dgrad:L.up|")) return 1;
      for (int ties = 0; ties < 2; ++ties) {
        if (conv_link_one(ICS_LINK_POOL, form, 3, 4, 8, 16, 64, 64, 0, 0, ties, form == 0 ? "pool_presum:P" : "pool_fwd")) return 1;
        if (conv_link_one(ICS_LINK_POOL, form, 2, 2, 8, 16, 16, 32, 0, 0, ties, "pool_fwd")) return 1;
        if (conv_link_one(ICS_LINK_POOL_SKIP, form, 2, 3, 8, 16, 64, 64, 128, 128, ties, "conv_dgrad:L.skip|")) return 1;
      }
    }
  g_ranks = 0;
  unsetenv("ICSG3D_DGRAD_BNFUSE_MIN");
  {
    ics_conv_link a;
    float buf[27 * 4 * 4 + 64] = {0};
    int bad = 0;
    memset(&a, 0, sizeof a);
    a.link = ICS_LINK_SAME; a.B = 1; a.max_batch = 1; a.S = 2; a.C0 = 4; a.pool_ties_all = 1; a.x0 = buf; a.dout = buf;
    a.P.Cout = 4; a.P.w = buf; a.P.gamma = buf; a.P.beta = buf;
    a.L = a.P;
    OK(ics_op_conv_link(&a));
    bad += ics_op_conv_link(NULL) == 0;
    a.link = 4; bad += ics_op_conv_link(&a) == 0; a.link = ICS_LINK_SAME;
    a.form = 2; bad += ics_op_conv_link(&a) == 0; a.form = 0;
    a.max_batch = 0; bad += ics_op_conv_link(&a) == 0; a.max_batch = 1;
    a.S = 3; bad += ics_op_conv_link(&a) == 0; a.S = 2;
    a.x0 = NULL; bad += ics_op_conv_link(&a) == 0; a.x0 = buf;
    a.dout = NULL; bad += ics_op_conv_link(&a) == 0; a.dout = buf;
    a.pool_ties_all = 2; bad += ics_op_conv_link(&a) == 0; a.pool_ties_all = 1;
    a.pooled = buf; bad += ics_op_conv_link(&a) == 0; a.pooled = NULL;             /* no pool in this link */
    a.L.gamma = NULL; bad += ics_op_conv_link(&a) == 0; a.L.gamma = buf;
    a.P.w = NULL; bad += ics_op_conv_link(&a) == 0; a.P.w = buf;
    a.link = ICS_LINK_POOL; bad += ics_op_conv_link(&a) == 0;                       /* K missing */
    a.S = 1; a.K = a.P; bad += ics_op_conv_link(&a) == 0; a.S = 2;                  /* nothing to pool */
    a.link = ICS_LINK_POOL_SKIP; bad += ics_op_conv_link(&a) == 0;                  /* q, Cq, dout_l missing */
    a.link = ICS_LINK_SAME;
    a.ranks = 5; bad += ics_op_conv_link(&a) == 0;
    a.ranks = -1; bad += ics_op_conv_link(&a) == 0;
    a.ranks = 3; a.max_batch = 0; bad += ics_op_conv_link(&a) == 0; a.max_batch = 1; a.ranks = 0;   /* max_batch < B */
    if (bad) { fprintf(stderr, "conv link: %d invalid argument sets accepted\n", bad); return 1; }
    OK(ics_op_conv_link(&a));                                                       /* still usable */
  }
  return 0;
}

/* ics_op_head_link: the routes of the c18 -> head link on a handle larger than the batch -- the fused route (ncls = 95, rows in
 * sixteens), each switch that takes another, a row count and class counts the fused kernels refuse, a class-weight table,
 * the forward alone, emulated ranks -- then every refusal. */
static int head_link_one(int B, int maxB, int S, int C0, int ncls, int cw, int want_grad, const char* site, const char* absent) {
  ics_head_link a;
  const int R = g_ranks > 0 ? g_ranks : 1;
  const int cap = 8192;
  char* text = malloc((size_t)cap * R);
  const size_t M = (size_t)R * B * S * S * S, nz = (size_t)ncls + 1;
  memset(&a, 0, sizeof a);
  a.ranks = g_ranks;
  a.B = B; a.max_batch = maxB; a.S = S; a.C0 = C0; a.ncls = ncls; a.want_grad = want_grad;
  a.x0 = calloc(M * C0, 4);
  a.w = calloc((size_t)27 * C0 * 128, 4); a.bias = calloc(128, 4); a.gamma = calloc(128, 4); a.beta = calloc(128, 4);
  a.wsoft = calloc((size_t)128 * ncls, 4); a.bsoft = calloc(ncls, 4); a.wsig = calloc(128, 4); a.bsig = calloc(1, 4);
  a.labels = calloc(M, 1);
  if (cw) a.class_weights = calloc(ncls, 4);
  a.y = malloc(M * 128 * 4);
  a.mean = malloc((size_t)R * 128 * 4); a.rstd = malloc((size_t)R * 128 * 4); a.scale = malloc((size_t)R * 128 * 4);
  a.shift = malloc((size_t)R * 128 * 4);
  a.dz = malloc(M * nz * 4); a.metrics = malloc((size_t)R * 5 * 4); a.sums = malloc((size_t)R * 7 * 8);
  a.dwsoft = malloc((size_t)R * 128 * ncls * 4); a.dwsig = malloc((size_t)R * 128 * 4); a.dbias_head = malloc((size_t)R * nz * 4);
  a.dw = malloc((size_t)R * 27 * C0 * 128 * 4); a.dbias = malloc((size_t)R * 128 * 4); a.dgamma = malloc((size_t)R * 128 * 4);
  a.dbeta = malloc((size_t)R * 128 * 4);
  a.dy_p = malloc(M * 128 * 4); a.dx0 = malloc(M * C0 * 4);
  a.sites = text; a.sites_cap = cap;
  OK(ics_op_head_link(&a));
  for (int r = 0; r < R; ++r) {
    const char* t = text + (size_t)r * cap;
    if (!strstr(t, "conv_fwd:P|") || (site && !strstr(t, site)) || (absent && strstr(t, absent))) {
      fprintf(stderr, "head link B %d S %d ncls %d ranks %d: launch sites (want %s, not %s) in\n%s", B, S, ncls, g_ranks,
              site ? site : "-", absent ? absent : "-", t);
      return 1;
    }
  }
  a.sites_cap = 9;                                     /* truncated, still terminated */
  OK(ics_op_head_link(&a));
  for (int r = 0; r < R; ++r)
    if (strlen(text + 9 * r) > 8) { fprintf(stderr, "head link: site text not truncated\n"); return 1; }
  free(text);
  free((void*)a.x0); free((void*)a.w); free((void*)a.bias); free((void*)a.gamma); free((void*)a.beta);
  free((void*)a.wsoft); free((void*)a.bsoft); free((void*)a.wsig); free((void*)a.bsig); free((void*)a.labels);
  free((void*)a.class_weights);
  free(a.y); free(a.mean); free(a.rstd); free(a.scale); free(a.shift); free(a.dz); free(a.metrics); free(a.sums);
  free(a.dwsoft); free(a.dwsig); free(a.dbias_head); free(a.dw); free(a.dbias); free(a.dgamma); free(a.dbeta);
  free(a.dy_p); free(a.dx0);
  return 0;
}
static int head_link_walk(void) {
  const char *T = "conv_dgrad:head|head_dgrad_kernel<true>", *F = "conv_dgrad:head|head_dgrad_kernel", *G = "conv_dgrad:head|conv_fwd_kernel<";
  for (int big = 0; big < 2; ++big) {
    const int mb = big ? 5 : 2;
    if (head_link_one(2, mb, 2, 16, 95, 0, 1, T, "bn_act_bwd:P")) return 1;          /* one tile                       */
    if (head_link_one(2, mb + 4, 2, 16, 95, 1, 1, T, "bn_act_bwd:P")) return 1;      /* class-weight table             */
    if (head_link_one(2, mb, 8, 16, 95, 0, 1, "head_fused", "head_softmax_loss")) return 1;
    if (head_link_one(2, mb, 4, 8, 95, 0, 0, "head_fused", "conv_dgrad:")) return 1; /* the forward and the loss alone */
    if (head_link_one(1, mb, 2, 16, 95, 0, 1, G, "head_fused")) return 1;            /* 8 rows: no fused kernel        */
    if (head_link_one(2, mb, 4, 16, 31, 0, 1, G, "head_fused")) return 1;
    if (head_link_one(2, mb, 4, 16, 20, 1, 1, G, "head_fused")) return 1;
    if (head_link_one(2, mb, 4, 16, 127, 0, 1, "head_softmax_loss", "head_fused")) return 1;
    if (head_link_one(2, mb, 4, 16, 2, 0, 1, "bn_act_bwd:P", "head_fused")) return 1;
  }
  setenv("ICSG3D_NO_HEAD_BNFUSE", "1", 1);
  if (head_link_one(3, 5, 4, 16, 95, 0, 1, F, "<true>")) return 1;
  setenv("ICSG3D_NO_BWD_FOLD", "1", 1);
  if (head_link_one(3, 5, 4, 16, 95, 0, 1, "bn_act_bwd:P", "<true>")) return 1;
  unsetenv("ICSG3D_NO_BWD_FOLD");
  unsetenv("ICSG3D_NO_HEAD_BNFUSE");
  setenv("ICSG3D_NO_FUSED_HEAD", "1", 1);
  if (head_link_one(3, 5, 4, 16, 95, 0, 1, G, "head_fused")) return 1;
  unsetenv("ICSG3D_NO_FUSED_HEAD");
  setenv("ICSG3D_NO_FAST_BNBWD", "1", 1);
  if (head_link_one(3, 5, 4, 16, 95, 0, 1, T, NULL)) return 1;
  unsetenv("ICSG3D_NO_FAST_BNBWD");
  for (g_ranks = 1; g_ranks <= 4; ++g_ranks) {
    if (head_link_one(2, 3, 4, 16, 95, 0, 1, "xhat_affine:head", "bn_act_bwd:P")) return 1;
    if (head_link_one(2, 3, 4, 16, 95, 0, 1, "head_bnfuse_exchange", "bn_act_bwd:P")) return 1;
    if (head_link_one(1, 1, 2, 16, 95, 0, 1, G, "head_fused")) return 1;             /* 8 rows per rank: P's all-reduce */
  }
  g_ranks = 0;
  {
    ics_head_link a;
    static float buf[27 * 4 * 128] = {0};
    static uint8_t lab[8] = {0};
    int bad = 0;
    memset(&a, 0, sizeof a);
    a.B = 1; a.max_batch = 1; a.S = 2; a.C0 = 4; a.ncls = 5; a.x0 = buf; a.w = buf; a.gamma = buf; a.beta = buf;
    a.wsoft = buf; a.bsoft = buf; a.wsig = buf; a.bsig = buf; a.labels = lab; a.want_grad = 1;
    OK(ics_op_head_link(&a));
    bad += ics_op_head_link(NULL) == 0;
    a.max_batch = 0; bad += ics_op_head_link(&a) == 0; a.max_batch = 1;
    a.B = 0; bad += ics_op_head_link(&a) == 0; a.B = 1;
    a.S = 3; bad += ics_op_head_link(&a) == 0; a.S = 2;
    a.C0 = 0; bad += ics_op_head_link(&a) == 0; a.C0 = 4;
    a.ncls = 1; bad += ics_op_head_link(&a) == 0;
    a.ncls = 128; bad += ics_op_head_link(&a) == 0; a.ncls = 5;
    a.x0 = NULL; bad += ics_op_head_link(&a) == 0; a.x0 = buf;
    a.w = NULL; bad += ics_op_head_link(&a) == 0; a.w = buf;
    a.gamma = NULL; bad += ics_op_head_link(&a) == 0; a.gamma = buf;
    a.wsig = NULL; bad += ics_op_head_link(&a) == 0; a.wsig = buf;
    a.bsoft = NULL; bad += ics_op_head_link(&a) == 0; a.bsoft = buf;
    a.labels = NULL; bad += ics_op_head_link(&a) == 0; a.labels = lab;
    lab[3] = 5; bad += ics_op_head_link(&a) == 0; lab[3] = 0;                         /* a label that is no class */
    a.bce_from_logits = 2; bad += ics_op_head_link(&a) == 0; a.bce_from_logits = 0;
    buf[2] = -1.f; a.class_weights = buf; bad += ics_op_head_link(&a) == 0; buf[2] = 0.f; a.class_weights = NULL;
    a.ranks = 5; bad += ics_op_head_link(&a) == 0;
    a.ranks = -1; bad += ics_op_head_link(&a) == 0; a.ranks = 0;
    if (bad) { fprintf(stderr, "head link: %d invalid argument sets accepted\n", bad); return 1; }
    OK(ics_op_head_link(&a));                                                         /* still usable */
  }
  return 0;
}

int main(void) {
  char name[256]; int cus; size_t hbm; int ndev = 0;
  OK(ics_device_count(&ndev));
  OK(ics_set_device(0));
  OK(ics_device_info(name, &cus, &hbm));
  printf("asan driver on %s (%s)\n", name, ics_version());
  setenv("ICSG3D_SYMMETRY_CHUNK_BYTES", "300000", 1);   /* the symmetry op over several chunks */
  setenv("ICSG3D_FINGERPRINT_CHUNK_BYTES", "4000", 1);  /* the fingerprint op over several chunks of both kernel kinds */
  setenv("ICSG3D_FINGERPRINT_CHUNK_PAIRS", "200000", 1); /* the nearest op one segment per launch */
  setenv("ICSG3D_MATCH_CHUNK_PAIRS", "7", 1);   /* the match planner over many chunks (read at the first match call) */
  setenv("ICSG3D_DGRAD_BNFUSE_MIN", "0", 1);   /* walk the BatchNorm-backward-in-backward-data fusion at these small sizes too */
  if (run(16, 1, 3, 0)) return 1;
  if (run(16, 4, 2, 1)) return 1;      /* 4 channels (Cin 44 -> padded loaders), single-rank communicator */
  if (run(32, 1, 2, 2)) return 1;      /* d = 32 plans, SyncBN */
  if (run(32, 1, 5, 0)) return 1;      /* plans that are not monotone in the batch: 3 grids on a 5-grid handle need more
                                          BatchNorm-backward blocks than 5 do (the engine's capacity checks fire if a
                                          workspace was sized for max_batch alone, round 6) */
  if (match_walk()) return 1;
  if (structure_walk()) return 1;
  if (structure_match_walk()) return 1;
  if (structure_symmetry_walk()) return 1;
  if (structure_fingerprint_walk()) return 1;
  if (latent_walk()) return 1;
  if (render_walk()) return 1;
  if (monitor_walk(NULL, NULL, NULL, NULL, NULL, NULL, 0, 0)) return 1;
  if (tsne_walk(NULL, NULL, NULL, NULL, NULL, 0)) return 1;
  {   /* single-op entry points: one shape per dispatch class they reach through the one-layer handle -- Winograd, the
         Winograd-domain GEMMs (backward-weight included: B % 4 == 0), the implicit GEMM, 1x1x1 -- buffers of the exact size */
    static const int shapes[4][5] = {{1, 8, 32, 32, 27}, {4, 4, 64, 64, 27}, {1, 8, 11, 16, 27}, {1, 1, 32, 256, 1}};
    for (int i = 0; i < 4; ++i) {
      const int B = shapes[i][0], S = shapes[i][1], Cin = shapes[i][2], Cout = shapes[i][3], taps = shapes[i][4];
      size_t nx = (size_t)B * S * S * S * Cin, ny = (size_t)B * S * S * S * Cout, nw = (size_t)taps * Cin * Cout;
      float *x = calloc(nx, 4), *y = calloc(ny, 4), *w = calloc(nw, 4), *b = calloc(Cout, 4), *dx = calloc(nx, 4), *dw = calloc(nw, 4);
      OK(ics_op_conv3d_forward(x, w, b, B, S, Cin, Cout, taps, 0, y));
      OK(ics_op_conv3d_forward(x, w, NULL, B, S, Cin, Cout, taps, 1, y));
      OK(ics_op_conv3d_backward(x, w, y, B, S, Cin, Cout, taps, dx, NULL));
      OK(ics_op_conv3d_backward(x, w, y, B, S, Cin, Cout, taps, NULL, dw));
      OK(ics_op_conv3d_backward(x, w, y, B, S, Cin, Cout, taps, dx, dw));
      if (ics_op_conv3d_forward(x, w, b, B, S, Cin, Cout, 8, 0, y) == 0 || ics_op_conv3d_backward(x, w, NULL, B, S, Cin, Cout, taps, dx, dw) == 0) {
        fprintf(stderr, "conv3d ops: invalid arguments accepted\n"); return 1;
      }
      free(x); free(y); free(w); free(b); free(dx); free(dw);
    }
  }
  if (conv_layer_walk()) return 1;
  if (conv_link_walk()) return 1;
  if (head_link_walk()) return 1;
  {   /* the op-level head: both launch sequences */
    const size_t M = 64;
    float *x = calloc(M * 128, 4), *ws = calloc(128 * 95, 4), *bs = calloc(95, 4), *wg = calloc(128, 4), bg[1] = {0.f};
    float *out = calloc(M * 96, 4), met[5];
    double sums[7];
    uint8_t* lab = calloc(M, 1);
    for (int f = 0; f < 2; ++f)
      for (int mode = 0; mode < 3; ++mode) OK(ics_op_unet_head(x, ws, bs, wg, bg, lab, M, 95, 0.f, mode, f, out, met, sums));
    {   /* the same with a class-weight table: the loss modes, a NULL table, and the refusals */
      float cw[95];
      for (int c = 0; c < 95; ++c) cw[c] = c ? 0.5f + (float)(c % 5) : 0.f;
      for (int f = 0; f < 2; ++f)
        for (int mode = 1; mode < 3; ++mode) OK(ics_op_unet_head_weighted(x, ws, bs, wg, bg, lab, M, 95, 0.f, mode, f, out, met, sums, cw));
      OK(ics_op_unet_head_weighted(x, ws, bs, wg, bg, lab, M, 95, 0.f, 0, 1, out, met, sums, NULL));
      int badw = ics_op_unet_head_weighted(x, ws, bs, wg, bg, lab, M, 95, 0.f, 0, 1, out, met, sums, cw) == 0;
      cw[3] = -2.f; badw += ics_op_unet_head_weighted(x, ws, bs, wg, bg, lab, M, 95, 0.f, 1, 1, out, met, sums, cw) == 0;
      cw[3] = NAN; badw += ics_op_unet_head_weighted(x, ws, bs, wg, bg, lab, M, 95, 0.f, 1, 0, out, met, sums, cw) == 0;
      if (badw) { fprintf(stderr, "weighted head: %d invalid argument sets accepted\n", badw); return 1; }
    }
    if (label_counts_walk()) return 1;
    free(x); free(ws); free(bs); free(wg); free(out); free(lab);
    /* ... and the finalisation from (all-reduced) sums */
    sums[6] = 64.0;
    OK(ics_op_unet_metrics_from_sums(sums, met));
    if (ics_op_unet_metrics_from_sums(NULL, met) == 0 || ics_op_unet_metrics_from_sums(sums, NULL) == 0) {
      fprintf(stderr, "metrics from sums: null argument accepted\n"); return 1;
    }
  }
  {   /* the DFC-VAE loss assembly in its three phases, buffers of the exact size */
    const int B = 3, latent = 20, n_mse = 5, pm_n[4] = {3, 0, 2, 1};
    const double per[4] = {8, 4, 2, 1};
    const float w[4] = {1.f, 0.f, 1.f, 1.f};
    float* mulv = calloc((size_t)B * 2 * latent, 4), met[4];
    double *mse = calloc(n_mse, 8), *pm = calloc(6, 8), sums[5] = {0, 0, 0, 0, 0};
    int bad = 0;
    OK(ics_op_vae_loss(mulv, B, latent, mse, n_mse, 100.0, pm, pm_n, per, w, 0.5f, 3e-4f, 0, NULL, met));
    OK(ics_op_vae_loss(mulv, B, latent, mse, n_mse, 100.0, pm, pm_n, per, w, 0.5f, 3e-4f, 1, sums, NULL));
    sums[3] = 3; sums[4] = 100;
    OK(ics_op_vae_loss(NULL, 0, 0, NULL, 0, 0.0, NULL, NULL, NULL, NULL, 0.5f, 3e-4f, 2, sums, met));
    bad += ics_op_vae_loss(mulv, B, latent, mse, n_mse, 100.0, pm, pm_n, per, w, 0.5f, 3e-4f, 3, sums, met) == 0;
    bad += ics_op_vae_loss(NULL, B, latent, mse, n_mse, 100.0, pm, pm_n, per, w, 0.5f, 3e-4f, 0, sums, met) == 0;
    bad += ics_op_vae_loss(mulv, 0, latent, mse, n_mse, 100.0, pm, pm_n, per, w, 0.5f, 3e-4f, 0, sums, met) == 0;
    bad += ics_op_vae_loss(mulv, B, latent, NULL, n_mse, 100.0, pm, pm_n, per, w, 0.5f, 3e-4f, 0, sums, met) == 0;
    bad += ics_op_vae_loss(mulv, B, latent, mse, n_mse, 0.0, pm, pm_n, per, w, 0.5f, 3e-4f, 0, sums, met) == 0;
    bad += ics_op_vae_loss(mulv, B, latent, mse, n_mse, 100.0, NULL, pm_n, per, w, 0.5f, 3e-4f, 0, sums, met) == 0;
    bad += ics_op_vae_loss(mulv, B, latent, mse, n_mse, 100.0, pm, pm_n, per, w, 0.5f, 3e-4f, 1, NULL, met) == 0;
    bad += ics_op_vae_loss(mulv, B, latent, mse, n_mse, 100.0, pm, pm_n, per, w, 0.5f, 3e-4f, 0, sums, NULL) == 0;
    bad += ics_op_vae_loss(NULL, 0, 0, NULL, 0, 0.0, NULL, NULL, NULL, NULL, 0.5f, 3e-4f, 2, NULL, met) == 0;
    if (bad) { fprintf(stderr, "vae loss: %d invalid argument sets accepted\n", bad); return 1; }
    free(mulv); free(mse); free(pm);
  }
  {   /* the latent link: forward only and with the backward pass, handle = and > batch, buffers of the exact size */
    const int shapes[4][4] = {{1, 1, 1, 1}, {3, 5, 20, 3}, {2, 2, 33, 7}, {5, 5, 256, 10}};
    int bad = 0;
    for (int k = 0; k < 4; ++k)
      for (int bwd = 0; bwd < 2; ++bwd) {
        const int B = shapes[k][0], lat = shapes[k][2], nc = shapes[k][3];
        ics_vae_latent a;
        memset(&a, 0, sizeof a);
        a.B = B; a.max_batch = shapes[k][1]; a.latent = lat; a.ncond = nc; a.beta = 1e-2f;
        a.h = calloc((size_t)B * lat, 4); a.eps = calloc((size_t)B * lat, 4); a.cond = calloc((size_t)B * nc, 4);
        a.w_mean = calloc((size_t)lat * lat, 4); a.w_lv = calloc((size_t)lat * lat, 4);
        if (k != 1) { a.b_mean = calloc(lat, 4); a.b_lv = calloc(lat, 4); }       /* the biases are optional */
        a.mulv = malloc((size_t)B * 2 * lat * 4); a.z = malloc((size_t)B * lat * 4); a.zc = malloc((size_t)B * (lat + nc) * 4);
        if (bwd) {
          a.dzc = calloc((size_t)B * (lat + nc), 4);
          a.dmulv = malloc((size_t)B * 2 * lat * 4); a.dw_mean = malloc((size_t)lat * lat * 4); a.dw_lv = malloc((size_t)lat * lat * 4);
          a.dbias = malloc((size_t)2 * lat * 4); a.dh = malloc((size_t)B * lat * 4);
        }
        OK(ics_op_vae_latent(&a));
        if (k == 1 && bwd) {
          setenv("ICSG3D_NO_VAE_SIDE_WGRAD", "1", 1);
          OK(ics_op_vae_latent(&a));
          unsetenv("ICSG3D_NO_VAE_SIDE_WGRAD");
          a.max_batch = 2; bad += ics_op_vae_latent(&a) == 0; a.max_batch = 5;
          a.latent = 0; bad += ics_op_vae_latent(&a) == 0; a.latent = lat;
          a.ncond = 0; bad += ics_op_vae_latent(&a) == 0; a.ncond = nc;
          { const float* t = a.h; a.h = NULL; bad += ics_op_vae_latent(&a) == 0; a.h = t; }
          { const float* t = a.eps; a.eps = NULL; bad += ics_op_vae_latent(&a) == 0; a.eps = t; }
          { const float* t = a.dzc; a.dzc = NULL; bad += ics_op_vae_latent(&a) == 0; a.dzc = t; }   /* gradients without dzc */
          bad += ics_op_vae_latent(NULL) == 0;
          OK(ics_op_vae_latent(&a));
        }
        free((void*)a.h); free((void*)a.eps); free((void*)a.cond); free((void*)a.w_mean); free((void*)a.w_lv);
        free((void*)a.b_mean); free((void*)a.b_lv); free((void*)a.dzc); free(a.mulv); free(a.z); free(a.zc);
        free(a.dmulv); free(a.dw_mean); free(a.dw_lv); free(a.dbias); free(a.dh);
      }
    if (bad) { fprintf(stderr, "vae latent: %d invalid argument sets accepted\n", bad); return 1; }
  }
  {   /* the squared-error partial sums: with and without the gradient, accumulating, blocks past the sample's end */
    const int B = 3, per[3] = {4100, 4099, 8}, bps[3] = {1, 16, 256};
    int bad = 0;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        float *x = calloc((size_t)B * per[i], 4), *y = calloc((size_t)B * per[i], 4), *g = calloc((size_t)B * per[i], 4);
        double* part = malloc((size_t)B * bps[j] * 8);
        OK(ics_op_sqdiff(x, y, B, per[i], bps[j], 0.f, 0, NULL, part));
        OK(ics_op_sqdiff(x, y, B, per[i], bps[j], 0.5f, 0, g, part));
        OK(ics_op_sqdiff(x, y, B, per[i], bps[j], 0.5f, 1, g, part));
        if (i == 0 && j == 0) {
          bad += ics_op_sqdiff(NULL, y, B, per[i], bps[j], 0.f, 0, NULL, part) == 0;
          bad += ics_op_sqdiff(x, y, B, per[i], bps[j], 0.f, 0, NULL, NULL) == 0;
          bad += ics_op_sqdiff(x, y, 0, per[i], bps[j], 0.f, 0, NULL, part) == 0;
          bad += ics_op_sqdiff(x, y, B, 0, bps[j], 0.f, 0, NULL, part) == 0;
          bad += ics_op_sqdiff(x, y, B, per[i], 0, 0.f, 0, NULL, part) == 0;
          bad += ics_op_sqdiff(x, y, B, per[i], bps[j], 0.f, 1, NULL, part) == 0;    /* nothing to accumulate into */
          bad += ics_op_sqdiff(x, y, B, per[i], bps[j], 0.f, 2, g, part) == 0;
        }
        free(x); free(y); free(g); free(part);
      }
    if (bad) { fprintf(stderr, "sqdiff: %d invalid argument sets accepted\n", bad); return 1; }
  }
  {   /* the pooling pass of the 125-product up-split backward: both kernels, several tiles per wave and two channel groups */
    const int shp[3][3] = {{2, 8, 32}, {1, 16, 64}, {1, 8, 512}};
    int bad = 0;
    for (int i = 0; i < 3; ++i) {
      const int B = shp[i][0], S = shp[i][1], N = shp[i][2];
      const size_t rows = (size_t)B * (S / 4) * (S / 4) * (S / 4);
      float *dy = calloc((size_t)B * S * S * S * N, 4), *out = malloc(125 * rows * N * 4);
      OK(ics_op_up125_pool(dy, B, S, N, 0, out));
      OK(ics_op_up125_pool(dy, B, S, N, 1, out));
      if (i == 0) {
        bad += ics_op_up125_pool(NULL, B, S, N, 1, out) == 0;
        bad += ics_op_up125_pool(dy, B, S, N, 1, NULL) == 0;
        bad += ics_op_up125_pool(dy, B, S, N, 2, out) == 0;
        bad += ics_op_up125_pool(dy, B, S, N, -1, out) == 0;
        bad += ics_op_up125_pool(dy, 0, S, N, 1, out) == 0;
        bad += ics_op_up125_pool(dy, B, 4, N, 1, out) == 0;
        bad += ics_op_up125_pool(dy, B, 12, N, 1, out) == 0;
        bad += ics_op_up125_pool(dy, B, S, 48, 1, out) == 0;
        bad += ics_op_up125_pool(dy, B, S, 16, 1, out) == 0;
      }
      free(dy); free(out);
    }
    if (bad) { fprintf(stderr, "up125 pool: %d invalid argument sets accepted\n", bad); return 1; }
  }
  {   /* connected components on host arrays */
    const int B = 2, d = 16;
    const size_t M = (size_t)B * d * d * d;
    uint8_t *mask = calloc(M, 1), *species = calloc(M, 1);
    int32_t* regions = malloc(M * sizeof(int32_t));
    int32_t counts[4];
    int32_t* stats = malloc((size_t)B * 32 * 11 * sizeof(int32_t));
    { int64_t* bnd = calloc((size_t)B * 32 * 8, 8); OK(ics_op_segment_atoms(mask, species, B, d, 3, 32, 95, regions, counts, stats, bnd)); free(bnd); }
    OK(ics_op_segment_atoms(mask, species, B, d, 3, 32, 95, regions, counts, stats, NULL));
    if (ics_op_segment_atoms(mask, species, B, 24, 3, 32, 95, regions, counts, stats, NULL) == 0) { fprintf(stderr, "grid check missing\n"); return 1; }
    free(mask); free(species); free(regions); free(stats);
  }
  {  /* segment_nuclei's box operations (round 4): host-side batching, descriptor tables, scratch sizing */
    int32_t dims[6] = {3, 4, 5, 2, 2, 7};
    int32_t vols[60 + 28], labels[60 + 28], wss[60 + 28], nlab[2], cls[2] = {1, 5};
    int32_t bstats[2 * 8 * 7], rstats[4 * 11];
    uint8_t sp[60];
    memset(vols, 0, sizeof vols); memset(sp, 0, sizeof sp);
    vols[7] = 1; vols[8] = 1; vols[61] = 5;
    OK(ics_op_label_boxes(vols, dims, 2, 1, 8, labels, nlab, bstats));
    OK(ics_op_label_boxes(vols, dims, 2, 3, 8, labels, nlab, NULL));
    OK(ics_op_watershed_split(vols, dims, cls, 2, 0, wss));
    OK(ics_op_watershed_split(vols, dims, cls, 2, 1, wss));
    OK(ics_op_region_stats(vols, sp, 3, 4, 5, 4, 95, rstats));
    dims[0] = 257;
    if (ics_op_label_boxes(vols, dims, 2, 1, 8, labels, nlab, bstats) == 0) { fprintf(stderr, "box extent check missing\n"); return 1; }
    if (ics_op_label_boxes(vols, dims + 3, 1, 2, 8, labels, nlab, bstats) == 0) { fprintf(stderr, "connectivity check missing\n"); return 1; }
    OK(ics_release_caches());     /* the per-thread stream and scratch of the box-level entry points (LeakSanitizer sees the rest) */
  }
  {  /* round 6: the HOST forms of the box operations are real code under this build (threads, heap flood, integer gift
        wrapping): a ragged pseudo-random volume, labelled here by a plain flood fill, through ics_op_component_bounds (with
        and without the exact hull count) and ics_op_watershed_split (many boxes: the thread pool; both tie rules) */
    enum { D = 20, H = 18, W = 16, V = D * H * W, ML = 512 };
    int32_t* vol = (int32_t*)calloc(V, 4);
    int32_t* lab = (int32_t*)calloc(V, 4);
    int32_t* stack = (int32_t*)malloc(V * 4);
    int32_t* st7 = (int32_t*)calloc(ML * 7, 4);
    unsigned lcg = 12345u;
    for (int i = 0; i < V; ++i) { lcg = lcg * 1664525u + 1013904223u; vol[i] = ((lcg >> 16) % 100) < 38; }
    for (int z = 6; z < 14; ++z) for (int y = 5; y < 13; ++y) for (int x = 4; x < 12; ++x) vol[(z * H + y) * W + x] = 1;   /* a solid core */
    int n = 0;
    for (int s0 = 0; s0 < V && n < ML; ++s0) {
      if (!vol[s0] || lab[s0]) continue;
      ++n;
      int top = 0; stack[top++] = s0; lab[s0] = n;
      int32_t* r = st7 + (n - 1) * 7;
      r[0] = 0; r[1] = D; r[2] = H; r[3] = W; r[4] = r[5] = r[6] = 0;
      while (top) {
        const int i = stack[--top], x = i % W, y = (i / W) % H, z = i / (W * H);
        r[0] += 1;
        if (z < r[1]) r[1] = z; if (y < r[2]) r[2] = y; if (x < r[3]) r[3] = x;
        if (z + 1 > r[4]) r[4] = z + 1; if (y + 1 > r[5]) r[5] = y + 1; if (x + 1 > r[6]) r[6] = x + 1;
        const int nb[6] = {z > 0 ? i - H * W : -1, z < D - 1 ? i + H * W : -1, y > 0 ? i - W : -1, y < H - 1 ? i + W : -1,
                           x > 0 ? i - 1 : -1, x < W - 1 ? i + 1 : -1};
        for (int k = 0; k < 6; ++k)
          if (nb[k] >= 0 && vol[nb[k]] && !lab[nb[k]]) { lab[nb[k]] = n; stack[top++] = nb[k]; }
      }
    }
    int32_t dims3[3] = {D, H, W}, nl[1] = {n};
    int64_t* bnd = (int64_t*)calloc((size_t)ML * 5, 8);
    OK(ics_op_component_bounds(lab, dims3, 1, nl, st7, ML, 3, 0.0, bnd));
    OK(ics_op_component_bounds(lab, dims3, 1, nl, st7, ML, 0, 0.3, bnd));
    OK(ics_op_component_bounds(lab, dims3, 1, nl, st7, ML, 3, 0.8, bnd));
    int exact = 0;
    for (int c = 0; c < n; ++c) {
      if (st7[c * 7] > 3 && !(bnd[c * 5 + 1] >= bnd[c * 5 + 2] && bnd[c * 5 + 2] >= bnd[c * 5])) { fprintf(stderr, "bounds out of order\n"); return 1; }
      if (bnd[c * 5 + 4]) { ++exact; if (bnd[c * 5 + 4] > bnd[c * 5 + 1] || bnd[c * 5 + 4] < bnd[c * 5 + 2]) { fprintf(stderr, "hull count outside its bounds\n"); return 1; } }
    }
    if (exact == 0) { fprintf(stderr, "the exact hull path was not exercised\n"); return 1; }
    /* every component as its own box {0, 1}, plus the whole volume: dozens of boxes through the thread pool */
    size_t tot = V; int nb = 1;
    for (int c = 0; c < n; ++c) tot += (size_t)(st7[c * 7 + 4] - st7[c * 7 + 1]) * (st7[c * 7 + 5] - st7[c * 7 + 2]) * (st7[c * 7 + 6] - st7[c * 7 + 3]);
    int32_t* boxes = (int32_t*)malloc(tot * 4);
    int32_t* out = (int32_t*)malloc(tot * 4);
    int32_t* bd = (int32_t*)malloc((size_t)(n + 1) * 3 * 4);
    int32_t* bc = (int32_t*)malloc((size_t)(n + 1) * 4);
    memcpy(boxes, vol, V * 4); bd[0] = D; bd[1] = H; bd[2] = W; bc[0] = 1;
    size_t off = V;
    for (int c = 0; c < n; ++c) {
      const int32_t* r = st7 + c * 7;
      const int bz = r[4] - r[1], by = r[5] - r[2], bx = r[6] - r[3];
      for (int z = 0; z < bz; ++z) for (int y = 0; y < by; ++y) for (int x = 0; x < bx; ++x)
        boxes[off + (z * by + y) * bx + x] = lab[((r[1] + z) * H + r[2] + y) * W + r[3] + x] == c + 1;
      bd[nb * 3] = bz; bd[nb * 3 + 1] = by; bd[nb * 3 + 2] = bx; bc[nb] = 1; ++nb;
      off += (size_t)bz * by * bx;
    }
    OK(ics_op_watershed_split(boxes, bd, bc, nb, 0, out));
    OK(ics_op_watershed_split(boxes, bd, bc, nb, 1, out));
    printf("asan driver: %d components, %d exact hull counts, %d boxes split on host threads\n", n, exact, nb);
    free(vol); free(lab); free(stack); free(st7); free(bnd); free(boxes); free(out); free(bd); free(bc);
  }
  {  /* boxes with an extent above 64 (whole grids at d >= 128): the host labeller next to a kernel box in one call, the
        host flood for the device form of the split, component bounds over the large box, and a refused stats row */
    enum { D = 70, H = 9, W = 11, V = D * H * W, ML = 64 };
    int32_t dims[6] = {D, H, W, 3, 4, 5};
    int32_t* vol = (int32_t*)calloc(V + 60, 4);
    int32_t* lab = (int32_t*)calloc(V + 60, 4);
    int32_t* wss = (int32_t*)calloc(V + 60, 4);
    int32_t* st = (int32_t*)calloc(2 * ML * 7, 4);
    int32_t nl[2], cls[2] = {1, 1};
    int64_t* bnd = (int64_t*)calloc(2 * ML * 5, 8);
    for (int z = 2; z < 68; ++z) for (int y = 1; y < 8; ++y) for (int x = 1; x < 10; ++x)      /* a bar with a notch */
      vol[(z * H + y) * W + x] = !(z > 30 && z < 40 && y < 5);
    vol[(0 * H + 0) * W + 0] = 1;
    vol[V + 7] = 1; vol[V + 8] = 1;
    OK(ics_op_label_boxes(vol, dims, 2, 1, ML, lab, nl, st));      /* (the kernel box's outputs are the stub's) */
    if (nl[0] != 2 || st[7] != 66 * 7 * 9 - 9 * 4 * 9 || st[8] != 2 || st[11] != 68) { fprintf(stderr, "large-box labels wrong\n"); return 1; }
    OK(ics_op_label_boxes(vol, dims, 2, 3, ML, lab, nl, NULL));
    setenv("ICSG3D_WS_DEVICE", "1", 1);
    OK(ics_op_watershed_split(vol, dims, cls, 2, 0, wss));
    unsetenv("ICSG3D_WS_DEVICE");
    OK(ics_op_watershed_split(vol, dims, cls, 2, 1, wss));
    setenv("ICSG3D_LABEL_HOST", "1", 1);      /* every box on the host labeller */
    OK(ics_op_label_boxes(vol, dims, 2, 1, ML, lab, nl, st));
    unsetenv("ICSG3D_LABEL_HOST");
    if (nl[0] != 2 || nl[1] != 1 || st[ML * 7] != 2) { fprintf(stderr, "host labeller wrong\n"); return 1; }
    OK(ics_op_component_bounds(lab, dims, 2, nl, st, ML, 3, 0.8, bnd));
    if (bnd[5 + 0] != st[7] || bnd[5 + 1] < bnd[5 + 2] || bnd[5 + 2] < bnd[5 + 0]) { fprintf(stderr, "large-box bounds wrong\n"); return 1; }
    st[7 + 4] = st[7 + 1];     /* an empty (inverted) z range for label 2 of box 0 */
    bnd[0] = -7;
    if (ics_op_component_bounds(lab, dims, 2, nl, st, ML, 3, 0.8, bnd) == 0 || bnd[0] != -7) { fprintf(stderr, "stats box check missing\n"); return 1; }
    printf("asan driver: large box labelled and bounded on host threads; %s\n", ics_last_error());
    free(vol); free(lab); free(wss); free(st); free(bnd);
  }
  printf("asan driver: all entry points walked, no sanitizer report\n");
  return 0;
}
