// The grids create_matrices.py computes per crystal (reference create_matrices.py:117-190), on the device:
//   density M  and species S        utils.density_matrix   (reference utils.py:97-144)
//   coordinate grid p               utils.coordinate_grid  (reference utils.py:88-94)
//   90-degree rotations             utils.random_rotation_3d (reference utils.py:193-222)
// in the reference's exact semantics (no periodic images, lattice angles ignored, fp64 throughout).
//
// One block = one job (a structure + up to three quarter turns) x 1024 output voxels.  The job's sites are staged in LDS
// (wave-uniform reads, broadcast); each lane owns four output voxels, 256 apart, and loops over the sites keeping the
// in-radius count, the running argmin and the density sum.  A rotated job evaluates every output voxel at its SOURCE
// index (scipy.ndimage.rotate by 90 degrees with reshape=False is np.rot90: an index permutation), so writes stay in
// output order and no second pass exists.  DESIGN.md section 12.
#include "voxelise.h"
#include "orient.h"    // rot_source: the rotation convention, shared with the feed's rotating pack
#include "scratch.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

// The species decision compares D = sqrt(((dx*dx + dy*dy) + dz*dz)) -- scipy cdist's order -- against sigma*label_frac
// and against the other sites' D: with no fused multiply-adds D is bit-identical to the reference's, and so is every
// decision.  The voxel centres follow numpy.linspace's operations for the same reason.
#pragma clang fp contract(off)

namespace ics {
namespace {

constexpr int kVoxThreads = 256, kVoxPerThread = 4;
constexpr size_t kVoxOpBudget = (size_t)256 << 20;   // device bytes of fp64 output per ics_op_voxelise chunk
constexpr int kVoxOpMaxJobs = 1024;

struct VoxJob {
  double abc[3];
  int site0, nsites;   // rows of the site table
  int rot[3];          // indices into [(0,1), (0,2), (1,2)] applied in order, -1 = none
  int pad;
};

struct VoxOut {
  double *M, *S, *p;          // op: [job][d^3], [job][d^3], [job][d^3][3]; each optional
  float* x;                   // engine: [job][d^3][C]
  int C;
  unsigned char* labels;      // engine: [job][d^3], optional
};

struct Axis {
  double start, step, half, gstep;
};
// density_matrix: linspace(-a*eps, a + a*eps, d+1)[:-1] + dv/2 with dv = (a + 2*a*eps)/d  (utils.py:102-115);
// coordinate_grid: linspace(0, l + 2*eps*l, d+1)[:-1]                                       (utils.py:89-91)
__device__ __forceinline__ Axis make_axis(double a, double eps, int d) {
  Axis x;
  x.start = -a * eps;
  const double stop = a + a * eps;
  x.step = (stop - x.start) / d;
  x.half = ((a + 2.0 * a * eps) / d) / 2.0;
  x.gstep = (a + 2.0 * eps * a) / d;
  return x;
}
__device__ __forceinline__ double centre(const Axis& x, int i) { return ((double)i * x.step + x.start) + x.half; }

template <bool ENGINE>
__global__ __launch_bounds__(kVoxThreads) void voxelise_kernel(const double* __restrict__ sites,
                                                              const VoxJob* __restrict__ jobs, int d, double eps,
                                                              double norm, VoxOut out) {
  __shared__ double sh[kVoxMaxSites * kVoxSiteDoubles];
  const VoxJob& J = jobs[blockIdx.y];
  const int ns = J.nsites;
  const double* src = sites + (size_t)J.site0 * kVoxSiteDoubles;
  for (int i = threadIdx.x; i < ns * kVoxSiteDoubles; i += kVoxThreads) sh[i] = src[i];
  const Axis ax = make_axis(J.abc[0], eps, d), ay = make_axis(J.abc[1], eps, d), az = make_axis(J.abc[2], eps, d);
  const int r0 = J.rot[0], r1 = J.rot[1], r2 = J.rot[2];
  __syncthreads();

  const size_t V = (size_t)d * d * d;
  const size_t dd = (size_t)d * d;
#pragma unroll 1
  for (int t = 0; t < kVoxPerThread; ++t) {
    const size_t o = ((size_t)blockIdx.x * kVoxPerThread + t) * kVoxThreads + threadIdx.x;
    if (o >= V) break;
    int i = (int)(o / dd), j = (int)((o / d) % d), k = (int)(o % d);
    rot_source(r2, d, i, j, k);   // the last rotation applied is undone first
    rot_source(r1, d, i, j, k);
    rot_source(r0, d, i, j, k);
    const double vx = centre(ax, i), vy = centre(ay, j), vz = centre(az, k);

    double m = 0.0, best = INFINITY, zin = 0.0;
    int cnt = 0, bi = 0;
#pragma unroll 2
    for (int s = 0; s < ns; ++s) {
      const double* q = sh + s * kVoxSiteDoubles;
      const double dx = vx - q[0], dy = vy - q[1], dz = vz - q[2];
      const double D = sqrt(dx * dx + dy * dy + dz * dz);
      if (D < q[3]) { ++cnt; zin = q[4]; }     // D < sigma_s * label_frac (utils.py:122)
      if (D < best) { best = D; bi = s; }      // np.argmin: first of equal minima
      const double e = (D * D) * q[6];          // -D^2 / (2 sigma_s^2)        (utils.py:135-138)
      if (e > -746.0) m += exp(e) * q[5];       // exp(e) is 0 below; * Z_s / sigma_s^3
    }
    // utils.py:117-134: no site in radius -> 0; one -> that site; two or more -> the nearest of ALL sites
    const double S = cnt == 0 ? 0.0 : (cnt == 1 ? zin : sh[bi * kVoxSiteDoubles + 4]);
    const double M = norm * m;
    const size_t g = (size_t)blockIdx.y * V + o;
    if (ENGINE) {
      if (out.C == 4) {
        const float4 v = make_float4((float)M, (float)((double)i * ax.gstep), (float)((double)j * ay.gstep),
                                     (float)((double)k * az.gstep));
        *reinterpret_cast<float4*>(out.x + g * 4) = v;
      } else {
        out.x[g] = (float)M;
      }
      if (out.labels) out.labels[g] = (unsigned char)S;
    } else {
      if (out.M) out.M[g] = M;
      if (out.S) out.S[g] = S;
      if (out.p) {
        out.p[g * 3 + 0] = (double)i * ax.gstep;
        out.p[g * 3 + 1] = (double)j * ay.gstep;
        out.p[g * 3 + 2] = (double)k * az.gstep;
      }
    }
  }
}

// Site table + job records of jobs[0..n): each structure a job names is packed once, rows < nsites only.  Per site
// (create_matrices.py:140,150 done by the caller): x, y, z, sigma*label_frac, Z, Z/sigma**3, -1/(2*sigma**2), 0 -- the
// per-site factors exactly as numpy forms them (utils.py:136-137: `z / (sigma ** 3)`, `2 * sigma ** 2`).
void vox_pack(const ics_structures* s, const int32_t* jobs, int n, double label_frac, std::vector<unsigned char>* buf,
              size_t* job_off) {
  std::unordered_map<int, int> site0;
  std::vector<double> tab;
  std::vector<VoxJob> rec(n);
  for (int b = 0; b < n; ++b) {
    const int st = jobs[b * 4];
    const int ns = s->nsites[st];
    auto it = site0.find(st);
    int first;
    if (it != site0.end()) {
      first = it->second;
    } else {
      first = (int)(tab.size() / kVoxSiteDoubles);
      site0.emplace(st, first);
      for (int r = 0; r < ns; ++r) {
        const size_t row = (size_t)st * s->max_sites + r;
        const double sg = s->sigma[row], z = s->z[row];
        const double v[kVoxSiteDoubles] = {s->xyz[row * 3], s->xyz[row * 3 + 1], s->xyz[row * 3 + 2], sg * label_frac,
                                           z, z / std::pow(sg, 3.0), -1.0 / (2.0 * (sg * sg)), 0.0};
        tab.insert(tab.end(), v, v + kVoxSiteDoubles);
      }
    }
    VoxJob& J = rec[b];
    std::memset(&J, 0, sizeof(J));
    for (int a = 0; a < 3; ++a) J.abc[a] = s->abc[(size_t)st * 3 + a];
    J.site0 = first;
    J.nsites = ns;
    for (int a = 0; a < 3; ++a) J.rot[a] = jobs[b * 4 + 1 + a];
  }
  *job_off = align_up(tab.size() * sizeof(double), 256);
  buf->assign(*job_off + rec.size() * sizeof(VoxJob), 0);
  std::memcpy(buf->data(), tab.data(), tab.size() * sizeof(double));
  std::memcpy(buf->data() + *job_off, rec.data(), rec.size() * sizeof(VoxJob));
}

int vox_launch(hipStream_t st, bool engine, const unsigned char* dev, size_t job_off, int n, int d, double eps,
               const VoxOut& out) {
  const size_t V = (size_t)d * d * d;
  const unsigned gx = (unsigned)((V + (size_t)kVoxThreads * kVoxPerThread - 1) / ((size_t)kVoxThreads * kVoxPerThread));
  const double norm = 1.0 / std::pow(2.0 * M_PI, 1.5);   // 1 / (2 pi)^1.5 (utils.py:140)
  const double* sites = reinterpret_cast<const double*>(dev);
  const VoxJob* jobs = reinterpret_cast<const VoxJob*>(dev + job_off);
  if (engine)
    ICS_LAUNCH(voxelise_kernel<true>, dim3(gx, n), dim3(kVoxThreads), 0, st, sites, jobs, d, eps, norm, out);
  else
    ICS_LAUNCH(voxelise_kernel<false>, dim3(gx, n), dim3(kVoxThreads), 0, st, sites, jobs, d, eps, norm, out);
  ICS_HIP(hipGetLastError());
  return 0;
}

}  // namespace

int voxelise_check(const ics_structures* s, const int32_t* jobs, int njobs, int d, double eps_frac, double label_frac,
                   int ncls) {
  ICS_CHECK(s != nullptr, "null structures");
  ICS_CHECK(s->nsites && s->xyz && s->z && s->sigma && s->abc, "null structure array");
  ICS_CHECK(s->count >= 1 && s->max_sites >= 1, "structures: count and max_sites must be >= 1");
  ICS_CHECK(jobs != nullptr && njobs >= 1, "jobs: need a non-null [njobs][4] array, njobs >= 1");
  ICS_CHECK(d >= 2 && d <= 256, "grid edge d must be in [2, 256]");
  ICS_CHECK(std::isfinite(eps_frac) && eps_frac >= 0.0, "eps_frac must be finite and >= 0");
  ICS_CHECK(std::isfinite(label_frac) && label_frac >= 0.0, "label_frac must be finite and >= 0");
  const int lim = std::min(s->max_sites, kVoxMaxSites);
  std::vector<char> seen((size_t)s->count, 0);
  for (int b = 0; b < njobs; ++b) {
    const int st = jobs[b * 4];
    ICS_CHECK(st >= 0 && st < s->count, "job " + std::to_string(b) + ": structure index " + std::to_string(st) +
                                            " outside [0, " + std::to_string(s->count) + ")");
    for (int a = 1; a < 4; ++a)
      ICS_CHECK(jobs[b * 4 + a] >= -1 && jobs[b * 4 + a] <= 2,
                "job " + std::to_string(b) + ": rotation index " + std::to_string(jobs[b * 4 + a]) + " not in {-1,0,1,2}");
    if (seen[st]) continue;
    seen[st] = 1;
    const std::string who = "structure " + std::to_string(st);
    const int ns = s->nsites[st];
    ICS_CHECK(ns >= 1 && ns <= lim, who + ": nsites " + std::to_string(ns) + " outside [1, " + std::to_string(lim) + "]");
    for (int a = 0; a < 3; ++a) {
      const double l = s->abc[(size_t)st * 3 + a];
      ICS_CHECK(std::isfinite(l) && l > 0.0, who + ": lattice lengths must be finite and > 0");
    }
    for (int r = 0; r < ns; ++r) {
      const size_t row = (size_t)st * s->max_sites + r;
      const double sg = s->sigma[row], z = s->z[row];
      ICS_CHECK(std::isfinite(s->xyz[row * 3]) && std::isfinite(s->xyz[row * 3 + 1]) && std::isfinite(s->xyz[row * 3 + 2]),
                who + ", site " + std::to_string(r) + ": coordinates must be finite");
      ICS_CHECK(std::isfinite(sg) && sg > 0.0, who + ", site " + std::to_string(r) + ": sigma must be finite and > 0");
      ICS_CHECK(std::isfinite(z) && z >= 0.0, who + ", site " + std::to_string(r) + ": Z must be finite and >= 0");
      if (ncls > 0)
        ICS_CHECK(z == std::floor(z) && z < ncls, who + ", site " + std::to_string(r) + ": Z " + std::to_string(z) +
                                                      " is not a class id in [0, " + std::to_string(ncls) + ")");
    }
  }
  return 0;
}

VoxStage::~VoxStage() {
  if (ev) { (void)hipEventSynchronize(ev); (void)hipEventDestroy(ev); }
  if (dev) (void)hipFree(dev);
  if (host) (void)hipHostFree(host);
}

int voxelise_engine(hipStream_t st, VoxStage& stage, const ics_structures* s, const int32_t* jobs, int batch, int d,
                    double eps_frac, double label_frac, float* x, int C, unsigned char* labels, const VoxBlob* blobs,
                    int nblob) {
  ICS_CHECK(C == 1 || C == 4, "voxelise feeds 1 (M) or 4 (M, p) input channels");
  std::vector<unsigned char> buf;
  size_t job_off = 0;
  vox_pack(s, jobs, batch, label_frac, &buf, &job_off);
  std::vector<size_t> blob_off(nblob);
  for (int b = 0; b < nblob; ++b) {
    blob_off[b] = align_up(buf.size(), 256);
    buf.resize(blob_off[b] + blobs[b].bytes);
    std::memcpy(buf.data() + blob_off[b], blobs[b].host, blobs[b].bytes);
  }
  if (!stage.ev) ICS_HIP(hipEventCreateWithFlags(&stage.ev, hipEventDisableTiming));
  ICS_HIP(hipEventSynchronize(stage.ev));   // the previous batch's upload has left the pinned buffer
  if (buf.size() > stage.cap) {
    if (stage.dev) { ICS_HIP(hipStreamSynchronize(st)); (void)hipFree(stage.dev); stage.dev = nullptr; }
    if (stage.host) { (void)hipHostFree(stage.host); stage.host = nullptr; }
    stage.cap = 0;
    const size_t cap = std::max(buf.size() * 2, (size_t)1 << 16);
    ICS_HIP(hipHostMalloc(reinterpret_cast<void**>(&stage.host), cap, 0));
    ICS_HIP(hipMalloc(reinterpret_cast<void**>(&stage.dev), cap));
    stage.cap = cap;
  }
  std::memcpy(stage.host, buf.data(), buf.size());
  ICS_HIP(hipMemcpyAsync(stage.dev, stage.host, buf.size(), hipMemcpyHostToDevice, st));
  ICS_HIP(hipEventRecord(stage.ev, st));
  for (int b = 0; b < nblob; ++b)
    ICS_HIP(hipMemcpyAsync(blobs[b].dev, stage.dev + blob_off[b], blobs[b].bytes, hipMemcpyDeviceToDevice, st));
  VoxOut out{nullptr, nullptr, nullptr, x, C, labels};
  return vox_launch(st, true, stage.dev, job_off, batch, d, eps_frac, out);
}

}  // namespace ics

using namespace ics;

// Host-pointer op: fp64 M / S [njobs][d][d][d], p [njobs][d][d][d][3] (each optional), chunked under a device-memory
// budget through the calling thread's scratch (scratch.h); synchronous.
extern "C" int ics_op_voxelise(const ics_structures* s, const int32_t* jobs, int njobs, int d, double eps_frac,
                               double label_frac, double* M, double* S, double* p) {
  ICS_TRY(voxelise_check(s, jobs, njobs, d, eps_frac, label_frac, 0));
  hipStream_t st;
  ICS_TRY(op_stream(&st));
  if (!M && !S && !p) return 0;
  const size_t V = (size_t)d * d * d;
  const size_t per_job = V * sizeof(double) * ((M ? 1 : 0) + (S ? 1 : 0) + (p ? 3 : 0));
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>(kVoxOpMaxJobs, kVoxOpBudget / per_job));
  std::vector<unsigned char> buf;
  for (int j0 = 0; j0 < njobs; j0 += chunk) {
    const int n = std::min(chunk, njobs - j0);
    size_t job_off = 0;
    vox_pack(s, jobs + (size_t)j0 * 4, n, label_frac, &buf, &job_off);
    const size_t nV = (size_t)n * V;
    Layout L;
    const auto s_in = L.add<unsigned char>(buf.size());
    const auto s_M = L.add<double>(M ? nV : 0);
    const auto s_S = L.add<double>(S ? nV : 0);
    const auto s_p = L.add<double>(p ? 3 * nV : 0);
    unsigned char* din;
    double *dM, *dS, *dp;
    ICS_TRY(L.reserve(s_in, &din, s_M, &dM, s_S, &dS, s_p, &dp));
    ICS_TRY(L.upload(s_in, buf.data(), buf.size(), st));
    VoxOut out{dM, dS, dp, nullptr, 0, nullptr};
    ICS_TRY(vox_launch(st, false, din, job_off, n, d, eps_frac, out));
    if (M) ICS_TRY(L.download(M + (size_t)j0 * V, s_M, nV, st));
    if (S) ICS_TRY(L.download(S + (size_t)j0 * V, s_S, nV, st));
    if (p) ICS_TRY(L.download(p + (size_t)j0 * V * 3, s_p, 3 * nV, st));
    ICS_HIP(hipStreamSynchronize(st));
  }
  return 0;
}
