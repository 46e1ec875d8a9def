// Declarations for voxelise.hip: the density / species / coordinate grids of create_matrices.py
// (reference utils.py:88-144, rotations :193-222) computed on the device.
#pragma once
#include "common.h"
#include "../../include/icsg3d.h"

namespace ics {

constexpr int kVoxMaxSites = 256;   // sites per structure staged in LDS
constexpr int kVoxSiteDoubles = 8;  // per site: x, y, z, sigma*label_frac, Z, Z/sigma^3, -1/(2 sigma^2), 0

// Validates structures, jobs and parameters (every structure a job names, rows < nsites only).  ncls > 0: Z must
// also be an integer in [0, ncls) (the U-Net's class ids).  Returns 0 or sets the error.
int voxelise_check(const ics_structures* s, const int32_t* jobs, int njobs, int d, double eps_frac,
                   double label_frac, int ncls);

// Per-engine staging of one batch's site table: pinned host memory, a device copy, and the event of the last upload
// (the host waits on it before it rewrites the pinned buffer).
struct VoxStage {
  unsigned char* host = nullptr;
  unsigned char* dev = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;
  VoxStage() = default;
  VoxStage(const VoxStage&) = delete;
  VoxStage& operator=(const VoxStage&) = delete;
  ~VoxStage();
};

// A host array that travels with the site table through the pinned staging buffer to `dev` (the VAE's cond / eps).
struct VoxBlob {
  const void* host;
  void* dev;
  size_t bytes;
};

// Engine feed: jobs [batch][4] (validated) -> x [batch][d^3][C] float32 (channel 0 = M, 1..3 = p when C == 4) and,
// when labels != nullptr, labels [batch][d^3] uint8 = S; the nblob blobs are copied too.  Enqueued on st; returns
// without waiting for the kernel.
int voxelise_engine(hipStream_t st, VoxStage& stage, const ics_structures* s, const int32_t* jobs, int batch, int d,
                    double eps_frac, double label_frac, float* x, int C, unsigned char* labels, const VoxBlob* blobs,
                    int nblob);

}  // namespace ics
