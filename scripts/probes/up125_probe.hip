// Step 0 of the 125-product up-split backward (csrc/up125.h): do the class GEMMs alone undercut the 27-tap GEMMs?
// Times, on dummy data, per layer (c17: rows 16384, Cout 128, Cu 128; c15: rows 2048, Cout 256, Cu 256; rows = B (S/4)^3):
//   backward-data   launch_gemm_zbatch at the four class groups (nb = 8, 4, 2, 1 blocks; nz = 8, 12, 6, 1 classes;
//                   K = nb Cout, N = Cu) against ONE plain GEMM of the 27-tap shape (M = 8 rows, K = 27 Cout)
//   backward-weight launch_conv_wgrad (GEMM phase only) once per class, [rows][Cu]^T x [rows][nb Cout], against the 27-tap
//                   shape (M = 8 rows, N = 27 Cout).  One launch per class is the UPPER bound of a z-batched launch.
// hipcc --offload-arch=gfx950 -O3 -I icsg3d_amd/csrc -I include up125_probe.hip -L icsg3d_amd -licsg3d_hip
#include "common.h"
#include <algorithm>
#include <cstdlib>

using namespace ics;

#define HIPOK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { fprintf(stderr, "%s -> %s\n", #e, hipGetErrorString(_e)); exit(2); } } while (0)
#define OK(e) do { if ((e) != 0) { fprintf(stderr, "%s failed\n", #e); exit(3); } } while (0)

__global__ void fill_kernel(float* p, size_t n, unsigned seed) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned h = (unsigned)i * 2654435761u + seed;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    p[i] = (float)(h & 0xffff) * (1.f / 65536.f) - 0.5f;
  }
}
static float* dalloc(size_t n, unsigned seed) {
  float* p = nullptr;
  HIPOK(hipMalloc(&p, n * sizeof(float)));
  fill_kernel<<<2048, 256>>>(p, n, seed);
  HIPOK(hipDeviceSynchronize());
  return p;
}

template <class F>
static double time_us(hipStream_t st, F&& f, int reps = 10) {
  hipEvent_t e0, e1;
  HIPOK(hipEventCreate(&e0)); HIPOK(hipEventCreate(&e1));
  std::vector<double> t;
  for (int r = 0; r < reps + 2; ++r) {
    HIPOK(hipEventRecord(e0, st));
    f();
    HIPOK(hipEventRecord(e1, st));
    HIPOK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPOK(hipEventElapsedTime(&ms, e0, e1));
    if (r >= 2) t.push_back(ms * 1e3);
  }
  std::sort(t.begin(), t.end());
  HIPOK(hipEventDestroy(e0)); HIPOK(hipEventDestroy(e1));
  return t[t.size() / 2];
}

static void layer(hipStream_t st, const char* name, int rows, int Cout, int Cu) {
  const int nbs[4] = {8, 4, 2, 1}, nzs[4] = {8, 12, 6, 1};
  const size_t nP = (size_t)125 * rows * Cout, nW = (size_t)125 * Cout * Cu, nO = (size_t)27 * rows * Cu;
  float* P = dalloc(std::max(nP, (size_t)8 * rows * 27 * Cout), 1);   // pooled dy (either form)
  float* W = dalloc(std::max(nW, (size_t)27 * Cout * Cu), 2);
  float* O = dalloc(std::max(nO, (size_t)8 * rows * Cu), 3);
  float* X = dalloc(nO, 4);
  printf("## %s: rows %d, Cout %d, Cu %d\n", name, rows, Cout, Cu);
  // ---- backward-data
  const double d27 = time_us(st, [&] { OK(launch_gemm_zbatch(st, 1, 8 * rows, 27 * Cout, Cu, P, W, O, 0)); });
  printf("dgrad 27-tap form  M %7d K %5d N %4d          %8.1f us\n", 8 * rows, 27 * Cout, Cu, d27);
  double dsum = 0;
  size_t po = 0, wo = 0, oo = 0;
  for (int gi = 0; gi < 4; ++gi) {
    const int nb = nbs[gi], nz = nzs[gi], K = nb * Cout;
    const float *Pg = P + po, *Wg = W + wo; float* Og = O + oo;
    const double t = time_us(st, [&] { OK(launch_gemm_zbatch(st, nz, rows, K, Cu, Pg, Wg, Og, 0)); });
    printf("dgrad class group  M %7d K %5d N %4d nz %2d    %8.1f us   %s\n", rows, K, Cu, nz, t, conv_last_kernel_id());
    dsum += t;
    po += (size_t)nz * rows * K; wo += (size_t)nz * K * Cu; oo += (size_t)nz * rows * Cu;
  }
  printf("dgrad class GEMMs together %8.1f us against %8.1f us (%.2f)\n", dsum, d27, dsum / d27);
  // ---- backward-weight
  {
    const ConvGeom g{8 * rows, 1, 0, Cu, 27 * Cout, 1, Cu, 27 * Cout, 0};
    const ConvSrc sx{X, nullptr, nullptr, Cu, 0, ACT_NONE, 0};
    const size_t wsn = conv_wgrad_workspace_floats(g, &sx, 1);
    float* ws = dalloc(wsn, 5);
    float* dw = dalloc((size_t)Cu * 27 * Cout, 6);
    // X has 27 rows x Cu floats; the 27-tap form reads 8 rows x Cu: inside it
    const double w27 = time_us(st, [&] { OK(launch_conv_wgrad(st, g, &sx, 1, P, 27 * Cout, dw, 27 * Cout, ws, wsn, 0, 0, 0, 1)); });
    printf("wgrad 27-tap form  M %7d K %5d N %5d  ws %zu MB   %8.1f us   %s\n", 8 * rows, Cu, 27 * Cout, wsn * 4 >> 20, w27,
           conv_last_kernel_id());
    HIPOK(hipFree(ws));
    double wsum = 0;
    po = 0;
    int cls = 0;
    for (int gi = 0; gi < 4; ++gi) {
      const int nb = nbs[gi], nz = nzs[gi], N = nb * Cout;
      const ConvGeom gc{rows, 1, 0, Cu, N, 1, Cu, N, 0};
      const size_t wn = conv_wgrad_workspace_floats(gc, &sx, 1);
      float* wsc = dalloc(wn, 7);
      const float* Pg = P + po;
      const int cls0 = cls;
      const double t = time_us(st, [&] {
        for (int z = 0; z < nz; ++z) {
          const ConvSrc sz{X + (size_t)(cls0 + z) * rows * Cu, nullptr, nullptr, Cu, 0, ACT_NONE, 0};
          OK(launch_conv_wgrad(st, gc, &sz, 1, Pg + (size_t)z * rows * N, N, dw, N, wsc, wn, 0, 0, 0, 1));
        }
      });
      printf("wgrad class group  M %7d K %5d N %5d nz %2d (one launch per class, ws %zu KB each)  %8.1f us   %s\n", rows, Cu, N,
             nz, wn * 4 >> 10, t, conv_last_kernel_id());
      wsum += t;
      po += (size_t)nz * rows * N;
      cls += nz;
      HIPOK(hipFree(wsc));
    }
    printf("wgrad class GEMMs together %8.1f us against %8.1f us (%.2f)\n", wsum, w27, wsum / w27);
    HIPOK(hipFree(dw));
  }
  HIPOK(hipFree(P)); HIPOK(hipFree(W)); HIPOK(hipFree(O)); HIPOK(hipFree(X));
  fflush(stdout);
}

int main() {
  hipStream_t st;
  HIPOK(hipStreamCreate(&st));
  layer(st, "c17", 16384, 128, 128);
  layer(st, "c15", 2048, 256, 256);
  layer(st, "c13", 256, 512, 512);
  HIPOK(hipStreamDestroy(st));
  return 0;
}
