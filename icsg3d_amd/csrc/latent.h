// Declarations for latent.hip: the walk between two latent codes of interpolate.py (reference interpolate.py:54-59),
// written as rows of the decoder's dense input zc = [z | cond].
#pragma once
#include "common.h"

namespace ics {

enum LatentMode : int { LATENT_LERP = 0, LATENT_SLERP = 1 };
constexpr double kSlerpMinSin = 1e-3;   // below it (parallel / antiparallel codes) a slerp pair takes the lerp

// The argument rules shared by ics_op_latent_path and the ics_vae_interpolate* chains: counts >= 1, alpha finite, a
// known mode.  0, or -1 with the error set naming the argument (`who` prefixes the message).
int latent_path_check(const char* who, int pairs, int latent, const double* alpha, int steps, int mode);
// Enqueue latent_path_kernel on st, DEVICE pointers: pair p reads za + p*z_stride and zb + p*z_stride (latent floats
// each) and cond + p*cond_stride (ncond floats; unread when ncond == 0), and writes for step k
//   zc  [(p*steps + k)*(latent + ncond)] = [code | cond]      (or nullptr)
//   path[(p*steps + k)*latent]           = code               (or nullptr)
// d_alpha: steps doubles on the device.
int launch_latent_path(hipStream_t st, const float* za, const float* zb, size_t z_stride, const float* cond,
                       size_t cond_stride, int ncond, int pairs, int latent, const double* d_alpha, int steps, int mode,
                       float* zc, float* path);

}  // namespace ics
