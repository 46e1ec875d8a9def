// Declarations for structure_symmetry.hip: the symmetry operations of a structure -- the structure tested against itself
// under the integer operations its own lattice admits -- and the group built from them (closure, orbits, projection onto
// the symmetric structure).  The predicate is the project's own; include/icsg3d.h states it in full under
// ics_op_structure_symmetry.  structure_match.hip compares PAIRS of structures under signed axis permutations and is left
// as it is; the device helpers the two share in spirit (nearest-atom scan, tag exchange, ordered sums) are restated here.
#pragma once
#include "common.h"

namespace ics {

constexpr int kSymMaxAtoms = 256;      // atoms per structure: one thread per atom
constexpr int kSymSmall = 64;          // atoms one wave takes
constexpr int kSymLatCap = 64;         // admissible lattice operations kept per structure
constexpr int kSymMaxSpecies = 94;
constexpr int kSymMaxOpsLimit = 4096;  // largest max_ops accepted
constexpr int kSymCodes = 19683;       // 3^9 matrices with entries in {-1, 0, 1}
constexpr int kSymIdentityCode = 16484;

// code = sum_k (W[k/3][k%3] + 1) 3^(8-k)  ->  W, row-major
__host__ __device__ inline void sym_decode(int code, int w[9]) {
  for (int k = 8; k >= 0; --k) { w[k] = code % 3 - 1; code /= 3; }
}
__host__ __device__ inline int sym_det(const int w[9]) {
  return w[0] * (w[4] * w[8] - w[5] * w[7]) - w[1] * (w[3] * w[8] - w[5] * w[6]) + w[2] * (w[3] * w[7] - w[4] * w[6]);
}
// index into the rotation-type histogram (-6, -4, -3, -2, -1, 1, 2, 3, 4, 6), or -1 for a (det, trace) in no row of the table
__host__ __device__ inline int sym_type_index(const int w[9]) {
  const int det = sym_det(w), tr = w[0] + w[4] + w[8];
  if (det == 1) return tr == 3 ? 5 : (tr >= -1 && tr <= 2 ? 7 + tr : -1);
  if (det == -1) return tr == -3 ? 4 : (tr >= -2 && tr <= 1 ? 2 + tr : -1);
  return -1;
}

// The argument rules of ics_op_structure_symmetry, every structure checked before anything is written: 0, or -1 with
// the error set naming the structure.
int structure_symmetry_check(const int32_t* offsets, const int32_t* species, const double* frac, const double* lattice,
                             const int32_t* eligible, int ns, double tol, double ltol, int max_ops);
// Host-pointer op on arguments structure_symmetry_check accepted: eligible structures sorted by atom count on the host,
// one upload, lattice operations for all of them, then per chunk of structures (candidate table, nearest-atom maps and
// operation lists under kSymChunkBytes; ICSG3D_SYMMETRY_CHUNK_BYTES shrinks it) the operation, scan and group kernels;
// synchronous on st.
int structure_symmetry_op(hipStream_t st, const int32_t* offsets, const int32_t* species, const double* frac,
                          const double* lattice, const int32_t* eligible, int ns, double tol, double ltol, int max_ops,
                          int32_t* n_lat, int32_t* n_ops, int32_t* n_point, int32_t* n_trans, int32_t* types,
                          int32_t* reason, int32_t* op_code, int32_t* op_anchor, double* op_t, double* op_rms,
                          int32_t* orbit, int32_t* mult, double* sym_frac, double* sym_G, double* sym_shift,
                          double* sym_resid);

}  // namespace ics
