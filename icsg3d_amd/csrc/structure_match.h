// Declarations for structure_match.hip: which generated crystals are the same structure (duplicates inside a run) and
// which are a structure of the training set, by the project's own predicate -- include/icsg3d.h states it in full under
// ics_op_structure_match.  match.hip is the EMD assignment of eval.py and has nothing to do with this file.
//
// Operation order (kMatchOps = 48 signed axis permutations P, f'_k = sign_k f[perm_k]): lexicographic over (permutation,
// sign pattern) -- permutations (0,1,2) (0,2,1) (1,0,2) (1,2,0) (2,0,1) (2,1,0), and per permutation the sign patterns
// (+,+,+) (+,+,-) (+,-,+) (+,-,-) (-,+,+) (-,+,-) (-,-,+) (-,-,-).  Index 0 is the identity.  ops_mode 0 keeps index 0,
// ops_mode 1 the 24 of determinant +1 in that order, ops_mode 2 all 48; a reported `op` indexes the mode's own list.
#pragma once
#include "common.h"

namespace ics {

constexpr int kMatchMaxAtoms = 256;   // atoms per structure: one thread per atom of A
constexpr int kMatchSmall = 64;       // atoms one wave takes
constexpr int kMatchOps = 48;
constexpr int kMatchMaxSpecies = 94;

// The op list of `ops_mode` (0..2) in the documented order: perm[k][3], sign[k][3]; returns the count (1, 24, 48).
int structure_match_ops(int ops_mode, int perm[][3], int sign[][3]);
// The argument rules of ics_op_structure_match, every structure checked before anything is written: 0, or -1 with the
// error set naming the structure.
int structure_match_check(const int32_t* offsets, const int32_t* species, const double* frac, const double* lattice,
                          const int32_t* eligible, int nq, int nref, double tol, double ltol, int ops_mode);
// Host-pointer op on arguments structure_match_check accepted: structures ordered by composition key on the host, pairs
// enumerated on the device from the bucket ranges, pair results chunked under kMatchChunkPairs (ICSG3D_MATCH_CHUNK_PAIRS
// shrinks it); synchronous on st.
int structure_match_op(hipStream_t st, const int32_t* offsets, const int32_t* species, const double* frac,
                       const double* lattice, const int32_t* eligible, int nq, int nref, double tol, double ltol,
                       int ops_mode, int32_t* dup_of, double* dup_rms, int32_t* dup_op, int32_t* ref_of,
                       double* ref_rms, int32_t* ref_op, int32_t* n_cmp);

}  // namespace ics
