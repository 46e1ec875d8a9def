// Declarations for structure.hip: the periodic structure behind generate.py's CIF stage (reference generate.py:250-263,
// utils.py:225-239: to_pymatgen_structure + structure.formula + structure.is_valid()), batched on the device.
#pragma once
#include "common.h"

namespace ics {

constexpr int kStructMaxAtoms = 2048;   // atoms per structure (generate.py's max_atoms)
constexpr int kStructMaxImage = 32;     // lattice translations searched per axis: |n| <= 32
constexpr int kStructHist = 95;         // histogram row: atomic numbers 0..94 (0 is never counted)
constexpr double kStructMaxCoord = 1e150;

// reason bits of an invalid structure (ics_op_structure_screen's `reason`)
constexpr int kStructReasonClose = 1;     // a pair at or under tol
constexpr int kStructReasonSpecies = 2;   // a species outside 1..94
constexpr int kStructReasonEmpty = 4;     // no atoms

// Per structure: the lattice of Lattice.from_parameters (rows va, vb, vc), its volume and the norms of the columns of
// its inverse.  0, or -1 where the six parameters make no cell.
int structure_cell(const double abc[3], const double angles[3], double M[9], double* volume, double g[3]);
// The argument rules of ics_op_structure_screen (include/icsg3d.h), every structure checked before anything is written:
// 0, or -1 with the error set naming the structure.
int structure_screen_check(const int32_t* offsets, const int32_t* species, const double* xyz, const double* abc,
                           const double* angles, int batch, double tol);
// Host-pointer op on arguments structure_screen_check accepted: chunked under a device-memory budget through the
// calling thread's scratch, one upload, at most two launches and one download per chunk; synchronous on st.
int structure_screen_op(hipStream_t st, const int32_t* offsets, const int32_t* species, const double* xyz,
                        const double* abc, const double* angles, int batch, double tol, double* lattice,
                        double* volume, double* frac, double* min_dist, int32_t* min_pair, int32_t* n_close,
                        int32_t* valid, int32_t* reason, double* nearest, int32_t* hist);

}  // namespace ics
