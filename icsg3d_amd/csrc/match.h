// Declarations for match.hip: the exact minimum-cost one-to-one matching behind eval.py's emd() (reference
// eval.py:45-53: cdist + linear_sum_assignment), batched on the device.
#pragma once
#include "common.h"

namespace ics {

constexpr int kMatchMaxPoints = 2048;   // points per set (MAX_SITES true sites, generate.py's max_atoms)

// The argument rules of ics_op_match_emd (include/icsg3d.h), every sample checked before anything is written: 0, or -1
// with the error set naming the sample.
int match_emd_check(const double* a, const int32_t* a_off, const double* b, const int32_t* b_off, int batch,
                    const double* emd);
// Host-pointer op behind ics_op_match_emd on arguments match_emd_check accepted: the batch solved in chunks under a
// device-memory budget through the calling thread's scratch; synchronous on st.
int match_emd_op(hipStream_t st, const double* a, const int32_t* a_off, const double* b, const int32_t* b_off,
                 int batch, double* emd, int32_t* match);

}  // namespace ics
