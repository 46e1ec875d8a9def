// Declarations for atomscore.hip: predicted atoms matched to true atoms sample by sample and tallied per species on the
// device (include/icsg3d.h, "atom score").
//
// THE RULE.  A sample has n true and m predicted atoms, each a position (fp64, voxel units) and a species id in [0, ncls).
//   d2(i, j) = ((dx * dx + dy * dy) + dz * dz), dx = t.x - p.x and so on, in fp64, this order, no FMA contraction.
//   A pair is admissible when d2 < tol2, strictly.  The matching is the greedy one under the strict total order
//   (d2, true index, predicted index): walk the admissible pairs in ascending order, take a pair when both atoms are free.
//   The kernel computes it as synchronous mutual-best rounds (every free true atom picks its smallest admissible free
//   partner by (d2, j), every free predicted atom its smallest by (d2, i); pairs that pick each other are matched; rounds
//   repeat until one matches nothing): the same set of pairs, no sort, no tie ambiguity.
//
// THE ACCUMULATOR: atom_acc_len(ncls) uint64 on the device, ADDED to (zero it first for the tallies of one call).
// K = ncls + 1, index ncls = "no atom":
//   [t * K + p]                      matched pairs by (true species, predicted species); [t * K + ncls] unmatched true atoms
//                                    (missed); [ncls * K + p] unmatched predicted atoms (spurious); [ncls * K + ncls] stays 0
//   [K * K + s]                      dist_q:   sum over matched pairs of true species s of llrint(sqrt(d2) * 2^20)
//   [K * K + ncls + s]               dist2_q:  the same of llrint(d2 * 2^20)
//   [K * K + 2 ncls + s]             dup:      unmatched predicted atoms of species s with some true atom within tol
//   [K * K + 3 ncls + s]             shadowed: unmatched true atoms of species s with some predicted atom within tol
//   [K * K + 4 ncls + b]             hist, b < 16: matched pairs with min(15, (int)floor(sqrt(d2) * hist_scale)) == b
//   [K * K + 4 ncls + 16 + k]        totals, k < 8: samples, failed, perfect, true atoms, predicted atoms, matched,
//                                    sum |n - m|, samples with no true atom
// sqrt is the correctly rounded fp64 one, llrint rounds half to even: integer sums, so no order can change them.
// A FAILED sample (statistics rows only: more kept components than max_atoms on either side) adds to samples and failed
// and to nothing else.
//
// PER-SAMPLE OUTPUTS (each optional): match [true atom] = the partner's index within the sample or -1;
// sample_stats [b][6] = {n, m, matched, species_agree, dup, shadowed} ({n, m, -1, -1, -1, -1} for a failed sample);
// dist_sum [b] = the sum of sqrt(d2) over the matched pairs in ascending true index, added serially (NaN when failed).
//
// THE GRID: one workgroup of kAtomScoreThreads lanes per sample.  Positions, species, picks and partners of both sides
// live in dynamic LDS, atom_score_lds_bytes(cap) for samples of at most cap atoms a side: 73 760 bytes at the limit of
// kAtomScoreMaxAtoms, raised above the 64 KiB default with hipFuncSetAttribute (a CU has 160 KiB).  The round loop ends
// when a round matches nothing and is bounded by min(n, m) rounds besides.
#pragma once
#include "common.h"

namespace ics {

constexpr int kAtomScoreThreads = 256, kAtomScoreMaxAtoms = 1024, kAtomScoreHistBins = 16, kAtomScoreTotals = 8;
constexpr int kAtomScoreMinCls = 2, kAtomScoreMaxCls = 127;
constexpr double kAtomScoreMaxCoord = 1e150;   // |coordinate| limit: d2 stays finite
constexpr double kAtomScoreMaxTol = 1e6;       // tol limit: llrint(d2 * 2^20) stays below 2^63
constexpr double kAtomScoreFix = 1048576.0;    // 2^20, the fixed-point scale of dist_q / dist2_q

constexpr size_t atom_acc_len(int ncls) {
  return (size_t)(ncls + 1) * (ncls + 1) + 4 * (size_t)ncls + kAtomScoreHistBins + kAtomScoreTotals;
}
// per side and atom: 3 doubles, species, pick, partner (36 bytes); 8 int counters behind the two sides
constexpr size_t atom_score_lds_bytes(int cap) { return (size_t)cap * 72 + 32; }

struct AtomScoreOut {
  unsigned long long* acc;   // required
  int* match;                // or nullptr
  int* sample_stats;         // or nullptr
  double* dist_sum;          // or nullptr
};

// Ragged sets: xyz [off[batch]][3] fp64, species [off[batch]] int32, off [batch + 1] (the layout ics_op_match_emd takes), all
// on the device and already validated: every set at most cap <= kAtomScoreMaxAtoms atoms.  match is indexed like t_species.
int launch_atom_score_ragged(hipStream_t st, const double* t_xyz, const int* t_species, const int* t_off, const double* p_xyz,
                             const int* p_species, const int* p_off, int batch, int ncls, double tol2, double hist_scale,
                             int cap, const AtomScoreOut& out);
// The statistics rows launch_segment_atoms leaves on the device: stats int32 [batch][max_atoms][kSegStatInts], counts int32
// [batch][2] ({components, kept components}).  Atom a of sample b has species stats[0] and the position
// (x, y, z) = ((double)sum x / (double)voxels, sum y / voxels, sum z / voxels), one correctly rounded division each.
// A sample whose kept components exceed max_atoms on either side is failed.  match is [batch][max_atoms].
int launch_atom_score_stats(hipStream_t st, const int* t_stats, const int* t_counts, const int* p_stats, const int* p_counts,
                            int batch, int max_atoms, int ncls, double tol2, double hist_scale, const AtomScoreOut& out);

// the argument rules tol, ncls share between the ops and the engine's accumulator; *tol2 and *hist_scale for the launches
int atom_score_params(const std::string& who, int ncls, double tol, double* tol2, double* hist_scale);

}  // namespace ics
