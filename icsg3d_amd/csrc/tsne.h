// Declarations for tsne.hip: the two-dimensional t-SNE map of a set of latent codes (the reference's viz.tsne_latent,
// i.e. sklearn.manifold.TSNE(n_components=2) at angle = 0): exact k nearest neighbours, the perplexity search, the
// symmetrised sparse affinities and gradient descent with exact (all-pairs) repulsion.
#pragma once
#include "common.h"
#include "icsg3d.h"

namespace ics {

constexpr int kTsneMaxPoints = 1 << 20;             // points per handle (time per iteration)
constexpr long long kTsneMaxEdges = 1LL << 28;      // n * k of one neighbour search (12 bytes each, twice that in CSR)
constexpr int kTsneMaxDim = 4096;

// ---- the handle (struct ics_tsne, defined in tsne.hip)
// rows of `dim` floats at src + r*stride_floats on the handle's device, ordered after the work already on src_stream
int tsne_append_device(ics_tsne* h, const float* src, size_t stride_floats, int rows, hipStream_t src_stream);
int tsne_device(const ics_tsne* h);
int tsne_dim(const ics_tsne* h);

}  // namespace ics
