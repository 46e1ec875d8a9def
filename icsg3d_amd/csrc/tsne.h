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

// ---- the two ops (HOST pointers, synchronous on st; arguments checked before anything is written)
// idx [n][k] int32, dist2 [n][k] fp64: the k nearest other rows of each row of x [n][dim] under the squared euclidean
// distance accumulated in fp64 in dimension order, sorted by (distance, index).
int tsne_knn_check(const float* x, int n, int dim, int k, const int32_t* idx, const double* dist2);
int tsne_knn_op(hipStream_t st, const float* x, int n, int dim, int k, int32_t* idx, double* dist2);
// cond_p [n][k]: sklearn.manifold._utils._binary_search_perplexity on float32(dist2).
int tsne_affinities_check(const double* dist2, int n, int k, double perplexity, const double* cond_p);
int tsne_affinities_op(hipStream_t st, const double* dist2, int n, int k, double perplexity, double* cond_p);

// ---- the handle (struct ics_tsne, defined in tsne.hip)
int tsne_create(const ics_tsne_config* cfg, ics_tsne** out);
int tsne_destroy(ics_tsne* h);
int tsne_append_host(ics_tsne* h, const float* codes, int rows);
// rows of `dim` floats at src + r*stride_floats on the handle's device, ordered after the work already on src_stream
int tsne_append_device(ics_tsne* h, const float* src, size_t stride_floats, int rows, hipStream_t src_stream);
int tsne_get_codes(ics_tsne* h, float* out, int rows);
int tsne_prepare(ics_tsne* h, const float* init, int init_rows, int init_cols, double seconds[3]);
int tsne_set_graph(ics_tsne* h, int n, const int64_t* indptr, const int32_t* indices, const double* vals,
                   const float* init, int init_rows, int init_cols);
int tsne_get_graph(ics_tsne* h, int64_t* indptr, int32_t* indices, double* vals, size_t capacity, size_t* nnz);
int tsne_gradient(ics_tsne* h, const float* y, double exaggeration, float* grad, double* kl);
int tsne_run(ics_tsne* h, int iters, int* done);
int tsne_read(ics_tsne* h, float* embedding, double* kl, double* grad_norm, int* n_iter, int* count);
int tsne_device(const ics_tsne* h);
int tsne_dim(const ics_tsne* h);

}  // namespace ics
