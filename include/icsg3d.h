/*
 * icsg3d.h -- C ABI of libicsg3d_hip.so, the MI355X (gfx950) engine for the ICSG3D hot path.
 *
 * The reference (by256/icsg3d) has no FFI: its boundary is the Python class surface of
 * unet/unet.py (AtomUnet) and vae/lattice_vae.py (LatticeDFCVAE) over Keras.  This header is what
 * those classes bind instead of Keras; each entry point cites the reference call it stands in for
 * (paths relative to the reference root).  icsg3d_amd/_lib.py is the ctypes binding;
 * INTEGRATION.md shows the reference-side stub.
 *
 * Conventions: every function returns 0 on success, non-zero on failure with the message in
 * ics_last_error() (thread-local).  Host tensors are caller-owned, dense, row-major, channels-last
 * (B,D,H,W,C) float32 unless stated; the library copies them.  All device memory is owned by the
 * handle and released by *_destroy.  A handle is bound to the HIP device current at creation and is
 * not thread-safe (the reference drives training from one thread: unet/unet.py:370).
 */
#ifndef ICSG3D_H
#define ICSG3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- library / device */
const char* ics_last_error(void);
const char* ics_version(void);
/* Device kernels this process has enqueued through the library so far (every launch site counts itself; the
 * runtime's copy / fill kernels and RCCL's kernels are not included).  bench.py reports the per-step difference as
 * kernel_launches_per_step; rocprofv3 --kernel-trace of the same command shows the same number of ics:: kernels. */
long long ics_kernel_launches(void);
int ics_device_count(int* count);
int ics_set_device(int device);
/* HIP device properties the benchmark reports (name is a 256-byte buffer). */
int ics_device_info(char* name, int* compute_units, size_t* hbm_bytes);

typedef struct ics_net ics_net; /* opaque: a U-Net or a DFC-VAE engine */

/* ---------------------------------------------------------------- AtomUnet
 * AtomUnet.__init__ / unet_3d_multiclass            (unet/unet.py:235-355)
 * loss = weighted_categorical_crossentropy(num_classes) + binary_crossentropy, Adam(lr)
 *                                                   (unet/unet.py:245-259) */
typedef struct ics_unet_config {
  int in_channels;   /* C of input_shape=(d,d,d,C): 1 or 4          (unet/unet.py:240) */
  int num_classes;   /* 95; accepted: 2 .. 127 (uint8 labels; the [soft | sig] logits are one row of <= 128 columns).
                      * 95 takes the fused head kernels, every other count the 1x1x1 GEMM + head_kernel (unet/unet.py:237) */
  int d;             /* grid edge, power of two >= 8 (32; 64 is a build extension) */
  int max_batch;     /* largest batch a single call may carry                             */
  float lr;          /* Adam learning rate                          (unet/unet.py:241,245) */
  float loss_weight; /* scalar class weight; <=0 selects float(num_classes)  */
  int pool_ties_all; /* 1: TF-CPU MaxPool3DGrad tie rule (default), 0: first max only     */
  int bn_unbias;     /* 1: Keras moving-variance n/(n-(1+eps)) rescale (default)          */
  int bce_from_logits; /* "binary_crossentropy" of the sig head (unet/unet.py:254-256): 0 (default) = the clipped-probability
                        * form -[t log p + (1-t) log(1-p)], p in [1e-7, 1-1e-7]; 1 = tf.keras.backend.binary_crossentropy's
                        * short-circuit for a Sigmoid producer op, sigmoid_cross_entropy_with_logits (TF 2.1; SURVEY App. B,
                        * confidence M).  The two agree to ~1e-7 relative except at saturated probabilities.       */
} ics_unet_config;

int ics_unet_create(const ics_unet_config* cfg, ics_net** out);

/* model.predict(X) -> [soft (B,d,d,d,num_classes), sig (B,d,d,d,1)]   (unet/unet.py:98,383-385;
 * callers generate.py:220, eval.py:166).  Eval-mode BatchNorm. */
int ics_unet_predict(ics_net* net, const float* x, int batch, float* soft, float* sig);
/* Fused inference tail (generate.py:220-225): argmax species + (sig >= thresh) mask, uint8. */
int ics_unet_predict_labels(ics_net* net, const float* x, int batch, float thresh,
                            uint8_t* species, uint8_t* mask);
/* model.train_on_batch / the per-batch step inside fit_generator (unet/unet.py:370): forward in
 * training mode, loss, backward, BN moving-stat update, Adam.  labels are uint8 class ids
 * (B,d,d,d) -- the one-hot of unet/data.py:89 is never built; the sigmoid target is labels != 0
 * (unet/data.py:87).  metrics = [Loss, lsoft, lsig, f1, wr] (unet/unet.py:250). */
int ics_unet_train_step(ics_net* net, const float* x, const uint8_t* labels, int batch,
                        float metrics[5]);
/* model.test_on_batch / validation pass: eval-mode BN, same metrics, no update. */
int ics_unet_test_step(ics_net* net, const float* x, const uint8_t* labels, int batch,
                       float metrics[5]);
/* The K.sum(...) terms behind the ratios of r_m / p_m / f1_m / wr_m (unet/unet.py:159-193) and the two loss means of
 * the LAST train / test step (data parallel: after the all-reduce, i.e. over the global batch):
 * sums = [sum_voxels wcce, sum_voxels bce, true_positives, predicted_positives, wr true_positives, wr possible_positives,
 * voxel count (= possible_positives of r_m: y_true is one-hot)].  The counts are integers held in doubles.
 * Valid only after a step that RETURNED metrics (ics_unet_train_step / _test_step, or _train_step_resident with a non-NULL
 * metrics pointer): a resident step enqueued without metrics skips the reduction over the ranks under data parallelism, and
 * the sums then still hold the last metric-returning step's values. */
int ics_unet_metric_sums(ics_net* net, double sums[7]);
/* Per-class loss weights (weighted_categorical_crossentropy's `weights` as the array of shape (C,) its docstring names,
 * unet/unet.py:196-221): w[count], count == num_classes, every weight finite and >= 0.  From then on every train and test
 * step -- synchronous, resident, fed -- weighs a voxel's softmax loss and its gradient by w[label] instead of the scalar
 * ics_unet_config.loss_weight; the mean is still taken over all B V voxels, the sigmoid loss and f1 / wr do not change, and
 * a voxel of a class with weight 0 contributes exactly 0 to the loss and an exactly zero softmax gradient row.  Predict
 * paths are unaffected.  w == NULL: back to the scalar.  The table lives in the engine's own device memory; with a
 * communicator ics_net_comm_broadcast_state sends it, and whether it is active, from the root to every rank. */
int ics_unet_set_class_weights(ics_net* net, const float* w, int count);
/* *active = 1 while a table is set (active may be NULL); w (may be NULL, else count == num_classes) receives the table, or
 * num_classes copies of the scalar loss weight while none is set. */
int ics_unet_get_class_weights(ics_net* net, float* w, int count, int* active);

/* Benchmark path: batch resident in HBM, steps enqueued back-to-back on the engine's stream. */
int ics_unet_upload_batch(ics_net* net, const float* x, const uint8_t* labels, int batch);
int ics_unet_train_step_resident(ics_net* net, float metrics_or_null[5]);
/* model.predict on the resident batch (unet/unet.py:383-385; BASELINE configs[0]), enqueued only: eval-mode forward, the
 * outputs stay in HBM -- probabilities, or with labels_only the uint8 argmax / (sig >= thresh) volumes (generate.py:221-225). */
int ics_unet_predict_resident(ics_net* net, int labels_only, float thresh);

/* ---------------------------------------------------------------- LatticeDFCVAE
 * LatticeDFCVAE.__init__/_set_model/build_encoder/build_decoder (vae/lattice_vae.py:89-230);
 * loss = mse + alpha*perceptual + beta*kld (vae/lattice_vae.py:232-270). The perceptual U-Net is
 * an ics_net created by ics_unet_create whose weights stay frozen (vae/lattice_vae.py:120). */
typedef struct ics_vae_config {
  int in_channels;  /* C                                           (vae/lattice_vae.py:91)  */
  int cond_shape;   /* 10                                          (vae/lattice_vae.py:102) */
  int latent_dim;   /* 256                                         (vae/lattice_vae.py:95)  */
  int filters[4];   /* 16,32,64,128                                (vae/lattice_vae.py:94)  */
  int d;            /* 32 (decoder seed (d/8)^3*4, encoder flatten (d/16)^3*4)              */
  int max_batch;
  float lr;         /* Adam(5e-4)                                  (vae/lattice_vae.py:98)  */
  float alpha;      /* 0.5  */
  float beta;       /* 3e-4 */
  float pm_layer_weights[4]; /* 1,1,1,1 for re_lu_2/4/6/8          (vae/lattice_vae.py:100-101) */
  int bn_unbias;
} ics_vae_config;

/* Accepted ranges (anything else is refused here, with ics_last_error naming the option, before any allocation):
 *   in_channels >= 1, max_batch >= 1, d a power of two >= 16;
 *   cond_shape >= 1, latent_dim >= 1, filters[i] in [1, 16384], latent_dim + cond_shape <= 16384,
 *   in_channels * (1 + cond_shape) <= 16384 (no layer input wider than 16384 channels: the width of the identity
 *   affine the convolution launchers read a BatchNorm-less source through) -- any width inside these: multiples of 32
 *   take the Winograd / vector kernels,
 *   multiples of 4 the four-channel element-wise kernels, everything else the scalar paths (same results, slower);
 *   widths past one block's 256 column groups (above 256, above 1024 for multiples of 4) loop over the columns;
 *   the analytic fold of the tiled condition into e0 exists for in_channels == 1 with filters[0] == 16 or 32, other
 *   widths run e0 as the (1 + cond_shape) * in_channels -channel convolution it is.
 * alpha, beta and pm_layer_weights are plain scalars of the loss (0 allowed). */
int ics_vae_create(const ics_vae_config* cfg, ics_net* perceptual_unet, ics_net** out);

/* encoder.predict([M, cond]) -> (z_mean, z_log_var, z)  (generate.py:196, interpolate.py:50-59);
 * eps is the N(0,1) draw of sampling() (vae/lattice_vae.py:53-66), injected by the caller. */
int ics_vae_encode(ics_net* net, const float* x, const float* cond, const float* eps, int batch,
                   float* z_mean, float* z_log_var, float* z);
/* decoder.predict([z, cond]) -> (B,d,d,d,C)             (generate.py:208, lattice_vae.py:351) */
int ics_vae_decode(ics_net* net, const float* z, const float* cond, int batch, float* recon);
/* model.train_on_batch([M,cond], M) (vae/lattice_vae.py:296) -> [Loss, PM, MSE, KLD]; the
 * perceptual U-Net runs BatchNorm on batch statistics, frozen. */
int ics_vae_train_step(ics_net* net, const float* x, const float* cond, const float* eps, int batch,
                       float metrics[4]);
/* model.test_on_batch (vae/lattice_vae.py:307): learning phase 0 everywhere. */
int ics_vae_test_step(ics_net* net, const float* x, const float* cond, const float* eps, int batch,
                      float metrics[4]);
int ics_vae_upload_batch(ics_net* net, const float* x, const float* cond, const float* eps, int batch);
int ics_vae_train_step_resident(ics_net* net, float metrics_or_null[4]);

/* Fused inference tail (generate.py:204-225, eval.py:163-175): decoder.predict([z, cond]) ->
 * unet.model.predict -> np.argmax(soft, -1) / (sig >= thresh), device-resident end to end (the
 * reconstruction is never copied to the host).  `unet` is any U-Net engine with the VAE's grid and
 * channel count.  Outputs, each optional (NULL to skip): species/mask uint8 (B,d,d,d); density = channel 0
 * of the reconstruction, float (B,d,d,d) (watershed input, generate.py:232); coord_minmax float (B,3,2) =
 * per-sample {min,max} of channels 1..3 -- all that to_lattice_params (utils.py:160-178) reads of the
 * coordinate channels (zeros when in_channels == 1). */
int ics_vae_decode_to_unet_labels(ics_net* vae, ics_net* unet, const float* z, const float* cond, int batch,
                                  float thresh, uint8_t* species, uint8_t* mask, float* density,
                                  float* coord_minmax);

/* Connected-component post-processing on the device: the integer part of watershed_clustering
 * (/root/reference/watershed.py:190-203) that follows the fused tail in generate.py:228-236 / eval.py.
 *   - segment_nuclei step 1 (watershed.py:52-56): measure.label(binary, connectivity=1) = 6-connected components
 *     numbered in raster order of their first voxel; components with <= min_voxels voxels are dropped (reference: 3);
 *   - R as segment_nuclei returns it when every kept component passes `convexity >= min_convexity`
 *     (watershed.py:85-92): kept components renumbered 1..n in ascending label order, 0 elsewhere;
 *   - centroids / majority_vote (watershed.py:153-187) per region: the most frequent non-zero species (equal counts:
 *     the larger id, as the reference's stable sort leaves it) and the integer coordinate sums of ALL its voxels.
 * The convexity test (watershed.py:80) and the split of non-convex components (watershed.py:95-150) continue from
 * these regions, counts and bounding boxes: ics_op_label_boxes / ics_op_watershed_split below, driven by
 * icsg3d_amd/watershed.py (the recursion and the Qhull convexity test run on the host, as in the reference).
 * Outputs: regions int32 (B,d,d,d) or NULL; counts int32 (B,2) = {components, kept components};
 * atom_stats int32 (B,max_atoms,11) = {species, voxels, sum_z, sum_y, sum_x, z0, y0, x0, z1, y1, x1} (axes 0,1,2 of the
 * volume -- the reference calls them x,y,z; bounding box half-open), rows >= kept components are empty.
 * A sample with more than max_atoms kept components reports counts[b][1] > max_atoms: its rows are truncated and the
 * caller must skip it (the reference skips a failed sample too, generate.py:228-236); the call itself succeeds.
 * convexity_bounds int64 (B,max_atoms,8) or NULL = {P, sum zz, sum yy, sum xx, sum zy, sum zx, sum yx, 0} per region:
 * P = the number of grid points of the region's bounding box inside its 26-direction polytope (directions in {-1,0,1}^3,
 * the voxels offset by +-0.5 along one axis at a time as convex_hull_image does).  The convex hull is a subset of that
 * polytope, so voxels / P is a LOWER bound of the convexity watershed.py:80-83 tests: where it reaches min_convexity no
 * hull is needed; the second moments decide coplanarity (the 3 x 3 scatter matrix is singular), i.e. the components for
 * which the reference stack's Qhull call fails.  Exact integer arithmetic (icsg3d_amd/watershed.py: refine_atoms).
 * Integer atomics only: results are bit-exact. */
int ics_op_segment_atoms(const uint8_t* mask, const uint8_t* species, int batch, int d, int min_voxels, int max_atoms,
                         int num_species, int32_t* regions, int32_t* counts, int32_t* atom_stats,
                         int64_t* convexity_bounds);
/* ---- segment_nuclei's non-convex branch and recursion (watershed.py:40-150) on boxes.  A box is a dense int32 volume
 * [D][H][W] (extents 1..256) -- a whole d^3 grid, a component cropped to its bounding box, or a watershed result that is
 * segmented again; `nbox` boxes lie back to back in `vols` / `boxes`, dims = [nbox][3].  HOST pointers.  Boxes up to 64
 * per axis run one workgroup per box; larger ones run on host threads (same results), and so does every box of
 * ics_op_label_boxes under ICSG3D_LABEL_HOST=1.
 * The scikit-image 0.17.2 routines these replace (requirements.txt:95) are absent from the image: PARITY UNPINNED, the
 * algorithms are restated in oracle/watershed_ref.py and the kernels are held to that restatement bit for bit.
 *   ics_op_label_boxes   = skimage.measure.label(box, connectivity) (watershed.py:52, :103): maximal sets of voxels of
 *     EQUAL non-zero value, numbered from 1 in raster order of their first voxel; connectivity 1 = 6 neighbours,
 *     3 = 26.  nlabels[nbox]; stats (or NULL) [nbox][max_labels][7] = {voxels, z0, y0, x0, z1, y1, x1} (half-open).
 *   ics_op_watershed_split = watershed.py:95-110 for a box with values {0, cls[b]}: fg / bg = erosion / dilation with
 *     ball(1) (out-of-box neighbours ignored), markers = label(fg) + 1 with `markers[(bg - fg) == 1] = 0` (the
 *     reference compares against 1, so the shell opens only for the component labelled 1), the priority flood of
 *     segmentation.watershed (two image levels; a binary heap on (level, age) with skimage's tie behaviour when
 *     tie = 0, FIFO when tie = 1), `wss[wss == 1] = 0`.  wss: labels 2.. or 0, before the reference's max_class shift. */
int ics_op_label_boxes(const int32_t* vols, const int32_t* dims, int nbox, int connectivity, int max_labels,
                       int32_t* labels, int32_t* nlabels, int32_t* stats);
int ics_op_watershed_split(const int32_t* boxes, const int32_t* dims, const int32_t* cls, int nbox, int tie, int32_t* wss);
/* Round 6: ics_op_watershed_split runs on HOST threads by default (one box per thread: the flood is a chain of dependent heap
 * operations, which one CPU core walks ~30x faster than one GPU lane and which cannot be spread over lanes without changing the
 * pop order the result depends on); ICSG3D_WS_DEVICE=1 selects the kernel.  Both are held to oracle/watershed_ref.py.
 * ics_op_component_bounds: the exact-integer bounds the convexity test of watershed.py:80-83 is decided from wherever they
 * are conclusive, for every component (labels 1..nlabels[b], more than min_voxels voxels) of the label volumes ics_op_label_boxes
 * returned (same dims / stats layout): bounds [nbox][max_labels][5] = {voxels, P, F, flat, H} with P >= count_nonzero(
 * convex_hull_image(component)) >= F -- P = bounding-box grid points inside the component's 26-direction polytope, F = the
 * component closed under axis-parallel line fills -- flat = 1 for coplanar / collinear components (the reference stack's
 * Qhull call fails there), and H = that count itself, computed exactly (integer gift wrapping over the +-0.5 offset voxel
 * set on doubled coordinates; a grid point on a facet counts as inside, as under the reference's 1e-10 tolerance) only where
 * hull_threshold > 0 and voxels / P < hull_threshold <= voxels / F, else 0 (also 0 where the hull search does not close:
 * the caller then uses Qhull).  Every stats row it reads (more than min_voxels voxels) must hold a non-empty box inside its
 * volume: the call is refused, naming the box, before anything is written.  Host threads; no device work. */
int ics_op_component_bounds(const int32_t* labels, const int32_t* dims, int nbox, const int32_t* nlabels, const int32_t* stats,
                            int max_labels, int min_voxels, double hull_threshold, int64_t* bounds);
/* The three box-level entry points below keep one stream and one grow-only device scratch buffer per host thread (they are
 * called tens of times per sample from the host recursion of segment_nuclei); this releases the calling thread's. */
int ics_release_caches(void);
/* centroids / majority_vote (watershed.py:153-187) for an arbitrary region volume R [D][H][W] (labels 1..num_labels, e.g.
 * what segment_nuclei returns after splits): stats [num_labels][11] as ics_op_segment_atoms; labels that do not occur
 * keep voxels = 0.  Pinned by the reference's own two functions (tests/golden/watershed_golden.npz). */
int ics_op_region_stats(const int32_t* R, const uint8_t* species, int D, int H, int W, int num_labels, int num_species,
                        int32_t* stats);
/* ics_vae_decode_to_unet_labels continued on the device through the component labelling above: the mask and species
 * volumes never leave HBM between the U-Net and the region statistics.  species/mask/density/coord_minmax/regions
 * and convexity_bounds are optional (NULL to skip). */
int ics_vae_decode_to_unet_atoms(ics_net* vae, ics_net* unet, const float* z, const float* cond, int batch,
                                 float thresh, int min_voxels, int max_atoms, uint8_t* species, uint8_t* mask,
                                 float* density, float* coord_minmax, int32_t* regions, int32_t* counts,
                                 int32_t* atom_stats, int64_t* convexity_bounds);

/* ---------------------------------------------------------------- voxelisation (create_matrices.py)
 * The arrays create_matrices.py saves per crystal (reference create_matrices.py:117-190), computed on the device in
 * the reference's semantics -- no periodic images, lattice angles ignored, fp64:
 *   M density  (2 pi)^-1.5 sum_s exp(-D^2 / (2 sigma_s^2)) Z_s / sigma_s^3      utils.density_matrix (utils.py:97-144)
 *   S species  0 when no site has D < sigma_s*label_frac, that site's Z when one does, else Z of argmin_s D over ALL sites
 *              (the double loop of utils.py:117-134; ties to the first site)
 *   p          p[i,j,k] = (x_i, y_j, z_k), x = linspace(0, a + 2*eps*a, d+1)[:-1]  utils.coordinate_grid (utils.py:88-94)
 * with D the euclidean distance from site s to the voxel centre linspace(-a*eps, a + a*eps, d+1)[:-1] + dv/2 per axis
 * (utils.py:102-115), flat voxel order product(x, y, z): M[i,j,k] has i along a.
 * A job = {structure, r0, r1, r2}: structure index, then up to three quarter turns applied in order, each an index into
 * [(0,1), (0,2), (1,2)] or -1 for none.  scipy.ndimage.rotate(X, 90, axes, reshape=False, mode="nearest") as
 * random_rotation_3d (utils.py:193-222) calls it equals np.rot90(X, 1, axes) on these grids, and that is what is applied
 * (p's channels are not permuted: only positions move, as in the reference). */
typedef struct ics_structures {
  int count, max_sites;  /* site arrays are [count][max_sites]; rows >= nsites[i] are never read                 */
  const int32_t* nsites; /* [count], 1..256                                                                       */
  const double* xyz;     /* [count][max_sites][3] cartesian = min-shifted frac * abc (utils.py:83-84, create_matrices.py:140) */
  const double* z;       /* [count][max_sites] atomic numbers                                                    */
  const double* sigma;   /* [count][max_sites] Gaussian width = sigma_frac * ionic radius (create_matrices.py:150)  */
  const double* abc;     /* [count][3] lattice lengths (create_matrices.py:129)                                  */
} ics_structures;
/* HOST pointers in and out.  jobs [njobs][4]; outputs each optional (NULL): M, S [njobs][d][d][d], p [njobs][d][d][d][3],
 * float64.  d in [2, 256].  Any njobs: chunked internally under a device-memory budget (the calling thread's scratch,
 * freed by ics_release_caches).  Synchronous. */
int ics_op_voxelise(const ics_structures* s, const int32_t* jobs, int njobs, int d, double eps_frac, double label_frac,
                    double* M, double* S, double* p);
/* The same grids written straight into the engine's resident batch (what ics_unet_upload_batch / ics_vae_upload_batch
 * would upload from the loaders of unet/data.py / vae/data.py over the saved files, bit for bit: float32 rounded from the
 * same fp64 values): x = M (C = 1) or [M, p] (C = 4); the U-Net's uint8 labels = S (Z must be a class id < num_classes);
 * the VAE's cond / eps are uploaded as by ics_vae_upload_batch.  Enqueued on the engine's stream (the ~1 KB of site data
 * per job goes through pinned memory); *_train_step_resident / ics_unet_predict_resident then run unchanged.
 * jobs [batch][4], batch <= max_batch, the engine's own d; in_channels must be 1 or 4. */
int ics_unet_voxelise_batch(ics_net* net, const ics_structures* s, const int32_t* jobs, int batch, double eps_frac,
                            double label_frac);
int ics_vae_voxelise_batch(ics_net* net, const ics_structures* s, const int32_t* jobs, int batch, double eps_frac,
                           double label_frac, const float* cond, const float* eps);

/* ---------------------------------------------------------------- evaluation (eval.py)
 * vae.model.predict([M, cond]) -> unet.model.predict -> argmax / (sig >= thresh) -> components + statistics
 * (eval.py:163-175 + watershed.py:190-203) on the batch placed by ics_vae_upload_batch / ics_vae_voxelise_batch (its eps
 * is the sampling draw, F8); learning phase 0.  Outputs as ics_vae_decode_to_unet_atoms, each optional except counts /
 * atom_stats; bit-identical to ics_vae_encode of the same batch followed by ics_vae_decode_to_unet_atoms of its z.
 * Refused: no resident batch, a U-Net of another d or C, a resident batch above the U-Net's max_batch.  The resident
 * batch is left unchanged. */
int ics_vae_reconstruct_resident_to_unet_atoms(ics_net* vae, ics_net* unet, float thresh, int min_voxels,
                                               int max_atoms, uint8_t* species, uint8_t* mask, float* density,
                                               float* coord_minmax, int32_t* regions, int32_t* counts,
                                               int32_t* atom_stats, int64_t* convexity_bounds);
/* emd()  (eval.py:45-53): per sample b, the minimum-cost one-to-one matching between point sets
 * A_b = a[a_off[b] .. a_off[b+1]) and B_b = b[b_off[b] .. b_off[b+1]) (float64 xyz, Angstrom) under euclidean distance;
 * emd[b] = matched distance sum / min(|A_b|, |B_b|) -- NaN when either set is empty, as the reference's 0/0.
 * match (optional) [a_off[batch]]: index into B_b of each point of A_b, -1 for an unmatched point.
 * Exact, fp64 (shortest augmenting paths with potentials, one workgroup per sample); results are the same run to run.
 * Refused, naming the sample, with nothing written: a set above 2048 points, offsets that do not start at 0 or
 * decrease, batch < 1, a coordinate that is not finite or exceeds 1e150 in magnitude.
 * HOST pointers, any batch (chunked internally), synchronous, the calling thread's op stream. */
int ics_op_match_emd(const double* a, const int32_t* a_off, const double* b, const int32_t* b_off, int batch,
                     double* emd, int32_t* match);

/* ---------------------------------------------------------------- structures (generate.py's CIF stage)
 * to_pymatgen_structure (utils.py:225-239) and structure.is_valid() (generate.py:251-263) for a ragged batch: structure
 * b holds atoms offsets[b] .. offsets[b+1]) with species (atomic numbers) and cartesian xyz (float64, Angstrom, the
 * orthogonal frame in which generate.py computes mu), lattice lengths abc [batch][3] and angles [batch][3] in degrees.
 *   lattice [batch][9]  rows va = [a sin(beta), 0, a cos(beta)], vb = [-b sin(alpha) cos(g), b sin(alpha) sin(g),
 *                       b cos(alpha)], vc = [0, 0, c], g = acos((cos(alpha) cos(beta) - cos(gamma)) / (sin(alpha)
 *                       sin(beta))) (Lattice.from_parameters; sine and cosine of exactly 90 degrees are 1 and 0)
 *   volume  [batch]     its determinant
 *   frac    [atoms][3]  xyz / abc: the atoms are placed in the 90-degree lattice and keep their fractional coordinates
 *                       when the lattice is swapped (utils.py:231-238); not wrapped into the cell
 *   min_dist [batch], min_pair [batch][2]  the smallest shortest-periodic distance over pairs i < j and that pair, ties
 *                       to the lexicographically smallest pair; +inf and (-1, -1) below two atoms
 *   n_close [batch]     pairs with distance <= tol
 *   valid, reason [batch]  valid = 1 where reason = 0; reason bits: 1 a pair at or under tol (is_valid's rule; a one-site
 *                       structure passes), 2 a species outside 1..94, 4 no atoms
 *   nearest [atoms]     each atom's distance to its nearest other atom (+inf for a lone atom)
 *   hist    [batch][95] atoms per atomic number (species outside 1..94 are not counted)
 * The shortest periodic distance is the exact minimum over ALL lattice translations of the wrapped fractional
 * difference (the image range per axis is derived from the cell), in fp64; results are the same bits run to run.
 * Refused, naming the structure, with nothing written: batch < 1, a null argument, a non-finite or negative tol, offsets
 * that do not start at 0 or decrease, more than 2048 atoms in a structure, a non-finite input, a cell length <= 0, angles
 * that make no cell (volume <= 0), a cell so skewed that the search would exceed 32 translations per axis, a coordinate
 * above 1e150 in magnitude.
 * HOST pointers, all outputs required, any batch (chunked internally), synchronous, the calling thread's op stream. */
int ics_op_structure_screen(const int32_t* offsets, const int32_t* species, const double* xyz, const double* abc,
                            const double* angles, int batch, double tol, double* lattice, double* volume, double* frac,
                            double* min_dist, int32_t* min_pair, int32_t* n_close, int32_t* valid, int32_t* reason,
                            double* nearest, int32_t* hist);
/* Which structures are the same crystal: duplicates among `nq` queries and hits in `nref` references.  The predicate is
 * this library's own -- exact, deterministic, no assignment solver; NO parity with pymatgen's StructureMatcher is
 * claimed (it is not a dependency and no fixture was recorded from it).
 * The packed table holds the nq queries followed by the nref references: structure s holds atoms offsets[s] ..
 * offsets[s+1]) with species (atomic numbers Z_i), fractional coordinates frac [atoms][3] (any real values, wrapped
 * internally: f - floor(f)) and lattice [nq+nref][9] = M, rows va, vb, vc as ics_op_structure_screen returns it;
 * G = M M^T.  eligible [nq+nref]: 0 = the structure is never compared (see below).
 *   Candidates.  (A, B) is compared only if both are eligible, n_A == n_B and the species histograms are equal.
 *   Operations.  Signed axis permutations P (3x3, entries 0/+-1) acting as f' = P f, f'_k = sign_k f[perm_k].  Their
 *     order is lexicographic over (permutation, sign pattern): permutations (0,1,2) (0,2,1) (1,0,2) (1,2,0) (2,0,1)
 *     (2,1,0), and per permutation the signs (+,+,+) (+,+,-) (+,-,+) (+,-,-) (-,+,+) (-,+,-) (-,-,+) (-,-,-); index 0 is
 *     the identity.  ops_mode 0: the identity; 1: the 24 of determinant +1 (what np.rot90 produces on the grids), in
 *     that order; 2: all 48.  A reported op indexes the list of the call's ops_mode.
 *     P is admissible for (A, B) when, with G' = P G_A P^T, |G'_kl - G_B,kl| <= ltol sqrt(G_B,kk G_B,ll) for all k, l.
 *   Anchor.  a0 = the lowest-index atom of A whose species has the smallest count in A (ties between species to the
 *     lower Z); anchor candidates are the atoms j of B of that species, in index order.
 *   One combination (P, j).  t = g_j - P f_a0; for every atom i of A, p_i = P f_i + t; among the atoms of B with
 *     Z == Z_i the one with the smallest wrapped-image distance (D = g - p_i, D -= rint(D), u = M_B^T D; ties to the
 *     lower index) is nb(i) with vector u_i.  The combination passes if (a) |u_i| <= 2 tol for all i, (b) nb is
 *     injective, (c) with ubar = mean_i u_i and r_i = u_i - ubar, max_i |r_i| <= tol.  Its score is
 *     rms = sqrt(mean_i |r_i|^2).
 *   Pair.  A and B match if some admissible P and some anchor j pass; the pair's rms is the minimum over the passing
 *     combinations and (op, anchor) its argmin, ties to the lower (op, anchor).
 * Outputs, per query q:
 *   dup_of [nq]      the smallest q' < q that matches q (A = q', B = q), -1 if none
 *   dup_rms [nq], dup_op [nq][2]   that pair's rms and (op, anchor = atom index in B); +inf and (-1, -1) if none
 *   ref_of [nq]      the reference (0 .. nref-1) with the smallest rms among the matching ones (A = q, B = reference),
 *                    ties to the lower index; -1 if none.  ref_rms [nq], ref_op [nq][2] as above
 *   n_cmp [nq][2]    candidate pairs compared against earlier queries and against references
 * An ineligible query comes back -1 / +inf / n_cmp 0 and is nobody's partner.
 * What makes "match" mean "the same crystal" is the caller's eligibility rule (icsg3d_amd.structures.eligibility): the
 * wrapped image is the only one that can lie within 2 tol when 2 tol g_k < 0.5 for the norms g of the columns of
 * inv(M) (enforced here, see the refusals), and nb is forced to be a bijection when every interatomic distance of both
 * structures exceeds 4 tol (the caller's: the screen's min_dist).
 * All arithmetic is fp64 with a fixed summation order and no floating-point atomics: the same bits run to run, for any
 * chunking.  ICSG3D_MATCH_CHUNK_PAIRS (read once per process) shrinks the number of pair results held at a time.
 * Refused, naming the structure, with nothing written: a null argument, nq < 1, nref < 0, a tolerance that is not
 * finite and > 0, ops_mode outside 0..2, offsets that do not start at 0 or decrease, and an ELIGIBLE structure with no
 * atoms or more than 256, a non-finite lattice entry or coordinate (or one above 1e15), a species outside 1..94, a
 * lattice volume <= 0, or a cell too thin for tol (2 tol g_k >= 0.5).
 * HOST pointers, all outputs required, any nq / nref (pairs are enumerated on the device from composition buckets and
 * chunked internally), synchronous, the calling thread's op stream. */
int ics_op_structure_match(const int32_t* offsets, const int32_t* species, const double* frac, const double* lattice,
                           const int32_t* eligible, int nq, int nref, double tol, double ltol, int ops_mode,
                           int32_t* dup_of, double* dup_rms, int32_t* dup_op, int32_t* ref_of, double* ref_rms,
                           int32_t* ref_op, int32_t* n_cmp);
/* Which symmetry a structure has: the operations (W, t) that map it onto itself within tol, and the group they form.  The
 * predicate is this library's own -- exact, deterministic -- and is pinned to a brute-force fp64 restatement
 * (tests/structure_symmetry_ref.py); NO parity with spglib or pymatgen's SpacegroupAnalyzer is claimed, and no space-group
 * name, number, standard setting or Wyckoff letter is produced.
 * Input: one packed table of ns structures laid out as for ics_op_structure_match: structure s holds atoms offsets[s] ..
 * offsets[s+1]) with species (atomic numbers 1..94), frac [atoms][3] (any reals, wrapped internally: f - floor(f)),
 * lattice [ns][9] = M (rows va, vb, vc), eligible [ns]; tol (Angstrom), ltol, and max_ops, the capacity of the
 * per-structure operation lists.  G = M M^T.
 *   Lattice operations.  Candidates are the 3x3 integer matrices W with entries in {-1, 0, 1} and determinant +-1 (6 960
 *     of the 19 683); code = sum_{k=0..8} (W[k/3][k%3] + 1) 3^(8-k); candidates are taken in ascending code; W acts on
 *     column vectors, f' = W f + t.  W is admissible when |(W^T G W)_kl - G_kl| <= ltol sqrt(G_kk G_ll) for all k, l (the
 *     form that preserves lengths for a general W; the match op's P G P^T coincides with it only for signed
 *     permutations).  Capacity: 64 admissible W per structure (exact lattices give at most 48); more sets reason bit 2,
 *     n_lat still counts them all, and no operation is evaluated: n_ops = n_point = n_trans = 0, types = 0.
 *     A lattice whose operations need an entry outside {-1, 0, 1} (a cell that is not reduced) reports fewer operations;
 *     it does not report wrong ones.
 *   Anchor.  a0 = the lowest-index atom of the rarest species (ties between species to the lower Z); the anchor
 *     candidates are the atoms j of that species, in index order.
 *   One combination (W, j).  t = f_j - W f_a0, p_i = W f_i + t; nb(i) = the same-species atom with the smallest
 *     wrapped-image distance (D = f - p_i, D -= rint(D), u = M^T D; ties to the lower index), u_i its vector.  The
 *     combination passes if (a) |u_i| <= 2 tol for all i, (b) nb is injective, (c) with ubar = mean_i u_i,
 *     max_i |u_i - ubar| <= tol.  It then IS the symmetry operation (W, t*): t* = t + M^-T ubar, the fitted translation in
 *     fractional coordinates, reported (and used below) wrapped into [0, 1); rms = sqrt(mean_i |u_i - ubar|^2).
 *     Operations are listed in the order (code ascending, anchor ascending).
 * Outputs, per structure:
 *   n_lat            the number of admissible W
 *   n_ops            all passing combinations, counted even beyond max_ops
 *   n_point          distinct W among the passing combinations
 *   n_trans          passing combinations with W = I (code 16484): the centring translations, identity included
 *   types [ns][10]   how many of the distinct W have rotation type -6, -4, -3, -2, -1, 1, 2, 3, 4, 6 in that order
 *                    (det +1 with trace 3, -1, 0, 1, 2 -> 1, 2, 3, 4, 6; det -1 with trace -3, 1, 0, -1, -2 -> -1, -2, -3,
 *                    -4, -6; a W with any other (det, trace), which only a loose ltol admits, is counted in no type)
 *                    -- these four over ALL passing combinations, whatever max_ops is
 *   op_code, op_anchor [ns][max_ops], op_t [ns][max_ops][3], op_rms [ns][max_ops]
 *                    the first min(n_ops, max_ops) operations (anchor = atom index in the structure); unused slots hold
 *                    -1 / -1 / NaN / NaN
 *   reason [ns]      bits: 1 not eligible, 2 lattice-operation overflow, 4 n_ops > max_ops, 8 not closed.
 *     Closed: for every ordered pair (g, h) of stored operations an operation with matrix W_g W_h and anchor
 *     nb_g(nb_h(a0)) is stored AND its nb equals nb_g o nb_h on every atom.  Closure is evaluated only when bits 1, 2 and
 *     4 are clear.
 * Where reason == 0:
 *   orbit [atoms]    the lowest structure-local index among nb_g(i) over all g;  mult [atoms]  the orbit size
 *   sym_frac [atoms][3]  fhat_k = f_k + (1 / n_ops) sum_g D_g,k with D_g,k = (W_g f_i + t*_g) - f_k for the i with
 *                    nb_g(i) = k, D -= rint(D); the sum in operation order; f the wrapped input; fhat is not re-wrapped
 *   sym_G [ns][9]    (1 / n_point) sum_W W^T G W over the distinct W, in code order
 *   sym_shift [ns]   max_k |M^T (fhat_k - f_k)|  (<= tol by rule (c): a mean of residuals each <= tol)
 *   sym_resid [ns]   the largest distance, measured with M, between W_g fhat_i + t*_g and fhat_nb_g(i) over all g and i,
 *                    after wrapping.  If the atoms are an exactly symmetric structure plus displacements e_i, then
 *                    t*_g = tau_g + (I - W_g) ebar: the fitted operations are the true ones with the origin moved by the
 *                    mean displacement, they compose exactly, and the average over them is an exact projection -- this
 *                    residual is rounding.
 * Where reason != 0: orbit[i] = i, mult = 1, sym_frac = the wrapped input, sym_G = G, sym_shift = sym_resid = 0.
 * What makes "operation" mean "symmetry" is the caller's eligibility rule, exactly as for ics_op_structure_match
 * (icsg3d_amd.structures.eligibility): min_dist > 4 tol forces nb to be a bijection, 2 tol g_k < 0.5 leaves one image.
 * All arithmetic is fp64 with a fixed summation order and no floating-point atomics: the same bits run to run and for
 * any chunking.  ICSG3D_SYMMETRY_CHUNK_BYTES (read once per process) shrinks the bytes of candidate table, nearest-atom
 * maps and operation lists held at a time.
 * Refused, naming the structure, with nothing written: a null argument, ns < 1, a tolerance that is not finite and > 0,
 * max_ops outside 1..4096, offsets that do not start at 0 or decrease, and an ELIGIBLE structure with no atoms or more
 * than 256, a non-finite lattice entry or coordinate (or one above 1e15), a species outside 1..94, a lattice volume <= 0,
 * or a cell too thin for tol (2 tol g_k >= 0.5).
 * HOST pointers, all outputs required, any ns (chunked internally), synchronous, the calling thread's op stream. */
int ics_op_structure_symmetry(const int32_t* offsets, const int32_t* species, const double* frac, const double* lattice,
                              const int32_t* eligible, int ns, double tol, double ltol, int max_ops, int32_t* n_lat,
                              int32_t* n_ops, int32_t* n_point, int32_t* n_trans, int32_t* types, int32_t* reason,
                              int32_t* op_code, int32_t* op_anchor, double* op_t, double* op_rms, int32_t* orbit,
                              int32_t* mult, double* sym_frac, double* sym_G, double* sym_shift, double* sym_resid);
/* A fixed-length structural fingerprint per crystal: the radial distribution function, plain and Z-weighted, with every
 * atom's nearest distance and coordination number.  The descriptor is this library's own -- exact, deterministic -- and is
 * pinned to a brute-force fp64 restatement (tests/structure_fingerprint_ref.py); NO parity with pymatgen's or matminer's
 * fingerprints is claimed.
 * Input: the packed table of ics_op_structure_match for ns structures: offsets, species (atomic numbers 1..94), frac
 * [atoms][3] (any reals, wrapped internally: f - floor(f)), lattice [ns][9] = M (rows va, vb, vc), eligible [ns].
 * Parameters (design parameters, not measured quantities): r_max > 0, the range in Angstrom; n_bins in 1..256; width = w
 * > 0, the half-width of the deposit kernel in Angstrom; cn_tol >= 0, the neighbour-distance slack.
 * With n atoms, V = det M, R = r_max + w and edges r_k = k r_max / n_bins:
 *   Pairs.  All ordered triples (i, j, T), T an integer vector, with d = |(f_j - f_i + T) M| and 0 < d < R; this includes
 *     an atom's own images (i = j, T != 0).  After wrapping, |T_k| <= floor(R g_k + 1) suffices, g_k the norm of column k
 *     of inv(M); the definition does not depend on the wrapping.
 *   Deposit.  A triangular kernel, so every output is a continuous function of every distance and a pair at d >= R
 *     deposits exactly 0 (no cutoff discontinuity, no erf): H(t) = 0 for t <= -1, (1 + t)^2 / 2 for -1 < t <= 0,
 *     1 - (1 - t)^2 / 2 for 0 < t < 1, 1 for t >= 1.  A pair adds H((r_{k+1} - d) / w) - H((r_k - d) / w) to bin k of
 *     `count` -- nothing where d >= r_{k+1} + w or d <= r_k - w, which is compared first, so outside the support the
 *     amount is exactly 0 -- and that amount times (Z_i Z_j) / (Zbar Zbar) to `countz`, Zbar the structure's mean Z.
 *   Normalisation.  g_k = count_k / (n (n / V) 4 pi / 3 (r_{k+1}^3 - r_k^3)); gZ_k the same with countz.  Both tend to 1
 *     at large r and do not depend on the choice of cell.
 *   Neighbours (the minimum-distance rule; no radius table).  nn_dist[i] = the smallest d over (j, T) for atom i;
 *     cn[i] = the number of (j, T) with d <= (1 + cn_tol) nn_dist[i].  This sweep is not limited to R: an atom's own image
 *     along the shortest lattice vector, of length l, bounds nn_dist, so the sweep of a structure reaches
 *     max(R, (1 + cn_tol) l) and its image range is |T_k| <= floor(max(R, (1 + cn_tol) l) g_k + 1).
 * Outputs: rdf [ns][2][n_bins] (g, then gZ), count [ns][n_bins] (the raw unweighted sums), n_pairs [ns] (int64: triples
 * with d < R), nn_dist [atoms], cn [atoms], reason [ns] with bits 1 = not eligible, 2 = the image range would exceed 32
 * on an axis.  Where reason != 0, rdf / count / nn_dist are NaN and cn and n_pairs are -1.
 * All arithmetic is fp64 with a fixed summation order and no floating-point atomics: a bin is the sum of its deposits in
 * the order (i's block of 64 atoms, j, T lexicographic with Ta slowest, i), the blocks added in ascending order; the same
 * bits run to run and for any chunking.  ICSG3D_FINGERPRINT_CHUNK_BYTES (read once per process) shrinks the bytes of
 * tables and results held at a time.
 * Refused, naming the structure, with nothing written: a null argument, ns < 1, a parameter outside its limits, offsets
 * that do not start at 0 or decrease, and an ELIGIBLE structure with no atoms or more than 256, a non-finite lattice entry
 * or coordinate (or one above 1e15), a species outside 1..94 or a lattice volume <= 0.  There is no thin-cell rule here.
 * HOST pointers, all outputs required, any ns (chunked internally), synchronous, the calling thread's op stream. */
int ics_op_structure_fingerprint(const int32_t* offsets, const int32_t* species, const double* frac, const double* lattice,
                                 const int32_t* eligible, int ns, double r_max, int n_bins, double width, double cn_tol,
                                 double* rdf, double* count, int64_t* n_pairs, double* nn_dist, int32_t* cn,
                                 int32_t* reason);
/* The nearest partners of fingerprints: fp [nq + nref][len] fp64, queries first; valid [nq + nref]; len >= 1, nq >= 1,
 * nref >= 0.  D(a, b) = sqrt((1 / len) sum_k (a_k - b_k)^2), computed from the differences directly in ascending k -- not
 * as |a|^2 + |b|^2 - 2 a.b, which cancels for the near-duplicates this op exists to rank.  D(a, b) and D(b, a) are the
 * same bits; exact copies give exactly 0.
 * Outputs (ties to the lower index; an invalid row is nobody's partner and comes back -1 / +inf, as does a row with no
 * partner): q_ref, q_ref_d [nq] the nearest reference (0 .. nref-1) of each query; ref_q, ref_q_d [nref] the nearest
 * query of each reference; q_q, q_q_d [nq] the nearest OTHER query; div_sum = sum of D over the valid query pairs q < q',
 * div_pairs their count.  The order of div_sum: number the valid queries 0, 1, ... in index order and cut them into
 * segments of 512; s_q = the sum over the segments, ascending, of (the sum of D(q, q') over the segment's q' > q,
 * ascending); div_sum = the sum of s_q over q ascending.
 * The same determinism contract as above: fixed order, no floating-point atomics, the same bits run to run and for any
 * chunking.  ICSG3D_FINGERPRINT_CHUNK_PAIRS (read once per process) shrinks the row x partner pairs of one launch.
 * Refused, with nothing written: a null argument (ref_q / ref_q_d may be null when nref == 0), len < 1, nq < 1,
 * nref < 0, a non-finite entry in a valid row (naming the row).
 * HOST pointers, any nq / nref (chunked internally), synchronous, the calling thread's op stream. */
int ics_op_fingerprint_nearest(const double* fp, const int32_t* valid, int len, int nq, int nref, int32_t* q_ref,
                               double* q_ref_d, int32_t* ref_q, double* ref_q_d, int32_t* q_q, double* q_q_d,
                               double* div_sum, int64_t* div_pairs);

/* ---------------------------------------------------------------- pictures (view_results.py)
 * The panels of view_results.py:152-183 -- viz.py:184-233 (the voxel panels of M, S and the watershed regions) and
 * viz.py:43-66 (plot_points_3d, the atoms) -- as ray casts at full resolution; the reference shrinks every volume to 10^3
 * because matplotlib draws one polygon set per voxel.  The picture is this library's own: no parity with matplotlib's
 * polygon renderer is claimed.
 * Camera: camera[2] = (elev, azim) in degrees as matplotlib's 3-D axes define them (defaults 30, -60); orthographic, width x
 * height pixels, looking at the grid centre, array axis 0 = x, 1 = y, 2 = z (up); the pixel-to-ray formula and the
 * compositing rule (path-length weighted front-to-back "over") are written down once, in icsg3d_amd/csrc/render.h.
 * out: float32 premultiplied RGBA in [0, 1], [batch][height][width][4].
 * All four refuse, with nothing written: batch outside [1, 65535], d outside [1, 256], an image side outside [1, 4096], a
 * null argument, a camera that is not finite, alpha outside [0, 1], npal < 1.
 * The three ics_op_* take HOST pointers, any batch (chunked internally), synchronous, the calling thread's op stream.
 *
 * ics_op_render_density (viz.py:184-233 on M): vol [batch][d][d][d][stride_c] float32, channel `channel`.  Colour is
 * lut[idx] (lut [256][3] float32) with matplotlib's index rule for floats: idx = int(v * 256), v == 1 -> 255, v < 0 -> 0,
 * v > 1 -> 255; NaN is empty.  mode 0: every voxel with v > floor has opacity alpha (floor < 0: the reference's picture,
 * everything drawn at alpha = 0.2); mode 1: opacity alpha * clip(v, 0, 1). */
int ics_op_render_density(const float* vol, int batch, int d, int stride_c, int channel, const float* lut, int mode,
                          float alpha, float floor, const double* camera, int width, int height, float* out);
/* viz.py:184-233 on S and on the watershed regions: labels [batch][d][d][d] int32; label 0 (or below) is empty, label k is
 * drawn in palette[(k - 1) % npal] (palette [npal][3] float32) at opacity alpha (the reference: 0.5). */
int ics_op_render_labels(const int32_t* labels, int batch, int d, const float* palette, int npal, float alpha,
                         const double* camera, int width, int height, float* out);
/* viz.py:43-66 (plot_points_3d): atoms in the packed layout of ics_op_structure_screen (sample b holds atoms offsets[b] ..
 * offsets[b+1]), xyz in voxel units, each a sphere of `radius` voxels.  Analytic ray-sphere intersection in fp64, the
 * nearest hit wins; colour palette[species mod npal] times max(0, n . eye), alpha 1; a miss is transparent.  Also refused:
 * offsets that do not start at 0 or decrease, a non-finite coordinate, radius <= 0. */
int ics_op_render_atoms(const int32_t* offsets, const int32_t* species, const double* xyz, int batch, int d, double radius,
                        const float* palette, int npal, const double* camera, int width, int height, float* out);
/* view_results.py:152-183, the M panels: the density picture of what the VAE engine holds, channel 0, read where it lies in
 * device memory.  which = 0: the resident input batch; which = 1: the reconstruction as the last decoder pass left it.
 * out [resident batch][height][width][4] is bit-identical to ics_op_render_density on the same values.  Refused: no
 * resident batch (also after ics_vae_interpolate, which clears the mark), which = 1 before any decoder pass over it. */
int ics_vae_render_resident(ics_net* vae, int which, int mode, float alpha, float floor, const float* lut,
                            const double* camera, int width, int height, float* out);

/* ---------------------------------------------------------------- training monitors
 * What the reference's two train loops draw when the validation loss improves: TrainingPlot.plot_segmentations,
 * plot_binary and plot_losses (unet/unet.py:39-157) and LatticeDFCVAE.plot_reconstructions, plot_samples, plot_kde and
 * plot_losses (vae/lattice_vae.py:327-337, 359-436), as three operations.  Their formulas are written down once, in
 * icsg3d_amd/csrc/monitor.h; no text is drawn, and no parity with matplotlib's resampling, antialiasing or layout is
 * claimed -- the colour index of a slice and the KDE are the parity claims.
 *
 * ics_op_render_slice: imshow(V[b, :, :, index, c]) with vmin / vmax the slice's own minimum and maximum.  vol
 * [batch][d][d][d][stride_c] of float32 (dtype 0), uint8 (1) or int32 (2), HOST pointer; channel `channel`, plane `index`
 * of array axis `axis`; row and column of the picture are the two remaining axes in array order, row 0 at the top; every
 * voxel becomes zoom x zoom pixels.  range_or_null: (vmin, vmax), or NULL for each image's own minimum and maximum over its
 * finite values.  Colour, in fp32: t = (v - vmin) / (vmax - vmin), index = min(255, (int)(t * 256)), t < 0 -> 0 (the rule
 * of ics_op_render_density after the normalisation); vmax == vmin -> 0 (matplotlib's Normalize); a non-finite value is left
 * out of the range and drawn transparent.  lut [256][3] float32.  out: float32 premultiplied RGBA, alpha 1,
 * [batch][d zoom][d zoom][4].  Any batch (chunked internally), synchronous, the calling thread's op stream.
 * Refused, with nothing written: a null argument, batch outside [1, 65535], d outside [1, 256], dtype, axis, index or
 * channel out of range, zoom outside [1, 64], an image side d * zoom above 4096, a range that is not finite or has
 * vmax < vmin. */
int ics_op_render_slice(const void* vol, int dtype, int batch, int d, int stride_c, int channel, int axis, int index,
                        const float* lut, const float* range_or_null, int zoom, float* out);
/* The same picture of the first `count` samples of what an engine holds, read where it lies in device memory and
 * bit-identical to ics_op_render_slice on the same values.
 * VAE, which = 0: the resident input batch; 1: the reconstruction a decoder pass has left since that batch came (a new
 * resident batch discards it here, so a picture never pairs an input with the reconstruction of the batch before).
 * U-Net, which = 0: the resident input batch; 1: the uint8 argmax species of the last labels predict
 * (ics_unet_predict_labels, ics_unet_predict_resident with labels_only); 2: the sigmoid probability of the last
 * probabilities predict (ics_unet_predict, ics_unet_predict_resident without labels_only); 3: the true labels uploaded with
 * the resident batch.  channel must be 0 for which = 1, 2, 3.
 * Also refused: no resident batch, count above it, VAE which = 1 before a decoder pass over `count` samples of this resident batch, U-Net
 * which = 1 after a probabilities-only predict (or none), which = 2 after a labels-only predict (or none), which = 3 for a
 * batch uploaded without labels.  Any other forward pass of the U-Net engine (a train or test step, a fused tail that
 * drives it) and a new resident batch discard what the last predict left. */
int ics_vae_render_slice_resident(ics_net* vae, int which, int channel, int count, int axis, int index, const float* lut,
                                  const float* range_or_null, int zoom, float* out);
int ics_unet_render_slice_resident(ics_net* unet, int which, int channel, int count, int axis, int index, const float* lut,
                                   const float* range_or_null, int zoom, float* out);

/* plot_kde (vae/lattice_vae.py:359-386): scipy.stats.gaussian_kde of every latent dimension, one launch for all of them,
 * entirely in fp64 over float32 codes z [n][dim] kept on the device.  For dimension j: var_j the sample variance (ddof = 1,
 * two passes), h2_j = var_j * n^(-2/5) (Scott's rule), density[j][k] = sum_i exp(-(x_k - z_ij)^2 / (2 h2_j)) /
 * (n sqrt(2 pi h2_j)).  bandwidth [dim] = sqrt(h2_j) and status [dim] are optional: status 1 marks a dimension with h2_j == 0
 * or not finite, whose density row is NaN (scipy raises LinAlgError there; here the call succeeds: a collapsed dimension is
 * what the plot is for); *count (optional) = n.
 * ics_op_kde_append takes HOST codes [rows][dim]; ics_op_kde_append_vae takes `batch` rows of what the VAE engine's last
 * encoder pass left, device to device: which = 0 z_mean, 1 the sampled z.  A non-finite code on that path is not seen by
 * the host and gives its dimension status 1.
 * Refused: a null argument, dim outside [1, 4096], capacity outside [2, 2^20], appending past the capacity, a non-finite
 * host code, evaluating with fewer than 2 codes, npts outside [1, 4096], a NaN grid point, an engine of another latent
 * width or device, no encoder pass since the engine's resident batch came (an upload alone is not one), batch above the
 * batch that pass ran on. */
typedef struct ics_kde ics_kde; /* opaque: the codes appended so far */
int ics_op_kde_create(int dim, int capacity, ics_kde** out);
int ics_op_kde_destroy(ics_kde* h);
int ics_op_kde_append(ics_kde* h, const float* codes, int rows);
int ics_op_kde_append_vae(ics_kde* h, ics_net* vae, int batch, int which);
int ics_op_kde_evaluate(ics_kde* h, const double* x, int npts, double* density, double* bandwidth, int32_t* status,
                        int* count);

/* plot_losses and the KDE curves: ncurves polylines of npts points, xy [ncurves][npts][2] float64 in data units, HOST
 * pointer.  A point that is not finite breaks the line (frames, tick marks and shorter curves are NaN-padded polylines).
 * window = (x0, x1, y0, y1) maps onto width x height pixels: px = (x - x0) / (x1 - x0) width, py = (1 - (y - y0) /
 * (y1 - y0)) height.  A curve covers a pixel by max over its segments of clamp(width_px / 2 + 0.5 - dist, 0, 1), dist the
 * distance from the pixel centre to the segment; curves are composited "over" in index order at opacity alpha * coverage in
 * colour palette[curve % npal] (palette [npal][3] float32), in fp64, rounded to float32 once.  out: premultiplied RGBA
 * [height][width][4].  Synchronous, the calling thread's op stream.
 * Refused: a null argument, npts outside [2, 4096], ncurves outside [1, 65535], an image side outside [1, 4096], a window
 * that is not finite or has x0 == x1 or y0 == y1, width_px <= 0, alpha outside [0, 1], npal < 1. */
int ics_op_render_lines(const double* xy, int ncurves, int npts, const double window[4], const float* palette, int npal,
                        double width_px, float alpha, int width, int height, float* out);

/* ---------------------------------------------------------------- interpolation (interpolate.py)
 * interpolate(a, b, cond, vae, num_interps, return_zs, max_alpha) (interpolate.py:47-64): encode both crystals under one
 * condition, walk a straight line between their SAMPLED codes (the encoder's third output, F8), decode every point.
 * alpha = np.linspace(0, max_alpha, num_interps) (interpolate.py:55) is passed in as `steps` doubles, any finite values.
 * mode 0, lerp -- the reference's arithmetic bit for bit (interpolate.py:54-56: a float32 difference, a float64 product
 * and sum, one rounding to float32 when Keras feeds the decoder):
 *     path[k][j] = fl32( fl64(za[j]) + alpha[k] * fl64( fl32(zb[j] - za[j]) ) ),   product and sum rounded separately;
 * mode 1, slerp (new, opt-in), in float64 from the float32 codes: c = a.b / (|a||b|), w = acos(clamp(c, -1, 1)),
 * s = sqrt(1 - c c), path[k] = fl32( sin((1 - t) w)/s a + sin(t w)/s b ), t = alpha[k]; a pair with |a| == 0, |b| == 0 or
 * s < 1e-3 takes the lerp for all its steps.  The dot products are summed in a fixed order: same bits run to run.
 *
 * ics_op_latent_path: the kernel alone (interpolate.py:54-56).  HOST pointers: za, zb [pairs][latent], path
 * [pairs][steps][latent]; any pairs (chunked internally), latent >= 1, steps >= 1; synchronous, the calling thread's op
 * stream and scratch. */
int ics_op_latent_path(const float* za, const float* zb, int pairs, int latent, const double* alpha, int steps,
                       int mode, float* path);
/* The whole of interpolate() for `pairs` pairs (interpolate.py:50-59): a, b [pairs][d^3][C], cond [pairs][cond_shape]
 * (tiled to every step, interpolate.py:58), eps_a, eps_b [pairs][latent] the sampling draws of the two encoder calls.
 * Outputs, each optional (NULL to skip): z_ends [pairs][2][latent] = (z_a, z_b); z_path [pairs][steps][latent];
 * recon [pairs*steps][d^3][C], frame p*steps + k.
 * One device-resident chain per group of g = min(max_batch / 2, max_batch / steps, pairs left) pairs: the 2g endpoints
 * (a0, b0, a1, b1, ...) in one encoder pass (learning phase 0), the path from the encoder's z into the decoder's
 * [z | cond] input, the decoder on g*steps frames.  Within one group the results are bit-identical to ics_vae_encode of
 * those 2g grids, ics_op_latent_path of its z and ics_vae_decode of the path at batch g*steps.
 * Refused, naming the argument, with nothing written and the handle usable afterwards: pairs < 1, steps < 1,
 * steps > max_batch, max_batch < 2, a non-finite alpha, an unknown mode, a null a / b / cond / eps_a / eps_b / alpha.
 * The chain OVERWRITES the engine's input batch with the endpoints and clears the resident-batch mark: a later
 * ics_vae_train_step_resident / ics_vae_reconstruct_resident_to_unet_atoms is refused ("no resident batch") until a
 * batch is uploaded again. */
int ics_vae_interpolate(ics_net* vae, const float* a, const float* b, const float* cond, const float* eps_a,
                        const float* eps_b, int pairs, const double* alpha, int steps, int mode, float* z_ends,
                        float* z_path, float* recon);
/* The same chain continued per group exactly as ics_vae_decode_to_unet_atoms (generate.py:204-236 for every frame of
 * interpolate.py:57-59): outputs as there for pairs*steps frames, frame p*steps + k, each optional except counts /
 * atom_stats; bit-identical to ics_vae_decode_to_unet_atoms of z_path at the group's batch.  A group's frames must fit
 * both engines: the chain GROUPS by the smaller limit, g = min(vae max_batch / 2, min(vae, unet max_batch) / steps),
 * and refuses only steps above that smaller max_batch -- and a U-Net of another d / C / device, a null counts /
 * atom_stats, max_atoms < 1, and everything ics_vae_interpolate refuses. */
int ics_vae_interpolate_to_unet_atoms(ics_net* vae, ics_net* unet, const float* a, const float* b, const float* cond,
                                      const float* eps_a, const float* eps_b, int pairs, const double* alpha, int steps,
                                      int mode, float thresh, int min_voxels, int max_atoms, float* z_ends,
                                      float* z_path, uint8_t* species, uint8_t* mask, float* density,
                                      float* coord_minmax, int32_t* regions, int32_t* counts, int32_t* atom_stats,
                                      int64_t* convexity_bounds);

/* ---------------------------------------------------------------- common to both engines */
int ics_net_destroy(ics_net* net);
int ics_net_sync(ics_net* net);
/* model.save_weights / load_weights / get_weights (unet/unet.py:261-264,378; lattice_vae.py:149,339):
 * named tensors in Keras layouts (conv kernel (3,3,3,Cin,Cout), dense (in,out)); BatchNorm moving
 * statistics are the non-trainable entries. */
int ics_net_num_tensors(ics_net* net, int* count);
int ics_net_tensor_info(ics_net* net, int index, const char** name, int* ndim, int64_t dims[5],
                        int* trainable);
int ics_net_set_tensor(ics_net* net, const char* name, const float* host, size_t count);
int ics_net_get_tensor(ics_net* net, const char* name, float* host, size_t count);
/* gradient of the last train step w.r.t. a trainable tensor (parity tests) */
int ics_net_get_grad(ics_net* net, const char* name, float* host, size_t count);
/* stored pre-BatchNorm activation s = pre_act(conv+b) of a conv layer ("c1".."c18", "e0".., "d0"..)
 * from the most recent forward, (B*S^3*Cout) floats.  Parity tests use it to pin ReLU masks whose
 * pre-activation is within fp32 rounding of the kink. */
int ics_net_get_activation(ics_net* net, const char* layer, float* host, size_t count);
/* the fp32 BatchNorm affine (scale = gamma*rstd, shift = beta - mean*scale) the most recent forward
 * applied to that layer's output; lets a test reproduce the engine's max-pool routing bit-exactly. */
int ics_net_get_bn_affine(ics_net* net, const char* layer, float* scale, float* shift, size_t count);
/* Diagnosis aid (round 6): with ICSG3D_DEBUG_CANARY=1 in the environment when the handle is created, every device buffer of
 * the handle is followed by 8 KB of guard bytes; this reports how many guards were written to (kernels running past the end of
 * their buffer) and describes the first few in ics_last_error(). */
int ics_net_check_canaries(ics_net* net, int* dirty);
int ics_net_set_lr(ics_net* net, float lr);
/* optimizer step counter (Adam t) and reset of its moments */
int ics_net_reset_optimizer(ics_net* net);
/* Adam moments over the flat parameter buffer (same order as the trainable tensors) + step count: lets the
 * host keep the optimizer state of keras.optimizers.Adam (unet/unet.py:245) when it re-creates an engine
 * for a larger batch.  count = ics_net_num_params. */
int ics_net_num_params(ics_net* net, size_t* count);
int ics_net_get_optimizer_state(ics_net* net, float* m, float* v, size_t count, int* step);
int ics_net_set_optimizer_state(ics_net* net, const float* m, const float* v, size_t count, int step);

/* Per-kernel timing with HIP events on the engine's stream (bench.py roofline): enable, run steps,
 * then read back rows {label, launches, total_ms, total_flop, total_bytes}. */
/* Two engines of one process on ONE stream: `net` enqueues on `other`'s stream from now on (its own is kept for destruction),
 * so their steps alternate in program order with no events and no host waits.  New (the reference trains its two nets in
 * separate runs): joint U-Net + DFC-VAE training on one GPU.  `other` must outlive `net`'s use of it. */
int ics_net_share_stream(ics_net* net, ics_net* other);
/* Device-clock bracket on the engine's stream: start records an event; stop records another, waits for it and returns the
 * milliseconds between them (bench.py's gpu_active_s, the self-check of ms_per_step). */
int ics_net_timer_start(ics_net* net);
int ics_net_timer_stop(ics_net* net, double* ms);
/* Measurement aid (no reference counterpart): the resident train step eagerly and as a replayed
 * hipGraph, milliseconds per step over `iters` steps each, and the number of nodes the captured graph holds.  The replay
 * repeats the captured step's host-computed Adam step size: for timing, not for training. */
int ics_net_graph_probe(ics_net* net, int iters, double* eager_ms, double* graph_ms, int* graph_nodes);
int ics_net_profile_enable(ics_net* net, int on);
/* Restrict the events to the launch sites whose label starts with `prefix` -- or with one of several prefixes separated by
 * ';' -- (NULL / "" = every launch): bench.py times its K steps with events on the dominant kernel's launch sites only, so
 * that the timed region is the training job. */
int ics_net_profile_filter(ics_net* net, const char* prefix);
int ics_net_profile_count(ics_net* net, int* rows);
int ics_net_profile_row(ics_net* net, int row, const char** label, int64_t* launches, double* total_ms,
                        double* total_flop, double* total_bytes);

/* ---------------------------------------------------------------- data parallel (new)
 * One process per GPU; the flat fp32 gradient buffer is summed over the ranks in ~4 buckets (last layer
 * first) on a second HIP stream while the backward pass continues, and scaled by 1/nranks inside Adam.
 * Loss / metric numerators and denominators are all-reduced when a step returns metrics (every rank must
 * ask on the same steps).  uid is an ncclUniqueId (128 bytes) from rank 0. */
int ics_comm_unique_id(char uid[128]);
int ics_net_comm_init(ics_net* net, int rank, int nranks, const char uid[128]);
int ics_net_comm_allreduce_max(ics_net* net, double* value); /* barrier + max over ranks */
/* rank `root`'s parameters, BN moving statistics, Adam moments, step count and (U-Net) class-weight table with its
 * active flag overwrite everyone's: replicas start identical (the class API initialises from an unseeded RNG) and train
 * with one loss.  No-op without a communicator. */
int ics_net_comm_broadcast_state(ics_net* net, int root);
/* 1: BatchNorm batch statistics (forward) and their gradient sums (backward) are exchanged over the
 * communicator, so N replicas x B grids normalise exactly like one process at N*B (the reference is
 * single-process: vae/lattice_vae.py:296, unet/unet.py:370).  0 (default): per-replica statistics; the
 * moving statistics are then averaged over the ranks after every step. */
int ics_net_set_sync_bn(ics_net* net, int on);
/* nranks = 0 without a communicator; buckets_last_step = gradient all-reduce messages of the last step */
int ics_net_comm_info(ics_net* net, int* rank, int* nranks, int* buckets_last_step);

/* ---------------------------------------------------------------- single-op entry points
 * (kernel parity tests against oracle/; host buffers, NDHWC)
 * The two conv3d ops run the engines' conv_forward / conv_backward on the one-layer handle of ics_op_conv_layer (below):
 * one plain source, no BatchNorm, max_batch = B, split-K off.  y = pre_act(conv(x, w) + bias), bias optional (zeros);
 * dx, dw optional: a NULL dx skips backward-data, a NULL dw is only not copied out. */
int ics_op_conv3d_forward(const float* x, const float* w, const float* bias, int B, int S, int Cin,
                          int Cout, int taps, int pre_act, float* y);
int ics_op_conv3d_backward(const float* x, const float* w, const float* dy, int B, int S, int Cin,
                           int Cout, int taps, float* dx, float* dw);

/* One convolution layer the way the ENGINES run it (kernel parity tests, tests/test_gpu_conv_layer.py): a temporary handle
 * with a single layer is built from the engines' own construction, packing and dispatch code, so a launch here takes the
 * template instantiation a training step takes -- BatchNorm-affine / activated / upsampled sources, the per-block
 * (count, mean, M2) statistics epilogue, accumulate on top of the up-channel launch, workspaces sized for max_batch.
 * The two entry points above launch the kernels in their plain form (one plain source, no statistics).
 *
 *   virtual input = channel concat over the sources of  act(x * scale + shift), nearest-upsampled by 2 where up = 1,
 *                   zero "same" padding AFTER that
 *   y     = pre_act(conv(virtual input, w) + bias)                       (stored, returned in y)
 *   o     = post_act(y * scale + shift), scale = gamma * rstd, shift = beta - mean * scale   (has_bn; batch statistics)
 *   dout  = gradient w.r.t. o (has_bn = 0: w.r.t. y), optional: without it only the forward pass runs
 *
 * Activations: 0 none, 1 ReLU, 2 LeakyReLU(0.3).
 * A condition source (src[1].bcast > 0) is the VAE encoder's Reshape -> K.tile -> Concatenate: spatially constant channels
 * behind the x channels.  The layer is then built as vae_build builds e0 -- whether the condition fold serves it (one x
 * channel, 16 or 32 filters, neither ICSG3D_NO_COND_FOLD nor ICSG3D_NO_THIN_C) is decided by the engine's own predicate,
 * every other configuration goes through the broadcast loader or the materialised padded input.
 * The ICSG3D_NO_* switches are read when the call builds its handle, as for every handle.  With ICSG3D_DEBUG_CANARY=1 the
 * call checks the guard bytes behind every buffer of the handle and fails, naming the buffers, if any was written to. */
typedef struct ics_conv_layer_src {
  const float* x;     /* [B][S^3][C], or [B][(S/2)^3][C] with up = 1                                     */
  const float* scale; /* [C] per-channel affine, or NULL (then shift is NULL too)                        */
  const float* shift;
  int C, up, act;
  int bcast;          /* > 0: a spatially constant source.  x is [B][bcast], C the number of channels it stands for
                         (C = bcast * channels of src[0]) and channel c has the value x[b][c % bcast].  Only as the last
                         of two sources, in a 3x3x3 layer, without affine, activation, up -- and without dx: the engines
                         never differentiate with respect to the condition, the call refuses it                    */
  float* dx;          /* out, optional (needs dout): gradient w.r.t. act(x * scale + shift), shaped as x */
} ics_conv_layer_src;
typedef struct ics_conv_layer {
  int B, max_batch;   /* the step runs B <= max_batch samples; the handle and every workspace are sized for max_batch */
  int S, taps, Cout;  /* S a power of two (>= 2 with an upsampled source); taps 27 (3x3x3 same) or 1                   */
  int pre_act, has_bn, post_act;
  int pad_input;      /* 1: thin inputs are zero-padded to the vector loaders' width (U-Net c1, VAE e0)                */
  int nsrc;           /* 1 or 2                                                                                        */
  ics_conv_layer_src src[2];
  const float *w, *bias, *gamma, *beta; /* w [taps][Cin][Cout], Cin = sum of src[].C; bias optional (zeros); gamma / beta
                                           [Cout], required with has_bn                                               */
  const float* dout;  /* [B][S^3][Cout] or NULL                                                                        */
  float* y;           /* out [B][S^3][Cout]                                                                            */
  float *mean, *rstd, *scale, *shift, *moving_mean, *moving_var; /* out [Cout], each optional (has_bn): the batch
                                           statistics, the affine, and the moving statistics after one update from (0, 1) */
  int rows_per_block; /* out: rows per statistics block (0: blocks of a parity launch over the low-res grid) ...      */
  int blocks;         /* ... and the number of blocks handed to the finalize kernel (has_bn)                           */
  float *dw, *dbias, *dgamma, *dbeta; /* out, each optional (need dout): [taps][Cin][Cout], [Cout], [Cout], [Cout]    */
  char* kernels;      /* out, optional: one line per launch site, "conv_fwd:L|<kernel>", "conv_fwd:L.up|<kernel>",
                         "conv_dgrad:L|<kernel>", "conv_wgrad:L.skip|<kernel>", ... -- <kernel> is the exact template
                         instantiation (as rocprofv3 names it) the site launched                                       */
  int kernels_cap;    /* bytes behind `kernels` (the text is truncated to fit, always NUL-terminated)                 */
  int ranks;          /* 0: one process, no SyncBN (every field as described above).  R = 1 .. 4: R data-parallel ranks
                         with SyncBN, EMULATED in this one call -- see "emulated ranks" below                          */
} ics_conv_layer;
/* Emulated ranks (ics_conv_layer.ranks, ics_conv_link.ranks = R in 1 .. 4).  B is then the PER-RANK batch and every rank
 * holds an equal shard: the SyncBN backward divides by B * S^3 * R (launch_layer_bwd and launch_head_bnfuse take the global
 * count as n * nranks), so unequal shards are not served, here or in a real data-parallel run.  Every input and output
 * tensor with a batch dimension holds R * B samples, rank-major (rank r owns samples [r B, (r + 1) B)); every other output
 * gets a leading [R]: mean, rstd, scale, shift, the moving statistics, dw, dbias, dgamma, dbeta (the parameter gradients
 * are each rank's LOCAL sums -- the gradient all-reduce of a train step is not part of this call), and `kernels` /
 * `sites`, which hold R texts of kernels_cap / sites_cap bytes each.  The parameters are shared by the ranks.
 * The call runs the body described above once per rank on that rank's shard, one rank after another on one stream, each
 * with a handle of its own whose SyncBN exchanges (the all-gather of launch_bn_finalize, the all-reduce of
 * launch_layer_bwd) go through device tables that outlive the handles instead of through RCCL; it repeats the ranks until
 * no table entry changes any more (at most collectives + 1 times, else it fails naming the collective) and returns the
 * outputs of the last repetition.  Every decision that depends on SyncBN being on (no producer BatchNorm-backward folds
 * that need local statistics, no xhat affine) is then taken as in a multi-rank run.  R = 1 runs the SyncBN kernels with
 * one rank.  No second process, no thread, no RCCL. */
int ics_op_conv_layer(ics_conv_layer* a);

/* Two or three layers LINKED the way the engines link them (kernel parity tests, tests/test_gpu_conv_link.py): a producer
 * P, fed by the plain tensor x0, and its consumer(s), built, packed, run forward (training) and backward by the engines' own
 * functions, with the gradient sources and the `next` argument unet_backward gives that link.  What one layer alone cannot
 * reach runs here: the consumer's backward-data launch that sums, or applies, the PRODUCER's BatchNorm backward (BwdStat,
 * conv_bnfuse_kernel, pool_bnfuse_kernel), the pool / upsample gradient sources of the BatchNorm-backward kernels, the
 * pooled-grid sums (launch_pool_presum) and the tie masks pool_fwd4_kernel leaves for them.
 *
 *   link ICS_LINK_SAME       P -> L                  L: gs_direct(dout), next = P;  P: gs_direct(L.dA)
 *        ICS_LINK_UP         P -> up -> L            L (up-split): next = P;  P: gs_direct(L.dxl) -- without the up-split
 *                                                    (ICSG3D_NO_UPSPLIT, or a width it refuses): P: gs_up(L.dA)
 *        ICS_LINK_POOL       P -> MaxPool -> K       K: gs_direct(dout);  P: gs_pool(K.dA), gs_none()
 *        ICS_LINK_POOL_SKIP  P -> MaxPool -> K  and  L = [P | up(q)], L.skip_prod = P
 *                                                    L (dout_l), then K (dout), then P: gs_pool(K.dA), g_skip(L)
 *   form 0: every layer is Conv -> ReLU -> BatchNorm (U-Net);  1: Conv -> BatchNorm -> LeakyReLU(0.3) (VAE).
 *
 * Geometry: P works on S^3 voxels (S a power of two), L on S^3 (SAME, POOL_SKIP) or (2S)^3 (UP), K on (S/2)^3; q is
 * [B][(S/2)^3][Cq].  All kernels are 3x3x3.  The handle is built as unet_build builds its own (weight gradients on the main
 * stream, Winograd kernels where their predicates accept the layer) in both forms: the VAE engine's own backward pass hands
 * no `next` to conv_backward, so form 1 of SAME / UP runs the LeakyReLU branches of the folds as a U-Net-style pass would.
 * The ICSG3D_* switches, ICSG3D_DGRAD_BNFUSE_MIN and ICSG3D_DEBUG_CANARY are honoured as in ics_op_conv_layer. */
enum { ICS_LINK_SAME = 0, ICS_LINK_UP = 1, ICS_LINK_POOL = 2, ICS_LINK_POOL_SKIP = 3 };
typedef struct ics_conv_link_layer {
  int Cout;           /* Cin follows from the link: P: C0; K: P.Cout; L: P.Cout (+ Cq in POOL_SKIP)                   */
  const float *w, *bias, *gamma, *beta; /* [27][Cin][Cout], [Cout] x 3; bias optional (zeros)                         */
  float* y;           /* out, optional: the stored activation [B][S_layer^3][Cout]                                    */
  float *mean, *rstd, *scale, *shift;   /* out, optional [Cout]                                                       */
  float *dw, *dbias, *dgamma, *dbeta;   /* out, optional                                                              */
} ics_conv_link_layer;
typedef struct ics_conv_link {
  int link, form;
  int B, max_batch, S;
  int C0, Cq;         /* channels of x0; of q (POOL_SKIP only)                                                        */
  int pool_ties_all;  /* MaxPool3D backward: 1 every tied element (TensorFlow CPU), 0 the first                        */
  const float* x0;    /* [B][S^3][C0]                                                                                 */
  const float* q;     /* [B][(S/2)^3][Cq], POOL_SKIP only                                                            */
  ics_conv_link_layer P, K, L;          /* K: POOL, POOL_SKIP; L: SAME, UP, POOL_SKIP                                 */
  const float* dout;  /* gradient w.r.t. the output of L (SAME, UP) or of K (POOL, POOL_SKIP)                         */
  const float* dout_l;/* POOL_SKIP: gradient w.r.t. the output of L                                                   */
  float* pooled;      /* out, optional: MaxPool3D(post_act(BN(P.y))) [B][(S/2)^3][P.Cout] (POOL, POOL_SKIP)           */
  float* dy_p;        /* out, optional: P's gradient w.r.t. its convolution output (behind the activation) [B][S^3][P.Cout] */
  float* dx0;         /* out, optional: [B][S^3][C0]                                                                  */
  char* sites;        /* out, optional: every profiler row of the call, one per line, in first-launch order: "bnfuse:L",
                         "pool_presum:P", "bn_act_bwd:P", "conv_dgrad:L|<kernel template instantiation>", ...          */
  int sites_cap;      /* bytes behind `sites` (truncated to fit, always NUL-terminated)                               */
  int ranks;          /* 0: no SyncBN; 1 .. 4: emulated data-parallel ranks with SyncBN, B per rank (see ics_conv_layer) */
} ics_conv_link;
int ics_op_conv_link(ics_conv_link* a);

/* The LAST link of the U-Net, c18 -> head, the way the engine runs it (kernel parity tests, tests/test_gpu_head_link.py): a
 * producer P in c18's place -- Conv 3x3x3 C0 -> 128, Conv -> ReLU -> BatchNorm, fed by the plain tensor x0 -- and the 1x1x1
 * head 128 -> ncls + 1 with the reference's two kernels and two biases, registered, allocated and packed by the functions
 * unet_build uses.  The call runs conv_forward(P) in training mode, unet_head_loss(mode 1, want_grad) and, with want_grad,
 * the head's part of unet_backward followed by what the engine runs for c18: conv_grads_from_dy(P) where the head's
 * backward-data launch already wrote P's dy (dy_in_place = 1), else conv_backward(P, gs_direct(head.dA)).
 *
 *   o  = gamma xhat + beta, xhat = (y - mean) rstd, y = relu(conv(x0, w) + bias)            (batch statistics)
 *   z  = o [wsoft | wsig] + [bsoft | bsig];  soft = softmax(z[:ncls]), sig = sigmoid(z[ncls])
 *   Loss = mean_v(wcce) + mean_v(bce) with the scalar loss_weight (<= 0: ncls) or the class_weights table, as
 *   ics_op_unet_head_weighted;  dz = dLoss/dz;  head dW = o^T dz, head dbias = column sums of dz;  d = dz [wsoft | wsig]^T;
 *   P: dgamma = sum_v d xhat, dbeta = sum_v d, dy = relu'(y) gamma rstd (d - dbeta / n - xhat dgamma / n), then dw, dbias, dx0.
 *
 * Which kernels serve the call is decided by the engine's predicates alone (head_fused_ok, head_dgrad_ok, the bnfuse
 * condition of unet_head_backward): ncls == 95 and B S^3 % 16 == 0 take head_fused_kernel, the weight-gradient GEMM on xhat,
 * head_bnfuse_kernel and head_dgrad_kernel<true>; ICSG3D_NO_HEAD_BNFUSE takes head_dgrad_kernel<false> with P's two
 * BatchNorm-backward sums folded in (ICSG3D_NO_BWD_FOLD: without them); ICSG3D_NO_FUSED_HEAD, every other ncls and every
 * other row count take the 1x1x1 GEMM + head_kernel and the implicit-GEMM backward-data.  `sites` tells them apart: the row
 * "head_fused" against "conv_fwd:head|<kernel>" + "head_softmax_loss", and "conv_dgrad:head|head_dgrad_kernel<true>",
 * "conv_dgrad:head|head_dgrad_kernel" (the <false> instantiation) or "conv_dgrad:head|conv_fwd_kernel<...>".
 * The ICSG3D_* switches, ICSG3D_DEBUG_CANARY and the refusals (before any launch, reason in ics_last_error) are those of
 * ics_op_conv_link.  ranks = 1 .. 4: emulated SyncBN ranks as in ics_conv_layer.ranks -- B per rank, x0 / labels / y / dz /
 * dy_p / dx0 rank-major, a leading [R] on every other output (metrics and sums included) and on `sites`; the collectives
 * are P's statistics gather and the head-fuse exchange of 256 doubles (without the fuse: P's backward all-reduce).  The
 * parameter gradients are each rank's local sums; P's dgamma / dbeta are, as in ics_op_conv_link, the local sums
 * sum_v d xhat and sum_v d over the rank's own voxels with the GLOBAL statistics in xhat.  metrics and sums under ranks are
 * each rank's LOCAL ones: the handle has no communicator (Net::comm is null), so the all-reduce of the seven sums that a
 * data-parallel step runs is not part of this call -- add the sums and call ics_op_unet_metrics_from_sums. */
typedef struct ics_head_link {
  int B, max_batch, S; /* S a power of two; the handle and every workspace are sized for max_batch >= B                  */
  int C0, ncls;        /* channels of x0; classes 2 .. 127                                                               */
  const float* x0;     /* [B][S^3][C0]                                                                                   */
  const float *w, *bias, *gamma, *beta;          /* P: [27][C0][128], [128] x 3; bias optional (zeros)                   */
  const float *wsoft, *bsoft, *wsig, *bsig;      /* [128][ncls], [ncls], [128], [1]                                      */
  const uint8_t* labels;                         /* [B][S^3], each < ncls                                                */
  float loss_weight;   /* <= 0: ncls                                                                                     */
  const float* class_weights;                    /* [ncls] finite, >= 0, or NULL (the scalar)                            */
  int bce_from_logits; /* ics_unet_config.bce_from_logits                                                                */
  int want_grad;       /* 0: forward and loss only (metrics, sums); 1: the backward pass too                             */
  float *y, *mean, *rstd, *scale, *shift;        /* out, optional: P's stored activation [B][S^3][128], [128] x 4        */
  float* dz;           /* out, optional: dLoss/dz [B][S^3][ncls + 1]                                                     */
  float* metrics;      /* out, optional: [5] = [Loss, lsoft, lsig, f1, wr]                                               */
  double* sums;        /* out, optional: [7] (ics_unet_metric_sums)                                                      */
  float *dwsoft, *dwsig, *dbias_head;            /* out, optional: [128][ncls], [128], [ncls + 1]                        */
  float *dw, *dbias, *dgamma, *dbeta;            /* out, optional: P's parameter gradients                               */
  float* dy_p;         /* out, optional: P's gradient w.r.t. its convolution output (behind the ReLU) [B][S^3][128]      */
  float* dx0;          /* out, optional: [B][S^3][C0]                                                                    */
  int dy_in_place;     /* out: 1 when the head's backward-data launch wrote P's dy (head_dgrad_kernel<true>)             */
  char* sites;         /* out, optional: every profiler row of the call, one per line, in first-launch order             */
  int sites_cap;       /* bytes behind `sites` (truncated to fit, always NUL-terminated)                                 */
  int ranks;           /* 0: no SyncBN; 1 .. 4: emulated data-parallel ranks with SyncBN, B per rank (see ics_conv_layer) */
} ics_head_link;
int ics_op_head_link(ics_head_link* a);

/* The two 1x1x1 heads with their losses and metrics on a GIVEN trunk output (kernel parity tests against the reference's own
 * formulas): soft = softmax(x wsoft + bsoft), sig = sigmoid(x wsig + bsig) (unet/unet.py:339-352), then
 * weighted_categorical_crossentropy / binary_crossentropy / f1_m / wr_m (unet/unet.py:159-221,252-259).
 * x [M][128], wsoft [128][ncls], bsoft [ncls], wsig [128], bsig [1], labels uint8 [M]; loss_weight <= 0: the scalar ncls.
 * mode 0: out [M][ncls+1] = probabilities (soft | sig); 1: metrics[5] and sums[7] (ics_unet_metric_sums) only;
 * 2: also out = dLoss/dlogits; + 4: binary_crossentropy in the logits form (ics_unet_config.bce_from_logits).  fused != 0: the GEMM inside the loss kernel (M % 16 == 0, ncls == 95), else GEMM + loss kernel.
 * ncls: 2 .. 127, the range of ics_unet_config.num_classes. */
int ics_op_unet_head(const float* x, const float* wsoft, const float* bsoft, const float* wsig, const float* bsig,
                     const uint8_t* labels, size_t M, int ncls, float loss_weight, int mode, int fused, float* out,
                     float metrics[5], double sums[7]);
/* The same with per-class loss weights: class_weights [ncls] (finite, >= 0) replaces the scalar in modes 1 and 2 (with a
 * table mode 0 is refused); NULL: ics_op_unet_head exactly. */
int ics_op_unet_head_weighted(const float* x, const float* wsoft, const float* bsoft, const float* wsig, const float* bsig,
                              const uint8_t* labels, size_t M, int ncls, float loss_weight, int mode, int fused, float* out,
                              float metrics[5], double sums[7], const float* class_weights);
/* metrics[5] = [Loss, lsoft, lsig, f1, wr] from the seven sums of ics_op_unet_head (ics_unet_metric_sums), added over the
 * shards of a global batch: the finalisation every rank of a data-parallel step runs after the all-reduce of the sums. */
int ics_op_unet_metrics_from_sums(const double sums[7], float metrics[5]);
/* The DFC-VAE's loss assembly on given partial sums.  mulv [B][2 * latent] = (mu | log variance); mse_partial [n_mse]
 * partial sums of the squared error over n_elems = B * voxels * channels elements; pm_partial: the partial sums of the four
 * perceptual taps one after another, pm_n[l] of them for tap l, pm_per[l] elements per sample and pm_w[l] the tap's weight.
 * phase 0: metrics[4] = [Loss, PM, MSE, KLD];  1: sums[5] = {KL, squared error, weighted PM, B, n_elems} only (out);
 * 2: metrics from sums (in; the other inputs are not read) -- the two halves a data-parallel step puts around its
 * all-reduce.  Loss = MSE + alpha PM + beta KLD. */
int ics_op_vae_loss(const float* mulv, int B, int latent, const double* mse_partial, int n_mse, double n_elems,
                    const double* pm_partial, const int pm_n[4], const double pm_per[4], const float pm_w[4], float alpha,
                    float beta, int phase, double sums[5], float metrics[4]);
/* The DFC-VAE's latent link on given inputs (kernel parity tests, tests/test_gpu_vae_latent.py): a temporary handle that
 * holds the z_mean | z_log_var GEMM (one N = 2 * latent layer over two reference kernels) and the latent buffers, built,
 * packed and run by the functions the engine's own encoder pass and train step call.
 *   mulv = h [w_mean | w_lv] + [b_mean | b_lv];  (mu | lv) = mulv;  z = mu + exp(lv / 2) eps;  zc = [z | cond]
 *   with dzc = dLoss/dzc (only its first `latent` columns are read) and KLD = mean_b(-1/2 sum_j(1 + lv - mu^2 - exp(lv))):
 *   dmulv = (dz + beta mu / B | dz eps exp(lv / 2) / 2 - beta (1 - exp(lv)) / (2 B)), dw_mean = h^T dmulv[:, :latent],
 *   dw_lv = h^T dmulv[:, latent:], dbias = column sums of dmulv, dh = dmulv [w_mean | w_lv]^T.
 * dzc = NULL: the forward pass only.  Every output is optional.  ICSG3D_DEBUG_CANARY as in ics_op_conv_layer. */
typedef struct ics_vae_latent {
  int B, max_batch;   /* the step runs B <= max_batch samples; the handle is sized for max_batch                      */
  int latent, ncond;
  float beta;
  const float* h;     /* [B][latent]: the encoder's dense output                                                    */
  const float *w_mean, *w_lv;           /* [latent][latent] each                                                      */
  const float *b_mean, *b_lv;           /* [latent] each, optional (zeros)                                            */
  const float* eps;   /* [B][latent]                                                                                  */
  const float* cond;  /* [B][ncond]                                                                                   */
  const float* dzc;   /* [B][latent + ncond], or NULL                                                                 */
  float *mulv, *z, *zc;                 /* out: [B][2 latent], [B][latent], [B][latent + ncond]                       */
  float *dmulv, *dw_mean, *dw_lv, *dbias, *dh; /* out (need dzc): [B][2 latent], [latent][latent] x 2, [2 latent], [B][latent] */
} ics_vae_latent;
int ics_op_vae_latent(ics_vae_latent* a);
/* The per-sample squared-error partial sums that feed mse_partial / pm_partial of ics_op_vae_loss, as the VAE step launches
 * them: a, b [B][per_sample]; partial_out [B][blocks_per_sample] = sums of (a - b)^2 over the blocks' chunks (a sample is cut
 * into blocks_per_sample chunks, rounded up to a multiple of 4 elements), accumulated in fp64.  grad_in_out [B][per_sample],
 * optional: coef * (b - a), written (accumulate = 0) or added to what it holds (accumulate = 1). */
int ics_op_sqdiff(const float* a, const float* b, int B, size_t per_sample, int blocks_per_sample, float coef, int accumulate,
                  float* grad_in_out, double* partial_out);
/* The pooling pass of the 125-product up-split backward alone: dy [B][S][S][S][N] -> out, the 125 blocks of every
 * 4 x 4 x 4 fine tile, 125 * B (S/4)^3 * N floats in the class-major layout of csrc/up125.h (up125_pooled_off).
 * variant 0: one wave per z type; variant 1: one wave per fine plane, every plane of a tile's window read once.
 * Refused before anything is launched: S not a power of two >= 8, N not 32 * 2^k, a batch whose blocks leave 32-bit
 * offsets.  Synchronous, the calling thread's op stream and scratch. */
int ics_op_up125_pool(const float* dy, int B, int S, int N, int variant, float* out);
/* kernel micro-benchmark on device-resident constant data, HIP-event timed: mode 0 forward
 * (ablate 0 = full kernel, 1 = MFMA+LDS reads only, 2 = MFMA only), 1 backward-data, 2 backward-weight. */
int ics_op_conv3d_bench(int B, int S, int Cin, int Cout, int taps, int mode, int ablate, int iters,
                        float* ms_per_launch);

/* ---------------------------------------------------------------- t-SNE map of the latent space
 * viz.tsne_latent (viz.py: sklearn.manifold.TSNE(n_components=2).fit_transform(Zs)) with the repulsion summed exactly
 * over all pairs, which is scikit-learn's objective at angle = 0.  Results are bit-identical
 * run to run.  Every call checks its arguments before it writes anything. */
/* The k nearest other rows of each row of x [n][dim] (1 <= dim <= 4096, 1 <= k <= n - 1) under the squared euclidean
 * distance, differences and squares accumulated in fp64 in dimension order: idx [n][k], dist2 [n][k], each row sorted
 * by (distance, index).  Host pointers, synchronous. */
int ics_op_tsne_knn(const float* x, int n, int dim, int k, int32_t* idx, double* dist2);
/* sklearn.manifold._utils._binary_search_perplexity on float32(dist2 [n][k]): cond_p [n][k] float64 conditional
 * probabilities (beta from 1, doubled / halved until bracketed, then bisected; at most 100 steps; stops at
 * |H - log(perplexity)| <= 1e-5).  0 < perplexity; host pointers, synchronous. */
int ics_op_tsne_affinities(const double* dist2, int n, int k, double perplexity, double* cond_p);

typedef struct ics_tsne ics_tsne; /* opaque: codes, affinities and the state of one gradient descent */
typedef struct ics_tsne_config {
  int dim;                    /* width of a code, 1..4096                                              */
  int capacity;               /* most codes the handle will hold, 2..2^20                              */
  int n_components;           /* 2 (anything else is refused)                                          */
  double perplexity;          /* TSNE(perplexity=30.0); must stay below the number of codes            */
  double early_exaggeration;  /* 12.0                                                                  */
  int exaggeration_iter;      /* 250 iterations at momentum 0.5 with P * early_exaggeration, <= max_iter */
  int max_iter;               /* 1000                                                                  */
  int n_iter_check;           /* 50: KL divergence and gradient norm every so many iterations          */
  int n_iter_without_progress;/* 300                                                                   */
  double min_grad_norm;       /* 1e-7                                                                  */
  double learning_rate;       /* <= 0: scikit-learn's "auto", max(n / early_exaggeration / 4, 50)      */
} ics_tsne_config;
int ics_op_tsne_create(const ics_tsne_config* cfg, ics_tsne** out);
int ics_op_tsne_destroy(ics_tsne* h);
/* rows more codes [rows][dim] from the host (finite values only) */
int ics_op_tsne_append(ics_tsne* h, const float* codes, int rows);
/* The device-resident path: the z_mean rows of the first `batch` samples of the VAE engine's most recent encoder
 * pass (ics_vae_encode, ics_vae_reconstruct_*) are copied device to device behind the handle's codes; nothing reaches
 * the host.  latent_dim must equal dim.  Non-finite codes are refused by ics_op_tsne_prepare. */
int ics_op_tsne_append_vae(ics_tsne* h, ics_net* vae, int batch);
/* the first `rows` codes back on the host (tests) */
int ics_op_tsne_get_codes(ics_tsne* h, float* out, int rows);
/* Neighbour search (k = min(n - 1, int(3 perplexity + 1))), affinities and P = (C + C^T) / sum in CSR form over the
 * codes appended so far, then the embedding is set to init [init_rows][init_cols] (init_rows = the number of codes,
 * init_cols = 2, finite) and the descent is rewound to iteration 0.  seconds (optional): wall time of the three stages.
 * Refused: fewer than 2 codes, perplexity >= the number of codes, non-finite codes, an init of another shape. */
int ics_op_tsne_prepare(ics_tsne* h, const float* init, int init_rows, int init_cols, double seconds[3]);
/* The same with P given: CSR over n <= capacity points, indptr [n + 1], column indices in [0, n), values >= 0. */
int ics_op_tsne_set_graph(ics_tsne* h, int n, const int64_t* indptr, const int32_t* indices, const double* vals,
                          const float* init, int init_rows, int init_cols);
/* P of the handle: indptr [n + 1]; indices / vals hold `capacity` entries (NULL, 0: only *nnz is returned). */
int ics_op_tsne_get_graph(ics_tsne* h, int64_t* indptr, int32_t* indices, double* vals, size_t capacity, size_t* nnz);
/* sklearn.manifold._t_sne._kl_divergence_bh(angle=0) of the embedding y [n][2] on float32(P * exaggeration):
 * grad [n][2] and the KL divergence.  Leaves the descent's state alone. */
int ics_op_tsne_gradient(ics_tsne* h, const float* y, double exaggeration, float* grad, double* kl);
/* Up to `iters` more iterations of sklearn.manifold._t_sne._gradient_descent under TSNE._tsne's schedule;
 * *done (optional) = 1 once max_iter is reached or one of the two stopping rules fired.  Synchronous. */
int ics_op_tsne_run(ics_tsne* h, int iters, int* done);
/* embedding [n][2] (optional), the KL divergence and gradient norm of the latest check, TSNE.n_iter_ (the index of
 * the last iteration run, -1 before the first) and the number of points; every pointer is optional. */
int ics_op_tsne_read(ics_tsne* h, float* embedding, double* kl, double* grad_norm, int* n_iter, int* count);

/* ---------------------------------------------------------------- fed steps: batch upload overlapped with the train step
 * The synchronous ics_*_train_step copies the batch from pageable memory on the compute stream and waits for the metrics.
 * A feed attached to an engine takes both off the step: the host writes the RAW arrays of a batch (the on-disk dtypes of
 * create_matrices.py's files, or a generator's float64 X and one-hot y) into one of `slots` pinned staging slots, a copy
 * stream uploads the slot while the previous step runs, and one pack kernel on the compute stream does what the host did
 * before: the cast to float32 (IEEE round to nearest even, ndarray.astype(np.float32)), the channel concatenate of up to
 * two x parts into NDHWC, and the labels as uint8 class ids.  The result is bit-identical to the synchronous step on the
 * host-prepared arrays.  icsg3d_amd/csrc/feed.h states the ordering rules.
 *
 * x parts: part i is [batch][d][d][d][x_channels[i]] of x_dtype[i] = 0 (float32, the code of ics_op_render_slice) or 3
 * (float64); the channels add up to the engine's in_channels.  label_kind: 0 none (VAE engines), 1 uint8 ids, 2 float64
 * ids (species_matrices), 3 float32 ids -- each [batch][d][d][d] -- or 4 one-hot float32 [batch][d][d][d][num_classes],
 * reduced by np.argmax's rule (the lowest index among equal maxima; the first NaN, if there is one).  Ids outside 0..255
 * and non-integer ids are the caller's error: they are converted as (uint8)(int)v, and nothing checks them.  A U-Net
 * feed needs labels (kind 1..4), a VAE feed carries cond [batch][cond_shape] and eps [batch][latent_dim] float32. */
typedef struct ics_feed_config {
  int slots;          /* 2..4 staging slots, each laid out for max_batch samples               */
  int x_parts;        /* 1 or 2                                                                */
  int x_channels[2];  /* channels of each part; their sum is the engine's in_channels          */
  int x_dtype[2];     /* 0 float32, 3 float64                                                  */
  int label_kind;     /* 0 none, 1 uint8 ids, 2 float64 ids, 3 float32 ids, 4 one-hot float32  */
} ics_feed_config;
/* Refused while a feed is open, and on any mismatch with the engine (channel sum, a label kind the engine has no use for). */
int ics_net_feed_open(ics_net* net, const ics_feed_config* cfg);
/* Drains the copy stream and the compute stream first; the pinned memory of every slot is gone afterwards.  Closing an
 * engine without a feed is refused; ics_net_destroy closes an open feed itself. */
int ics_net_feed_close(ics_net* net);
/* The pinned arrays of `slot`, each sized for max_batch samples (NULL for what the feed does not carry; every output
 * pointer is optional).  Blocks until the slot's last upload has completed -- on that event and on nothing else -- after
 * which the host may rewrite them. */
int ics_net_feed_slot(ics_net* net, int slot, void** x0, void** x1, void** labels, float** cond, float** eps);
/* Enqueues the upload of the first `batch` samples of the slot on the copy stream and returns.  Refused: a slot that was
 * not obtained (ics_net_feed_slot) since its last submit, a slot whose submitted batch no step has consumed yet,
 * batch outside [1, max_batch]. */
int ics_net_feed_submit(ics_net* net, int slot, int batch);
/* ics_net_feed_submit plus a rotation table [batch][3] (entries -1..2, the r0,r1,r2 of ics_op_voxelise); rot == NULL is
 * ics_net_feed_submit.  The table is read before the call returns. It belongs to this submit only: the step that
 * consumes the slot packs through it, a later plain submit of the same slot packs unrotated.
 * Entry r >= 0 is np.rot90(X, 1, axes=[(0,1),(0,2),(1,2)][r]) of the sample's three spatial axes, applied in the order r0,
 * r1, r2 to every per-voxel array (all x parts, ids, one-hot rows): channels travel with their voxel and no value changes
 * (the coordinate channels are neither swapped nor negated); cond and eps are untouched.  A table of -1 only takes the
 * kernel of the plain submit.  An entry outside -1..2 is refused, naming the sample and the value. */
int ics_net_feed_submit_rot(ics_net* net, int slot, int batch, const int32_t* rot);
/* Pack the submitted slot into the engine's input buffers and run the resident step on it, enqueued only: *ticket names
 * the step's metrics.  Refused: a slot that was never submitted or whose batch a step has already consumed, the other
 * engine kind. */
int ics_unet_train_step_fed(ics_net* net, int slot, int* ticket);
int ics_unet_test_step_fed(ics_net* net, int slot, int* ticket);
int ics_vae_train_step_fed(ics_net* net, int slot, int* ticket);
int ics_vae_test_step_fed(ics_net* net, int slot, int* ticket);
/* Waits for the step behind `ticket` only and returns its 5 (U-Net) or 4 (VAE) metrics.  The 64 most recent tickets
 * can be read, in any order and more than once; an older one is refused. */
int ics_net_feed_metrics(ics_net* net, int ticket, float* metrics);
/* The pack kernel alone on host arrays: x [batch][d][d][d][sum of x_channels] float32 and, with a label kind,
 * out_labels [batch][d][d][d] uint8.  cfg->slots is not read; d a power of two >= 8; num_classes 2..127 (one-hot only).
 * Synchronous, the calling thread's op stream and scratch. */
int ics_op_feed_pack(const ics_feed_config* cfg, const void* x0, const void* x1, const void* labels, int batch, int d,
                     int num_classes, float* x, uint8_t* out_labels);
/* ics_op_feed_pack through a rotation table (NULL: none). */
int ics_op_feed_pack_rot(const ics_feed_config* cfg, const void* x0, const void* x1, const void* labels,
                         const int32_t* rot, int batch, int d, int num_classes, float* x, uint8_t* out_labels);
/* Exact class counts of n label ids on the device (train_unet.py's inverse-frequency class weights): labels are uint8,
 * float64 or float32 ids (label_kind 1, 2, 3 of ics_feed_config; the one-hot kind 4 is refused), counts [ncls] is
 * OVERWRITTEN with the number of labels equal to each class id, and *out_of_range receives the number of values that are
 * no class id -- below 0, at or above ncls, non-integral, NaN -- which are counted there and index nothing.  n is arbitrary
 * (0 gives zeros); ncls 2 .. 127.  Synchronous, the calling thread's op stream and scratch. */
int ics_op_label_counts(const void* labels, int label_kind, size_t n, int ncls, int64_t* counts, int64_t* out_of_range);

/* ---- confusion matrix: the U-Net scored per species on the device (eval_unet.py, train_unet.py --class_report) ----
 * The reference scores its segmentation with two global ratios (unet/unet.py:159-193, f1_m and wr_m), both dominated by
 * the ~98 % background voxels.  A per-class table needs the argmax species of generate.py:221-222, the thresholded sigmoid
 * of generate.py:224-225 and the true labels S of unet/data.py:81-100 side by side: all three are in device memory after
 * a labels predict, so they are counted there.
 *
 * ics_op_confusion: n (true, predicted) pairs from host arrays.  true_labels are uint8, float64 or float32 ids
 * (label_kind 1, 2, 3 of ics_feed_config; the one-hot kind 4 is refused), pred is uint8.  matrix [ncls*ncls] is OVERWRITTEN:
 * [t * ncls + p] = the pairs whose values are both class ids -- t by ics_op_label_counts' rule in its own type
 * (0 <= t < ncls, integral, no NaN), p < ncls; every other pair is counted in *out_of_range and indexes nothing, so
 * sum(matrix) + *out_of_range = n.  With a mask (uint8, generate.py:224-225's sig >= thresh), occupancy[4] receives the
 * 2 x 2 table [(t != 0) * 2 + (mask != 0)] over the pairs whose t is a class id (the sigmoid target is S != 0,
 * unet/data.py:87); mask and occupancy are both NULL or both given.  n is arbitrary (0 gives zeros); ncls 2 .. 127.
 * Alignment: true_labels must be aligned to its element size (1, 4 or 8 bytes); pred and mask are bytes.  Refused with
 * nothing written: null arguments, ncls outside [2, 127], a one-hot or unknown kind, an unaligned label pointer.
 * Synchronous, the calling thread's op stream and scratch. */
int ics_op_confusion(const void* true_labels, int label_kind, const uint8_t* pred, const uint8_t* mask_or_null, size_t n,
                     int ncls, int64_t* matrix, int64_t* occupancy_or_null, int64_t* out_of_range);
/* The kernel's launch constants: lanes per block, pairs one lane takes per grid-stride pass, the grid cap.  A count
 * above threads * lane_pairs * max_blocks pairs makes every lane pass more than once (tests size their inputs by it). */
int ics_op_confusion_grid(int* threads, int* lane_pairs, int* max_blocks);
/* An accumulator [ncls*ncls + 1 + 4] of 64-bit counts in the U-Net engine's own memory (num_classes must be <= 127).
 * It is allocated by the first open -- an engine that never opens one keeps its memory layout -- and kept until the
 * engine is destroyed; opening again, like ics_unet_confusion_reset, zeroes it.  Every entry point below runs eval-mode
 * forward passes only (model.predict, generate.py:220): weights, BatchNorm moving statistics, Adam's moments and step
 * count and the class-weight table are not touched.  A VAE handle, a null argument, and a reset / step / batch / read
 * before open are refused with nothing written. */
int ics_unet_confusion_open(ics_net* net);
int ics_unet_confusion_reset(ics_net* net);
/* On the resident batch, which must have been placed WITH labels (ics_unet_upload_batch with labels,
 * ics_unet_voxelise_batch, a fed step): eval forward, argmax species and sig >= thresh (generate.py:221-225; the fused
 * head at num_classes 95, GEMM + softmax + labels kernel otherwise), then the count of (label, species, mask) added to
 * the accumulator.  Enqueued only, no host wait.  The species / mask volumes stay where a labels predict leaves them:
 * ics_unet_render_slice_resident(which = 1) works afterwards. */
int ics_unet_confusion_step(ics_net* net, float thresh);
/* The upload of ics_unet_upload_batch(x, labels, batch) followed by ics_unet_confusion_step, for callers with host
 * arrays.  Returns once the upload has read x and labels (the caller may reuse them); the forward pass and the count are
 * enqueued only, so the host can load the next batch while this one runs. */
int ics_unet_confusion_batch(ics_net* net, const float* x, const uint8_t* labels, int batch, float thresh);
/* Waits for the engine's stream and copies the accumulator out: matrix [ncls*ncls], occupancy [4], *out_of_range,
 * *voxels = the pairs counted since the last open / reset (sum(matrix) + *out_of_range).  May be called repeatedly; it
 * does not reset. */
int ics_unet_confusion_read(ics_net* net, int64_t* matrix, int64_t occupancy[4], int64_t* out_of_range, int64_t* voxels);

/* ---- atom score: the U-Net scored atom by atom on the device (eval_unet.py --atoms) ----
 * The confusion matrix above scores voxels.  What generate.py and eval.py consume is atoms: connected components of the
 * thresholded mask with a majority species and a centroid.  These entry points match the predicted atoms of a sample to
 * its true atoms and tally the result per species.
 *
 * THE RULE (the project's own, exact and deterministic).  A sample has n true and m predicted atoms, each an fp64 position
 * in voxel units and a species id in [0, ncls).  d2 = ((dx*dx + dy*dy) + dz*dz) with dx = t.x - p.x and so on, in fp64, in
 * this order, without FMA contraction.  A pair is admissible when d2 < tol*tol, strictly (tol*tol computed once on the
 * host).  The matching is the greedy one under the strict total order (d2, true index, predicted index): walk the
 * admissible pairs in ascending order and take a pair when both of its atoms are free.
 *
 * THE TALLIES, all int64 and OVERWRITTEN.  K = ncls + 1; index ncls means "no atom".
 *   matrix [K*K]      [t*K + p] matched pairs by (true, predicted) species; [t*K + ncls] unmatched true atoms (missed);
 *                     [ncls*K + p] unmatched predicted atoms (spurious)
 *   dist_q [ncls]     by true species: sum over matched pairs of llrint(sqrt(d2) * 2^20) (sqrt correctly rounded, half to even)
 *   dist2_q [ncls]    the same of llrint(d2 * 2^20)
 *   dup [ncls]        by predicted species: unmatched predicted atoms with some true atom within tol ("found twice / split")
 *   shadowed [ncls]   by true species: unmatched true atoms with some predicted atom within tol ("two atoms, one blob")
 *   hist [16]         matched distances: bin min(15, (int)floor(sqrt(d2) * (16.0 / tol)))
 *   totals [8]        samples, failed, perfect, true atoms, predicted atoms, matched, sum |n - m|, samples with no true atom;
 *                     perfect: every atom of both sides matched and every pair agreeing in species; a failed sample
 *                     (volumes and engine forms: more kept components than max_atoms on either side) adds to samples and
 *                     failed and to nothing else
 * PER-SAMPLE OUTPUTS, each optional (null): match int32 = the partner's index within the sample or -1, per true atom;
 * sample_stats int32 [batch][6] = {n, m, matched, species_agree, dup, shadowed} ({n, m, -1, -1, -1, -1} when failed);
 * dist_sum double [batch] = the sum of sqrt(d2) over the matched pairs in ascending true index, added serially (the same
 * bits run to run; NaN when failed).
 *
 * ics_op_atom_score: ragged sets in ics_op_match_emd's layout -- t_xyz [t_off[batch]][3], t_species [t_off[batch]],
 * t_off [batch + 1], and the same for p; match is [t_off[batch]].  Any batch (solved in chunks).  Refused with nothing
 * written, naming the sample: null required arguments, batch < 1, ncls outside [2, 127], tol not finite, <= 0 or above 1e6,
 * offsets that do not start at 0 or decrease, a set above 1024 atoms, a species outside [0, ncls), a coordinate that is not
 * finite or exceeds 1e150 in magnitude.  Synchronous, the calling thread's op stream and scratch. */
int ics_op_atom_score(const double* t_xyz, const int32_t* t_species, const int32_t* t_off, const double* p_xyz,
                      const int32_t* p_species, const int32_t* p_off, int batch, int ncls, double tol, int64_t* matrix,
                      int64_t* dist_q, int64_t* dist2_q, int64_t* dup, int64_t* shadowed, int64_t* hist, int64_t* totals,
                      int32_t* match, int32_t* sample_stats, double* dist_sum);
/* The same from volumes, without a network: true_labels, pred_species and pred_mask are uint8 [batch][d][d][d], d a power of
 * two in [2, 256] (a grid below 16 is laid into the corner of a zeroed 16^3 one).  Predicted atoms are the components of
 * pred_mask != 0 with more than min_voxels voxels, their species the majority vote of pred_species (0 when every voxel
 * carries 0); true atoms are ALL components of true_labels != 0 with the label volume as species.  An atom's position is
 * (x, y, z) = (sum x / voxels, sum y / voxels, sum z / voxels), one fp64 division each; atoms are numbered as
 * ics_op_segment_atoms numbers them.  max_atoms <= 1024; match is [batch][max_atoms] (-1 behind a sample's atoms). */
int ics_op_atom_score_volumes(const uint8_t* true_labels, const uint8_t* pred_species, const uint8_t* pred_mask, int batch,
                              int d, int min_voxels, int max_atoms, int ncls, double tol, int64_t* matrix, int64_t* dist_q,
                              int64_t* dist2_q, int64_t* dup, int64_t* shadowed, int64_t* hist, int64_t* totals,
                              int32_t* match, int32_t* sample_stats, double* dist_sum);
/* The kernel's constants: lanes per workgroup (one workgroup per sample), atoms per side and sample, and the samples and
 * atoms (both sides) one launch of ics_op_atom_score takes at most (tests size their batches by them). */
int ics_op_atom_score_limits(int* threads, int* max_atoms, int* chunk_samples, int* chunk_atoms);
/* The accumulator in the U-Net engine's own memory (num_classes <= 127, d >= 16): the counter block and two segmentation
 * workspaces for max_batch samples, allocated by the first open -- an engine that never opens one keeps its memory layout
 * -- and kept until the engine is destroyed.  Open zeroes the counters; a later open may change tol and min_voxels and
 * zeroes again, a different max_atoms is refused.  Every entry point runs eval-mode forward passes only: weights, BatchNorm
 * moving statistics, Adam's moments and step count, the class-weight table and (unless with_confusion) an open confusion
 * accumulator are not touched.  A VAE handle, a null argument and a reset / step / batch / read before open are refused. */
int ics_unet_atom_score_open(ics_net* net, double tol, int min_voxels, int max_atoms);
int ics_unet_atom_score_reset(ics_net* net);
/* On the resident batch, placed WITH labels (as ics_unet_confusion_step): eval forward, argmax species and sig >= thresh,
 * the components of the predictions (min_voxels) and of the true labels, the matching and its tallies ADDED to the
 * accumulator.  Enqueued only, no host wait.  with_confusion = 1 also adds the voxel pairs of the same labels to the open
 * confusion accumulator (one forward for both scores); without an open one it is refused.  Leaves the species / mask
 * volumes where a labels predict leaves them. */
int ics_unet_atom_score_step(ics_net* net, float thresh, int with_confusion);
/* The upload of ics_unet_upload_batch(x, labels, batch) followed by the step; returns once the upload has read x and
 * labels, like ics_unet_confusion_batch. */
int ics_unet_atom_score_batch(ics_net* net, const float* x, const uint8_t* labels, int batch, float thresh, int with_confusion);
/* Waits for the engine's stream and copies the tallies out (layout above).  May be called repeatedly; it does not reset. */
int ics_unet_atom_score_read(ics_net* net, int64_t* matrix, int64_t* dist_q, int64_t* dist2_q, int64_t* dup, int64_t* shadowed,
                             int64_t hist[16], int64_t totals[8]);

#ifdef __cplusplus
}
#endif
#endif /* ICSG3D_H */
