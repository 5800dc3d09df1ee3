/*
 * sqfa_hip.h -- C ABI of libsqfa_hip.so, the MI355X (gfx950) implementation of the
 * SQFA pairwise SPD-distance hot path.
 *
 * Plain C, plain pointers and sizes; no torch / C++ types cross this boundary.
 * All data pointers are DEVICE pointers (HBM) unless stated otherwise; all work is
 * enqueued on `stream` (a hipStream_t passed as void*), nothing synchronises.
 *
 * What each entry point replaces in the reference (paths relative to the
 * reference repository root):
 *
 *   sqfa_airm_pairwise   the whole chain executed per closure evaluation
 *       spd_inv_sqrt               src/sqfa/linalg.py:144-162   (per-class whitening)
 *       conjugate_matrix           src/sqfa/linalg.py:19-45     (all-pairs W_j A_i W_j^T)
 *       generalized_eigenvalues    src/sqfa/linalg.py:48-70     (batched eigvalsh + flip)
 *       affine_invariant_sq        src/sqfa/distances.py:46-67  (sum log^2)
 *       affine_invariant           src/sqfa/distances.py:70-89  (sqrt(. + 1e-6))
 *       fisher_rao_lower_bound[_sq] src/sqfa/distances.py:177-237 (scale = 1/2 on embeddings)
 *       closure loss               src/sqfa/_optim.py:88-96     (-mean over i>j) via uniform_weight
 *       check_distances_valid      src/sqfa/_optim.py:16-30     via nonfinite_out
 *       autograd backward of all of the above (torch LinalgEighBackward0 x2, BmmBackward)
 *                                  via gradA_out / gradB_out (closed form)
 *
 *   sqfa_gauss_class_factors, sqfa_gauss_scores   the step the reference's tutorial judges a fit by
 *       get_qda_accuracy           docs/source/tutorials/digit_processing.md (scikit-learn's
 *                                  QuadraticDiscriminantAnalysis on the features, on the host)
 *   sqfa_gauss_*_nested            the same figure against the number of filters kept, all K leading counts in one pass
 *                                  (no counterpart in the reference)
 *
 * The reference-side binding a maintainer would add is shown in INTEGRATION.md.
 */
#ifndef SQFA_HIP_H
#define SQFA_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* element types */
#define SQFA_F32 0
#define SQFA_F64 1

/* status codes (return values) */
#define SQFA_OK                 0
#define SQFA_ERR_BAD_ARGUMENT  -1   /* null pointer, negative size, bad dtype, bad shard ... */
#define SQFA_ERR_UNSUPPORTED_M -2   /* m outside [1, sqfa_hip_max_dim()] (or the smaller limit of a function) */
#define SQFA_ERR_WORKSPACE     -3   /* workspace_bytes smaller than sqfa_airm_workspace_bytes() */
#define SQFA_ERR_LAUNCH        -4   /* a HIP launch failed; see sqfa_hip_last_error() */

/* Library / build identification. */
int sqfa_hip_version(void);            /* 1000*major + minor */
const char *sqfa_hip_arch(void);       /* "gfx950" */
int sqfa_hip_max_dim(void);            /* largest matrix size m of the pair functions sqfa_airm_* (128) */

/*
 * Matrix sizes.  The sqfa_airm_* functions take 1 <= m <= 128:
 *   m <= 64       register-resident lane-group kernels (pair_kernel.hpp, pair_kernel_2d.hpp), geometry table configs.hpp
 *   64 < m <= 128 the LDS pair kernel (pair_kernel_lds.hip): one workgroup per pair at a time, the matrix in LDS, padded
 *                 size round_up(m, 8); tiles of TI x TJ pairs from 16 x 16 down to 2 x 2 chosen from (nA, nB, m) only
 *                 (every shard of a job uses the same tiling).  Of sqfa_airm_options only sweep_counter applies there (it
 *                 then counts pairs, not wave rounds); geometry_policy, class_factor_policy and mean_metric_policy are
 *                 ignored (no small-launch rows, no class factor pass).  Workspace: the factors (nA m^2 + nB m^2 / 2 values)
 *                 and a slab of P (1/TI + 1/TJ) lower triangles for P pairs: 2.1 GB at C = 1000, m = 128, float32.
 * The per-class SPD functions (sqfa_spd_function*) and the Gaussian pair terms keep m <= 64, the projection and the
 * Gaussian class scores (sqfa_gauss_scores) K <= 64.
 */
const char *sqfa_hip_last_error(void); /* text of the last HIP error seen by this library (host thread local) */

/*
 * Tile geometry used for a given problem (informational): tiles form an
 * n_tiles_i x n_tiles_j grid over (A classes) x (B classes); tile (bi,bj) is
 * processed by a call iff (bi + bj) % shard_count == shard_index (and, in self mode,
 * it contains a pair i>j).  tile_j / n_tiles_j describe the WIDEST tiling; a call
 * whose shard would not fill the GPU halves the tile width (possibly repeatedly), which
 * changes which pairs a shard evaluates but never the union over the shards of one
 * shard_count.  Returns SQFA_OK or an error code.
 */
int sqfa_airm_tiling(int nA, int nB, int m, int dtype,
                     int *tile_i, int *tile_j, int *n_tiles_i, int *n_tiles_j, int *padded_m);

/* Bytes of device workspace sqfa_airm_pairwise[_opt] needs for this problem with ANY shard_count and ANY options (0 on error). */
size_t sqfa_airm_workspace_bytes(int nA, int nB, int m, int dtype);
/* The same for calls with this shard_count and geometry policy only (the lane geometry and the tile width, hence the slab,
 * depend on them): at C=1000, m=16 55 MB for shard_count 1 (the slab holds exactly the tiles a shard owns) instead of the
 * bound above.  geometry_policy: as in sqfa_airm_options (0 for sqfa_airm_pairwise). */
size_t sqfa_airm_workspace_bytes_sharded(int nA, int nB, int m, int dtype, int shard_count, int geometry_policy);

/* Per-call options of sqfa_airm_pairwise_opt / sqfa_airm_eigenvalues_backward (NULL = all defaults).  There is no
 * process-wide policy state in the library: what a call does depends on its arguments only.
 *   geometry_policy      launches with few pairs run on "small-launch" lane geometries (more lanes per pair, same padded
 *                        sizes: configs.hpp, SQFA_CONFIGS_F32_SMALL): 0 = by pair count (default), 1 = wherever such a row
 *                        exists, -1 = never (tests run both kinds of row; A/B timing)
 *   class_factor_policy  the class factor pass K0b (pair_kernel.hpp, class_factor_kernel) runs for launches with enough
 *                        pairs to pay for its latency: 0 = by pair count (default), 1 = always, -1 = never.  Results agree
 *                        to rounding either way; every shard of a job must pass the same value.
 *   sweep_counter        NULL, or a device buffer of two uint64 {sum of Jacobi sweeps, number of wave rounds} the tile
 *                        kernel adds to atomically (introspection for benchmarks)
 *   mean_metric_policy   1 = when the factor pass runs, sizes m <= 17 and m = 25..32 orthogonalise the factor columns in the
 *                        metric of the MEAN class (class_factor_mean_kernel) instead of the plain inner product: 0.2-0.8
 *                        fewer sweeps (-8 % at m = 16 / 17) for classes that share a dominant covariance, as real class
 *                        statistics do; +1-3 % on classes scattered around a multiple of I (BASELINE's synthetic
 *                        generator), hence opt-in.  0 (default) / -1 = off.  Every shard of a job passes the same value.
 *   launch_policy        which launches a call is made of; the results are bit-identical whatever the value (tests, A/B
 *                        timing).  0 (default) = every fused launch that applies, -1 = the separate launches throughout
 *                        (Cholesky, class factor pass, pair tiles, slab reduction), > 0 = a mask of SQFA_LAUNCH_* bits: only
 *                        those fused launches.  SQFA_LAUNCH_FUSED_PROLOGUE: when the class factor pass runs in the plain
 *                        metric on a register row with m <= 24, the A side's Cholesky factor, inverse, slab slot table and
 *                        factor pass are ONE launch (class_prologue_kernel).  SQFA_LAUNCH_FUSED_REDUCTION is reserved: no call
 *                        interprets it, the slab is always reduced by finalize_kernel. */
#define SQFA_LAUNCH_FUSED_PROLOGUE  1
#define SQFA_LAUNCH_FUSED_REDUCTION 2
typedef struct sqfa_airm_options {
  int geometry_policy;
  int class_factor_policy;
  unsigned long long *sweep_counter;
  int mean_metric_policy;
  int launch_policy;
} sqfa_airm_options;

/*
 * Pairwise affine-invariant distances between two batches of SPD matrices, the
 * weighted sum of those distances, and the gradient of that sum.
 *
 *   A        (nA, m, m) row-major contiguous SPD matrices (dtype)
 *   B        (nB, m, m) or NULL.  NULL (with nB == 0) selects SELF mode: B is A and
 *            only the unordered pairs i > j are evaluated (the reference evaluates
 *            all ordered pairs and then keeps i > j, src/sqfa/_optim.py:94).
 *   scale    d2 = scale * sum_k log(lambda_k)^2      (1 for AIRM, 0.5 for Calvo-Oller)
 *   eps      D = sqrt(d2 + eps) when sqrt_mode != 0, else D = d2
 *   pair_weights  NULL, or (nA, nB) row-major (dtype): w_ij.  In SELF mode the weight
 *            of the unordered pair {i,j} is w_ij + w_ji.
 *   uniform_weight  used when pair_weights == NULL: every evaluated pair has this
 *            weight (e.g. -1/P for the closure loss, P the GLOBAL pair count).
 *   shard_index, shard_count   tile shard processed by this call (0,1 = everything).
 *   loss_out      (1) dtype: sum over evaluated pairs of w * D          (may be NULL)
 *   gradA_out     (nA, m, m) dtype: d loss / d A (SELF mode: full gradient wrt the
 *                 shared batch).  NULL = forward only (no eigenvectors kept).
 *   gradB_out     (nB, m, m) dtype, cross mode only (ignored / may be NULL in SELF mode)
 *   dist_out      (nA, nB) dtype: D_ij for evaluated pairs; SELF mode also writes D_ji
 *                 and the diagonal (sqrt(eps) or 0).  Entries of tiles outside the shard
 *                 are left untouched.                                       (may be NULL)
 *   eig_out       (nA, nB, m) dtype: generalized eigenvalues of (A_i, B_j), UNSORTED;
 *                 SELF mode mirrors 1/lambda into (j,i) and writes ones on the diagonal.
 *                                                                           (may be NULL)
 *   nonfinite_out (2) int32: {#pairs with D = NaN, #pairs with D = +-inf} among the
 *                 evaluated pairs                                           (may be NULL)
 *   workspace     device scratch of at least sqfa_airm_workspace_bytes() bytes
 *   stream        hipStream_t
 *
 * Outputs of this shard only; a multi-GPU caller sums loss/grad/nonfinite over shards.
 * Results are bitwise reproducible run to run for fixed inputs and sharding.
 */
int sqfa_airm_pairwise(const void *A, int nA, const void *B, int nB, int m, int dtype,
                       double scale, double eps, int sqrt_mode,
                       const void *pair_weights, double uniform_weight,
                       int shard_index, int shard_count,
                       void *loss_out, void *gradA_out, void *gradB_out,
                       void *dist_out, void *eig_out, int *nonfinite_out,
                       void *workspace, size_t workspace_bytes, void *stream);
/* The same call with explicit options (NULL = sqfa_airm_pairwise). */
int sqfa_airm_pairwise_opt(const void *A, int nA, const void *B, int nB, int m, int dtype,
                           double scale, double eps, int sqrt_mode,
                           const void *pair_weights, double uniform_weight,
                           int shard_index, int shard_count,
                           void *loss_out, void *gradA_out, void *gradB_out,
                           void *dist_out, void *eig_out, int *nonfinite_out,
                           void *workspace, size_t workspace_bytes, void *stream,
                           const sqfa_airm_options *options);

/*
 * Pairwise Bures-Wasserstein distances between SPD matrices (the distance_fun the reference's tutorial builds,
 * docs/source/tutorials/distances.md:127-178: bw_distance_sq / bw_distance), their weighted sum and its gradient:
 *     bw2(A, B) = tr A + tr B - 2 sum_k sqrt(lambda_k(A B)),   D = sqrt(|bw2| + eps) when sqrt_mode != 0, else D = bw2
 * Same kernels as sqfa_airm_pairwise with a second spectral function: the B-side factor is R_j (R_j^T R_j = B_j, lower
 * triangular) in place of L_j^-1, and sum_k sigma_k of X = R_j F_i replaces sum_k log^2 lambda_k.
 * Arguments, modes (self / cross), pair weights, shards, outputs and guarantees as sqfa_airm_pairwise_opt, without scale and
 * eig_out: no sync, no allocation, no float atomics; bitwise reproducible for fixed inputs and sharding; the shards of one
 * shard_count sum to the whole; a non-SPD class counts as a NaN / inf distance.  1 <= m <= 128 (SQFA_ERR_UNSUPPORTED_M).
 * options: geometry_policy, class_factor_policy and sweep_counter as for sqfa_airm_pairwise_opt; mean_metric_policy does not
 * apply (the factor pass, where it runs, uses the plain inner product).
 * Workspace: sqfa_bw_workspace_bytes[_sharded] (the affine-invariant queries are NOT enough: the B-side gradient needs
 * R_j^-1 and two more m x m double buffers per class).
 */
size_t sqfa_bw_workspace_bytes(int nA, int nB, int m, int dtype);
size_t sqfa_bw_workspace_bytes_sharded(int nA, int nB, int m, int dtype, int shard_count, int geometry_policy);
int sqfa_bw_pairwise(const void *A, int nA, const void *B, int nB, int m, int dtype,
                     double eps, int sqrt_mode,
                     const void *pair_weights, double uniform_weight,
                     int shard_index, int shard_count,
                     void *loss_out, void *gradA_out, void *gradB_out,
                     void *dist_out, int *nonfinite_out,
                     void *workspace, size_t workspace_bytes, void *stream,
                     const sqfa_airm_options *options);

/*
 * Backward of the generalized eigenvalues themselves (the reference's generalized_eigenvalues,
 * src/sqfa/linalg.py:48-70, is autograd-transparent and its tutorial builds custom distance_funs
 * on it, docs/source/tutorials/distances.md:127-178): gradient of
 *     sum_{i,j,k} eig_weights[i,j,k] * lambda_k(A_i, B_j)
 * with respect to A and B, in closed form (d lambda_k/dA = u_k u_k^T, d lambda_k/dB = -lambda_k u_k u_k^T
 * for the generalized eigenvectors U, U^T B U = I).
 *   eig_weights  (nA, nB, m) dtype, indexed like sqfa_airm_pairwise's eig_out of the SAME inputs
 *                (its unsorted column order is a deterministic function of the inputs; a caller that
 *                sorts the eigenvalues scatters its upstream gradient back through the permutation)
 *   gradA_out (nA,m,m), gradB_out (nB,m,m; cross mode); SELF mode (B NULL, nB 0): eig_weights[j,i,k]
 *                weighs the mirrored value 1/lambda_k and the result is the gradient wrt the shared batch.
 *   workspace as for sqfa_airm_pairwise; options: those of the call that produced eig_out (the column order depends on
 *   the lane geometry), NULL = defaults.
 */
int sqfa_airm_eigenvalues_backward(const void *A, int nA, const void *B, int nB, int m, int dtype,
                                   const void *eig_weights, void *gradA_out, void *gradB_out,
                                   void *workspace, size_t workspace_bytes, void *stream,
                                   const sqfa_airm_options *options);

/*
 * T_c = Psi_c F^T for c = 0..C-1: the streaming half of the projection S_c = F Psi_c F^T of the
 * class scatter matrices into feature space.  Replaces conjugate_matrix
 * (src/sqfa/linalg.py:19-45) as called by transform_scatters (src/sqfa/model.py:172-188):
 * Psi (C,D,D) is read from HBM exactly once; S_c = F T_c and, in the backward pass,
 * dL/dF = sum_c (G_c + G_c^T) T_c^T need only T (C,D,K).  Psi_c is assumed symmetric
 * (covariance / second-moment matrices).
 *   F (K,D) row-major, Psi (C,D,D), T_out (C,D,K) row-major; float32 or float64, D % 4 == 0, K <= 64, Psi 16-byte
 *   aligned -- it is read with 16-byte loads only; F and T_out may have any element alignment
 *   (SQFA_ERR_UNSUPPORTED_M otherwise, decided before any HIP call: the caller keeps its own path for those inputs).
 */
int sqfa_project_scatters(const void *F, int K, int D, const void *Psi, int C, int dtype, void *T_out,
                          void *stream);

/*
 * The same product from BLOCK-TRIANGULAR PACKED statistics: symmetric Psi_c stored once (per fit) as its lower block
 * triangle -- row blocks of 16 rows, each holding the 16 x 64 tiles of the column stripes up to and including its 64-wide
 * diagonal block, contiguous -- so that every closure streams 51-54 % of the bytes of the full tensor (D = 784: 54.1 %,
 * 2048: 51.6 %, 3072: 51.0 %) and the statistics need half the memory.  Both halves of the symmetric product come from
 * the same tile (project_packed_kernel.hip); results agree with sqfa_project_scatters to rounding (other summation order).
 *   sqfa_packed_scatter_elems(D)    elements per class of the packed form (0: D not supported)
 *   sqfa_pack_scatters              Psi (C,D,D) -> packed_out (C, sqfa_packed_scatter_elems(D)); reads the LOWER triangle
 *                                   and the diagonal blocks of Psi
 *   sqfa_project_scatters_packed    T_out (C,D,K) = Psi_c F^T from the packed form
 * float32, D % 16 == 0, 16 <= D <= 4096, K <= 64; 16-byte aligned pointers: Psi and packed_out of sqfa_pack_scatters,
 * packed and F of sqfa_project_scatters_packed, and its T_out when K % 4 == 0 (these kernels have no scalar paths)
 * (SQFA_ERR_UNSUPPORTED_M otherwise, decided before any HIP call: keep the full tensor and sqfa_project_scatters).
 * One workgroup per class: meant for C >= a few hundred classes.
 */
size_t sqfa_packed_scatter_elems(int D);
int sqfa_pack_scatters(const void *Psi, int C, int D, int dtype, void *packed_out, void *stream);
int sqfa_project_scatters_packed(const void *F, int K, int D, const void *packed, int C, int dtype, void *T_out,
                                 void *stream);

/*
 * The two small products around it, each reading T (C,D,K) once:
 *   sqfa_feature_scatters           S_c = F T_c            -> S_out (C,K,K)   (the projected scatters;
 *                                   noise / embedding are added by the caller)
 *   sqfa_feature_scatters_backward  P_g = sum over the classes c = g, g + n_groups, ... of
 *                                   (G_c + G_c^T) T_c^T  -> partial_out (n_groups,K,D); G (C,K,K) is
 *                                   the gradient wrt S; dL/dF = sum_g P_g (fixed order: reproducible)
 * They replace the einsum of conjugate_matrix (src/sqfa/linalg.py:41) and its autograd backward.
 * float32 or float64, K <= 64; forward needs D % 4 == 0
 * (SQFA_ERR_UNSUPPORTED_M otherwise: the caller keeps its own expression).
 */
int sqfa_feature_scatters(const void *F, int K, int D, const void *T, int C, int dtype, void *S_out, void *stream);
int sqfa_feature_scatters_backward(const void *G, const void *T, int C, int D, int K, int dtype, int n_groups,
                                   void *partial_out, void *stream);

/*
 * Closure glue: the same two products with the elementwise steps around them folded in, and the
 * parametrization, so that one closure evaluation is 8 (SecondMomentsSQFA) / 11 (SQFA) launches.
 *   sqfa_feature_scatters_ex        as sqfa_feature_scatters, plus `noise` added to the diagonal (the
 *                                   feature_noise regulariser, src/sqfa/model.py:537-538) and, when means_f
 *                                   (C,K) (the projected class means) is not NULL, the Calvo-Oller embedding
 *                                   [[S + m m^T, m], [m^T, 1]] (src/sqfa/distances.py:141-174) written as
 *                                   (C, K+1, K+1) into S_out
 *   sqfa_feature_scatters_backward_ex  as sqfa_feature_scatters_backward for G stored with row pitch / class
 *                                   size ldg (K, or K+1 to read the top-left block of a gradient wrt the embedding);
 *                                   g_symmetric != 0: the caller guarantees G_c = G_c^T (true for the gradients
 *                                   sqfa_airm_pairwise writes), G_c + G_c^T is then read as 2 G_c along rows only
 *   sqfa_embed_backward_means       gm_out (C,K) = (G + G^T) m + gE[:K,K] + gE[K,:K]: gradient wrt the projected means
 *   sqfa_sphere_forward             F = X / ||X||_row, norms_out (K)    (Sphere.forward, src/sqfa/constraints.py:37)
 *   sqfa_sphere_backward            grad_out (K,D) = gloss * (gF - F (F.gF)) / ||X||  with
 *                                   gF = extra + sum_g partials[g]  (partials (n_groups,K,D) from the backward
 *                                   product; extra (K,D) optional; gloss: device scalar or NULL = 1;
 *                                   norms NULL = no constraint: grad_out = gloss * gF)
 */
int sqfa_feature_scatters_ex(const void *F, int K, int D, const void *T, int C, int dtype, double noise,
                             const void *means_f, void *S_out, void *stream);
int sqfa_feature_scatters_backward_ex(const void *G, int ldg, const void *T, int C, int D, int K, int dtype,
                                      int n_groups, int g_symmetric, void *partial_out, void *stream);
int sqfa_embed_backward_means(const void *gE, const void *means_f, int C, int K, int dtype, void *gm_out, void *stream);
int sqfa_sphere_forward(const void *X, int K, int D, int dtype, void *F_out, void *norms_out, void *stream);
int sqfa_sphere_backward(const void *X, const void *norms, int K, int D, int dtype, const void *partials, int n_groups,
                         const void *extra, const void *gloss, void *grad_out, void *stream);

/*
 * L-BFGS search direction in compact form for optimizer state kept on the device (the reference optimises
 * with torch.optim.LBFGS, src/sqfa/_optim.py:78-82; this evaluates the same two-loop recursion as two
 * triangular solves and four (history x n) products in six launches, sqfa_amd/_lbfgs.py).
 *   S, Y (h, n): ring buffers of steps and gradient differences; SY (h, h): SY[i][j] = s_i . y_j; h <= 128
 *   sqfa_lbfgs_push        writes (s, y) into ring row `slot` and refreshes row and column `slot` of SY
 *   sqfa_lbfgs_direction   d_out (n) = -H g for the k pairs listed (HOST array `slots`, chronological order, no ring
 *                          row twice: SQFA_ERR_BAD_ARGUMENT); H_diag: device scalar (initial Hessian scale) or NULL = 1.
 *                          Guarantee: d_out depends only on rows `slots` of S and Y and on the entries SY[a][b] with a
 *                          and b both in `slots`; every other row and entry may hold anything, NaN included (stale
 *                          pairs of a ring that has not filled up or was reset), and d_out is bitwise the same.
 *                          Both calls write nothing but their outputs (row `slot` of S and Y, row and column `slot` of
 *                          SY; d_out) and `work`.
 *   work                   scratch of sqfa_lbfgs_work_elems(h, n) elements of the dtype, shared by both calls
 *                          (partial dot products, solve vectors, one n-vector)
 */
int sqfa_lbfgs_max_history(void);
size_t sqfa_lbfgs_work_elems(int h, int n);
int sqfa_lbfgs_push(void *S, void *Y, void *SY, int h, int n, int slot, const void *s, const void *y, void *work,
                    int dtype, void *stream);
/* y_out = g - g_prev, s_out = t d, scalars_out (5) = [max|g|, max|s|, y.s, y.y, y.s / y.y]: the element-wise part of an
 * iteration and its stopping-rule scalars in two launches; work: sqfa_lbfgs_work_elems(h, n) >= 1024 elements */
int sqfa_lbfgs_step_stats(const void *g, const void *g_prev, const void *d, double t, int n, void *y_out, void *s_out,
                          void *scalars_out, void *work, int dtype, void *stream);
int sqfa_lbfgs_direction(const void *S, const void *Y, const void *SY, int h, int n, const int *slots, int k,
                         const void *g, const void *H_diag, void *d_out, void *work, int dtype, void *stream);

/*
 * Per-pair Gaussian terms behind the reference's other distance_fun operators -- bhattacharyya
 * (src/sqfa/distances.py:240-280), mahalanobis[_sq] (:283-361), hellinger (:364-393),
 * fisher_rao_same_cov (:396-432) -- which all reduce to, with Sbar_ij = (Sigma_i + Sigma_j)/2 and
 * delta_ij = mu_i - mu_j:
 *     Q_ij  = delta^T Sbar^-1 delta          LD_ij = log det Sbar
 * The reference materialises the (nA,nB,K,K) tensor of mean covariances and runs batched inv / logdet
 * on it; here one lane group factorises one pair at a time and only (nA,nB) outputs exist.
 *   muA (nA,m), covA (nA,m,m), muB (nB,m), covB (nB,m,m): row-major, dtype; m <= 64
 *   Q_out, LD_out   (nA,nB) dtype, either may be NULL
 *   gQ, gLD         (nA,nB) dtype upstream gradients (either may be NULL), used when gcovA_out != NULL:
 *   gmuA_out (nA,m), gcovA_out (nA,m,m): gradient of sum_ij (gQ_ij Q_ij + gLD_ij LD_ij) wrt muA / covA
 *                   (full symmetric matrices).  Both NULL = forward only.
 * The B-side gradient is the same call with A and B swapped and gQ / gLD transposed; when B is A the
 * caller passes gQ + gQ^T, gLD + gLD^T and takes the A side as the total.  Deterministic (no atomics).
 */
int sqfa_gauss_pair_terms(const void *muA, const void *covA, int nA, const void *muB, const void *covB, int nB,
                          int m, int dtype, const void *gQ, const void *gLD, void *Q_out, void *LD_out,
                          void *gmuA_out, void *gcovA_out, void *stream);

/*
 * Fused closure loss of the Gaussian pair distances: for the n classes N(mu_c, Sigma_c), with Q_ij and LD_ij as above,
 * ld_c = log det Sigma_c and Bh_ij = Q_ij/8 + (LD_ij - (ld_i + ld_j)/2)/2,
 *     kind SQFA_GAUSS_BHATTACHARYYA   D_ij = Bh_ij
 *          SQFA_GAUSS_HELLINGER       D_ij = sqrt(1 - exp(-Bh_ij) + eps)
 *          SQFA_GAUSS_MAHALANOBIS_SQ  D_ij = Q_ij
 *          SQFA_GAUSS_MAHALANOBIS     D_ij = sqrt(Q_ij + eps)
 *     loss = uniform_weight * sum_{i>j} D_ij      (uniform_weight = -1/P, P = n(n-1)/2: the reference's -mean)
 * together with its gradient wrt mu and Sigma, in one pass over the pairs: the same pair kernels as
 * sqfa_gauss_pair_terms in their fused mode (the distance and its partial derivatives are formed the moment a pair is
 * factorised; no (n,n) matrix is stored unless dist_out is given, no pair is factorised twice), after a per-class
 * pre-pass for ld_c (Bhattacharyya / Hellinger only) and before a one-workgroup reduction of the per-class partial
 * losses and counters.  No float atomics anywhere: results are bitwise reproducible.
 *   mu (n,m), cov (n,m,m): row-major, dtype; n >= 2, m <= 64
 *   loss_out (1) dtype or NULL; gmu_out (n,m) and gcov_out (n,m,m, full symmetric matrices): both or neither (NULL, NULL =
 *   forward only); dist_out (n,n) or NULL: D_ij, both triangles, the diagonal as the reference gives it (0, or
 *   sqrt(eps) for the two square-root kinds); nonfinite_out (2) int32 or NULL: {#NaN, #inf} among the pairs i > j
 *   (a mean covariance that is not positive definite yields NaN and is counted, never a fault)
 *   workspace: sqfa_gauss_pairwise_workspace_bytes(n, m, dtype) bytes (0 = shape or dtype not supported)
 * Returns SQFA_ERR_BAD_ARGUMENT (null mu / cov, n < 2, dtype, kind, exactly one of gmu_out / gcov_out),
 * SQFA_ERR_UNSUPPORTED_M (m > 64), SQFA_ERR_WORKSPACE.
 */
#define SQFA_GAUSS_BHATTACHARYYA  0
#define SQFA_GAUSS_HELLINGER      1
#define SQFA_GAUSS_MAHALANOBIS_SQ 2
#define SQFA_GAUSS_MAHALANOBIS    3
size_t sqfa_gauss_pairwise_workspace_bytes(int n, int m, int dtype);
int sqfa_gauss_pairwise_loss(const void *mu, const void *cov, int n, int m, int dtype, int kind,
                             double eps, double uniform_weight,
                             void *loss_out, void *gmu_out, void *gcov_out, void *dist_out, int *nonfinite_out,
                             void *workspace, size_t workspace_bytes, void *stream);
/*
 * The same with per-pair weights:  loss = sum_{i>j} w_ij D_ij,  w_ij = pair_weights[i*n + j].
 *   pair_weights (n,n) dtype, row-major, or NULL.  NULL: this IS sqfa_gauss_pairwise_loss (same kernels, same bits);
 *   otherwise uniform_weight is ignored.  The matrix MUST BE SYMMETRIC: the kernels visit the ordered pairs -- class row i
 *   owns its gradient and weighs the pair (i, j) with w_ij, class row j weighs it with w_ji, and the loss counts j < i
 *   with w_ij -- so both entries are read and an asymmetric matrix gives a gradient that belongs to no loss.  The diagonal
 *   is never read into a result.  Every pair is evaluated and counted in nonfinite_out whatever its weight; dist_out is
 *   unweighted.  (For the closure's -sum W D / sum W the caller passes -W / sum_{i>j} W.)
 * Workspace, limits, error codes and reproducibility as above.
 */
int sqfa_gauss_pairwise_loss_weighted(const void *mu, const void *cov, int n, int m, int dtype, int kind,
                                      double eps, const void *pair_weights, double uniform_weight,
                                      void *loss_out, void *gmu_out, void *gcov_out, void *dist_out, int *nonfinite_out,
                                      void *workspace, size_t workspace_bytes, void *stream);

/*
 * Fused closure loss of the log-Euclidean distances (log_euclidean[_sq] of the reference, src/sqfa/distances.py:92-138, as
 * a model's distance_fun): for the n SPD matrices S_c, with L_c = log S_c and d2_ij = || L_i - L_j ||_F^2,
 *     sqrt_mode 0   D_ij = d2_ij
 *     sqrt_mode 1   D_ij = sqrt(d2_ij + eps)
 *     loss = uniform_weight * sum_{i>j} D_ij      (uniform_weight = -1/P, P = n(n-1)/2: the reference's -mean)
 * together with its gradient wrt S.  Stages, all on the caller's stream: the per-class stages of sqfa_spd_function (L, and
 * the double-precision U and lambda of the backward); ONE pass over the ordered pairs (log_euclidean_kernel.hip: the
 * differences L_i - L_j are formed entry by entry -- no Gram-matrix expansion, which loses the digits that matter for close
 * classes -- and every class row has one writer); sqfa_spd_function_backward on G_i = sum_{j != i} c_ij (L_i - L_j);
 * a one-workgroup reduction of the per-class partial losses and counters.  No float atomics anywhere: results are
 * bitwise reproducible.  No (n,n) matrix is stored unless dist_out is given.
 *   S (n,m,m): row-major, dtype; n >= 2, 1 <= m <= 64
 *   loss_out (1) dtype or NULL; gradS_out (n,m,m, full symmetric matrices) or NULL = forward only; dist_out (n,n) or NULL:
 *   D_ij, both triangles, the diagonal as the reference gives it (0, or sqrt(eps) for the square-root kind);
 *   nonfinite_out (2) int32 or NULL: {#NaN, #inf} among the pairs i > j (a class that is not positive definite yields
 *   NaN and is counted, never a fault)
 *   workspace: sqfa_log_euclidean_workspace_bytes(n, m, dtype) bytes (0 = shape or dtype not supported)
 * Returns SQFA_ERR_BAD_ARGUMENT (null S, n < 2, m < 1, dtype, sqrt_mode outside {0, 1}), SQFA_ERR_UNSUPPORTED_M (m > 64),
 * SQFA_ERR_WORKSPACE; every argument check runs before the first HIP call.
 */
size_t sqfa_log_euclidean_workspace_bytes(int n, int m, int dtype);
int sqfa_log_euclidean_pairwise_loss(const void *S, int n, int m, int dtype, int sqrt_mode,
                                     double eps, double uniform_weight,
                                     void *loss_out, void *gradS_out, void *dist_out, int *nonfinite_out,
                                     void *workspace, size_t workspace_bytes, void *stream);
/*
 * The same with per-pair weights:  loss = sum_{i>j} w_ij D_ij,  G_i = sum_{j != i} c_ij (L_i - L_j) with
 * c_ij = 2 w_ij | w_ij / D_ij,  w_ij = pair_weights[i*n + j].
 *   pair_weights (n,n) dtype, row-major, or NULL.  NULL: this IS sqfa_log_euclidean_pairwise_loss (same kernels, same
 *   bits); otherwise uniform_weight is ignored.  The matrix MUST BE SYMMETRIC (the pass visits the ordered pairs: row i
 *   reads w_ij, row j reads w_ji, the loss counts j < i with w_ij).  The diagonal is never read into a result.  Every pair
 *   is evaluated and counted in nonfinite_out whatever its weight; dist_out is unweighted.
 * Workspace, limits, error codes and the order of the argument checks as above.
 */
int sqfa_log_euclidean_pairwise_loss_weighted(const void *S, int n, int m, int dtype, int sqrt_mode,
                                              double eps, const void *pair_weights, double uniform_weight,
                                              void *loss_out, void *gradS_out, void *dist_out, int *nonfinite_out,
                                              void *workspace, size_t workspace_bytes, void *stream);

/*
 * Fused closure loss of the Jeffreys divergence (the symmetric Kullback-Leibler divergence) between the n class Gaussians
 * N(mu_c, Sigma_c): with P_c = Sigma_c^-1 and delta = mu_i - mu_j,
 *     J_ij = KL(i||j) + KL(j||i) = -1/2 <P_i - P_j, Sigma_i - Sigma_j> + 1/2 delta^T (P_i + P_j) delta
 *     sqrt_mode 0   D_ij = J_ij
 *     sqrt_mode 1   D_ij = sqrt(J_ij + eps)
 *     loss = sum_{i>j} w_ij D_ij,  w_ij = uniform_weight, or pair_weights[i*n + j]
 * together with its gradient wrt mu and Sigma.  Stages, all on the caller's stream (jeffreys_kernel.hip): per-class
 * precisions (Cholesky and triangular inverse, double inside; exactly symmetric); ONE pass over the ordered pairs in the
 * explicit-difference form above (the textbook form with two traces cancels the digits that matter for close classes), O(m^2)
 * per pair, every class row with one writer; a per-class finish gcov_i = GSigma_i - P_i sym(GP_i) P_i; a one-workgroup
 * reduction of the per-class partial losses and counters.  No host read-back, no allocation, no float atomics: results are
 * bitwise reproducible and the call may be captured in a HIP graph.
 *   mu (n,m) or NULL (zero means: the divergence of the SPD matrices themselves), cov (n,m,m): row-major, dtype;
 *   n >= 2, 1 <= m <= 64
 *   pair_weights (n,n) dtype, symmetric, or NULL (then uniform_weight).  The pass visits the ordered pairs: row i reads w_ij,
 *   row j reads w_ji, the loss counts j < i with w_ij.  The diagonal is never read into a result.  Every pair is evaluated
 *   and counted in nonfinite_out whatever its weight; dist_out is unweighted.
 *   loss_out (1) dtype or NULL; gmu_out (n,m) and gcov_out (n,m,m, exactly symmetric): both or neither (NULL, NULL = forward
 *   only); with mu == NULL gmu_out must be NULL and gcov_out alone selects the gradient; dist_out (n,n) or NULL: D_ij, both
 *   triangles, the diagonal 0 or sqrt(eps); nonfinite_out (2) int32 or NULL: {#NaN, #inf} among the pairs i > j (a class that
 *   is not positive definite yields NaN and is counted, never a fault)
 *   workspace: sqfa_jeffreys_workspace_bytes(n, m, dtype) bytes (0 = shape or dtype not supported)
 * Returns SQFA_ERR_BAD_ARGUMENT (null cov, n < 2, m < 1, dtype, sqrt_mode outside {0, 1}, gmu_out / gcov_out as above),
 * SQFA_ERR_UNSUPPORTED_M (m > 64), SQFA_ERR_WORKSPACE, checked in that order; every argument check runs before the first
 * HIP call.
 */
size_t sqfa_jeffreys_workspace_bytes(int n, int m, int dtype);
int sqfa_jeffreys_pairwise_loss(const void *mu, const void *cov, int n, int m, int dtype, int sqrt_mode,
                                double eps, const void *pair_weights, double uniform_weight,
                                void *loss_out, void *gmu_out, void *gcov_out, void *dist_out, int *nonfinite_out,
                                void *workspace, size_t workspace_bytes, void *stream);

/*
 * Fused closure loss of the Stein divergence (Jensen-Bregman log-det divergence, S-divergence) between the n SPD matrices
 * S_c:
 *     S_ij = logdet((S_i + S_j)/2) - 1/2 logdet S_i - 1/2 logdet S_j
 *     sqrt_mode 0   D_ij = S_ij
 *     sqrt_mode 1   D_ij = sqrt(|S_ij| + eps)
 *     loss = sum_{i>j} w_ij D_ij,  w_ij = uniform_weight, or pair_weights[i*n + j]
 * together with its gradient  gradS_i = sum_{j != i} c_ij 1/2 (Sbar_ij^-1 - S_i^-1),  Sbar_ij = (S_i + S_j)/2,  c_ij = w_ij
 * (sqrt_mode 0) or w_ij sign(S_ij) / (2 sqrt(|S_ij| + eps)) (sqrt_mode 1).  Stages, all on the caller's stream
 * (stein_kernel.hip): per-class Cholesky (double inside) for logdet S_c and S_c^-1; ONE pass over the ordered pairs that
 * factors Sbar_ij in registers, one lane group per pair, every class row with one writer; a per-class finish; a
 * one-workgroup reduction of the per-class partial losses and counters.  No host read-back, no allocation, no float
 * atomics: results are bitwise reproducible and the call may be captured in a HIP graph.
 *   S (n,m,m): row-major, dtype, symmetric; n >= 2, 1 <= m <= 64
 *   pair_weights (n,n) dtype, symmetric, or NULL (then uniform_weight).  The pass visits the ordered pairs: row i reads w_ij,
 *   row j reads w_ji, the loss counts j < i with w_ij.  The diagonal is never read into a result.  Every pair is evaluated
 *   and counted in nonfinite_out whatever its weight; dist_out is unweighted.
 *   loss_out (1) dtype or NULL; gradS_out (n,m,m, exactly symmetric) or NULL (forward only); dist_out (n,n) or NULL: D_ij,
 *   both triangles, the diagonal 0 or sqrt(eps); nonfinite_out (2) int32 or NULL: {#NaN, #inf} among the pairs i > j (a
 *   class with a pivot that is not positive yields NaN for its pairs and is counted, never a fault)
 *   workspace: sqfa_stein_workspace_bytes(n, m, dtype) bytes (0 = shape or dtype not supported)
 * Returns SQFA_ERR_BAD_ARGUMENT (null S, n < 2, m < 1, dtype, sqrt_mode outside {0, 1}), SQFA_ERR_UNSUPPORTED_M (m > 64),
 * SQFA_ERR_WORKSPACE, checked in that order; every argument check runs before the first HIP call.
 */
size_t sqfa_stein_workspace_bytes(int n, int m, int dtype);
int sqfa_stein_pairwise_loss(const void *S, int n, int m, int dtype, int sqrt_mode,
                             double eps, const void *pair_weights, double uniform_weight,
                             void *loss_out, void *gradS_out, void *dist_out, int *nonfinite_out,
                             void *workspace, size_t workspace_bytes, void *stream);

/*
 * Gaussian class scores: quadratic discriminant analysis in feature space.  For features z_n (K), class means mu_c, class
 * covariances Sigma_c = L_c L_c^T and priors pi_c
 *     score[n][c] = -1/2 |L_c^-1 (z_n - mu_c)|^2 - sum_k log (L_c)_kk - K/2 log 2 pi + log pi_c  =  log p(z_n, c),
 * evaluated in this whitened-difference form (gauss_scores_kernel.hip).  Two entries, both on the caller's stream, nothing
 * allocated, synchronised or read back, no float atomics (bitwise reproducible), usable inside a HIP graph:
 *
 * sqfa_gauss_class_factors -- once per classifier; one workgroup per class, Cholesky in double in LDS.
 *   means (C,K) dtype or NULL (zero-mean classes); cov (C,K,K) dtype, symmetric (the lower triangle is read);
 *   log_priors (C) FLOAT64 or NULL (uniform: -log C); -inf is a class that never wins
 *   W_out (C,K,K) dtype: W_c = L_c^-1, lower triangular, exact zeros above the diagonal
 *   offset_out (C) FLOAT64: -sum_k log (L_c)_kk - K/2 log 2 pi + log pi_c
 *   bad_out (1) int32: the number of classes with a pivot that is not positive and finite, a mean that is not finite, or a
 *   log prior that is NaN or +inf (their W and offset are NaN).  The call sets it: the caller reads it once.
 *
 * sqfa_gauss_scores -- once per batch of samples.  A workgroup owns 64 samples and a range of classes; per class
 *   y = W_c (Z_tile - mu_c) on the exact MFMA (16x16x4), the blocks of W_c above the diagonal skipped, rows of y squared and
 *   summed, the offset added.  The running (max, index) and (max, sum exp) of every sample are carried in registers across
 *   the classes and, where the classes are split over workgroups, merged in the order of the splits by a second launch.
 *   Z (N,K) dtype; means (C,K) or NULL (no subtraction); W, offset as written by sqfa_gauss_class_factors
 *   Each output may be NULL (not wanted):
 *   scores_out (N,C) dtype; argmax_out (N) int64 with best_out (N) dtype, the winning score (best_out needs argmax_out);
 *   logsumexp_out (N) dtype: log p(z_n).  With scores_out == NULL nothing of size (N,C) is written anywhere.
 *   Ties go to the lowest class index; a class whose score is -inf never wins against a finite one and adds nothing to the
 *   sum.  A sample whose row holds a NaN gets index -1, NaN in best_out and logsumexp_out, and is counted in
 *   nonfinite_out (1) int32 (never NULL; the call sets it).  argmax_out / best_out / logsumexp_out are the same bits
 *   whether or not scores_out is asked for.
 *   workspace: sqfa_gauss_scores_workspace_bytes(N, C, K, dtype) bytes (0 = shape or dtype not supported): the partial
 *   reductions of at most 16 class splits, 16 bytes (float32) per sample and split; no N C term.
 * 1 <= K <= 64, C >= 1, N >= 1.  Return SQFA_ERR_BAD_ARGUMENT (null input, sizes < 1, dtype, best_out without argmax_out),
 * SQFA_ERR_UNSUPPORTED_M (K > 64, or more than 2^31 - 1 sample tiles), SQFA_ERR_WORKSPACE, checked in that order; every
 * argument check runs before the first HIP call.
 */
size_t sqfa_gauss_scores_workspace_bytes(long long N, int C, int K, int dtype);
int sqfa_gauss_class_factors(const void *means, const void *cov, const double *log_priors, int C, int K, int dtype,
                             void *W_out, double *offset_out, int *bad_out, void *stream);
int sqfa_gauss_scores(const void *Z, long long N, const void *means, const void *W, const double *offset, int C, int K,
                      int dtype, void *scores_out, long long *argmax_out, void *best_out, void *logsumexp_out,
                      int *nonfinite_out, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The log-loss of the Gaussian class scores and its gradients (gauss_log_loss_kernel.hip).  In the notation above, with
 * W_c = L_c^-1, y_nc = W_c (z_n - mu_c), s_nc = -1/2 |y_nc|^2 + offset_c, lse_n = logsumexp_c s_nc and labels y_n in [0, C):
 *     ll_n = s_{n, y_n} - lse_n  (<= 0),     loss = -1/N sum_n ll_n
 *     p_nc = exp(s_nc - lse_n),  r_nc = g (p_nc - [c == y_n]) / N       (g: the upstream scalar)
 *     dloss/dz_n = - sum_c W_c^T (r_nc y_nc),   dloss/dmu_c = W_c^T sum_n r_nc y_nc,
 *     dloss/dSigma_c = 1/2 W_c^T ( sum_n r_nc (y_nc y_nc^T - I) ) W_c   (symmetric)
 * Priors enter through offset_c only and get no gradient; a class with offset -inf has p_nc = 0.  With C = 1 the posterior
 * is 1 by definition: ll_n = 0 and every gradient is 0 exactly.  Both entries run on the caller's stream, allocate,
 * synchronise and read back nothing, use no float atomics (every sum in a fixed order: bitwise reproducible), and choose
 * every grid and split from (N, C, K, dtype) alone.  Nothing of size N C or C N K is formed.
 *
 * sqfa_gauss_log_loss -- the scores pass (log-sum-exp only), a label pass (one sample per lane, y = W_y (z - mu_y) in
 *   double) and a one-workgroup reduction.
 *   Z (N,K) dtype; labels (N) int64; means (C,K) or NULL; W (C,K,K) and offset (C) FLOAT64 as written by
 *   sqfa_gauss_class_factors
 *   loss_out (1) dtype: the sum over the samples is accumulated in double; NaN when any flag is non-zero
 *   label_log_proba_out (N) dtype or NULL: ll_n (NaN for a flagged sample)
 *   logsumexp_out (N) dtype, required: the backward reads it
 *   flags_out (3) int32 (the call sets them): samples whose score row holds a NaN, labels outside [0, C), labels whose
 *   class has offset -inf.  Labels are data: a label is range-checked before anything is addressed with it, an out-of-range
 *   label is counted and its gathers go to class 0.
 *   workspace: sqfa_gauss_log_loss_workspace_bytes(N, C, K, dtype) bytes: that of the scores pass and 8 bytes per 64 samples.
 *
 * sqfa_gauss_log_loss_backward -- the same inputs, logsumexp (N) as written by the forward call and upstream (1) dtype ON
 *   THE DEVICE, or NULL for 1.  Each of gradZ_out (N,K), grad_means_out (C,K), grad_cov_out (C,K,K) may be NULL (at least
 *   one is not; grad_means_out needs means); the outputs are the same bits whichever subset is asked for, and grad_cov_out
 *   is exactly symmetric.  The r of the labelled class is formed as -g P_n / N with P_n = sum_{c != y_n} p_nc, never as p - 1
 *   (which is all rounding where the posterior is nearly 1).  gradZ: a workgroup owns 64 samples and a split of the classes,
 *   recomputes y on the exact MFMA and feeds its accumulators, scaled by r, to the second product W_c^T (r y) as they stand;
 *   class splits are merged in split order, and the labelled class's term is added per sample (its label range-checked first).
 *   This pass runs whichever subset is asked for: it yields P_n.  grad_means / grad_cov: a workgroup owns a class and a split of the samples, y^T = (Z - mu)^T W^T with the
 *   samples on the rows, M_c = sum r y y^T on the MFMA with the samples as the contraction index; the partials
 *   (sample splits, C, K^2 + K + 1) are summed per class in split order, in double, and W_c^T (.) W_c applied.
 *   Samples the forward call flagged are the caller's to refuse: they give NaN or meaningless gradients, never a fault.
 *   workspace: sqfa_gauss_log_loss_backward_workspace_bytes(N, C, K, dtype) bytes, whatever subset is asked for.
 *
 * sqfa_gauss_log_loss_layout -- informational: the class splits (and groups of 4 classes per split) of the sample-owned
 *   pass and the sample splits (and 16-sample tiles per split) of the class-owned pass.
 * 1 <= K <= 64, C >= 1, N >= 1.  Return SQFA_ERR_BAD_ARGUMENT (null input or required output, sizes < 1, dtype, no gradient
 * asked for, grad_means_out without means), SQFA_ERR_UNSUPPORTED_M (K > 64, or more than 2^31 - 1 sample tiles),
 * SQFA_ERR_WORKSPACE, checked in that order; every argument check runs before the first HIP call.  The workspace queries
 * return 0 for an unsupported shape or dtype.
 */
size_t sqfa_gauss_log_loss_workspace_bytes(long long N, int C, int K, int dtype);
size_t sqfa_gauss_log_loss_backward_workspace_bytes(long long N, int C, int K, int dtype);
int sqfa_gauss_log_loss_layout(long long N, int C, int K, int dtype, int *class_splits, int *groups_per_split,
                               int *sample_splits, long long *tiles_per_split);
int sqfa_gauss_log_loss(const void *Z, const long long *labels, long long N, const void *means, const void *W,
                        const double *offset, int C, int K, int dtype, void *loss_out, void *label_log_proba_out,
                        void *logsumexp_out, int *flags_out, void *workspace, size_t workspace_bytes, void *stream);
int sqfa_gauss_log_loss_backward(const void *Z, const long long *labels, long long N, const void *means, const void *W,
                                 const double *offset, int C, int K, int dtype, const void *logsumexp,
                                 const void *upstream, void *gradZ_out, void *grad_means_out, void *grad_cov_out,
                                 void *workspace, size_t workspace_bytes, void *stream);

/*
 * Nested Gaussian class scores (gauss_nested_kernel.hip): the K classifiers that see only the first k = 1 .. K features,
 * from one pass.  The leading k x k block of L_c is the Cholesky factor of the leading block of Sigma_c and the first k
 * entries of y = L_c^-1 (z - mu_c) depend on the first k features only, so
 *     score_k[n][c] = -1/2 sum_{i<k} y_i^2 + offset_k[c],   offset_k[c] = -sum_{i<k} log (L_c)_ii - k/2 log 2 pi + log pi_c
 * is a prefix sum over the rows of the y of sqfa_gauss_scores.  Column k - 1 of every (N,K) output belongs to the classifier
 * on the first k features; column K - 1 is the full classifier (to rounding: the squares are summed in another order than
 * in sqfa_gauss_scores).  All entries run on the caller's stream, allocate, synchronise and read back nothing and use no
 * float atomics: every sum is in a fixed order, the results are bitwise reproducible and do not depend on which outputs
 * are asked for.  Nothing of size (N,C) or (N,C,K) is formed.
 *
 * sqfa_gauss_class_factors_nested -- sqfa_gauss_class_factors with offsets_out (C,K) FLOAT64: offsets_out[c][k-1] =
 *   offset_k[c], the log-pivots accumulated in double in ascending order.  W_out has the bits sqfa_gauss_class_factors
 *   writes; offsets_out[c][K-1] is its offset to rounding (the same terms, which the compiler is free to contract
 *   differently in the two kernels).  A bad class gets NaN in W and in all K offsets and counts once.
 *
 * sqfa_gauss_scores_nested -- the geometry, LDS stage and MFMA product of sqfa_gauss_scores; the inclusive prefix of y^2
 *   over the rows is a scan over the lane's accumulator registers, an exclusive scan across the four lane quarters and a
 *   carry between the 16-row blocks, and every lane carries (max, index) and (max, sum exp) for each of its rows across the
 *   classes.  Where the classes are split over workgroups a second launch merges the (splits, N, K) partials in split order.
 *   Z (N,K) dtype; means (C,K) or NULL; W (C,K,K), offsets (C,K) FLOAT64 as written by sqfa_gauss_class_factors_nested
 *   argmax_out (N,K) int64 or NULL: ties to the lowest class index in every column
 *   logsumexp_out (N,K) dtype or NULL (at least one of the two is asked for; argmax alone evaluates no exp)
 *   A sample is flagged when any of its K prefix rows holds a NaN (a zero of W times a non-finite feature is NaN on the
 *   MFMA, so the early prefixes of such a sample are not kept): all K of its columns are -1 / NaN and it is counted once
 *   in nonfinite_out (1) int32 (never NULL; the call sets it).
 *   workspace: sqfa_gauss_scores_nested_workspace_bytes(N, C, K, dtype) bytes (0 = shape or dtype not supported): K times
 *   that of sqfa_gauss_scores; 16 bytes where the classes are not split.
 *
 * sqfa_gauss_label_scores_nested -- the label pass of the log-loss with prefixes: one sample per lane, y = W_y (z - mu_y)
 *   in double with a running sum of squares, ll_out[n][k-1] = score_k[n][y_n] - logsumexp[n][k-1] (<= 0, 0 with C = 1).
 *   labels (N) int64, range-checked before anything is addressed with them (an out-of-range label gathers class 0);
 *   logsumexp (N,K) as written by sqfa_gauss_scores_nested; ll_out (N,K) dtype, NaN in all K columns for a flagged sample
 *   flags_out (3) int32: [1] labels outside [0, C) and [2] labels whose class has offset -inf are set by the call; [0] is
 *   left alone: hand flags_out to sqfa_gauss_scores_nested as its nonfinite_out first and the three read as those of
 *   sqfa_gauss_log_loss.
 * 1 <= K <= 64, C >= 1, N >= 1.  Return SQFA_ERR_BAD_ARGUMENT (null input or required output, sizes < 1, dtype, no output
 * asked for), SQFA_ERR_UNSUPPORTED_M (K > 64, or more than 2^31 - 1 sample tiles), SQFA_ERR_WORKSPACE, checked in that
 * order; every argument check runs before the first HIP call.
 */
size_t sqfa_gauss_scores_nested_workspace_bytes(long long N, int C, int K, int dtype);
int sqfa_gauss_class_factors_nested(const void *means, const void *cov, const double *log_priors, int C, int K, int dtype,
                                    void *W_out, double *offsets_out, int *bad_out, void *stream);
int sqfa_gauss_scores_nested(const void *Z, long long N, const void *means, const void *W, const double *offsets, int C,
                             int K, int dtype, long long *argmax_out, void *logsumexp_out, int *nonfinite_out,
                             void *workspace, size_t workspace_bytes, void *stream);
int sqfa_gauss_label_scores_nested(const void *Z, const long long *labels, long long N, const void *means, const void *W,
                                   const double *offsets, int C, int K, int dtype, const void *logsumexp, void *ll_out,
                                   int *flags_out, void *stream);

/*
 * The k best classes of every sample and the rank of its labelled class (gauss_topk_kernel.hip), from the scores of
 * sqfa_gauss_scores without the (N,C) matrix.  Both rest on one total order of (score, class): higher score first, equal
 * scores: lower class index first; a -inf score (a class of prior 0) is an ordinary entry that comes after every finite one.
 * Every score is formed by the statements of sqfa_gauss_scores on the same geometry and has the bits that call writes into
 * scores_out, so the results are those of a stable descending sort of that matrix.  Both entries run on the caller's stream,
 * allocate, synchronise and read back nothing, use no float atomics, choose every grid and split from (N, C, K, dtype, k)
 * alone, are bitwise reproducible and do not depend on which optional outputs are asked for.  Nothing of size (N,C) is formed.
 *
 * sqfa_gauss_scores_topk -- the loop of sqfa_gauss_scores with a sorted list of 1, 2, 4 or 8 (the smallest >= k) entries per
 *   lane in place of (max, index); the lane quarters and, in a second launch, the class splits are joined by list merges.
 *   Z (N,K) dtype; means (C,K) or NULL; W (C,K,K), offset (C) FLOAT64 as written by sqfa_gauss_class_factors
 *   index_out (N,k) int64: the k first classes under the order, best first; column 0 is argmax_out of sqfa_gauss_scores
 *   score_out (N,k) dtype or NULL: their scores, non-increasing
 *   A sample whose score row holds a NaN gets index -1 and score NaN in all k columns and is counted once in
 *   nonfinite_out (1) int32 (never NULL; the call sets it).
 *   workspace: sqfa_gauss_scores_topk_workspace_bytes(N, C, K, dtype, k) bytes: the partial lists, (splits <= 16) x N x list
 *   size x (a value and an int32); 16 bytes where the classes are not split.
 *
 * sqfa_gauss_label_rank -- rank_out[n] = the number of classes c != y_n with s_nc > t_n or (s_nc == t_n and c < y_n), where
 *   t_n = s_{n, y_n}: 0 where argmax_out of sqfa_gauss_scores is y_n.  A pre-pass forms t_n with the bits of the scores pass
 *   (one wave takes its 16 samples in turn, stages the labelled class and runs the 16-column product; column j of an MFMA
 *   product depends on column j of its right operand alone), then the loop of sqfa_gauss_scores counts per lane; quarters and
 *   class splits are joined by integer sums.
 *   labels (N) int64, range-checked before anything is addressed with them (an out-of-range label gathers class 0)
 *   rank_out (N) int64: -1 for a label outside [0, C) and for a sample whose score row holds a NaN
 *   label_score_out (N) dtype or NULL: t_n, NaN for a label outside [0, C)
 *   flags_out (2) int32 (the call sets them): samples whose score row holds a NaN, labels outside [0, C)
 *   workspace: sqfa_gauss_label_rank_workspace_bytes(N, C, K, dtype) bytes: 8 N and, where the classes are split,
 *   (splits <= 16) x N int32.
 * 1 <= k <= min(8, C), 1 <= K <= 64, C >= 1, N >= 1.  Return SQFA_ERR_BAD_ARGUMENT (null input or required output, sizes < 1,
 * dtype, k outside [1, min(8, C)]), SQFA_ERR_UNSUPPORTED_M (K > 64, or more than 2^31 - 1 sample tiles), SQFA_ERR_WORKSPACE,
 * checked in that order; every argument check runs before the first HIP call.  The workspace queries return 0 for an
 * unsupported shape, dtype or k.
 */
size_t sqfa_gauss_scores_topk_workspace_bytes(long long N, int C, int K, int dtype, int k);
int sqfa_gauss_scores_topk(const void *Z, long long N, const void *means, const void *W, const double *offset, int C, int K,
                           int dtype, int k, long long *index_out, void *score_out, int *nonfinite_out, void *workspace,
                           size_t workspace_bytes, void *stream);
size_t sqfa_gauss_label_rank_workspace_bytes(long long N, int C, int K, int dtype);
int sqfa_gauss_label_rank(const void *Z, const long long *labels, long long N, const void *means, const void *W,
                          const double *offset, int C, int K, int dtype, long long *rank_out, void *label_score_out,
                          int *flags_out, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Matrix functions of SPD matrices, f(S) = Q f(Lambda) Q^T per class, and their backward -- spd_log and spd_sqrt of the
 * reference (src/sqfa/linalg.py:165-183, 121-141: torch.linalg.eigh + einsum), as used by log_euclidean[_sq]
 * (src/sqfa/distances.py:92-138).  The eigen-decomposition is one-sided Jacobi, run to convergence, on the Cholesky
 * factor of each class (S = L L^T, L V = Q Sigma  =>  lambda = sigma^2 with the relative accuracy log needs), in double
 * whatever the dtype; results are bitwise reproducible.
 *   S (n,m,m) dtype, F_out (n,m,m) dtype or NULL; U_out (n,m,m) and lam_out (n,m): FLOAT64, eigenvectors as columns,
 *   eigenvalues unsorted -- what sqfa_spd_function_backward needs (a non-SPD class yields NaN there and in F_out)
 *   kind: SQFA_SPD_LOG, SQFA_SPD_SQRT, SQFA_SPD_INV_SQRT (the symmetric inverse root)
 *   workspace: sqfa_spd_function_workspace_bytes(n, m, dtype) bytes; m <= 64 (0 bytes / SQFA_ERR_UNSUPPORTED_M above)
 * sqfa_spd_function_backward: gradS_out (n,m,m) dtype = Q [(Q^T sym(G) Q) o Gamma] Q^T for the upstream gradient
 *   G (n,m,m) dtype wrt F (Daleckii-Krein; Gamma = divided differences of f, evaluated in forms that stay finite for
 *   repeated eigenvalues, where torch's eigh backward -- the reference's autograd -- returns inf / NaN).
 */
#define SQFA_SPD_LOG 0
#define SQFA_SPD_SQRT 1
#define SQFA_SPD_INV_SQRT 2
size_t sqfa_spd_function_workspace_bytes(int n, int m, int dtype);
int sqfa_spd_function(const void *S, int n, int m, int dtype, int kind, void *F_out, double *U_out, double *lam_out,
                      void *workspace, size_t workspace_bytes, void *stream);
int sqfa_spd_function_backward(const double *U, const double *lam, const void *G, int n, int m, int dtype, int kind,
                               void *gradS_out, void *stream);

/*
 * The orthogonal filter constraint (constraint="orthogonal" of the reference, src/sqfa/model.py:416-431, which registers
 * torch.nn.utils.parametrizations.orthogonal: torch's _Orthogonal with orthogonal_map="householder" -- the map torch picks
 * for n_filters != n_dim -- and use_trivialization=True), forward and backward, in compact WY form:
 *     V (D,K) = strictly-lower(X^T) + [I_K; 0],  s_i = int(X[i,i]) (the stored +-1 diagonal, not differentiated)
 *     M = striu(V^T V) + diag(|v_i|^2 / 2),  W = M^-1 V_top^T,  P = [I_K; 0] - V W   (= H_1 ... H_K [I_K; 0], orgqr convention)
 *     F = (base (P * s))^T
 * in place of tril -> column norms -> torch.linalg.householder_product -> sign -> base @ Q and their autograd backward.
 * Every K x K quantity (V^T V, M, both triangular solves) is computed in double whatever the dtype; sums over D are
 * per-block partial sums added in a fixed order (no atomics): results are bitwise reproducible.  Nothing is allocated,
 * synchronised or read back: the calls can be captured in a HIP graph on the caller's stream.
 *   X (K,D) raw parameter, base (D,D), F_out / gF / gX_out (K,D): row-major, dtype; 1 <= K <= 64, K < D
 *   gX_out: gradient of sum(F * gF) wrt X, exactly 0 on and above the diagonal of X^T (as torch returns)
 *   workspace: sqfa_orthogonal_workspace_bytes(K, D, dtype) bytes for either call (0 = shape or dtype not supported).
 *   sqfa_orthogonal_backward recomputes M and W from X: it needs X, base, gF and ANY workspace of that size, nothing
 *   of a forward call's workspace.
 * Returns SQFA_ERR_BAD_ARGUMENT (null pointers, K < 1, K >= D, dtype), SQFA_ERR_UNSUPPORTED_M (K > 64),
 * SQFA_ERR_WORKSPACE; every argument check runs before the first HIP call.
 */
size_t sqfa_orthogonal_workspace_bytes(int K, int D, int dtype);
int sqfa_orthogonal_forward(const void *X, const void *base, int K, int D, int dtype,
                            void *F_out, void *workspace, size_t workspace_bytes, void *stream);
int sqfa_orthogonal_backward(const void *X, const void *base, const void *gF, int K, int D, int dtype,
                             void *gX_out, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Class statistics from labelled points -- class_statistics of the reference (src/sqfa/statistics.py:8-124: per class a
 * boolean mask, the mean, the centred X_c^T X_c / (n_c - 1), optional OAS shrinkage, and cov + mu mu^T, inside a Python
 * loop) -- as a segmented, centred SYRK on the exact f32 / f64 MFMA, and the same statistics accumulated over batches.
 *   points (N,D) row-major, dtype; any D >= 1 (16-byte loads where D % (16 / element size) == 0 and the base is
 *   16-byte aligned, one element per load otherwise: same results bit for bit)
 *   row_index (N) int64 or NULL: row k of class c is points[row_index[class_start[c] + k]] -- the indices of a stable
 *   sort of the labels, so no sorted copy of the points is made; NULL = the rows are already grouped by class
 *   class_start (C+1) int64: exclusive cumulative sum of the class sizes, class_start[C] = N.  The sizes are read on
 *   the device only; the launch geometry depends on C and D alone.  N = 0 is valid (every class empty).
 *   means_out (C,D), cov_out (C,D,D), second_out (C,D,D) or NULL: dtype.
 *   estimator  SQFA_COV_EMPIRICAL  cov = sum (x - mu)(x - mu)^T / (n_c - 1), second = cov + mu mu^T from the same registers
 *              SQFA_COV_OAS        the same shrunk towards tr/D I (Chen et al. 2010, rho clamped at 1; statistics.py:57-94)
 *              SQFA_COV_SCATTER    cov_out = the raw centred sum, no division; second_out is not written
 *   An empty class gives NaN means and NaN matrices, a class of one point a finite mean and a NaN covariance (0/0), as
 *   the reference's expressions do.  Rows are centred in the dtype, the means are summed in double.
 * One workgroup per (class, 64 x 64 tile of the lower block triangle); an off-diagonal tile is stored as computed and
 * transposed, so every (D,D) output is EXACTLY symmetric.  No split over rows, no atomics, every sum in a fixed order:
 * results are bitwise reproducible.  Nothing is allocated, synchronised or read back; capturable in a HIP graph.
 *   workspace: sqfa_class_moments_workspace_bytes(C, D, dtype) bytes for any of the three calls (0 = not supported:
 *   dtype, C < 1, D < 1, C > 65535, or more than 2^31 - 1 (class, tile) workgroups).
 *
 * sqfa_class_moments_update: the batched merge of Chan, Golub and LeVeque.  counts (C) FLOAT64, means (C,D) and
 *   m2 (C,D,D) dtype are the running state, read and written (start from zeros).  With mu_b, M2_b the mean and centred
 *   sum of the batch's rows of a class (computed as above), delta = mu_b - means and n = counts + n_b:
 *       m2 += M2_b + (counts n_b / n) delta delta^T;   means += delta n_b / n;   counts = n
 *   (counts = 0: means = mu_b, m2 += M2_b).  A class with no row in the batch is left untouched, bit for bit.  No raw
 *   second moments are formed anywhere (sum x x^T - n mu mu^T cancels in float32).  m2 stays exactly symmetric.
 * sqfa_class_moments_finalize: statistics from such a state: cov_out = m2 / (counts - 1) (SQFA_COV_EMPIRICAL) or its OAS
 *   shrinkage (SQFA_COV_OAS), second_out (or NULL) = cov + means means^T; counts < 1 gives NaN matrices.
 * sqfa_class_shrinkage: the OAS coefficients alone, measured from the points with NOTHING of size (D,D) written: the
 *   SYRK of sqfa_class_moments(SQFA_COV_OAS) in a measuring mode (same grid, chunk walk, MFMA, s = v / (n_c - 1) rounded
 *   to the dtype, per-tile tr S and sum S o S in double) and a finish kernel that sums the partials in the same order and
 *   forms rho by the same expression.  means (C,D) in: sqfa_class_means.  keep_out (C) = (T)(1 - rho_c) and shift_out (C)
 *   = (T)(rho_c tr S_c / D), dtype: the very bits SQFA_COV_OAS applies, OAS(S_c) = keep_c S_c + shift_c I.  rho_out (C)
 *   FLOAT64 or NULL.  A class below two points gets NaN in all three.  Workspace as above (the partials are all it uses).
 * Return SQFA_ERR_BAD_ARGUMENT (null pointers -- points may be NULL only when N = 0 --, N < 0, C < 1, D < 1, dtype,
 * estimator), SQFA_ERR_UNSUPPORTED_M (the grid limits above), SQFA_ERR_WORKSPACE; every check runs before the first HIP call.
 */
#define SQFA_COV_EMPIRICAL 0
#define SQFA_COV_OAS       1
#define SQFA_COV_SCATTER   2
size_t sqfa_class_moments_workspace_bytes(int C, int D, int dtype);
int sqfa_class_moments(const void *points, long long N, int D, const long long *row_index,
                       const long long *class_start, int C, int dtype, int estimator,
                       void *means_out, void *cov_out, void *second_out,
                       void *workspace, size_t workspace_bytes, void *stream);
int sqfa_class_moments_update(const void *points, long long N, int D, const long long *row_index,
                              const long long *class_start, int C, int dtype,
                              double *counts, void *means, void *m2,
                              void *workspace, size_t workspace_bytes, void *stream);
int sqfa_class_moments_finalize(const double *counts, const void *means, const void *m2, int C, int D, int dtype,
                                int estimator, void *cov_out, void *second_out,
                                void *workspace, size_t workspace_bytes, void *stream);
int sqfa_class_shrinkage(const void *points, long long N, int D, const long long *row_index,
                         const long long *class_start, int C, int dtype, const void *means,
                         void *keep_out, void *shift_out, double *rho_out,
                         void *workspace, size_t workspace_bytes, void *stream);

/*
 * Feature moments from labelled points, with nothing of size (C,D,D): per closure evaluation they replace the class
 * statistics of the reference (src/sqfa/statistics.py:8-124) followed by transform_scatters (src/sqfa/model.py:172-188,
 * conjugate_matrix src/sqfa/linalg.py:19-45), through  F cov_c F^T = cov(F x | c)  and  F mu_c = mean(F x | c)
 * (empirical estimator).  points, row_index, class_start as for sqfa_class_moments; any D >= 1 (16-byte loads where
 * D % (16 / element size) == 0 and points, means and F are 16-byte aligned, one element per load otherwise: the same bits).
 *   sqfa_class_means   means_out (C,D) alone: the kernel sqfa_class_moments runs (sums in double), the same bits as its
 *                      means_out; an empty class gives NaN.  C <= 65535 (SQFA_ERR_UNSUPPORTED_M).
 *   row_class (N) int64: the class of GROUPED row g, i.e. the sorted labels (labels[row_index]); values in 0..C-1.
 *   sqfa_class_feature_moments   F (K,D), K <= 64.  Outputs, all in the dtype:
 *       zc_out (N,K)       F (x - mu_class), the row centred in D-space in the dtype BEFORE the product, in GROUPED order
 *                          (row g belongs to points[row_index[g]]); kept by the caller for the backward call
 *       means_f_out (C,K)  F mu_c
 *       cov_f_out (C,K,K)  sum_{i in c} zc_i zc_i^T / (n_c - 1), plus `noise` on the diagonal
 *       second_f_out (C,K,K) or NULL   cov_f_out + means_f means_f^T
 *     Both matrices equal their transposes bit for bit.  An empty class gives NaN means and matrices, a class of one point
 *     a finite mean and NaN matrices, as sqfa_class_moments.
 *   sqfa_class_feature_moments_backward   G (C, ldg, ldg block, top-left K x K used, row pitch ldg; NOT assumed symmetric)
 *     = dL/dcov_f, g_means (C,K) or NULL = dL/dmeans_f (a caller that used second_f folds its gradient G2 in first:
 *     G += G2, g_means += (G2 + G2^T) means_f).  With w_i = (G_c + G_c^T) zc_i / (n_c - 1):
 *         dL/dF = sum_i w_i (x_i - mu_class)^T + sum_c g_c mu_c^T = sum_p partial_out[p]
 *     partial_out (n_groups,K,D), 1 <= n_groups <= 65535: the layout sqfa_feature_scatters_backward writes and
 *     sqfa_sphere_backward sums.  The mean term IS folded in here (its rows are shared out over the groups like the
 *     points); the sum over the groups is left to the caller.  Classes with n_c < 2 contribute nothing through G, empty
 *     classes nothing through g_means (NaN entries of G, g_means or means there are never read into the result).
 *   workspace: sqfa_class_feature_moments_workspace_bytes(N, C, D, K, dtype) bytes for either call (0 = not supported:
 *   dtype, N < 0, C < 1, D < 1, K < 1, K > 64, C > 65535, or a grid beyond 2^31 - 1 workgroups).
 * Class sizes are read on the device only; every grid is a function of (N, C, D, K, n_groups); no atomics, every sum in
 * a fixed order (bitwise reproducible); nothing is allocated, synchronised or read back; capturable in a HIP graph.
 * Return SQFA_ERR_BAD_ARGUMENT (null pointers -- points, row_class and zc may be NULL only when N = 0 --, N < 0, C < 1,
 * D < 1, K < 1, dtype, ldg < K, n_groups), SQFA_ERR_UNSUPPORTED_M (K > 64 and the limits above), SQFA_ERR_WORKSPACE, in
 * this order; every check runs before the first HIP call.
 *
 * The shrunk entries: the same moments of OAS-shrunk class covariances, OAS(S_c) = keep_c S_c + shift_c I with keep, shift
 * (C) in the dtype from sqfa_class_shrinkage, through  F OAS(S_c) F^T = keep_c F S_c F^T + shift_c F F^T:
 *   sqfa_class_feature_moments_shrunk   cov_f_out = keep_c sum zc_i zc_i^T / (n_c - 1) + shift_c F F^T + noise I; F F^T (K,K)
 *     is formed once per call (one launch more), every element in one fixed order, so both matrices stay exactly symmetric.
 *     Same NaN pattern (keep and shift of a class below two points are NaN already).
 *   sqfa_class_feature_moments_shrunk_backward   takes F (K,D) as well:
 *         dL/dF = sum_i keep_c w_i (x_i - mu_class)^T + H F + sum_c g_c mu_c^T,   H = sum_{c: n_c >= 2} shift_c (G_c + G_c^T)
 *     H F through K more virtual rows (the filters, weighted by the columns of H), H by one launch more, the classes
 *     summed in a fixed order and those with n_c < 2 left out by select: NaN in their G, keep and shift never reaches the
 *     result.  A class with n_c >= 2 and NaN coefficients (zero variance, D = 1) gives NaN, as the dense statistics do.
 *   workspace: sqfa_class_feature_moments_shrunk_workspace_bytes (the query above plus K more weight rows and one (K,K)
 *   block; 0 where that one is 0).  Checks, return codes and their order as above; keep and shift must not be NULL.
 */
int sqfa_class_means(const void *points, long long N, int D, const long long *row_index,
                     const long long *class_start, int C, int dtype, void *means_out, void *stream);
size_t sqfa_class_feature_moments_workspace_bytes(long long N, int C, int D, int K, int dtype);
int sqfa_class_feature_moments(const void *points, long long N, int D, const long long *row_index,
                               const long long *row_class, const long long *class_start, int C,
                               const void *means, const void *F, int K, int dtype, double noise,
                               void *zc_out, void *means_f_out, void *cov_f_out, void *second_f_out,
                               void *workspace, size_t workspace_bytes, void *stream);
int sqfa_class_feature_moments_backward(const void *points, long long N, int D, const long long *row_index,
                                        const long long *row_class, const long long *class_start, int C,
                                        const void *means, const void *zc, const void *G, int ldg,
                                        const void *g_means, int K, int dtype, int n_groups, void *partial_out,
                                        void *workspace, size_t workspace_bytes, void *stream);
size_t sqfa_class_feature_moments_shrunk_workspace_bytes(long long N, int C, int D, int K, int dtype);
int sqfa_class_feature_moments_shrunk(const void *points, long long N, int D, const long long *row_index,
                                      const long long *row_class, const long long *class_start, int C,
                                      const void *means, const void *F, int K, int dtype, double noise,
                                      const void *keep, const void *shift,
                                      void *zc_out, void *means_f_out, void *cov_f_out, void *second_f_out,
                                      void *workspace, size_t workspace_bytes, void *stream);
int sqfa_class_feature_moments_shrunk_backward(const void *points, long long N, int D, const long long *row_index,
                                               const long long *row_class, const long long *class_start, int C,
                                               const void *means, const void *F, const void *zc, const void *G, int ldg,
                                               const void *g_means, const void *keep, const void *shift,
                                               int K, int dtype, int n_groups, void *partial_out,
                                               void *workspace, size_t workspace_bytes, void *stream);

/* Introspection (benchmarks / development; not needed by a reference-side binding).
 *
 * sqfa_airm_profile(1): every following sqfa_airm_pairwise call brackets its pair tile kernel
 *   with hipEvents recorded on the caller's stream.  sqfa_airm_profile_read synchronises on
 *   those events, returns the summed kernel time [ms] and the number of launches, and
 *   releases them (call it outside any timed region).  The switch is an atomic flag; it changes what is
 *   RECORDED around a launch, never which kernel runs. */
int sqfa_airm_profile(int enable);
int sqfa_airm_profile_read(double *tile_kernel_ms_total, int *launches);
int sqfa_project_profile_read(double *kernel_ms_total, int *launches);  /* same, for sqfa_project_scatters */

#ifdef __cplusplus
}
#endif
#endif /* SQFA_HIP_H */
