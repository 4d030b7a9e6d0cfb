/*
 * kfac_hip.h — C ABI of the MI355X (gfx950) KFAC curvature engine.
 *
 * Plain pointers and sizes only (no torch types): every buffer is device memory
 * owned by the caller, every call is asynchronous on the given HIP stream
 * (passed as an opaque `void*` = hipStream_t) and does no implicit sync, no
 * allocation and no host<->device copy of data, so calls can be captured into a
 * HIP graph.  Return value: 0 = launched, <0 = bad argument / launch failure
 * (kfac_strerror).  Numerical failure (a non-positive pivot) is reported in a
 * DEVICE int array `info`, LAPACK style, for the caller to read when it syncs.
 *
 * Each entry point names the reference interface it replaces
 * (paths under TianmingQiu/BNN_KFAC).  The Python binding (ctypes) lives in
 * bnn_kfac_amd/_native.py; INTEGRATION.md shows the binding a maintainer of the
 * reference would add.
 */
#ifndef KFAC_HIP_H
#define KFAC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__) || defined(__clang__)
#define KFAC_API __attribute__((visibility("default")))
#else
#define KFAC_API
#endif

typedef void* kfac_stream_t; /* hipStream_t */

enum kfac_status {
  KFAC_OK = 0,
  KFAC_EINVAL = -1,     /* bad argument (null pointer, bad shape, bad layout) */
  KFAC_ELAUNCH = -2,    /* a HIP launch failed */
  KFAC_EWORKSPACE = -3, /* workspace too small */
};

/* ------------------------------------------------------------------ factors
 * F = beta * F + alpha * X~^T X~, X~ = [X | 1] (ones column iff has_ones),
 * X the (rows x cols) input whose element (k, i) is addressed per `layout`:
 *   KFAC_ROWMAJOR: ptr[k*ld + i]                     (Linear a, Linear g_rec)
 *   KFAC_CHANNEL : ptr[(k/L)*sB + (k%L) + i*L]        (Conv2d g_rec (B,C,Ho*Wo))
 *   KFAC_PATCH   : implicit im2col of x (B,C,H,W):   k = b*L + oh*Wo + ow,
 *                  i = c*kh*kw + ki*kw + kj  ->  x[b, c, oh*sh+ki-ph, ow*sw+kj-pw]
 *                  (0 outside the image)           (Conv2d a, F.unfold order)
 * F is n x n row-major with n = cols + has_ones, written exactly symmetric.
 * Replaces models/curvatures.py:341-363 (unfold/permute + the two torch.mm
 * calls + the per-batch-mean `/ float(cols)` + the `+=` accumulation).     */
enum kfac_layout { KFAC_ROWMAJOR = 0, KFAC_CHANNEL = 1, KFAC_PATCH = 2 };

typedef struct kfac_operand {
  const float* ptr;
  int32_t layout;
  int32_t cols;
  int64_t rows;
  int32_t has_ones;
  /* Multi-batch ROWMAJOR job (nseg > 1): rows of its LAST batch when that batch is
   * shorter than `rows` (a pass's ragged last batch), 0 = every batch has `rows`.
   * That batch enters with its own per-batch mean, alpha * rows / last_rows (the
   * reference's `/ forward.shape[1]` per update, curvatures.py:349,356); the other
   * batches with alpha.                                                       */
  int32_t last_rows;
  int64_t ld;  /* ROWMAJOR row stride (elements) */
  int64_t L;   /* CHANNEL/PATCH: positions per sample (Ho*Wo) */
  int64_t sB;  /* CHANNEL/PATCH: sample stride (elements) */
  int32_t C, H, W, kh, kw, sh, sw, ph, pw, Ho, Wo, reserved1; /* PATCH geometry */
} kfac_operand;

typedef struct kfac_factor_job {
  kfac_operand x;
  float alpha; /* 1/cols = per-batch mean (curvatures.py:349,356); 1/B_global when sharded */
  float beta;  /* 0 = first update assigns, 1 = later updates add (curvatures.py:359-363) */
  float* F;
  int64_t ldF;
  /* Optional deferred reduction (NULL = reduce into F in this call).  With `acc`
   * set, kfac_factor_update leaves F alone and keeps this factor's split-K partial
   * tiles in the caller's accumulator instead:  acc = acc_beta*acc + alpha*partial
   * (acc_beta 0 on the first update after a flush, 1 after).  kfac_factor_flush
   * then writes F = beta*F + alpha*sum(acc) once, e.g. at the end of a data pass,
   * so a pass of U updates runs U MFMA launches + 1 reduce instead of U + U.
   * acc_splits and the size come from kfac_factor_accum_plan; F = sum of the
   * partials either way (floating-point summation order differs).            */
  float* acc;
  int32_t acc_splits;
  float acc_beta;
  /* Optional multi-batch job (nseg > 1): the update covers nseg batches of x's
   * shape at once, F += alpha * sum_s X_s~^T X_s~, X_s the operand x with
   * ptr = seg_ptrs[s].  seg_ptrs is a HOST array of nseg device pointers, read
   * during the call and passed to the kernel as launch arguments (no copy, no
   * device table; graph-capturable); every base must share x.ptr's alignment
   * modulo 16 bytes.  One launch then walks K across the batches in place
   * (K = nseg * x.rows, up to 64 bases per launch, more run as back-to-back
   * launches), so a pass of U equal batches costs about one MFMA launch instead
   * of U.  Equivalent to nseg jobs with the same alpha (the reference's per-batch
   * mean over equal batches).  nseg 0 or 1 = the single batch at x.ptr.  Every
   * layout: a KFAC_PATCH / KFAC_CHANNEL job's images are the nseg batches' B
   * images each, in order (one launch per conv factor for the queued batches when
   * an image fits the LDS-staged kernel; else one launch per batch).           */
  const void* seg_ptrs;
  int32_t nseg;
  /* Deferred reduction, several jobs of one factor in ONE call (e.g. a pass's full
   * batches as one multi-batch job and its short last batch as another): slabs per
   * tile of the accumulator `acc` points into, 0 = acc_splits.  Each job owns its
   * own slab range [s0, s0 + acc_splits) of an accumulator of acc_stride slabs per
   * tile and passes acc = base + s0 * 64*64*sizeof(float) bytes (ranges must not
   * overlap); kfac_factor_flush then takes acc = base, acc_splits = acc_stride =
   * the total.  kfac_factor_accum_plan's bytes are linear in the splits, so the
   * accumulator of such a factor is the sum of its jobs' planned bytes.          */
  int32_t acc_stride;
} kfac_factor_job;

/* Workspace (split-K slabs) needed by kfac_factor_update for these jobs. */
KFAC_API size_t kfac_factor_workspace_bytes(const kfac_factor_job* jobs, int njobs);
/* All jobs of one KFAC.update() in one grouped MFMA launch + one reduce launch.
 * Replaces KFAC.update, models/curvatures.py:325-365. */
KFAC_API int kfac_factor_update(const kfac_factor_job* jobs, int njobs, void* workspace,
                       size_t workspace_bytes, kfac_stream_t stream);

/* Accumulator layout for these jobs (acc ignored): splits[j] and bytes[j] of job
 * j's deferred-reduction accumulator, planned for this batch shape (later
 * batches of any row count may use it).                                    */
KFAC_API int kfac_factor_accum_plan(const kfac_factor_job* jobs, int njobs, int32_t* splits,
                           size_t* bytes);
/* Which kernel family these jobs would run on, for inspection; no GPU needed and no
 * device call made.  family[j] = the kfac_prof_id (below) of the family job j's launch
 * group gets from the grouping and the router kfac_factor_update uses (row-major jobs
 * share groups of up to 16, every conv job is a group of its own), after
 * kfac_factor_accum_plan's validation (KFAC_EINVAL; a NULL `family` too).  It reports
 * the FIRST routing of the group: a multi-batch conv job off the image-staged kernels
 * answers KFAC_PROF_FACTOR_TILES and runs there, one launch per batch; a group
 * kfac_factor_update splits (a ragged last batch, more than 64 batch bases) is routed
 * again per piece.                                                            */
KFAC_API int kfac_factor_route(const kfac_factor_job* jobs, int njobs, int32_t* family);
/* F = beta*F + alpha*sum(acc) for every job (all must carry acc): the reduce
 * step of kfac_factor_update, deferred (x is only read for the factor size). */
KFAC_API int kfac_factor_flush(const kfac_factor_job* jobs, int njobs, kfac_stream_t stream);

/* kfac_factor_tiles_x3's work units of a factor of P 32-column panels (2 <= P <= 64), for
 * inspection; no GPU needed.  Unit i in out[6 i .. 6 i + 5]: its up to four panels
 * a < b < c < d (-1: none), the 6-bit mask of the panel pairs (32 x 32 blocks) it owns --
 * bit 0 (b, a), 1 (c, a), 2 (d, a), 3 (c, b), 4 (d, b), 5 (d, c) -- and the 4-bit mask of the
 * panels whose diagonal block it owns.  Fills at most cap units; returns the number of
 * units of the table (0: P out of range).                                           */
KFAC_API int kfac_x3_unit_table(int P, int32_t* out, int cap);
/* The task workgroup `block` of a kfac_factor_tiles_x3 launch computes when every one of
 * its njobs jobs has `splits` K-splits, for inspection; no GPU needed.  units[j] = units of
 * job j (kfac_x3_unit_table's count; 1 for a factor of n <= 32); `blocks` = splits x the sum
 * of units[], the launch's workgroups.  xcd_job_unit_split[0..3] = the XCD the workgroup is
 * dispatched to (block % 8), the job, the job's unit and the K-split, exactly as the kernel
 * decodes them: split-major across the launch, every XCD a contiguous range of that order.
 * KFAC_EINVAL: null pointers, njobs outside 1..16, a count below 1, blocks not splits x
 * the units, block outside 0..blocks-1.                                              */
KFAC_API int kfac_x3_task_decode(const int32_t* units, int njobs, int splits, int blocks, int block,
                        int32_t* xcd_job_unit_split);

/* Single-factor conveniences (same kernels). */
KFAC_API int kfac_syrk_linear(const float* x, int64_t B, int64_t d, int64_t ldx, int has_ones,
                     float alpha, float beta, float* F, int64_t ldF, void* workspace,
                     size_t workspace_bytes, kfac_stream_t stream);
KFAC_API int kfac_syrk_conv(const float* x, int64_t B, int C, int H, int W, int kh, int kw, int sh,
                   int sw, int ph, int pw, int has_ones, float alpha, float beta, float* F,
                   int64_t ldF, void* workspace, size_t workspace_bytes, kfac_stream_t stream);
KFAC_API int kfac_syrk_convgrad(const float* g, int64_t B, int C, int64_t L, float alpha, float beta,
                       float* F, int64_t ldF, void* workspace, size_t workspace_bytes,
                       kfac_stream_t stream);

/* ---------------------------------------------------------------- inversion
 * R = scale * (F + F^T)/2 + shift * I, computed in fp64 on the device, then
 *   KFAC_OUT_INV_CHOL: out = L, lower, L L^T = R^{-1}   (= cholesky(inverse(R)))
 *   KFAC_OUT_INVERSE : out = R^{-1} (full, symmetric)
 * via C = chol(P R P) (P the exchange matrix), X = C^{-1}, L = P X^T P.
 * KFAC.invert passes scale = sqrt(multiply), shift = sqrt(add)
 * (models/curvatures.py:367-398); the regression block passes scale = N,
 * shift = N*tau with KFAC_OUT_INVERSE (regression_ll_block.py:130-133).
 * info[j] (device) = 0, or the 1-based index of the first non-positive pivot
 * of job j (the reference's RuntimeError / LinAlgError condition).  Pivots are
 * counted in the elimination's own order, that of the flipped matrix P R P:
 * pivot p belongs to row n - p + 1 of F, counted from 1 (a NaN pivot counts as
 * non-positive).  Every call writes every info[j], 0 included; a failed job's
 * `out` is unspecified, the other jobs of the call are not affected.
 * `out` must not alias F (nor any other job's F): the launch that reads F
 * already writes the zero blocks of `out`.                                    */
enum kfac_inv_out { KFAC_OUT_INV_CHOL = 0, KFAC_OUT_INVERSE = 1 };

typedef struct kfac_invert_job {
  const float* F;
  int64_t ldF;
  int32_t n;
  int32_t out_kind;
  double scale;
  double shift;
  float* out;
  int64_t ldo;
} kfac_invert_job;

KFAC_API size_t kfac_invert_workspace_bytes(const kfac_invert_job* jobs, int njobs);
KFAC_API int kfac_invert(const kfac_invert_job* jobs, int njobs, void* workspace, size_t workspace_bytes,
                int32_t* info, kfac_stream_t stream);
/* kfac_invert that also signals when the inputs are consumed: `inputs_read` (a
 * hipEvent_t, may be NULL) is recorded on `stream` right after the launches that
 * read the F factors (the first of each job group: R' is built from F there), so
 * the caller may overwrite F (e.g. accumulate the next data pass) once the event
 * completes while the rest of the inversion still runs.  Same results as
 * kfac_invert.                                                               */
KFAC_API int kfac_invert_ex(const kfac_invert_job* jobs, int njobs, void* workspace,
                   size_t workspace_bytes, int32_t* info, void* inputs_read, kfac_stream_t stream);
/* Single-factor convenience: KFAC.invert for one factor. */
KFAC_API int kfac_damped_inv_chol(const float* F, int n, int64_t ldF, double sqrt_s, double sqrt_n,
                         float* L, int64_t ldL, void* workspace, size_t workspace_bytes,
                         int32_t* info, kfac_stream_t stream);

/* ------------------------------------------------------------ eigenvalues
 * Symmetric eigendecomposition of (F + F^T)/2 (fp64 on device): evals ascending
 * (torch.symeig / eigvalsh order), evecs (optional, may be NULL) as columns,
 * row-major n x n fp32.  Replaces models/utilities.py:120-159.           */
typedef struct kfac_eig_job {
  const float* F;
  int64_t ldF;
  int32_t n;
  int32_t reserved;
  double* evals;
  float* evecs;
  int64_t ldv;
} kfac_eig_job;

KFAC_API size_t kfac_eig_workspace_bytes(const kfac_eig_job* jobs, int njobs);
KFAC_API int kfac_syev(const kfac_eig_job* jobs, int njobs, void* workspace, size_t workspace_bytes,
              int32_t* info, kfac_stream_t stream);

/* ------------------------------------------------- predictive variance
 * v[j][b] = J_jb kron(K1_j, K2_j) J_jb^T without forming the Kronecker product:
 * with M = J_jb viewed (nA x nG) row-major (the reference's flat order
 * a*nG + g), v = <K1^T M, M K2^T>_F.  K1/K2 may be flagged lower-triangular
 * (Cholesky factors) to skip their zero blocks: a flagged factor must hold zeros
 * in its upper triangle, since only the tiles strictly above the diagonal tiles
 * are skipped and the diagonal tiles are read in full.
 * out[b] = sum_j |v[j][b]| if abs_sum else sum_j v[j][b].
 * Replaces classification_ll_block.py:126-132 (torch.kron + J H J^T) and
 * regression_ll_block.py:128-139 (kronecker_product + J H J^T).          */
typedef struct kfac_quad_job {
  const float* J;
  int64_t ldJ; /* stride between the nb rows of J (elements) */
  int32_t nA, nG;
  const float* K1;
  int64_t ld1;
  const float* K2;
  int64_t ld2;
  int32_t lower1, lower2;
  float* v; /* optional (may be NULL): nb raw values for this job */
} kfac_quad_job;

KFAC_API size_t kfac_quadform_workspace_bytes(const kfac_quad_job* jobs, int njobs, int64_t nb);
KFAC_API int kfac_kron_quadform(const kfac_quad_job* jobs, int njobs, int64_t nb, int abs_sum, float* out,
                       void* workspace, size_t workspace_bytes, kfac_stream_t stream);

/* ------------------------------------------------- GLM predictive covariance
 * The full output covariance of the linearised (GLM) predictive under the posterior
 * kfac_sample draws from: vec(S) (S = K1 z K2^T, index a*nG + g) has covariance
 * K1 K1^T (x) K2 K2^T, so with M_r = Jacobian row r = b*nc + c (sample b, output c)
 * viewed (nA x nG) row-major,
 *   cov[b][c][c'] = sum_j < K1_j^T M_{b,c} K2_j , K1_j^T M_{b,c'} K2_j >_F
 * without forming the Kronecker product.  M is in the POSTERIOR's order
 * (M[a][g] = dW[g][a], M[nA-1][g] = db[g]), not kfac_quad_job's reference order.
 * cov is nb x nc x nc, each block bitwise symmetric; partial sums are reduced in a
 * fixed order in fp64 (no atomics): two calls give identical bits, and a sample's block
 * depends on that sample's rows only.  accumulate: cov += the sum, else cov = it.
 * At most 8 jobs and nc <= 32 per call.                                        */
typedef struct kfac_cov_job {
  const float* J; /* row r = b*nc + c at J + r*ldJ: nA*nG elements, index a*nG + g */
  int64_t ldJ;
  int32_t nA, nG;
  const float* K1;
  int64_t ld1;
  const float* K2;
  int64_t ld2;
  int32_t lower1, lower2; /* K1 / K2 lower-triangular: their zero K-range is skipped */
} kfac_cov_job;

KFAC_API size_t kfac_kron_cov_workspace_bytes(const kfac_cov_job* jobs, int njobs, int64_t nb, int nc);
KFAC_API int kfac_kron_cov(const kfac_cov_job* jobs, int njobs, int64_t nb, int nc, int accumulate,
                  float* cov, void* workspace, size_t workspace_bytes, kfac_stream_t stream);

/* ------------------------------- GLM predictive covariance, factored (Linear layers)
 * The same covariance for layers whose Jacobian row is rank one, without the rows.  For
 * a Linear layer M_{b,c} = abar_b delta_{b,c}^T, abar_b = [a_b | 1] the layer's input and
 * delta_{b,c} = d f_c(x_b) / d z at the layer's output z, so K1^T M K2 =
 * (K1^T abar_b)(K2^T delta_{b,c})^T and
 *   cov[b] (+)= sum_j s_j[b] * V_{j,b} V_{j,b}^T ,
 *   s_j[b] = || K1_j^T abar_{j,b} ||^2 ,   V_{j,b} = Delta_{j,b} K2_j   (nc x nG),
 * Delta_{j,b} the nc rows delta_{b,c}.  These jobs take row-major (Linear) inputs.  A
 * Conv2d layer's row is a sum over positions, not rank one: kfac_cov_conv_rows (below)
 * forms its rows on the device from the same (input, output Jacobian) pair, and they go
 * through kfac_kron_cov / kfac_kron_cov_sweep / kfac_kron_cov_joint as kfac_cov_job::J.
 * s_j[b] is summed over 64-column tiles of abar K1 in tile order, V V^T over K segments
 * in segment order, the jobs in job order, all in fp64 and without atomics: two calls
 * give identical bits, a sample's block depends on that sample only, and every nc x nc
 * block is bitwise symmetric (the lower triangle is computed and mirrored).
 * accumulate: cov += the sum, else cov = it.  At most 8 jobs and nc <= 32 per call. */
typedef struct kfac_cov_outer_job {
  const float* a; /* nb x cols row-major, row stride lda: the layer's input */
  int64_t lda;
  int32_t cols, has_ones; /* nA = cols + has_ones (implicit ones column last) */
  const float* D; /* row r = b*nc + c at D + r*ldD: nG elements, d f_c(x_b) / d z[g] */
  int64_t ldD;
  int32_t nG, reserved;
  const float* K1; /* nA x nA */
  int64_t ld1;
  const float* K2; /* nG x nG */
  int64_t ld2;
  int32_t lower1, lower2; /* K1 / K2 lower-triangular: their zero K-range is skipped */
} kfac_cov_outer_job;

KFAC_API size_t kfac_kron_cov_outer_workspace_bytes(const kfac_cov_outer_job* jobs, int njobs,
                                                    int64_t nb, int nc);
KFAC_API int kfac_kron_cov_outer(const kfac_cov_outer_job* jobs, int njobs, int64_t nb, int nc,
                                 int accumulate, float* cov, void* workspace, size_t workspace_bytes,
                                 kfac_stream_t stream);

/* ------------------------------- Conv2d Jacobian rows for the GLM predictive
 * The rows kfac_cov_job::J wants, for a Conv2d layer, from the pair the factored route
 * captures: the layer's input a (nb images C x H x W, x.sB apart; x is a KFAC_PATCH
 * operand over all nb*L positions, its ones column the bias row) and D, the Jacobian of
 * the outputs at the layer's output, D_{b,c} (nG x L, L = Ho*Wo) at D + (b*nc + c)*ldD:
 *   M_{b,c}[k][g]    = sum_p patch_b[p][k] * D_{b,c}[g][p]     (k < cols, F.unfold's order)
 *   M_{b,c}[cols][g] = sum_p D_{b,c}[g][p]                     (has_ones: the bias row)
 * written at M + (b*nc + c)*ldM, element k*nG + g, nA = cols + has_ones: the POSTERIOR's
 * order.  Only those nA*nG elements of each row are written.  One launch, no workspace:
 * per sample one fp32-MFMA GEMM over all nc*nG columns, an element one k-ordered fma chain
 * over the sample's positions (no split-K, no atomics).  Hence two calls give identical
 * bits, and a row depends on a_b, D_{b,c} and the shapes only: not on nb, not on nc, not on
 * where its columns fall among the tiles.  Zero padding, dilation 1, groups 1.  At most 8
 * jobs per call, nc >= 1 has no cap; kh, kw < 2^15, C*H*W < 2^31, x.sB >= C*H*W,
 * ldD >= nG*L, ldM >= nA*nG, every patch inside the padded image, x.rows = nb*L; nb,
 * nc*nG and the task count (nb x 64-row tiles x 64-column tiles, summed over the jobs)
 * must fit 31 bits.                                                               */
typedef struct kfac_cov_conv_rows_job {
  kfac_operand x; /* layout KFAC_PATCH, rows = nb*L */
  const float* D;
  int64_t ldD;
  int32_t nG, reserved;
  float* M;
  int64_t ldM;
} kfac_cov_conv_rows_job;

KFAC_API int kfac_cov_conv_rows(const kfac_cov_conv_rows_job* jobs, int njobs, int64_t nb, int nc,
                                kfac_stream_t stream);

/* ----------------------------- GLM predictive covariance, joint across the samples
 * The calls above stop at the block diagonal.  With rows r = b*nc + c, R = nb*nc, and
 * T_r = K1^T M_r K2, the joint calls give the whole R x R matrix
 *   kfac_kron_cov_joint        cov[r][r'] (+)= sum_j < T_{j,r} , T_{j,r'} >_F
 *   kfac_kron_cov_outer_joint  cov[r][r'] (+)= sum_j S_j[b(r)][b(r')] * W_j[r][r'] ,
 *                              S_j = U_j U_j^T (U = Abar K1, nb x nA), W_j = V_j V_j^T
 *                              (V = Delta K2, R x nG): Linear layers, no row formed
 * (jobs as kfac_cov_job / kfac_cov_outer_job; the diagonal blocks b(r) = b(r') are what
 * kfac_kron_cov / kfac_kron_cov_outer compute).  cov is R x R with row stride ldc >= R;
 * columns >= R of a row are not touched.  K (nA*nG, or nA and nG) is cut into 2048-long
 * segments that depend on K alone; 64x64 tiles of the Grams are summed over a segment in
 * fp32 (MFMA, exact products, k-ordered), the partials over segments in segment order and
 * over jobs in job order in fp64, without atomics.  Hence: two calls give identical bits;
 * the R x R matrix is bitwise symmetric (the lower triangle is computed and mirrored);
 * diagonal entries are >= 0; and an entry depends on its two rows, the factors and the
 * job shapes only -- not on nb, nor on where the rows sit in the call -- so the joint
 * covariance of a subset of the samples has the bits of those sub-blocks of the whole.
 * accumulate: cov += the sum, else cov = it.  At most 8 jobs per call; nc >= 1 has no
 * cap (rows are tiled, not classes; nb = 1 gives one sample's full covariance), R and
 * every launch's task count must fit 31 bits (R <= 2^21).                            */
KFAC_API size_t kfac_kron_cov_joint_workspace_bytes(const kfac_cov_job* jobs, int njobs, int64_t nb,
                                                    int nc);
KFAC_API int kfac_kron_cov_joint(const kfac_cov_job* jobs, int njobs, int64_t nb, int nc, int accumulate,
                                 float* cov, int64_t ldc, void* workspace, size_t workspace_bytes,
                                 kfac_stream_t stream);
KFAC_API size_t kfac_kron_cov_outer_joint_workspace_bytes(const kfac_cov_outer_job* jobs, int njobs,
                                                          int64_t nb, int nc);
KFAC_API int kfac_kron_cov_outer_joint(const kfac_cov_outer_job* jobs, int njobs, int64_t nb, int nc,
                                       int accumulate, float* cov, int64_t ldc, void* workspace,
                                       size_t workspace_bytes, kfac_stream_t stream);

/* ----------------------------- GLM predictive covariance, any number of outputs
 * kfac_kron_cov / kfac_kron_cov_outer with the classes tiled instead of capped: the same
 * jobs, the same cov (nb x nc x nc contiguous, sample stride nc*nc), nc >= 1 with no cap
 * (a CIFAR-100 or ImageNet head).  T_r (or s_j[b] and V) come from the same launches as in
 * those calls, over all nb*nc rows at once; a sample's block is then cut into 64x64 class
 * tiles and every tile pair ti >= tj is the joint calls' Gram tile on that sample's rows:
 *   kfac_kron_cov_tiled        cov[b][c][c'] (+)= sum_j < T_{j,b,c} , T_{j,b,c'} >_F
 *   kfac_kron_cov_outer_tiled  cov[b]        (+)= sum_j s_j[b] * V_{j,b} V_{j,b}^T
 * K (nA*nG, or nG) is cut into 2048-long segments that depend on K alone; a tile is summed
 * over a segment in fp32 (MFMA, exact products, k-ordered), the partials over segments in
 * segment order, (outer: times s_j[b], summed over its 64-column tiles in tile order,) over
 * jobs in job order, all in fp64, without atomics.  Hence: two calls give identical bits;
 * every block is bitwise symmetric (the lower triangle is computed and mirrored); diagonal
 * entries are >= 0; a sample's block depends on that sample only, so chunking the samples
 * changes no bit; and kfac_kron_cov_tiled's block b has exactly the bits of block (b, b) of
 * kfac_kron_cov_joint on the same jobs (one Gram body, segmentation and reduce order).
 * accumulate: cov += the sum, else cov = it.  At most 8 jobs per call; nb*nc, rows*nG,
 * rows*nA as in the calls above, and the Gram launch's task count (nb x segments x tile
 * pairs, summed over the jobs) must fit 31 bits.  Workspace per job: U and T (dense) or
 * the row-norm partials and V (outer), plus nb * ceil(K/2048) * t(t+1)/2 partials of
 * 64x64 floats, t = ceil(nc/64).                                                     */
KFAC_API size_t kfac_kron_cov_tiled_workspace_bytes(const kfac_cov_job* jobs, int njobs, int64_t nb,
                                                    int nc);
KFAC_API int kfac_kron_cov_tiled(const kfac_cov_job* jobs, int njobs, int64_t nb, int nc, int accumulate,
                                 float* cov, void* workspace, size_t workspace_bytes,
                                 kfac_stream_t stream);
KFAC_API size_t kfac_kron_cov_outer_tiled_workspace_bytes(const kfac_cov_outer_job* jobs, int njobs,
                                                          int64_t nb, int nc);
KFAC_API int kfac_kron_cov_outer_tiled(const kfac_cov_outer_job* jobs, int njobs, int64_t nb, int nc,
                                       int accumulate, float* cov, void* workspace,
                                       size_t workspace_bytes, kfac_stream_t stream);

/* --------------------------- GLM Monte-Carlo predictive: logit draws, softmax statistics
 * A posterior weight draw is S = K1 Z K2^T (kfac_sample; Z is its z, index a*nG + g), and
 * the linearised network is linear in the weights, so draw s moves logit row r = b*nc + c by
 *   F[s][r] (+)= sum_j < M_{j,r} , K1_j Z_{j,s} K2_j^T >_F = sum_j < T_{j,r} , Z_{j,s} >_F ,
 * T_r = K1^T M_r K2 the projected row of the covariance calls: exactly what kfac_sample's
 * draw from Z_s would do to the linearised logits, jointly for all samples of the call (one
 * draw is one weight sample), with covariance kfac_kron_cov_joint's.  No Cholesky of the
 * covariance, no weight sample, no forward pass; any nc, any rank.
 *   kfac_glm_draws        rows given (Conv2d rows, dense Jacobians): T by the projection of
 *                         kfac_kron_cov_joint, then F = Z T^T over K = nA*nG
 *   kfac_glm_draws_outer  Linear layers, no row formed: T_r = u_b v_r^T, so
 *                         F[s][r] = u_b^T Z_s v_r with U = Abar K1 (nb x nA) and
 *                         V = Delta K2 (R x nG), kfac_kron_cov_outer_joint's U and V;
 *                         per draw 2*nb*nA*nG flops, Z read once per 64 samples
 * Z_s is nA*nG elements at Z + s*ldZ (ldZ >= nA*nG), the draw in kfac_sample's order.
 * F[s][r] is at F + s*ldF + r, R = nb*nc, ldF >= R; columns >= R are never touched.
 * accumulate: F += the sum over jobs, else F = it.
 * Sums: a 64x64 tile over one 2048-long segment of K = nA*nG (rows given), or W = U Z_s over
 * all of nA and then W V over one 64-column tile of nG (outer), in fp32 (MFMA, exact
 * products, k-ordered); the segments (g-tiles) in order and the jobs in job order in fp64;
 * no atomics.  The cut points depend on nA and nG alone.  Hence: two calls give identical
 * bits; F[s][r] depends on row r's inputs, draw s, the factors and the job shapes only --
 * not on nb or ns, nor on where the sample sits in the call or the draw sits in Z -- so
 * chunking the samples or the draws changes no bit.
 * At most 8 jobs per call; nc >= 1 and ns >= 1 have no cap; R, ns, rows*nG, rows*nA and
 * every launch's task count must fit 31 bits.  KFAC_EINVAL: null pointers, pitches below
 * the widths, njobs outside 1..8, nb, nc or ns < 1, ldF < R; KFAC_EWORKSPACE: a workspace
 * below the query's answer.  All of it is checked before any launch.  Workspace per job:
 * U and T (rows given) plus ceil(K/2048) x ceil(R/64) x ceil(ns/64) tiles of 64x64 floats;
 * U, V, V^T (outer) plus ns x ceil(nG/64) x R floats.                                   */
typedef struct kfac_draw_job { /* rows given: Conv2d rows, dense Jacobians */
  kfac_cov_job rows; /* J, K1, K2, lower1/2 exactly as kfac_kron_cov_joint takes them */
  const float* Z;    /* draw s at Z + s*ldZ: nA*nG elements, index a*nG + g (kfac_sample's z) */
  int64_t ldZ;
} kfac_draw_job;

typedef struct kfac_draw_outer_job { /* Linear layers, no row formed */
  kfac_cov_outer_job rows; /* a, D, K1, K2 exactly as kfac_kron_cov_outer_joint takes them */
  const float* Z;
  int64_t ldZ;
} kfac_draw_outer_job;

KFAC_API size_t kfac_glm_draws_workspace_bytes(const kfac_draw_job* jobs, int njobs, int64_t nb, int nc,
                                               int64_t ns);
KFAC_API int kfac_glm_draws(const kfac_draw_job* jobs, int njobs, int64_t nb, int nc, int64_t ns,
                            int accumulate, float* F, int64_t ldF, void* workspace, size_t workspace_bytes,
                            kfac_stream_t stream);
KFAC_API size_t kfac_glm_draws_outer_workspace_bytes(const kfac_draw_outer_job* jobs, int njobs, int64_t nb,
                                                     int nc, int64_t ns);
KFAC_API int kfac_glm_draws_outer(const kfac_draw_outer_job* jobs, int njobs, int64_t nb, int nc, int64_t ns,
                                  int accumulate, float* F, int64_t ldF, void* workspace,
                                  size_t workspace_bytes, kfac_stream_t stream);

/* The softmax statistics of the draws: with y_s = mean[b] + F[s][b] (nc logits),
 *   psum[b][c] (+)= sum_s softmax(y_s)[c] ,   hsum[b] (+)= sum_s H(softmax(y_s))   (nats),
 * H = log sum_c e^y - sum_c p_c y after subtracting the row maximum.  mean is nb x nc with
 * row stride ldm >= nc, F as above (ldF >= nb*nc), psum nb x nc and hsum nb contiguous fp64.
 * Evaluated in fp64 from the fp32 inputs (exp and log in fp64: logits of +-80 neither
 * overflow nor give NaN), the draws summed in draw order; one launch, no workspace, no
 * atomics, any nc.  accumulate: the running sums go on from psum / hsum (the draws given in
 * chunks change no bit against one call), else they start at 0.
 * KFAC_EINVAL: null pointers, ns, nb or nc < 1, ldm < nc, ldF < nb*nc.                  */
KFAC_API int kfac_softmax_mc(const float* mean, int64_t ldm, const float* F, int64_t ldF, int64_t ns,
                             int64_t nb, int nc, int accumulate, double* psum, double* hsum,
                             kfac_stream_t stream);

/* ------------------------------ GLM predictive covariance over a damping grid
 * With A = VA diag(lamA) VA^T and G = VG diag(lamG) VG^T (kfac_syev), kfac_invert's
 * factors satisfy L_A L_A^T = VA diag(wA) VA^T, wA[i] = 1 / (sqrt(s) lamA[i] + sqrt(n)),
 * and likewise for G: in the eigenbasis a damping (n, s) is a pair of weight vectors.
 * For nt of them at once (1 <= nt <= 64), cov is nt x nb x nc x nc:
 *   kfac_kron_cov_sweep        Y_{b,c} = VA^T M_{b,c} VG once per call, then
 *     cov[t][b][c][c'] (+)= sum_j sum_{i,g} wA_t[i] wG_t[g] Y_{b,c}[i][g] Y_{b,c'}[i][g]
 *   kfac_kron_cov_outer_sweep  p_b = VA^T abar_b and Q_b = Delta_b VG once per call, then
 *     cov[t][b] (+)= sum_j (sum_i wA_t[i] p_b[i]^2) * Q_b diag(wG_t) Q_b^T
 * The weights are plain non-negative numbers (the calls know nothing of damping); row t
 * of wA / wG is grid point t.  The guarantees of kfac_kron_cov / kfac_kron_cov_outer hold
 * per grid point (fixed-order fp64 reduction, no atomics, bitwise symmetric blocks, a
 * sample's block depends on that sample only), and slice t of an nt-call has the bits of
 * the nt = 1 call with row t's weights.  At most 8 jobs and nc <= 32 per call.         */
typedef struct kfac_cov_sweep_job {
  const float* J; /* as kfac_cov_job */
  int64_t ldJ;
  int32_t nA, nG;
  const float* VA; /* nA x nA, eigenvectors as columns (kfac_syev's evecs) */
  int64_t ldA;
  const float* VG; /* nG x nG */
  int64_t ldG;
  const float* wA; /* nt x nA, row t at wA + t*ldwA */
  int64_t ldwA;
  const float* wG; /* nt x nG */
  int64_t ldwG;
} kfac_cov_sweep_job;

KFAC_API size_t kfac_kron_cov_sweep_workspace_bytes(const kfac_cov_sweep_job* jobs, int njobs,
                                                    int64_t nb, int nc, int nt);
KFAC_API int kfac_kron_cov_sweep(const kfac_cov_sweep_job* jobs, int njobs, int64_t nb, int nc, int nt,
                                 int accumulate, float* cov, void* workspace, size_t workspace_bytes,
                                 kfac_stream_t stream);

typedef struct kfac_cov_outer_sweep_job {
  const float* a; /* as kfac_cov_outer_job */
  int64_t lda;
  int32_t cols, has_ones;
  const float* D;
  int64_t ldD;
  int32_t nG, reserved;
  const float* VA; /* nA x nA, nA = cols + has_ones */
  int64_t ldA;
  const float* VG; /* nG x nG */
  int64_t ldG;
  const float* wA; /* nt x nA */
  int64_t ldwA;
  const float* wG; /* nt x nG */
  int64_t ldwG;
} kfac_cov_outer_sweep_job;

KFAC_API size_t kfac_kron_cov_outer_sweep_workspace_bytes(const kfac_cov_outer_sweep_job* jobs,
                                                          int njobs, int64_t nb, int nc, int nt);
KFAC_API int kfac_kron_cov_outer_sweep(const kfac_cov_outer_sweep_job* jobs, int njobs, int64_t nb,
                                       int nc, int nt, int accumulate, float* cov, void* workspace,
                                       size_t workspace_bytes, kfac_stream_t stream);

/* ------------------- GLM predictive covariance with per-entry eigenbasis weights
 * The sweep calls' weights are rank one, w[i][g] = wA[i] wG[g]; a posterior that keeps the
 * KFAC eigenbases but refits every one of the nA*nG eigenvalues (EFB.sample draws
 * S = VA (Z o Lambda^-T) VG^T, Lambda^- = EFB.inv_state (nG x nA)) needs an arbitrary
 * non-negative W[i][g] (for EFB: W[i][g] = Lambda^-[g][i]^2).  For nt weight matrices at
 * once (1 <= nt <= 64), cov is nt x nb x nc x nc:
 *   kfac_kron_cov_full        Y_{b,c} = VA^T M_{b,c} VG once per call, then
 *     cov[t][b][c][c'] (+)= sum_j sum_{i,g} W_t[i][g] Y_{b,c}[i][g] Y_{b,c'}[i][g]
 *   kfac_kron_cov_outer_full  p_b = VA^T abar_b and Q_b = Delta_b VG once per call, then
 *     cov[t][b] (+)= sum_j Q_b diag(r_{t,b}) Q_b^T ,  r_{t,b}[g] = sum_i p_b[i]^2 W_t[i][g]
 *     (r = (P o P) W_t: one nb x nA by nA x nG GEMM per grid point)
 * W is nt matrices in the posterior's flat order i*nG + g, grid point t at W + t*ldW,
 * ldW >= nA*nG.  The weights are plain non-negative numbers: the calls know nothing of
 * damping.  Guarantees (the sweep calls'): every reduction runs in a fixed order, the sums
 * across segments and across jobs in fp64; no atomics; two calls give identical bits; every
 * nc x nc block is bitwise symmetric with a non-negative diagonal; a sample's block depends
 * on that sample only; slice t of an nt-call has the bits of the nt = 1 call with W_t.
 * At most 8 jobs and nc <= 32 per call; KFAC_EINVAL is returned before any launch,
 * KFAC_EWORKSPACE when the workspace is smaller than the query's answer.                */
typedef struct kfac_cov_full_job {
  const float* J; /* as kfac_cov_job */
  int64_t ldJ;
  int32_t nA, nG;
  const float* VA; /* nA x nA, eigenvectors as columns */
  int64_t ldA;
  const float* VG; /* nG x nG */
  int64_t ldG;
  const float* W; /* nt x (nA*nG), element (t, i, g) at W[t*ldW + i*nG + g] */
  int64_t ldW;
} kfac_cov_full_job;

KFAC_API size_t kfac_kron_cov_full_workspace_bytes(const kfac_cov_full_job* jobs, int njobs, int64_t nb,
                                                   int nc, int nt);
KFAC_API int kfac_kron_cov_full(const kfac_cov_full_job* jobs, int njobs, int64_t nb, int nc, int nt,
                                int accumulate, float* cov, void* workspace, size_t workspace_bytes,
                                kfac_stream_t stream);

typedef struct kfac_cov_outer_full_job {
  const float* a; /* as kfac_cov_outer_job */
  int64_t lda;
  int32_t cols, has_ones;
  const float* D;
  int64_t ldD;
  int32_t nG, reserved;
  const float* VA; /* nA x nA, nA = cols + has_ones */
  int64_t ldA;
  const float* VG; /* nG x nG */
  int64_t ldG;
  const float* W; /* nt x (nA*nG), as kfac_cov_full_job */
  int64_t ldW;
} kfac_cov_outer_full_job;

KFAC_API size_t kfac_kron_cov_outer_full_workspace_bytes(const kfac_cov_outer_full_job* jobs, int njobs,
                                                         int64_t nb, int nc, int nt);
KFAC_API int kfac_kron_cov_outer_full(const kfac_cov_outer_full_job* jobs, int njobs, int64_t nb, int nc,
                                      int nt, int accumulate, float* cov, void* workspace,
                                      size_t workspace_bytes, kfac_stream_t stream);

/* ------- GLM predictive covariance over a damping grid / with per-entry weights, any number of outputs
 * The four weighted calls above with the classes tiled instead of capped: the same job
 * structs, the same cov (nt x nb x nc x nc contiguous), nc >= 1 with no cap, 1 <= nt <= 64.
 * The projections are the capped calls' own launches over all nb*nc rows at once; a sample's
 * block is then cut into 64x64 class tiles and every tile pair ti >= tj is one weighted Gram
 * tile of that sample's projected rows X_b (nc x K),
 *   part[r][r'] = sum_k X_b[r][k] * (w_t[k] * X_b[r'][k]) ,
 * the weight folded into one operand as it is loaded (no product is stored):
 *   kfac_kron_cov_full_tiled         X = Y (K = nA*nG), w_t[k] = W_t[k]
 *   kfac_kron_cov_sweep_tiled        X = Y (K = nA*nG), w_t[k] = wA_t[k / nG] * wG_t[k % nG]
 *   kfac_kron_cov_outer_full_tiled   X = Q_b (K = nG),  w_t = r_{t,b}
 *   kfac_kron_cov_outer_sweep_tiled  X = Q_b (K = nG),  w_t = wG_t, the block times
 *                                    s_{t,b} = sum_i wA_t[i] p_b[i]^2
 * K is cut into 2048-long segments that depend on K alone; a tile is summed over a segment in
 * fp32 (MFMA, exact products, one k-ordered chain from 0 per element), the partials over
 * segments in segment order, (outer sweep: times s_{t,b}, summed over its 64-column tiles in
 * tile order,) over jobs in job order, all in fp64, without atomics.  Hence: two calls give
 * identical bits; every block is bitwise symmetric (the lower triangle is computed and
 * mirrored); a sample's block depends on that sample only, so chunking the samples changes no
 * bit; slice t has the bits of the nt = 1 call with grid point t's weights (one grid point per
 * Gram task); and with every weight equal to 1 kfac_kron_cov_full_tiled and
 * kfac_kron_cov_sweep_tiled give, on every slice, the bits of kfac_kron_cov_tiled with
 * K1 = VA, K2 = VG dense (one tile body, segmentation and reduce order; x * 1 is exact).
 * Against the capped calls (nc <= 32 is valid here: one tile pair) the summation order
 * differs: agreement to fp32 rounding.  accumulate: cov += the sum, else cov = it.
 * At most 8 jobs per call; nb*nc, rows*nG, rows*nA as in the calls above, and the Gram
 * launch's task count (nb x segments x nt x tile pairs, summed over the jobs) must fit 31
 * bits.  KFAC_EINVAL is returned before any launch, KFAC_EWORKSPACE when the workspace is
 * smaller than the query's answer.  Workspace per job, every part rounded up to 256 bytes,
 * P = nt * nb * ceil(K/2048) * t(t+1)/2 partials of 64x64 floats, t = ceil(nc/64):
 *   full_tiled, sweep_tiled   U and T (nb*nc*nA*nG floats each), P with K = nA*nG
 *   outer_full_tiled          P2T (nA*nb), R (nt*nb*nG), V (nb*nc*nG), P with K = nG
 *   outer_sweep_tiled         the row-norm partials (nt*ceil(nA/64)*nb), V, P with K = nG */
KFAC_API size_t kfac_kron_cov_full_tiled_workspace_bytes(const kfac_cov_full_job* jobs, int njobs,
                                                         int64_t nb, int nc, int nt);
KFAC_API int kfac_kron_cov_full_tiled(const kfac_cov_full_job* jobs, int njobs, int64_t nb, int nc, int nt,
                                      int accumulate, float* cov, void* workspace, size_t workspace_bytes,
                                      kfac_stream_t stream);
KFAC_API size_t kfac_kron_cov_outer_full_tiled_workspace_bytes(const kfac_cov_outer_full_job* jobs,
                                                               int njobs, int64_t nb, int nc, int nt);
KFAC_API int kfac_kron_cov_outer_full_tiled(const kfac_cov_outer_full_job* jobs, int njobs, int64_t nb,
                                            int nc, int nt, int accumulate, float* cov, void* workspace,
                                            size_t workspace_bytes, kfac_stream_t stream);
KFAC_API size_t kfac_kron_cov_sweep_tiled_workspace_bytes(const kfac_cov_sweep_job* jobs, int njobs,
                                                          int64_t nb, int nc, int nt);
KFAC_API int kfac_kron_cov_sweep_tiled(const kfac_cov_sweep_job* jobs, int njobs, int64_t nb, int nc,
                                       int nt, int accumulate, float* cov, void* workspace,
                                       size_t workspace_bytes, kfac_stream_t stream);
KFAC_API size_t kfac_kron_cov_outer_sweep_tiled_workspace_bytes(const kfac_cov_outer_sweep_job* jobs,
                                                                int njobs, int64_t nb, int nc, int nt);
KFAC_API int kfac_kron_cov_outer_sweep_tiled(const kfac_cov_outer_sweep_job* jobs, int njobs, int64_t nb,
                                             int nc, int nt, int accumulate, float* cov, void* workspace,
                                             size_t workspace_bytes, kfac_stream_t stream);

/* ------------------- GLM predictive covariance under the INF posterior
 * INF (low-rank EFB plus a diagonal correction) is Gaussian with precision
 *   P = s (U Lambda U^T + D+) + n I ,  U = kron(UA, UG)  (nA*nG x r, r = ra*rg).
 * By Woodbury, with w = 1 / (s D+ + n) (nA x nG, flat order i*nG + g), sigma = sqrt(s Lambda),
 * B = chol(I + sigma U^T diag(w) U sigma) and F = B^-1 diag(sigma) (r x r):
 *   P^-1 = diag(w) - diag(w) U F^T F U^T diag(w) ,
 *   cov[b][c][c'] (+)= sum_j [ sum_{i,g} W[i][g] M_{b,c}[i][g] M_{b,c'}[i][g] - < F t_{b,c}, F t_{b,c'} > ] ,
 *   t_{b,c}[p*rg + q] = sum_{i,g} UA[i][p] W[i][g] M_{b,c}[i][g] UG[g][q] .
 *   kfac_inf_cov        dense rows M (J as kfac_cov_job): X = UA^T (M o W), t = X UG, y = t F^T,
 *                       then the per-entry weighted Gram of the raw rows minus the Gram of y
 *   kfac_inf_cov_outer  Linear layers, M_{b,c} = abar_b delta_{b,c}^T, no row is formed:
 *                       rho_b[g] = sum_i abar_b[i]^2 W[i][g] and H_b[p][g] = sum_i UA[i][p] abar_b[i] W[i][g]
 *                       from ONE GEMM, t_{b,c}[p][q] = sum_g H_b[p][g] delta_{b,c}[g] UG[g][q], y = t F^T,
 *                       then Delta_b diag(rho_b) Delta_b^T minus the Gram of y
 * W and F are plain numbers (W >= 0): the calls know nothing of damping.  Guarantees: every
 * reduction runs in a fixed order, the sums across segments, the difference of the two terms
 * and the sum across jobs in fp64; no atomics; two calls give identical bits; every nc x nc
 * block is bitwise symmetric; a sample's block depends on that sample only (chunking the
 * samples changes no bit).  The diagonal is the difference of two non-negative sums and is
 * NOT clamped: where the low-rank term cancels the diagonal one it may come out negative at
 * rounding level.  At most 8 jobs and nc <= 32 per call; KFAC_EINVAL is returned before any
 * launch, KFAC_EWORKSPACE when the workspace is smaller than the query's answer.          */
typedef struct kfac_inf_cov_job {
  const float* J; /* as kfac_cov_job */
  int64_t ldJ;
  int32_t nA, nG;
  const float* UA; /* nA x ra, row-major */
  int64_t ldA;
  int32_t ra;
  const float* UG; /* nG x rg */
  int64_t ldG;
  int32_t rg;
  const float* W; /* nA*nG, element (i, g) at W[i*nG + g] */
  int64_t ldW;    /* >= nA*nG */
  const float* F; /* r x r, row-major, r = ra*rg, index p*rg + q */
  int64_t ldF;
} kfac_inf_cov_job;

KFAC_API size_t kfac_inf_cov_workspace_bytes(const kfac_inf_cov_job* jobs, int njobs, int64_t nb, int nc);
KFAC_API int kfac_inf_cov(const kfac_inf_cov_job* jobs, int njobs, int64_t nb, int nc, int accumulate,
                          float* cov, void* workspace, size_t workspace_bytes, kfac_stream_t stream);

typedef struct kfac_inf_cov_outer_job {
  const float* a; /* as kfac_cov_outer_job */
  int64_t lda;
  int32_t cols, has_ones;
  const float* D;
  int64_t ldD;
  int32_t nG, reserved;
  const float* UA; /* nA x ra, nA = cols + has_ones */
  int64_t ldA;
  int32_t ra;
  const float* UG; /* nG x rg */
  int64_t ldG;
  int32_t rg;
  const float* W; /* as kfac_inf_cov_job */
  int64_t ldW;
  const float* F;
  int64_t ldF;
} kfac_inf_cov_outer_job;

KFAC_API size_t kfac_inf_cov_outer_workspace_bytes(const kfac_inf_cov_outer_job* jobs, int njobs, int64_t nb,
                                                   int nc);
KFAC_API int kfac_inf_cov_outer(const kfac_inf_cov_outer_job* jobs, int njobs, int64_t nb, int nc,
                                int accumulate, float* cov, void* workspace, size_t workspace_bytes,
                                kfac_stream_t stream);

/* ------- GLM predictive covariance under the INF posterior, any number of outputs
 * The two calls above with the classes tiled instead of capped: the same job structs and
 * arguments, the same cov (nb x nc x nc contiguous), the same mathematics, nc >= 1 with no cap.
 * The projections (h | x, t, y) are the capped calls' own launches over all nb*nc rows at once.
 * A sample's block is then cut into 64x64 class tiles and every tile pair ti >= tj is computed
 * as two separate fp32 tile Grams,
 *   part1[c][c'] = sum_k R_b[c][k] * (w_b[k] * R_b[c'][k])   the weight folded into one operand
 *                                                           as it is loaded; R_b the RAW rows:
 *       kfac_inf_cov_tiled        R_b = J (stride ldJ), K = nA*nG, w = W
 *       kfac_inf_cov_outer_tiled  R_b = Delta_b (stride ldD), K = nG, w_b = rho_b
 *   part2[c][c'] = < y_{b,c}, y_{b,c'} >                     K = r = ra*rg
 * in ONE Gram launch.  K is cut into 2048-long segments that depend on K alone; a tile is summed
 * over a segment in fp32 (MFMA, one k-ordered chain from 0 per element); the reduce forms
 *   sum_jobs ( sum_segments part1 - sum_segments part2 )
 * in fp64, segments in segment order, jobs in job order, without atomics: the difference of the
 * two terms is never taken in fp32.  Hence: two calls give identical bits; every block is
 * bitwise symmetric (the lower triangle is computed and mirrored); a sample's block depends on
 * that sample only, so chunking the samples changes no bit; padded leading dimensions change no
 * bit; and with F = 0 kfac_inf_cov_tiled gives the bits of kfac_kron_cov_full_tiled (nt = 1) on
 * the same J and W with VA, VG identity matrices (one tile body, segmentation and reduce order;
 * x * 1 and s - 0 are exact).  Against the capped calls (nc <= 32 is valid here: one tile pair)
 * the segmentation differs (256 against 2048): agreement to fp32 rounding.  The diagonal is not
 * clamped.  accumulate: cov += the sum, else cov = it.
 * At most 8 jobs per call; nb*nc must stay below 2^31 - 64, as must the capped calls' column
 * and row counts (nb*nc*nG and nb*nc*ra dense, nb*(ra+1) outer), the tile pairs and the Gram
 * launch's task count (nb x (segments of term 1 + of term 2) x tile pairs, summed over the
 * jobs) must fit 31 bits.  KFAC_EINVAL is returned before any launch, KFAC_EWORKSPACE when the
 * workspace is smaller than the query's answer.  Workspace per job, in this order, every part
 * rounded up to 256 bytes, P(K) = nb * ceil(K/2048) * t(t+1)/2 partials of 64x64 floats,
 * t = ceil(nc/64):
 *   inf_cov_tiled         X (nb*nc*ra*nG floats), T and Y (nb*nc*r each), P(nA*nG), P(r)
 *   inf_cov_outer_tiled   HR (nb*(ra+1)*nG floats), T and Y (nb*nc*r each), P(nG), P(r)      */
KFAC_API size_t kfac_inf_cov_tiled_workspace_bytes(const kfac_inf_cov_job* jobs, int njobs, int64_t nb,
                                                   int nc);
KFAC_API int kfac_inf_cov_tiled(const kfac_inf_cov_job* jobs, int njobs, int64_t nb, int nc, int accumulate,
                                float* cov, void* workspace, size_t workspace_bytes, kfac_stream_t stream);
KFAC_API size_t kfac_inf_cov_outer_tiled_workspace_bytes(const kfac_inf_cov_outer_job* jobs, int njobs,
                                                         int64_t nb, int nc);
KFAC_API int kfac_inf_cov_outer_tiled(const kfac_inf_cov_outer_job* jobs, int njobs, int64_t nb, int nc,
                                      int accumulate, float* cov, void* workspace, size_t workspace_bytes,
                                      kfac_stream_t stream);

/* ------- GLM Monte-Carlo predictive under the INF posterior: exact logit draws
 * With P^-1 = diag(w) - diag(w) U F^T F U^T diag(w) as above, c = sqrt(w) entrywise, Z (nA x nG)
 * and eps (r) standard normal and independent,
 *   x = c o Z - w o [ UA mat(F^T q) UG^T ] ,   q = F vec(UA^T (c o Z) UG) + B^-1 eps
 * is distributed N(0, P^-1) exactly (Matheron's rule on the Woodbury form; without the eps part
 * the covariance lacks a term).  No square root beyond sqrt(w).  The draw moves logit row
 * r = b*nc + c' of the linearised network by
 *   F[s][r] (+)= sum_j [ < M_{j,r} o C_j , Z_{j,s} > - < y_{j,r} , q_{j,s} > ] ,   y_r = F t_r ,
 * t_r, y_r exactly the projections of kfac_inf_cov / kfac_inf_cov_outer.  One draw is one weight
 * sample for all samples of the call: the draws are jointly consistent.
 *   kfac_inf_draws        rows given (Conv2d rows, dense Jacobians)
 *   kfac_inf_draws_outer  Linear layers, M_{b,c'} = abar_b delta_{b,c'}^T, no row is formed: the
 *                         first term is abar_b^T (C o Z_s) delta_{b,c'}
 * A job is the covariance call's job plus C (nA*nG floats sqrt(w), flat order i*nG + g; passed,
 * never computed here), Binv (r x r, row stride ldB), Z (draw s at Z + s*ldZ: nA*nG values in
 * kfac_sample's order) and E (draw s at E + s*ldE: r values).  Plain numbers: the calls know
 * nothing of damping.  F[s][r] is at F + s*ldF + r, R = nb*nc, ldF >= R; columns >= R are never
 * touched.  accumulate: F += the sum over jobs, else F = it.
 * Stages (fp32 MFMA, exact products, every output element ONE k-ordered chain from 0; products
 * that are operands are formed as a panel is loaded and never stored):
 *   y       the covariance calls' own projection launches (h | x, t, y) on the rows, R x r
 *   F g     the dense projection launches with rows := draws, J := Z, W := C:
 *           G[s] = F vec(UA^T (C o Z_s) UG), ns x r
 *   q       Q = G + E Binv^T: the y-launch result G plus ONE second k-ordered chain over r
 *           (E Binv^T from 0), added once; q_s reads draw s only
 *   first   outer: one task per (draw, 64-column g-tile, 64-sample tile):
 *           W[b][g] = sum_a abar_b[a] (C[a][g] Z_s[a][g]) over all of nA (the raw a with the
 *           implicit ones column; C*Z rounded to fp32 once, as loaded), then
 *           part[s][g-tile][r] = sum_{g in tile} W[b(r)][g] Delta[r][g], one fma chain in g order
 *           on the raw Delta (read through a transpose);
 *           dense: a 64 x 64 tile of Z (C o J)^T over one 2048-long segment of K = nA*nG, the
 *           raw rows at ldJ scaled by C as they are loaded
 *   second  a 64 x 64 tile of Q Y^T over one 2048-long segment of r
 *   reduce  F[s][r] (+)= sum_jobs ( sum_{g-tiles | segments} first - sum_segments second ) in fp64,
 *           parts in part order, jobs in job order; no atomics; the difference is never taken
 *           in fp32.  The cut points depend on nA, nG and r alone.
 * Guarantees: two calls give identical bits; F[s][r] depends on row r's inputs, draw s, the
 * operands and the job shapes only -- not on nb or ns, nor on where the sample or the draw sits
 * -- so chunking the samples or the draws changes no bit; pad columns of F are never touched;
 * with F = 0 and Binv = 0 kfac_inf_draws_outer gives the bits of kfac_glm_draws_outer on the
 * same a, Delta with identity K1, K2 and Z pre-multiplied by C in fp32 (one tile body, g-tile
 * cut and reduce order; x * 1 and s - 0 are exact).
 * At most 8 jobs per call; nc >= 1 and ns >= 1 have no cap; R, ns, the projections' column and
 * row counts (R*nG and R*ra dense, nb*(ra+1) outer, ns*nG, ns*ra) and every launch's task count
 * must fit 31 bits.  KFAC_EINVAL: null pointers, pitches below the widths, njobs outside 1..8,
 * nb, nc or ns < 1, ldF < R; KFAC_EWORKSPACE: a workspace below the query's answer.  All of it
 * is checked before any launch.  Workspace per job, in this order, every part rounded up to
 * 256 bytes, T(K) = ceil(K/2048) x ceil(R/64) x ceil(ns/64) tiles of 64x64 floats:
 *   the rows' HX (R*ra*nG floats dense, nb*(ra+1)*nG outer), T and Y (R*r each); the draws' X
 *   (ns*ra*nG), T and G (ns*r each); Q (ns*r); outer: Dt (nG*R) and ns x ceil(nG/64) x R floats,
 *   dense: T(nA*nG); then T(r).                                                           */
typedef struct kfac_inf_draw_job { /* rows given: Conv2d rows, dense Jacobians */
  kfac_inf_cov_job rows; /* J, UA, UG, W, F exactly as kfac_inf_cov takes them */
  const float* C;        /* nA*nG: sqrt(W) entrywise, contiguous */
  const float* Binv;     /* r x r, row-major */
  int64_t ldB;
  const float* Z;        /* draw s at Z + s*ldZ: nA*nG elements, index i*nG + g */
  int64_t ldZ;
  const float* E;        /* draw s at E + s*ldE: r elements */
  int64_t ldE;
} kfac_inf_draw_job;

typedef struct kfac_inf_draw_outer_job { /* Linear layers, no row formed */
  kfac_inf_cov_outer_job rows; /* a, D, UA, UG, W, F exactly as kfac_inf_cov_outer takes them */
  const float* C;
  const float* Binv;
  int64_t ldB;
  const float* Z;
  int64_t ldZ;
  const float* E;
  int64_t ldE;
} kfac_inf_draw_outer_job;

KFAC_API size_t kfac_inf_draws_workspace_bytes(const kfac_inf_draw_job* jobs, int njobs, int64_t nb, int nc,
                                               int64_t ns);
KFAC_API int kfac_inf_draws(const kfac_inf_draw_job* jobs, int njobs, int64_t nb, int nc, int64_t ns,
                            int accumulate, float* F, int64_t ldF, void* workspace, size_t workspace_bytes,
                            kfac_stream_t stream);
KFAC_API size_t kfac_inf_draws_outer_workspace_bytes(const kfac_inf_draw_outer_job* jobs, int njobs, int64_t nb,
                                                     int nc, int64_t ns);
KFAC_API int kfac_inf_draws_outer(const kfac_inf_draw_outer_job* jobs, int njobs, int64_t nb, int nc, int64_t ns,
                                  int accumulate, float* F, int64_t ldF, void* workspace,
                                  size_t workspace_bytes, kfac_stream_t stream);

/* -------------------------------------------------------- posterior samples
 * out_j = (LA_j Z_j LG_j^T)^T, shape (nG x nA): KFAC.sample, curvatures.py:400-405,
 * with Z (nA x nG row-major) supplied by the caller (torch.randn, the reference's
 * draw).  LA/LG are lower-triangular with zero upper triangles (KFAC.invert's
 * factors): tiles above the diagonal are skipped.  Columns a < wcols go to W[g*ldW + a]; when wcols == nA-1 column
 * nA-1 goes to bias[g] (Curvature._replace, curvatures.py:68-82; bias may be NULL
 * to drop it).  accumulate: W += sample (sample_and_replace) else W = sample.
 * At most 8 jobs per call.                                                    */
typedef struct kfac_sample_job {
  const float* LA;
  int64_t ldA;
  const float* LG;
  int64_t ldG;
  const float* Z;
  int32_t nA, nG;
  float* W;
  int64_t ldW;
  float* bias;
  int32_t wcols;
  int32_t dense; /* 1: LA/LG are full matrices (EFB eigenvectors, curvatures.py:466-473) */
} kfac_sample_job;

KFAC_API size_t kfac_sample_workspace_bytes(const kfac_sample_job* jobs, int njobs);
KFAC_API int kfac_sample(const kfac_sample_job* jobs, int njobs, int accumulate, void* workspace,
                size_t workspace_bytes, kfac_stream_t stream);

/* ------------------------------------------------ eigenbasis curvatures
 * kfac_efb_update: EFB.update (models/curvatures.py:427-449) for up to 8 layers:
 *   state = [state +] (VG^T grad VA) ** 2          (nG x nA, elementwise square)
 *   diag  = [diag  +] (grad ** 2) * scale           (scale = batch size; diag may be NULL)
 * grad is the layer's (nG x nA) weight gradient with the bias gradient as its last
 * column; VA (nA x nA) and VG (nG x nG) the factors' eigenvectors (columns).  "+"
 * when accumulate != 0, else the results are written.  Two launches; the projection
 * VG^T grad lives in the workspace (nG x nA floats per layer).                  */
typedef struct kfac_efb_job {
  const float* VA;
  int64_t ldA;
  const float* VG;
  int64_t ldG;
  const float* grad;
  int64_t ld_grad;
  float* state;
  int64_t ld_state;
  float* diag;
  int64_t ld_diag;
  int32_t nA, nG;
  int32_t accumulate;
  float scale;
} kfac_efb_job;

KFAC_API size_t kfac_efb_workspace_bytes(const kfac_efb_job* jobs, int njobs);
KFAC_API int kfac_efb_update(const kfac_efb_job* jobs, int njobs, void* workspace, size_t workspace_bytes,
                             kfac_stream_t stream);

/* kfac_kron_gram: INF.pre_sampler's V_s^T V_s (curvatures.py:548-580), V_s =
 * c * kron(UA, UG) * sigma, without forming V_s ((nA*nG) x (la*lg)):
 *   out[(p*lg+q)*ldo + p2*lg+q2] = sigma[p*lg+q] * sum_{a,g} c[a*nG+g]^2 UA[a][p] UA[a][p2]
 *                                  UG[g][q] UG[g][q2] * sigma[p2*lg+q2]
 * UA (nA x la, ldA), UG (nG x lg, ldG), c (nA*nG), sigma (la*lg).  Symmetric up
 * to one rounding of the sigma scaling.  Workspace: nA x lg^2 floats per job; up
 * to 8 jobs.                                                                    */
typedef struct kfac_gram_job {
  const float* UA;
  int64_t ldA;
  const float* UG;
  int64_t ldG;
  const float* c;
  const float* sigma;
  float* out;
  int64_t ldo;
  int32_t nA, nG, la, lg;
} kfac_gram_job;

KFAC_API size_t kfac_gram_workspace_bytes(const kfac_gram_job* jobs, int njobs);
KFAC_API int kfac_kron_gram(const kfac_gram_job* jobs, int njobs, void* workspace, size_t workspace_bytes,
                            kfac_stream_t stream);

/* ------------------------------------------------- packed lower triangles
 * For the data-parallel collectives (no reference counterpart: the reference is
 * single-device).  Row i of a factor's lower triangle lives at
 * packed[offset + i(i+1)/2 .. + i], so a factor takes n(n+1)/2 floats and the
 * caller lays the factors out back to back.
 *   kfac_tri_pack  : packed <- lower triangles of the F's (the all-reduce of the
 *                    per-rank factor sums, curvatures.py:359-363 summed over ranks)
 *   kfac_tri_unpack: F <- packed, upper triangle mirrored (KFAC_TRI_SYMMETRIC: the
 *                    reduced A, G) or zeroed (KFAC_TRI_LOWER: the L_A, L_G of a
 *                    sharded inversion, curvatures.py:391-398, after the gather). */
enum kfac_tri_mode { KFAC_TRI_SYMMETRIC = 0, KFAC_TRI_LOWER = 1 };

typedef struct kfac_tri_job {
  float* F;
  int64_t ldF;
  int32_t n;
  int32_t reserved;
  int64_t offset; /* elements into `packed` */
} kfac_tri_job;

KFAC_API int kfac_tri_pack(const kfac_tri_job* jobs, int njobs, float* packed, kfac_stream_t stream);
KFAC_API int kfac_tri_unpack(const kfac_tri_job* jobs, int njobs, const float* packed, int mode,
                             kfac_stream_t stream);

/* -------------------------------------------------------------- profiling
 * Optional HIP-event timing of the library's own launches, recorded on the
 * stream each kernel is launched on (off by default; not graph-capturable when
 * on).  One slot per kernel family, named as rocprofv3 names the kernels:
 *   0 kfac_factor_tiles_t (fp32-MFMA SYRK: row-major, LDS-DMA, register-staged conv),
 *   1 kfac_factor_reduce, 2 the whole invert call, 3 kfac_quad tiles,
 *   4 kfac_factor_syrk3 (bf16x3, split in the workgroup; largest n >= 2048),
 *   5 kfac_factor_tiles_x3 (bf16x3, split in registers; largest n >= 256),
 *   6 kfac_factor_conv (image-staged conv factors, both the im2col and the
 *     channel-major operand), 7 kfac_factor_channel_small (channel factors n <= 8),
 *   8 the whole kfac_syev call,
 *   9 kfac_factor_conv_x3 (im2col factors with n > 32, bf16x3 from an LDS im2col),
 *   10 kfac_factor_conv_x3s (im2col factors with 17 <= n <= 32, bf16x3 from
 *     column-shifted image copies),
 *   11 kfac_factor_conv_x3f (stride-1 im2col factors with 32 < n <= 160, bf16x3 from
 *     flattened column copies),
 *   12 kfac_factor_channel_x3 (channel-major factors with 8 < n <= 32, bf16x3 from
 *     fragments loaded straight from HBM).
 * kfac_profile_read syncs the recorded events.  kfac_profile_read_work also
 * returns the slot's algorithmic work: `work` = flops, for the factor slots (0, 4-7, 9-12)
 * sum_jobs K_rows * n (n + 1) (lower triangle incl. the diagonal, 2 flops per
 * product; curvatures.py:341-356); `bytes` = HBM bytes, for the factor slots each
 * operand read once (rows x cols x 4; an im2col operand: its images), for the syev
 * slot the tridiagonalisations' sum_k (n - k)^2 x 16 ~ 16 n^3 / 3 (n > 128). */
enum kfac_prof_id { KFAC_PROF_FACTOR_TILES = 0, KFAC_PROF_FACTOR_REDUCE = 1, KFAC_PROF_INVERT = 2,
                    KFAC_PROF_QUAD_TILES = 3, KFAC_PROF_FACTOR_SYRK3 = 4, KFAC_PROF_FACTOR_X3 = 5,
                    KFAC_PROF_FACTOR_CONV = 6, KFAC_PROF_FACTOR_CHANNEL_SMALL = 7, KFAC_PROF_SYEV = 8,
                    KFAC_PROF_FACTOR_CONV_X3 = 9, KFAC_PROF_FACTOR_CONV_X3S = 10,
                    KFAC_PROF_FACTOR_CONV_X3F = 11, KFAC_PROF_FACTOR_CHANNEL_X3 = 12, KFAC_PROF_COUNT = 13 };
KFAC_API int kfac_profile_enable(int on);
KFAC_API int kfac_profile_read(int id, double* total_ms, int64_t* launches);
KFAC_API int kfac_profile_read_work(int id, double* total_ms, int64_t* launches, double* work,
                                   double* bytes);
KFAC_API int kfac_profile_reset(void);

/* ------------------------------------------------------------------- misc */
/* KFAC.invert beside the next data pass (curvatures.py:367-398, overlapped), one call:
 * record `order` on `main`, make `side` wait for it, run kfac_invert_ex on `side`
 * (`inputs_read` recorded after the F-reading launch, may be NULL), copy the njobs
 * verdicts from `info` (device) to `info_host` (pinned host memory) and record `done`
 * on `side`.  Events come from kfac_event_create. */
KFAC_API int kfac_invert_pipelined(const kfac_invert_job* jobs, int njobs, void* workspace,
                                   size_t workspace_bytes, int32_t* info, int32_t* info_host,
                                   void* order, void* inputs_read, void* done, kfac_stream_t main,
                                   kfac_stream_t side);

/* Raw HIP events for the host side's stream ordering (no reference counterpart: the
 * reference is synchronous).  query: 1 complete, 0 pending, < 0 error. */
KFAC_API int kfac_event_create(void** event);
/* flags bit 0: ordering-only event (no system-scope fence when recorded / waited on):
 * for stream-to-stream order on one device, not for host reads after a sync. */
KFAC_API int kfac_event_create_ex(void** event, int flags);
KFAC_API int kfac_event_destroy(void* event);
KFAC_API int kfac_event_record(void* event, kfac_stream_t stream);
KFAC_API int kfac_stream_wait_event(kfac_stream_t stream, void* event);
KFAC_API int kfac_event_query(void* event);
KFAC_API int kfac_event_synchronize(void* event);

/* Release every HIP object the library keeps across calls (the inversion's cached
 * hipGraphs and their events, the profiling event pool), waiting for their last
 * use first.  Call before the HIP runtime shuts down (the Python binding registers
 * it with atexit); later calls simply rebuild what they need.  No reference
 * counterpart (the reference keeps no device state). */
KFAC_API int kfac_release(void);

/* Environment knobs, read once when the library is loaded.  get: any
 * knob's current value (KFAC_EINVAL for an unknown name).  set: only the per-call ones
 * (KFAC_INV_GRAPH, KFAC_INV_LOOKAHEAD, KFAC_EIG_G, KFAC_EIG_RB), between calls; the
 * kernel-selection knobs (KFAC_SYRK3, KFAC_TILES_X3, KFAC_CONV_*) are fixed at load. */
KFAC_API int kfac_set_knob(const char* name, int value);
KFAC_API int kfac_get_knob(const char* name, int* value);

KFAC_API const char* kfac_strerror(int status);
KFAC_API const char* kfac_version(void);

#ifdef __cplusplus
}
#endif
#endif /* KFAC_HIP_H */
