// Joint GLM predictive: the output covariance ACROSS the samples of a call.
//
// covariance.hip / covariance_outer.hip stop at the block diagonal (cov[b], nc x nc).  With
// rows r = b*nc + c, R = nb*nc, and T_r = K1^T M_r K2 as there,
//   cov[r][r'] = sum_jobs < T_r, T_r' >_F                                   (R x R),
// the function-space posterior over the call's inputs.  Two routes, one Gram body
// (cov_joint_gram_tile, covariance_common.h: a 64x64 tile ti >= tj of X X^T over one
// JSEG-long K segment, fp32 MFMA, four quadrants, fp32 partial):
//   kfac_kron_cov_joint        T by kfac_cov_apply_u / kfac_cov_apply_t (all rows of the
//                              call at once, as the per-sample call), then X = T_j
//                              (R x nA*nG):  cov = sum_j T_j T_j^T
//   kfac_kron_cov_outer_joint  Linear layers, no row formed: T_{b,c} = u_b v_{b,c}^T, so
//                              cov[r][r'] = sum_j S_j[b(r)][b(r')] * W_j[r][r'],
//                              S_j = U_j U_j^T (U = Abar K1, nb x nA: kfac_cov_outer_u),
//                              W_j = V_j V_j^T (V = Delta K2, R x nG: kfac_cov_outer_v);
//                              the Grams of U and V are task ranges of ONE launch.
//   reduce                     per output tile: the partials summed over segments in
//                              segment order, then over jobs in job order, in fp64; the
//                              lower element is written with its mirror.  No atomics.
// K is cut into segments [s*JSEG, (s+1)*JSEG) by K alone, and an element of a partial is
// one k-ordered fma chain over its two rows, so an entry of cov depends on its two rows,
// the factors and the job shapes only: not on nb, not on where the rows sit among the
// tiles.  The covariance of a subset of the samples has the bits of the whole's sub-blocks.
// Gram tasks are ordered (operand, segment, tile pair) and run in plain block order: the
// tile pairs of one segment, which share its row panels, are in flight together.
// nc has no cap here: rows are tiled, not classes.
#include "covariance_common.h"

namespace kfac {

constexpr int JMAXX = 2 * CMAXJ;   // Gram operands per call: T_j, or U_j and V_j
constexpr int JMAXT = 32768;       // row tiles: tile pairs (and tri_decode's products) fit 31 bits
constexpr int JRED = JTILE2 / NTHREADS;  // reduce blocks per tile

struct JointGramDev {
  const float* X;   // rows x K, K contiguous per row
  float* partial;   // [tile pair][segment][64 x 64]
  int64_t K;
  int rows, nseg, npairs, begin;  // begin: first task of this operand
};

struct JointArgs {
  int nx, njobs, nc, accumulate;
  int R, npairs;    // rows and tile pairs of cov
  int64_t ldc;
  float* cov;
  int end[JMAXX];
  JointGramDev x[JMAXX];
};
static_assert(sizeof(JointArgs) <= 4096, "kernel argument block");

// Gram partial: one tile pair of one operand over one K segment.
__global__ __launch_bounds__(NTHREADS) void kfac_cov_joint_gram(JointArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const JointGramDev& G = args.x[cov_find_job(args.end, args.nx, task)];
  const int local = task - G.begin;
  const int seg = local / G.npairs, pair = local - seg * G.npairs;
  int ti, tj;
  tri_decode(pair, ti, tj);
  const int64_t k0 = (int64_t)seg * JSEG;
  cov_joint_gram_tile(G.X, G.K, G.rows, ti, tj, k0, min(G.K, k0 + JSEG),
                      G.partial + ((int64_t)pair * G.nseg + seg) * JTILE2, lds);
}

// segments in order, fp64
__device__ __forceinline__ double joint_partial_sum(const JointGramDev& G, int pair, int e) {
  const float* part = G.partial + (int64_t)pair * G.nseg * JTILE2 + e;
  double s = 0.0;
  for (int i = 0; i < G.nseg; ++i) s += (double)part[(int64_t)i * JTILE2];
  return s;
}

// cov tile (ti >= tj) (+)= sum over jobs (in job order) of the segment sums; the lower
// element and its mirror are written.  FACTORED: job j's term is S_j[b][b'] * W_j[r][r']
// (operands 2j = U_j, 2j + 1 = V_j), else the sum of T_j's partials (operand j).
// Grid (tile pairs, JRED): a block owns four rows of the tile, a thread one element (one
// block per tile left most CUs idle on the MLP's 55 tiles).
template <bool FACTORED>
__device__ __forceinline__ void joint_reduce_tile(const JointArgs& args) {
  const int pair = blockIdx.x;
  int ti, tj;
  tri_decode(pair, ti, tj);
  const int nc = args.nc;
  const int e = blockIdx.y * NTHREADS + threadIdx.x;
  const int r = ti * TILE + (e >> 6), c = tj * TILE + (e & (TILE - 1));
  if (r >= args.R || c > r) return;
  double total = 0.0;
  if (FACTORED) {
    const int b = r / nc, b2 = c / nc;  // b >= b2
    const int tb = b >> 6, tb2 = b2 >> 6;
    const int spair = tb * (tb + 1) / 2 + tb2;
    const int se = (b & (TILE - 1)) * TILE + (b2 & (TILE - 1));
    for (int j = 0; j < args.njobs; ++j)
      total += joint_partial_sum(args.x[2 * j], spair, se) * joint_partial_sum(args.x[2 * j + 1], pair, e);
  } else {
    for (int j = 0; j < args.njobs; ++j) total += joint_partial_sum(args.x[j], pair, e);
  }
  float* lo = args.cov + (int64_t)r * args.ldc + c;
  const float v = args.accumulate ? (float)((double)*lo + total) : (float)total;
  *lo = v;
  args.cov[(int64_t)c * args.ldc + r] = v;
}

__global__ __launch_bounds__(NTHREADS) void kfac_cov_joint_reduce(JointArgs args) {
  joint_reduce_tile<false>(args);
}

__global__ __launch_bounds__(NTHREADS) void kfac_cov_outer_joint_reduce(JointArgs args) {
  joint_reduce_tile<true>(args);
}

// kfac_cov_rownorm's tile of (Abar K1)^T, stored instead of squared: U[b][i] (nb x nA) at
// OuterJobDev::norm.  A wave's quadrant holds 32 i x 32 b with b along the lanes.
__global__ __launch_bounds__(NTHREADS) void kfac_cov_outer_u(OuterArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const OuterJobDev& C = args.job[cov_find_job(args.n_end, args.njobs, task)];
  const int local = task - C.n_begin;
  const int i0 = (local / C.bt) * TILE, b0 = (local % C.bt) * TILE;
  const OpDev k1 = rowmajor_op(C.K1, C.nA, C.nA, C.ld1);
  const OpDev at = samplerows_op(C.a, C.cols, C.ones, (int)args.nb, C.lda);
  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  // U[i][b] = sum_k K1[k][i] abar[b][k]; K1 lower => k >= i0
  contract_tile<KFAC_ROWMAJOR, KFAC_SAMPLEROWS>(k1, i0, at, b0, C.lower1 ? i0 : 0, C.nA, false, true,
                                                lds, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = b0 + (wave & 1) * 32 + (lane & 31);
  if (b >= args.nb) return;
  float* dst = C.norm + b * C.nA;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int i = i0 + (wave >> 1) * 32 + acc_row(v, lane);
    if (i < C.nA) dst[i] = acc[v];
  }
}

// The U launch alone (kfac_glm_draws_outer contracts U with the draws, not with itself).
int cov_launch_outer_u(const OuterArgs& args, int64_t nn, hipStream_t s) {
  hipLaunchKernelGGL(kfac_cov_outer_u, dim3((unsigned)nn), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

static int64_t joint_nseg(int64_t K) { return cdiv(K, JSEG); }
static int64_t joint_npairs(int64_t rows) {
  const int64_t t = cdiv(rows, TILE);
  return t * (t + 1) / 2;
}
static size_t joint_partial_bytes(int64_t rows, int64_t K) {
  return align_up((size_t)(joint_npairs(rows) * joint_nseg(K)) * JTILE2 * sizeof(float), 256);
}
// R = nb*nc with 32-bit rows and at most JMAXT row tiles, or 0
static int64_t joint_rows(int64_t nb, int nc) {
  if (nb <= 0 || nc <= 0 || nb > (int64_t)JMAXT * TILE / nc) return 0;
  return nb * nc;
}

// operand x of the Gram launch; false: its tasks do not fit 31 bits
static bool joint_add_operand(JointArgs& a, int64_t rows, int64_t K, int64_t& ntasks) {
  JointGramDev& g = a.x[a.nx];
  g.K = K;
  g.rows = (int)rows;
  g.nseg = (int)joint_nseg(K);
  g.npairs = (int)joint_npairs(rows);
  g.begin = (int)ntasks;
  if (joint_nseg(K) >= ((int64_t)1 << 31) / joint_npairs(rows)) return false;
  ntasks += joint_npairs(rows) * joint_nseg(K);
  if (ntasks >= (int64_t)1 << 31) return false;
  a.end[a.nx++] = (int)ntasks;
  return true;
}

}  // namespace kfac

using namespace kfac;

extern "C" size_t kfac_kron_cov_joint_workspace_bytes(const kfac_cov_job* jobs, int njobs, int64_t nb,
                                                      int nc) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ) return 0;
  const int64_t R = joint_rows(nb, nc);
  if (!R) return 0;
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) {
    if (jobs[i].nA <= 0 || jobs[i].nG <= 0) return 0;
    total += 2 * cov_t_bytes(jobs[i], R) + joint_partial_bytes(R, (int64_t)jobs[i].nA * jobs[i].nG);
  }
  return total;
}

extern "C" int kfac_kron_cov_joint(const kfac_cov_job* jobs, int njobs, int64_t nb, int nc,
                                   int accumulate, float* cov, int64_t ldc, void* workspace,
                                   size_t workspace_bytes, kfac_stream_t stream) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ || !cov) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!cov_job_ok(jobs[i])) return KFAC_EINVAL;
  const int64_t R = joint_rows(nb, nc);
  if (!R || ldc < R) return KFAC_EINVAL;
  CovArgs ap{};
  JointArgs args{};
  ap.njobs = args.njobs = njobs;
  ap.nc = args.nc = nc;
  ap.nb = nb;
  args.accumulate = accumulate;
  args.R = (int)R;
  args.npairs = (int)joint_npairs(R);
  args.ldc = ldc;
  args.cov = cov;
  if (!cov_fill_apply(jobs, njobs, R, ap)) return KFAC_EINVAL;
  int64_t ng = 0;
  for (int i = 0; i < njobs; ++i)
    if (!joint_add_operand(args, R, (int64_t)jobs[i].nA * jobs[i].nG, ng)) return KFAC_EINVAL;
  if (!workspace || workspace_bytes < kfac_kron_cov_joint_workspace_bytes(jobs, njobs, nb, nc))
    return KFAC_EWORKSPACE;
  char* ws = (char*)workspace;
  for (int i = 0; i < njobs; ++i) {
    CovJobDev& d = ap.job[i];
    const size_t tb = cov_t_bytes(jobs[i], R);
    d.U = reinterpret_cast<float*>(ws); ws += tb;
    d.T = reinterpret_cast<float*>(ws); ws += tb;
    args.x[i].X = d.T;
    args.x[i].partial = reinterpret_cast<float*>(ws);
    ws += joint_partial_bytes(R, args.x[i].K);
  }
  hipStream_t s = (hipStream_t)stream;
  const int rc = cov_launch_apply(ap, s);
  if (rc != KFAC_OK) return rc;
  hipLaunchKernelGGL(kfac_cov_joint_gram, dim3((unsigned)ng), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_cov_joint_reduce, dim3((unsigned)args.npairs, JRED), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

extern "C" size_t kfac_kron_cov_outer_joint_workspace_bytes(const kfac_cov_outer_job* jobs, int njobs,
                                                            int64_t nb, int nc) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ) return 0;
  const int64_t R = joint_rows(nb, nc);
  if (!R) return 0;
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) {
    if (jobs[i].cols <= 0 || jobs[i].nG <= 0) return 0;
    total += outer_u_bytes(jobs[i], nb) + outer_v_bytes(jobs[i], R) +
             joint_partial_bytes(nb, outer_nA(jobs[i])) + joint_partial_bytes(R, jobs[i].nG);
  }
  return total;
}

extern "C" int kfac_kron_cov_outer_joint(const kfac_cov_outer_job* jobs, int njobs, int64_t nb, int nc,
                                         int accumulate, float* cov, int64_t ldc, void* workspace,
                                         size_t workspace_bytes, kfac_stream_t stream) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ || !cov) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!outer_job_ok(jobs[i])) return KFAC_EINVAL;
  const int64_t R = joint_rows(nb, nc);
  if (!R || ldc < R) return KFAC_EINVAL;
  OuterArgs op{};
  JointArgs args{};
  op.njobs = args.njobs = njobs;
  op.nc = args.nc = nc;
  op.nb = nb;
  args.accumulate = accumulate;
  args.R = (int)R;
  args.npairs = (int)joint_npairs(R);
  args.ldc = ldc;
  args.cov = cov;
  int64_t nn = 0, nv = 0, ng = 0;
  if (!cov_fill_outer(jobs, njobs, nb, R, op, nn, nv)) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!joint_add_operand(args, nb, op.job[i].nA, ng) || !joint_add_operand(args, R, jobs[i].nG, ng))
      return KFAC_EINVAL;
  if (!workspace || workspace_bytes < kfac_kron_cov_outer_joint_workspace_bytes(jobs, njobs, nb, nc))
    return KFAC_EWORKSPACE;
  char* ws = (char*)workspace;
  for (int i = 0; i < njobs; ++i) {
    OuterJobDev& d = op.job[i];
    d.norm = reinterpret_cast<float*>(ws); ws += outer_u_bytes(jobs[i], nb);  // U, nb x nA
    d.V = reinterpret_cast<float*>(ws); ws += outer_v_bytes(jobs[i], R);
    args.x[2 * i].X = d.norm;
    args.x[2 * i].partial = reinterpret_cast<float*>(ws); ws += joint_partial_bytes(nb, d.nA);
    args.x[2 * i + 1].X = d.V;
    args.x[2 * i + 1].partial = reinterpret_cast<float*>(ws); ws += joint_partial_bytes(R, d.nG);
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(kfac_cov_outer_u, dim3((unsigned)nn), dim3(NTHREADS), 0, s, op);
  KFAC_CHECK_LAUNCH();
  const int rc = cov_launch_outer_v(op, nv, s);
  if (rc != KFAC_OK) return rc;
  hipLaunchKernelGGL(kfac_cov_joint_gram, dim3((unsigned)ng), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_cov_outer_joint_reduce, dim3((unsigned)args.npairs, JRED), dim3(NTHREADS), 0,
                     s, args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}
