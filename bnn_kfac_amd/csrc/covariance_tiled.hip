// GLM predictive for any number of outputs: the per-sample covariance with the CLASSES tiled.
//
// covariance.hip / covariance_outer.hip hold a sample's nc x nc block in one 32x32 MFMA
// quadrant (nc <= 32).  Here a sample's block is cut into 64x64 class tiles, ntile =
// ceil(nc / 64), and every tile pair ti >= tj goes through the joint call's Gram body
// (cov_joint_gram_tile, covariance_common.h) on that sample's rows alone:
//   kfac_kron_cov_tiled        T by kfac_cov_apply_u / kfac_cov_apply_t (all nb*nc rows of the
//                              call at once, unchanged), then per sample X_b = T_j + b*nc*K
//                              (nc x K, K = nA*nG):  cov[b] = sum_j X_b X_b^T
//   kfac_kron_cov_outer_tiled  Linear layers, no row formed: s_j[b] by kfac_cov_rownorm and
//                              V = Delta K2 by kfac_cov_outer_v (both unchanged), then
//                              X_b = V_j + b*nc*nG (nc x nG):  cov[b] = sum_j s_j[b] X_b X_b^T
//   gram                       one task per (job, sample b, K segment, tile pair): a 64x64
//                              fp32 partial at [b][pair][segment]
//   reduce                     per (sample, tile pair): the partials summed over segments in
//                              segment order, (outer: times s_j[b], its column-tile partials
//                              summed in tile order,) then over jobs in job order, all in
//                              fp64; the lower element is written with its mirror into
//                              cov[b] (nc x nc contiguous).  No atomics.
// K is cut into segments [s*JSEG, (s+1)*JSEG) by K alone, and an element of a partial is one
// k-ordered fma chain over its two rows, so a block depends on its sample's rows, the
// factors and the job shapes only: chunking the samples changes no bit, two calls give
// identical bits, every block is bitwise symmetric.  The dense route shares the Gram body,
// the segmentation and the reduce order with kfac_kron_cov_joint: block b has exactly the
// bits of the joint call's block (b, b) on the same jobs.
// Gram tasks are ordered (job, sample, segment, tile pair) and run in plain block order: the
// tile pairs of one sample and segment, which share its row panels, are in flight together
// (covariance_joint.hip's reasoning for its own order).
#include "covariance_common.h"

namespace kfac {

struct TiledGramDev {
  const float* X;     // nb*nc x K, K contiguous per row
  float* partial;     // [sample][tile pair][segment][64 x 64]
  const float* norm;  // outer: at x nb column-tile partials of s_j[b]
  int64_t K;
  int nseg, at, begin;  // begin: first task of this job
};

struct TiledArgs {
  int njobs, nc, accumulate, npairs;
  int64_t nb;
  float* cov;
  int end[CMAXJ];
  TiledGramDev x[CMAXJ];
};
static_assert(sizeof(TiledArgs) <= 4096, "kernel argument block");

// Gram partial: one tile pair of one sample of one job over one K segment.
__global__ __launch_bounds__(NTHREADS) void kfac_cov_tiled_gram(TiledArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const TiledGramDev& G = args.x[cov_find_job(args.end, args.njobs, task)];
  const int local = task - G.begin;
  const int bs = local / args.npairs, pair = local - bs * args.npairs;
  const int64_t b = bs / G.nseg;
  const int seg = bs - (int)b * G.nseg;
  int ti, tj;
  tri_decode(pair, ti, tj);
  const int64_t k0 = (int64_t)seg * JSEG;
  cov_joint_gram_tile(G.X + b * args.nc * G.K, G.K, args.nc, ti, tj, k0, min(G.K, k0 + JSEG),
                      G.partial + ((b * args.npairs + pair) * G.nseg + seg) * JTILE2, lds);
}

// cov[b] tile (ti >= tj) (+)= sum over jobs (in job order) of the segment sums (in segment
// order), fp64; OUTER: job j's sum times s_j[b].  Grid (nb * tile pairs, JTILE2 / NTHREADS):
// a block owns four rows of the tile, a thread one element, as the joint reduce.
template <bool OUTER>
__device__ __forceinline__ void tiled_reduce_tile(const TiledArgs& args) {
  __shared__ double scale[CMAXJ];
  const int64_t b = blockIdx.x / args.npairs;
  const int pair = blockIdx.x - (int)b * args.npairs;
  if (OUTER) {
    if ((int)threadIdx.x < args.njobs) {
      const TiledGramDev& G = args.x[threadIdx.x];
      double s = 0.0;
      for (int t = 0; t < G.at; ++t) s += (double)G.norm[(int64_t)t * args.nb + b];
      scale[threadIdx.x] = s;
    }
    __syncthreads();
  }
  int ti, tj;
  tri_decode(pair, ti, tj);
  const int nc = args.nc;
  const int e = blockIdx.y * NTHREADS + threadIdx.x;
  const int r = ti * TILE + (e >> 6), c = tj * TILE + (e & (TILE - 1));
  if (r >= nc || c > r) return;
  double total = 0.0;
  for (int j = 0; j < args.njobs; ++j) {
    const TiledGramDev& G = args.x[j];
    const float* part = G.partial + (b * args.npairs + pair) * G.nseg * JTILE2 + e;
    double s = 0.0;
    for (int i = 0; i < G.nseg; ++i) s += (double)part[(int64_t)i * JTILE2];
    total += OUTER ? scale[j] * s : s;
  }
  float* cov = args.cov + b * nc * nc;
  float* lo = cov + (int64_t)r * nc + c;
  const float v = args.accumulate ? (float)((double)*lo + total) : (float)total;
  *lo = v;
  cov[(int64_t)c * nc + r] = v;
}

__global__ __launch_bounds__(NTHREADS) void kfac_cov_tiled_reduce(TiledArgs args) {
  tiled_reduce_tile<false>(args);
}

__global__ __launch_bounds__(NTHREADS) void kfac_cov_outer_tiled_reduce(TiledArgs args) {
  tiled_reduce_tile<true>(args);
}

static size_t tiled_partial_bytes(int64_t nb, int nc, int64_t K) {
  return align_up((size_t)(nb * tiled_npairs(nc) * cdiv(K, JSEG)) * JTILE2 * sizeof(float), 256);
}

// job i of the Gram launch: nb samples x segments x tile pairs; false: the tasks (and with
// them the reduce's nb * tile pairs blocks) do not fit 31 bits
static bool tiled_add_job(TiledArgs& a, int i, int64_t K, int64_t& ntasks) {
  const int64_t lim = (int64_t)1 << 31;
  TiledGramDev& g = a.x[i];
  const int64_t nseg = cdiv(K, JSEG);
  g.K = K;
  g.nseg = (int)nseg;
  g.begin = (int)ntasks;
  if (nseg >= lim / a.npairs || a.nb >= lim / (nseg * a.npairs)) return false;
  ntasks += a.nb * nseg * a.npairs;
  if (ntasks >= lim) return false;
  a.end[i] = (int)ntasks;
  return true;
}

template <bool OUTER>
static int tiled_launch_gram_reduce(const TiledArgs& args, int64_t ng, hipStream_t s) {
  hipLaunchKernelGGL(kfac_cov_tiled_gram, dim3((unsigned)ng), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  const dim3 grid((unsigned)(args.nb * args.npairs), JTILE2 / NTHREADS);
  if (OUTER)
    hipLaunchKernelGGL(kfac_cov_outer_tiled_reduce, grid, dim3(NTHREADS), 0, s, args);
  else
    hipLaunchKernelGGL(kfac_cov_tiled_reduce, grid, dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

}  // namespace kfac

using namespace kfac;

extern "C" size_t kfac_kron_cov_tiled_workspace_bytes(const kfac_cov_job* jobs, int njobs, int64_t nb,
                                                      int nc) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ) return 0;
  const int64_t rows = tiled_rows(nb, nc);
  if (!rows) return 0;
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) {
    if (jobs[i].nA <= 0 || jobs[i].nG <= 0) return 0;
    total += 2 * cov_t_bytes(jobs[i], rows) + tiled_partial_bytes(nb, nc, (int64_t)jobs[i].nA * jobs[i].nG);
  }
  return total;
}

extern "C" int kfac_kron_cov_tiled(const kfac_cov_job* jobs, int njobs, int64_t nb, int nc,
                                   int accumulate, float* cov, void* workspace, size_t workspace_bytes,
                                   kfac_stream_t stream) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ || !cov) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!cov_job_ok(jobs[i])) return KFAC_EINVAL;
  const int64_t rows = tiled_rows(nb, nc);
  if (!rows) return KFAC_EINVAL;
  CovArgs ap{};
  TiledArgs args{};
  ap.njobs = args.njobs = njobs;
  ap.nc = args.nc = nc;
  ap.nb = args.nb = nb;
  args.accumulate = accumulate;
  args.npairs = (int)tiled_npairs(nc);
  args.cov = cov;
  if (!cov_fill_apply(jobs, njobs, rows, ap)) return KFAC_EINVAL;
  int64_t ng = 0;
  for (int i = 0; i < njobs; ++i)
    if (!tiled_add_job(args, i, (int64_t)jobs[i].nA * jobs[i].nG, ng)) return KFAC_EINVAL;
  if (!workspace || workspace_bytes < kfac_kron_cov_tiled_workspace_bytes(jobs, njobs, nb, nc))
    return KFAC_EWORKSPACE;
  char* ws = (char*)workspace;
  for (int i = 0; i < njobs; ++i) {
    CovJobDev& d = ap.job[i];
    const size_t tb = cov_t_bytes(jobs[i], rows);
    d.U = reinterpret_cast<float*>(ws); ws += tb;
    d.T = reinterpret_cast<float*>(ws); ws += tb;
    args.x[i].X = d.T;
    args.x[i].partial = reinterpret_cast<float*>(ws);
    ws += tiled_partial_bytes(nb, nc, args.x[i].K);
  }
  hipStream_t s = (hipStream_t)stream;
  const int rc = cov_launch_apply(ap, s);
  if (rc != KFAC_OK) return rc;
  return tiled_launch_gram_reduce<false>(args, ng, s);
}

extern "C" size_t kfac_kron_cov_outer_tiled_workspace_bytes(const kfac_cov_outer_job* jobs, int njobs,
                                                            int64_t nb, int nc) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ) return 0;
  const int64_t rows = tiled_rows(nb, nc);
  if (!rows) return 0;
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) {
    if (jobs[i].cols <= 0 || jobs[i].nG <= 0) return 0;
    total += outer_norm_bytes(jobs[i], nb) + outer_v_bytes(jobs[i], rows) +
             tiled_partial_bytes(nb, nc, jobs[i].nG);
  }
  return total;
}

extern "C" int kfac_kron_cov_outer_tiled(const kfac_cov_outer_job* jobs, int njobs, int64_t nb, int nc,
                                         int accumulate, float* cov, void* workspace,
                                         size_t workspace_bytes, kfac_stream_t stream) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ || !cov) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!outer_job_ok(jobs[i])) return KFAC_EINVAL;
  const int64_t rows = tiled_rows(nb, nc);
  if (!rows) return KFAC_EINVAL;
  OuterArgs op{};
  TiledArgs args{};
  op.njobs = args.njobs = njobs;
  op.nc = args.nc = nc;
  op.nb = args.nb = nb;
  args.accumulate = accumulate;
  args.npairs = (int)tiled_npairs(nc);
  args.cov = cov;
  int64_t nn = 0, nv = 0, ng = 0;
  if (!cov_fill_outer(jobs, njobs, nb, rows, op, nn, nv)) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!tiled_add_job(args, i, jobs[i].nG, ng)) return KFAC_EINVAL;
  if (!workspace || workspace_bytes < kfac_kron_cov_outer_tiled_workspace_bytes(jobs, njobs, nb, nc))
    return KFAC_EWORKSPACE;
  char* ws = (char*)workspace;
  for (int i = 0; i < njobs; ++i) {
    OuterJobDev& d = op.job[i];
    d.norm = reinterpret_cast<float*>(ws); ws += outer_norm_bytes(jobs[i], nb);
    d.V = reinterpret_cast<float*>(ws); ws += outer_v_bytes(jobs[i], rows);
    args.x[i].X = d.V;
    args.x[i].norm = d.norm;
    args.x[i].at = d.at;
    args.x[i].partial = reinterpret_cast<float*>(ws);
    ws += tiled_partial_bytes(nb, nc, d.nG);
  }
  hipStream_t s = (hipStream_t)stream;
  int rc = cov_launch_rownorm(op, nn, s);
  if (rc != KFAC_OK) return rc;
  rc = cov_launch_outer_v(op, nv, s);
  if (rc != KFAC_OK) return rc;
  return tiled_launch_gram_reduce<true>(args, ng, s);
}
