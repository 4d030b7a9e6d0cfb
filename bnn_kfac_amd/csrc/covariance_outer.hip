// Factored GLM predictive: a Linear layer's output covariance without its Jacobian rows.
//
// A Linear layer's Jacobian row is rank one: with abar_b = [a_b | 1] the layer's input
// and delta_{b,c} = d f_c(x_b) / d z at the layer's output z, M_{b,c} = abar_b delta_{b,c}^T,
// so T_{b,c} = K1^T M_{b,c} K2 = (K1^T abar_b)(K2^T delta_{b,c})^T and
//   cov[b][c][c'] = sum_jobs s_j[b] * (V_{j,b} V_{j,b}^T)[c][c'] ,
//   s_j[b] = || K1_j^T abar_{j,b} ||^2 ,   V_{j,b} = Delta_{j,b} K2_j   (nc x nG).
// Per call (<= 8 jobs, nb samples, nc <= 32):
//   rownorm: 64x64 tiles of Abar K1 (nb x nA by nA x nA) on contract_tile's fp32 MFMA
//            (exact fp32 products); the product is NOT written: the epilogue squares the
//            tile and sums it over its 64 columns into partial [job][column tile][b].
//            The ones column of abar is synthesised by the panel loader (OpDev::ones).
//            A lower-triangular K1 leaves column tile i0 the K-range [i0, nA).
//   v      : V = Delta K2, kfac_cov_apply_t's tile (covariance_common.h) over the
//            (nb*nc x nG) matrix of the delta rows
//   gram   : V_b V_b^T, kfac_cov_gram's segment with K = nG
//   reduce : per sample, each job's gram partials summed over segments and multiplied by
//            s_j[b] (its column-tile partials summed in tile order in fp64), then summed
//            over jobs in job order, all in fp64; the lower triangle is mirrored.
// No atomics: two calls give identical bits, a sample's block depends on that sample
// only, and every block is bitwise symmetric.
// Rownorm tasks are ordered column-tile major, heaviest first, and run in plain block
// order (covariance.hip's finding: per-XCD ranges put the long tiles on one XCD).
//
// kfac_kron_cov_outer_sweep (end of this file): up to 64 dampings at once in the factors'
// eigenbasis.  The projections abar V_A and Delta V_G run once (K1 = V_A, K2 = V_G, dense);
// kfac_cov_rownorm_w weights the squares per grid point in its epilogue, and
// kfac_cov_outer_sweep_gram / _reduce form Q_b diag(wG) Q_b^T per grid point.
#include "covariance_common.h"

namespace kfac {

// One 64 (columns i of K1) x 64 (samples b) tile of (Abar K1)^T, squared and summed over
// i: norm[tile i][b].  A wave's quadrant holds 32 i x 32 b with b along the lanes, so a
// lane sums its 16 registers, adds the other half-wave's, and the two waves that share
// the samples are added through LDS: one fixed order.
__global__ __launch_bounds__(NTHREADS) void kfac_cov_rownorm(OuterArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const OuterJobDev& C = args.job[cov_find_job(args.n_end, args.njobs, task)];
  const int local = task - C.n_begin;
  const int ti = local / C.bt;
  const int i0 = ti * TILE, b0 = (local % C.bt) * TILE;
  const OpDev k1 = rowmajor_op(C.K1, C.nA, C.nA, C.ld1);
  const OpDev at = samplerows_op(C.a, C.cols, C.ones, (int)args.nb, C.lda);
  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  // U[i][b] = sum_k K1[k][i] abar[b][k]; K1 lower => k >= i0
  contract_tile<KFAC_ROWMAJOR, KFAC_SAMPLEROWS>(k1, i0, at, b0, C.lower1 ? i0 : 0, C.nA, false, true,
                                                lds, acc);
  // (contract_tile leaves through a barrier: lds is free; columns i >= nA are zero)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float s = 0.f;
#pragma unroll
  for (int v = 0; v < 16; ++v) s += acc[v] * acc[v];
  s += __shfl_xor(s, 32);
  if (lane < 32) lds[wave * 32 + lane] = s;
  __syncthreads();
  if (threadIdx.x < TILE) {
    const int qj = threadIdx.x >> 5, j = threadIdx.x & 31;
    const int64_t b = b0 + qj * 32 + j;
    // waves (qi, qj) = (0, qj) and (1, qj)
    if (b < args.nb) C.norm[(int64_t)ti * args.nb + b] = lds[qj * 32 + j] + lds[(2 + qj) * 32 + j];
  }
}

__global__ __launch_bounds__(NTHREADS) void kfac_cov_outer_v(OuterArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const OuterJobDev& C = args.job[cov_find_job(args.v_end, args.njobs, task)];
  const int local = task - C.v_begin;
  cov_times_k2_tile(C.D, C.ldD, C.vrows, C.nG, C.K2, C.ld2, C.lower2, (local / C.tg) * TILE,
                    (local % C.tg) * TILE, C.V, lds);
}

__global__ __launch_bounds__(NTHREADS) void kfac_cov_outer_gram(OuterArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const OuterJobDev& C = args.job[cov_find_job(args.g_end, args.njobs, task)];
  const int64_t local = task - C.g_begin;
  const int64_t b = local / C.nseg;
  const int seg = (int)(local % C.nseg);
  const int nc = args.nc;
  const int64_t K = C.nG;
  const int64_t k0 = (int64_t)seg * GSEG;
  cov_gram_segment(C.V + b * nc * K, K, nc, k0, min(K, k0 + GSEG), C.partial + local * nc * nc, lds);
}

// cov[b] (+)= sum over jobs (in job order) of s_j[b] * (segment partials in segment
// order), fp64; s_j[b] = its column-tile partials in tile order, fp64.
__global__ __launch_bounds__(NTHREADS) void kfac_cov_outer_reduce(OuterArgs args) {
  __shared__ double scale[CMAXJ];
  const int64_t b = blockIdx.x;
  const int nc = args.nc, n2 = nc * nc;
  if ((int)threadIdx.x < args.njobs) {
    const OuterJobDev& C = args.job[threadIdx.x];
    double s = 0.0;
    for (int t = 0; t < C.at; ++t) s += (double)C.norm[(int64_t)t * args.nb + b];
    scale[threadIdx.x] = s;
  }
  __syncthreads();
  float* cov = args.cov + b * n2;
  for (int e = threadIdx.x; e < n2; e += NTHREADS) {
    const int c = e / nc, c2 = e - c * nc;
    if (c2 > c) continue;
    double total = 0.0;
    for (int j = 0; j < args.njobs; ++j) {
      const OuterJobDev& C = args.job[j];
      const float* part = C.partial + b * C.nseg * n2 + e;
      double s = 0.0;
      for (int i = 0; i < C.nseg; ++i) s += (double)part[(int64_t)i * n2];
      total += scale[j] * s;
    }
    const float v = args.accumulate ? (float)((double)cov[e] + total) : (float)total;
    cov[e] = v;
    cov[c2 * nc + c] = v;
  }
}

// ---- damping sweep (kfac_kron_cov_outer_sweep): K1 = V_A, K2 = V_G (dense), the
// projections p = V_A^T abar and Q = Delta V_G once, then per grid point tau
//   cov_tau[b] = sum_jobs (sum_i wA_tau[i] p_b[i]^2) * Q_b diag(wG_tau) Q_b^T .
constexpr int RNTG = 16;  // grid points per cross-wave sum of the weighted row norm
static_assert(SMAXT * TILE + RNTG * 4 * 32 <= 4 * PANEL, "weights + wave sums fit the staging buffer");

// kfac_cov_rownorm's tile with a weighted epilogue: norm[tau][tile i][b] =
// sum_{i in tile} wA_tau[i] * (abar_b V_A)[i]^2 for every tau, the tile's ntau x 64
// weights staged in LDS (0 past nA); per tau the sums run in kfac_cov_rownorm's order.
__global__ __launch_bounds__(NTHREADS) void kfac_cov_rownorm_w(OuterArgs args, SweepArgs sw) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const int jb = cov_find_job(args.n_end, args.njobs, task);
  const OuterJobDev& C = args.job[jb];
  const SweepWeights& W = sw.job[jb];
  const int local = task - C.n_begin;
  const int ti = local / C.bt;
  const int i0 = ti * TILE, b0 = (local % C.bt) * TILE;
  const OpDev k1 = rowmajor_op(C.K1, C.nA, C.nA, C.ld1);
  const OpDev at = samplerows_op(C.a, C.cols, C.ones, (int)args.nb, C.lda);
  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  contract_tile<KFAC_ROWMAJOR, KFAC_SAMPLEROWS>(k1, i0, at, b0, 0, C.nA, false, true, lds, acc);
  // (contract_tile leaves through a barrier: lds is free; columns i >= nA are zero)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ntau = sw.ntau;
  float* red = lds + SMAXT * TILE;
  for (int e = tid; e < ntau * TILE; e += NTHREADS) {
    const int i = i0 + (e & (TILE - 1));
    const float w = W.wA[(int64_t)(e >> 6) * W.ldwA + min(i, C.nA - 1)];
    lds[e] = i < C.nA ? w : 0.f;
  }
  __syncthreads();
  float sq[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) sq[v] = acc[v] * acc[v];
  const int wrow = (wave >> 1) * 32 + 4 * (lane >> 5);  // + acc_row's (v & 3) + 8 * (v >> 2)
  for (int t0 = 0; t0 < ntau; t0 += RNTG) {
    const int ng = min(RNTG, ntau - t0);
    for (int t = 0; t < ng; ++t) {
      const float* w = lds + (t0 + t) * TILE + wrow;
      float s = 0.f;
#pragma unroll
      for (int v = 0; v < 16; ++v) s += w[(v & 3) + 8 * (v >> 2)] * sq[v];
      s += __shfl_xor(s, 32);
      if (lane < 32) red[t * 128 + wave * 32 + lane] = s;
    }
    __syncthreads();
    for (int e = tid; e < ng * TILE; e += NTHREADS) {
      const int t = e >> 6, x = e & (TILE - 1), qj = x >> 5, j = x & 31;
      const int64_t b = b0 + x;
      // waves (qi, qj) = (0, qj) and (1, qj)
      if (b < args.nb)
        C.norm[((int64_t)(t0 + t) * C.at + ti) * args.nb + b] =
            red[t * 128 + qj * 32 + j] + red[t * 128 + (2 + qj) * 32 + j];
    }
    __syncthreads();
  }
}

// Weighted Gram partials of Q_b over one WSEG-long segment of nG, every tau.
__global__ __launch_bounds__(NTHREADS) void kfac_cov_outer_sweep_gram(OuterArgs args, SweepArgs sw) {
  __shared__ __attribute__((aligned(16))) float lds[WGRAM_LDS];
  const int task = blockIdx.x;
  const int jb = cov_find_job(args.g_end, args.njobs, task);
  const OuterJobDev& C = args.job[jb];
  const int64_t local = task - C.g_begin;
  const int64_t b = local / C.nseg;
  const int seg = (int)(local % C.nseg);
  const int nc = args.nc;
  const int64_t K = C.nG;
  cov_wgram_segment<WGRAM_VECTOR>(C.V + b * nc * K, K, nc, (int64_t)seg * WSEG, sw.job[jb], C.nG, sw.ntau,
                           C.partial + local * nc * nc, args.nb * C.nseg * nc * nc, lds);
}

// cov[tau][b] (+)= kfac_cov_outer_reduce's sum over tau's norms and partials; grid (nb, ntau).
__global__ __launch_bounds__(NTHREADS) void kfac_cov_outer_sweep_reduce(OuterArgs args) {
  __shared__ double scale[CMAXJ];
  const int64_t b = blockIdx.x, tau = blockIdx.y;
  const int nc = args.nc, n2 = nc * nc;
  if ((int)threadIdx.x < args.njobs) {
    const OuterJobDev& C = args.job[threadIdx.x];
    double s = 0.0;
    for (int t = 0; t < C.at; ++t) s += (double)C.norm[(tau * C.at + t) * args.nb + b];
    scale[threadIdx.x] = s;
  }
  __syncthreads();
  float* cov = args.cov + (tau * args.nb + b) * n2;
  for (int e = threadIdx.x; e < n2; e += NTHREADS) {
    const int c = e / nc, c2 = e - c * nc;
    if (c2 > c) continue;
    double total = 0.0;
    for (int j = 0; j < args.njobs; ++j) {
      const OuterJobDev& C = args.job[j];
      const float* part = C.partial + (tau * args.nb + b) * C.nseg * n2 + e;
      double s = 0.0;
      for (int i = 0; i < C.nseg; ++i) s += (double)part[(int64_t)i * n2];
      total += scale[j] * s;
    }
    const float v = args.accumulate ? (float)((double)cov[e] + total) : (float)total;
    cov[e] = v;
    cov[c2 * nc + c] = v;
  }
}

// The row-norm launch alone (kfac_kron_cov_outer_tiled forms its own Grams from V).
int cov_launch_rownorm(const OuterArgs& args, int64_t nn, hipStream_t s) {
  hipLaunchKernelGGL(kfac_cov_rownorm, dim3((unsigned)nn), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

// The weighted row-norm launch alone (kfac_kron_cov_outer_sweep_tiled forms its own Grams).
int cov_launch_rownorm_w(const OuterArgs& args, const SweepArgs& sw, int64_t nn, hipStream_t s) {
  hipLaunchKernelGGL(kfac_cov_rownorm_w, dim3((unsigned)nn), dim3(NTHREADS), 0, s, args, sw);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

// The V launch alone (kfac_kron_cov_outer_joint forms its own Grams from U and V).
int cov_launch_outer_v(const OuterArgs& args, int64_t nv, hipStream_t s) {
  hipLaunchKernelGGL(kfac_cov_outer_v, dim3((unsigned)nv), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

static int64_t outer_nseg(const kfac_cov_outer_job& j) { return cdiv(j.nG, GSEG); }
static size_t outer_partial_bytes(const kfac_cov_outer_job& j, int64_t nb, int nc) {
  return align_up((size_t)(nb * outer_nseg(j)) * nc * nc * sizeof(float), 256);
}
}  // namespace kfac

using namespace kfac;

extern "C" size_t kfac_kron_cov_outer_workspace_bytes(const kfac_cov_outer_job* jobs, int njobs,
                                                      int64_t nb, int nc) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ || nb <= 0 || nc <= 0 || nc > CMAXC) return 0;
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) {
    if (jobs[i].cols <= 0 || jobs[i].nG <= 0) return 0;
    total += outer_norm_bytes(jobs[i], nb) + outer_v_bytes(jobs[i], nb * nc) +
             outer_partial_bytes(jobs[i], nb, nc);
  }
  return total;
}

extern "C" int kfac_kron_cov_outer(const kfac_cov_outer_job* jobs, int njobs, int64_t nb, int nc,
                                   int accumulate, float* cov, void* workspace,
                                   size_t workspace_bytes, kfac_stream_t stream) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ || nb <= 0 || nc <= 0 || nc > CMAXC || !cov)
    return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!outer_job_ok(jobs[i])) return KFAC_EINVAL;
  const int64_t lim = (int64_t)1 << 31;
  // samples and delta rows are indexed with 32-bit columns: nb*nc (and with it every
  // launch's task count) stays below 2^31
  if (nb >= (lim - TILE) / nc) return KFAC_EINVAL;
  const int64_t rows = nb * nc;
  OuterArgs args{};
  args.njobs = njobs;
  args.nc = nc;
  args.accumulate = accumulate;
  args.nb = nb;
  args.cov = cov;
  int64_t nn = 0, nv = 0, ng = 0;
  if (!cov_fill_outer(jobs, njobs, nb, rows, args, nn, nv)) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i) {
    OuterJobDev& d = args.job[i];
    d.nseg = (int)outer_nseg(jobs[i]);
    d.g_begin = (int)ng;
    ng += nb * d.nseg;
    if (ng >= lim) return KFAC_EINVAL;
    args.g_end[i] = (int)ng;
  }
  if (!workspace || workspace_bytes < kfac_kron_cov_outer_workspace_bytes(jobs, njobs, nb, nc))
    return KFAC_EWORKSPACE;
  char* ws = (char*)workspace;
  for (int i = 0; i < njobs; ++i) {
    OuterJobDev& d = args.job[i];
    d.norm = reinterpret_cast<float*>(ws); ws += outer_norm_bytes(jobs[i], nb);
    d.V = reinterpret_cast<float*>(ws); ws += outer_v_bytes(jobs[i], rows);
    d.partial = reinterpret_cast<float*>(ws); ws += outer_partial_bytes(jobs[i], nb, nc);
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(kfac_cov_rownorm, dim3((unsigned)nn), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_cov_outer_v, dim3((unsigned)nv), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_cov_outer_gram, dim3((unsigned)ng), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_cov_outer_reduce, dim3((unsigned)nb), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

// ------------------------------------------------------------------ damping sweep
namespace kfac {
static int64_t osweep_nseg(const kfac_cov_outer_sweep_job& j) { return cdiv(j.nG, WSEG); }
static size_t osweep_norm_bytes(const kfac_cov_outer_sweep_job& j, int64_t nb, int nt) {
  return align_up((size_t)(cdiv(osweep_nA(j), TILE) * nb) * nt * sizeof(float), 256);
}
static size_t osweep_v_bytes(const kfac_cov_outer_sweep_job& j, int64_t rows) {
  return align_up((size_t)rows * (size_t)j.nG * sizeof(float), 256);
}
static size_t osweep_partial_bytes(const kfac_cov_outer_sweep_job& j, int64_t nb, int nc, int nt) {
  return align_up((size_t)(nb * osweep_nseg(j)) * nc * nc * nt * sizeof(float), 256);
}
}  // namespace kfac

extern "C" size_t kfac_kron_cov_outer_sweep_workspace_bytes(const kfac_cov_outer_sweep_job* jobs,
                                                            int njobs, int64_t nb, int nc, int nt) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ || nb <= 0 || nc <= 0 || nc > CMAXC || nt <= 0 ||
      nt > SMAXT)
    return 0;
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) {
    if (jobs[i].cols <= 0 || jobs[i].nG <= 0) return 0;
    total += osweep_norm_bytes(jobs[i], nb, nt) + osweep_v_bytes(jobs[i], nb * nc) +
             osweep_partial_bytes(jobs[i], nb, nc, nt);
  }
  return total;
}

extern "C" int kfac_kron_cov_outer_sweep(const kfac_cov_outer_sweep_job* jobs, int njobs, int64_t nb,
                                         int nc, int nt, int accumulate, float* cov, void* workspace,
                                         size_t workspace_bytes, kfac_stream_t stream) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ || nb <= 0 || nc <= 0 || nc > CMAXC || nt <= 0 ||
      nt > SMAXT || !cov)
    return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!osweep_job_ok(jobs[i])) return KFAC_EINVAL;
  const int64_t lim = (int64_t)1 << 31;
  // (kfac_kron_cov_outer's limit: 32-bit sample and delta-row columns, 32-bit task counts)
  if (nb >= (lim - TILE) / nc) return KFAC_EINVAL;
  const int64_t rows = nb * nc;
  OuterArgs args{};
  SweepArgs sw{};
  args.njobs = njobs;
  args.nc = nc;
  args.accumulate = accumulate;
  args.nb = nb;
  args.cov = cov;
  sw.ntau = nt;
  int64_t nn = 0, nv = 0, ng = 0;
  for (int i = 0; i < njobs; ++i) {
    const kfac_cov_outer_sweep_job& q = jobs[i];
    if (osweep_nA(q) >= lim - TILE) return KFAC_EINVAL;
    OuterJobDev& d = args.job[i];
    d.a = q.a; d.D = q.D; d.K1 = q.VA; d.K2 = q.VG;
    d.lda = q.lda; d.ldD = q.ldD; d.ld1 = q.ldA; d.ld2 = q.ldG;
    d.cols = q.cols;
    d.ones = q.has_ones ? q.cols : -1;
    d.nA = (int)osweep_nA(q);
    d.nG = q.nG;
    d.at = (int)cdiv(d.nA, TILE);
    d.bt = (int)cdiv(nb, TILE);
    d.tg = (int)cdiv(q.nG, TILE);
    d.nseg = (int)osweep_nseg(q);
    d.lower1 = d.lower2 = 0;
    d.vrows = (int)rows;
    d.n_begin = (int)nn; d.v_begin = (int)nv; d.g_begin = (int)ng;
    nn += (int64_t)d.at * d.bt;
    nv += cdiv(rows, TILE) * d.tg;
    ng += nb * d.nseg;
    if (nn >= lim || nv >= lim || ng >= lim) return KFAC_EINVAL;
    args.n_end[i] = (int)nn; args.v_end[i] = (int)nv; args.g_end[i] = (int)ng;
    sw.job[i].wA = q.wA; sw.job[i].wG = q.wG;
    sw.job[i].ldwA = q.ldwA; sw.job[i].ldwG = q.ldwG;
  }
  if (!workspace ||
      workspace_bytes < kfac_kron_cov_outer_sweep_workspace_bytes(jobs, njobs, nb, nc, nt))
    return KFAC_EWORKSPACE;
  char* ws = (char*)workspace;
  for (int i = 0; i < njobs; ++i) {
    OuterJobDev& d = args.job[i];
    d.norm = reinterpret_cast<float*>(ws); ws += osweep_norm_bytes(jobs[i], nb, nt);
    d.V = reinterpret_cast<float*>(ws); ws += osweep_v_bytes(jobs[i], rows);
    d.partial = reinterpret_cast<float*>(ws); ws += osweep_partial_bytes(jobs[i], nb, nc, nt);
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(kfac_cov_rownorm_w, dim3((unsigned)nn), dim3(NTHREADS), 0, s, args, sw);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_cov_outer_v, dim3((unsigned)nv), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_cov_outer_sweep_gram, dim3((unsigned)ng), dim3(NTHREADS), 0, s, args, sw);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_cov_outer_sweep_reduce, dim3((unsigned)nb, (unsigned)nt), dim3(NTHREADS), 0,
                     s, args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}
