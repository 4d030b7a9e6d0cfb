// GLM predictive with per-entry eigenbasis weights (kfac_kron_cov_full,
// kfac_kron_cov_outer_full): the sweep calls of covariance.hip / covariance_outer.hip with
// an arbitrary non-negative W[i][g] in place of the rank-one wA[i] wG[g].  A posterior that
// keeps the KFAC eigenbases V_A, V_G and refits every eigenvalue (EFB) has
//   cov[b][c][c'] = sum_layers sum_{i,g} W[i][g] Y_{b,c}[i][g] Y_{b,c'}[i][g] ,
//   Y_{b,c} = V_A^T M_{b,c} V_G ,
// W in the posterior's flat order i*nG + g, nt of them per call (grid point t at W + t*ldW).
//
// Dense rows (kfac_kron_cov_full): kfac_cov_apply_u / kfac_cov_apply_t project the rows
// once (K1 = V_A, K2 = V_G, dense), then
//   gram  : kfac_cov_full_gram, cov_wgram_segment's flat mode: thread t of a WSEG-long
//           segment reads W_tau[k0 + t], no division and no wA wG product
//   reduce: kfac_cov_sweep_reduce.
//
// Factored Linear (kfac_kron_cov_outer_full): the row is rank one, M_{b,c} = abar_b
// delta_{b,c}^T, so Y_{b,c} = p_b q_{b,c}^T with p_b = V_A^T abar_b, Q_b = Delta_b V_G and
//   cov[b] = Q_b diag(r_b) Q_b^T ,   r_b[g] = sum_i p_b[i]^2 W[i][g] :
//   proj2 : kfac_cov_rownorm_w's tile of (Abar V_A)^T with the epilogue replaced by a store
//           of the squares: P2T[i][b] = p_b[i]^2 (nA x nb; the accumulator is i x b already)
//   r     : kfac_cov_full_r, R_t = P2T^T W_t (nb x nA by nA x nG per grid point) on 64x64
//           contract_tile tiles, both operands k-major; tasks (t, sample tile, g tile); an
//           element is ONE k-ordered chain over nA, so it depends on its own sample's
//           column of P2T and its own g column of W_t only, not on nb, nt or the tile
//   v     : kfac_cov_outer_v, Q = Delta V_G
//   gram  : kfac_cov_outer_full_gram, cov_wgram_segment's K = nG mode with sample b's
//           weights at R + b*nG, grid points nb*nG apart
//   reduce: kfac_cov_sweep_reduce (the weights carry the whole scale: no factor is left).
// W >= 0 and the squares make every r >= 0, so a block's diagonal is a sum of non-negative
// products.  No atomics; all the sweep calls' guarantees hold (kfac_hip.h).
#include "covariance_common.h"

namespace kfac {

// Weighted Gram partials of the projected rows, per-entry weights: kfac_cov_sweep_gram
// with sw.job[j].wG = W_j, ldwG = ldW_j (wA unused).
__global__ __launch_bounds__(NTHREADS) void kfac_cov_full_gram(CovArgs args, SweepArgs sw) {
  __shared__ __attribute__((aligned(16))) float lds[WGRAM_LDS];
  const int task = blockIdx.x;
  const int j = cov_find_job(args.g_end, args.njobs, task);
  const CovJobDev& C = args.job[j];
  const int64_t local = task - C.g_begin;
  const int64_t b = local / C.nseg;
  const int seg = (int)(local % C.nseg);
  const int nc = args.nc;
  const int64_t K = (int64_t)C.nA * C.nG;
  cov_wgram_segment<WGRAM_FLAT>(C.T + b * nc * K, K, nc, (int64_t)seg * WSEG, sw.job[j], C.nG, sw.ntau,
                                C.partial + local * nc * nc, args.nb * C.nseg * nc * nc, lds);
}

// One 64 (columns i of V_A) x 64 (samples b) tile of (Abar V_A)^T, squared and stored:
// P2T[i][b] (C.norm, nA x nb).  Element (i, b) is one k-ordered chain over nA.
__global__ __launch_bounds__(NTHREADS) void kfac_cov_proj2(OuterArgs args) {
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
  contract_tile<KFAC_ROWMAJOR, KFAC_SAMPLEROWS>(k1, i0, at, b0, 0, C.nA, false, true, lds, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = b0 + (wave & 1) * 32 + (lane & 31);
  if (b >= args.nb) return;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int i = i0 + (wave >> 1) * 32 + acc_row(v, lane);
    if (i < C.nA) C.norm[(int64_t)i * args.nb + b] = acc[v] * acc[v];
  }
}

// One 64 (samples b) x 64 (g) tile of R_t = P2T^T W_t: R[t][b][g] = sum_i P2T[i][b] W_t[i][g].
__global__ __launch_bounds__(NTHREADS) void kfac_cov_full_r(OuterArgs args, FullOuterArgs fa) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const int jb = cov_find_job(fa.r_end, args.njobs, task);
  const OuterJobDev& C = args.job[jb];
  const int local = task - fa.r_begin[jb];
  const int per = C.bt * C.tg;
  const int t = local / per, rem = local - t * per;
  const int b0 = (rem / C.tg) * TILE, g0 = (rem % C.tg) * TILE;
  const OpDev p2 = rowmajor_op(C.norm, C.nA, (int)args.nb, args.nb);
  const OpDev w = rowmajor_op(fa.W[jb] + (int64_t)t * fa.ldW[jb], C.nA, C.nG, C.nG);
  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  contract_tile<KFAC_ROWMAJOR, KFAC_ROWMAJOR>(p2, b0, w, g0, 0, C.nA, false, true, lds, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = g0 + (wave & 1) * 32 + (lane & 31);
  if (g >= C.nG) return;
  float* dst = fa.R[jb] + (int64_t)t * args.nb * C.nG + g;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int64_t b = b0 + (wave >> 1) * 32 + acc_row(v, lane);
    if (b < args.nb) dst[b * C.nG] = acc[v];
  }
}

// Weighted Gram partials of Q_b over one WSEG-long segment of nG, every tau, sample b's
// own weight vectors r_{tau,b}.
__global__ __launch_bounds__(NTHREADS) void kfac_cov_outer_full_gram(OuterArgs args, FullOuterArgs fa) {
  __shared__ __attribute__((aligned(16))) float lds[WGRAM_LDS];
  const int task = blockIdx.x;
  const int jb = cov_find_job(args.g_end, args.njobs, task);
  const OuterJobDev& C = args.job[jb];
  const int64_t local = task - C.g_begin;
  const int64_t b = local / C.nseg;
  const int seg = (int)(local % C.nseg);
  const int nc = args.nc;
  const int64_t K = C.nG;
  const SweepWeights w{nullptr, fa.R[jb] + b * K, 0, args.nb * K};
  cov_wgram_segment<WGRAM_VECTOR>(C.V + b * nc * K, K, nc, (int64_t)seg * WSEG, w, C.nG, fa.ntau,
                                  C.partial + local * nc * nc, args.nb * C.nseg * nc * nc, lds);
}

static bool full_call_ok(const void* jobs, int njobs, int64_t nb, int nc, int nt) {
  return jobs && njobs > 0 && njobs <= CMAXJ && nb > 0 && nc > 0 && nc <= CMAXC && nt > 0 && nt <= SMAXT;
}

static int64_t full_nseg(const kfac_cov_full_job& j) { return cdiv((int64_t)j.nA * j.nG, WSEG); }
static size_t full_t_bytes(const kfac_cov_full_job& j, int64_t rows) {
  return align_up((size_t)rows * (size_t)j.nA * (size_t)j.nG * sizeof(float), 256);
}
static size_t full_partial_bytes(const kfac_cov_full_job& j, int64_t nb, int nc, int nt) {
  return align_up((size_t)(nb * full_nseg(j)) * nc * nc * nt * sizeof(float), 256);
}

static int64_t ofull_nseg(const kfac_cov_outer_full_job& j) { return cdiv(j.nG, WSEG); }
static size_t ofull_p2_bytes(const kfac_cov_outer_full_job& j, int64_t nb) {
  return align_up((size_t)(ofull_nA(j) * nb) * sizeof(float), 256);
}
static size_t ofull_r_bytes(const kfac_cov_outer_full_job& j, int64_t nb, int nt) {
  return align_up((size_t)nb * (size_t)j.nG * nt * sizeof(float), 256);
}
static size_t ofull_v_bytes(const kfac_cov_outer_full_job& j, int64_t rows) {
  return align_up((size_t)rows * (size_t)j.nG * sizeof(float), 256);
}
static size_t ofull_partial_bytes(const kfac_cov_outer_full_job& j, int64_t nb, int nc, int nt) {
  return align_up((size_t)(nb * ofull_nseg(j)) * nc * nc * nt * sizeof(float), 256);
}

// The projection launches alone (kfac_kron_cov_outer_full_tiled forms its own Grams from R and V).
int cov_launch_proj2(const OuterArgs& args, int64_t nn, hipStream_t s) {
  hipLaunchKernelGGL(kfac_cov_proj2, dim3((unsigned)nn), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

int cov_launch_full_r(const OuterArgs& args, const FullOuterArgs& fa, int64_t nr, hipStream_t s) {
  hipLaunchKernelGGL(kfac_cov_full_r, dim3((unsigned)nr), dim3(NTHREADS), 0, s, args, fa);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}
}  // namespace kfac

using namespace kfac;

extern "C" size_t kfac_kron_cov_full_workspace_bytes(const kfac_cov_full_job* jobs, int njobs, int64_t nb,
                                                     int nc, int nt) {
  if (!full_call_ok(jobs, njobs, nb, nc, nt)) return 0;
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) {
    if (jobs[i].nA <= 0 || jobs[i].nG <= 0) return 0;
    total += 2 * full_t_bytes(jobs[i], nb * nc) + full_partial_bytes(jobs[i], nb, nc, nt);
  }
  return total;
}

extern "C" int kfac_kron_cov_full(const kfac_cov_full_job* jobs, int njobs, int64_t nb, int nc, int nt,
                                  int accumulate, float* cov, void* workspace, size_t workspace_bytes,
                                  kfac_stream_t stream) {
  if (!full_call_ok(jobs, njobs, nb, nc, nt) || !cov) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!full_job_ok(jobs[i])) return KFAC_EINVAL;
  const int64_t lim = (int64_t)1 << 31;
  if (nb >= lim / nc) return KFAC_EINVAL;
  const int64_t rows = nb * nc;
  CovArgs args{};
  SweepArgs sw{};
  args.njobs = njobs;
  args.nc = nc;
  args.accumulate = accumulate;
  args.nb = nb;
  args.cov = cov;
  sw.ntau = nt;
  kfac_cov_job plain[CMAXJ];
  for (int i = 0; i < njobs; ++i) {
    const kfac_cov_full_job& q = jobs[i];
    plain[i] = kfac_cov_job{q.J, q.ldJ, q.nA, q.nG, q.VA, q.ldA, q.VG, q.ldG, 0, 0};
  }
  // (kfac_kron_cov's limits: 32-bit columns of the stacked operands, 32-bit task counts)
  if (!cov_fill_apply(plain, njobs, rows, args)) return KFAC_EINVAL;
  int64_t ng = 0;
  for (int i = 0; i < njobs; ++i) {
    CovJobDev& d = args.job[i];
    d.nseg = (int)full_nseg(jobs[i]);
    d.g_begin = (int)ng;
    ng += nb * d.nseg;
    if (ng >= lim) return KFAC_EINVAL;
    args.g_end[i] = (int)ng;
    sw.job[i].wA = nullptr; sw.job[i].ldwA = 0;
    sw.job[i].wG = jobs[i].W; sw.job[i].ldwG = jobs[i].ldW;
  }
  args.ng = (int)ng;
  if (!workspace || workspace_bytes < kfac_kron_cov_full_workspace_bytes(jobs, njobs, nb, nc, nt))
    return KFAC_EWORKSPACE;
  char* ws = (char*)workspace;
  for (int i = 0; i < njobs; ++i) {
    CovJobDev& d = args.job[i];
    const size_t tb = full_t_bytes(jobs[i], rows);
    d.U = reinterpret_cast<float*>(ws); ws += tb;
    d.T = reinterpret_cast<float*>(ws); ws += tb;
    d.partial = reinterpret_cast<float*>(ws); ws += full_partial_bytes(jobs[i], nb, nc, nt);
  }
  hipStream_t s = (hipStream_t)stream;
  const int st = cov_launch_apply(args, s);
  if (st != KFAC_OK) return st;
  hipLaunchKernelGGL(kfac_cov_full_gram, dim3((unsigned)ng), dim3(NTHREADS), 0, s, args, sw);
  KFAC_CHECK_LAUNCH();
  return cov_launch_sweep_reduce(args, nt, s);
}

extern "C" size_t kfac_kron_cov_outer_full_workspace_bytes(const kfac_cov_outer_full_job* jobs, int njobs,
                                                           int64_t nb, int nc, int nt) {
  if (!full_call_ok(jobs, njobs, nb, nc, nt)) return 0;
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) {
    if (jobs[i].cols <= 0 || jobs[i].nG <= 0) return 0;
    total += ofull_p2_bytes(jobs[i], nb) + ofull_r_bytes(jobs[i], nb, nt) + ofull_v_bytes(jobs[i], nb * nc) +
             ofull_partial_bytes(jobs[i], nb, nc, nt);
  }
  return total;
}

extern "C" int kfac_kron_cov_outer_full(const kfac_cov_outer_full_job* jobs, int njobs, int64_t nb, int nc,
                                        int nt, int accumulate, float* cov, void* workspace,
                                        size_t workspace_bytes, kfac_stream_t stream) {
  if (!full_call_ok(jobs, njobs, nb, nc, nt) || !cov) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!ofull_job_ok(jobs[i])) return KFAC_EINVAL;
  const int64_t lim = (int64_t)1 << 31;
  // (kfac_kron_cov_outer's limit: 32-bit sample and delta-row columns, 32-bit task counts)
  if (nb >= (lim - TILE) / nc) return KFAC_EINVAL;
  const int64_t rows = nb * nc;
  OuterArgs args{};
  FullOuterArgs fa{};
  args.njobs = njobs;
  args.nc = nc;
  args.accumulate = accumulate;
  args.nb = nb;
  args.cov = cov;
  fa.ntau = nt;
  kfac_cov_outer_job plain[CMAXJ];
  for (int i = 0; i < njobs; ++i) {
    const kfac_cov_outer_full_job& q = jobs[i];
    plain[i] = kfac_cov_outer_job{q.a, q.lda, q.cols, q.has_ones, q.D, q.ldD, q.nG, 0,
                                  q.VA, q.ldA, q.VG, q.ldG, 0, 0};
  }
  int64_t nn = 0, nv = 0, nr = 0, ng = 0;
  if (!cov_fill_outer(plain, njobs, nb, rows, args, nn, nv)) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i) {
    OuterJobDev& d = args.job[i];
    d.nseg = (int)ofull_nseg(jobs[i]);
    d.g_begin = (int)ng;
    fa.r_begin[i] = (int)nr;
    ng += nb * d.nseg;
    nr += (int64_t)nt * d.bt * d.tg;
    if (ng >= lim || nr >= lim) return KFAC_EINVAL;
    args.g_end[i] = (int)ng;
    fa.r_end[i] = (int)nr;
    fa.W[i] = jobs[i].W;
    fa.ldW[i] = jobs[i].ldW;
  }
  if (!workspace || workspace_bytes < kfac_kron_cov_outer_full_workspace_bytes(jobs, njobs, nb, nc, nt))
    return KFAC_EWORKSPACE;
  CovArgs red{};  // what kfac_cov_sweep_reduce reads: the partials and their segment counts
  red.njobs = njobs;
  red.nc = nc;
  red.accumulate = accumulate;
  red.nb = nb;
  red.cov = cov;
  char* ws = (char*)workspace;
  for (int i = 0; i < njobs; ++i) {
    OuterJobDev& d = args.job[i];
    d.norm = reinterpret_cast<float*>(ws); ws += ofull_p2_bytes(jobs[i], nb);  // P2T, nA x nb
    fa.R[i] = reinterpret_cast<float*>(ws); ws += ofull_r_bytes(jobs[i], nb, nt);
    d.V = reinterpret_cast<float*>(ws); ws += ofull_v_bytes(jobs[i], rows);
    d.partial = reinterpret_cast<float*>(ws); ws += ofull_partial_bytes(jobs[i], nb, nc, nt);
    red.job[i].partial = d.partial;
    red.job[i].nseg = d.nseg;
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(kfac_cov_proj2, dim3((unsigned)nn), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_cov_full_r, dim3((unsigned)nr), dim3(NTHREADS), 0, s, args, fa);
  KFAC_CHECK_LAUNCH();
  const int st = cov_launch_outer_v(args, nv, s);
  if (st != KFAC_OK) return st;
  hipLaunchKernelGGL(kfac_cov_outer_full_gram, dim3((unsigned)ng), dim3(NTHREADS), 0, s, args, fa);
  KFAC_CHECK_LAUNCH();
  return cov_launch_sweep_reduce(red, nt, s);
}
