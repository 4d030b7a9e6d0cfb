// Weighted GLM predictive for any number of outputs: the damping-sweep and per-entry-weight
// covariance calls with the CLASSES tiled.
//
// covariance.hip / covariance_outer.hip / covariance_full.hip keep one 32x32 MFMA quadrant per
// grid point (cov_wgram_segment, nc <= 32).  Here a sample's block is cut into 64x64 class
// tiles, ntile = ceil(nc / 64), exactly as covariance_tiled.hip cuts it, and every tile pair
// ti >= tj is a WEIGHTED Gram tile of that sample's projected rows X_b (nc x K):
//   part[r][r'] = sum_{k in segment} X_b[r][k] * (w[k] * X_b[r'][k]) .
// The A operand is the plain CHANNEL panel of tile ti's rows, the B operand Panel<KFAC_WCHANNEL>
// (covariance_common.h: the class-tiled INF calls run it on their raw rows):
// tile tj's rows times the k-row's weight as they are loaded (no product is stored), the way
// Panel<KFAC_INF_WJ> forms w.M.  A diagonal tile therefore stages two panels; it still skips
// its upper quadrant.  The weights of a task are w_base + t*stride_t + b*stride_b:
//   flat      K = nA*nG, w[k] = W_t[k]                        kfac_kron_cov_full_tiled
//   rank one  K = nA*nG, w[k] = wA_t[k / nG] * wG_t[k % nG]   kfac_kron_cov_sweep_tiled
//             ((a, g) of a thread's k: one division at init, then advanced by BK)
//   vector    K = nG, R[t][b][g] (per sample)                 kfac_kron_cov_outer_full_tiled
//             K = nG, wG_t[g] (shared), the block times s_{t,b} kfac_kron_cov_outer_sweep_tiled
// The projections are the capped calls' own launches (cov_launch_apply; kfac_cov_proj2,
// kfac_cov_full_r, kfac_cov_outer_v; kfac_cov_rownorm_w), over all nb*nc rows at once.
//   gram    one task per (job, sample b, K segment, grid point t, tile pair): a 64x64 fp32
//           partial at [t][b][pair][segment].  One grid point per task: slice t depends on
//           nothing but its own weights.
//   reduce  per (grid point, sample, tile pair): the partials summed over segments in segment
//           order, (outer sweep: times s_{t,b}, kfac_cov_rownorm_w's column-tile partials
//           summed in tile order,) then over jobs in job order, all in fp64; the lower element
//           is written with its mirror into cov[t][b] (nc x nc contiguous).  No atomics.
// K is cut into segments [s*JSEG, (s+1)*JSEG) by K alone and an element of a partial is one
// k-ordered fma chain from 0 over its segment -- covariance_tiled.hip's segmentation, chain
// and reduce order: with every weight 1 (x * 1 is exact) the dense calls give the bits of
// kfac_kron_cov_tiled on the same rows.  Tasks are ordered (job, sample, segment, grid point,
// tile pair), so the tasks that share a sample's row panels are in flight together.
#include "covariance_common.h"

namespace kfac {

struct WTiledJobDev {
  const float* X;     // nb*nc x K, K contiguous per row
  float* partial;     // [grid point][sample][tile pair][segment][64 x 64]
  const float* norm;  // outer sweep: nt x at x nb column-tile partials of s_{t,b}
  const float* wA;    // rank one: grid point t at wA + t*ldwA
  const float* wG;    // the weights (flat: W; vector: R or wG) at wG + t*stride_t + b*stride_b
  int64_t K, ldwA, stride_t, stride_b;
  int nseg, at, begin, nG, mode;  // begin: first task of this job; mode: WGramMode
};

struct WTiledArgs {
  int njobs, nc, nt, accumulate, npairs, scaled;
  int64_t nb;
  float* cov;
  int end[CMAXJ];
  WTiledJobDev x[CMAXJ];
};
static_assert(sizeof(WTiledArgs) <= 4096, "kernel argument block");

// Gram partial: one tile pair of one sample of one job over one K segment at one grid point.
__global__ __launch_bounds__(NTHREADS) void kfac_cov_wtiled_gram(WTiledArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const WTiledJobDev& G = args.x[cov_find_job(args.end, args.njobs, task)];
  const int local = task - G.begin;
  const int q = local / args.npairs, pair = local - q * args.npairs;
  const int bs = q / args.nt, t = q - bs * args.nt;
  const int64_t b = bs / G.nseg;
  const int seg = bs - (int)b * G.nseg;
  int ti, tj;
  tri_decode(pair, ti, tj);
  const int64_t k0 = (int64_t)seg * JSEG, k1 = min(G.K, k0 + JSEG);
  const float* X = G.X + b * args.nc * G.K;
  const OpDev xa = channel_op(X, G.K, args.nc, G.K);
  const OpDev xw = wchannel_op(X, G.K, G.K, args.nc, G.wA + (int64_t)t * G.ldwA,
                               G.wG + (int64_t)t * G.stride_t + b * G.stride_b, G.nG, G.mode);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool active = !(ti == tj && wave == 1);  // quadrant (0, 1) of a diagonal tile
  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  contract_tile<KFAC_CHANNEL, KFAC_WCHANNEL>(xa, ti * TILE, xw, tj * TILE, k0, k1, false, active, lds, acc);
  if (!active) return;
  float* part = G.partial + ((((int64_t)t * args.nb + b) * args.npairs + pair) * G.nseg + seg) * JTILE2;
  float* dst = part + (wave >> 1) * 32 * TILE + (wave & 1) * 32 + (lane & 31);
#pragma unroll
  for (int v = 0; v < 16; ++v) dst[acc_row(v, lane) * TILE] = acc[v];
}

// cov[t][b] tile (ti >= tj) (+)= sum over jobs (in job order) of the segment sums (in segment
// order), fp64; scaled: job j's sum times s_{j,t,b}.  Grid (nb * tile pairs, JTILE2 / NTHREADS,
// nt): a block owns four rows of the tile, a thread one element, as the tiled reduce.
__global__ __launch_bounds__(NTHREADS) void kfac_cov_wtiled_reduce(WTiledArgs args) {
  __shared__ double scale[CMAXJ];
  const int64_t b = blockIdx.x / args.npairs, t = blockIdx.z;
  const int pair = blockIdx.x - (int)b * args.npairs;
  if (args.scaled) {
    if ((int)threadIdx.x < args.njobs) {
      const WTiledJobDev& G = args.x[threadIdx.x];
      double s = 0.0;
      for (int i = 0; i < G.at; ++i) s += (double)G.norm[(t * G.at + i) * args.nb + b];
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
    const WTiledJobDev& G = args.x[j];
    const float* part = G.partial + ((t * args.nb + b) * args.npairs + pair) * G.nseg * JTILE2 + e;
    double s = 0.0;
    for (int i = 0; i < G.nseg; ++i) s += (double)part[(int64_t)i * JTILE2];
    total += args.scaled ? scale[j] * s : s;
  }
  float* cov = args.cov + (t * args.nb + b) * nc * nc;
  float* lo = cov + (int64_t)r * nc + c;
  const float v = args.accumulate ? (float)((double)*lo + total) : (float)total;
  *lo = v;
  cov[(int64_t)c * nc + r] = v;
}

static bool wtiled_call_ok(const void* jobs, int njobs, int nt) {
  return jobs && njobs > 0 && njobs <= CMAXJ && nt > 0 && nt <= SMAXT;
}
static size_t wtiled_partial_bytes(int64_t nb, int nc, int nt, int64_t K) {
  return align_up((size_t)(nb * tiled_npairs(nc) * cdiv(K, JSEG)) * nt * JTILE2 * sizeof(float), 256);
}
static size_t wtiled_t_bytes(int64_t rows, int64_t nA, int64_t nG) {
  return align_up((size_t)rows * (size_t)nA * (size_t)nG * sizeof(float), 256);
}
static size_t wtiled_f_bytes(int64_t n) { return align_up((size_t)n * sizeof(float), 256); }

// false: the tile pairs do not fit 31 bits
static bool wtiled_head(WTiledArgs& a, int njobs, int64_t nb, int nc, int nt, int accumulate, float* cov) {
  if (tiled_npairs(nc) >= ((int64_t)1 << 31)) return false;
  a.njobs = njobs;
  a.nc = nc;
  a.nt = nt;
  a.accumulate = accumulate;
  a.npairs = (int)tiled_npairs(nc);
  a.nb = nb;
  a.cov = cov;
  return true;
}

// job i of the Gram launch: nb samples x segments x grid points x tile pairs; false: the tasks
// (and with them the reduce's nb * tile pairs blocks) do not fit 31 bits
static bool wtiled_add_job(WTiledArgs& a, int i, int64_t K, int nG, int mode, int64_t& ntasks) {
  const int64_t lim = (int64_t)1 << 31;
  WTiledJobDev& g = a.x[i];
  const int64_t nseg = cdiv(K, JSEG);
  g.K = K;
  g.nG = nG;
  g.mode = mode;
  g.nseg = (int)nseg;
  g.begin = (int)ntasks;
  const int64_t per = nseg * a.nt * a.npairs;  // nseg < 2^31, nt <= 64, npairs < 2^50: no overflow
  if (nseg >= lim / a.npairs || per >= lim || a.nb >= lim / per) return false;
  ntasks += a.nb * per;
  if (ntasks >= lim) return false;
  a.end[i] = (int)ntasks;
  return true;
}

static int wtiled_launch_gram_reduce(const WTiledArgs& args, int64_t ng, hipStream_t s) {
  hipLaunchKernelGGL(kfac_cov_wtiled_gram, dim3((unsigned)ng), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  const dim3 grid((unsigned)(args.nb * args.npairs), JTILE2 / NTHREADS, (unsigned)args.nt);
  hipLaunchKernelGGL(kfac_cov_wtiled_reduce, grid, dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

// The dense calls: U, T, partials per job; T by cov_launch_apply with K1 = V_A, K2 = V_G dense.
template <class Job>
static size_t wtiled_dense_bytes(const Job* jobs, int njobs, int64_t nb, int nc, int nt) {
  if (!wtiled_call_ok(jobs, njobs, nt)) return 0;
  const int64_t rows = tiled_rows(nb, nc);
  if (!rows) return 0;
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) {
    if (jobs[i].nA <= 0 || jobs[i].nG <= 0) return 0;
    total += 2 * wtiled_t_bytes(rows, jobs[i].nA, jobs[i].nG) +
             wtiled_partial_bytes(nb, nc, nt, (int64_t)jobs[i].nA * jobs[i].nG);
  }
  return total;
}

// weights(i, g): the weight fields of Gram job g from job i
template <class Job, class Weights>
static int wtiled_dense(const Job* jobs, int njobs, int64_t nb, int nc, int nt, int accumulate, float* cov,
                        void* workspace, size_t workspace_bytes, hipStream_t s, int mode, Weights weights) {
  const int64_t rows = tiled_rows(nb, nc);
  if (!rows) return KFAC_EINVAL;
  CovArgs ap{};
  WTiledArgs args{};
  ap.njobs = njobs;
  ap.nc = nc;
  ap.nb = nb;
  if (!wtiled_head(args, njobs, nb, nc, nt, accumulate, cov)) return KFAC_EINVAL;
  kfac_cov_job plain[CMAXJ];
  for (int i = 0; i < njobs; ++i) {
    const Job& q = jobs[i];
    plain[i] = kfac_cov_job{q.J, q.ldJ, q.nA, q.nG, q.VA, q.ldA, q.VG, q.ldG, 0, 0};
  }
  if (!cov_fill_apply(plain, njobs, rows, ap)) return KFAC_EINVAL;
  int64_t ng = 0;
  for (int i = 0; i < njobs; ++i) {
    if (!wtiled_add_job(args, i, (int64_t)jobs[i].nA * jobs[i].nG, jobs[i].nG, mode, ng)) return KFAC_EINVAL;
    weights(jobs[i], args.x[i]);
  }
  if (!workspace || workspace_bytes < wtiled_dense_bytes(jobs, njobs, nb, nc, nt)) return KFAC_EWORKSPACE;
  char* ws = (char*)workspace;
  for (int i = 0; i < njobs; ++i) {
    CovJobDev& d = ap.job[i];
    const size_t tb = wtiled_t_bytes(rows, jobs[i].nA, jobs[i].nG);
    d.U = reinterpret_cast<float*>(ws); ws += tb;
    d.T = reinterpret_cast<float*>(ws); ws += tb;
    args.x[i].X = d.T;
    args.x[i].partial = reinterpret_cast<float*>(ws);
    ws += wtiled_partial_bytes(nb, nc, nt, args.x[i].K);
  }
  const int rc = cov_launch_apply(ap, s);
  if (rc != KFAC_OK) return rc;
  return wtiled_launch_gram_reduce(args, ng, s);
}

}  // namespace kfac

using namespace kfac;

extern "C" size_t kfac_kron_cov_full_tiled_workspace_bytes(const kfac_cov_full_job* jobs, int njobs,
                                                           int64_t nb, int nc, int nt) {
  return wtiled_dense_bytes(jobs, njobs, nb, nc, nt);
}

extern "C" int kfac_kron_cov_full_tiled(const kfac_cov_full_job* jobs, int njobs, int64_t nb, int nc, int nt,
                                        int accumulate, float* cov, void* workspace, size_t workspace_bytes,
                                        kfac_stream_t stream) {
  if (!wtiled_call_ok(jobs, njobs, nt) || !cov) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!full_job_ok(jobs[i])) return KFAC_EINVAL;
  return wtiled_dense(jobs, njobs, nb, nc, nt, accumulate, cov, workspace, workspace_bytes,
                      (hipStream_t)stream, WGRAM_FLAT, [](const kfac_cov_full_job& q, WTiledJobDev& g) {
                        g.wA = nullptr; g.ldwA = 0;
                        g.wG = q.W; g.stride_t = q.ldW; g.stride_b = 0;
                      });
}

extern "C" size_t kfac_kron_cov_sweep_tiled_workspace_bytes(const kfac_cov_sweep_job* jobs, int njobs,
                                                            int64_t nb, int nc, int nt) {
  return wtiled_dense_bytes(jobs, njobs, nb, nc, nt);
}

extern "C" int kfac_kron_cov_sweep_tiled(const kfac_cov_sweep_job* jobs, int njobs, int64_t nb, int nc,
                                         int nt, int accumulate, float* cov, void* workspace,
                                         size_t workspace_bytes, kfac_stream_t stream) {
  if (!wtiled_call_ok(jobs, njobs, nt) || !cov) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!sweep_job_ok(jobs[i])) return KFAC_EINVAL;
  return wtiled_dense(jobs, njobs, nb, nc, nt, accumulate, cov, workspace, workspace_bytes,
                      (hipStream_t)stream, WGRAM_RANK1, [](const kfac_cov_sweep_job& q, WTiledJobDev& g) {
                        g.wA = q.wA; g.ldwA = q.ldwA;
                        g.wG = q.wG; g.stride_t = q.ldwG; g.stride_b = 0;
                      });
}

extern "C" size_t kfac_kron_cov_outer_full_tiled_workspace_bytes(const kfac_cov_outer_full_job* jobs,
                                                                 int njobs, int64_t nb, int nc, int nt) {
  if (!wtiled_call_ok(jobs, njobs, nt)) return 0;
  const int64_t rows = tiled_rows(nb, nc);
  if (!rows) return 0;
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) {
    if (jobs[i].cols <= 0 || jobs[i].nG <= 0) return 0;
    // P2T (nA x nb), R (nt x nb x nG), V (rows x nG), the partials
    total += wtiled_f_bytes(ofull_nA(jobs[i]) * nb) + wtiled_f_bytes(nb * jobs[i].nG * nt) +
             wtiled_f_bytes(rows * jobs[i].nG) + wtiled_partial_bytes(nb, nc, nt, jobs[i].nG);
  }
  return total;
}

extern "C" int kfac_kron_cov_outer_full_tiled(const kfac_cov_outer_full_job* jobs, int njobs, int64_t nb,
                                              int nc, int nt, int accumulate, float* cov, void* workspace,
                                              size_t workspace_bytes, kfac_stream_t stream) {
  if (!wtiled_call_ok(jobs, njobs, nt) || !cov) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!ofull_job_ok(jobs[i])) return KFAC_EINVAL;
  const int64_t rows = tiled_rows(nb, nc);
  if (!rows) return KFAC_EINVAL;
  const int64_t lim = (int64_t)1 << 31;
  OuterArgs op{};
  FullOuterArgs fa{};
  WTiledArgs args{};
  op.njobs = njobs;
  op.nc = nc;
  op.nb = nb;
  fa.ntau = nt;
  if (!wtiled_head(args, njobs, nb, nc, nt, accumulate, cov)) return KFAC_EINVAL;
  kfac_cov_outer_job plain[CMAXJ];
  for (int i = 0; i < njobs; ++i) {
    const kfac_cov_outer_full_job& q = jobs[i];
    plain[i] = kfac_cov_outer_job{q.a, q.lda, q.cols, q.has_ones, q.D, q.ldD, q.nG, 0,
                                  q.VA, q.ldA, q.VG, q.ldG, 0, 0};
  }
  int64_t nn = 0, nv = 0, nr = 0, ng = 0;
  if (!cov_fill_outer(plain, njobs, nb, rows, op, nn, nv)) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i) {
    const OuterJobDev& d = op.job[i];
    fa.r_begin[i] = (int)nr;
    nr += (int64_t)nt * d.bt * d.tg;
    if (nr >= lim) return KFAC_EINVAL;
    fa.r_end[i] = (int)nr;
    fa.W[i] = jobs[i].W;
    fa.ldW[i] = jobs[i].ldW;
    if (!wtiled_add_job(args, i, jobs[i].nG, jobs[i].nG, WGRAM_VECTOR, ng)) return KFAC_EINVAL;
  }
  if (!workspace ||
      workspace_bytes < kfac_kron_cov_outer_full_tiled_workspace_bytes(jobs, njobs, nb, nc, nt))
    return KFAC_EWORKSPACE;
  char* ws = (char*)workspace;
  for (int i = 0; i < njobs; ++i) {
    OuterJobDev& d = op.job[i];
    WTiledJobDev& g = args.x[i];
    d.norm = reinterpret_cast<float*>(ws); ws += wtiled_f_bytes(ofull_nA(jobs[i]) * nb);  // P2T
    fa.R[i] = reinterpret_cast<float*>(ws); ws += wtiled_f_bytes(nb * jobs[i].nG * nt);
    d.V = reinterpret_cast<float*>(ws); ws += wtiled_f_bytes(rows * jobs[i].nG);
    g.X = d.V;
    g.wA = nullptr; g.ldwA = 0;
    g.wG = fa.R[i]; g.stride_t = nb * (int64_t)d.nG; g.stride_b = d.nG;
    g.partial = reinterpret_cast<float*>(ws);
    ws += wtiled_partial_bytes(nb, nc, nt, d.nG);
  }
  hipStream_t s = (hipStream_t)stream;
  int rc = cov_launch_proj2(op, nn, s);
  if (rc != KFAC_OK) return rc;
  rc = cov_launch_full_r(op, fa, nr, s);
  if (rc != KFAC_OK) return rc;
  rc = cov_launch_outer_v(op, nv, s);
  if (rc != KFAC_OK) return rc;
  return wtiled_launch_gram_reduce(args, ng, s);
}

extern "C" size_t kfac_kron_cov_outer_sweep_tiled_workspace_bytes(const kfac_cov_outer_sweep_job* jobs,
                                                                  int njobs, int64_t nb, int nc, int nt) {
  if (!wtiled_call_ok(jobs, njobs, nt)) return 0;
  const int64_t rows = tiled_rows(nb, nc);
  if (!rows) return 0;
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) {
    if (jobs[i].cols <= 0 || jobs[i].nG <= 0) return 0;
    // the weighted row-norm partials (nt x ceil(nA/64) x nb), V (rows x nG), the partials
    total += wtiled_f_bytes(cdiv(osweep_nA(jobs[i]), TILE) * nb * nt) + wtiled_f_bytes(rows * jobs[i].nG) +
             wtiled_partial_bytes(nb, nc, nt, jobs[i].nG);
  }
  return total;
}

extern "C" int kfac_kron_cov_outer_sweep_tiled(const kfac_cov_outer_sweep_job* jobs, int njobs, int64_t nb,
                                               int nc, int nt, int accumulate, float* cov, void* workspace,
                                               size_t workspace_bytes, kfac_stream_t stream) {
  if (!wtiled_call_ok(jobs, njobs, nt) || !cov) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!osweep_job_ok(jobs[i])) return KFAC_EINVAL;
  const int64_t rows = tiled_rows(nb, nc);
  if (!rows) return KFAC_EINVAL;
  OuterArgs op{};
  SweepArgs sw{};
  WTiledArgs args{};
  op.njobs = njobs;
  op.nc = nc;
  op.nb = nb;
  sw.ntau = nt;
  if (!wtiled_head(args, njobs, nb, nc, nt, accumulate, cov)) return KFAC_EINVAL;
  args.scaled = 1;
  kfac_cov_outer_job plain[CMAXJ];
  for (int i = 0; i < njobs; ++i) {
    const kfac_cov_outer_sweep_job& q = jobs[i];
    plain[i] = kfac_cov_outer_job{q.a, q.lda, q.cols, q.has_ones, q.D, q.ldD, q.nG, 0,
                                  q.VA, q.ldA, q.VG, q.ldG, 0, 0};
    sw.job[i].wA = q.wA; sw.job[i].wG = q.wG;
    sw.job[i].ldwA = q.ldwA; sw.job[i].ldwG = q.ldwG;
  }
  int64_t nn = 0, nv = 0, ng = 0;
  if (!cov_fill_outer(plain, njobs, nb, rows, op, nn, nv)) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!wtiled_add_job(args, i, jobs[i].nG, jobs[i].nG, WGRAM_VECTOR, ng)) return KFAC_EINVAL;
  if (!workspace ||
      workspace_bytes < kfac_kron_cov_outer_sweep_tiled_workspace_bytes(jobs, njobs, nb, nc, nt))
    return KFAC_EWORKSPACE;
  char* ws = (char*)workspace;
  for (int i = 0; i < njobs; ++i) {
    OuterJobDev& d = op.job[i];
    WTiledJobDev& g = args.x[i];
    d.norm = reinterpret_cast<float*>(ws); ws += wtiled_f_bytes((int64_t)d.at * nb * nt);
    d.V = reinterpret_cast<float*>(ws); ws += wtiled_f_bytes(rows * jobs[i].nG);
    g.X = d.V;
    g.norm = d.norm;
    g.at = d.at;
    g.wA = nullptr; g.ldwA = 0;
    g.wG = jobs[i].wG; g.stride_t = jobs[i].ldwG; g.stride_b = 0;
    g.partial = reinterpret_cast<float*>(ws);
    ws += wtiled_partial_bytes(nb, nc, nt, d.nG);
  }
  hipStream_t s = (hipStream_t)stream;
  int rc = cov_launch_rownorm_w(op, sw, nn, s);
  if (rc != KFAC_OK) return rc;
  rc = cov_launch_outer_v(op, nv, s);
  if (rc != KFAC_OK) return rc;
  return wtiled_launch_gram_reduce(args, ng, s);
}
