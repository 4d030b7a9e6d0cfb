// GLM Monte-Carlo predictive: logit draws without weight samples.
//
// A posterior weight draw is S = K1 Z K2^T (kfac_sample, posterior order a*nG + g), and the
// network is linear in the weights under the GLM, so draw s perturbs logit row r = b*nc + c by
//   dF[s][r] = sum_jobs < M_r , K1 Z_s K2^T >_F = sum_jobs < T_r , Z_s >_F ,  T_r = K1^T M_r K2,
// the projected row the covariance calls already form.  Two routes:
//   kfac_glm_draws        T by kfac_cov_apply_u / kfac_cov_apply_t (cov_launch_apply), then
//                         F = Z T^T: an NT GEMM over K = nA*nG, 64 draws x 64 rows per tile
//                         (contract_tile, fp32 MFMA), K cut into JSEG-long segments by K alone,
//                         one fp32 partial tile per segment.
//   kfac_glm_draws_outer  Linear layers: T_r = u_b v_r^T with U = Abar K1 (kfac_cov_outer_u)
//                         and V = Delta K2 (kfac_cov_outer_v), so dF[s][r] = u_b^T Z_s v_r.
//                         One task per (draw, 64-column g-tile, 64-sample tile): the 64x64
//                         tile W[b][g] = sum_a U[b][a] Z_s[a][g] (fp32 MFMA, K = nA, Z_s the
//                         row-major B operand: its loads run along g), put in LDS and, while
//                         it is there, contracted with V's g-tile for every class:
//                           part[s][g-tile][r] = sum_{g in tile} W[b(r)][g] V[r][g]
//                         (a thread owns a row r and walks g in order; V is read through its
//                         transpose Vt (nG x R), so the lanes' loads run along r).  W never
//                         reaches global memory.  The tasks of a draw partition Z_s's columns:
//                         every element of Z is read once per sample tile, whatever the
//                         number of g-tiles, so the g range is always split over workgroups
//                         and a draw of one wide layer fills the device on its own.
//   reduce                F[s][r] (+)= the partials in segment (g-tile) order, then the jobs
//                         in job order, in fp64.  No atomics.
// An element of a partial is one k-ordered fma chain whose length and cut points depend on nA
// and nG alone; it reads row r's inputs and draw s only.  Hence F[s][r] does not depend on nb,
// ns, or on where the sample or the draw sits in the call.
//
// kfac_softmax_mc: the softmax statistics of mean + F, one wave per sample, fp64 throughout.
#include "covariance_common.h"

namespace kfac {

constexpr int DRED = JTILE2 / NTHREADS;  // reduce blocks per 64x64 tile
constexpr int WP = TILE + 1;             // LDS pitch of the W tile
static_assert(TILE * WP <= 4 * PANEL, "the W tile fits the staging buffer");

// ------------------------------------------------------------------ rows given
struct DrawJobDev {
  const float* T;   // R x K, row r = K1^T M_r K2
  const float* Z;   // ns x K, row stride ldZ
  float* partial;   // [segment][row tile][draw tile][64 draws x 64 rows]
  int64_t K, ldZ;
  int nseg, begin;  // begin: first task of this job
};

struct DrawArgs {
  int njobs, accumulate;
  int R, ns, rt, st;  // rows, draws, their 64-tiles
  int64_t ldF;
  float* F;
  int end[CMAXJ];
  DrawJobDev job[CMAXJ];
};

// Partial: 64 draws x 64 rows of Z T^T over one K segment.  A = Z (the tile's rows are
// draws), B = T (the lanes walk r: the partial and F are written along r).
__global__ __launch_bounds__(NTHREADS) void kfac_glm_draws_tile(DrawArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const DrawJobDev& C = args.job[cov_find_job(args.end, args.njobs, task)];
  const int local = task - C.begin;
  const int per = args.rt * args.st;
  const int seg = local / per, tile = local - seg * per;
  const int tr = tile / args.st, ts = tile - tr * args.st;
  const OpDev z = channel_op(C.Z, C.K, args.ns, C.ldZ);
  const OpDev t = channel_op(C.T, C.K, args.R, C.K);
  const int64_t k0 = (int64_t)seg * JSEG;
  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  contract_tile<KFAC_CHANNEL, KFAC_CHANNEL>(z, ts * TILE, t, tr * TILE, k0, min(C.K, k0 + JSEG), false, true,
                                            lds, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* dst = C.partial + (int64_t)local * JTILE2 + (wave >> 1) * 32 * TILE + (wave & 1) * 32 + (lane & 31);
#pragma unroll
  for (int v = 0; v < 16; ++v) dst[acc_row(v, lane) * TILE] = acc[v];
}

// F tile (+)= the segments in order, then the jobs in order, fp64.  Grid (tiles, DRED).
__global__ __launch_bounds__(NTHREADS) void kfac_glm_draws_reduce(DrawArgs args) {
  const int tile = blockIdx.x;
  const int tr = tile / args.st, ts = tile - tr * args.st;
  const int e = blockIdx.y * NTHREADS + threadIdx.x;
  const int s = ts * TILE + (e >> 6), r = tr * TILE + (e & (TILE - 1));
  if (s >= args.ns || r >= args.R) return;
  const int64_t per = (int64_t)args.rt * args.st;
  double total = 0.0;
  for (int j = 0; j < args.njobs; ++j) {
    const DrawJobDev& C = args.job[j];
    const float* part = C.partial + (int64_t)tile * JTILE2 + e;
    double sum = 0.0;
    for (int i = 0; i < C.nseg; ++i) sum += (double)part[(int64_t)i * per * JTILE2];
    total += sum;
  }
  float* f = args.F + (int64_t)s * args.ldF + r;
  *f = args.accumulate ? (float)((double)*f + total) : (float)total;
}

// ------------------------------------------------------------------ Linear layers
struct DrawOuterJobDev {
  const float* U;   // nb x nA
  const float* V;   // R x nG
  float* Vt;        // nG x R
  const float* Z;   // draw s at Z + s*ldZ: nA x nG row-major
  float* partial;   // [draw][g-tile][R]
  int64_t ldZ;
  int nA, nG, tg;
  int begin, t_begin;  // first task of this job in the tile / transpose launch
};

struct DrawOuterArgs {
  int njobs, nc, accumulate;
  int R, nb, bt;
  int64_t ns, ldF;
  float* F;
  int end[CMAXJ], t_end[CMAXJ];
  DrawOuterJobDev job[CMAXJ];
};
static_assert(sizeof(DrawOuterArgs) <= 4096, "kernel argument block");

// Vt = V^T, 64x64 tiles through LDS: both sides run along the lanes.
__global__ __launch_bounds__(NTHREADS) void kfac_glm_draws_vt(DrawOuterArgs args) {
  __shared__ float tile[TILE * WP];
  const int task = blockIdx.x;
  const DrawOuterJobDev& C = args.job[cov_find_job(args.t_end, args.njobs, task)];
  const int local = task - C.t_begin;
  const int r0 = (local / C.tg) * TILE, g0 = (local % C.tg) * TILE;
  const int x = threadIdx.x & 63, y0 = threadIdx.x >> 6;
  for (int y = y0; y < TILE; y += 4) {
    const int r = r0 + y, g = g0 + x;
    if (r < args.R && g < C.nG) tile[y * WP + x] = C.V[(int64_t)r * C.nG + g];
  }
  __syncthreads();
  for (int y = y0; y < TILE; y += 4) {
    const int g = g0 + y, r = r0 + x;
    if (r < args.R && g < C.nG) C.Vt[(int64_t)g * args.R + r] = tile[x * WP + y];
  }
}

// The hot kernel: one (draw, g-tile, sample tile).  W = U_tile Z_s[:, g-tile] by MFMA,
// then part[r] = sum_g W[b(r)][g] V[r][g] for the tile's rows r = b*nc + c, every c.
__global__ __launch_bounds__(NTHREADS) void kfac_glm_draws_outer_tile(DrawOuterArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const DrawOuterJobDev& C = args.job[cov_find_job(args.end, args.njobs, task)];
  const int local = task - C.begin;
  const int per = C.tg * args.bt;
  const int s = local / per, rem = local - s * per;
  const int gt = rem / args.bt, b0 = (rem - gt * args.bt) * TILE, g0 = gt * TILE;
  const OpDev u = channel_op(C.U, C.nA, args.nb, C.nA);
  const OpDev z = rowmajor_op(C.Z + (int64_t)s * C.ldZ, C.nA, C.nG, C.nG);
  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  // W[b][g] = sum_a U[b][a] Z_s[a][g]
  contract_tile<KFAC_CHANNEL, KFAC_ROWMAJOR>(u, b0, z, g0, 0, C.nA, false, true, lds, acc);
  // (contract_tile leaves through a barrier: lds is free)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* w = lds + (wave >> 1) * 32 * WP + (wave & 1) * 32 + (lane & 31);
#pragma unroll
  for (int v = 0; v < 16; ++v) w[acc_row(v, lane) * WP] = acc[v];
  __syncthreads();
  const int nc = args.nc, R = args.R;
  const int nrows = min(TILE, args.nb - b0) * nc;
  const int gl = min(TILE, C.nG - g0);
  const int64_t r0 = (int64_t)b0 * nc;
  const float* vt = C.Vt + (int64_t)g0 * R + r0;
  float* part = C.partial + ((int64_t)s * C.tg + gt) * R + r0;
  for (int p = tid; p < nrows; p += NTHREADS) {
    const float* wb = lds + (p / nc) * WP;
    const float* vp = vt + p;
    float sum = 0.f;
#pragma unroll 8
    for (int g = 0; g < gl; ++g) sum = fmaf(wb[g], vp[(int64_t)g * R], sum);
    part[p] = sum;
  }
}

// F[s][r] (+)= the g-tile partials in tile order, then the jobs in job order, fp64.
// Grid: draws x 256-row blocks, the row blocks of a draw adjacent.
__global__ __launch_bounds__(NTHREADS) void kfac_glm_draws_outer_reduce(DrawOuterArgs args, int rblocks) {
  const int64_t s = blockIdx.x / rblocks;
  const int r = (blockIdx.x - (int)s * rblocks) * NTHREADS + threadIdx.x;
  if (r >= args.R) return;
  double total = 0.0;
  for (int j = 0; j < args.njobs; ++j) {
    const DrawOuterJobDev& C = args.job[j];
    const float* part = C.partial + s * C.tg * args.R + r;
    double sum = 0.0;
    for (int i = 0; i < C.tg; ++i) sum += (double)part[(int64_t)i * args.R];
    total += sum;
  }
  float* f = args.F + s * args.ldF + r;
  *f = args.accumulate ? (float)((double)*f + total) : (float)total;
}

// ------------------------------------------------------------------ softmax statistics
__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) x = fmax(x, __shfl_xor(x, m));
  return x;
}
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) x += __shfl_xor(x, m);
  return x;
}

// One wave per sample; lane l owns the classes l, l + 64, ... and their psum entries, the
// draws go through in order.  With y = mean + F - max:  H = log sum e^y - sum p y.
__global__ __launch_bounds__(NTHREADS) void kfac_softmax_mc_kernel(const float* mean, int64_t ldm,
                                                                   const float* F, int64_t ldF, int64_t ns,
                                                                   int64_t nb, int nc, int accumulate,
                                                                   double* psum, double* hsum) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * (NTHREADS / 64) + (threadIdx.x >> 6);
  if (b >= nb) return;
  const float* mu = mean + b * ldm;
  double* ps = psum + b * nc;
  // class `lane` (all of them up to nc = 64) lives in registers; classes lane + 64, ... go
  // through psum itself.  The running sums go on from psum / hsum: chunking the draws
  // changes no bit.
  const bool own = lane < nc;
  const double mu0 = own ? (double)mu[lane] : 0.0;
  double p0 = (accumulate && own) ? ps[lane] : 0.0;
  if (!accumulate)
    for (int c = lane + 64; c < nc; c += 64) ps[c] = 0.0;
  double h = accumulate ? hsum[b] : 0.0;
  const float* f = F + b * nc;
  float f0 = own ? f[lane] : 0.f;
  for (int64_t s = 0; s < ns; ++s, f += ldF) {
    const double y0 = mu0 + (double)f0;
    if (own && s + 1 < ns) f0 = f[ldF + lane];  // the next draw's load is under way
    double top = own ? y0 : -INFINITY;
    for (int c = lane + 64; c < nc; c += 64) top = fmax(top, (double)mu[c] + (double)f[c]);
    top = wave_max(top);
    const double e0 = own ? exp(y0 - top) : 0.0;
    double se = e0, sy = own ? e0 * (y0 - top) : 0.0;
    for (int c = lane + 64; c < nc; c += 64) {
      const double y = ((double)mu[c] + (double)f[c]) - top;
      const double e = exp(y);
      se += e;
      sy += e * y;
    }
    se = wave_sum(se);
    sy = wave_sum(sy);
    h += log(se) - sy / se;
    p0 += e0 / se;
    for (int c = lane + 64; c < nc; c += 64) ps[c] += exp(((double)mu[c] + (double)f[c]) - top) / se;
  }
  if (own) ps[lane] = p0;
  if (lane == 0) hsum[b] = h;
}

// ------------------------------------------------------------------ host
// R = nb*nc for 32-bit row indices, or 0
static int64_t draw_rows(int64_t nb, int nc, int64_t ns) {
  const int64_t lim = ((int64_t)1 << 31) - TILE;
  if (nb <= 0 || nc <= 0 || ns <= 0 || ns >= lim || nb >= lim / nc) return 0;
  return nb * nc;
}
static size_t draw_partial_bytes(int64_t R, int64_t ns, int64_t K) {
  return align_up((size_t)(cdiv(K, JSEG) * cdiv(R, TILE) * cdiv(ns, TILE)) * JTILE2 * sizeof(float), 256);
}
static size_t draw_outer_partial_bytes(const kfac_cov_outer_job& j, int64_t R, int64_t ns) {
  return align_up((size_t)ns * (size_t)cdiv(j.nG, TILE) * (size_t)R * sizeof(float), 256);
}

}  // namespace kfac

using namespace kfac;

extern "C" size_t kfac_glm_draws_workspace_bytes(const kfac_draw_job* jobs, int njobs, int64_t nb, int nc,
                                                 int64_t ns) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ) return 0;
  const int64_t R = draw_rows(nb, nc, ns);
  if (!R) return 0;
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) {
    const kfac_cov_job& q = jobs[i].rows;
    if (q.nA <= 0 || q.nG <= 0) return 0;
    total += 2 * cov_t_bytes(q, R) + draw_partial_bytes(R, ns, (int64_t)q.nA * q.nG);
  }
  return total;
}

extern "C" int kfac_glm_draws(const kfac_draw_job* jobs, int njobs, int64_t nb, int nc, int64_t ns,
                              int accumulate, float* F, int64_t ldF, void* workspace, size_t workspace_bytes,
                              kfac_stream_t stream) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ || !F) return KFAC_EINVAL;
  kfac_cov_job rows[CMAXJ];
  for (int i = 0; i < njobs; ++i) {
    rows[i] = jobs[i].rows;
    if (!cov_job_ok(rows[i]) || !jobs[i].Z || jobs[i].ldZ < (int64_t)rows[i].nA * rows[i].nG) return KFAC_EINVAL;
  }
  const int64_t R = draw_rows(nb, nc, ns);
  if (!R || ldF < R) return KFAC_EINVAL;
  const int64_t lim = (int64_t)1 << 31;
  CovArgs ap{};
  DrawArgs args{};
  ap.njobs = args.njobs = njobs;
  ap.nc = nc;
  ap.nb = nb;
  args.accumulate = accumulate;
  args.R = (int)R;
  args.ns = (int)ns;
  args.rt = (int)cdiv(R, TILE);
  args.st = (int)cdiv(ns, TILE);
  args.ldF = ldF;
  args.F = F;
  if (!cov_fill_apply(rows, njobs, R, ap)) return KFAC_EINVAL;
  const int64_t tiles = (int64_t)args.rt * args.st;
  if (tiles >= lim) return KFAC_EINVAL;
  int64_t ntasks = 0;
  for (int i = 0; i < njobs; ++i) {
    DrawJobDev& d = args.job[i];
    d.K = (int64_t)rows[i].nA * rows[i].nG;
    d.Z = jobs[i].Z;
    d.ldZ = jobs[i].ldZ;
    d.nseg = (int)cdiv(d.K, JSEG);
    d.begin = (int)ntasks;
    if (d.nseg >= lim / tiles) return KFAC_EINVAL;
    ntasks += d.nseg * tiles;
    if (ntasks >= lim) return KFAC_EINVAL;
    args.end[i] = (int)ntasks;
  }
  if (!workspace || workspace_bytes < kfac_glm_draws_workspace_bytes(jobs, njobs, nb, nc, ns))
    return KFAC_EWORKSPACE;
  char* ws = (char*)workspace;
  for (int i = 0; i < njobs; ++i) {
    CovJobDev& c = ap.job[i];
    const size_t tb = cov_t_bytes(rows[i], R);
    c.U = reinterpret_cast<float*>(ws); ws += tb;
    c.T = reinterpret_cast<float*>(ws); ws += tb;
    args.job[i].T = c.T;
    args.job[i].partial = reinterpret_cast<float*>(ws);
    ws += draw_partial_bytes(R, ns, args.job[i].K);
  }
  hipStream_t s = (hipStream_t)stream;
  const int rc = cov_launch_apply(ap, s);
  if (rc != KFAC_OK) return rc;
  hipLaunchKernelGGL(kfac_glm_draws_tile, dim3((unsigned)ntasks), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_glm_draws_reduce, dim3((unsigned)tiles, DRED), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

extern "C" size_t kfac_glm_draws_outer_workspace_bytes(const kfac_draw_outer_job* jobs, int njobs, int64_t nb,
                                                       int nc, int64_t ns) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ) return 0;
  const int64_t R = draw_rows(nb, nc, ns);
  if (!R) return 0;
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) {
    const kfac_cov_outer_job& q = jobs[i].rows;
    if (q.cols <= 0 || q.nG <= 0) return 0;
    total += outer_u_bytes(q, nb) + 2 * outer_v_bytes(q, R) + draw_outer_partial_bytes(q, R, ns);
  }
  return total;
}

extern "C" int kfac_glm_draws_outer(const kfac_draw_outer_job* jobs, int njobs, int64_t nb, int nc, int64_t ns,
                                    int accumulate, float* F, int64_t ldF, void* workspace,
                                    size_t workspace_bytes, kfac_stream_t stream) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ || !F) return KFAC_EINVAL;
  kfac_cov_outer_job rows[CMAXJ];
  for (int i = 0; i < njobs; ++i) {
    rows[i] = jobs[i].rows;
    if (!outer_job_ok(rows[i]) || !jobs[i].Z || jobs[i].ldZ < outer_nA(rows[i]) * rows[i].nG) return KFAC_EINVAL;
  }
  const int64_t R = draw_rows(nb, nc, ns);
  if (!R || ldF < R) return KFAC_EINVAL;
  const int64_t lim = (int64_t)1 << 31;
  OuterArgs op{};
  DrawOuterArgs args{};
  op.njobs = args.njobs = njobs;
  op.nc = args.nc = nc;
  op.nb = nb;
  args.accumulate = accumulate;
  args.R = (int)R;
  args.nb = (int)nb;
  args.bt = (int)cdiv(nb, TILE);
  args.ns = ns;
  args.ldF = ldF;
  args.F = F;
  int64_t nn = 0, nv = 0, ntasks = 0;
  if (!cov_fill_outer(rows, njobs, nb, R, op, nn, nv)) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i) {
    DrawOuterJobDev& d = args.job[i];
    const OuterJobDev& o = op.job[i];
    d.Z = jobs[i].Z;
    d.ldZ = jobs[i].ldZ;
    d.nA = o.nA; d.nG = o.nG; d.tg = o.tg;
    d.t_begin = o.v_begin;  // the transpose walks V's tiles: kfac_cov_outer_v's task ranges
    args.t_end[i] = op.v_end[i];
    d.begin = (int)ntasks;
    const int64_t per = (int64_t)d.tg * args.bt;
    if (per >= lim || ns >= lim / per) return KFAC_EINVAL;
    ntasks += ns * per;
    if (ntasks >= lim) return KFAC_EINVAL;
    args.end[i] = (int)ntasks;
  }
  const int64_t rblocks = cdiv(R, NTHREADS);
  if (ns >= lim / rblocks) return KFAC_EINVAL;
  if (!workspace || workspace_bytes < kfac_glm_draws_outer_workspace_bytes(jobs, njobs, nb, nc, ns))
    return KFAC_EWORKSPACE;
  char* ws = (char*)workspace;
  for (int i = 0; i < njobs; ++i) {
    OuterJobDev& o = op.job[i];
    DrawOuterJobDev& d = args.job[i];
    o.norm = reinterpret_cast<float*>(ws); ws += outer_u_bytes(rows[i], nb);  // U, nb x nA
    o.V = reinterpret_cast<float*>(ws); ws += outer_v_bytes(rows[i], R);
    d.U = o.norm;
    d.V = o.V;
    d.Vt = reinterpret_cast<float*>(ws); ws += outer_v_bytes(rows[i], R);
    d.partial = reinterpret_cast<float*>(ws); ws += draw_outer_partial_bytes(rows[i], R, ns);
  }
  hipStream_t s = (hipStream_t)stream;
  int rc = cov_launch_outer_u(op, nn, s);
  if (rc != KFAC_OK) return rc;
  rc = cov_launch_outer_v(op, nv, s);
  if (rc != KFAC_OK) return rc;
  hipLaunchKernelGGL(kfac_glm_draws_vt, dim3((unsigned)nv), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_glm_draws_outer_tile, dim3((unsigned)ntasks), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_glm_draws_outer_reduce, dim3((unsigned)(ns * rblocks)), dim3(NTHREADS), 0, s, args,
                     (int)rblocks);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

extern "C" int kfac_softmax_mc(const float* mean, int64_t ldm, const float* F, int64_t ldF, int64_t ns,
                               int64_t nb, int nc, int accumulate, double* psum, double* hsum,
                               kfac_stream_t stream) {
  if (!mean || !F || !psum || !hsum || ns <= 0 || nb <= 0 || nc <= 0) return KFAC_EINVAL;
  const int64_t lim = (int64_t)1 << 31;
  if (ns >= lim || nb >= lim / nc || ldm < nc || ldF < nb * nc) return KFAC_EINVAL;
  const int64_t blocks = cdiv(nb, NTHREADS / 64);
  hipLaunchKernelGGL(kfac_softmax_mc_kernel, dim3((unsigned)blocks), dim3(NTHREADS), 0, (hipStream_t)stream,
                     mean, ldm, F, ldF, ns, nb, nc, accumulate, psum, hsum);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}
