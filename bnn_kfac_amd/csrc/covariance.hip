// GLM predictive: the full output covariance J Sigma J^T under the KFAC posterior.
//
// KFAC.sample draws S = L_A z L_G^T (nA x nG), so vec(S) (index a*nG + g) has
// covariance K1 K1^T (x) K2 K2^T with K1 = L_A, K2 = L_G.  With M_r the Jacobian row
// r = b*nc + c (sample b, output c) viewed (nA x nG) row-major,
//   cov[b][c][c'] = sum_layers < T_{b,c}, T_{b,c'} >_F ,   T_r = K1^T M_r K2 ,
// never forming the Kronecker product.  Per call (<= 8 layers, nb samples, nc <= 32):
//   apply : T_r for every row, as two GEMMs over ALL rows at once (fp32 MFMA, exact
//           fp32 products, 64x64 tiles of contract_tile; lower-triangular K1 / K2 skip
//           their zero K-range):
//             U = K1^T [M_0 | M_1 | ...]   (nA x rows*nG: column j = (row j / nG, g = j % nG))
//             T = [U_0 ; U_1 ; ...] K2     (rows*nA x nG: the U_r stacked are one tall matrix)
//           so a layer with a narrow nG (10 classes) fills its tiles with other rows'
//           columns instead of padding.
//   gram  : cov_b = T_b T_b^T, K split over workgroups (each a GSEG-long segment of the
//           nc rows, staged through LDS, narrow 32x32 MFMA), fp32 partials
//   reduce: partials summed per sample in a fixed order (segments, then jobs) in fp64;
//           the lower triangle is computed and mirrored, so cov[b] is bitwise symmetric.
// Apply tasks are ordered a-tile major, heaviest first (a lower-triangular K1 leaves tile
// a0 the K-range [a0, nA)), and run in plain block order: the round-robin dispatch gives
// every XCD the same mix.  Contiguous per-XCD ranges (xcd_task) put the long a-tiles on
// XCD 0 and the short ones on XCD 7 and measured 1.5x slower; K1 fits any one L2.
//
// kfac_kron_cov_sweep (end of this file): the same covariance for up to 64 dampings at
// once in the factors' eigenbasis.  apply runs once with K1 = V_A, K2 = V_G (dense); a
// damping is a pair of weight vectors, and kfac_cov_sweep_gram / kfac_cov_sweep_reduce
// form one weighted Gram per grid point from the staged rows (cov_wgram_segment).
#include "covariance_common.h"

namespace kfac {

constexpr int KFAC_ROWBATCH = 16;   // panel layout of [M_0 | M_1 | ...] (internal to this file)

// element (k, j) = p[(j / L) * sB + k * L + j % L]: row j / L of J viewed (nA x nG), L = nG
__device__ __forceinline__ OpDev rowbatch_op(const float* p, int rows, int cols, int64_t L, int64_t sB) {
  OpDev d{};
  d.ptr = p; d.layout = KFAC_ROWBATCH; d.rows = rows; d.cols = cols; d.ld = L; d.L = L; d.sB = sB;
  d.ones = -1;
  return d;
}

// Panel<ROWMAJOR>'s thread map (16 lanes x 4 columns walk a panel row) over the columns
// of [M_0 | M_1 | ...]: within one M_r they are contiguous, so the lanes still read whole
// segments.  With nG, the row stride and the base multiples of 4 floats a thread's 4
// columns lie in one M_r, 16 bytes aligned: one 16-byte load.
template <>
struct Panel<KFAC_ROWBATCH> {
  static constexpr int PITCH = TILE + 4;
  const float* base;
  int64_t ld, kend;
  int64_t off[4];  // offset of column c4 + q at k = 0, or -1 past the last column
  int c4, r0;
  bool vec;
  __device__ __forceinline__ void init(const OpDev& op, const float* base_, int col0, int tid,
                                       int64_t k_end, int64_t) {
    base = base_; ld = op.ld; kend = k_end;
    c4 = (tid & 15) * 4; r0 = tid >> 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = col0 + c4 + q;
      const int r = j / (int)op.L;
      off[q] = j < op.cols ? r * op.sB + (j - r * (int)op.L) : -1;
    }
    vec = off[3] >= 0 && ((op.L & 3) == 0) && ((op.sB & 3) == 0) &&
          ((reinterpret_cast<uintptr_t>(base) & 15) == 0);
  }
  __device__ __forceinline__ void load(int64_t k, float (&v)[8]) const {
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int64_t row = k + r0 + 16 * m;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < kend) {
        const float* p = base + row * ld;
        if (vec) {
          x = *reinterpret_cast<const float4*>(p + off[0]);
        } else {
          float e[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) e[q] = off[q] >= 0 ? p[off[q]] : 0.f;
          x = make_float4(e[0], e[1], e[2], e[3]);
        }
      }
      v[4 * m + 0] = x.x; v[4 * m + 1] = x.y; v[4 * m + 2] = x.z; v[4 * m + 3] = x.w;
    }
  }
  __device__ __forceinline__ void store(float* lds, const float (&v)[8]) const {
#pragma unroll
    for (int m = 0; m < 2; ++m)
      *reinterpret_cast<float4*>(lds + (r0 + 16 * m) * PITCH + c4) =
          make_float4(v[4 * m], v[4 * m + 1], v[4 * m + 2], v[4 * m + 3]);
  }
};

// Apply, launch 1: one 64x64 tile of U = K1^T [M_0 | M_1 | ...]; column j = (r, g) goes
// to U[r][a][g] (the U_r back to back: one (rows*nA x nG) matrix for launch 2).
__global__ __launch_bounds__(NTHREADS) void kfac_cov_apply_u(CovArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const CovJobDev& C = args.job[cov_find_job(args.u_end, args.njobs, task)];
  const int local = task - C.u_begin;
  const int ct = (C.ucols + TILE - 1) / TILE;
  const int a0 = (local / ct) * TILE, j0 = (local % ct) * TILE;
  const OpDev k1 = rowmajor_op(C.K1, C.nA, C.nA, C.ld1);
  const OpDev m = rowbatch_op(C.J, C.nA, C.ucols, C.nG, C.ldJ);
  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  // U[a][j] = sum_k K1[k][a] M[k][j]; K1 lower => k >= a0
  contract_tile<KFAC_ROWMAJOR, KFAC_ROWBATCH>(k1, a0, m, j0, C.lower1 ? a0 : 0, C.nA, false, true,
                                              lds, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = j0 + (wave & 1) * 32 + (lane & 31);
  if (j >= C.ucols) return;
  const int r = j / C.nG, g = j - r * C.nG;
  float* dst = C.U + (int64_t)r * C.nA * C.nG + g;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int a = a0 + (wave >> 1) * 32 + acc_row(v, lane);
    if (a < C.nA) dst[(int64_t)a * C.nG] = acc[v];
  }
}

// Launch 2: one 64x64 tile of T = U K2, U the (rows*nA x nG) stack.
__global__ __launch_bounds__(NTHREADS) void kfac_cov_apply_t(CovArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const CovJobDev& C = args.job[cov_find_job(args.t_end, args.njobs, task)];
  const int local = task - C.t_begin;
  cov_times_k2_tile(C.U, C.nG, C.trows, C.nG, C.K2, C.ld2, C.lower2, (local / C.tg) * TILE,
                    (local % C.tg) * TILE, C.T, lds);
}

// Gram partial: rows c of sample b over one K segment, lower triangle of the nc x nc
// block.
__global__ __launch_bounds__(NTHREADS) void kfac_cov_gram(CovArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const CovJobDev& C = args.job[cov_find_job(args.g_end, args.njobs, task)];
  const int64_t local = task - C.g_begin;
  const int64_t b = local / C.nseg;
  const int seg = (int)(local % C.nseg);
  const int nc = args.nc;
  const int64_t K = (int64_t)C.nA * C.nG;
  const int64_t k0 = (int64_t)seg * GSEG;
  cov_gram_segment(C.T + b * nc * K, K, nc, k0, min(K, k0 + GSEG), C.partial + local * nc * nc, lds);
}

// cov[b] (+)= sum over jobs (in job order) of the segment partials (in segment order),
// fp64; lower triangle mirrored.
__global__ __launch_bounds__(NTHREADS) void kfac_cov_reduce(CovArgs args) {
  const int64_t b = blockIdx.x;
  const int nc = args.nc, n2 = nc * nc;
  float* cov = args.cov + b * n2;
  for (int e = threadIdx.x; e < n2; e += NTHREADS) {
    const int c = e / nc, c2 = e - c * nc;
    if (c2 > c) continue;
    double total = 0.0;
    for (int j = 0; j < args.njobs; ++j) {
      const CovJobDev& C = args.job[j];
      const float* part = C.partial + b * C.nseg * n2 + e;
      double s = 0.0;
      for (int i = 0; i < C.nseg; ++i) s += (double)part[(int64_t)i * n2];
      total += s;
    }
    const float v = args.accumulate ? (float)((double)cov[e] + total) : (float)total;
    cov[e] = v;
    cov[c2 * nc + c] = v;
  }
}

// Damping sweep (kfac_kron_cov_sweep): apply_u / apply_t above run once with K1 = V_A,
// K2 = V_G (dense), so T_r = V_A^T M_r V_G; these two launches then weight it per tau.
// Weighted Gram partials: rows c of sample b over one WSEG-long K segment, every tau;
// partial is ntau x nb x nseg x nc*nc.
__global__ __launch_bounds__(NTHREADS) void kfac_cov_sweep_gram(CovArgs args, SweepArgs sw) {
  __shared__ __attribute__((aligned(16))) float lds[WGRAM_LDS];
  const int task = blockIdx.x;
  const int j = cov_find_job(args.g_end, args.njobs, task);
  const CovJobDev& C = args.job[j];
  const int64_t local = task - C.g_begin;
  const int64_t b = local / C.nseg;
  const int seg = (int)(local % C.nseg);
  const int nc = args.nc;
  const int64_t K = (int64_t)C.nA * C.nG;
  cov_wgram_segment<WGRAM_RANK1>(C.T + b * nc * K, K, nc, (int64_t)seg * WSEG, sw.job[j], C.nG, sw.ntau,
                          C.partial + local * nc * nc, args.nb * C.nseg * nc * nc, lds);
}

// cov[tau][b] (+)= kfac_cov_reduce's sum over tau's partials; grid (nb, ntau).
__global__ __launch_bounds__(NTHREADS) void kfac_cov_sweep_reduce(CovArgs args) {
  const int64_t b = blockIdx.x, tau = blockIdx.y;
  const int nc = args.nc, n2 = nc * nc;
  float* cov = args.cov + (tau * args.nb + b) * n2;
  for (int e = threadIdx.x; e < n2; e += NTHREADS) {
    const int c = e / nc, c2 = e - c * nc;
    if (c2 > c) continue;
    double total = 0.0;
    for (int j = 0; j < args.njobs; ++j) {
      const CovJobDev& C = args.job[j];
      const float* part = C.partial + (tau * args.nb + b) * C.nseg * n2 + e;
      double s = 0.0;
      for (int i = 0; i < C.nseg; ++i) s += (double)part[(int64_t)i * n2];
      total += s;
    }
    const float v = args.accumulate ? (float)((double)cov[e] + total) : (float)total;
    cov[e] = v;
    cov[c2 * nc + c] = v;
  }
}

// The two apply launches alone (kfac_kron_cov_joint forms its own Gram from T).
int cov_launch_apply(const CovArgs& args, hipStream_t s) {
  hipLaunchKernelGGL(kfac_cov_apply_u, dim3((unsigned)args.nu), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_cov_apply_t, dim3((unsigned)args.nt), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

// The sweep reduce alone (covariance_full.hip forms its own weighted Gram partials).
int cov_launch_sweep_reduce(const CovArgs& args, int ntau, hipStream_t s) {
  hipLaunchKernelGGL(kfac_cov_sweep_reduce, dim3((unsigned)args.nb, (unsigned)ntau), dim3(NTHREADS), 0, s,
                     args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

static int64_t cov_nseg(const kfac_cov_job& j) { return cdiv((int64_t)j.nA * j.nG, GSEG); }
static size_t cov_partial_bytes(const kfac_cov_job& j, int64_t nb, int nc) {
  return align_up((size_t)(nb * cov_nseg(j)) * nc * nc * sizeof(float), 256);
}
}  // namespace kfac

using namespace kfac;

extern "C" size_t kfac_kron_cov_workspace_bytes(const kfac_cov_job* jobs, int njobs, int64_t nb,
                                                int nc) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ || nb <= 0 || nc <= 0 || nc > CMAXC) return 0;
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) {
    if (jobs[i].nA <= 0 || jobs[i].nG <= 0) return 0;
    total += 2 * cov_t_bytes(jobs[i], nb * nc) + cov_partial_bytes(jobs[i], nb, nc);
  }
  return total;
}

extern "C" int kfac_kron_cov(const kfac_cov_job* jobs, int njobs, int64_t nb, int nc, int accumulate,
                             float* cov, void* workspace, size_t workspace_bytes,
                             kfac_stream_t stream) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ || nb <= 0 || nc <= 0 || nc > CMAXC || !cov)
    return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!cov_job_ok(jobs[i])) return KFAC_EINVAL;
  const int64_t lim = (int64_t)1 << 31;
  if (nb >= lim / nc) return KFAC_EINVAL;
  const int64_t rows = nb * nc;
  CovArgs args{};
  args.njobs = njobs;
  args.nc = nc;
  args.accumulate = accumulate;
  args.nb = nb;
  args.cov = cov;
  if (!cov_fill_apply(jobs, njobs, rows, args)) return KFAC_EINVAL;
  const int64_t nu = args.nu, nt = args.nt;
  int64_t ng = 0;
  for (int i = 0; i < njobs; ++i) {
    CovJobDev& d = args.job[i];
    d.nseg = (int)cov_nseg(jobs[i]);
    d.g_begin = (int)ng;
    ng += nb * d.nseg;
    if (ng >= lim) return KFAC_EINVAL;
    args.g_end[i] = (int)ng;
  }
  if (!workspace || workspace_bytes < kfac_kron_cov_workspace_bytes(jobs, njobs, nb, nc))
    return KFAC_EWORKSPACE;
  char* ws = (char*)workspace;
  for (int i = 0; i < njobs; ++i) {
    CovJobDev& d = args.job[i];
    const size_t tb = cov_t_bytes(jobs[i], rows);
    d.U = reinterpret_cast<float*>(ws); ws += tb;
    d.T = reinterpret_cast<float*>(ws); ws += tb;
    d.partial = reinterpret_cast<float*>(ws); ws += cov_partial_bytes(jobs[i], nb, nc);
  }
  args.nu = (int)nu; args.nt = (int)nt; args.ng = (int)ng;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(kfac_cov_apply_u, dim3((unsigned)nu), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_cov_apply_t, dim3((unsigned)nt), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_cov_gram, dim3((unsigned)ng), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_cov_reduce, dim3((unsigned)nb), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

// ------------------------------------------------------------------ damping sweep
static int64_t sweep_nseg(const kfac_cov_sweep_job& j) { return cdiv((int64_t)j.nA * j.nG, WSEG); }
static size_t sweep_t_bytes(const kfac_cov_sweep_job& j, int64_t rows) {
  return align_up((size_t)rows * (size_t)j.nA * (size_t)j.nG * sizeof(float), 256);
}
static size_t sweep_partial_bytes(const kfac_cov_sweep_job& j, int64_t nb, int nc, int nt) {
  return align_up((size_t)(nb * sweep_nseg(j)) * nc * nc * nt * sizeof(float), 256);
}

extern "C" size_t kfac_kron_cov_sweep_workspace_bytes(const kfac_cov_sweep_job* jobs, int njobs,
                                                      int64_t nb, int nc, int nt) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ || nb <= 0 || nc <= 0 || nc > CMAXC || nt <= 0 ||
      nt > SMAXT)
    return 0;
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) {
    if (jobs[i].nA <= 0 || jobs[i].nG <= 0) return 0;
    total += 2 * sweep_t_bytes(jobs[i], nb * nc) + sweep_partial_bytes(jobs[i], nb, nc, nt);
  }
  return total;
}

extern "C" int kfac_kron_cov_sweep(const kfac_cov_sweep_job* jobs, int njobs, int64_t nb, int nc,
                                   int nt, int accumulate, float* cov, void* workspace,
                                   size_t workspace_bytes, kfac_stream_t stream) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ || nb <= 0 || nc <= 0 || nc > CMAXC || nt <= 0 ||
      nt > SMAXT || !cov)
    return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!sweep_job_ok(jobs[i])) return KFAC_EINVAL;
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
  int64_t nu = 0, ntl = 0, ng = 0;
  for (int i = 0; i < njobs; ++i) {
    const kfac_cov_sweep_job& q = jobs[i];
    // (kfac_kron_cov's limits: 32-bit columns of the stacked operands, 32-bit task counts)
    if (rows * q.nG >= lim - TILE || rows * q.nA >= lim - TILE) return KFAC_EINVAL;
    CovJobDev& d = args.job[i];
    d.J = q.J; d.K1 = q.VA; d.K2 = q.VG;
    d.ldJ = q.ldJ; d.ld1 = q.ldA; d.ld2 = q.ldG;
    d.nA = q.nA; d.nG = q.nG;
    d.tg = (int)cdiv(q.nG, TILE);
    d.nseg = (int)sweep_nseg(q);
    d.lower1 = d.lower2 = 0;
    d.ucols = (int)(rows * q.nG);
    d.trows = (int)(rows * q.nA);
    d.u_begin = (int)nu; d.t_begin = (int)ntl; d.g_begin = (int)ng;
    nu += cdiv(q.nA, TILE) * cdiv(d.ucols, TILE);
    ntl += cdiv(d.trows, TILE) * d.tg;
    ng += nb * d.nseg;
    if (nu >= lim || ntl >= lim || ng >= lim) return KFAC_EINVAL;
    args.u_end[i] = (int)nu; args.t_end[i] = (int)ntl; args.g_end[i] = (int)ng;
    sw.job[i].wA = q.wA; sw.job[i].wG = q.wG;
    sw.job[i].ldwA = q.ldwA; sw.job[i].ldwG = q.ldwG;
  }
  if (!workspace || workspace_bytes < kfac_kron_cov_sweep_workspace_bytes(jobs, njobs, nb, nc, nt))
    return KFAC_EWORKSPACE;
  char* ws = (char*)workspace;
  for (int i = 0; i < njobs; ++i) {
    CovJobDev& d = args.job[i];
    const size_t tb = sweep_t_bytes(jobs[i], rows);
    d.U = reinterpret_cast<float*>(ws); ws += tb;
    d.T = reinterpret_cast<float*>(ws); ws += tb;
    d.partial = reinterpret_cast<float*>(ws); ws += sweep_partial_bytes(jobs[i], nb, nc, nt);
  }
  args.nu = (int)nu; args.nt = (int)ntl; args.ng = (int)ng;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(kfac_cov_apply_u, dim3((unsigned)nu), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_cov_apply_t, dim3((unsigned)ntl), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_cov_sweep_gram, dim3((unsigned)ng), dim3(NTHREADS), 0, s, args, sw);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_cov_sweep_reduce, dim3((unsigned)nb, (unsigned)nt), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}
