// What covariance.hip (kfac_kron_cov) and covariance_outer.hip (kfac_kron_cov_outer)
// share: the limits of one call, the operand views, and the bodies of the two kernels
// both routes run -- a 64x64 tile of (tall matrix) x K2, and one K segment of a sample's
// nc x nc Gram block -- and what their damping sweeps share: the weight views and the
// weighted Gram of a staged segment for a group of grid points; and what the joint calls
// (covariance_joint.hip) take from both: the argument blocks of the apply / V launches, the
// Abar^T panel, and the 64x64 Gram tile all three of their operands go through; the
// class-tiled per-sample calls (covariance_tiled.hip) run that tile on one sample's rows; the
// class-tiled weighted calls (covariance_wtiled.hip) take the sweep / per-entry calls' job
// checks and projection launches and the tiled calls' row and tile-pair counts, and share their
// weighted panel with the class-tiled INF calls (covariance_inf_tiled.hip); the draw calls (covariance_draws.hip) start from the same apply / U / V launches.
#pragma once

#include "kfac_common.h"

namespace kfac {

constexpr int CMAXJ = 8;
constexpr int CMAXC = 32;           // nc: one 32x32 MFMA quadrant
constexpr int GSEG = 2048;          // K elements per gram workgroup (multiple of BK)

__device__ __forceinline__ int cov_find_job(const int* ends, int njobs, int task) {
  int j = 0;
  while (j + 1 < njobs && task >= ends[j]) ++j;
  return j;
}

__device__ __forceinline__ OpDev rowmajor_op(const float* p, int rows, int cols, int64_t ld) {
  OpDev d{};
  d.ptr = p; d.layout = KFAC_ROWMAJOR; d.rows = rows; d.cols = cols; d.ld = ld; d.ones = -1;
  return d;
}

// element (k, i) = p[i * L + k]
__device__ __forceinline__ OpDev channel_op(const float* p, int64_t rows, int cols, int64_t L) {
  OpDev d{};
  d.ptr = p; d.layout = KFAC_CHANNEL; d.rows = rows; d.cols = cols; d.L = L; d.sB = 0; d.ones = -1;
  return d;
}

// One 64x64 tile (rows i0.., columns g0..) of T = X K2: X is (trows x nG) with row stride
// ldX >= nG (A-operand element (g, i) = X[i*ldX + g]), T is (trows x nG) contiguous.
// K2 lower => the K-range starts at g0.
__device__ __forceinline__ void cov_times_k2_tile(const float* X, int64_t ldX, int trows, int nG,
                                                  const float* K2, int64_t ld2, int lower2, int i0,
                                                  int g0, float* T, float* lds) {
  const OpDev xt = channel_op(X, nG, trows, ldX);
  const OpDev k2 = rowmajor_op(K2, nG, nG, ld2);
  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  // T[i][g'] = sum_g X[i][g] K2[g][g']
  contract_tile<KFAC_CHANNEL, KFAC_ROWMAJOR>(xt, i0, k2, g0, lower2 ? g0 : 0, nG, false, true, lds,
                                             acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = g0 + (wave & 1) * 32 + (lane & 31);
  if (g >= nG) return;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int i = i0 + (wave >> 1) * 32 + acc_row(v, lane);
    if (i < trows) T[(int64_t)i * nG + g] = acc[v];
  }
}

// Gram partial of one sample over the K segment [k0, k1): Tb is that sample's nc rows of
// K elements (contiguous), part its nc x nc block (lower triangle written).  Every wave
// contracts its quarter of each staged panel (contract_tile's narrow mode); the four
// partials are summed in a fixed order.
__device__ __forceinline__ void cov_gram_segment(const float* Tb, int64_t K, int nc, int64_t k0,
                                                 int64_t k1, float* part, float* lds) {
  const OpDev t = channel_op(Tb, K, nc, K);
  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  contract_tile<KFAC_CHANNEL, KFAC_CHANNEL>(t, 0, t, 0, k0, k1, true, true, lds, acc, true);
  // (contract_tile leaves through a barrier: lds is free)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int RP = 33;
  static_assert(4 * 32 * RP <= 4 * PANEL, "wave partials fit the staging buffer");
#pragma unroll
  for (int v = 0; v < 16; ++v) lds[(wave * 32 + acc_row(v, lane)) * RP + (lane & 31)] = acc[v];
  __syncthreads();
  for (int e = threadIdx.x; e < nc * nc; e += NTHREADS) {
    const int c = e / nc, c2 = e - c * nc;
    if (c2 > c) continue;
    const int o = c * RP + c2;
    part[e] = (lds[o] + lds[32 * RP + o]) + (lds[64 * RP + o] + lds[96 * RP + o]);
  }
}

// ---- damping sweeps (kfac_kron_cov_sweep / kfac_kron_cov_outer_sweep): the operands
// projected on the factors' eigenvectors once, then one weighted Gram per grid point tau
constexpr int SMAXT = 64;           // grid points per call
constexpr int WSEG = NTHREADS;      // K elements per weighted-gram workgroup: thread t stages k0 + t
constexpr int WTG = 4;              // grid points per accumulator group (4 x 16 registers)
constexpr int WPITCH = 33;          // staged segment [k][c]: column writes conflict-free
// floats: the staged segment, one group's weight panel, the four wave partials
constexpr int WGRAM_LDS = WSEG * WPITCH + WTG * WSEG + 4 * 32 * WPITCH;
static_assert(WGRAM_LDS * sizeof(float) <= 65536, "static LDS");

struct SweepWeights {
  const float* wA;  // nt x nA, row tau at wA + tau*ldwA
  const float* wG;  // nt x nG (WGRAM_FLAT: nt x nA*nG, the per-entry weights)
  int64_t ldwA, ldwG;
};
struct SweepArgs {
  int ntau;
  SweepWeights job[CMAXJ];
};

// Weighted Gram partials of one sample over the K segment [k0, k0 + WSEG): for every grid
// point tau, part[tau * part_stride] (nc x nc, lower triangle written) =
//   sum_k w_tau[k] Tb[c][k] Tb[c'][k] ,
//   w_tau[k] = wA_tau[k / nG] * wG_tau[k % nG] (WGRAM_RANK1: K = nA*nG),
//              wG_tau[k]                        (WGRAM_VECTOR: K = nG), or
//              W_tau[k], W_tau = wG + tau*ldwG  (WGRAM_FLAT: K = nA*nG, one weight per
//              entry in the rows' own flat order; wA unused: no division, no product).
// The sample's nc row segments are staged ONCE ([k][c], thread t owns k0 + t and its
// (a, g): one division per thread, none in a loop); the grid points then go through in
// groups of WTG on the staged data: a group's weights are staged beside the segment, and
// each tau owns an accumulator that takes the wave's quarter of the segment in k order
// (the B fragment scaled by its k-row's weight: one multiply per MFMA and tau), so slice
// tau does not depend on nt or on its place in the group.  The four wave partials are
// summed in cov_gram_segment's fixed order.  Loads are unconditional (clamped index).
// ldT: the stride between the sample's rows where they are not K apart (0: K).
enum WGramMode { WGRAM_VECTOR = 0, WGRAM_RANK1 = 1, WGRAM_FLAT = 2 };

template <WGramMode MODE>
__device__ __forceinline__ void cov_wgram_segment(const float* Tb, int64_t K, int nc, int64_t k0,
                                                  const SweepWeights& W, int nG, int nt, float* part,
                                                  int64_t part_stride, float* lds, int64_t ldT = 0) {
  float* xs = lds;
  float* wl = xs + WSEG * WPITCH;
  float* red = wl + WTG * WSEG;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, rr = lane & 31;
  const bool live = k0 + tid < K;
  const int64_t kc = live ? k0 + tid : K - 1;
  const float* src = Tb + kc;
  const int64_t rs = ldT ? ldT : K;
#pragma unroll 8
  for (int c = 0; c < 32; ++c) {
    const float x = src[(int64_t)min(c, nc - 1) * rs];
    xs[tid * WPITCH + c] = (live && c < nc) ? x : 0.f;
  }
  int64_t ia = 0, ig = kc;
  if (MODE == WGRAM_RANK1) {
    ia = kc / nG;
    ig = kc - ia * nG;
  }
  const int klen = (int)min((int64_t)WSEG, K - k0);
  const int kb = wave * (WSEG / 4);
  for (int t0 = 0; t0 < nt; t0 += WTG) {
    const int ng = min(WTG, nt - t0);
#pragma unroll
    for (int t = 0; t < WTG; ++t) {
      const int64_t tt = min(t0 + t, nt - 1);
      float w = W.wG[tt * W.ldwG + ig];
      if (MODE == WGRAM_RANK1) w *= W.wA[tt * W.ldwA + ia];
      wl[t * WSEG + tid] = live ? w : 0.f;
    }
    __syncthreads();  // (the first pass: the segment too)
    floatx16 acc[WTG];
#pragma unroll
    for (int t = 0; t < WTG; ++t)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
    for (int k = kb; k < kb + WSEG / 4 && k < klen; k += 2) {
      const float a = xs[(k + h) * WPITCH + rr];
#pragma unroll
      for (int t = 0; t < WTG; ++t)
        if (t < ng)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, a * wl[t * WSEG + k + h], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < WTG; ++t) {
      if (t < ng) {
#pragma unroll
        for (int v = 0; v < 16; ++v) red[(wave * 32 + acc_row(v, lane)) * WPITCH + rr] = acc[t][v];
        __syncthreads();
        float* p = part + (int64_t)(t0 + t) * part_stride;
        for (int e = tid; e < nc * nc; e += NTHREADS) {
          const int c = e / nc, c2 = e - c * nc;
          if (c2 > c) continue;
          const int o = c * WPITCH + c2;
          p[e] = (red[o] + red[32 * WPITCH + o]) + (red[64 * WPITCH + o] + red[96 * WPITCH + o]);
        }
        __syncthreads();
      }
    }
  }
}

// OpDev has one pointer: the second operand of a product formed in a loader rides in sB.
__device__ __forceinline__ int64_t aux_bits(const float* p) { return (int64_t)reinterpret_cast<intptr_t>(p); }
__device__ __forceinline__ const float* aux_ptr(int64_t v) {
  return reinterpret_cast<const float*>((intptr_t)v);
}

// ---- what the joint calls (covariance_joint.hip) share with the per-sample ones: the
// argument blocks of the apply / V launches, the Abar^T panel, the job checks
struct CovJobDev {
  const float* J;
  const float* K1;
  const float* K2;
  float* U;        // rows x nA*nG
  float* T;        // rows x nA*nG, row r = K1^T M_r K2 in a*nG + g order
  float* partial;  // nb x nseg x nc*nc
  int64_t ldJ, ld1, ld2;
  int nA, nG, tg, nseg, lower1, lower2;
  int ucols, trows;                // rows*nG, rows*nA
  int u_begin, t_begin, g_begin;   // first task in the U / T / gram launch
};

struct CovArgs {
  int njobs, nc, accumulate;
  int nu, nt, ng;  // tasks of the U / T / gram launch
  int64_t nb;
  float* cov;
  int u_end[CMAXJ], t_end[CMAXJ], g_end[CMAXJ];
  CovJobDev job[CMAXJ];
};
static_assert(sizeof(CovArgs) <= 4096, "kernel argument block");

struct OuterJobDev {
  const float* a;
  const float* D;
  const float* K1;
  const float* K2;
  float* norm;     // at x nb: sum over column tile t of (abar_b K1)^2
  float* V;        // nb*nc x nG
  float* partial;  // nb x nseg x nc*nc
  int64_t lda, ldD, ld1, ld2;
  int cols, ones, nA, nG;  // ones = cols if has_ones else -1
  int at, bt, tg, nseg, lower1, lower2;
  int vrows;                       // nb*nc
  int n_begin, v_begin, g_begin;   // first task in the rownorm / V / gram launch
};

struct OuterArgs {
  int njobs, nc, accumulate;
  int64_t nb;
  float* cov;
  int n_end[CMAXJ], v_end[CMAXJ], g_end[CMAXJ];
  OuterJobDev job[CMAXJ];
};
static_assert(sizeof(OuterArgs) <= 4096, "kernel argument block");

// kfac_kron_cov_outer_full's R launch (covariance_full.hip)
struct FullOuterArgs {
  int ntau;
  int r_begin[CMAXJ], r_end[CMAXJ];  // tasks of the R launch
  const float* W[CMAXJ];
  int64_t ldW[CMAXJ];
  float* R[CMAXJ];                   // ntau x nb x nG
};

// kfac_cov_apply_u + kfac_cov_apply_t (covariance.hip) on a filled block: U, then T, for
// all rows of every job; kfac_cov_outer_v (covariance_outer.hip): V = Delta K2.
int cov_launch_apply(const CovArgs& args, hipStream_t s);
int cov_launch_outer_v(const OuterArgs& args, int64_t nv, hipStream_t s);
// kfac_cov_rownorm (covariance_outer.hip) on a filled block: norm[tile][b], nn tasks.
int cov_launch_rownorm(const OuterArgs& args, int64_t nn, hipStream_t s);
// kfac_cov_outer_u (covariance_joint.hip) on a filled block: U = Abar K1 (nb x nA) at
// OuterJobDev::norm, nn tasks (the row-norm launch's ranges).
int cov_launch_outer_u(const OuterArgs& args, int64_t nn, hipStream_t s);
// kfac_cov_sweep_reduce (covariance.hip) on a block whose njobs, nc, nb, accumulate, cov and
// the jobs' partial (ntau x nb x nseg x nc*nc) / nseg are filled.
int cov_launch_sweep_reduce(const CovArgs& args, int ntau, hipStream_t s);

// kfac_cov_proj2 (P2T at OuterJobDev::norm, nn tasks: the row-norm launch's ranges) and
// kfac_cov_full_r (R_t = P2T^T W_t, nr tasks) of covariance_full.hip, and kfac_cov_rownorm_w
// (covariance_outer.hip: norm[tau][tile][b], nn tasks) on filled blocks.
int cov_launch_proj2(const OuterArgs& args, int64_t nn, hipStream_t s);
int cov_launch_full_r(const OuterArgs& args, const FullOuterArgs& fa, int64_t nr, hipStream_t s);
int cov_launch_rownorm_w(const OuterArgs& args, const SweepArgs& sw, int64_t nn, hipStream_t s);

constexpr int KFAC_SAMPLEROWS = 17;  // panel layout of Abar^T (internal to the outer routes)

// element (k, b) = k < rows ? p[b * ld + k] : (k == ones ? 1 : 0): Abar^T, samples as
// the operand's columns.  rows = the stored columns of a, cols = nb.
__device__ __forceinline__ OpDev samplerows_op(const float* p, int kcols, int ones, int nb,
                                               int64_t ld) {
  OpDev d{};
  d.ptr = p; d.layout = KFAC_SAMPLEROWS; d.rows = kcols; d.cols = nb; d.ld = ld; d.ones = ones;
  return d;
}

// Panel<CHANNEL>'s thread map (32 lanes walk k, contiguous in a sample's row) with the
// ones entry on the K axis: row k == ones of the panel is 1 for every sample.
template <>
struct Panel<KFAC_SAMPLEROWS> {
  static constexpr int PITCH = LDP;
  const float* base;
  int64_t ld, kend;
  int r, c0, col0, nb, krows, ones;
  __device__ __forceinline__ void init(const OpDev& op, const float* base_, int col0_, int tid,
                                       int64_t k_end, int64_t) {
    base = base_; ld = op.ld; kend = k_end; nb = op.cols; krows = (int)op.rows; ones = op.ones;
    r = tid & 31; c0 = tid >> 5; col0 = col0_;
  }
  __device__ __forceinline__ void load(int64_t k, float (&v)[8]) const {
    const int64_t kk = k + r;
    const bool ok = kk < kend;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int b = col0 + c0 + 8 * m;
      float x = 0.f;
      if (ok && b < nb) x = kk < krows ? base[(int64_t)b * ld + kk] : (kk == ones ? 1.f : 0.f);
      v[m] = x;
    }
  }
  __device__ __forceinline__ void store(float* lds, const float (&v)[8]) const {
#pragma unroll
    for (int m = 0; m < 8; ++m) lds[r * LDP + c0 + 8 * m] = v[m];
  }
};

static inline size_t cov_t_bytes(const kfac_cov_job& j, int64_t rows) {
  return align_up((size_t)rows * (size_t)j.nA * (size_t)j.nG * sizeof(float), 256);
}
static inline bool cov_job_ok(const kfac_cov_job& q) {
  return q.J && q.K1 && q.K2 && q.nA > 0 && q.nG > 0 && q.ld1 >= q.nA && q.ld2 >= q.nG &&
         q.ldJ >= (int64_t)q.nA * q.nG;
}
static inline int64_t outer_nA(const kfac_cov_outer_job& j) { return (int64_t)j.cols + (j.has_ones != 0); }
static inline size_t outer_v_bytes(const kfac_cov_outer_job& j, int64_t rows) {
  return align_up((size_t)rows * (size_t)j.nG * sizeof(float), 256);
}
// U = Abar K1 (nb x nA): kfac_cov_outer_u's output
static inline size_t outer_u_bytes(const kfac_cov_outer_job& j, int64_t nb) {
  return align_up((size_t)nb * (size_t)outer_nA(j) * sizeof(float), 256);
}
static inline size_t outer_norm_bytes(const kfac_cov_outer_job& j, int64_t nb) {
  return align_up((size_t)(cdiv(outer_nA(j), TILE) * nb) * sizeof(float), 256);
}
static inline bool outer_job_ok(const kfac_cov_outer_job& q) {
  return q.a && q.D && q.K1 && q.K2 && q.cols > 0 && q.nG > 0 && q.lda >= q.cols &&
         q.ldD >= q.nG && q.ld1 >= outer_nA(q) && q.ld2 >= q.nG;
}

// the job checks of the weighted calls (capped and class-tiled)
static inline bool sweep_job_ok(const kfac_cov_sweep_job& q) {
  return q.J && q.VA && q.VG && q.wA && q.wG && q.nA > 0 && q.nG > 0 && q.ldA >= q.nA &&
         q.ldG >= q.nG && q.ldwA >= q.nA && q.ldwG >= q.nG && q.ldJ >= (int64_t)q.nA * q.nG;
}
static inline int64_t osweep_nA(const kfac_cov_outer_sweep_job& j) { return (int64_t)j.cols + (j.has_ones != 0); }
static inline bool osweep_job_ok(const kfac_cov_outer_sweep_job& q) {
  return q.a && q.D && q.VA && q.VG && q.wA && q.wG && q.cols > 0 && q.nG > 0 && q.lda >= q.cols &&
         q.ldD >= q.nG && q.ldA >= osweep_nA(q) && q.ldG >= q.nG && q.ldwA >= osweep_nA(q) &&
         q.ldwG >= q.nG;
}
static inline bool full_job_ok(const kfac_cov_full_job& q) {
  return q.J && q.VA && q.VG && q.W && q.nA > 0 && q.nG > 0 && q.ldA >= q.nA && q.ldG >= q.nG &&
         q.ldW >= (int64_t)q.nA * q.nG && q.ldJ >= (int64_t)q.nA * q.nG;
}
static inline int64_t ofull_nA(const kfac_cov_outer_full_job& j) { return (int64_t)j.cols + (j.has_ones != 0); }
static inline bool ofull_job_ok(const kfac_cov_outer_full_job& q) {
  return q.a && q.D && q.VA && q.VG && q.W && q.cols > 0 && q.nG > 0 && q.lda >= q.cols &&
         q.ldD >= q.nG && q.ldA >= ofull_nA(q) && q.ldG >= q.nG && q.ldW >= ofull_nA(q) * q.nG;
}

// The apply part of a CovArgs block (jobs' operands, the U / T task ranges, nu, nt) for
// `rows` rows per job; U, T and the Gram fields are the caller's.  The stacked operands
// are indexed with 32-bit columns: false where rows*nG, rows*nA or a task count reach 2^31.
static inline bool cov_fill_apply(const kfac_cov_job* jobs, int njobs, int64_t rows, CovArgs& args) {
  const int64_t lim = (int64_t)1 << 31;
  int64_t nu = 0, nt = 0;
  for (int i = 0; i < njobs; ++i) {
    const kfac_cov_job& q = jobs[i];
    if (rows * q.nG >= lim - TILE || rows * q.nA >= lim - TILE) return false;
    CovJobDev& d = args.job[i];
    d.J = q.J; d.K1 = q.K1; d.K2 = q.K2;
    d.ldJ = q.ldJ; d.ld1 = q.ld1; d.ld2 = q.ld2;
    d.nA = q.nA; d.nG = q.nG;
    d.tg = (int)cdiv(q.nG, TILE);
    d.lower1 = q.lower1 != 0;
    d.lower2 = q.lower2 != 0;
    d.ucols = (int)(rows * q.nG);
    d.trows = (int)(rows * q.nA);
    d.u_begin = (int)nu; d.t_begin = (int)nt;
    nu += cdiv(q.nA, TILE) * cdiv(d.ucols, TILE);
    nt += cdiv(d.trows, TILE) * d.tg;
    if (nu >= lim || nt >= lim) return false;
    args.u_end[i] = (int)nu; args.t_end[i] = (int)nt;
  }
  args.nu = (int)nu; args.nt = (int)nt;
  return true;
}

// The projection part of an OuterArgs block (jobs' operands, the Abar K1 and Delta K2 task
// ranges; nn, nv their task counts) for nb samples and `rows` = nb*nc delta rows; norm, V
// and the Gram fields are the caller's.  false where nA or a task count reach 2^31.
static inline bool cov_fill_outer(const kfac_cov_outer_job* jobs, int njobs, int64_t nb, int64_t rows,
                                  OuterArgs& args, int64_t& nn, int64_t& nv) {
  const int64_t lim = (int64_t)1 << 31;
  nn = nv = 0;
  for (int i = 0; i < njobs; ++i) {
    const kfac_cov_outer_job& q = jobs[i];
    if (outer_nA(q) >= lim - TILE) return false;
    OuterJobDev& d = args.job[i];
    d.a = q.a; d.D = q.D; d.K1 = q.K1; d.K2 = q.K2;
    d.lda = q.lda; d.ldD = q.ldD; d.ld1 = q.ld1; d.ld2 = q.ld2;
    d.cols = q.cols;
    d.ones = q.has_ones ? q.cols : -1;
    d.nA = (int)outer_nA(q);
    d.nG = q.nG;
    d.at = (int)cdiv(d.nA, TILE);
    d.bt = (int)cdiv(nb, TILE);
    d.tg = (int)cdiv(q.nG, TILE);
    d.lower1 = q.lower1 != 0;
    d.lower2 = q.lower2 != 0;
    d.vrows = (int)rows;
    d.n_begin = (int)nn; d.v_begin = (int)nv;
    nn += (int64_t)d.at * d.bt;
    nv += cdiv(rows, TILE) * d.tg;
    if (nn >= lim || nv >= lim) return false;
    args.n_end[i] = (int)nn; args.v_end[i] = (int)nv;
  }
  return true;
}

// ---- joint covariance (kfac_kron_cov_joint / kfac_kron_cov_outer_joint) and the class-tiled
// per-sample covariance (kfac_kron_cov_tiled / kfac_kron_cov_outer_tiled)
constexpr int JSEG = GSEG;          // K elements per joint-gram task: a function of K alone
constexpr int JTILE2 = TILE * TILE; // floats per tile partial

// tile pairs ti >= tj of an nc x nc block
static inline int64_t tiled_npairs(int nc) {
  const int64_t t = cdiv(nc, TILE);
  return t * (t + 1) / 2;
}
// rows = nb*nc with 32-bit rows (the sibling calls' limit), or 0
static inline int64_t tiled_rows(int64_t nb, int nc) {
  const int64_t lim = (int64_t)1 << 31;
  if (nb <= 0 || nc <= 0 || nb >= (lim - TILE) / nc) return 0;
  return nb * nc;
}

// One 64x64 tile (ti >= tj) of X X^T over the K segment [k0, k1): X is rows x K with K
// contiguous per row, part the fp32 64x64 partial (row-major, row = the tile-ti row).  The
// four waves hold one 32x32 quadrant each (contract_tile's normal mode), so element
// (r, r') is one k-ordered fma chain over the segment from 0: it depends on rows r and r'
// and on [k0, k1) only, not on the tile it sits in.  A diagonal tile stages one panel
// (`same`) and skips its upper quadrant, which is never read.
__device__ __forceinline__ void cov_joint_gram_tile(const float* X, int64_t K, int rows, int ti, int tj,
                                                    int64_t k0, int64_t k1, float* part, float* lds) {
  const OpDev x = channel_op(X, K, rows, K);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool same = ti == tj;
  const bool active = !(same && wave == 1);  // quadrant (0, 1) of a diagonal tile
  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  contract_tile<KFAC_CHANNEL, KFAC_CHANNEL>(x, ti * TILE, x, tj * TILE, k0, k1, same, active, lds, acc);
  if (!active) return;
  float* dst = part + (wave >> 1) * 32 * TILE + (wave & 1) * 32 + (lane & 31);
#pragma unroll
  for (int v = 0; v < 16; ++v) dst[acc_row(v, lane) * TILE] = acc[v];
}

// ---- the weighted tile operand of the class-tiled weighted calls (covariance_wtiled.hip) and
// of the class-tiled INF calls' first term (covariance_inf_tiled.hip)
constexpr int KFAC_WCHANNEL = 23;  // (k, j) = w[k] * X[j*ld + k]

// X (rows x K, K contiguous per row, rows ld >= K apart) with row k of the panel scaled by w[k]
__device__ __forceinline__ OpDev wchannel_op(const float* X, int64_t K, int64_t ld, int rows, const float* wA,
                                             const float* wG, int nG, int mode) {
  OpDev d{};
  d.ptr = X; d.layout = KFAC_WCHANNEL; d.rows = K; d.cols = rows; d.L = ld; d.ones = -1;
  d.sB = aux_bits(wG); d.ld = aux_bits(wA); d.C = nG; d.H = mode;
  return d;
}

// Panel<CHANNEL>'s thread map (32 lanes walk k, contiguous in a row of X); a thread's k row
// has ONE weight per stage, read (rank one: formed) once and applied to its 8 elements.
// Loads are issued for k_first, k_first + BK, ... in order, so (a, g) of the thread's row is
// advanced, not divided.
template <>
struct Panel<KFAC_WCHANNEL> {
  static constexpr int PITCH = LDP;
  const float* base;
  const float* wA;
  const float* wG;
  int64_t L, kend, kk, ia;  // kk: row k + r of the next load, (ia, ig) its (a, g)
  int r, c0, col0, cols, nG, ig;
  bool rank1;
  __device__ __forceinline__ void init(const OpDev& op, const float* base_, int col0_, int tid,
                                       int64_t k_end, int64_t k_first) {
    base = base_; wG = aux_ptr(op.sB); wA = aux_ptr(op.ld); L = op.L; kend = k_end; cols = op.cols;
    nG = op.C; rank1 = op.H == WGRAM_RANK1;
    r = tid & 31; c0 = tid >> 5; col0 = col0_;
    kk = k_first + r;
    ia = 0; ig = 0;
    if (rank1) {
      ia = kk / nG;
      ig = (int)(kk - ia * nG);
    }
  }
  __device__ __forceinline__ void load(int64_t, float (&v)[8]) {
    const bool ok = kk < kend;
    float w = 0.f;
    if (ok) w = rank1 ? wA[ia] * wG[ig] : wG[kk];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int col = col0 + c0 + 8 * m;
      float x = 0.f;
      if (ok && col < cols) x = w * base[(int64_t)col * L + kk];
      v[m] = x;
    }
    kk += BK;
    if (rank1) {
      ig += BK;
      while (ig >= nG) { ig -= nG; ++ia; }
    }
  }
  __device__ __forceinline__ void store(float* lds, const float (&v)[8]) const {
#pragma unroll
    for (int m = 0; m < 8; ++m) lds[r * LDP + c0 + 8 * m] = v[m];
  }
};

}  // namespace kfac
