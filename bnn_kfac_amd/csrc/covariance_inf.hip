// GLM predictive under the INF posterior (kfac_inf_cov, kfac_inf_cov_outer): INF keeps a
// rank-r eigen part U Lambda U^T, U = kron(UA, UG), and a diagonal correction, so by Woodbury
//   P^-1 = diag(w) - diag(w) U F^T F U^T diag(w)            (kfac_hip.h: w, F)
//   cov[b][c][c'] = sum_{i,g} W[i][g] M_{b,c}[i][g] M_{b,c'}[i][g] - < y_{b,c}, y_{b,c'} > ,
//   y_{b,c} = F t_{b,c} ,  t_{b,c}[p*rg + q] = sum_{i,g} UA[i][p] W[i][g] M_{b,c}[i][g] UG[g][q] .
// Every GEMM is a task list of 64x64 contract_tile tiles; an output element is ONE k-ordered
// chain from 0, so it depends on its own row and column only, not on nb or the tile.
//
// Dense rows (kfac_inf_cov):
//   x     : kfac_inf_x, X_row = UA^T (M_row o W): rows p, K = nA, columns (row, g); the
//           weight is applied in the panel loader (Panel<KFAC_INF_WJ>)
//   t     : kfac_inf_t, T = X UG: rows (row, p), K = nG, columns q
//   y     : kfac_inf_y, Y = T F^T: rows (b, c), K = r
//   gram  : kfac_inf_gram1_dense, cov_wgram_segment's flat mode on the RAW rows (stride ldJ);
//           kfac_inf_gram2, cov_gram_segment on y_b over ISEG-long segments of r
//   reduce: kfac_inf_reduce, fp64, first - second, jobs in order.
//
// Factored Linear (kfac_inf_cov_outer): M_{b,c} = abar_b delta_{b,c}^T, no row is formed:
//   h     : kfac_inf_h, one GEMM whose rows are (b, p), p <= ra, K = nA, columns g:
//           HR[b][p][g] = sum_i (abar_b[i] UA[i][p]) W[i][g] for p < ra (H_b) and
//           HR[b][ra][g] = sum_i abar_b[i]^2 W[i][g] (rho_b); the left operand is formed in
//           the panel loader (Panel<KFAC_INF_AU>), which carries the ones column
//   t     : kfac_inf_t, rows (b, c, p), K = nG, columns q; the left operand
//           H_b[p][g] delta_{b,c}[g] is formed in the loader (Panel<KFAC_INF_HD>)
//   y     : kfac_inf_y
//   gram  : kfac_inf_gram1_outer, cov_wgram_segment's K = nG mode on Delta_b (stride ldD)
//           with rho_b; kfac_inf_gram2
//   reduce: kfac_inf_reduce.
// No atomics, plain vector stores; the diagonal is a difference of two non-negative sums and
// is not clamped (kfac_hip.h).
#include "covariance_inf.h"

namespace kfac {

constexpr int KFAC_INF_AU = 20;  // (k = i, m = (b, p)) = abar_b[i] * (p < ra ? UA[i][p] : abar_b[i])
constexpr int KFAC_INF_HD = 21;  // (k = g, m = (b, c, p)) = HR[b][p][g] * D[b*nc + c][g]
constexpr int KFAC_INF_WJ = 22;  // (k = i, j = (row, g)) = W[i][g] * J[row][i*nG + g]
constexpr int ISEG = WSEG;       // elements of r per kfac_inf_gram2 workgroup (multiple of BK)

// a (nb x kcols, stride lda), UA (nA x ra, stride ldA); columns m < ncols = nb*(ra + 1)
__device__ __forceinline__ OpDev inf_au_op(const float* a, int kcols, int ones, int64_t lda, const float* UA,
                                           int64_t ldA, int ra, int ncols) {
  OpDev d{};
  d.ptr = a; d.layout = KFAC_INF_AU; d.rows = kcols; d.cols = ncols; d.ld = lda; d.ones = ones;
  d.L = ldA; d.sB = aux_bits(UA); d.C = ra;
  return d;
}

// HR (nb x (ra+1) x nG), D (nb*nc x nG, stride ldD); columns m < ncols = nb*nc*ra
__device__ __forceinline__ OpDev inf_hd_op(const float* HR, int nG, const float* D, int64_t ldD, int ra,
                                           int nc, int ncols) {
  OpDev d{};
  d.ptr = HR; d.layout = KFAC_INF_HD; d.rows = nG; d.cols = ncols; d.ld = ldD; d.ones = -1;
  d.L = nG; d.sB = aux_bits(D); d.C = ra; d.H = nc;
  return d;
}

// J (rows x nA*nG, stride ldJ), W (nA*nG); columns j < ncols = rows*nG
__device__ __forceinline__ OpDev inf_wj_op(const float* J, int nA, int nG, int64_t ldJ, const float* W,
                                           int ncols) {
  OpDev d{};
  d.ptr = J; d.layout = KFAC_INF_WJ; d.rows = nA; d.cols = ncols; d.ld = ldJ; d.ones = -1;
  d.L = nG; d.sB = aux_bits(W);
  return d;
}

// Panel<SAMPLEROWS>'s thread map (32 lanes walk k = i, contiguous in a sample's row); a
// column's sample and p are decoded once.
template <>
struct Panel<KFAC_INF_AU> {
  static constexpr int PITCH = LDP;
  const float* a;
  const float* UA;
  int64_t ldA, kend;
  int64_t aoff[8];
  int pp[8];  // p of the column, -1 past the last column
  int r, c0, krows, ones, ra;
  __device__ __forceinline__ void init(const OpDev& op, const float* base_, int col0, int tid,
                                       int64_t k_end, int64_t) {
    a = base_; UA = aux_ptr(op.sB); ldA = op.L; kend = k_end; krows = (int)op.rows; ones = op.ones;
    ra = op.C; r = tid & 31; c0 = tid >> 5;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int col = col0 + c0 + 8 * m;
      const int b = col / (ra + 1);
      pp[m] = col < op.cols ? col - b * (ra + 1) : -1;
      aoff[m] = (int64_t)b * op.ld;
    }
  }
  __device__ __forceinline__ void load(int64_t k, float (&v)[8]) const {
    const int64_t kk = k + r;
    const bool ok = kk < kend;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      float x = 0.f;
      if (ok && pp[m] >= 0) {
        const float ab = kk < krows ? a[aoff[m] + kk] : (kk == ones ? 1.f : 0.f);
        x = ab * (pp[m] < ra ? UA[kk * ldA + pp[m]] : ab);
      }
      v[m] = x;
    }
  }
  __device__ __forceinline__ void store(float* lds, const float (&v)[8]) const {
#pragma unroll
    for (int m = 0; m < 8; ++m) lds[r * LDP + c0 + 8 * m] = v[m];
  }
};

// The same thread map over k = g: both factors are contiguous in g.
template <>
struct Panel<KFAC_INF_HD> {
  static constexpr int PITCH = LDP;
  const float* H;
  const float* D;
  int64_t kend;
  int64_t hoff[8], doff[8];  // hoff -1 past the last column
  int r, c0;
  __device__ __forceinline__ void init(const OpDev& op, const float* base_, int col0, int tid,
                                       int64_t k_end, int64_t) {
    H = base_; D = aux_ptr(op.sB); kend = k_end; r = tid & 31; c0 = tid >> 5;
    const int ra = op.C, nc = op.H;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int col = col0 + c0 + 8 * m;
      const int row = col / ra, p = col - row * ra;
      const int64_t b = row / nc;
      hoff[m] = col < op.cols ? (b * (ra + 1) + p) * op.L : -1;
      doff[m] = (int64_t)row * op.ld;
    }
  }
  __device__ __forceinline__ void load(int64_t k, float (&v)[8]) const {
    const int64_t kk = k + r;
    const bool ok = kk < kend;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      float x = 0.f;
      if (ok && hoff[m] >= 0) x = H[hoff[m] + kk] * D[doff[m] + kk];
      v[m] = x;
    }
  }
  __device__ __forceinline__ void store(float* lds, const float (&v)[8]) const {
#pragma unroll
    for (int m = 0; m < 8; ++m) lds[r * LDP + c0 + 8 * m] = v[m];
  }
};

// Panel<ROWMAJOR>'s thread map (16 lanes x 4 columns walk a panel row) over the columns
// (row, g) of [M_0 | M_1 | ...]: within one row they are contiguous in J and in W.
template <>
struct Panel<KFAC_INF_WJ> {
  static constexpr int PITCH = TILE + 4;
  const float* J;
  const float* W;
  int64_t nG, kend;
  int64_t joff[4];  // offset of column c4 + q at i = 0, -1 past the last column
  int gq[4];
  int c4, r0;
  __device__ __forceinline__ void init(const OpDev& op, const float* base_, int col0, int tid,
                                       int64_t k_end, int64_t) {
    J = base_; W = aux_ptr(op.sB); nG = op.L; kend = k_end;
    c4 = (tid & 15) * 4; r0 = tid >> 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = col0 + c4 + q;
      const int row = j / (int)op.L;
      gq[q] = j - row * (int)op.L;
      joff[q] = j < op.cols ? (int64_t)row * op.ld + gq[q] : -1;
    }
  }
  __device__ __forceinline__ void load(int64_t k, float (&v)[8]) const {
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int64_t i = k + r0 + 16 * m;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float x = 0.f;
        if (i < kend && joff[q] >= 0) x = J[joff[q] + i * nG] * W[i * nG + gq[q]];
        v[4 * m + q] = x;
      }
    }
  }
  __device__ __forceinline__ void store(float* lds, const float (&v)[8]) const {
#pragma unroll
    for (int m = 0; m < 2; ++m)
      *reinterpret_cast<float4*>(lds + (r0 + 16 * m) * PITCH + c4) =
          make_float4(v[4 * m], v[4 * m + 1], v[4 * m + 2], v[4 * m + 3]);
  }
};

__device__ __forceinline__ void zero(floatx16& acc) {
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
}

// One 64 (m = (b, p)) x 64 (g) tile of HR = [abar o UA | abar o abar]^T W.
__global__ __launch_bounds__(NTHREADS) void kfac_inf_h(InfArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const InfJobDev& C = args.job[cov_find_job(args.h_end, args.njobs, task)];
  const int local = task - C.h_begin;
  const int m0 = (local / C.hn) * TILE, g0 = (local % C.hn) * TILE;
  const OpDev au = inf_au_op(C.a, C.cols, C.ones, C.lda, C.UA, C.ldA, C.ra, C.hcols);
  const OpDev w = rowmajor_op(C.W, C.nA, C.nG, C.nG);
  floatx16 acc;
  zero(acc);
  contract_tile<KFAC_INF_AU, KFAC_ROWMAJOR>(au, m0, w, g0, 0, C.nA, false, true, lds, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = g0 + (wave & 1) * 32 + (lane & 31);
  if (g >= C.nG) return;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int m = m0 + (wave >> 1) * 32 + acc_row(v, lane);
    if (m < C.hcols) C.HX[(int64_t)m * C.nG + g] = acc[v];
  }
}

// One 64 (p) x 64 (j = (row, g)) tile of X_row = UA^T (M_row o W): X[row][p][g].
__global__ __launch_bounds__(NTHREADS) void kfac_inf_x(InfArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const InfJobDev& C = args.job[cov_find_job(args.h_end, args.njobs, task)];
  const int local = task - C.h_begin;
  const int p0 = (local / C.hn) * TILE, j0 = (local % C.hn) * TILE;
  const OpDev ua = rowmajor_op(C.UA, C.nA, C.ra, C.ldA);
  const OpDev wj = inf_wj_op(C.J, C.nA, C.nG, C.ldJ, C.W, C.hcols);
  floatx16 acc;
  zero(acc);
  contract_tile<KFAC_ROWMAJOR, KFAC_INF_WJ>(ua, p0, wj, j0, 0, C.nA, false, true, lds, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = j0 + (wave & 1) * 32 + (lane & 31);
  if (j >= C.hcols) return;
  const int row = j / C.nG, g = j - row * C.nG;
  float* dst = C.HX + (int64_t)row * C.ra * C.nG + g;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int p = p0 + (wave >> 1) * 32 + acc_row(v, lane);
    if (p < C.ra) dst[(int64_t)p * C.nG] = acc[v];
  }
}

// One 64 (m = (row, p)) x 64 (q) tile of T = (left operand) UG: T[m][q], row m of T is
// t_row's entries p*rg + q.  OUTER: the left operand is H_b[p][g] delta_row[g], else X.
template <bool OUTER>
__global__ __launch_bounds__(NTHREADS) void kfac_inf_t(InfArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const InfJobDev& C = args.job[cov_find_job(args.t_end, args.njobs, task)];
  const int local = task - C.t_begin;
  const int m0 = (local / C.tn) * TILE, q0 = (local % C.tn) * TILE;
  const OpDev ug = rowmajor_op(C.UG, C.nG, C.rg, C.ldG);
  floatx16 acc;
  zero(acc);
  if (OUTER) {
    const OpDev hd = inf_hd_op(C.HX, C.nG, C.D, C.ldD, C.ra, args.nc, C.trows);
    contract_tile<KFAC_INF_HD, KFAC_ROWMAJOR>(hd, m0, ug, q0, 0, C.nG, false, true, lds, acc);
  } else {
    const OpDev x = channel_op(C.HX, C.nG, C.trows, C.nG);
    contract_tile<KFAC_CHANNEL, KFAC_ROWMAJOR>(x, m0, ug, q0, 0, C.nG, false, true, lds, acc);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = q0 + (wave & 1) * 32 + (lane & 31);
  if (q >= C.rg) return;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int m = m0 + (wave >> 1) * 32 + acc_row(v, lane);
    if (m < C.trows) C.T[(int64_t)m * C.rg + q] = acc[v];
  }
}

// One 64 (row) x 64 (j) tile of Y = T F^T: Y[row][j] = sum_k T[row][k] F[j][k].
__global__ __launch_bounds__(NTHREADS) void kfac_inf_y(InfArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const InfJobDev& C = args.job[cov_find_job(args.y_end, args.njobs, task)];
  const int local = task - C.y_begin;
  const int i0 = (local / C.yn) * TILE, j0 = (local % C.yn) * TILE;
  const OpDev t = channel_op(C.T, C.r, args.rows, C.r);
  const OpDev f = channel_op(C.F, C.r, C.r, C.ldF);
  floatx16 acc;
  zero(acc);
  contract_tile<KFAC_CHANNEL, KFAC_CHANNEL>(t, i0, f, j0, 0, C.r, false, true, lds, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = j0 + (wave & 1) * 32 + (lane & 31);
  if (j >= C.r) return;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int i = i0 + (wave >> 1) * 32 + acc_row(v, lane);
    if (i < args.rows) C.Y[(int64_t)i * C.r + j] = acc[v];
  }
}

// First term, factored: Delta_b diag(rho_b) Delta_b^T over one WSEG-long segment of nG.
__global__ __launch_bounds__(NTHREADS) void kfac_inf_gram1_outer(InfArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[WGRAM_LDS];
  const int task = blockIdx.x;
  const InfJobDev& C = args.job[cov_find_job(args.g1_end, args.njobs, task)];
  const int64_t local = task - C.g1_begin;
  const int64_t b = local / C.nseg1;
  const int seg = (int)(local % C.nseg1);
  const int nc = args.nc;
  const SweepWeights w{nullptr, C.HX + (b * (C.ra + 1) + C.ra) * C.nG, 0, 0};
  cov_wgram_segment<WGRAM_VECTOR>(C.D + b * nc * C.ldD, C.nG, nc, (int64_t)seg * WSEG, w, C.nG, 1,
                                  C.part1 + local * nc * nc, 0, lds, C.ldD);
}

// First term, dense rows: sum_k W[k] J_{b,c}[k] J_{b,c'}[k] over one WSEG-long segment.
__global__ __launch_bounds__(NTHREADS) void kfac_inf_gram1_dense(InfArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[WGRAM_LDS];
  const int task = blockIdx.x;
  const InfJobDev& C = args.job[cov_find_job(args.g1_end, args.njobs, task)];
  const int64_t local = task - C.g1_begin;
  const int64_t b = local / C.nseg1;
  const int seg = (int)(local % C.nseg1);
  const int nc = args.nc;
  const SweepWeights w{nullptr, C.W, 0, 0};
  cov_wgram_segment<WGRAM_FLAT>(C.J + b * nc * C.ldJ, (int64_t)C.nA * C.nG, nc, (int64_t)seg * WSEG, w,
                                C.nG, 1, C.part1 + local * nc * nc, 0, lds, C.ldJ);
}

// Second term: the Gram of y_b over one ISEG-long segment of r.
__global__ __launch_bounds__(NTHREADS) void kfac_inf_gram2(InfArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const InfJobDev& C = args.job[cov_find_job(args.g2_end, args.njobs, task)];
  const int64_t local = task - C.g2_begin;
  const int64_t b = local / C.nseg2;
  const int64_t k0 = (local % C.nseg2) * ISEG;
  const int nc = args.nc;
  cov_gram_segment(C.Y + b * nc * C.r, C.r, nc, k0, min(k0 + (int64_t)ISEG, (int64_t)C.r),
                   C.part2 + local * nc * nc, lds);
}

// cov[b] (+)= sum_j (sum_seg part1 - sum_seg part2), fp64, fixed order; the lower triangle is
// computed and mirrored.  Not clamped.
__global__ __launch_bounds__(NTHREADS) void kfac_inf_reduce(InfArgs args) {
  const int64_t b = blockIdx.x;
  const int nc = args.nc, n2 = nc * nc;
  float* cov = args.cov + b * n2;
  for (int e = threadIdx.x; e < n2; e += NTHREADS) {
    const int c = e / nc, c2 = e - c * nc;
    if (c2 > c) continue;
    double total = 0.0;
    for (int j = 0; j < args.njobs; ++j) {
      const InfJobDev& C = args.job[j];
      const float* p1 = C.part1 + b * C.nseg1 * n2 + e;
      const float* p2 = C.part2 + b * C.nseg2 * n2 + e;
      double s1 = 0.0, s2 = 0.0;
      for (int i = 0; i < C.nseg1; ++i) s1 += (double)p1[(int64_t)i * n2];
      for (int i = 0; i < C.nseg2; ++i) s2 += (double)p2[(int64_t)i * n2];
      total += s1 - s2;
    }
    const float v = args.accumulate ? (float)((double)cov[e] + total) : (float)total;
    cov[e] = v;
    cov[c2 * nc + c] = v;
  }
}

static bool inf_call_ok(const void* jobs, int njobs, int64_t nb, int nc) {
  return jobs && njobs > 0 && njobs <= CMAXJ && nb > 0 && nc > 0 && nc <= CMAXC;
}

static size_t inf_part_bytes(int64_t K, int64_t seg, int64_t nb, int nc) {
  return align_up((size_t)(nb * cdiv(K, seg)) * nc * nc * sizeof(float), 256);
}
static size_t inf_job_bytes(const InfDims& d, int64_t nb, int nc) {
  return inf_hx_bytes(d) + 2 * inf_ty_bytes(d, nb * nc) + inf_part_bytes(d.k1, WSEG, nb, nc) +
         inf_part_bytes(d.ra * d.rg, ISEG, nb, nc);
}

// Job i's device block: the projection part (inf_fill_proj), then the task ranges of the two
// Gram launches (n[3], n[4]) and their partials.  false where a 32-bit column, row or task
// count would overflow.
static bool inf_fill(InfArgs& args, int i, const InfDims& d, int64_t hcols, int64_t hm, int64_t hn, char*& ws,
                     int64_t (&n)[5]) {
  const int64_t lim = ((int64_t)1 << 31) - TILE;
  const int64_t nb = args.nb, r = d.ra * d.rg;
  const int nc = args.nc;
  if (d.k1 >= lim * WSEG) return false;
  if (!inf_fill_proj(args, i, d, hcols, hm, hn, ws, n)) return false;
  InfJobDev& C = args.job[i];
  C.nseg1 = (int)cdiv(d.k1, WSEG);
  C.nseg2 = (int)cdiv(r, ISEG);
  C.g1_begin = (int)n[3]; C.g2_begin = (int)n[4];
  n[3] += nb * C.nseg1;
  n[4] += nb * C.nseg2;
  if (n[3] >= lim || n[4] >= lim) return false;
  args.g1_end[i] = (int)n[3]; args.g2_end[i] = (int)n[4];
  if (ws) {
    C.part1 = reinterpret_cast<float*>(ws); ws += inf_part_bytes(d.k1, WSEG, nb, nc);
    C.part2 = reinterpret_cast<float*>(ws); ws += inf_part_bytes(r, ISEG, nb, nc);
  }
  return true;
}

int inf_launch_proj(const InfArgs& args, bool outer, const int64_t* n, hipStream_t s) {
  if (outer)
    hipLaunchKernelGGL(kfac_inf_h, dim3((unsigned)n[0]), dim3(NTHREADS), 0, s, args);
  else
    hipLaunchKernelGGL(kfac_inf_x, dim3((unsigned)n[0]), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  if (outer)
    hipLaunchKernelGGL(kfac_inf_t<true>, dim3((unsigned)n[1]), dim3(NTHREADS), 0, s, args);
  else
    hipLaunchKernelGGL(kfac_inf_t<false>, dim3((unsigned)n[1]), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_inf_y, dim3((unsigned)n[2]), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

// The second term's Gram partials and the reduce: the same for both routes.
static int inf_launch_tail(const InfArgs& args, const int64_t (&n)[5], hipStream_t s) {
  hipLaunchKernelGGL(kfac_inf_gram2, dim3((unsigned)n[4]), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_inf_reduce, dim3((unsigned)args.nb), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}
}  // namespace kfac

using namespace kfac;

extern "C" size_t kfac_inf_cov_workspace_bytes(const kfac_inf_cov_job* jobs, int njobs, int64_t nb, int nc) {
  if (!inf_call_ok(jobs, njobs, nb, nc)) return 0;
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) {
    const kfac_inf_cov_job& q = jobs[i];
    if (q.nA <= 0 || q.nG <= 0 || q.ra <= 0 || q.rg <= 0) return 0;
    total += inf_job_bytes(inf_dims(q, nb, nc), nb, nc);
  }
  return total;
}

extern "C" int kfac_inf_cov(const kfac_inf_cov_job* jobs, int njobs, int64_t nb, int nc, int accumulate,
                            float* cov, void* workspace, size_t workspace_bytes, kfac_stream_t stream) {
  if (!inf_call_ok(jobs, njobs, nb, nc) || !cov) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!inf_job_ok(jobs[i])) return KFAC_EINVAL;
  const int64_t lim = (int64_t)1 << 31;
  if (nb >= (lim - TILE) / nc) return KFAC_EINVAL;
  const bool have = workspace && workspace_bytes >= kfac_inf_cov_workspace_bytes(jobs, njobs, nb, nc);
  InfArgs args{};
  args.njobs = njobs;
  args.nc = nc;
  args.accumulate = accumulate;
  args.rows = (int)(nb * nc);
  args.nb = nb;
  args.cov = cov;
  char* ws = have ? (char*)workspace : nullptr;
  int64_t n[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < njobs; ++i) {
    const kfac_inf_cov_job& q = jobs[i];
    inf_set_operands(args.job[i], q);
    int64_t hcols, hm, hn;
    inf_h_shape(q, nb, nc, hcols, hm, hn);
    if (!inf_fill(args, i, inf_dims(q, nb, nc), hcols, hm, hn, ws, n)) return KFAC_EINVAL;
  }
  if (!have) return KFAC_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int rc = inf_launch_proj(args, false, n, s);
  if (rc != KFAC_OK) return rc;
  hipLaunchKernelGGL(kfac_inf_gram1_dense, dim3((unsigned)n[3]), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  return inf_launch_tail(args, n, s);
}

extern "C" size_t kfac_inf_cov_outer_workspace_bytes(const kfac_inf_cov_outer_job* jobs, int njobs, int64_t nb,
                                                     int nc) {
  if (!inf_call_ok(jobs, njobs, nb, nc)) return 0;
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) {
    const kfac_inf_cov_outer_job& q = jobs[i];
    if (q.cols <= 0 || q.nG <= 0 || q.ra <= 0 || q.rg <= 0) return 0;
    total += inf_job_bytes(inf_dims(q, nb, nc), nb, nc);
  }
  return total;
}

extern "C" int kfac_inf_cov_outer(const kfac_inf_cov_outer_job* jobs, int njobs, int64_t nb, int nc,
                                  int accumulate, float* cov, void* workspace, size_t workspace_bytes,
                                  kfac_stream_t stream) {
  if (!inf_call_ok(jobs, njobs, nb, nc) || !cov) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!inf_outer_job_ok(jobs[i])) return KFAC_EINVAL;
  const int64_t lim = (int64_t)1 << 31;
  if (nb >= (lim - TILE) / nc) return KFAC_EINVAL;
  const bool have = workspace && workspace_bytes >= kfac_inf_cov_outer_workspace_bytes(jobs, njobs, nb, nc);
  InfArgs args{};
  args.njobs = njobs;
  args.nc = nc;
  args.accumulate = accumulate;
  args.rows = (int)(nb * nc);
  args.nb = nb;
  args.cov = cov;
  char* ws = have ? (char*)workspace : nullptr;
  int64_t n[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < njobs; ++i) {
    const kfac_inf_cov_outer_job& q = jobs[i];
    inf_set_operands(args.job[i], q);
    int64_t hcols, hm, hn;
    inf_h_shape(q, nb, nc, hcols, hm, hn);
    if (!inf_fill(args, i, inf_dims(q, nb, nc), hcols, hm, hn, ws, n)) return KFAC_EINVAL;
  }
  if (!have) return KFAC_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int rc = inf_launch_proj(args, true, n, s);
  if (rc != KFAC_OK) return rc;
  hipLaunchKernelGGL(kfac_inf_gram1_outer, dim3((unsigned)n[3]), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  return inf_launch_tail(args, n, s);
}
